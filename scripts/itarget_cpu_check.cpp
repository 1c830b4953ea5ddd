// Host run of the instance-target kernels of biapy_amd/csrc/itarget.hip: the same steps (csrc/itarget_core.h: the id a value counts for, a run's
// contribution with its largest distance, the block's table with its overflow route and its flush, the init and finish rows, the rcmax pass from
// the ends of a run, the channel values; csrc/regionprops_core.h and scripts/label_walk_host.h: the run walk) in the launch sequence of
// bpx_itarget_ids / bpx_itarget_stats / bpx_itarget_pack - sequentially and with the blocks and their waves spread over std::threads on
// std::atomic - checked against a per-voxel statement written with plain loops.  The distances are arbitrary non-negative floats (+inf among
// them): the records do not care where they come from.  Every buffer has exactly its size, so a step outside is the sanitizer's.
// Cases: batches of 1 and 3 with ids reused across samples, 2-D and 3-D, rows of 63 .. 257 voxels, every voxel its own id (512 and 3000 ids: more
// than a block's table), values that are no id, all background, n_max = 0; spans of OVL_SPAN, 256 and 512; every channel, both contour modes,
// connectivity 1..3, both D forms.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -I biapy_amd/csrc -I scripts scripts/itarget_cpu_check.cpp -o itarget_cpu_check
//   ./itarget_cpu_check
// Prints one line per case and exits nonzero on the first mismatch.  Host only: never loaded into Python.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "itarget_core.h"
#include "label_walk_host.h"

template <class T> static void atomic_min(std::atomic<T>& a, T v) {
  T cur = a.load(std::memory_order_relaxed);
  while (v < cur && !a.compare_exchange_weak(cur, v, std::memory_order_relaxed)) {}
}
template <class T> static void atomic_max(std::atomic<T>& a, T v) {
  T cur = a.load(std::memory_order_relaxed);
  while (v > cur && !a.compare_exchange_weak(cur, v, std::memory_order_relaxed)) {}
}

struct HostMem {     // the global records, or a block's table when keys != nullptr (one maximum per slot there, as in ItLds)
  std::atomic<uint32_t>* area_p;
  std::atomic<uint64_t>* sums_p;
  std::atomic<int32_t>* box_p;
  std::atomic<uint32_t>* max_p[2];
  std::atomic<int32_t>* keys = nullptr;
  std::atomic<uint32_t>* claimed = nullptr;
  void area(uint32_t r, uint32_t c) const { area_p[r].fetch_add(c, std::memory_order_relaxed); }
  void sum(uint32_t r, int k, uint64_t v) const { sums_p[(size_t)r * 3 + k].fetch_add(v, std::memory_order_relaxed); }
  void lo(uint32_t r, int k, int32_t v) const { atomic_min(box_p[(size_t)r * 6 + k], v); }
  void hi(uint32_t r, int k, int32_t v) const { atomic_max(box_p[(size_t)r * 6 + 3 + k], v); }
  void umax(uint32_t r, int k, uint32_t v) const { atomic_max(max_p[keys ? 0 : k][r], v); }
  int32_t kload(uint32_t s) const { return keys[s].load(std::memory_order_relaxed); }
  int32_t kcas(uint32_t s, int32_t label) const {
    int32_t expected = 0;
    keys[s].compare_exchange_strong(expected, label, std::memory_order_relaxed);
    return expected;
  }
  uint32_t nclaimed() const { return claimed->load(std::memory_order_relaxed); }
  void claim() const { claimed->fetch_add(1, std::memory_order_relaxed); }
  uint32_t area_of(uint32_t s) const { return area_p[s].load(); }
  uint64_t sum_of(uint32_t s, int k) const { return sums_p[(size_t)s * 3 + k].load(); }
  int32_t lo_of(uint32_t s, int k) const { return box_p[(size_t)s * 6 + k].load(); }
  int32_t hi_of(uint32_t s, int k) const { return box_p[(size_t)s * 6 + 3 + k].load(); }
  uint32_t umax_of(uint32_t s, int) const { return max_p[0][s].load(); }
};

static void parallel_for(int threads, int64_t count, const std::function<void(int64_t)>& f) {   // item q runs on thread q % threads
  if (threads <= 1) { for (int64_t q = 0; q < count; ++q) f(q); return; }
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([=, &f] { for (int64_t q = t; q < count; q += threads) f(q); });
  for (auto& th : pool) th.join();
}

struct Geom { int Z, Y, X, n_max; };
struct Case {
  std::string name;
  int B;
  Geom g;
  int ndim;
  std::vector<float> t;       // B * Z * Y * X values
  std::vector<float> d;       // their "distances"
};

struct Records {              // finished, as the pack pass reads them
  std::vector<uint64_t> cen;
  std::vector<int32_t> box;
  std::vector<uint32_t> area, dmax, rcmax;
};

// the launch sequence of bpx_itarget_stats on the ids of one batch; `span` = OVL_SPAN on the device
static Records stats_host(const std::vector<int32_t>& ids, const Case& c, const double s3[3], int64_t span, int threads) {
  const int64_t n = (int64_t)c.g.Z * c.g.Y * c.g.X, rows = (int64_t)c.B * (c.g.n_max + 1);
  Records out;
  out.area.assign((size_t)rows, 7); out.cen.assign((size_t)rows * 3, 7); out.box.assign((size_t)rows * 6, 7);
  out.dmax.assign((size_t)rows, 7); out.rcmax.assign((size_t)rows, 7);
  for (int64_t r = 0; r < rows; ++r) it_init_row(&out.area[(size_t)r], &out.cen[(size_t)r * 3], &out.box[(size_t)r * 6], &out.dmax[(size_t)r], &out.rcmax[(size_t)r]);
  std::unique_ptr<std::atomic<uint32_t>[]> area(new std::atomic<uint32_t>[(size_t)rows]), dmax(new std::atomic<uint32_t>[(size_t)rows]),
      rcmax(new std::atomic<uint32_t>[(size_t)rows]);
  std::unique_ptr<std::atomic<uint64_t>[]> sums(new std::atomic<uint64_t>[(size_t)rows * 3]);
  std::unique_ptr<std::atomic<int32_t>[]> box(new std::atomic<int32_t>[(size_t)rows * 6]);
  for (int64_t r = 0; r < rows; ++r) {
    area[(size_t)r].store(out.area[(size_t)r]); dmax[(size_t)r].store(out.dmax[(size_t)r]); rcmax[(size_t)r].store(out.rcmax[(size_t)r]);
    for (int k = 0; k < 3; ++k) sums[(size_t)r * 3 + k].store(out.cen[(size_t)r * 3 + k]);
    for (int k = 0; k < 6; ++k) box[(size_t)r * 6 + k].store(out.box[(size_t)r * 6 + k]);
  }
  const HostMem m{area.get(), sums.get(), box.get(), {dmax.get(), rcmax.get()}};
  const int64_t spans = (n + span - 1) / span, blocks = (spans + OVL_WAVES - 1) / OVL_WAVES;
  for (int pass = 0; pass < 2; ++pass) {                       // 0: accumulate, then the finish; 1: the rcmax pass
    parallel_for(threads, blocks * c.B, [&](int64_t q) {       // a block (x, b): its own table, OVL_WAVES spans of sample b, the flush
      const int64_t blk = q % blocks, b = q / blocks;
      const uint32_t base = (uint32_t)(b * (c.g.n_max + 1));
      const std::vector<int32_t> labels(ids.begin() + b * n, ids.begin() + (b + 1) * n);       // the sample alone: a step outside it is caught
      const std::vector<float> dist(c.d.begin() + b * n, c.d.begin() + (b + 1) * n);
      std::unique_ptr<std::atomic<int32_t>[]> lkeys(new std::atomic<int32_t>[RP_LOCAL_SLOTS]), lbox(new std::atomic<int32_t>[RP_LOCAL_SLOTS * 6]);
      std::unique_ptr<std::atomic<uint32_t>[]> larea(new std::atomic<uint32_t>[RP_LOCAL_SLOTS]), lmax(new std::atomic<uint32_t>[RP_LOCAL_SLOTS]);
      std::unique_ptr<std::atomic<uint64_t>[]> lsums(new std::atomic<uint64_t>[RP_LOCAL_SLOTS * 3]);
      std::atomic<uint32_t> lclaimed{0};
      for (int s = 0; s < RP_LOCAL_SLOTS; ++s) {
        lkeys[(size_t)s].store(0); larea[(size_t)s].store(0); lmax[(size_t)s].store(0);
        for (int k = 0; k < 3; ++k) { lsums[(size_t)s * 3 + k].store(0); lbox[(size_t)s * 6 + k].store(RP_LO_INIT); lbox[(size_t)s * 6 + 3 + k].store(RP_HI_INIT); }
      }
      const HostMem loc{larea.get(), lsums.get(), lbox.get(), {lmax.get(), nullptr}, lkeys.get(), &lclaimed};
      parallel_for(threads > 1 ? 2 : 1, OVL_WAVES, [&](int64_t w) {
        const int64_t begin = (blk * OVL_WAVES + w) * span;
        if (begin >= n) return;
        lw_walk_runs_host(labels, c.g, begin, std::min(n, begin + span), [&](int32_t label, int32_t z, int32_t y, int32_t x0, uint32_t L) {
          if (pass == 0) {
            std::vector<uint32_t> bits(L);                      // exactly the run: it_run_max reads no further
            std::memcpy(bits.data(), &dist.at((size_t)(((int64_t)z * c.g.Y + y) * c.g.X + x0)), (size_t)L * 4);
            it_emit(loc, m, base, label, z, y, x0, L, it_run_max(bits.data(), L));
          } else {
            const size_t r = (size_t)(base + (uint32_t)label) * 3;
            const double cen[3] = {it_double(sums[r].load()), it_double(sums[r + 1].load()), it_double(sums[r + 2].load())};
            it_emit_rc(loc, m, base, label, it_run_rc_max(cen, z, y, x0, L, s3));
          }
        });
      });
      for (int s = 0; s < RP_LOCAL_SLOTS; ++s) {
        if (pass == 0) it_merge(loc, (uint32_t)s, m, base);
        else it_merge_rc(loc, (uint32_t)s, m, base);
      }
    });
    if (pass == 0)
      for (int64_t r = 0; r < rows; ++r) {                     // the finish
        uint32_t a = area[(size_t)r].load();
        uint64_t sm[3];
        int32_t bx[6];
        for (int k = 0; k < 3; ++k) sm[k] = sums[(size_t)r * 3 + k].load();
        for (int k = 0; k < 6; ++k) bx[k] = box[(size_t)r * 6 + k].load();
        it_finish_row(&a, sm, bx);
        for (int k = 0; k < 3; ++k) sums[(size_t)r * 3 + k].store(sm[k]);
        for (int k = 0; k < 6; ++k) box[(size_t)r * 6 + k].store(bx[k]);
      }
  }
  for (int64_t r = 0; r < rows; ++r) {
    out.area[(size_t)r] = area[(size_t)r].load(); out.dmax[(size_t)r] = dmax[(size_t)r].load(); out.rcmax[(size_t)r] = rcmax[(size_t)r].load();
    for (int k = 0; k < 3; ++k) out.cen[(size_t)r * 3 + k] = sums[(size_t)r * 3 + k].load();
    for (int k = 0; k < 6; ++k) out.box[(size_t)r * 6 + k] = box[(size_t)r * 6 + k].load();
  }
  return out;
}

// the statement: plain loops over the voxels of every sample
static std::vector<float> brute(const Case& c, const ItPack& p, int64_t& faults) {
  const int Z = c.g.Z, Y = c.g.Y, X = c.g.X, N = c.g.n_max;
  const int64_t n = (int64_t)Z * Y * X;
  std::vector<float> out((size_t)(c.B * p.channels * n), -7.f);
  faults = 0;
  for (int b = 0; b < c.B; ++b) {
    std::vector<int32_t> id((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      const float v = c.t[(size_t)(b * n + i)];
      const bool ok = std::isfinite(v) && v >= 0 && v <= N && std::floor(v) == v;
      faults += !ok;
      id[(size_t)i] = ok ? (int32_t)v : 0;
    }
    std::vector<double> A((size_t)N + 1, 0), S((size_t)(N + 1) * 3, 0);
    std::vector<int> lo((size_t)(N + 1) * 3, 1 << 30), hi((size_t)(N + 1) * 3, -1);
    std::vector<float> dm((size_t)N + 1, 0.f), rm((size_t)N + 1, 0.f);
    auto at = [&](int z, int y, int x) { return (size_t)(((int64_t)z * Y + y) * X + x); };
    for (int z = 0; z < Z; ++z) for (int y = 0; y < Y; ++y) for (int x = 0; x < X; ++x) {
      const int l = id[at(z, y, x)];
      if (!l) continue;
      const int q[3] = {z, y, x};
      A[(size_t)l] += 1;
      dm[(size_t)l] = std::max(dm[(size_t)l], c.d[(size_t)(b * n) + at(z, y, x)]);
      for (int k = 0; k < 3; ++k) { S[(size_t)l * 3 + k] += q[k]; lo[(size_t)l * 3 + k] = std::min(lo[(size_t)l * 3 + k], q[k]); hi[(size_t)l * 3 + k] = std::max(hi[(size_t)l * 3 + k], q[k]); }
    }
    auto rc_of = [&](int l, int z, int y, int x) {
      const double dz = (z - S[(size_t)l * 3] / A[(size_t)l]) * p.s[0], dy = (y - S[(size_t)l * 3 + 1] / A[(size_t)l]) * p.s[1], dx = (x - S[(size_t)l * 3 + 2] / A[(size_t)l]) * p.s[2];
      return (float)std::sqrt((dz * dz + dy * dy) + dx * dx);
    };
    for (int z = 0; z < Z; ++z) for (int y = 0; y < Y; ++y) for (int x = 0; x < X; ++x)
      if (const int l = id[at(z, y, x)]) rm[(size_t)l] = std::max(rm[(size_t)l], rc_of(l, z, y, x));
    for (int z = 0; z < Z; ++z) for (int y = 0; y < Y; ++y) for (int x = 0; x < X; ++x) {
      const int l = id[at(z, y, x)];
      bool edge = false;
      for (int dz = -1; dz <= 1; ++dz) for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
        const int k = std::abs(dz) + std::abs(dy) + std::abs(dx);
        if (k == 0 || k > p.conn || (p.ndim == 2 && dz) || z + dz < 0 || z + dz >= Z || y + dy < 0 || y + dy >= Y || x + dx < 0 || x + dx >= X) continue;
        edge |= id[at(z + dz, y + dy, x + dx)] != l;
      }
      const bool contour = edge && (p.mode == IT_MODE_THICK || l > 0);
      const int q[3] = {z, y, x};
      for (int ch = 0; ch < p.channels; ++ch) {
        const int code = it_code(p.codes, ch);
        float v = 0.f;
        if (code == IT_C) v = contour;
        else if (l > 0) {
          const float d = c.d[(size_t)(b * n) + at(z, y, x)];
          if (code == IT_F) v = !((p.flags & IT_FLAG_F_EXCLUDES_C) && contour);
          else if (code == IT_D) v = (p.flags & IT_FLAG_D_RAW) ? ((p.flags & IT_FLAG_D_CLIP) ? std::min(d, p.clip) : d) : std::isinf(d) ? 1.f : d / dm[(size_t)l];
          else if (code == IT_DC) v = rm[(size_t)l] == 0.f ? 1.f : 1.f - rc_of(l, z, y, x) / rm[(size_t)l];
          else {
            const int a = code == IT_Z ? 0 : code == IT_V ? 1 : 2;
            const double cen = S[(size_t)l * 3 + a] / A[(size_t)l], o = q[a] - cen, e = o >= 0 ? hi[(size_t)l * 3 + a] - cen : cen - lo[(size_t)l * 3 + a];
            v = e == 0 ? 0.f : (float)(o / e);
          }
        }
        out[(size_t)((b * p.channels + ch) * n) + at(z, y, x)] = v;
      }
    }
  }
  return out;
}

static int failures = 0;

static void check(const Case& c) {
  const int64_t n = (int64_t)c.g.Z * c.g.Y * c.g.X;
  const uint32_t all = c.ndim == 3 ? 0x7654321u : 0x654321u;
  const int nch = c.ndim == 3 ? 7 : 6;
  const double samp[2][3] = {{1, 1, 1}, {2.0, 1.0, 0.5}};
  int configs = 0;
  for (int mode : {IT_MODE_THICK, IT_MODE_INNER})
    for (int conn = 1; conn <= c.ndim; ++conn)
      for (int flags : {0, IT_FLAG_F_EXCLUDES_C | IT_FLAG_D_RAW, IT_FLAG_D_RAW | IT_FLAG_D_CLIP}) {
        const double* s3 = samp[(conn + mode) & 1];
        const ItPack p{all, nch, c.ndim, conn, mode, flags, 1.75f, {s3[0], s3[1], s3[2]}};
        int64_t want_faults = 0;
        const std::vector<float> want = brute(c, p, want_faults);
        for (int64_t span : {(int64_t)OVL_SPAN, (int64_t)256, (int64_t)512})
          for (int threads : {1, 4}) {
            if ((conn > 1 || flags) && (span != OVL_SPAN || threads != 1)) continue;      // the records do not depend on these options
            std::vector<int32_t> ids((size_t)(c.B * n));
            int64_t faults = 0;
            for (int64_t i = 0; i < c.B * n; ++i) { uint32_t f; ids[(size_t)i] = it_id_f32(c.t[(size_t)i], c.g.n_max, f); faults += f; }
            const Records rec = stats_host(ids, c, s3, span, threads);
            const ItRecords view{rec.cen.data(), rec.box.data(), rec.dmax.data(), rec.rcmax.data()};
            std::vector<float> got((size_t)(c.B * nch * n), -9.f);
            for (int b = 0; b < c.B; ++b) {
              const std::vector<int32_t> sample(ids.begin() + b * n, ids.begin() + (b + 1) * n);      // it_differs sees one sample
              const uint32_t base = (uint32_t)(b * (c.g.n_max + 1));
              for (int64_t i = 0; i < n; ++i) {
                const RpPos q = rp_pos_of((uint32_t)i, c.g.Y, c.g.X);
                const int32_t l = sample[(size_t)i];
                const bool edge = it_needs_contour(p) && it_differs(sample.data(), c.g.Z, c.g.Y, c.g.X, q.z, q.y, q.x, p.ndim, p.conn, l);
                for (int ch = 0; ch < nch; ++ch)
                  got[(size_t)((b * nch + ch) * n + i)] = it_value(it_code(p.codes, ch), p, view, base + (uint32_t)l, l, edge, c.d[(size_t)(b * n + i)], q.z, q.y, q.x);
              }
            }
            ++configs;
            if (faults != want_faults || std::memcmp(got.data(), want.data(), got.size() * 4) != 0) {
              ++failures;
              size_t k = 0;
              while (k < got.size() && std::memcmp(&got[k], &want[k], 4) == 0) ++k;
              std::printf("MISMATCH %s mode %d conn %d flags %d span %lld threads %d: faults %lld / %lld, first at %zu: %g against %g\n", c.name.c_str(), mode,
                          conn, flags, (long long)span, threads, (long long)faults, (long long)want_faults, k, k < got.size() ? got[k] : 0.f, k < got.size() ? want[k] : 0.f);
            }
          }
      }
  std::printf("%-44s B %d  %3d x %3d x %4d  n_max %5d  %3d configurations\n", c.name.c_str(), c.B, c.g.Z, c.g.Y, c.g.X, c.g.n_max, configs);
}

// ids in boxes of random size (instances that touch, pieces of one id apart), the same generator for every sample so ids recur across samples
static Case make(const std::string& name, std::mt19937& rng, int B, int Z, int Y, int X, int ndim, int n_max, int labels, double bad) {
  Case c{name, B, Geom{Z, Y, X, n_max}, ndim, {}, {}};
  const int64_t n = (int64_t)Z * Y * X;
  c.t.assign((size_t)(B * n), 0.f);
  c.d.resize((size_t)(B * n));
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  const float odd[] = {-1.f, 2.5f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), (float)n_max + 1.f};
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k < labels * 2; ++k) {
      const int z0 = (int)(uni(rng) * Z), y0 = (int)(uni(rng) * Y), x0 = (int)(uni(rng) * X);
      const int z1 = std::min(Z, z0 + 1 + (int)(uni(rng) * 4)), y1 = std::min(Y, y0 + 1 + (int)(uni(rng) * 6)), x1 = std::min(X, x0 + 1 + (int)(uni(rng) * 90));
      const float id = (float)(1 + (int)(uni(rng) * (labels + 1)));                     // labels + 1 may lie above n_max
      for (int z = z0; z < z1; ++z) for (int y = y0; y < y1; ++y) for (int x = x0; x < x1; ++x) c.t[(size_t)(b * n + ((int64_t)z * Y + y) * X + x)] = id;
    }
    for (int64_t i = 0; i < n; ++i) {
      if (uni(rng) < bad) c.t[(size_t)(b * n + i)] = odd[(int)(uni(rng) * 6)];
      c.d[(size_t)(b * n + i)] = uni(rng) < 0.01 ? std::numeric_limits<float>::infinity() : (float)(uni(rng) * 9.0) + 0.5f;
    }
  }
  return c;
}

int main() {
  std::mt19937 rng(0);
  check(make("blobs 13 x 22 x 37, batch of 3", rng, 3, 13, 22, 37, 3, 9, 9, 0.0));
  check(make("2-D 45 x 50, batch of 3", rng, 3, 1, 45, 50, 2, 7, 7, 0.0));
  check(make("tiny 3 x 5 x 7", rng, 3, 3, 5, 7, 3, 3, 3, 0.0));
  check(make("values that are no id, ids above n_max", rng, 2, 4, 9, 40, 3, 5, 6, 0.05));
  for (int X : {1, 63, 64, 65, 255, 256, 257}) check(make("rows of " + std::to_string(X), rng, 1, 2, 3, X, 3, 5, 5, 0.0));
  check(make("all background", rng, 2, 4, 6, 10, 3, 5, 0, 0.0));
  check(make("n_max = 0 under ids", rng, 1, 4, 6, 10, 3, 0, 4, 0.0));
  for (int side : {8, 0}) {                                   // 512 ids in one block, 3000 in one span: past the table either way
    Case c{side ? "8^3, every voxel its own id" : "1 x 30 x 100, every voxel its own id", 1, side ? Geom{8, 8, 8, 512} : Geom{1, 30, 100, 3000}, side ? 3 : 2, {}, {}};
    const int n = side ? 512 : 3000;
    for (int i = 0; i < n; ++i) { c.t.push_back((float)(n - i)); c.d.push_back(1.f + (float)(i % 7)); }
    check(c);
  }
  { Case c{"an instance filling its sample", 2, Geom{3, 5, 7, 2}, 3, std::vector<float>(210, 2.f), std::vector<float>(210, std::numeric_limits<float>::infinity())};
    check(c); }
  if (failures) std::printf("FAILED: %d mismatches\n", failures);
  else std::printf("every case agrees with the per-voxel loops\n");
  return failures ? 1 : 0;
}
