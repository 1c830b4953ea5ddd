// Host run of the shape properties of biapy_amd/csrc/shapeprops.hip: the same steps (csrc/shapeprops_core.h: the closed-form moments of a run, the
// moments bound, the 128-bit covariance numerator and the finish row, the faces of a lane's voxels, the per-lane counter, the border and class
// rules of the 2-D perimeter, the merges of the block's tables; csrc/regionprops_core.h: label clamp, head rule, coordinates, carry step, slot
// search) in the launch sequences of bpx_region_moments, bpx_region_faces and bpx_region_perimeter2d - spans of `span` voxels walked in trips of
// 256 by a "wave" of 64 lanes, four waves to a block with its table; tiles of 16 x 64 pixels - sequentially and with the blocks and their waves
// spread over std::threads on std::atomic, checked against brute-force loops over the voxels.  The wave's shuffles and ballots are plain loops
// here; every load goes through a bounds-checked accessor under the guard the kernel uses, so an address outside the volume ends the run.
// Cases: random label volumes (runs that continue across row ends), 0 / 1 / 7 / 1000 labels (1000 overflow the block's table), X = 1, Y = 1,
// Z = 1, rows one below, at and above 64, 256 and 8192, a label filling the volume, the longest row the moments bound admits (2^21 voxels: the
// closed form's largest intermediate is just below 2^64) and the refusal one above it, every voxel its own label, labels above n_max and
// negative ones.  The 128-bit numerator is held against a schoolbook product of 32-bit limbs.  A development aid:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -pthread -I biapy_amd/csrc scripts/shapeprops_cpu_check.cpp -o shapeprops_cpu_check
//   ./shapeprops_cpu_check
// Prints one line per case and exits nonzero on the first mismatch.  Not loaded into Python, not part of the test suite.
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "shapeprops_core.h"
#include "label_walk_host.h"

struct HostKeys {
  std::atomic<int32_t>* keys = nullptr;
  std::atomic<uint32_t>* claimed = nullptr;
  int32_t kload(uint32_t s) const { return keys[s].load(std::memory_order_relaxed); }
  int32_t kcas(uint32_t s, int32_t label) const {
    int32_t expected = 0;
    keys[s].compare_exchange_strong(expected, label, std::memory_order_relaxed);
    return expected;
  }
  uint32_t nclaimed() const { return claimed->load(std::memory_order_relaxed); }
  void claim() const { claimed->fetch_add(1, std::memory_order_relaxed); }
};
struct HostMom : HostKeys {      // the global rows, or a block's table when keys != nullptr
  std::atomic<uint64_t>* p = nullptr;
  void mom(uint32_t r, int k, uint64_t v) const { p[(size_t)r * SP_MOMENTS + k].fetch_add(v, std::memory_order_relaxed); }
  uint64_t mom_of(uint32_t s, int k) const { return p[(size_t)s * SP_MOMENTS + k].load(); }
};
template <class T> struct HostCnt : HostKeys {
  std::atomic<T>* p = nullptr;
  void cnt(uint32_t r, int k, uint32_t v) const { p[(size_t)r * SP_COUNTERS + k].fetch_add((T)v, std::memory_order_relaxed); }
  uint32_t cnt_of(uint32_t s, int k) const { return (uint32_t)p[(size_t)s * SP_COUNTERS + k].load(); }
};

// a block's table: keys, the counter of claimed slots and `width` zeroed fields per slot
template <class T> struct Table {
  std::unique_ptr<std::atomic<int32_t>[]> keys{new std::atomic<int32_t>[RP_LOCAL_SLOTS]};
  std::unique_ptr<std::atomic<T>[]> fields;
  std::atomic<uint32_t> claimed{0};
  explicit Table(int width) : fields(new std::atomic<T>[(size_t)RP_LOCAL_SLOTS * width]) {
    for (int s = 0; s < RP_LOCAL_SLOTS; ++s) keys[(size_t)s].store(0);
    for (int s = 0; s < RP_LOCAL_SLOTS * width; ++s) fields[(size_t)s].store(0);
  }
};

static void parallel_for(int threads, int64_t count, const std::function<void(int64_t)>& f) {   // item q runs on thread q % threads
  if (threads <= 1) { for (int64_t q = 0; q < count; ++q) f(q); return; }
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([=, &f] { for (int64_t q = t; q < count; q += threads) f(q); });
  for (auto& th : pool) th.join();
}

struct Geom { int Z, Y, X, n_max; };
static int failures = 0;

// a load of the kernels: the address must lie inside the volume
static int32_t at(const std::vector<int32_t>& labels, int64_t i) {
  if (i < 0 || i >= (int64_t)labels.size()) { std::printf("LOAD OUTSIDE THE VOLUME: %lld of %zu\n", (long long)i, labels.size()); std::abort(); }
  return labels[(size_t)i];
}

// ---- moments: sp_moments_kernel, one wave's span: the walk of label_walk_host.h with the moments' emit --------------------------------------------
static void moments_span(const HostMom& loc, const HostMom& m, const std::vector<int32_t>& labels, const Geom& g, int64_t begin, int64_t end) {
  lw_walk_runs_host(labels, g, begin, end, [&](int32_t label, int32_t z, int32_t y, int32_t x0, uint32_t L) { sp_emit_moments(loc, m, label, z, y, x0, L); });
}

// ---- faces: sp_faces_kernel, one wave's span; `rowvec` takes the 16-byte path where the kernel would -------------------------------------------------
static void faces_span(const HostCnt<uint32_t>& loc, const HostCnt<uint64_t>& m, const std::vector<int32_t>& labels, const Geom& g, int64_t begin, int64_t end) {
  const RpStride stride = rp_stride(g.Y, g.X);
  const bool rowvec = (g.X & 3) == 0;
  const int64_t plane = (int64_t)g.Y * g.X;
  RpPos lane_at[OVL_LANES];
  for (int l = 0; l < OVL_LANES; ++l) lane_at[l] = rp_pos_of((uint32_t)(begin + OVL_VPL * l), g.Y, g.X);
  for (int64_t t = begin; t < end; t += OVL_TRIP) {
    int32_t lab[OVL_LANES][OVL_VPL];
    RpPos pos[OVL_LANES][OVL_VPL];
    for (int l = 0; l < OVL_LANES; ++l)
      for (int e = 0; e < OVL_VPL; ++e) {
        const int64_t i = t + OVL_VPL * l + e;
        lab[l][e] = rp_label(i < end ? at(labels, i) : 0, g.n_max);
        if (e) { pos[l][e] = pos[l][e - 1]; rp_step(pos[l][e], g.Y, g.X); } else pos[l][0] = lane_at[l];
      }
    for (int l = 0; l < OVL_LANES; ++l) {
      const int64_t i0 = t + OVL_VPL * l;
      int32_t left = l ? lab[l - 1][OVL_VPL - 1] : 0, right = l < OVL_LANES - 1 ? lab[l + 1][0] : 0;      // the shuffles: lane 0 / 63 receive their own value, unused
      if (l == 0) left = lab[0][OVL_VPL - 1];
      if (l == OVL_LANES - 1) right = lab[l][0];
      if (l == 0 && lab[l][0] > 0 && pos[l][0].x > 0) left = rp_label(at(labels, i0 - 1), g.n_max);
      if (l == OVL_LANES - 1 && lab[l][OVL_VPL - 1] > 0 && pos[l][OVL_VPL - 1].x < g.X - 1) right = rp_label(at(labels, i0 + OVL_VPL), g.n_max);
      if ((lab[l][0] | lab[l][1] | lab[l][2] | lab[l][3]) == 0) continue;
      int32_t ym[OVL_VPL], yp[OVL_VPL], zm[OVL_VPL], zp[OVL_VPL];
      if (rowvec && i0 + OVL_VPL <= end) {
        for (int e = 0; e < OVL_VPL; ++e) {
          ym[e] = pos[l][0].y > 0 ? rp_label(at(labels, i0 - g.X + e), g.n_max) : SP_OUTSIDE;
          yp[e] = pos[l][0].y < g.Y - 1 ? rp_label(at(labels, i0 + g.X + e), g.n_max) : SP_OUTSIDE;
          zm[e] = pos[l][0].z > 0 ? rp_label(at(labels, i0 - plane + e), g.n_max) : SP_OUTSIDE;
          zp[e] = pos[l][0].z < g.Z - 1 ? rp_label(at(labels, i0 + plane + e), g.n_max) : SP_OUTSIDE;
        }
      } else {
        for (int e = 0; e < OVL_VPL; ++e) {
          const bool on = lab[l][e] > 0;
          ym[e] = on && pos[l][e].y > 0 ? rp_label(at(labels, i0 + e - g.X), g.n_max) : SP_OUTSIDE;
          yp[e] = on && pos[l][e].y < g.Y - 1 ? rp_label(at(labels, i0 + e + g.X), g.n_max) : SP_OUTSIDE;
          zm[e] = on && pos[l][e].z > 0 ? rp_label(at(labels, i0 + e - plane), g.n_max) : SP_OUTSIDE;
          zp[e] = on && pos[l][e].z < g.Z - 1 ? rp_label(at(labels, i0 + e + plane), g.n_max) : SP_OUTSIDE;
        }
      }
      sp_lane_faces(loc, m, lab[l], pos[l], left, right, ym, yp, zm, zp, g.X);
    }
    for (int l = 0; l < OVL_LANES; ++l) rp_advance(lane_at[l], stride, g.Y, g.X);
  }
}

struct Shape {
  std::vector<int64_t> mom, faces;
  std::vector<int32_t> classes;
  bool operator==(const Shape& o) const { return mom == o.mom && faces == o.faces && classes == o.classes; }
};

template <class T, class U> static std::vector<U> unload(const std::unique_ptr<std::atomic<T>[]>& a, size_t n) {
  std::vector<U> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = (U)a[i].load();
  return v;
}

// the launch sequences; `span` = OVL_SPAN on the device; classes only for Z = 1
static Shape shape_host(const std::vector<int32_t>& labels, const Geom& g, int64_t span, int threads) {
  const int64_t n = (int64_t)labels.size();
  const size_t rows = (size_t)g.n_max + 1;
  std::unique_ptr<std::atomic<uint64_t>[]> mom(new std::atomic<uint64_t>[rows * SP_MOMENTS]), faces(new std::atomic<uint64_t>[rows * SP_COUNTERS]);
  std::unique_ptr<std::atomic<uint32_t>[]> classes(new std::atomic<uint32_t>[rows * SP_COUNTERS]);
  for (size_t i = 0; i < rows * SP_MOMENTS; ++i) mom[i].store(0);                          // the zero pass
  for (size_t i = 0; i < rows * SP_COUNTERS; ++i) { faces[i].store(0); classes[i].store(0); }
  HostMom gm; gm.p = mom.get();
  HostCnt<uint64_t> gf; gf.p = faces.get();
  HostCnt<uint32_t> gc; gc.p = classes.get();
  const int64_t spans = (n + span - 1) / span, blocks = (spans + OVL_WAVES - 1) / OVL_WAVES;
  parallel_for(threads, blocks, [&](int64_t blk) {
    Table<uint64_t> tm(SP_MOMENTS);
    Table<uint32_t> tf(SP_COUNTERS);
    HostMom lm; lm.keys = tm.keys.get(); lm.claimed = &tm.claimed; lm.p = tm.fields.get();
    HostCnt<uint32_t> lf; lf.keys = tf.keys.get(); lf.claimed = &tf.claimed; lf.p = tf.fields.get();
    parallel_for(threads > 1 ? 2 : 1, OVL_WAVES, [&](int64_t w) {
      const int64_t begin = (blk * OVL_WAVES + w) * span;
      if (begin >= n) return;
      moments_span(lm, gm, labels, g, begin, std::min(n, begin + span));
      faces_span(lf, gf, labels, g, begin, std::min(n, begin + span));
    });
    for (int s = 0; s < RP_LOCAL_SLOTS; ++s) { sp_merge_moments(lm, (uint32_t)s, gm); sp_merge_counts(lf, (uint32_t)s, gf); }
  });
  if (g.Z == 1) {                                                                         // sp_perimeter_kernel
    const int64_t tiles_x = (g.X + SP_TX - 1) / SP_TX, tiles = tiles_x * ((g.Y + SP_TY - 1) / SP_TY);
    parallel_for(threads, tiles, [&](int64_t b) {
      Table<uint32_t> tc(SP_COUNTERS);
      HostCnt<uint32_t> lc; lc.keys = tc.keys.get(); lc.claimed = &tc.claimed; lc.p = tc.fields.get();
      const int y0 = (int)(b / tiles_x) * SP_TY, x0 = (int)(b % tiles_x) * SP_TX;
      std::vector<int32_t> lab((size_t)SP_LH * SP_LW);                                    // exactly the tile: an index past it is the sanitizer's
      std::vector<unsigned char> bor((size_t)SP_BH * SP_BW);
      for (int i = 0; i < SP_LH * SP_LW; ++i) {
        const int64_t gy = (int64_t)y0 - 2 + i / SP_LW, gx = (int64_t)x0 - 2 + i % SP_LW;
        lab[(size_t)i] = gy >= 0 && gy < g.Y && gx >= 0 && gx < g.X ? rp_label(at(labels, gy * g.X + gx), g.n_max) : 0;
      }
      for (int i = 0; i < SP_BH * SP_BW; ++i) {
        const size_t c = (size_t)((i / SP_BW + 1) * SP_LW + i % SP_BW + 1);
        bor[(size_t)i] = sp_is_border(lab.at(c), lab.at(c - SP_LW), lab.at(c + SP_LW), lab.at(c - 1), lab.at(c + 1)) ? 1 : 0;
      }
      for (int th = 0; th < 256; ++th) {
        const int ty = th / (SP_TX / 4), tx = (th % (SP_TX / 4)) * 4;
        SpCount acc{0, {0, 0, 0}};
        for (int e = 0; e < 4; ++e) {
          const int cls = sp_pixel_class(lab, bor, ty, tx + e);
          sp_count_step(lc, gc, acc, cls < 0 ? 0 : lab[(size_t)((ty + 2) * SP_LW + tx + e + 2)], cls == 0, cls == 1, cls == 2);
        }
        sp_count_flush(lc, gc, acc);
      }
      for (int s = 0; s < RP_LOCAL_SLOTS; ++s) sp_merge_counts(lc, (uint32_t)s, gc);
    });
  }
  return Shape{unload<uint64_t, int64_t>(mom, rows * SP_MOMENTS), unload<uint64_t, int64_t>(faces, rows * SP_COUNTERS),
               unload<uint32_t, int32_t>(classes, rows * SP_COUNTERS)};
}

// the statement: one visit per voxel
static Shape shape_brute(const std::vector<int32_t>& labels, const Geom& g) {
  const size_t rows = (size_t)g.n_max + 1;
  Shape out{std::vector<int64_t>(rows * SP_MOMENTS, 0), std::vector<int64_t>(rows * SP_COUNTERS, 0), std::vector<int32_t>(rows * SP_COUNTERS, 0)};
  auto lab = [&](int64_t z, int64_t y, int64_t x) -> int32_t {
    if (z < 0 || y < 0 || x < 0 || z >= g.Z || y >= g.Y || x >= g.X) return -1;
    const int32_t l = labels[(size_t)((z * g.Y + y) * g.X + x)];
    return l > 0 && l <= g.n_max ? l : 0;
  };
  auto border = [&](int64_t y, int64_t x) -> bool {
    const int32_t l = lab(0, y, x);
    return l > 0 && (lab(0, y - 1, x) != l || lab(0, y + 1, x) != l || lab(0, y, x - 1) != l || lab(0, y, x + 1) != l);
  };
  for (int64_t z = 0; z < g.Z; ++z)
    for (int64_t y = 0; y < g.Y; ++y)
      for (int64_t x = 0; x < g.X; ++x) {
        const int32_t l = lab(z, y, x);
        if (l <= 0) continue;
        const int64_t v[SP_MOMENTS] = {z * z, y * y, x * x, z * y, z * x, y * x};
        for (int k = 0; k < SP_MOMENTS; ++k) out.mom[(size_t)l * SP_MOMENTS + k] += v[k];
        out.faces[(size_t)l * 3 + 0] += (lab(z - 1, y, x) != l) + (lab(z + 1, y, x) != l);
        out.faces[(size_t)l * 3 + 1] += (lab(z, y - 1, x) != l) + (lab(z, y + 1, x) != l);
        out.faces[(size_t)l * 3 + 2] += (lab(z, y, x - 1) != l) + (lab(z, y, x + 1) != l);
        if (g.Z != 1 || !border(y, x)) continue;
        int code = 1;
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx)
            if ((dy || dx) && lab(0, y + dy, x + dx) == l && border(y + dy, x + dx)) code += (dy == 0 || dx == 0) ? 2 : 10;
        const bool c0 = code == 5 || code == 7 || code == 15 || code == 17 || code == 25 || code == 27;
        const int cls = c0 ? 0 : (code == 21 || code == 33) ? 1 : (code == 13 || code == 23) ? 2 : -1;
        if (cls >= 0) ++out.classes[(size_t)l * 3 + (size_t)cls];
      }
  return out;
}

static void check(const std::string& name, const std::vector<int32_t>& labels, const Geom& g) {
  const Shape want = shape_brute(labels, g);
  const bool big = labels.size() > 500000;
  for (int64_t span : {(int64_t)OVL_SPAN, (int64_t)256, (int64_t)512}) {
    if (big && span != OVL_SPAN) continue;
    for (int threads : {1, 4}) {
      const Shape got = shape_host(labels, g, span, threads);
      if (!(got == want)) {
        ++failures;
        std::printf("MISMATCH %s span %lld threads %d: moments %d faces %d classes %d\n", name.c_str(), (long long)span, threads, got.mom == want.mom,
                    got.faces == want.faces, got.classes == want.classes);
      }
    }
  }
  std::printf("%-44s %5d x %5d x %7d  n_max %7d\n", name.c_str(), g.Z, g.Y, g.X, g.n_max);
}

static std::vector<int32_t> runs(std::mt19937& rng, size_t n, int labels, double bg, double mean_run) {
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  std::vector<int32_t> v(n);
  int32_t cur = 0;
  for (size_t i = 0; i < n; ++i) {
    if (i == 0 || uni(rng) < 1.0 / mean_run) {
      const double u = uni(rng);
      cur = u < bg ? (uni(rng) < 0.3 ? -(int32_t)(1 + uni(rng) * 5) : 0) : labels ? 1 + (int32_t)(uni(rng) * (labels + 2)) : 0;      // labels + 1, labels + 2: above n_max
    }
    v[i] = cur;
  }
  return v;
}

// ---- the 128-bit numerator against a schoolbook product of 32-bit limbs --------------------------------------------------------------------------------
struct Limbs { uint32_t w[4]; };
static Limbs school_mul(uint64_t a, uint64_t b) {
  const uint32_t x[2] = {(uint32_t)a, (uint32_t)(a >> 32)}, y[2] = {(uint32_t)b, (uint32_t)(b >> 32)};
  uint64_t acc[4] = {0, 0, 0, 0};
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) {
      const uint64_t p = (uint64_t)x[i] * y[j];
      acc[i + j] += (uint32_t)p;
      acc[i + j + 1] += p >> 32;
    }
  Limbs r;
  uint64_t carry = 0;
  for (int k = 0; k < 4; ++k) { const uint64_t s = acc[k] + carry; r.w[k] = (uint32_t)s; carry = s >> 32; }
  return r;
}
static bool school_less(const Limbs& a, const Limbs& b) {
  for (int k = 3; k >= 0; --k)
    if (a.w[k] != b.w[k]) return a.w[k] < b.w[k];
  return false;
}
static Limbs school_sub(const Limbs& a, const Limbs& b) {   // a >= b
  Limbs r;
  int64_t borrow = 0;
  for (int k = 0; k < 4; ++k) {
    int64_t d = (int64_t)a.w[k] - b.w[k] - borrow;
    borrow = d < 0;
    r.w[k] = (uint32_t)(d + (borrow << 32));
  }
  return r;
}
static void check_numerator(uint64_t A, uint64_t M, uint64_t Sa, uint64_t Sb) {
  const SpWide got = sp_cov_numerator(A, M, Sa, Sb);
  const Limbs p = school_mul(A, M), q = school_mul(Sa, Sb);
  const bool neg = school_less(p, q);
  const Limbs d = neg ? school_sub(q, p) : school_sub(p, q);
  const uint64_t hi = ((uint64_t)d.w[3] << 32) | d.w[2], lo = ((uint64_t)d.w[1] << 32) | d.w[0];
  if (got.hi != hi || got.lo != lo || got.neg != neg) {
    ++failures;
    std::printf("MISMATCH numerator A %llu M %llu Sa %llu Sb %llu\n", (unsigned long long)A, (unsigned long long)M, (unsigned long long)Sa, (unsigned long long)Sb);
  }
}

int main() {
  std::mt19937 rng(0);
  const int shapes[][3] = {{9, 21, 37}, {8, 16, 64}, {1, 33, 70}, {1, 37, 41}, {5, 1, 1}, {1, 300, 1}, {300, 1, 1}, {1, 1, 300}, {7, 5, 1}, {3, 7, 2}, {5, 9, 3},
                           {2, 3, 4}, {6, 1, 40}, {3, 2, 63}, {3, 2, 64}, {3, 2, 65}, {1, 2, 255}, {2, 2, 256}, {1, 2, 257}, {1, 2, 8191}, {1, 2, 8192},
                           {2, 2, 8193}, {2, 130, 129}, {1, 40, 132}, {3, 20, 68}};
  for (const auto& s : shapes)
    for (int labels : {0, 1, 7, 1000})
      for (double run : {1.0, 3.0, 40.0, 3000.0}) {
        const Geom g{s[0], s[1], s[2], labels};
        check("random L" + std::to_string(labels) + " run " + std::to_string((int)run), runs(rng, (size_t)s[0] * s[1] * s[2], labels, 0.5, run), g);
      }
  for (int X : {1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193}) {                        // one label fills the volume: faces only on its hull
    const Geom g{2, 3, X, 5};
    check("one label fills 2 x 3 x " + std::to_string(X), std::vector<int32_t>((size_t)6 * X, 5), g);
  }
  { const Geom g{1, 17, 70, 2};                                                           // a checkerboard of two labels and one-pixel lines
    std::vector<int32_t> v((size_t)17 * 70);
    for (int y = 0; y < 17; ++y) for (int x = 0; x < 70; ++x) v[(size_t)y * 70 + x] = 1 + ((x + y) & 1);
    check("checkerboard of two labels", v, g);
    for (int y = 0; y < 17; ++y) for (int x = 0; x < 70; ++x) v[(size_t)y * 70 + x] = (y % 3 == 0) ? 1 : (x % 5 == 0) ? 2 : 0;
    check("one-pixel lines", v, g); }
  { const Geom g{1, 1, 1100000, 3}; check("one label fills a row of 1 100 000", std::vector<int32_t>((size_t)1100000, 3), g); }
  { const Geom g{3, 3, 70000, 1}; check("one label, rows of 70 000", std::vector<int32_t>((size_t)9 * 70000, 1), g); }
  { const int E = 1 << 21;                                                                // the moments bound: E (E - 1)^2 < 2^63 <= (E + 1) E^2
    if (!sp_moments_fit(E, E) || sp_moments_fit((int64_t)E + 1, (int64_t)E + 1)) { ++failures; std::printf("MISMATCH the moments bound at 2^21\n"); }
    if (!sp_moments_fit(INT32_MAX, 1) || !sp_moments_fit(1, 1) || sp_moments_fit(INT32_MAX, INT32_MAX) || sp_moments_fit((int64_t)1 << 30, (int64_t)1 << 17) ||
        !sp_moments_fit(((int64_t)1 << 30) - 1, ((int64_t)1 << 16) + 1)) { ++failures; std::printf("MISMATCH the moments bound\n"); }
    const Geom g{1, 1, E, 1};
    check("the longest row the moments bound admits", std::vector<int32_t>((size_t)E, 1), g); }
  { const Geom g{4, 32, 64, 8192};
    std::vector<int32_t> v(8192);
    for (int i = 0; i < 8192; ++i) v[(size_t)i] = 8192 - i;
    check("every voxel its own label", v, g); }
  { const Geom g{5, 40, 100, 9}; check("all background", std::vector<int32_t>(20000, 0), g); }
  { const Geom g{5, 40, 100, 0}; check("n_max = 0 under labels", runs(rng, 20000, 7, 0.3, 9.0), g); }
  { const Geom g{5, 40, 100, 3}; check("labels above n_max = 3", runs(rng, 20000, 7, 0.3, 9.0), g); }
  { const Geom g{1, 90, 100, 4}; check("negative labels only", std::vector<int32_t>(9000, -3), g); }
  { const Geom g{1, 1, 300, 1000}; check("labels of INT32_MAX, n_max 1000", std::vector<int32_t>(300, INT32_MAX), g); }

  // the numerator: the extremes the entry admits (A < 2^31, M < 2^63, S < 2^62), equal products, a negative numerator, random operands
  check_numerator(0, 0, 0, 0);
  check_numerator(((uint64_t)1 << 31) - 1, ((uint64_t)1 << 63) - 1, 0, 0);
  check_numerator(1, 0, ((uint64_t)1 << 62) - 1, ((uint64_t)1 << 62) - 1);
  check_numerator(3, 12, 6, 6);
  check_numerator(UINT64_MAX, UINT64_MAX, UINT64_MAX, UINT64_MAX - 1);
  check_numerator(UINT64_MAX, UINT64_MAX - 1, UINT64_MAX, UINT64_MAX);
  for (int i = 0; i < 200000; ++i) {
    const uint64_t a = ((uint64_t)rng() << 32 | rng()) >> (rng() % 64), b = ((uint64_t)rng() << 32 | rng()) >> (rng() % 64);
    const uint64_t c = ((uint64_t)rng() << 32 | rng()) >> (rng() % 64), d = ((uint64_t)rng() << 32 | rng()) >> (rng() % 64);
    check_numerator(a, b, c, d);
  }
  // the finish row of a full cube of edge E: covariance (E^2 - 1) / 12 per axis, 0 off the diagonal; an absent label: zeros
  for (int64_t E : {1, 2, 7, 64, 1000}) {
    const int32_t area = (int32_t)(E * E * E);
    const int64_t s1 = E * E * (E * (E - 1) / 2), s2 = E * E * ((E - 1) * E * (2 * E - 1) / 6), sc = E * (E * (E - 1) / 2) * (E * (E - 1) / 2);
    const int64_t sums[3] = {s1, s1, s1}, mom[SP_MOMENTS] = {s2, s2, s2, sc, sc, sc};
    double cov[SP_MOMENTS];
    sp_finish_row(&area, sums, mom, cov);
    for (int k = 0; k < SP_MOMENTS; ++k)
      if (cov[k] != (k < 3 ? (double)(E * E - 1) / 12.0 : 0.0)) { ++failures; std::printf("MISMATCH cube %lld cov[%d] = %.17g\n", (long long)E, k, cov[k]); }
  }
  { const int32_t area = 0; const int64_t sums[3] = {5, 6, 7}, mom[SP_MOMENTS] = {1, 2, 3, 4, 5, 6}; double cov[SP_MOMENTS];
    sp_finish_row(&area, sums, mom, cov);
    for (int k = 0; k < SP_MOMENTS; ++k) if (cov[k] != 0.0) { ++failures; std::printf("MISMATCH absent label cov[%d]\n", k); } }
  if (failures) std::printf("FAILED: %d mismatches\n", failures);
  else std::printf("all cases agree with the per-voxel loop\n");
  return failures ? 1 : 0;
}
