// Host run of the region properties of biapy_amd/csrc/regionprops.hip: the same steps (csrc/regionprops_core.h: the label a voxel counts for, the
// head rule, a lane's coordinates by rp_pos_of / rp_step / rp_advance, the carry step, the closed-form contribution of a run, the block's table
// keyed by label and its merge, the init and finish rows; csrc/overlap_core.h: the head positions in a trip) in the launch sequence of
// bpx_region_props - init; accumulate over spans of `span` voxels walked in trips of 256 by a "wave" of 64 lanes, four waves to a block, in form
// (a) straight to the per-label arrays and in form (b) through the block's own table that is merged into them; finish - sequentially and with the
// blocks and their waves spread over std::threads on std::atomic, checked against a brute-force loop over the voxels.  The walk of a span is
// scripts/label_walk_host.h's (shared with shapeprops_cpu_check.cpp): the wave's shuffle and ballots are plain loops there; everything that
// decides a run, its coordinates or its contribution is the shared code.
// Cases: random label volumes (runs of geometric length that continue across row ends), 0 / 1 / 7 / 1000 labels (1000 overflow the block's
// table), X = 1, X one below, at and above 64, 256 and 8192, one label filling a row of 1 100 000 voxels (L x0 passes 2^32), every voxel its own
// label, all background, labels above n_max and negative ones, n_max = 0.  Spans of OVL_SPAN and, to meet many span ends in small volumes, of
// 256 and 512.  A development aid for finding an off-by-one at a row, trip or span end before the kernels run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -I biapy_amd/csrc scripts/regionprops_cpu_check.cpp -o regionprops_cpu_check
//   ./regionprops_cpu_check
// Prints one line per case and exits nonzero on the first mismatch.  Not loaded into Python, not part of the test suite.
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdio>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "regionprops_core.h"
#include "label_walk_host.h"

template <class T> static void atomic_min(std::atomic<T>& a, T v) {
  T cur = a.load(std::memory_order_relaxed);
  while (v < cur && !a.compare_exchange_weak(cur, v, std::memory_order_relaxed)) {}
}
template <class T> static void atomic_max(std::atomic<T>& a, T v) {
  T cur = a.load(std::memory_order_relaxed);
  while (v > cur && !a.compare_exchange_weak(cur, v, std::memory_order_relaxed)) {}
}

struct HostMem {     // the global arrays, or a block's table when keys != nullptr
  std::atomic<uint32_t>* area_p;
  std::atomic<uint64_t>* sums_p;
  std::atomic<int32_t>* box_p;
  std::atomic<int32_t>* keys = nullptr;
  std::atomic<uint32_t>* claimed = nullptr;
  void area(uint32_t r, uint32_t c) const { area_p[r].fetch_add(c, std::memory_order_relaxed); }
  void sum(uint32_t r, int k, uint64_t v) const { sums_p[(size_t)r * 3 + k].fetch_add(v, std::memory_order_relaxed); }
  void lo(uint32_t r, int k, int32_t v) const { atomic_min(box_p[(size_t)r * 6 + k], v); }
  void hi(uint32_t r, int k, int32_t v) const { atomic_max(box_p[(size_t)r * 6 + 3 + k], v); }
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
};

static void parallel_for(int threads, int64_t count, const std::function<void(int64_t)>& f) {   // item q runs on thread q % threads: neighbouring spans on different threads
  if (threads <= 1) { for (int64_t q = 0; q < count; ++q) f(q); return; }
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([=, &f] { for (int64_t q = t; q < count; q += threads) f(q); });
  for (auto& th : pool) th.join();
}

struct Geom { int Z, Y, X, n_max; };

// one wave's span [begin, end): rp_accumulate_kernel's call of the walk (label_walk_host.h); loc == nullptr is form (a)
static void accumulate_span(const HostMem* loc, const HostMem& m, const std::vector<int32_t>& labels, const Geom& g, int64_t begin, int64_t end) {
  lw_walk_runs_host(labels, g, begin, end, [&](int32_t label, int32_t z, int32_t y, int32_t x0, uint32_t L) {
    if (loc) rp_emit(*loc, m, label, z, y, x0, L);
    else rp_emit(m, label, z, y, x0, L);
  });
}

struct Props {
  std::vector<int32_t> area, box;
  std::vector<int64_t> sums;
  bool operator==(const Props& o) const { return area == o.area && box == o.box && sums == o.sums; }
};

// the launch sequence of bpx_region_props; `span` = OVL_SPAN on the device
static Props props_host(const std::vector<int32_t>& labels, const Geom& g, int64_t span, int threads, bool local) {
  const int64_t n = (int64_t)labels.size(), rows = (int64_t)g.n_max + 1;
  Props out;                                                   // exactly n_max + 1 rows: a write past them is the sanitizer's
  out.area.assign((size_t)rows, -7);
  out.sums.assign((size_t)rows * 3, -7);
  out.box.assign((size_t)rows * 6, -7);
  for (int64_t r = 0; r < rows; ++r) rp_init_row(&out.area[(size_t)r], &out.sums[(size_t)r * 3], &out.box[(size_t)r * 6]);          // init
  std::unique_ptr<std::atomic<uint32_t>[]> area(new std::atomic<uint32_t>[(size_t)rows]);
  std::unique_ptr<std::atomic<uint64_t>[]> sums(new std::atomic<uint64_t>[(size_t)rows * 3]);
  std::unique_ptr<std::atomic<int32_t>[]> box(new std::atomic<int32_t>[(size_t)rows * 6]);
  for (int64_t r = 0; r < rows; ++r) {
    area[(size_t)r].store((uint32_t)out.area[(size_t)r]);
    for (int k = 0; k < 3; ++k) sums[(size_t)r * 3 + k].store((uint64_t)out.sums[(size_t)r * 3 + k]);
    for (int k = 0; k < 6; ++k) box[(size_t)r * 6 + k].store(out.box[(size_t)r * 6 + k]);
  }
  const HostMem m{area.get(), sums.get(), box.get()};
  const int64_t spans = (n + span - 1) / span;
  parallel_for(threads, (spans + OVL_WAVES - 1) / OVL_WAVES, [&](int64_t blk) {          // a block: its own table, OVL_WAVES spans, the flush
    std::unique_ptr<std::atomic<int32_t>[]> lkeys(new std::atomic<int32_t>[RP_LOCAL_SLOTS]);
    std::unique_ptr<std::atomic<uint32_t>[]> larea(new std::atomic<uint32_t>[RP_LOCAL_SLOTS]);
    std::unique_ptr<std::atomic<uint64_t>[]> lsums(new std::atomic<uint64_t>[RP_LOCAL_SLOTS * 3]);
    std::unique_ptr<std::atomic<int32_t>[]> lbox(new std::atomic<int32_t>[RP_LOCAL_SLOTS * 6]);
    std::atomic<uint32_t> lclaimed{0};
    for (int s = 0; s < RP_LOCAL_SLOTS; ++s) {
      lkeys[(size_t)s].store(0);
      larea[(size_t)s].store(0);
      for (int k = 0; k < 3; ++k) { lsums[(size_t)s * 3 + k].store(0); lbox[(size_t)s * 6 + k].store(RP_LO_INIT); lbox[(size_t)s * 6 + 3 + k].store(RP_HI_INIT); }
    }
    const HostMem loc{larea.get(), lsums.get(), lbox.get(), lkeys.get(), &lclaimed};
    parallel_for(threads > 1 ? 2 : 1, OVL_WAVES, [&](int64_t w) {
      const int64_t begin = (blk * OVL_WAVES + w) * span;
      if (begin < n) accumulate_span(local ? &loc : nullptr, m, labels, g, begin, std::min(n, begin + span));
    });
    if (local)
      for (int s = 0; s < RP_LOCAL_SLOTS; ++s) rp_merge(loc, (uint32_t)s, m);
  });
  for (int64_t r = 0; r < rows; ++r) {                                                   // finish
    out.area[(size_t)r] = (int32_t)area[(size_t)r].load();
    for (int k = 0; k < 3; ++k) out.sums[(size_t)r * 3 + k] = (int64_t)sums[(size_t)r * 3 + k].load();
    for (int k = 0; k < 6; ++k) out.box[(size_t)r * 6 + k] = box[(size_t)r * 6 + k].load();
    rp_finish_row(r, &out.area[(size_t)r], &out.sums[(size_t)r * 3], &out.box[(size_t)r * 6]);
  }
  return out;
}

// the statement: one visit per voxel
static Props props_brute(const std::vector<int32_t>& labels, const Geom& g) {
  const size_t rows = (size_t)g.n_max + 1;
  Props out;
  out.area.assign(rows, 0);
  out.sums.assign(rows * 3, 0);
  out.box.assign(rows * 6, 0);
  std::vector<char> seen(rows, 0);
  size_t i = 0;
  for (int z = 0; z < g.Z; ++z)
    for (int y = 0; y < g.Y; ++y)
      for (int x = 0; x < g.X; ++x, ++i) {
        const int32_t l = labels[i];
        if (l <= 0 || l > g.n_max) continue;
        const int c[3] = {z, y, x};
        ++out.area[(size_t)l];
        for (int k = 0; k < 3; ++k) {
          out.sums[(size_t)l * 3 + k] += c[k];
          int32_t &lo = out.box[(size_t)l * 6 + k], &hi = out.box[(size_t)l * 6 + 3 + k];
          lo = seen[(size_t)l] ? std::min(lo, c[k]) : c[k];
          hi = seen[(size_t)l] ? std::max(hi, c[k] + 1) : c[k] + 1;
        }
        seen[(size_t)l] = 1;
      }
  return out;
}

static int failures = 0;

static void check(const std::string& name, const std::vector<int32_t>& labels, const Geom& g) {
  const Props want = props_brute(labels, g);
  const bool big = labels.size() > 500000;                     // the long rows: the device's span only, fewer thread counts
  for (int64_t span : {(int64_t)OVL_SPAN, (int64_t)256, (int64_t)512}) {
    if (big && span != OVL_SPAN) continue;
    for (int threads : {1, 4})
      for (bool local : {false, true})
        if (!(props_host(labels, g, span, threads, local) == want)) {
          ++failures;
          std::printf("MISMATCH %s span %lld threads %d form %s\n", name.c_str(), (long long)span, threads, local ? "(b)" : "(a)");
        }
  }
  int64_t present = 0;
  for (int32_t a : want.area) present += a != 0;
  std::printf("%-40s %5d x %5d x %7d  n_max %7d  labels present %7lld\n", name.c_str(), g.Z, g.Y, g.X, g.n_max, (long long)present);
}

// labels in runs of geometric length that do not stop at row ends: `labels` ids, background with weight `bg`, some negative, some above n_max
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

int main() {
  std::mt19937 rng(0);
  const int shapes[][3] = {{9, 21, 37}, {8, 16, 64}, {1, 33, 70}, {5, 1, 1}, {1, 300, 1}, {300, 1, 1}, {1, 1, 300}, {7, 5, 1}, {3, 7, 2}, {5, 9, 3}, {2, 3, 4},
                           {3, 2, 63}, {3, 2, 64}, {3, 2, 65}, {1, 2, 255}, {2, 2, 256}, {1, 2, 257}, {1, 2, 8191}, {1, 2, 8192}, {2, 2, 8193}, {2, 130, 129}};
  for (const auto& s : shapes)
    for (int labels : {0, 1, 7, 1000})
      for (double run : {1.0, 3.0, 40.0, 3000.0}) {
        const Geom g{s[0], s[1], s[2], labels};
        check("random L" + std::to_string(labels) + " run " + std::to_string((int)run), runs(rng, (size_t)s[0] * s[1] * s[2], labels, 0.5, run), g);
      }
  for (int X : {1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193}) {                        // one label through every row: the rows must cut the run
    const Geom g{2, 3, X, 5};
    check("one label, rows of " + std::to_string(X), std::vector<int32_t>((size_t)6 * X, 5), g);
  }
  { const Geom g{1, 2, 1100000, 3}; check("one label fills rows of 1 100 000", std::vector<int32_t>((size_t)2 * 1100000, 3), g); }
  { const Geom g{3, 3, 70000, 1}; check("one label, sum x passes 2^32", std::vector<int32_t>((size_t)9 * 70000, 1), g); }
  { const Geom g{4, 32, 64, 8192};
    std::vector<int32_t> v(8192);
    for (int i = 0; i < 8192; ++i) v[(size_t)i] = 8192 - i;
    check("every voxel its own label", v, g); }
  { const Geom g{5, 40, 100, 9}; check("all background", std::vector<int32_t>(20000, 0), g); }
  { const Geom g{5, 40, 100, 0}; check("n_max = 0 under labels", runs(rng, 20000, 7, 0.3, 9.0), g); }
  { const Geom g{5, 40, 100, 3}; check("labels above n_max = 3", runs(rng, 20000, 7, 0.3, 9.0), g); }
  { const Geom g{1, 90, 100, 4}; check("negative labels only", std::vector<int32_t>(9000, -3), g); }
  { const Geom g{1, 1, 300, 1000}; check("labels of INT32_MAX, n_max 1000", std::vector<int32_t>(300, INT32_MAX), g); }
  if (failures) std::printf("FAILED: %d mismatches\n", failures);
  else std::printf("all cases agree with the per-voxel loop\n");
  return failures ? 1 : 0;
}
