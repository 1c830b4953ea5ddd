// Host run of the label-overlap table of biapy_amd/csrc/overlap.hip: the same steps (csrc/overlap_core.h: key, hash, bounded insert, the heads of a
// trip and their run lengths, the carry step, the local-then-global count) in the launch sequence of bpx_label_overlap - clear; count over spans
// of `span` voxels walked in trips of 256 by a "wave" of 64 lanes, four waves to a block with its own small table that is flushed into the global
// one; compact - sequentially and with the blocks and their waves spread over std::threads on std::atomic, checked against a std::map
// count.  The wave's shuffle and ballots are plain loops here; everything that decides a run length or touches the table is the shared code.
// Cases: random label volumes (runs of geometric length), all background, all distinct pairs, spans that end one voxel before, on and after a key
// change, max_pairs exactly K, overflow (num = -1, nothing written outside the buffers: the sanitizers watch).  Spans of OVL_SPAN and, to meet many
// span ends in small volumes, of 256 and 512.  A development aid for finding an off-by-one at a trip or span end, an unbounded probe loop or a
// wrong overflow decision before the kernels run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -I biapy_amd/csrc scripts/overlap_cpu_check.cpp -o overlap_cpu_check
//   ./overlap_cpu_check
// Prints one line per case and exits nonzero on the first mismatch.  Not loaded into Python, not part of the test suite.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <functional>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "overlap_core.h"

struct HostMem {
  std::atomic<uint64_t>* keys;
  std::atomic<uint32_t>* counts;
  std::atomic<uint32_t>* claimed;
  uint64_t kload(uint32_t s) const { return keys[s].load(std::memory_order_relaxed); }
  uint64_t kcas(uint32_t s, uint64_t key) const {
    uint64_t expected = OVL_EMPTY;
    keys[s].compare_exchange_strong(expected, key, std::memory_order_relaxed);
    return expected;
  }
  void cadd(uint32_t s, uint32_t c) const { counts[s].fetch_add(c, std::memory_order_relaxed); }
  uint32_t nclaimed() const { return claimed->load(std::memory_order_relaxed); }
  void claim() const { claimed->fetch_add(1, std::memory_order_relaxed); }
};

static void parallel_for(int threads, int64_t count, const std::function<void(int64_t)>& f) {   // item q runs on thread q % threads: neighbouring spans on different threads
  if (threads <= 1) { for (int64_t q = 0; q < count; ++q) f(q); return; }
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([=, &f] { for (int64_t q = t; q < count; q += threads) f(q); });
  for (auto& th : pool) th.join();
}

// one wave's span [begin, end): ovl_count_kernel, step for step
static void count_span(const HostMem& loc, const HostMem& m, const std::vector<int32_t>& a, const std::vector<int32_t>& b, int64_t begin, int64_t end, uint32_t mask, uint32_t max_pairs) {
  OvlRun run{OVL_EMPTY, 0};
  for (int64_t t = begin; t < end; t += OVL_TRIP) {
    const uint32_t valid = (uint32_t)std::min<int64_t>(OVL_TRIP, end - t);
    uint64_t key[OVL_LANES][OVL_VPL];
    for (int l = 0; l < OVL_LANES; ++l)
      for (int e = 0; e < OVL_VPL; ++e) {
        const int64_t i = t + OVL_VPL * l + e;
        key[l][e] = i < end ? ovl_key(a[(size_t)i], b[(size_t)i]) : ovl_key(0, 0);      // lw_load4: 0 past the end
      }
    uint64_t H[OVL_VPL] = {0, 0, 0, 0};
    for (int l = 0; l < OVL_LANES; ++l)
      for (int e = 0; e < OVL_VPL; ++e) {
        const uint64_t prev = e ? key[l][e - 1] : l ? key[l - 1][OVL_VPL - 1] : run.key;
        if ((uint32_t)(OVL_VPL * l + e) < valid && key[l][e] != prev) H[e] |= (uint64_t)1 << l;
      }
    const bool any = (H[0] | H[1] | H[2] | H[3]) != 0;
    uint32_t first = 0, last = 0;
    uint64_t last_key = 0;
    if (any) {
      first = ovl_first_head(H);
      last = ovl_last_head(H);
      for (int l = 0; l < OVL_LANES; ++l)
        for (int e = 0; e < OVL_VPL; ++e) {
          const uint32_t pos = (uint32_t)(OVL_VPL * l + e);
          if (((H[e] >> l) & 1) && pos != last) ovl_count(loc, m, key[l][e], ovl_next_head(H, l, e, valid) - pos, mask, max_pairs);
        }
      last_key = key[last / OVL_VPL][last % OVL_VPL];
    }
    OvlRun done{OVL_EMPTY, 0};
    if (ovl_carry_step(run, done, any, first, last, last_key, valid)) ovl_count(loc, m, done.key, done.count, mask, max_pairs);
  }
  if (run.count != 0) ovl_count(loc, m, run.key, run.count, mask, max_pairs);
}

struct Result { int num; std::map<uint64_t, uint32_t> table; bool filler_ok; };

// the launch sequence of bpx_label_overlap; `span` = OVL_SPAN on the device
static Result overlap_host(const std::vector<int32_t>& a, const std::vector<int32_t>& b, int64_t max_pairs, int64_t span, int threads) {
  const int64_t n = (int64_t)a.size(), slots = ovl_slots(max_pairs);
  std::unique_ptr<std::atomic<uint64_t>[]> keys(new std::atomic<uint64_t>[(size_t)slots]);
  std::unique_ptr<std::atomic<uint32_t>[]> counts(new std::atomic<uint32_t>[(size_t)slots]);
  std::atomic<uint32_t> claimed{0};
  std::vector<int64_t> keys_out((size_t)max_pairs, 0);       // exactly max_pairs entries: a write past them is the sanitizer's
  std::vector<int32_t> counts_out((size_t)max_pairs, -7);
  const HostMem m{keys.get(), counts.get(), &claimed};
  for (int64_t s = 0; s < slots; ++s) {                                                  // clear
    keys[(size_t)s].store(OVL_EMPTY);
    counts[(size_t)s].store(0);
    if (s < max_pairs) { keys_out[(size_t)s] = INT64_MAX; counts_out[(size_t)s] = 0; }
  }
  const uint32_t mask = (uint32_t)(slots - 1);
  const int64_t spans = (n + span - 1) / span;
  parallel_for(threads, (spans + OVL_WAVES - 1) / OVL_WAVES, [&](int64_t blk) {          // a block: its own table, OVL_WAVES spans, the flush
    std::unique_ptr<std::atomic<uint64_t>[]> lkeys(new std::atomic<uint64_t>[OVL_LOCAL_SLOTS]);
    std::unique_ptr<std::atomic<uint32_t>[]> lcounts(new std::atomic<uint32_t>[OVL_LOCAL_SLOTS]);
    std::atomic<uint32_t> lclaimed{0};
    for (int s = 0; s < OVL_LOCAL_SLOTS; ++s) { lkeys[(size_t)s].store(OVL_EMPTY); lcounts[(size_t)s].store(0); }
    const HostMem loc{lkeys.get(), lcounts.get(), &lclaimed};
    parallel_for(threads > 1 ? 2 : 1, OVL_WAVES, [&](int64_t w) {
      const int64_t begin = (blk * OVL_WAVES + w) * span;
      if (begin < n) count_span(loc, m, a, b, begin, std::min(n, begin + span), mask, (uint32_t)max_pairs);
    });
    for (int s = 0; s < OVL_LOCAL_SLOTS; ++s)
      if (lkeys[(size_t)s].load() != OVL_EMPTY) ovl_insert(m, lkeys[(size_t)s].load(), lcounts[(size_t)s].load(), mask, (uint32_t)max_pairs);
  });
  int64_t cursor = 0;                                                                    // compact
  for (int64_t s = 0; s < slots; ++s) {
    const uint64_t k = keys[(size_t)s].load();
    if (k == OVL_EMPTY) continue;
    const int64_t pos = cursor++;
    if (pos < max_pairs) { keys_out[(size_t)pos] = (int64_t)k; counts_out[(size_t)pos] = (int32_t)counts[(size_t)s].load(); }
  }
  Result r;
  r.num = claimed.load() > (uint32_t)max_pairs ? -1 : (int)claimed.load();
  r.filler_ok = true;
  if (r.num >= 0) {
    if (cursor != r.num) r.filler_ok = false;                                            // the counter is the number of occupied slots
    for (int64_t k = 0; k < max_pairs; ++k) {
      if (k < r.num) r.table[(uint64_t)keys_out[(size_t)k]] += (uint32_t)counts_out[(size_t)k];
      else if (keys_out[(size_t)k] != INT64_MAX || counts_out[(size_t)k] != 0) r.filler_ok = false;
    }
    if ((int64_t)r.table.size() != r.num) r.filler_ok = false;                           // no key twice
  }
  return r;
}

static int failures = 0;

static void check(const std::string& name, const std::vector<int32_t>& a, const std::vector<int32_t>& b, int64_t max_pairs) {
  std::map<uint64_t, uint32_t> want;
  for (size_t i = 0; i < a.size(); ++i) ++want[ovl_key(a[i], b[i])];
  const int K = (int64_t)want.size() > max_pairs ? -1 : (int)want.size();
  for (int64_t span : {(int64_t)OVL_SPAN, (int64_t)256, (int64_t)512})
    for (int threads : {1, 4}) {
      const Result r = overlap_host(a, b, max_pairs, span, threads);
      if (r.num != K || !r.filler_ok || (K >= 0 && r.table != want)) {
        ++failures;
        std::printf("MISMATCH %s span %lld threads %d: num %d, want %d\n", name.c_str(), (long long)span, threads, r.num, K);
      }
    }
  std::printf("%-44s n %7zu  max_pairs %7lld  K %6zu  num %d\n", name.c_str(), a.size(), (long long)max_pairs, want.size(), K);
}

// labels in runs of geometric length: `labels` ids (0 = background with weight `bg`), some negative
static std::vector<int32_t> runs(std::mt19937& rng, size_t n, int labels, double bg, double mean_run) {
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  std::vector<int32_t> v(n);
  int32_t cur = 0;
  for (size_t i = 0; i < n; ++i) {
    if (i == 0 || uni(rng) < 1.0 / mean_run) {
      const double u = uni(rng);
      cur = u < bg ? (uni(rng) < 0.3 ? -(int32_t)(1 + uni(rng) * 5) : 0) : labels ? 1 + (int32_t)(uni(rng) * labels) : 0;
    }
    v[i] = cur;
  }
  return v;
}

int main() {
  std::mt19937 rng(0);
  for (size_t n : {(size_t)1, (size_t)7, (size_t)255, (size_t)256, (size_t)257, (size_t)300, (size_t)6993, (size_t)8191, (size_t)8192, (size_t)8193, (size_t)40000})
    for (int labels : {0, 1, 7, 1000})
      for (double run : {1.0, 3.0, 40.0, 3000.0}) {
        const auto a = runs(rng, n, labels, 0.6, run), b = runs(rng, n, labels, 0.5, run * 1.7);
        check("random L" + std::to_string(labels) + " run " + std::to_string((int)run), a, b, (int64_t)std::min<size_t>(n, 1 << 21));
      }
  { std::vector<int32_t> z(20000, 0); check("all background", z, z, 20000); check("all background, max_pairs 1", z, z, 1); }
  { std::vector<int32_t> a(20000, 5), b(20000, 9); check("one uniform positive pair", a, b, 1); }
  { std::vector<int32_t> a(9000, -3), b(9000, INT32_MIN); check("negative labels only", a, b, 4); }
  { std::vector<int32_t> a(300, INT32_MAX), b(300, INT32_MAX); check("the largest key", a, b, 2); }
  { const int n = 8192;
    std::vector<int32_t> a(n), b(n);
    for (int i = 0; i < n; ++i) { a[i] = 1 + i; b[i] = n - i; }
    check("all distinct, max_pairs n", a, b, n);
    a.resize(100); b.resize(100);
    check("all distinct, max_pairs K = 100", a, b, 100);
    check("overflow: 100 pairs, max_pairs 16", a, b, 16);
    check("overflow: 100 pairs, max_pairs 99", a, b, 99);
    check("overflow: 100 pairs, max_pairs 1", a, b, 1); }
  // a key change one voxel before, on and after the end of a span (256, 512, OVL_SPAN) and of a trip
  for (int64_t edge : {(int64_t)256, (int64_t)512, (int64_t)OVL_SPAN, (int64_t)2 * OVL_SPAN})
    for (int d = -1; d <= 1; ++d)
      for (int64_t n : {edge + d, edge + d + 1, edge + 300, 3 * edge}) {
        if (n <= edge + d) continue;
        std::vector<int32_t> a((size_t)n, 3), b((size_t)n, 0);
        for (int64_t i = edge + d; i < n; ++i) { a[(size_t)i] = 4; b[(size_t)i] = 2; }
        check("change at " + std::to_string(edge) + (d < 0 ? " - 1" : d ? " + 1" : ""), a, b, 2);
      }
  { std::vector<int32_t> a, b;                  // K exactly max_pairs, with repeats: 37 pairs, each many times, in runs and scattered
    for (int r = 0; r < 500; ++r) for (int k = 0; k < 37; ++k) for (int q = 0; q < 1 + (r + k) % 5; ++q) { a.push_back(k % 7); b.push_back(k); }
    check("K = max_pairs = 37 with repeats", a, b, 37);
    check("overflow by one: max_pairs 36", a, b, 36); }
  { const size_t n = 100000;                    // overflow with a table that fills completely: the probe loop's bound
    std::vector<int32_t> a(n), b(n);
    for (size_t i = 0; i < n; ++i) { a[i] = (int32_t)(i % 1000); b[i] = (int32_t)(i / 1000); }
    check("overflow: 10^5 pairs, max_pairs 5", a, b, 5); }
  if (failures) std::printf("FAILED: %d mismatches\n", failures);
  else std::printf("all cases agree with the std::map count\n");
  return failures ? 1 : 0;
}
