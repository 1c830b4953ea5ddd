// Sparse contingency table of two int32 label volumes on the device: every distinct pair (a[i], b[i]) with the number of voxels that carry it,
// background pairs included (a label <= 0 is background 0, as the markers of the watershed).  What the instance matcher (prepost.matching: IoU,
// F1, panoptic quality against a ground truth) and, later, instance merging across chunk faces start from; the reference fills a dense
// (1 + max_true) x (1 + max_pred) matrix on the host.
//
// THE TABLE (overlap_core.h): open addressing, linear probing, `slots` = the power of two >= 2 * max_pairs; a slot is a 64-bit key a << 32 | b,
// claimed with one 64-bit compare-and-swap, and a 32-bit count raised with integer atomic adds.  A counter of claimed slots decides overflow: with
// more than max_pairs distinct pairs the call writes *num_d = -1 and returns normally (keys_d / counts_d are then unspecified).
// LAUNCHES, fixed by (n, max_pairs): clear (table, counters, keys_d = INT64_MAX, counts_d = 0), count, compact (the occupied slots, in unspecified
// order, to keys_d / counts_d [0, K); *num_d = K or -1).  Nothing is read back, integer atomics only, capturable; every loop is bounded by a launch
// parameter or by the slot count (overlap_core.h), none by what another thread does.
//
// THE COUNT PASS does not issue one atomic per voxel: label volumes are piecewise constant, (0, 0) alone usually covers most of a volume, and one
// add per voxel would send some 10^9 adds to one address at 1024^3.  A WAVE owns a contiguous SPAN of OVL_SPAN = 8192 voxels (the reasoning for the
// length: overlap_core.h) and walks it in trips of 256: lane l holds the voxels 4 l .. 4 l + 3 of the trip (one 16-byte load per input where both
// pointers are 16-byte aligned, four 4-byte loads otherwise - the same voxels either way; the next trip's loads are issued before this trip is
// worked on).  A voxel whose key differs from its predecessor's is a HEAD (the predecessor of a lane's first voxel comes from the lane before it by
// a shuffle, that of the trip's first voxel is the carried run's key); four ballots give every lane the heads of the whole trip, and a head's run
// length is the distance to the next head - found in those masks by bit arithmetic, which is the segmented sum of the equal keys of neighbouring
// lanes without a reduction tree.  Only the lanes that hold a head touch the table.  The run that is still open at the end of a trip is CARRIED in
// registers (key, length - uniform over the wave) into the next trip and goes to the table when a trip brings a head, or at the end of the span:
// a uniform span costs one table update.  THE BLOCK'S OWN TABLE: the four waves of a block send their runs to a table of 512 slots in LDS first
// (the same ovl_insert over an LDS policy); the runs of one object row after row, and the background runs between the objects, meet there instead of
// at one address of the global table.  What the local table does not take goes to the global one directly, and at the end of the block every
// occupied local slot is added to the global table once: an all-background block costs one global add.
// bpx_debug_set_overlap_per_voxel(1) selects the form with one insert per voxel, for scripts/overlap_timing.py only; the same table.
#include "bpx_common.h"
#include "label_walk.h"
#include "overlap_core.h"

namespace {

#define OVL_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct OvlDev {    // relaxed agent-scope accesses (never register-cached), the atomics at the memory side
  unsigned long long* keys;
  unsigned* counts;
  unsigned* claimed;
  __device__ __forceinline__ uint64_t kload(uint32_t s) const { return __hip_atomic_load(keys + s, OVL_RLX_AGENT); }
  __device__ __forceinline__ uint64_t kcas(uint32_t s, uint64_t key) const {
    unsigned long long expected = OVL_EMPTY;
    __hip_atomic_compare_exchange_strong(keys + s, &expected, (unsigned long long)key, __ATOMIC_RELAXED, OVL_RLX_AGENT);
    return expected;                                  // the value before, OVL_EMPTY when the exchange took place
  }
  __device__ __forceinline__ void cadd(uint32_t s, uint32_t c) const { __hip_atomic_fetch_add(counts + s, c, OVL_RLX_AGENT); }
  __device__ __forceinline__ uint32_t nclaimed() const { return __hip_atomic_load(claimed, OVL_RLX_AGENT); }
  __device__ __forceinline__ void claim() const { __hip_atomic_fetch_add(claimed, 1u, OVL_RLX_AGENT); }
};

#define OVL_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

struct OvlLds {    // the block's table in LDS
  unsigned long long* keys;
  unsigned* counts;
  unsigned* claimed;
  __device__ __forceinline__ uint64_t kload(uint32_t s) const { return __hip_atomic_load(keys + s, OVL_RLX_WG); }
  __device__ __forceinline__ uint64_t kcas(uint32_t s, uint64_t key) const {
    unsigned long long expected = OVL_EMPTY;
    __hip_atomic_compare_exchange_strong(keys + s, &expected, (unsigned long long)key, __ATOMIC_RELAXED, OVL_RLX_WG);
    return expected;
  }
  __device__ __forceinline__ void cadd(uint32_t s, uint32_t c) const { __hip_atomic_fetch_add(counts + s, c, OVL_RLX_WG); }
  __device__ __forceinline__ uint32_t nclaimed() const { return __hip_atomic_load(claimed, OVL_RLX_WG); }
  __device__ __forceinline__ void claim() const { __hip_atomic_fetch_add(claimed, 1u, OVL_RLX_WG); }
};

// clear: thread t takes slots t, t + T ... - ceil(slots / T) trips, fixed by the launch
__global__ void __launch_bounds__(256) ovl_clear_kernel(OvlDev m, unsigned* cursor, int64_t slots, int64_t max_pairs, long long* __restrict__ keys_out,
                                                        int* __restrict__ counts_out) {
  for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (int64_t)gridDim.x * 256) {
    m.keys[s] = OVL_EMPTY;
    m.counts[s] = 0;
    if (s < max_pairs) { keys_out[s] = INT64_MAX; counts_out[s] = 0; }      // max_pairs <= slots / 2
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { *m.claimed = 0; *cursor = 0; }
}

// count: wave w of the grid owns the voxels [w * OVL_SPAN, (w + 1) * OVL_SPAN) below n.  LOOP BOUND: OVL_SPAN / OVL_TRIP = 32 trips; the clear and
// the flush of the local table OVL_LOCAL_SLOTS / 256 = 2 trips.  Every wave reaches both barriers, with or without voxels.
__global__ void __launch_bounds__(64 * OVL_WAVES) ovl_count_kernel(OvlDev m, const int* __restrict__ a, const int* __restrict__ b, int64_t n, uint32_t mask,
                                                                   uint32_t max_pairs) {
  __shared__ unsigned long long lkeys[OVL_LOCAL_SLOTS];
  __shared__ unsigned lcounts[OVL_LOCAL_SLOTS];
  __shared__ unsigned lclaimed;
  const OvlLds loc{lkeys, lcounts, &lclaimed};
  for (int s = threadIdx.x; s < OVL_LOCAL_SLOTS; s += 64 * OVL_WAVES) { lkeys[s] = OVL_EMPTY; lcounts[s] = 0; }
  if (threadIdx.x == 0) lclaimed = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t begin = ((int64_t)blockIdx.x * OVL_WAVES + (threadIdx.x >> 6)) * OVL_SPAN;
  if (begin < n) {                                                      // the whole wave
    const int64_t end = begin + OVL_SPAN < n ? begin + OVL_SPAN : n;
    const bool vec = lw_aligned16(a) && lw_aligned16(b);                // spans start at multiples of 8192 voxels: aligned as the pointers are
    OvlRun run{OVL_EMPTY, 0};
    int va[OVL_VPL], vb[OVL_VPL], na[OVL_VPL] = {0, 0, 0, 0}, nb[OVL_VPL] = {0, 0, 0, 0};
    lw_load4(a, begin + OVL_VPL * lane, end, vec, va);
    lw_load4(b, begin + OVL_VPL * lane, end, vec, vb);
    for (int64_t t = begin; t < end; t += OVL_TRIP) {
      const uint32_t valid = (uint32_t)(end - t < OVL_TRIP ? end - t : OVL_TRIP);
      if (t + OVL_TRIP < end) {                                         // the next trip's voxels are on their way while this trip is worked on
        lw_load4(a, t + OVL_TRIP + OVL_VPL * lane, end, vec, na);
        lw_load4(b, t + OVL_TRIP + OVL_VPL * lane, end, vec, nb);
      }
      uint64_t key[OVL_VPL];
#pragma unroll
      for (int e = 0; e < OVL_VPL; ++e) key[e] = ovl_key(va[e], vb[e]);
      uint64_t prev = __shfl_up((unsigned long long)key[OVL_VPL - 1], 1, OVL_LANES);
      if (lane == 0) prev = run.key;
      uint64_t H[OVL_VPL];
#pragma unroll
      for (int e = 0; e < OVL_VPL; ++e)
        H[e] = __ballot((uint32_t)(OVL_VPL * lane + e) < valid && key[e] != (e ? key[e - 1] : prev));
      const bool any = (H[0] | H[1] | H[2] | H[3]) != 0;                // uniform, as everything derived from H alone
      uint32_t first = 0, last = 0;
      uint64_t last_key = 0;
      if (any) {
        first = ovl_first_head(H);
        last = ovl_last_head(H);
#pragma unroll
        for (int e = 0; e < OVL_VPL; ++e) {
          const uint32_t pos = (uint32_t)(OVL_VPL * lane + e);
          if (((H[e] >> lane) & 1) && pos != last)                      // a run that ends inside the trip: its head's lane sends it
            ovl_count(loc, m, key[e], ovl_next_head(H, lane, e, valid) - pos, mask, max_pairs);
        }
        const int le = (int)(last & (OVL_VPL - 1));
        const uint64_t mine = le == 0 ? key[0] : le == 1 ? key[1] : le == 2 ? key[2] : key[3];
        last_key = __shfl((unsigned long long)mine, (int)(last / OVL_VPL), OVL_LANES);
      }
      OvlRun done{OVL_EMPTY, 0};
      if (ovl_carry_step(run, done, any, first, last, last_key, valid) && lane == 0) ovl_count(loc, m, done.key, done.count, mask, max_pairs);
#pragma unroll
      for (int e = 0; e < OVL_VPL; ++e) { va[e] = na[e]; vb[e] = nb[e]; }
    }
    if (lane == 0 && run.count != 0) ovl_count(loc, m, run.key, run.count, mask, max_pairs);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < OVL_LOCAL_SLOTS; s += 64 * OVL_WAVES)   // the flush: every pair of the block once
    if (lkeys[s] != OVL_EMPTY) ovl_insert(m, lkeys[s], lcounts[s], mask, max_pairs);
}

// the timing script's other form: one insert per voxel.  LOOP BOUND: ceil(n / T) trips.
__global__ void __launch_bounds__(256) ovl_count_per_voxel_kernel(OvlDev m, const int* __restrict__ a, const int* __restrict__ b, int64_t n, uint32_t mask,
                                                                  uint32_t max_pairs) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) ovl_insert(m, ovl_key(a[i], b[i]), 1u, mask, max_pairs);
}

// compact: the occupied slots to the front of keys_out / counts_out, one cursor add per wave.  LOOP BOUND: ceil(slots / T) trips, the same for
// every lane of a wave (the bound is rounded up to whole waves, so the ballot always sees all 64 lanes).
__global__ void __launch_bounds__(256) ovl_compact_kernel(OvlDev m, unsigned* cursor, int64_t slots, int64_t max_pairs, long long* __restrict__ keys_out,
                                                          int* __restrict__ counts_out, int* __restrict__ num) {
  const int lane = threadIdx.x & 63;
  const int64_t padded = (slots + 63) / 64 * 64;
  for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < padded; s += (int64_t)gridDim.x * 256) {
    const uint64_t key = s < slots ? (uint64_t)m.keys[s] : OVL_EMPTY;
    const bool full = key != OVL_EMPTY;
    const uint64_t mask = __ballot(full);
    if (mask == 0) continue;
    unsigned base = 0;
    if (lane == 0) base = __hip_atomic_fetch_add(cursor, (unsigned)__builtin_popcountll(mask), OVL_RLX_AGENT);
    base = __shfl(base, 0, OVL_LANES);
    const int64_t pos = (int64_t)base + __builtin_popcountll(mask & (((uint64_t)1 << lane) - 1));
    if (full && pos < max_pairs) {                                      // past max_pairs only on overflow
      keys_out[pos] = (long long)key;
      counts_out[pos] = (int)m.counts[s];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned k = *m.claimed;                                      // final: the count pass has ended
    *num = k > (unsigned)max_pairs ? -1 : (int)k;
  }
}

int g_overlap_per_voxel = 0;   // bpx_debug_set_overlap_per_voxel: 0 (default) = spans, run lengths and the carry; 1 = one insert per voxel; same table

}  // namespace

extern "C" int bpx_debug_set_overlap_per_voxel(int on) { g_overlap_per_voxel = on ? 1 : 0; return 0; }

extern "C" int64_t bpx_overlap_workspace(int64_t max_pairs) {
  const int64_t slots = ovl_slots(max_pairs);
  if (slots < 1) return -1;
  return slots * 12 + 16;                                               // keys, counts, the counter of claimed slots and the compact cursor
}

extern "C" int bpx_label_overlap(const int32_t* a_d, const int32_t* b_d, int64_t n, int64_t max_pairs, int64_t* keys_d, int32_t* counts_d,
                                 int32_t* num_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  const char* fn = "bpx_label_overlap";
  BPX_CHECK(a_d && b_d && keys_d && counts_d && num_d && ws_d, "%s: null pointer", fn);
  BPX_CHECK(n >= 1, "%s: n must be at least 1 (got %lld)", fn, (long long)n);
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels: volumes of 2^31 voxels or more are not supported (int32 counts)", fn, (long long)n);
  BPX_CHECK(max_pairs >= 1, "%s: max_pairs must be at least 1 (got %lld)", fn, (long long)max_pairs);
  const int64_t need = bpx_overlap_workspace(max_pairs);
  BPX_CHECK(need > 0, "%s: max_pairs %lld is refused: the table would pass 2^31 slots", fn, (long long)max_pairs);
  BPX_CHECK(ws_bytes >= need, "%s: workspace too small (%lld bytes, bpx_overlap_workspace says %lld)", fn, (long long)ws_bytes, (long long)need);
  BPX_CHECK((((uintptr_t)a_d | (uintptr_t)b_d | (uintptr_t)counts_d | (uintptr_t)num_d) & 3) == 0 && (((uintptr_t)keys_d | (uintptr_t)ws_d) & 7) == 0,
            "%s: a, b, counts and num must be 4-byte aligned, keys and the workspace 8-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  const int64_t slots = ovl_slots(max_pairs);
  unsigned long long* tkeys = reinterpret_cast<unsigned long long*>(ws_d);
  unsigned* tcounts = reinterpret_cast<unsigned*>(tkeys + slots);
  unsigned* claimed = tcounts + slots;
  unsigned* cursor = claimed + 1;
  const OvlDev m{tkeys, tcounts, claimed};
  const uint32_t mask = (uint32_t)(slots - 1), mp = (uint32_t)max_pairs;
  long long* keys_out = reinterpret_cast<long long*>(keys_d);
  ovl_clear_kernel<<<lw_rows_grid(slots), 256, 0, s>>>(m, cursor, slots, max_pairs, keys_out, counts_d);
  if (g_overlap_per_voxel) ovl_count_per_voxel_kernel<<<lw_rows_grid(n), 256, 0, s>>>(m, a_d, b_d, n, mask, mp);
  else ovl_count_kernel<<<lw_span_blocks(n), 64 * OVL_WAVES, 0, s>>>(m, a_d, b_d, n, mask, mp);
  ovl_compact_kernel<<<lw_rows_grid(slots), 256, 0, s>>>(m, cursor, slots, max_pairs, keys_out, counts_d, num_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
