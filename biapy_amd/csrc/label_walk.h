// What the per-label measurements (regionprops.hip, shapeprops.hip, intensityprops.hip) and the overlap table (overlap.hip) share beyond the
// steps of regionprops_core.h / overlap_core.h: the label load, the key policy of a block's table in LDS, the walk of a wave over the runs of
// its span, and the host side's grids and volume checks.  One definition each; a further per-label measurement brings its record and its emit.
// The device parts compile under hipcc only; scripts/label_walk_host.h replays the walk on the host for the check programs.
//
// THE RUN WALK (lw_walk_runs) does not issue one set of atomics per voxel.  The span, trip and head scheme is overlap.hip's: a WAVE owns a
// contiguous SPAN of OVL_SPAN = 8192 voxels and walks it in trips of 256, lane l holding the voxels 4 l .. 4 l + 3 of the trip (one 16-byte load
// where the pointer is 16-byte aligned, four 4-byte loads otherwise - the same voxels either way; the next trip's load is issued before this
// trip is worked on).  A voxel whose label differs from its predecessor's OR that starts a row (x == 0) is a HEAD; four ballots give every lane
// the heads of the whole trip and a head's run length is the distance to the next head.  Every run so lies inside one row and its contribution
// is closed form (regionprops_core.h: rp_apply; shapeprops_core.h: sp_apply_moments).  Only the lanes that hold the head of a labelled run call
// `emit`; background runs are dropped.  The run still open at a trip's end is CARRIED in registers (label, length, head position - uniform over
// the wave) and goes out when a trip brings a head or the span ends.  A lane's (z, y, x) comes from two divisions at the span's start and moves
// on by additions and compares (rp_step, rp_advance).  `emit(label, z, y, x0, L)` receives every finished run of a label > 0 exactly once, from
// one lane; what it does with the run (which record, a block's table first or the global rows) is the caller's, as are the table's clear, the
// barriers and the flush.  The walk is inlined into its kernel with the emit, no call and no dispatch: against the walk written out in each
// kernel it costs no register, no wave per SIMD and no scratch (profiles/kernel_resources.txt).
#pragma once
#include <stdint.h>

#include "regionprops_core.h"

// ---- the host side of an entry point ---------------------------------------------------------------------------------------------------------
// 16 blocks of 256 threads per CU at most for the passes over rows, slots or words
inline unsigned lw_rows_grid(int64_t n) { const int64_t b = (n + 255) / 256; return (unsigned)(b < 4096 ? b : 4096); }
// the blocks of a pass over n voxels in spans: a wave to a span, OVL_WAVES waves to a block
inline unsigned lw_span_blocks(int64_t n) { return (unsigned)(((n + OVL_SPAN - 1) / OVL_SPAN + OVL_WAVES - 1) / OVL_WAVES); }

// the refusals every per-label entry shares, in this order; `fn` names the entry; declares n = Z * Y * X
#define LW_CHECK_VOLUME(fn, Z, Y, X, n_max)                                                                                                       \
  BPX_CHECK((Z) >= 1 && (Y) >= 1 && (X) >= 1, "%s: extents must be at least 1 (got %d x %d x %d)", fn, Z, Y, X);                                  \
  const int64_t n = (int64_t)(Z) * (Y) * (X);                                                                                                     \
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels: volumes of 2^31 voxels or more are not supported", fn, (long long)n);                       \
  BPX_CHECK((n_max) >= 0 && (n_max) < INT32_MAX, "%s: n_max must be in [0, 2^31 - 1) (got %d)", fn, n_max)

#if defined(__HIPCC__)
#include "bpx_common.h"

#define LW_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define LW_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

// ---- the key policy of a block's table in LDS (regionprops_core.h: rp_local_slot); a table derives from it and adds its record's fields ---------
struct LwKeysLds {
  int* keys;
  unsigned* claimed;
  __device__ __forceinline__ int32_t kload(uint32_t s) const { return __hip_atomic_load(keys + s, LW_RLX_WG); }
  __device__ __forceinline__ int32_t kcas(uint32_t s, int32_t label) const {
    int expected = 0;
    __hip_atomic_compare_exchange_strong(keys + s, &expected, (int)label, __ATOMIC_RELAXED, LW_RLX_WG);
    return expected;                                  // the value before, 0 when the exchange took place
  }
  __device__ __forceinline__ uint32_t nclaimed() const { return __hip_atomic_load(claimed, LW_RLX_WG); }
  __device__ __forceinline__ void claim() const { __hip_atomic_fetch_add(claimed, 1u, LW_RLX_WG); }
};

// ---- the label load ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool lw_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// voxels i .. i + 3 of x, those below `end`: one 16-byte load where `vec`, 4-byte loads otherwise and at the end of the span; 0 past the end
__device__ __forceinline__ void lw_load4(const int* __restrict__ x, int64_t i, int64_t end, bool vec, int v[OVL_VPL]) {
  if (i + OVL_VPL <= end) {
    if (vec) {
      const u32x4_t w = *reinterpret_cast<const u32x4_t*>(x + i);
      v[0] = (int)w[0]; v[1] = (int)w[1]; v[2] = (int)w[2]; v[3] = (int)w[3];
    } else {
      v[0] = x[i]; v[1] = x[i + 1]; v[2] = x[i + 2]; v[3] = x[i + 3];
    }
  } else {
#pragma unroll
    for (int e = 0; e < OVL_VPL; ++e) v[e] = (i + e < end) ? x[i + e] : 0;
  }
}

// ---- the run walk: the whole wave, over the voxels [begin, end) of its span.  LOOP BOUND: OVL_SPAN / OVL_TRIP = 32 trips ---------------------------
template <class Emit>
__device__ __forceinline__ void lw_walk_runs(const int* labels, int64_t begin, int64_t end, int lane, int Y, int X, int n_max, RpStride stride,
                                             Emit&& emit) {
  const bool vec = lw_aligned16(labels);                                // spans start at multiples of 8192 voxels: aligned as the pointer is
  RpRun run{RP_NO_LABEL, 0, 0, 0, 0};
  RpPos at = rp_pos_of((uint32_t)(begin + OVL_VPL * lane), Y, X);       // of this lane's first voxel of the trip
  int v[OVL_VPL], nv[OVL_VPL] = {0, 0, 0, 0};
  lw_load4(labels, begin + OVL_VPL * lane, end, vec, v);
  for (int64_t t = begin; t < end; t += OVL_TRIP) {
    const uint32_t valid = (uint32_t)(end - t < OVL_TRIP ? end - t : OVL_TRIP);
    if (t + OVL_TRIP < end) lw_load4(labels, t + OVL_TRIP + OVL_VPL * lane, end, vec, nv);     // on its way while this trip is worked on
    int32_t lab[OVL_VPL];
    RpPos pos[OVL_VPL];
    pos[0] = at;
#pragma unroll
    for (int e = 0; e < OVL_VPL; ++e) {
      lab[e] = rp_label(v[e], n_max);
      if (e) { pos[e] = pos[e - 1]; rp_step(pos[e], Y, X); }
    }
    int32_t prev = __shfl_up(lab[OVL_VPL - 1], 1, OVL_LANES);
    if (lane == 0) prev = run.label;
    uint64_t H[OVL_VPL];
#pragma unroll
    for (int e = 0; e < OVL_VPL; ++e)
      H[e] = __ballot((uint32_t)(OVL_VPL * lane + e) < valid && rp_is_head(lab[e], e ? lab[e - 1] : prev, pos[e].x));
    const bool any = (H[0] | H[1] | H[2] | H[3]) != 0;                  // uniform, as everything derived from H alone
    uint32_t first = 0, last = 0;
    int32_t last_label = 0;
    RpPos last_pos{0, 0, 0};
    if (any) {
      first = ovl_first_head(H);
      last = ovl_last_head(H);
#pragma unroll
      for (int e = 0; e < OVL_VPL; ++e) {
        const uint32_t p = (uint32_t)(OVL_VPL * lane + e);
        if (((H[e] >> lane) & 1) && p != last && lab[e] > 0)            // a labelled run that ends inside the trip: its head's lane sends it
          emit(lab[e], pos[e].z, pos[e].y, pos[e].x, ovl_next_head(H, lane, e, valid) - p);
      }
      const int le = (int)(last & (OVL_VPL - 1)), ll = (int)(last / OVL_VPL);
      const int32_t my_label = le == 0 ? lab[0] : le == 1 ? lab[1] : le == 2 ? lab[2] : lab[3];
      const int32_t my_z = le == 0 ? pos[0].z : le == 1 ? pos[1].z : le == 2 ? pos[2].z : pos[3].z;      // field by field: registers, not addresses
      const int32_t my_y = le == 0 ? pos[0].y : le == 1 ? pos[1].y : le == 2 ? pos[2].y : pos[3].y;
      const int32_t my_x = le == 0 ? pos[0].x : le == 1 ? pos[1].x : le == 2 ? pos[2].x : pos[3].x;
      last_label = __shfl(my_label, ll, OVL_LANES);
      last_pos = RpPos{__shfl(my_z, ll, OVL_LANES), __shfl(my_y, ll, OVL_LANES), __shfl(my_x, ll, OVL_LANES)};
    }
    RpRun done{RP_NO_LABEL, 0, 0, 0, 0};
    if (rp_carry_step(run, done, any, first, last, last_label, last_pos, valid) && lane == 0) emit(done.label, done.z, done.y, done.x0, done.count);
    rp_advance(at, stride, Y, X);
#pragma unroll
    for (int e = 0; e < OVL_VPL; ++e) v[e] = nv[e];
  }
  if (lane == 0 && run.count != 0 && run.label > 0) emit(run.label, run.z, run.y, run.x0, run.count);
}
#endif  // __HIPCC__
