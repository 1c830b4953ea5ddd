// Region properties of an int32 label volume (Z, Y, X) on the device: for every label l in 1..n_max its voxel count (area), the sums of its
// voxels' coordinates (exact int64; the centroid is their quotient) and its half-open bounding box - scikit-image's regionprops area / bbox /
// centroid, scipy.ndimage's find_objects / center_of_mass.  What the detection workflow (centroids of the labelled blobs) and the instance
// workflow (measure every instance, drop those that fail a property test) take next after label() / watershed(); the reference copies the label
// volume to the host for it.
//
// LAUNCHES, fixed by (Z, Y, X, n_max): init (area and sums 0, box minima INT32_MAX, maxima -1), accumulate, finish (maxima made exclusive; row 0
// and the labels no voxel carries all zeros).  The outputs are the accumulators: no workspace.  Integer atomics only (uint32 / uint64 add, int32
// min / max, relaxed, agent scope): the same bits every run.  Nothing is read back, capturable; every loop is bounded by a launch parameter or a
// constant of regionprops_core.h, none by what another thread does.
//
// THE ACCUMULATE PASS does not issue one set of atomics per voxel.  The span, trip and head scheme is overlap.hip's: a WAVE owns a contiguous
// SPAN of OVL_SPAN = 8192 voxels and walks it in trips of 256, lane l holding the voxels 4 l .. 4 l + 3 of the trip (one 16-byte load where the
// pointer is 16-byte aligned, four 4-byte loads otherwise - the same voxels either way; the next trip's load is issued before this trip is worked
// on).  A voxel whose label differs from its predecessor's OR that starts a row (x == 0) is a HEAD; four ballots give every lane the heads of the
// whole trip and a head's run length is the distance to the next head.  Every run so lies inside one row and its contribution is closed form
// (regionprops_core.h: rp_apply): area += L, sum z += L z, sum y += L y, sum x += L x0 + L (L - 1) / 2, box min= (z, y, x0), max= (z, y, x0 + L - 1).
// Only the lanes that hold the head of a labelled run touch memory; background runs are dropped.  The run still open at a trip's end is
// CARRIED in registers (label, length, head position - uniform over the wave) and goes out when a trip brings a head or the span ends.
// A lane's (z, y, x) comes from two divisions at the span's start and moves on by additions and compares (rp_step, rp_advance).
// TWO FORMS, the same bits: (a) every finished run goes straight to the global per-label arrays; (b) the block's four waves first merge their runs
// in a table of RP_LOCAL_SLOTS = 256 records keyed by label in LDS - 14 340 bytes, eleven blocks per CU by LDS where the 32 waves of a CU allow
// eight, so LDS does not limit the occupancy (the registers do: 74 VGPRs, 6 waves per SIMD; form (a) 66 VGPRs, 7 waves; 512 slots, 28 676 bytes,
// would allow five) - which is merged into the global arrays once per occupied slot at the block's end; what the table does not take goes to
// global directly.  Form (b) is the default: on labelled volumes the runs of one object meet in LDS instead of at the object's one global
// record (balls at 1024^3: 2.34 ms against 221 ms; a mask with one component through the whole volume: 9.0 ms against 3.7 s).  Form (a) stays selectable because it wins
// on one measured input, the volume without labels (no table to clear and flush: 8 % at 1024^3).  bpx_debug_set_regionprops_local picks the
// form (environment: BPX_REGIONPROPS_LOCAL); figures: profiles/regionprops_timing.json, DESIGN.md section 4.
#include <algorithm>

#include "bpx_common.h"
#include "regionprops_core.h"

namespace {

#define RP_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define RP_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

struct RpDev {     // the global per-label arrays, the atomics at the memory side
  unsigned* area_p;
  unsigned long long* sums_p;
  int* box_p;
  __device__ __forceinline__ void area(uint32_t r, uint32_t c) const { __hip_atomic_fetch_add(area_p + r, c, RP_RLX_AGENT); }
  __device__ __forceinline__ void sum(uint32_t r, int k, uint64_t v) const {
    __hip_atomic_fetch_add(sums_p + (int64_t)r * 3 + k, (unsigned long long)v, RP_RLX_AGENT);
  }
  __device__ __forceinline__ void lo(uint32_t r, int k, int32_t v) const { __hip_atomic_fetch_min(box_p + (int64_t)r * 6 + k, v, RP_RLX_AGENT); }
  __device__ __forceinline__ void hi(uint32_t r, int k, int32_t v) const { __hip_atomic_fetch_max(box_p + (int64_t)r * 6 + 3 + k, v, RP_RLX_AGENT); }
};

struct RpLds {     // the block's table in LDS
  int* keys;
  unsigned* area_p;
  unsigned long long* sums_p;
  int* box_p;
  unsigned* claimed;
  __device__ __forceinline__ int32_t kload(uint32_t s) const { return __hip_atomic_load(keys + s, RP_RLX_WG); }
  __device__ __forceinline__ int32_t kcas(uint32_t s, int32_t label) const {
    int expected = 0;
    __hip_atomic_compare_exchange_strong(keys + s, &expected, (int)label, __ATOMIC_RELAXED, RP_RLX_WG);
    return expected;                                  // the value before, 0 when the exchange took place
  }
  __device__ __forceinline__ uint32_t nclaimed() const { return __hip_atomic_load(claimed, RP_RLX_WG); }
  __device__ __forceinline__ void claim() const { __hip_atomic_fetch_add(claimed, 1u, RP_RLX_WG); }
  __device__ __forceinline__ void area(uint32_t s, uint32_t c) const { __hip_atomic_fetch_add(area_p + s, c, RP_RLX_WG); }
  __device__ __forceinline__ void sum(uint32_t s, int k, uint64_t v) const { __hip_atomic_fetch_add(sums_p + s * 3 + k, (unsigned long long)v, RP_RLX_WG); }
  __device__ __forceinline__ void lo(uint32_t s, int k, int32_t v) const { __hip_atomic_fetch_min(box_p + s * 6 + k, v, RP_RLX_WG); }
  __device__ __forceinline__ void hi(uint32_t s, int k, int32_t v) const { __hip_atomic_fetch_max(box_p + s * 6 + 3 + k, v, RP_RLX_WG); }
  __device__ __forceinline__ uint32_t area_of(uint32_t s) const { return area_p[s]; }
  __device__ __forceinline__ uint64_t sum_of(uint32_t s, int k) const { return sums_p[s * 3 + k]; }
  __device__ __forceinline__ int32_t lo_of(uint32_t s, int k) const { return box_p[s * 6 + k]; }
  __device__ __forceinline__ int32_t hi_of(uint32_t s, int k) const { return box_p[s * 6 + 3 + k]; }
};

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// voxels i .. i + 3 of x, those below `end`: one 16-byte load where x allows it, 4-byte loads otherwise and at the end of the span; 0 past the end
__device__ __forceinline__ void load4(const int* __restrict__ x, int64_t i, int64_t end, bool vec, int v[OVL_VPL]) {
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

// init / finish: thread t takes the rows t, t + T ...  LOOP BOUND: ceil(rows / T) trips, fixed by the launch
__global__ void __launch_bounds__(256) rp_init_kernel(int* __restrict__ area, int64_t* __restrict__ sums, int* __restrict__ box, int64_t rows) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256)
    rp_init_row(area + r, sums + r * 3, box + r * 6);
}
__global__ void __launch_bounds__(256) rp_finish_kernel(int* __restrict__ area, int64_t* __restrict__ sums, int* __restrict__ box, int64_t rows) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256)
    rp_finish_row(r, area + r, sums + r * 3, box + r * 6);
}

// accumulate: wave w of the grid owns the voxels [w * OVL_SPAN, (w + 1) * OVL_SPAN) below n.  LOOP BOUND: OVL_SPAN / OVL_TRIP = 32 trips; with
// LOCAL the clear and the flush of the block's table RP_LOCAL_SLOTS / 256 = 1 trip.  Every wave reaches both barriers, with or without voxels.
template <bool LOCAL>
__global__ void __launch_bounds__(64 * OVL_WAVES) rp_accumulate_kernel(RpDev m, const int* __restrict__ labels, int64_t n, int Y, int X, int n_max,
                                                                       RpStride stride) {
  __shared__ int lkeys[LOCAL ? RP_LOCAL_SLOTS : 1];
  __shared__ unsigned larea[LOCAL ? RP_LOCAL_SLOTS : 1];
  __shared__ unsigned long long lsums[LOCAL ? RP_LOCAL_SLOTS * 3 : 1];
  __shared__ int lbox[LOCAL ? RP_LOCAL_SLOTS * 6 : 1];
  __shared__ unsigned lclaimed;
  const RpLds loc{lkeys, larea, lsums, lbox, &lclaimed};
  if constexpr (LOCAL) {
    for (int s = threadIdx.x; s < RP_LOCAL_SLOTS; s += 64 * OVL_WAVES) {
      lkeys[s] = 0;
      larea[s] = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) { lsums[s * 3 + k] = 0; lbox[s * 6 + k] = RP_LO_INIT; lbox[s * 6 + 3 + k] = RP_HI_INIT; }
    }
    if (threadIdx.x == 0) lclaimed = 0;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int64_t begin = ((int64_t)blockIdx.x * OVL_WAVES + (threadIdx.x >> 6)) * OVL_SPAN;
  if (begin < n) {                                                      // the whole wave
    const int64_t end = begin + OVL_SPAN < n ? begin + OVL_SPAN : n;
    const bool vec = aligned16(labels);                                 // spans start at multiples of 8192 voxels: aligned as the pointer is
    auto emit = [&](int32_t label, int32_t z, int32_t y, int32_t x0, uint32_t L) {
      if constexpr (LOCAL) rp_emit(loc, m, label, z, y, x0, L);
      else rp_emit(m, label, z, y, x0, L);
    };
    RpRun run{RP_NO_LABEL, 0, 0, 0, 0};
    RpPos at = rp_pos_of((uint32_t)(begin + OVL_VPL * lane), Y, X);     // of this lane's first voxel of the trip
    int v[OVL_VPL], nv[OVL_VPL] = {0, 0, 0, 0};
    load4(labels, begin + OVL_VPL * lane, end, vec, v);
    for (int64_t t = begin; t < end; t += OVL_TRIP) {
      const uint32_t valid = (uint32_t)(end - t < OVL_TRIP ? end - t : OVL_TRIP);
      if (t + OVL_TRIP < end) load4(labels, t + OVL_TRIP + OVL_VPL * lane, end, vec, nv);     // on its way while this trip is worked on
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
      const bool any = (H[0] | H[1] | H[2] | H[3]) != 0;                // uniform, as everything derived from H alone
      uint32_t first = 0, last = 0;
      int32_t last_label = 0;
      RpPos last_pos{0, 0, 0};
      if (any) {
        first = ovl_first_head(H);
        last = ovl_last_head(H);
#pragma unroll
        for (int e = 0; e < OVL_VPL; ++e) {
          const uint32_t p = (uint32_t)(OVL_VPL * lane + e);
          if (((H[e] >> lane) & 1) && p != last && lab[e] > 0)          // a labelled run that ends inside the trip: its head's lane sends it
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
  if constexpr (LOCAL) {
    __syncthreads();
    for (int s = threadIdx.x; s < RP_LOCAL_SLOTS; s += 64 * OVL_WAVES) rp_merge(loc, (uint32_t)s, m);   // the flush: every label of the block once
  }
}

constexpr int RP_DEFAULT_LOCAL = 1;
int g_regionprops_local = RP_DEFAULT_LOCAL;   // bpx_debug_set_regionprops_local: 1 = form (b), the block's table in LDS first; 0 = form (a), every run to global; same bits

// 16 blocks of 256 threads per CU at most for the passes over the rows (as overlap.hip's grid_of)
unsigned grid_of(int64_t n) { return (unsigned)std::min<int64_t>(cdiv64(n, 256), 4096); }

}  // namespace

extern "C" int bpx_debug_set_regionprops_local(int on) { g_regionprops_local = on < 0 ? RP_DEFAULT_LOCAL : on ? 1 : 0; return 0; }   // negative: back to the default

extern "C" int bpx_region_props(const int32_t* labels_d, int Z, int Y, int X, int n_max, int32_t* area_d, int64_t* sums_d, int32_t* bbox_d,
                                bpx_stream_t stream) {
  const char* fn = "bpx_region_props";
  BPX_CHECK(labels_d && area_d && sums_d && bbox_d, "%s: null pointer", fn);
  BPX_CHECK(Z >= 1 && Y >= 1 && X >= 1, "%s: extents must be at least 1 (got %d x %d x %d)", fn, Z, Y, X);
  const int64_t n = (int64_t)Z * Y * X;
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels: volumes of 2^31 voxels or more are not supported", fn, (long long)n);
  BPX_CHECK(n_max >= 0 && n_max < INT32_MAX, "%s: n_max must be in [0, 2^31 - 1) (got %d)", fn, n_max);
  BPX_CHECK((((uintptr_t)labels_d | (uintptr_t)area_d | (uintptr_t)bbox_d) & 3) == 0 && ((uintptr_t)sums_d & 7) == 0,
            "%s: labels, area and bbox must be 4-byte aligned, sums 8-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)n_max + 1;
  const RpDev m{reinterpret_cast<unsigned*>(area_d), reinterpret_cast<unsigned long long*>(sums_d), bbox_d};
  const unsigned blocks = (unsigned)cdiv64(cdiv64(n, OVL_SPAN), OVL_WAVES);
  rp_init_kernel<<<grid_of(rows), 256, 0, s>>>(area_d, sums_d, bbox_d, rows);
  if (g_regionprops_local) rp_accumulate_kernel<true><<<blocks, 64 * OVL_WAVES, 0, s>>>(m, labels_d, n, Y, X, n_max, rp_stride(Y, X));
  else rp_accumulate_kernel<false><<<blocks, 64 * OVL_WAVES, 0, s>>>(m, labels_d, n, Y, X, n_max, rp_stride(Y, X));
  rp_finish_kernel<<<grid_of(rows), 256, 0, s>>>(area_d, sums_d, bbox_d, rows);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
