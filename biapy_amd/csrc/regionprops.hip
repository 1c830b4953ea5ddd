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
// THE ACCUMULATE PASS does not issue one set of atomics per voxel: a wave walks the runs of its span of OVL_SPAN = 8192 voxels (label_walk.h:
// lw_walk_runs, where the span, trip, head and carry scheme is written up; shapeprops.hip's moments pass is the same walk with another emit) and
// every finished run of a label contributes in closed form (regionprops_core.h: rp_apply): area += L, sum z += L z, sum y += L y,
// sum x += L x0 + L (L - 1) / 2, box min= (z, y, x0), max= (z, y, x0 + L - 1).
// TWO FORMS, the same bits: (a) every finished run goes straight to the global per-label arrays; (b) the block's four waves first merge their runs
// in a table of RP_LOCAL_SLOTS = 256 records keyed by label in LDS - 14 340 bytes, eleven blocks per CU by LDS where the 32 waves of a CU allow
// eight, so LDS does not limit the occupancy (the registers do: 72 VGPRs, 7 waves per SIMD; form (a) 64 VGPRs, 8 waves; 512 slots, 28 676 bytes,
// would allow five) - which is merged into the global arrays once per occupied slot at the block's end; what the table does not take goes to
// global directly.  Form (b) is the default: on labelled volumes the runs of one object meet in LDS instead of at the object's one global
// record (balls at 1024^3: 2.34 ms against 221 ms; a mask with one component through the whole volume: 9.0 ms against 3.7 s).  Form (a) stays selectable because it wins
// on one measured input, the volume without labels (no table to clear and flush: 8 % at 1024^3).  bpx_debug_set_regionprops_local picks the
// form (environment: BPX_REGIONPROPS_LOCAL); figures: profiles/regionprops_timing.json, DESIGN.md section 4.
#include "bpx_common.h"
#include "label_walk.h"
#include "regionprops_core.h"

namespace {

struct RpDev {     // the global per-label arrays, the atomics at the memory side
  unsigned* area_p;
  unsigned long long* sums_p;
  int* box_p;
  __device__ __forceinline__ void area(uint32_t r, uint32_t c) const { __hip_atomic_fetch_add(area_p + r, c, LW_RLX_AGENT); }
  __device__ __forceinline__ void sum(uint32_t r, int k, uint64_t v) const {
    __hip_atomic_fetch_add(sums_p + (int64_t)r * 3 + k, (unsigned long long)v, LW_RLX_AGENT);
  }
  __device__ __forceinline__ void lo(uint32_t r, int k, int32_t v) const { __hip_atomic_fetch_min(box_p + (int64_t)r * 6 + k, v, LW_RLX_AGENT); }
  __device__ __forceinline__ void hi(uint32_t r, int k, int32_t v) const { __hip_atomic_fetch_max(box_p + (int64_t)r * 6 + 3 + k, v, LW_RLX_AGENT); }
};

struct RpLds : LwKeysLds {     // the block's table in LDS
  unsigned* area_p;
  unsigned long long* sums_p;
  int* box_p;
  __device__ __forceinline__ void area(uint32_t s, uint32_t c) const { __hip_atomic_fetch_add(area_p + s, c, LW_RLX_WG); }
  __device__ __forceinline__ void sum(uint32_t s, int k, uint64_t v) const { __hip_atomic_fetch_add(sums_p + s * 3 + k, (unsigned long long)v, LW_RLX_WG); }
  __device__ __forceinline__ void lo(uint32_t s, int k, int32_t v) const { __hip_atomic_fetch_min(box_p + s * 6 + k, v, LW_RLX_WG); }
  __device__ __forceinline__ void hi(uint32_t s, int k, int32_t v) const { __hip_atomic_fetch_max(box_p + s * 6 + 3 + k, v, LW_RLX_WG); }
  __device__ __forceinline__ uint32_t area_of(uint32_t s) const { return area_p[s]; }
  __device__ __forceinline__ uint64_t sum_of(uint32_t s, int k) const { return sums_p[s * 3 + k]; }
  __device__ __forceinline__ int32_t lo_of(uint32_t s, int k) const { return box_p[s * 6 + k]; }
  __device__ __forceinline__ int32_t hi_of(uint32_t s, int k) const { return box_p[s * 6 + 3 + k]; }
};

// init / finish: thread t takes the rows t, t + T ...  LOOP BOUND: ceil(rows / T) trips, fixed by the launch
__global__ void __launch_bounds__(256) rp_init_kernel(int* __restrict__ area, int64_t* __restrict__ sums, int* __restrict__ box, int64_t rows) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256)
    rp_init_row(area + r, sums + r * 3, box + r * 6);
}
__global__ void __launch_bounds__(256) rp_finish_kernel(int* __restrict__ area, int64_t* __restrict__ sums, int* __restrict__ box, int64_t rows) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256)
    rp_finish_row(r, area + r, sums + r * 3, box + r * 6);
}

// accumulate: wave w of the grid owns the voxels [w * OVL_SPAN, (w + 1) * OVL_SPAN) below n and walks their runs (label_walk.h: lw_walk_runs,
// 32 trips).  LOOP BOUND: with LOCAL the clear and the flush of the block's table RP_LOCAL_SLOTS / 256 = 1 trip.  Every wave reaches both
// barriers, with or without voxels.
template <bool LOCAL>
__global__ void __launch_bounds__(64 * OVL_WAVES) rp_accumulate_kernel(RpDev m, const int* __restrict__ labels, int64_t n, int Y, int X, int n_max,
                                                                       RpStride stride) {
  __shared__ int lkeys[LOCAL ? RP_LOCAL_SLOTS : 1];
  __shared__ unsigned larea[LOCAL ? RP_LOCAL_SLOTS : 1];
  __shared__ unsigned long long lsums[LOCAL ? RP_LOCAL_SLOTS * 3 : 1];
  __shared__ int lbox[LOCAL ? RP_LOCAL_SLOTS * 6 : 1];
  __shared__ unsigned lclaimed;
  const RpLds loc{{lkeys, &lclaimed}, larea, lsums, lbox};
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
    lw_walk_runs(labels, begin, end, lane, Y, X, n_max, stride, [&](int32_t label, int32_t z, int32_t y, int32_t x0, uint32_t L) {
      if constexpr (LOCAL) rp_emit(loc, m, label, z, y, x0, L);
      else rp_emit(m, label, z, y, x0, L);
    });
  }
  if constexpr (LOCAL) {
    __syncthreads();
    for (int s = threadIdx.x; s < RP_LOCAL_SLOTS; s += 64 * OVL_WAVES) rp_merge(loc, (uint32_t)s, m);   // the flush: every label of the block once
  }
}

constexpr int RP_DEFAULT_LOCAL = 1;
int g_regionprops_local = RP_DEFAULT_LOCAL;   // bpx_debug_set_regionprops_local: 1 = form (b), the block's table in LDS first; 0 = form (a), every run to global; same bits

}  // namespace

extern "C" int bpx_debug_set_regionprops_local(int on) { g_regionprops_local = on < 0 ? RP_DEFAULT_LOCAL : on ? 1 : 0; return 0; }   // negative: back to the default

extern "C" int bpx_region_props(const int32_t* labels_d, int Z, int Y, int X, int n_max, int32_t* area_d, int64_t* sums_d, int32_t* bbox_d,
                                bpx_stream_t stream) {
  const char* fn = "bpx_region_props";
  BPX_CHECK(labels_d && area_d && sums_d && bbox_d, "%s: null pointer", fn);
  LW_CHECK_VOLUME(fn, Z, Y, X, n_max);
  BPX_CHECK((((uintptr_t)labels_d | (uintptr_t)area_d | (uintptr_t)bbox_d) & 3) == 0 && ((uintptr_t)sums_d & 7) == 0,
            "%s: labels, area and bbox must be 4-byte aligned, sums 8-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)n_max + 1;
  const RpDev m{reinterpret_cast<unsigned*>(area_d), reinterpret_cast<unsigned long long*>(sums_d), bbox_d};
  const unsigned blocks = lw_span_blocks(n);
  rp_init_kernel<<<lw_rows_grid(rows), 256, 0, s>>>(area_d, sums_d, bbox_d, rows);
  if (g_regionprops_local) rp_accumulate_kernel<true><<<blocks, 64 * OVL_WAVES, 0, s>>>(m, labels_d, n, Y, X, n_max, rp_stride(Y, X));
  else rp_accumulate_kernel<false><<<blocks, 64 * OVL_WAVES, 0, s>>>(m, labels_d, n, Y, X, n_max, rp_stride(Y, X));
  rp_finish_kernel<<<lw_rows_grid(rows), 256, 0, s>>>(area_d, sums_d, bbox_d, rows);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
