// Shape properties of an int32 label volume (Z, Y, X) on the device, beside regionprops.hip's area / bbox / centroid: for every label l in
// 1..n_max its raw second-order coordinate sums and the covariance formed from them (inertia axes, elongation), the number of its voxel faces
// per axis (surface, sphericity) and, in 2-D, the three weight classes of scikit-image's perimeter estimator (perimeter, circularity) - what the
// instance workflow's property filter measures after label() / watershed(); the reference copies the label volume to the host for it.
//
// Integer atomics only (uint32 / uint64 add, relaxed): the same bits every run.  Nothing is read back, capturable; every loop is bounded by a
// launch parameter or a constant of shapeprops_core.h / regionprops_core.h, none by what another thread does.
//
// bpx_region_moments: zero, accumulate, finish (the finish only with cov_d).  THE ACCUMULATE PASS is regionprops.hip's, the one walk of
// label_walk.h (lw_walk_runs: spans, trips, heads, the carried run) with another emit: a run x0 .. x0 + L - 1 of row (z, y) contributes in
// closed form (sp_apply_moments) into the block's 256-slot table keyed by label in LDS (13 KB), which is merged into the global rows once per
// occupied slot.  An earlier version wrote the walk out here a second time for fear of what sharing would cost bpx_region_props in registers
// and speed (its bits cannot change: integers reached by commutative atomics); inlined with its emit the shared walk costs neither kernel a
// register, a wave per SIMD or scratch (profiles/kernel_resources.txt; timings: DESIGN.md section 4).
//
// bpx_region_faces: zero, count.  The same spans, trips and lanes; no runs: a lane that holds a labelled voxel also loads its voxels' neighbours
// in the rows y - 1, y + 1 and the planes z - 1, z + 1 (16-byte loads where the pointer and X allow it; they come from cache: a volume is read
// from memory once), gets its x neighbours from the lanes beside it (the first and last lane of a trip load theirs), compares labels - a cut
// between lanes, trips or spans is never a face - sums the faces of its consecutive voxels of one label (sp_count_step) and sends only sums that
// are not zero: the voxels inside an object cost no atomic.
//
// bpx_region_perimeter2d: zero, classify.  A block takes a tile of 16 x 64 pixels: labels with a halo of 2 into LDS, border flags with a halo
// of 1 from them, then the class of every border pixel of the tile (sp_pixel_class), summed per lane and label as the faces are.
#include <algorithm>

#include "bpx_common.h"
#include "label_walk.h"
#include "shapeprops_core.h"

namespace {

struct MomDev {    // the global rows
  unsigned long long* mom_p;
  __device__ __forceinline__ void mom(uint32_t r, int k, uint64_t v) const {
    __hip_atomic_fetch_add(mom_p + (int64_t)r * SP_MOMENTS + k, (unsigned long long)v, LW_RLX_AGENT);
  }
};
struct MomLds : LwKeysLds {
  unsigned long long* mom_p;
  __device__ __forceinline__ void mom(uint32_t s, int k, uint64_t v) const { __hip_atomic_fetch_add(mom_p + s * SP_MOMENTS + k, (unsigned long long)v, LW_RLX_WG); }
  __device__ __forceinline__ uint64_t mom_of(uint32_t s, int k) const { return mom_p[s * SP_MOMENTS + k]; }
};

template <class T> struct CntDev {    // T: unsigned long long (faces), unsigned (perimeter classes)
  T* cnt_p;
  __device__ __forceinline__ void cnt(uint32_t r, int k, uint32_t v) const { __hip_atomic_fetch_add(cnt_p + (int64_t)r * SP_COUNTERS + k, (T)v, LW_RLX_AGENT); }
};
struct CntLds : LwKeysLds {
  unsigned* cnt_p;
  __device__ __forceinline__ void cnt(uint32_t s, int k, uint32_t v) const { __hip_atomic_fetch_add(cnt_p + s * SP_COUNTERS + k, v, LW_RLX_WG); }
  __device__ __forceinline__ uint32_t cnt_of(uint32_t s, int k) const { return cnt_p[s * SP_COUNTERS + k]; }
};

// thread t zeroes the words t, t + T ...  LOOP BOUND: ceil(words / T) trips, fixed by the launch
__global__ void __launch_bounds__(256) sp_zero_kernel(uint32_t* __restrict__ p, int64_t words) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) p[i] = 0;
}

// moments: wave w of the grid owns the voxels [w * OVL_SPAN, (w + 1) * OVL_SPAN) below n and walks their runs (label_walk.h: lw_walk_runs, 32
// trips).  LOOP BOUND: the clear and the flush of the block's table RP_LOCAL_SLOTS / 256 = 1 trip.  Every wave reaches both barriers, with or
// without voxels.
__global__ void __launch_bounds__(64 * OVL_WAVES) sp_moments_kernel(MomDev m, const int* __restrict__ labels, int64_t n, int Y, int X, int n_max, RpStride stride) {
  __shared__ int lkeys[RP_LOCAL_SLOTS];
  __shared__ unsigned long long lmom[RP_LOCAL_SLOTS * SP_MOMENTS];
  __shared__ unsigned lclaimed;
  const MomLds loc{{lkeys, &lclaimed}, lmom};
  for (int s = threadIdx.x; s < RP_LOCAL_SLOTS; s += 64 * OVL_WAVES) {
    lkeys[s] = 0;
#pragma unroll
    for (int k = 0; k < SP_MOMENTS; ++k) lmom[s * SP_MOMENTS + k] = 0;
  }
  if (threadIdx.x == 0) lclaimed = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t begin = ((int64_t)blockIdx.x * OVL_WAVES + (threadIdx.x >> 6)) * OVL_SPAN;
  if (begin < n) {                                                      // the whole wave
    const int64_t end = begin + OVL_SPAN < n ? begin + OVL_SPAN : n;
    lw_walk_runs(labels, begin, end, lane, Y, X, n_max, stride,
                 [&](int32_t label, int32_t z, int32_t y, int32_t x0, uint32_t L) { sp_emit_moments(loc, m, label, z, y, x0, L); });
  }
  __syncthreads();
  for (int s = threadIdx.x; s < RP_LOCAL_SLOTS; s += 64 * OVL_WAVES) sp_merge_moments(loc, (uint32_t)s, m);   // the flush: every label of the block once
}

// thread t takes the rows t, t + T ...  LOOP BOUND: ceil(rows / T) trips, fixed by the launch
__global__ void __launch_bounds__(256) sp_finish_kernel(const int* __restrict__ area, const int64_t* __restrict__ sums, const int64_t* __restrict__ mom,
                                                        double* __restrict__ cov, int64_t rows) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256)
    sp_finish_row(area + r, sums + r * 3, mom + r * SP_MOMENTS, cov + r * SP_MOMENTS);
}

// the labels (after rp_label) of the four voxels j .. j + 3, all inside the volume; `vec`: j is a multiple of 4 voxels from a 16-byte aligned base
__device__ __forceinline__ void neighbours4(const int* __restrict__ x, int64_t j, bool vec, int n_max, int32_t out[OVL_VPL]) {
  int v[OVL_VPL];
  if (vec) {
    const u32x4_t w = *reinterpret_cast<const u32x4_t*>(x + j);
    v[0] = (int)w[0]; v[1] = (int)w[1]; v[2] = (int)w[2]; v[3] = (int)w[3];
  } else {
    v[0] = x[j]; v[1] = x[j + 1]; v[2] = x[j + 2]; v[3] = x[j + 3];
  }
#pragma unroll
  for (int e = 0; e < OVL_VPL; ++e) out[e] = rp_label(v[e], n_max);
}

// faces: the spans, trips and lanes of the moments pass.  LOOP BOUND: 32 trips; the clear and the flush of the block's table 1 trip.
// Every address formed lies inside the volume: a neighbour is loaded only where the voxel's own coordinate says it exists.
__global__ void __launch_bounds__(64 * OVL_WAVES) sp_faces_kernel(CntDev<unsigned long long> m, const int* __restrict__ labels, int64_t n, int Z, int Y, int X,
                                                                  int n_max, RpStride stride) {
  __shared__ int lkeys[RP_LOCAL_SLOTS];
  __shared__ unsigned lcnt[RP_LOCAL_SLOTS * SP_COUNTERS];
  __shared__ unsigned lclaimed;
  const CntLds loc{{lkeys, &lclaimed}, lcnt};
  for (int s = threadIdx.x; s < RP_LOCAL_SLOTS; s += 64 * OVL_WAVES) {
    lkeys[s] = 0;
#pragma unroll
    for (int k = 0; k < SP_COUNTERS; ++k) lcnt[s * SP_COUNTERS + k] = 0;
  }
  if (threadIdx.x == 0) lclaimed = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t begin = ((int64_t)blockIdx.x * OVL_WAVES + (threadIdx.x >> 6)) * OVL_SPAN;
  if (begin < n) {                                                      // the whole wave
    const int64_t end = begin + OVL_SPAN < n ? begin + OVL_SPAN : n;
    const bool vec = lw_aligned16(labels);
    const bool rowvec = vec && (X & 3) == 0;                            // a lane's four voxels share a row, and the rows above and below are aligned as it is
    const int64_t plane = (int64_t)Y * X;
    RpPos at = rp_pos_of((uint32_t)(begin + OVL_VPL * lane), Y, X);
    int v[OVL_VPL], nv[OVL_VPL] = {0, 0, 0, 0};
    lw_load4(labels, begin + OVL_VPL * lane, end, vec, v);
    for (int64_t t = begin; t < end; t += OVL_TRIP) {
      if (t + OVL_TRIP < end) lw_load4(labels, t + OVL_TRIP + OVL_VPL * lane, end, vec, nv);
      const int64_t i0 = t + OVL_VPL * lane;                            // this lane's first voxel; voxel e exists when i0 + e < end (else its label is 0)
      int32_t lab[OVL_VPL];
      RpPos pos[OVL_VPL];
      pos[0] = at;
#pragma unroll
      for (int e = 0; e < OVL_VPL; ++e) {
        lab[e] = rp_label(v[e], n_max);
        if (e) { pos[e] = pos[e - 1]; rp_step(pos[e], Y, X); }
      }
      // the x neighbours across lanes: by shuffle inside the trip, by a load at its two ends (a voxel with x > 0 has a predecessor in the volume,
      // one with x < X - 1 a successor); a voxel past `end` has label 0 and asks for nothing
      int32_t left = __shfl_up(lab[OVL_VPL - 1], 1, OVL_LANES), right = __shfl_down(lab[0], 1, OVL_LANES);
      if (lane == 0 && lab[0] > 0 && pos[0].x > 0) left = rp_label(labels[i0 - 1], n_max);
      if (lane == OVL_LANES - 1 && lab[OVL_VPL - 1] > 0 && pos[OVL_VPL - 1].x < X - 1) right = rp_label(labels[i0 + OVL_VPL], n_max);
      if ((lab[0] | lab[1] | lab[2] | lab[3]) != 0) {                   // labels are >= 0: some voxel of the lane is labelled
        int32_t ym[OVL_VPL], yp[OVL_VPL], zm[OVL_VPL], zp[OVL_VPL];
        if (rowvec && i0 + OVL_VPL <= end) {
#pragma unroll
          for (int e = 0; e < OVL_VPL; ++e) ym[e] = yp[e] = zm[e] = zp[e] = SP_OUTSIDE;
          if (pos[0].y > 0) neighbours4(labels, i0 - X, true, n_max, ym);
          if (pos[0].y < Y - 1) neighbours4(labels, i0 + X, true, n_max, yp);
          if (pos[0].z > 0) neighbours4(labels, i0 - plane, true, n_max, zm);
          if (pos[0].z < Z - 1) neighbours4(labels, i0 + plane, true, n_max, zp);
        } else {
#pragma unroll
          for (int e = 0; e < OVL_VPL; ++e) {
            const bool on = lab[e] > 0;                                 // a labelled voxel exists, so its coordinates are those of a voxel of the volume
            ym[e] = on && pos[e].y > 0 ? rp_label(labels[i0 + e - X], n_max) : SP_OUTSIDE;
            yp[e] = on && pos[e].y < Y - 1 ? rp_label(labels[i0 + e + X], n_max) : SP_OUTSIDE;
            zm[e] = on && pos[e].z > 0 ? rp_label(labels[i0 + e - plane], n_max) : SP_OUTSIDE;
            zp[e] = on && pos[e].z < Z - 1 ? rp_label(labels[i0 + e + plane], n_max) : SP_OUTSIDE;
          }
        }
        sp_lane_faces(loc, m, lab, pos, left, right, ym, yp, zm, zp, X);
      }
      rp_advance(at, stride, Y, X);
#pragma unroll
      for (int e = 0; e < OVL_VPL; ++e) v[e] = nv[e];
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < RP_LOCAL_SLOTS; s += 64 * OVL_WAVES) sp_merge_counts(loc, (uint32_t)s, m);
}

// perimeter classes: block b takes tile (b / tiles_x, b % tiles_x).  LOOP BOUNDS: the label tile 20 x 68 in 6 trips of 256 threads, the border tile
// 18 x 66 in 5, four pixels of a row per thread, the table's clear and flush 1 trip.
__global__ void __launch_bounds__(256) sp_perimeter_kernel(CntDev<unsigned> m, const int* __restrict__ labels, int Y, int X, int n_max, int tiles_x) {
  __shared__ int lkeys[RP_LOCAL_SLOTS];
  __shared__ unsigned lcnt[RP_LOCAL_SLOTS * SP_COUNTERS];
  __shared__ unsigned lclaimed;
  __shared__ int lab[SP_LH * SP_LW];
  __shared__ unsigned char bor[SP_BH * SP_BW];
  const CntLds loc{{lkeys, &lclaimed}, lcnt};
  for (int s = threadIdx.x; s < RP_LOCAL_SLOTS; s += 256) {
    lkeys[s] = 0;
#pragma unroll
    for (int k = 0; k < SP_COUNTERS; ++k) lcnt[s * SP_COUNTERS + k] = 0;
  }
  if (threadIdx.x == 0) lclaimed = 0;
  const int y0 = (int)(blockIdx.x / (unsigned)tiles_x) * SP_TY, x0 = (int)(blockIdx.x % (unsigned)tiles_x) * SP_TX;
  for (int i = threadIdx.x; i < SP_LH * SP_LW; i += 256) {
    const int64_t gy = (int64_t)y0 - 2 + i / SP_LW, gx = (int64_t)x0 - 2 + i % SP_LW;       // outside the image: background
    lab[i] = gy >= 0 && gy < Y && gx >= 0 && gx < X ? rp_label(labels[gy * X + gx], n_max) : 0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SP_BH * SP_BW; i += 256) {
    const int c = (i / SP_BW + 1) * SP_LW + i % SP_BW + 1;
    bor[i] = sp_is_border(lab[c], lab[c - SP_LW], lab[c + SP_LW], lab[c - 1], lab[c + 1]) ? 1 : 0;
  }
  __syncthreads();
  const int ty = threadIdx.x / (SP_TX / 4), tx = (threadIdx.x % (SP_TX / 4)) * 4;
  SpCount acc{0, {0, 0, 0}};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int cls = sp_pixel_class(lab, bor, ty, tx + e);
    sp_count_step(loc, m, acc, cls < 0 ? 0 : lab[(ty + 2) * SP_LW + tx + e + 2], cls == 0, cls == 1, cls == 2);
  }
  sp_count_flush(loc, m, acc);
  __syncthreads();
  for (int s = threadIdx.x; s < RP_LOCAL_SLOTS; s += 256) sp_merge_counts(loc, (uint32_t)s, m);
}

}  // namespace

extern "C" int bpx_region_moments(const int32_t* labels_d, int Z, int Y, int X, int n_max, const int32_t* area_d, const int64_t* sums_d, int64_t* mom_d,
                                  double* cov_d, bpx_stream_t stream) {
  const char* fn = "bpx_region_moments";
  BPX_CHECK(labels_d && mom_d && (!cov_d || (area_d && sums_d)), "%s: null pointer", fn);
  LW_CHECK_VOLUME(fn, Z, Y, X, n_max);
  BPX_CHECK((((uintptr_t)labels_d | (uintptr_t)area_d) & 3) == 0 && (((uintptr_t)sums_d | (uintptr_t)mom_d | (uintptr_t)cov_d) & 7) == 0,
            "%s: labels and area must be 4-byte aligned, sums, moments and covariance 8-byte aligned", fn);
  BPX_CHECK(sp_moments_fit(n, std::max(Z, std::max(Y, X))), "%s: %d x %d x %d: n * (Emax - 1)^2 must stay below 2^63 for the moments to fit int64", fn, Z, Y, X);
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)n_max + 1;
  const MomDev m{reinterpret_cast<unsigned long long*>(mom_d)};
  const unsigned blocks = lw_span_blocks(n);
  sp_zero_kernel<<<lw_rows_grid(rows * SP_MOMENTS * 2), 256, 0, s>>>(reinterpret_cast<uint32_t*>(mom_d), rows * SP_MOMENTS * 2);
  sp_moments_kernel<<<blocks, 64 * OVL_WAVES, 0, s>>>(m, labels_d, n, Y, X, n_max, rp_stride(Y, X));
  if (cov_d) sp_finish_kernel<<<lw_rows_grid(rows), 256, 0, s>>>(area_d, sums_d, mom_d, cov_d, rows);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_region_faces(const int32_t* labels_d, int Z, int Y, int X, int n_max, int64_t* faces_d, bpx_stream_t stream) {
  const char* fn = "bpx_region_faces";
  BPX_CHECK(labels_d && faces_d, "%s: null pointer", fn);
  LW_CHECK_VOLUME(fn, Z, Y, X, n_max);
  BPX_CHECK(((uintptr_t)labels_d & 3) == 0 && ((uintptr_t)faces_d & 7) == 0, "%s: labels must be 4-byte aligned, faces 8-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)n_max + 1;
  const CntDev<unsigned long long> m{reinterpret_cast<unsigned long long*>(faces_d)};
  const unsigned blocks = lw_span_blocks(n);
  sp_zero_kernel<<<lw_rows_grid(rows * SP_COUNTERS * 2), 256, 0, s>>>(reinterpret_cast<uint32_t*>(faces_d), rows * SP_COUNTERS * 2);
  sp_faces_kernel<<<blocks, 64 * OVL_WAVES, 0, s>>>(m, labels_d, n, Z, Y, X, n_max, rp_stride(Y, X));
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_region_perimeter2d(const int32_t* labels_d, int Y, int X, int n_max, int32_t* classes_d, bpx_stream_t stream) {
  const char* fn = "bpx_region_perimeter2d";
  BPX_CHECK(labels_d && classes_d, "%s: null pointer", fn);
  LW_CHECK_VOLUME(fn, 1, Y, X, n_max);
  BPX_CHECK((((uintptr_t)labels_d | (uintptr_t)classes_d) & 3) == 0, "%s: labels and classes must be 4-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)n_max + 1;
  const CntDev<unsigned> m{reinterpret_cast<unsigned*>(classes_d)};
  const int tiles_x = (int)cdiv64(X, SP_TX);                            // tiles_x * tiles_y <= n / 1024 + X / 64 + Y / 16 + 1: below 2^31
  const int64_t tiles = (int64_t)tiles_x * cdiv64(Y, SP_TY);
  sp_zero_kernel<<<lw_rows_grid(rows * SP_COUNTERS), 256, 0, s>>>(reinterpret_cast<uint32_t*>(classes_d), rows * SP_COUNTERS);
  sp_perimeter_kernel<<<(unsigned)tiles, 256, 0, s>>>(m, labels_d, Y, X, n_max, tiles_x);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
