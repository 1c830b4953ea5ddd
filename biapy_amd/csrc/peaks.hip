// Local maxima of a float32 or int32 volume (Z, Y, X) on the device: the voxels whose 64-bit key (value, then raster-first index: peaks_core.h)
// is the maximum of the box [z-rz, z+rz] x [y-ry, y+ry] x [x-rx, x+rx] clipped to the volume, whose value passes the threshold and which keep
// the border margin - skimage.feature.peak_local_max's point creation for the detection workflow and the markers of the "distance map ->
// peaks -> watershed" recipe, with a deterministic tie rule that makes its ensure_spacing pass unnecessary (no two peaks lie in each other's box).
//
// LAUNCHES, fixed by (Z, Y, X, radii): one that clears the counter and fills the key array with 0, then one pass per axis with a nonzero radius
// and more than one voxel (one pass when there is no such axis), X then Y then Z.  Thread t owns chunk t % chunks of row t / chunks, a chunk
// being 4 voxels of the row, and everything it computes is peaks_core.h's peaks_lane.  The first pass forms the keys from the image (4 bytes read per voxel), the passes
// between write and read the running maxima as 8-byte keys in the workspace (two key volumes at most, 16 bytes per voxel), the last pass
// reads the image once more for the voxel's own key and writes the 0 / 1 mask; the 2 r + 1 (or 2 r + 4) fetches per voxel of a pass hit rows
// that neighbouring lanes fetch as well and are left to the caches.  A block gathers its peaks in LDS and takes its slots of the key array by
// ONE atomic on the counter; past max_peaks keys are dropped and the count keeps counting.  Which slot a key lands in may vary between runs,
// the set of keys may not.  No loop that a launch parameter or a constant does not bound; nothing read back; capturable.
#include "bpx_common.h"
#include "peaks_core.h"

namespace {

// LOOP BOUND: none - one slot per thread
__global__ void __launch_bounds__(256) peaks_init_kernel(uint64_t* __restrict__ keys, int max_peaks, int* __restrict__ num) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t == 0) *num = 0;
  if (keys && t < (uint32_t)max_peaks) keys[t] = 0;
}

// LOOP BOUNDS: those of peaks_lane; 4 voxels.  `total` = Z * Y * chunks < 2^31; no thread leaves before the last barrier
template <bool SRC_IMG, bool FINAL>
__global__ void __launch_bounds__(256) peaks_kernel(PeaksPass p, uint64_t* __restrict__ keys, int max_peaks, int* __restrict__ num, uint32_t chunks,
                                                    uint32_t total) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  uint64_t own[PEAKS_V];
  uint32_t found = 0;
  if (t < total) {
    const uint32_t row = t / chunks;
    found = peaks_lane<SRC_IMG, FINAL>(p, (int)(row / (uint32_t)p.Y), (int)(row % (uint32_t)p.Y), (int)(t - row * chunks), own);
  }
  if constexpr (FINAL) {
    __shared__ int block_count, block_base;
    if (threadIdx.x == 0) block_count = 0;
    __syncthreads();
    const int mine = __popc(found);
    int slot = 0;
    if (mine) slot = atomicAdd(&block_count, mine);
    __syncthreads();
    if (threadIdx.x == 0 && block_count) block_base = atomicAdd(num, block_count);
    __syncthreads();
    if (mine && keys) {
      slot += block_base;
#pragma unroll
      for (int e = 0; e < PEAKS_V; ++e)
        if (found >> e & 1u) {
          if (slot < max_peaks) keys[slot] = own[e];
          ++slot;
        }
    }
  }
}

}  // namespace

extern "C" int64_t bpx_peaks_workspace(int Z, int Y, int X) {
  if (Z < 1 || Y < 1 || X < 1) return -1;
  const int64_t n = (int64_t)Z * Y * X;
  if (n >= ((int64_t)1 << 31)) return -1;
  return 2 * n * (int64_t)sizeof(uint64_t);
}

extern "C" int bpx_peak_local_max(const void* img_d, int dtype, int Z, int Y, int X, int rz, int ry, int rx, double threshold, int bz, int by, int bx,
                                  void* mask_d, void* keys_d, int max_peaks, int* num_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  const char* fn = "bpx_peak_local_max";
  BPX_CHECK(img_d && num_d && ws_d, "%s: null pointer (img_d, num_d and ws_d are required)", fn);
  BPX_CHECK(mask_d || keys_d, "%s: no output: mask_d and keys_d are both null", fn);
  BPX_CHECK(Z >= 1 && Y >= 1 && X >= 1, "%s: extents must be at least 1 (got %d x %d x %d)", fn, Z, Y, X);
  const int64_t n = (int64_t)Z * Y * X;
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels: volumes of 2^31 voxels or more are not supported", fn, (long long)n);
  BPX_CHECK(dtype == BPX_F32 || dtype == BPX_I32, "%s: dtype must be float32 or int32 (got %d)", fn, dtype);
  BPX_CHECK(rz >= 0 && rz <= PEAKS_MAX_RADIUS && ry >= 0 && ry <= PEAKS_MAX_RADIUS && rx >= 0 && rx <= PEAKS_MAX_RADIUS,
            "%s: radii must be in 0..%d (got %d, %d, %d)", fn, PEAKS_MAX_RADIUS, rz, ry, rx);
  BPX_CHECK(bz >= 0 && by >= 0 && bx >= 0, "%s: the border margin must not be negative (got %d, %d, %d)", fn, bz, by, bx);
  BPX_CHECK(threshold == threshold, "%s: the threshold is NaN (pass -inf for none)", fn);
  BPX_CHECK(!keys_d || max_peaks >= 1, "%s: max_peaks must be at least 1 (got %d)", fn, max_peaks);
  BPX_CHECK(ws_bytes >= bpx_peaks_workspace(Z, Y, X), "%s: workspace too small: %lld bytes given, %lld needed", fn, (long long)ws_bytes,
            (long long)bpx_peaks_workspace(Z, Y, X));
  BPX_CHECK(((uintptr_t)img_d & 3) == 0, "%s: the image must be 4-byte aligned", fn);
  BPX_CHECK(((uintptr_t)ws_d & 7) == 0 && ((uintptr_t)keys_d & 7) == 0, "%s: the workspace and the key array must be 8-byte aligned", fn);
  BPX_CHECK(mask_d != img_d, "%s: mask_d must not be img_d (a voxel's neighbours are read after it is written)", fn);
  hipStream_t s = (hipStream_t)stream;
  uint64_t* keys = static_cast<uint64_t*>(keys_d);
  peaks_init_kernel<<<keys ? (unsigned)cdiv(max_peaks, 256) : 1u, 256, 0, s>>>(keys, max_peaks, num_d);

  PeaksStep steps[3];
  const int passes = peaks_plan(Z, Y, X, rz, ry, rx, steps);
  PeaksPass p{};
  p.img = img_d;
  p.mask = static_cast<uint8_t*>(mask_d);
  p.Z = Z; p.Y = Y; p.X = X;
  p.is_f32 = dtype == BPX_F32;
  p.thr_none = threshold == -__builtin_inf();
  p.thr = threshold;
  p.bz = bz; p.by = by; p.bx = bx;
  uint8_t* vol[2] = {static_cast<uint8_t*>(ws_d), static_cast<uint8_t*>(ws_d) + n * (int64_t)sizeof(uint64_t)};
  const uint32_t chunks = (uint32_t)cdiv(X, PEAKS_V), total = (uint32_t)((int64_t)Z * Y * chunks);
  const unsigned blocks = (unsigned)cdiv64(total, 256);
  for (int i = 0; i < passes; ++i) {                  // LOOP BOUND: 3
    const bool first = steps[i].src < 0, last = steps[i].dst < 0;
    p.axis = steps[i].axis;
    p.r = steps[i].r;
    p.src = first ? nullptr : vol[steps[i].src];
    p.dst = last ? nullptr : vol[steps[i].dst];
    if (first && last) peaks_kernel<true, true><<<blocks, 256, 0, s>>>(p, keys, max_peaks, num_d, chunks, total);
    else if (first) peaks_kernel<true, false><<<blocks, 256, 0, s>>>(p, keys, max_peaks, num_d, chunks, total);
    else if (last) peaks_kernel<false, true><<<blocks, 256, 0, s>>>(p, keys, max_peaks, num_d, chunks, total);
    else peaks_kernel<false, false><<<blocks, 256, 0, s>>>(p, keys, max_peaks, num_d, chunks, total);
  }
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
