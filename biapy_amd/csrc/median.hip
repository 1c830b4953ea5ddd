// Median filter of a float32 or uint8 volume (Z, Y, X) on the device: at every voxel the element of rank W / 2 among the W = sz * sy * sx values
// of its window, the border resolved as "reflect", "nearest" or "constant" - scipy.ndimage.median_filter(x, size=(sz, sy, sx), mode=, cval=), the
// first step of the reference's post-processing of a prediction.  Exact selection on order-preserving uint32 keys, no arithmetic: the bits
// that went in come out.
//
// ONE LAUNCH, fixed by (Z, Y, X, dtype, sizes).  A block of 256 threads owns median_plan's tile of TZ x TY x 64 outputs: it stages the tile and
// its halo into LDS as keys, the border mode resolved once per staged element (4-byte or 1-byte loads, consecutive along x across a wave; the
// halo's re-reads by neighbouring blocks are left to the caches), and after one barrier every thread runs its outputs' windows through the
// selection network of the window COUNT, reading LDS at consecutive addresses across the wave with offsets that are the same for every lane.
// Everything that decides a result is median_core.h's: median_stage, median_lane and what they call; this file maps a block to its tile and
// picks the instance; a volume so thin and long that it needs 2^24 tiles or more is refused after the other checks.  No atomics, no workspace, nothing read back, no loop that a constant or a launch parameter does not bound; capturable.
#include "bpx_common.h"
#include "median_core.h"

namespace {

// LOOP BOUNDS: those of median_stage and median_lane
template <int WI> __global__ void __launch_bounds__(MEDIAN_THREADS) median_kernel(MedianArgs a) {
  extern __shared__ uint32_t median_img[];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
  const uint32_t b = blockIdx.x, by_z = b / (uint32_t)a.tiles_x;
  const int x0 = (int)(b - by_z * (uint32_t)a.tiles_x) * a.p.TX;
  const int z0 = (int)(by_z / (uint32_t)a.tiles_y) * a.p.TZ, y0 = (int)(by_z % (uint32_t)a.tiles_y) * a.p.TY;
  median_stage(a, median_img, z0, y0, x0, wave, lane);
  __syncthreads();
  median_lane<WI>(a, median_img, z0, y0, x0, wave, lane);
}

template <int WI> void median_launch(const MedianArgs& a, unsigned blocks, hipStream_t s) {
  median_kernel<WI><<<blocks, MEDIAN_THREADS, (size_t)a.p.lds_bytes, s>>>(a);
}

}  // namespace

extern "C" int bpx_median_filter(const void* in_d, int dtype, int Z, int Y, int X, int sz, int sy, int sx, int mode, double cval, void* out_d,
                                 bpx_stream_t stream) {
  const char* fn = "bpx_median_filter";
  BPX_CHECK(in_d && out_d, "%s: null pointer (in_d and out_d are required)", fn);
  BPX_CHECK(Z >= 1 && Y >= 1 && X >= 1, "%s: extents must be at least 1 (got %d x %d x %d)", fn, Z, Y, X);
  const int64_t n = (int64_t)Z * Y * X;
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels: volumes of 2^31 voxels or more are not supported", fn, (long long)n);
  BPX_CHECK(dtype == BPX_F32 || dtype == BPX_U8, "%s: dtype must be float32 or uint8 (got %d)", fn, dtype);
  BPX_CHECK(sz >= 1 && sz <= MEDIAN_MAX_SIZE && sy >= 1 && sy <= MEDIAN_MAX_SIZE && sx >= 1 && sx <= MEDIAN_MAX_SIZE && (sz & sy & sx & 1),
            "%s: sizes must be odd and in 1..%d (got %d, %d, %d)", fn, MEDIAN_MAX_SIZE, sz, sy, sx);
  const int W = sz * sy * sx;
  BPX_CHECK(W <= MEDIAN_MAX_WINDOW, "%s: a window of %d x %d x %d = %d voxels: at most %d are supported", fn, sz, sy, sx, W, MEDIAN_MAX_WINDOW);
  BPX_CHECK(mode == MEDIAN_REFLECT || mode == MEDIAN_NEAREST || mode == MEDIAN_CONSTANT, "%s: unknown mode %d (0 reflect, 1 nearest, 2 constant)", fn,
            mode);
  const bool is_f32 = dtype == BPX_F32;
  if (is_f32) BPX_CHECK(__builtin_isfinite(cval) && __builtin_isfinite((float)cval), "%s: cval must be finite as float32 (got %g)", fn, cval);
  else BPX_CHECK(cval >= 0.0 && cval <= 255.0 && cval == (double)(int)cval, "%s: cval must be an integer in 0..255 for uint8 (got %g)", fn, cval);
  BPX_CHECK(out_d != in_d, "%s: out_d must not be in_d (a voxel's neighbours are read after it is written)", fn);
  BPX_CHECK(!is_f32 || (((uintptr_t)in_d | (uintptr_t)out_d) & 3) == 0, "%s: float32 volumes must be 4-byte aligned", fn);

  MedianArgs a{};
  a.in = in_d;
  a.out = out_d;
  a.Z = Z; a.Y = Y; a.X = X;
  a.sz = sz; a.sy = sy; a.sx = sx;
  a.mode = mode;
  a.is_f32 = is_f32;
  a.ckey = median_cval_key(cval, is_f32);
  a.W = W;
  a.p = median_plan(sz, sy, sx);
  a.tiles_x = cdiv(X, a.p.TX);
  a.tiles_y = cdiv(Y, a.p.TY);
  const int64_t blocks = (int64_t)cdiv(Z, a.p.TZ) * a.tiles_y * a.tiles_x;
  BPX_CHECK(blocks < ((int64_t)1 << 24), "%s: a %d x %d x %d volume needs %lld tiles of %d x %d x %d, more than one launch holds", fn, Z, Y, X,
            (long long)blocks, a.p.TZ, a.p.TY, a.p.TX);
  hipStream_t s = (hipStream_t)stream;
  switch (median_instance(W)) {
    case 3: median_launch<3>(a, (unsigned)blocks, s); break;
    case 5: median_launch<5>(a, (unsigned)blocks, s); break;
    case 7: median_launch<7>(a, (unsigned)blocks, s); break;
    case 9: median_launch<9>(a, (unsigned)blocks, s); break;
    case 15: median_launch<15>(a, (unsigned)blocks, s); break;
    case 25: median_launch<25>(a, (unsigned)blocks, s); break;
    case 27: median_launch<27>(a, (unsigned)blocks, s); break;
    case 49: median_launch<49>(a, (unsigned)blocks, s); break;
    case 75: median_launch<75>(a, (unsigned)blocks, s); break;
    case 125: median_launch<125>(a, (unsigned)blocks, s); break;
    default: BPX_FAIL("%s: no instance for a window of %d voxels", fn, W);
  }
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
