// Separable correlation of a float32 volume (Z, Y, X) with one run-time 1-D kernel per axis, the border resolved as "reflect", "mirror",
// "nearest" or "constant": scipy.ndimage.correlate1d along z, then y, then x.  The Gaussian, its derivatives and the Laplacian of Gaussian are
// ways to fill the weights (biapy_amd/prepost.py: separable_filter, gaussian_filter, gaussian_laplace).
//
// ONE LAUNCH PER ACTIVE AXIS, fixed by (Z, Y, X, radii).  A pass reads its input about once: a block stages its tile and halo into LDS (4-byte
// loads, consecutive along the contiguous dimension across a wave; the halo's re-reads by neighbouring blocks are left to the caches), and
// after one barrier every thread produces 8 consecutive outputs along the filtered axis from a register window.  z and y keep the contiguous
// dimension on the lanes (sepfilter_lanes_kernel); x stages skewed row segments (sepfilter_rows_kernel) and stores 16 bytes where the address
// allows.  The passes ping-pong between out_d and ws_d so that the last writes out_d; in_d is never written.  The weights travel by value in
// the kernel arguments (65 floats per launch): no allocation, no copy, nothing read back; capturable.  Everything that decides a result is
// sepfilter_core.h's; this file maps a block to its tile.  No atomics; no loop that a constant or a launch parameter does not bound.
#include "bpx_common.h"
#include "sepfilter_core.h"

namespace {

// LOOP BOUNDS: those of sepfilter_stage_lanes and sepfilter_lane
__global__ void __launch_bounds__(SEPFILTER_THREADS) sepfilter_lanes_kernel(SepfilterArgs a) {
  extern __shared__ float sepfilter_img[];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
  const uint32_t b = blockIdx.x, by_i = b / (uint32_t)a.tiles_i;
  const int64_t i0 = (int64_t)(b - by_i * (uint32_t)a.tiles_i) * SEPFILTER_LANES;
  const int o = (int)(by_i / (uint32_t)a.tiles_a), a0 = (int)(by_i % (uint32_t)a.tiles_a) * a.p.TA;
  sepfilter_stage_lanes(a, sepfilter_img, o, a0, i0, wave, lane);
  __syncthreads();
  sepfilter_lane(a, sepfilter_img, o, a0, i0, wave, lane);
}

// LOOP BOUNDS: those of sepfilter_stage_rows and sepfilter_row
__global__ void __launch_bounds__(SEPFILTER_THREADS) sepfilter_rows_kernel(SepfilterArgs a) {
  extern __shared__ float sepfilter_img[];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
  const uint32_t b = blockIdx.x, by_x = b / (uint32_t)a.tiles_a;
  const int x0 = (int)(b - by_x * (uint32_t)a.tiles_a) * SEPFILTER_ROW_TX;
  const int64_t row0 = (int64_t)by_x * SEPFILTER_ROWS;
  sepfilter_stage_rows(a, sepfilter_img, row0, x0, wave, lane);
  __syncthreads();
  sepfilter_row(a, sepfilter_img, row0, x0, (int)threadIdx.x);
}

struct Pass {
  const float* w;
  int r, outer, n;
  int64_t inner;
};

bool finite_weights(const float* w, int r) {
  for (int j = 0; j < 2 * r + 1; ++j)
    if (!__builtin_isfinite(w[j])) return false;
  return true;
}

bool overlap(const void* p, const void* q, int64_t bytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)bytes && b < a + (uintptr_t)bytes;
}

// the axes with weights: 0 .. 3, or -1 when a radius is above the maximum (negative: the axis is skipped)
int active_axes(int rz, int ry, int rx) {
  if (rz > SEPFILTER_MAX_RADIUS || ry > SEPFILTER_MAX_RADIUS || rx > SEPFILTER_MAX_RADIUS) return -1;
  return (rz >= 0) + (ry >= 0) + (rx >= 0);
}

}  // namespace

extern "C" int64_t bpx_sepfilter_workspace(int Z, int Y, int X, int rz, int ry, int rx) {
  if (Z < 1 || Y < 1 || X < 1) return -1;
  const int64_t n = (int64_t)Z * Y * X;
  if (n >= ((int64_t)1 << 31)) return -1;
  const int active = active_axes(rz, ry, rx);
  if (active < 0) return -1;
  return active >= 2 ? 4 * n : 0;
}

extern "C" int bpx_sepfilter(const void* in_d, int Z, int Y, int X, const float* wz, int rz, const float* wy, int ry, const float* wx, int rx,
                             int mode, double cval, void* out_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  const char* fn = "bpx_sepfilter";
  BPX_CHECK(in_d && out_d, "%s: null pointer (in_d and out_d are required)", fn);
  BPX_CHECK((wz || rz < 0) && (wy || ry < 0) && (wx || rx < 0),
            "%s: null pointer: weights are required for a radius that is not negative (radii %d, %d, %d; a skipped axis has no weights and a "
            "negative radius)", fn, rz, ry, rx);
  BPX_CHECK(Z >= 1 && Y >= 1 && X >= 1, "%s: extents must be at least 1 (got %d x %d x %d)", fn, Z, Y, X);
  const int64_t n = (int64_t)Z * Y * X;
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels: volumes of 2^31 voxels or more are not supported", fn, (long long)n);
  BPX_CHECK((!wz || (rz >= 0 && rz <= SEPFILTER_MAX_RADIUS)) && (!wy || (ry >= 0 && ry <= SEPFILTER_MAX_RADIUS)) &&
                (!wx || (rx >= 0 && rx <= SEPFILTER_MAX_RADIUS)),
            "%s: the radius of an axis with weights must be in 0..%d (got %d, %d, %d)", fn, SEPFILTER_MAX_RADIUS, rz, ry, rx);
  BPX_CHECK((!wz || finite_weights(wz, rz)) && (!wy || finite_weights(wy, ry)) && (!wx || finite_weights(wx, rx)), "%s: a weight is not finite", fn);
  BPX_CHECK(mode >= SEPFILTER_REFLECT && mode <= SEPFILTER_CONSTANT, "%s: unknown mode %d (0 reflect, 1 mirror, 2 nearest, 3 constant)", fn, mode);
  BPX_CHECK(__builtin_isfinite(cval) && __builtin_isfinite((float)cval), "%s: cval must be finite as float32 (got %g)", fn, cval);

  Pass passes[3];
  int np = 0;
  if (wz) passes[np++] = Pass{wz, rz, 1, Z, (int64_t)Y * X};
  if (wy) passes[np++] = Pass{wy, ry, Z, Y, (int64_t)X};
  if (wx) passes[np++] = Pass{wx, rx, Z * Y, X, 1};
  const int64_t need = np >= 2 ? 4 * n : 0;
  BPX_CHECK(need == 0 || (ws_d && ws_bytes >= need), "%s: workspace too small: %lld bytes given, %lld needed (bpx_sepfilter_workspace)", fn,
            (long long)(ws_d ? ws_bytes : 0), (long long)need);
  BPX_CHECK(!overlap(in_d, out_d, 4 * n), "%s: out_d must not be in_d (a voxel's neighbours are read after it is written)", fn);
  BPX_CHECK(need == 0 || (!overlap(ws_d, in_d, 4 * n) && !overlap(ws_d, out_d, 4 * n)), "%s: ws_d must not be in_d or out_d (the passes alternate between ws_d and out_d)", fn);
  BPX_CHECK((((uintptr_t)in_d | (uintptr_t)out_d | (need ? (uintptr_t)ws_d : 0)) & 3) == 0, "%s: float32 volumes must be 4-byte aligned", fn);

  hipStream_t s = (hipStream_t)stream;
  if (np == 0) {                                      // no active axis: a copy of the bits
    const hipError_t e = hipMemcpyAsync(out_d, in_d, (size_t)(4 * n), hipMemcpyDeviceToDevice, s);
    BPX_CHECK(e == hipSuccess, "%s: copy failed: %s", fn, hipGetErrorString(e));
    return 0;
  }
  const float* src = static_cast<const float*>(in_d);
  for (int i = 0; i < np; ++i) {
    const Pass& ps = passes[i];
    float* dst = static_cast<float*>((np - 1 - i) % 2 == 0 ? out_d : ws_d);       // the last pass writes out_d
    SepfilterArgs a{};
    a.in = src;
    a.out = dst;
    a.inner = ps.inner;
    a.outer = ps.outer;
    a.n = ps.n;
    a.r = ps.r;
    a.mode = mode;
    a.cval = (float)cval;
    for (int j = 0; j < 2 * ps.r + 1; ++j) a.w[j] = ps.w[j];
    const bool rows = ps.inner == 1;
    a.p = sepfilter_plan(ps.r, rows);
    int64_t blocks;
    if (rows) {
      a.tiles_a = cdiv(ps.n, SEPFILTER_ROW_TX);
      a.tiles_i = 1;
      a.wide = ((uintptr_t)dst & 15) == 0 && ps.n % 4 == 0;
      blocks = cdiv64(ps.outer, SEPFILTER_ROWS) * a.tiles_a;
    } else {
      a.tiles_a = cdiv(ps.n, a.p.TA);
      a.tiles_i = (int)cdiv64(ps.inner, SEPFILTER_LANES);
      blocks = (int64_t)ps.outer * a.tiles_a * a.tiles_i;
    }
    // a tile holds at least one voxel: blocks <= Z * Y * X < 2^31
    if (rows) sepfilter_rows_kernel<<<(unsigned)blocks, SEPFILTER_THREADS, (size_t)a.p.lds_bytes, s>>>(a);
    else sepfilter_lanes_kernel<<<(unsigned)blocks, SEPFILTER_THREADS, (size_t)a.p.lds_bytes, s>>>(a);
    BPX_LAUNCH_CHECK(fn);
    src = dst;
  }
  return 0;
}
