// Noise2Void on the device (biapy_amd/n2v.py states the semantics, include/biapy_amd.h the entry points): the blind-spot masking of a float32
// (B,Z,Y,X,C) batch with its (B,2C,Z,Y,X) target, and the masked MSE loss on that target.
//
// Masking, two launches:
//   n2v_stream_kernel  x_masked = x and target = 0 at memory rate: 16-byte stores from the destination's first 16-byte boundary on (16-byte
//                      loads where the source is aligned there too, four 4-byte loads otherwise), a scalar head and tail.  Thread 0 of block 0
//                      also moves the counter: state[1] = state[0] (the value this call draws with), state[0] += 1 - no other thread of the
//                      launch reads the state, so no ticket and no atomic is needed.
//   n2v_sparse_kernel  one thread per (sample, channel, box): n2v_box (n2v_core.h) under state[1], one load of the INPUT at the source, the
//                      three words (masked value, original, 1) and the two inspection hooks.  Boxes are disjoint, so no two threads write one word.
// Random numbers: Philox4x32-10, key (seed low ^ 0x4E32564D, seed high), counter words (box, (sample << 4) | channel | (stream << 28), counter
// low, counter high); stream 0 the position, stream 1 the replacement.
//
// Loss: loss = sum e^2 / sum m over the whole batch, e = v - pred m, v = target[:, :C], m = target[:, C:]; the per-channel loss's layout (plain_losses.hip) from the
// shared pieces of loss_parts.h: grid (blocks, N C), fp32 partials of both sums per block in a fixed order, a one-block finish in double
// (strided_sums_256) that also stores 1 / sum m for the backward.
#include <math.h>

#include "loss_parts.h"
#include "n2v_core.h"

namespace {

// dst[0..n) = src[0..n) (COPY) or 0: 16-byte stores from dst's first 16-byte boundary on
template <bool COPY>
__device__ __forceinline__ void stream_fill(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int64_t n) {
  const int64_t lead = (int64_t)(((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u) >> 2), head = lead < n ? lead : n;
  const int64_t n4 = (n - head) >> 2, tail0 = head + 4 * n4;
  const bool src16 = COPY && (((uintptr_t)(src + head)) & 15u) == 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    u32x4_t v = u32x4_t{0u, 0u, 0u, 0u};
    if (COPY) {
      const uint32_t* s = src + head + 4 * i;
      if (src16) v = *reinterpret_cast<const u32x4_t*>(s);
      else v = u32x4_t{s[0], s[1], s[2], s[3]};
    }
    *reinterpret_cast<u32x4_t*>(dst + head + 4 * i) = v;
  }
  if (blockIdx.x == 0) {
    if ((int64_t)threadIdx.x < head) dst[threadIdx.x] = COPY ? src[threadIdx.x] : 0u;
    if ((int64_t)threadIdx.x < n - tail0) dst[tail0 + threadIdx.x] = COPY ? src[tail0 + threadIdx.x] : 0u;
  }
}

__global__ void __launch_bounds__(256) n2v_stream_kernel(const uint32_t* __restrict__ x, uint32_t* __restrict__ xo, int64_t n, uint32_t* __restrict__ t,
                                                         int64_t nt, uint64_t* __restrict__ state) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t q = state[0];
    state[1] = q;
    state[0] = q + 1;
  }
  stream_fill<true>(x, xo, n);
  stream_fill<false>(nullptr, t, nt);
}

__global__ void __launch_bounds__(256) n2v_sparse_kernel(const float* __restrict__ x, N2VGeom g, int C, int64_t boxes, int64_t total, uint64_t seed, float sigma,
                                                         const uint64_t* __restrict__ state, float* __restrict__ xo, float* __restrict__ t,
                                                         int32_t* __restrict__ coords, int32_t* __restrict__ sources) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= total) return;
  const uint64_t q = state[1];
  const int64_t bc = j / boxes;
  const uint32_t i = (uint32_t)(j - bc * boxes), b = (uint32_t)(bc / C), c = (uint32_t)(bc - (int64_t)b * C);
  const N2VPick pk = n2v_box(g, (uint32_t)seed ^ N2V_KEY_XOR, (uint32_t)(seed >> 32), (uint32_t)q, (uint32_t)(q >> 32), b, c, i);
  coords[j] = (int32_t)pk.coord;
  sources[j] = (int32_t)pk.source;
  if (pk.coord < 0) return;
  const int64_t V = (int64_t)g.Z * g.Y * g.X;
  const float orig = x[((int64_t)b * V + pk.coord) * C + c];
  float v = pk.source == pk.coord ? orig : x[((int64_t)b * V + pk.source) * C + c];
  if (g.manip == N2V_NORMAL_ADDITIVE) {                                  // augment.hip's noise4, its cosine element
    const float u1 = (float)((pk.r0 >> 8) + 1u) * 5.9604644775390625e-8f;
    const float u2 = (float)(pk.r1 >> 8) * 5.9604644775390625e-8f;
    const float rad = sqrtf(-2.f * logf(u1)), ang = 6.283185307179586f * u2;
    v = __fadd_rn(orig, __fmul_rn(sigma, rad * cosf(ang)));
  }
  xo[((int64_t)b * V + pk.coord) * C + c] = v;
  const int64_t plane = ((int64_t)b * 2 * C + c) * V + pk.coord;
  t[plane] = orig;
  t[plane + (int64_t)C * V] = 1.f;
}

// ---- the masked MSE ---------------------------------------------------------------------------------------------------------------------------
// grid (blocks, N C): partial sums of e^2 and of m over plane (n, c) -> part[plane * nb + block] and part[(N C + plane) * nb + block]
__global__ void __launch_bounds__(256) n2v_loss_sums_kernel(const float* __restrict__ pred, const float* __restrict__ target, int64_t vox, int C,
                                                            float* __restrict__ part) {
  const int plane = blockIdx.y, n = plane / C, c = plane - n * C;
  const float* pp = pred + (size_t)plane * vox;
  const float* vp = target + ((size_t)n * 2 * C + c) * vox;
  const float* mp = vp + (size_t)C * vox;
  float s[2] = {0.f, 0.f};                      // sum e^2, sum m
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < vox; i += (int64_t)gridDim.x * 256) {
    const float m = mp[i], e = vp[i] - pp[i] * m;
    s[0] += e * e;
    s[1] += m;
  }
  s[0] = wave_sum(s[0]);
  s[1] = wave_sum(s[1]);
  __shared__ float red[4][2];
  four_wave_hand_over(s, red);
  if (threadIdx.x == 0) {
    part[(size_t)plane * gridDim.x + blockIdx.x] = four_wave_sum_seq(red, 0);
    part[((size_t)gridDim.y + plane) * gridDim.x + blockIdx.x] = four_wave_sum_seq(red, 1);
  }
}

// out[0] = sum e^2 / sum m, out[1] = 1 / sum m (both 0 when nothing is masked): fixed-order double sums of the count partials of either kind
__global__ void __launch_bounds__(256) n2v_loss_finish_kernel(const float* __restrict__ part, int64_t count, float* __restrict__ out) {
  __shared__ double red[2][256];
  double s[2];                                  // sum e^2, sum m
  strided_sums_256(count, [&](int k, int64_t q) { return part[(size_t)k * count + q]; }, red, s);
  if (threadIdx.x == 0) {
    const bool any = s[1] > 0.;
    out[0] = any ? (float)(s[0] / s[1]) : 0.f;
    out[1] = any ? (float)(1. / s[1]) : 0.f;
  }
}

// dpred = (gup inv) * (-2 (m e)), inv = saved[1]
__global__ void __launch_bounds__(256) n2v_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, int64_t vox, int C,
                                                           const float* __restrict__ saved, const float* __restrict__ gup, float* __restrict__ dpred) {
  const int plane = blockIdx.y, n = plane / C, c = plane - n * C;
  const float k = gup[0] * saved[1];
  const float* pp = pred + (size_t)plane * vox;
  const float* vp = target + ((size_t)n * 2 * C + c) * vox;
  const float* mp = vp + (size_t)C * vox;
  float* dp = dpred + (size_t)plane * vox;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < vox; i += (int64_t)gridDim.x * 256) {
    const float m = mp[i], e = vp[i] - pp[i] * m;
    dp[i] = k * (-2.f * (m * e));
  }
}

bool spans_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

// the checked, normalised geometry of a configuration on a (Z, Y, X) sample; 0 or an error
int n2v_geom(const char* fn, const bpx_n2v_cfg* cfg, int Z, int Y, int X, N2VGeom& g, int64_t& boxes) {
  BPX_CHECK(cfg, "%s: null pointer", fn);
  BPX_CHECK(Z > 0 && Y > 0 && X > 0, "%s: bad extents", fn);
  BPX_CHECK((int64_t)Z * Y * X < (1ll << 31), "%s: a sample of %lld voxels; 2^31 or more are not supported (the hooks are int32)", fn, (long long)Z * Y * X);
  BPX_CHECK(cfg->manipulator >= N2V_UNIFORM_WITH_CP && cfg->manipulator <= N2V_NORMAL_ADDITIVE, "%s: unknown manipulator %d", fn, cfg->manipulator);
  const int dim[3] = {Z, Y, X};
  int s[3], r[3], n[3];
  for (int a = 0; a < 3; ++a) {
    BPX_CHECK(cfg->box[a] >= 1 && cfg->box[a] <= N2V_MAX_BOX, "%s: box edge %d outside 1..%d", fn, cfg->box[a], N2V_MAX_BOX);
    BPX_CHECK(cfg->radius[a] >= 0 && cfg->radius[a] <= N2V_MAX_RADIUS, "%s: radius %d outside 0..%d", fn, cfg->radius[a], N2V_MAX_RADIUS);
    s[a] = dim[a] == 1 ? 1 : cfg->box[a];
    r[a] = dim[a] == 1 ? 0 : cfg->radius[a];
    n[a] = (dim[a] + s[a] - 1) / s[a];
  }
  BPX_CHECK(isfinite(cfg->sigma), "%s: sigma must be finite", fn);
  boxes = (int64_t)n[0] * n[1] * n[2];
  BPX_CHECK(boxes < (1ll << 31), "%s: %lld boxes per sample; 2^31 or more are not supported", fn, (long long)boxes);
  g.Z = Z; g.Y = Y; g.X = X;
  g.sz = s[0]; g.sy = s[1]; g.sx = s[2];
  g.nz = n[0]; g.ny = n[1]; g.nx = n[2];
  g.rz = r[0]; g.ry = r[1]; g.rx = r[2];
  g.manip = cfg->manipulator;
  return 0;
}

}  // namespace

extern "C" int64_t bpx_n2v_boxes(const bpx_n2v_cfg* cfg, int Z, int Y, int X) {
  N2VGeom g;
  int64_t boxes = 0;
  return n2v_geom("bpx_n2v_boxes", cfg, Z, Y, X, g, boxes) ? -1 : boxes;
}

extern "C" int bpx_n2v_mask(const float* x_d, int B, int Z, int Y, int X, int C, const bpx_n2v_cfg* cfg, uint64_t* state_d, float* x_out_d,
                            float* target_d, int32_t* coords_d, int32_t* sources_d, bpx_stream_t stream) {
  const char* fn = "bpx_n2v_mask";
  BPX_CHECK(x_d && cfg && state_d && x_out_d && target_d && coords_d && sources_d, "%s: null pointer", fn);
  BPX_CHECK(B > 0 && B < (1 << 24), "%s: 1 to 2^24 - 1 samples (got %d)", fn, B);
  BPX_CHECK(C >= 1 && C <= N2V_MAX_CHANNELS, "%s: 1..%d channels (got %d)", fn, N2V_MAX_CHANNELS, C);
  N2VGeom g;
  int64_t boxes = 0;
  if (n2v_geom(fn, cfg, Z, Y, X, g, boxes)) return 1;
  BPX_CHECK((((uintptr_t)x_d | (uintptr_t)x_out_d | (uintptr_t)target_d | (uintptr_t)coords_d | (uintptr_t)sources_d) & 3) == 0 && ((uintptr_t)state_d & 7) == 0,
            "%s: tensors must be 4-byte aligned, the state 8-byte aligned", fn);
  const int64_t V = (int64_t)Z * Y * X, n = (int64_t)B * V * C, total = (int64_t)B * C * boxes;
  BPX_CHECK(!spans_overlap(x_d, n * 4, x_out_d, n * 4) && !spans_overlap(x_d, n * 4, target_d, n * 8) && !spans_overlap(x_out_d, n * 4, target_d, n * 8),
            "%s: the outputs overlap the input or each other: the masking reads the input and cannot run in place", fn);
  BPX_CHECK(cdiv64(total, 256) < (1ll << 31), "%s: %lld boxes exceed one launch", fn, (long long)total);
  const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>(1, cdiv64(n * 3 / 4, 256 * 4)), 256 * 32);
  n2v_stream_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(reinterpret_cast<const uint32_t*>(x_d), reinterpret_cast<uint32_t*>(x_out_d), n,
                                                             reinterpret_cast<uint32_t*>(target_d), 2 * n, state_d);
  BPX_LAUNCH_CHECK(fn);
  n2v_sparse_kernel<<<(unsigned)cdiv64(total, 256), 256, 0, (hipStream_t)stream>>>(x_d, g, C, boxes, total, cfg->seed, cfg->sigma, state_d, x_out_d, target_d,
                                                                                    coords_d, sources_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_n2v_loss_blocks(int64_t voxels) { return loss_blocks(voxels); }

static int n2v_loss_args(const char* fn, int N, int C, int64_t voxels) {
  BPX_CHECK(N > 0 && C >= 1 && C <= N2V_MAX_CHANNELS && voxels > 0, "%s: bad extents (N %d, C %d, voxels %lld; 1..%d channels)", fn, N, C, (long long)voxels,
            N2V_MAX_CHANNELS);
  BPX_CHECK((int64_t)N * C <= 65535, "%s: N * C = %lld planes exceed one launch", fn, (long long)N * C);
  return 0;
}

extern "C" int bpx_n2v_loss_sums(const float* pred_d, const float* target_d, int N, int C, int64_t voxels, float* partials_d, bpx_stream_t stream) {
  const char* fn = "bpx_n2v_loss_sums";
  BPX_CHECK(pred_d && target_d && partials_d, "%s: null pointer", fn);
  if (n2v_loss_args(fn, N, C, voxels)) return 1;
  dim3 grid((unsigned)bpx_n2v_loss_blocks(voxels), (unsigned)(N * C));
  n2v_loss_sums_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(pred_d, target_d, voxels, C, partials_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_n2v_loss_finish(const float* partials_d, int N, int C, int64_t voxels, float* out_d, bpx_stream_t stream) {
  const char* fn = "bpx_n2v_loss_finish";
  BPX_CHECK(partials_d && out_d, "%s: null pointer", fn);
  if (n2v_loss_args(fn, N, C, voxels)) return 1;
  n2v_loss_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>(partials_d, (int64_t)N * C * bpx_n2v_loss_blocks(voxels), out_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_n2v_loss_bwd(const float* pred_d, const float* target_d, int N, int C, int64_t voxels, const float* saved_d, const float* gup_d,
                                float* dpred_d, bpx_stream_t stream) {
  const char* fn = "bpx_n2v_loss_bwd";
  BPX_CHECK(pred_d && target_d && saved_d && gup_d && dpred_d, "%s: null pointer", fn);
  if (n2v_loss_args(fn, N, C, voxels)) return 1;
  dim3 grid((unsigned)bpx_n2v_loss_blocks(voxels), (unsigned)(N * C));
  n2v_loss_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(pred_d, target_d, voxels, C, saved_d, gup_d, dpred_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
