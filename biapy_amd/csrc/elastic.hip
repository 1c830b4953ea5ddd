// Elastic deformation of the device augmenter (step 0b of biapy_amd/augment.py, which states the semantics; include/biapy_amd.h the record and
// the field): the draw of a sample's alpha, the uniform noise of the displacement field, and the gather of image and target through the
// smoothed field.  The smoothing between the last two is bpx_sepfilter (sepfilter.hip), unchanged.  The per-voxel arithmetic - coordinate,
// clamp, border rule, taps, interpolation - is augment_core.h's, shared with the affine warp of augment.hip.
//
// Random numbers: Philox4x32-10 (philox.h).  The draw: key = seed, counter words (sample, 24, c low, c high), c = the call's counter value out of
// words 5-6 of the sample's augmentation record; r0 fires, r1 is alpha's uniform.  The noise: key (seed low ^ 0x454C4153, seed high) - no other
// stream shares it - counter words (q low, q high ^ (sample << 8), c low, c high), q = element / 4, element = linear (plane, y, x) index within
// the sample's field; word j of the block serves element 4 q + j.
#include "bpx_common.h"
#include "philox.h"
#include "augment_core.h"

namespace {

constexpr int AREC = BPX_AUG_REC_WORDS, EREC = BPX_ELASTIC_REC_WORDS;

__global__ void __launch_bounds__(256) elastic_draw_kernel(uint64_t seed, uint64_t thr, float a_lo, float a_hi, int B, const uint32_t* __restrict__ rec,
                                                           uint32_t* __restrict__ el) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint32_t cl = rec[(size_t)b * AREC + BPX_AUG_W_CTR], ch = rec[(size_t)b * AREC + BPX_AUG_W_CTR + 1];
  uint32_t r[4];
  philox4x32_10((uint32_t)b, (uint32_t)BPX_ELASTIC_STREAM, cl, ch, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  const bool fired = (uint64_t)r[0] < thr;
  const float alpha = fired ? aug_uniform(r[1], a_lo, a_hi) : 0.f;
  u32x4_t* dst = reinterpret_cast<u32x4_t*>(el + (size_t)b * EREC);
  dst[0] = u32x4_t{fired ? BPX_ELASTIC_F_FIRED : 0u, __float_as_uint(alpha), cl, ch};
  dst[1] = u32x4_t{0u, 0u, 0u, 0u};
}

// thread i = (sample, q): one Philox block, the four elements 4 q .. 4 q + 3 of the sample's n-element field (nq = ceil(n / 4) blocks per sample)
__global__ void __launch_bounds__(256) elastic_noise_kernel(uint64_t seed, int B, int64_t n, int64_t nq, const uint32_t* __restrict__ el,
                                                            float* __restrict__ field) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * nq) return;
  const int b = (int)(i / nq);
  const int64_t q = i - (int64_t)b * nq;
  const uint32_t cl = el[(size_t)b * EREC + BPX_ELASTIC_W_CTR], ch = el[(size_t)b * EREC + BPX_ELASTIC_W_CTR + 1];
  uint32_t r[4];
  philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32) ^ ((uint32_t)b << 8), cl, ch, (uint32_t)seed ^ BPX_ELASTIC_KEY_XOR, (uint32_t)(seed >> 32), r);
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = (float)(r[j] >> 8) * 5.9604644775390625e-8f * 2.f - 1.f;
  float* dst = field + (int64_t)b * n + 4 * q;
  if (4 * q + 4 <= n && ((uintptr_t)dst & 15) == 0) {
    *reinterpret_cast<f32x4_t*>(dst) = f32x4_t{v[0], v[1], v[2], v[3]};
  } else {                                                       // the tail of a sample, or a sample that starts off a 16-byte boundary
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * q + j < n) dst[j] = v[j];
  }
}

// One workgroup = one (sample, run of up to EZ consecutive z, ET x ET tile of (Y, X)) of the OUTPUT, never two samples: flags and alpha are
// uniform over it.  Phase 1: one thread per (y, x) of the tile loads the voxel's two displacement words once and leaves its taps
// (augment_core.h: elastic_voxel) in LDS.  Phase 2, after ONE barrier: for every z of the run, consecutive lanes walk consecutive output
// elements (x, c) of a row and read the voxel's taps from LDS - the same words for all C + Ct channels and all z of the run - then the source
// with plain loads.  Offsets into the batch are 64-bit; an index within a plane is below 2^30 (the field has fewer than 2^31 elements).
constexpr int ET = 32, EZ = 8, EVOX = ET * ET;
struct ElasticGeom { int Z, Y, X, tiles_x, tiles_y, zruns; };

template <typename TT, int MODE>
__global__ void __launch_bounds__(256) elastic_apply_kernel(const float* __restrict__ x, const TT* __restrict__ t, ElasticGeom g, int C, int Ct,
                                                            const uint32_t* __restrict__ el, const float* __restrict__ field, float cval,
                                                            float* __restrict__ xo, TT* __restrict__ to) {
  __shared__ int s_o00[EVOX], s_o01[EVOX], s_o10[EVOX], s_o11[EVOX], s_on[EVOX];
  __shared__ float s_wx[EVOX], s_wy[EVOX];
  __shared__ uint32_t s_mask[EVOX];
  const int tiles = g.tiles_x * g.tiles_y;
  const int64_t per_sample = (int64_t)g.zruns * tiles;
  const int b = (int)((int64_t)blockIdx.x / per_sample);
  const int rest = (int)((int64_t)blockIdx.x - (int64_t)b * per_sample);
  const int zr = rest / tiles, tile = rest % tiles;
  const int z0 = zr * EZ, nz = min(EZ, g.Z - z0);
  const int yo0 = (tile / g.tiles_x) * ET, xo0 = (tile % g.tiles_x) * ET;
  const int nyo = min(ET, g.Y - yo0), nxo = min(ET, g.X - xo0);
  const int Y = g.Y, X = g.X;
  const int64_t plane_vox = (int64_t)Y * X;

  const uint32_t flags = el[(size_t)b * EREC + BPX_ELASTIC_W_FLAGS];
  if (flags) {                                                     // uniform over the workgroup
    const float alpha = __uint_as_float(el[(size_t)b * EREC + BPX_ELASTIC_W_ALPHA]);
    const float* sy = field + (int64_t)b * 2 * plane_vox;
    const float* sx = sy + plane_vox;
    const int py = max(2 * Y - 2, 1), px = max(2 * X - 2, 1);
    for (int v = threadIdx.x; v < nyo * ET; v += 256) {
      const int r = v / ET, xl = v % ET;
      if (xl < nxo) {
        const int y = yo0 + r, xv = xo0 + xl;
        const int o = y * X + xv;
        const ElasticTaps tp = elastic_voxel<MODE>(y, xv, alpha, sy[o], sx[o], Y, X, py, px);
        s_o00[v] = tp.o00; s_o01[v] = tp.o01; s_o10[v] = tp.o10; s_o11[v] = tp.o11; s_on[v] = tp.on;
        s_wx[v] = tp.wx; s_wy[v] = tp.wy; s_mask[v] = tp.mask;
      }
    }
    __syncthreads();
  }

  const float rcp_c = 1.f / (float)C, rcp_ct = 1.f / (float)Ct;
  for (int zz = 0; zz < nz; ++zz) {
    const int64_t plane = ((int64_t)b * g.Z + z0 + zz) * plane_vox;   // the sample's z plane, in voxels: source and destination alike
    const float* xs = x + plane * C;
    const TT* ts = t + plane * Ct;
    // ---- image ----
    {
      const int ipr = nxo * C, items = nyo * ipr;                  // < 2^15 items, rows of at most 2^9 elements: small_div is exact
      const float rcp = 1.f / (float)ipr;
      for (int i = threadIdx.x; i < items; i += 256) {
        const int r = small_div(i, rcp), e = i - r * ipr;
        const int xl = C == 1 ? e : small_div(e, rcp_c), c = e - xl * C;
        const int64_t dst = ((int64_t)(yo0 + r) * X + xo0 + xl) * C + c;
        float out;
        if (!flags) {
          out = xs[dst];
        } else {
          const int v = r * ET + xl;
          float v00 = xs[(int64_t)s_o00[v] * C + c], v01 = xs[(int64_t)s_o01[v] * C + c];
          float v10 = xs[(int64_t)s_o10[v] * C + c], v11 = xs[(int64_t)s_o11[v] * C + c];
          if constexpr (MODE == BPX_WARP_CONSTANT) {
            const uint32_t m = s_mask[v];
            v00 = m & 1u ? v00 : cval; v01 = m & 2u ? v01 : cval;
            v10 = m & 4u ? v10 : cval; v11 = m & 8u ? v11 : cval;
          }
          out = warp_lerp(v00, v01, v10, v11, s_wx[v], s_wy[v]);
        }
        xo[plane * C + dst] = out;
      }
    }
    // ---- target: the nearest voxel ----
    {
      const int ipr = nxo * Ct, items = nyo * ipr;
      const float rcp = 1.f / (float)ipr;
      for (int i = threadIdx.x; i < items; i += 256) {
        const int r = small_div(i, rcp), e = i - r * ipr;
        const int xl = Ct == 1 ? e : small_div(e, rcp_ct), c = e - xl * Ct;
        const int64_t dst = ((int64_t)(yo0 + r) * X + xo0 + xl) * Ct + c;
        TT out;
        if (!flags) {
          out = ts[dst];
        } else {
          const int v = r * ET + xl;
          out = ts[(int64_t)s_on[v] * Ct + c];
          if constexpr (MODE == BPX_WARP_CONSTANT) out = s_mask[v] & ELASTIC_IN_NEAREST ? out : (TT)0;
        }
        to[plane * Ct + dst] = out;
      }
    }
  }
}

template <typename TT>
void launch_elastic(int mode, unsigned blocks, hipStream_t s, const float* x, const TT* t, ElasticGeom g, int C, int Ct, const uint32_t* el,
                    const float* field, float cval, float* xo, TT* to) {
  if (mode == BPX_WARP_CONSTANT) elastic_apply_kernel<TT, BPX_WARP_CONSTANT><<<blocks, 256, 0, s>>>(x, t, g, C, Ct, el, field, cval, xo, to);
  else if (mode == BPX_WARP_REFLECT) elastic_apply_kernel<TT, BPX_WARP_REFLECT><<<blocks, 256, 0, s>>>(x, t, g, C, Ct, el, field, cval, xo, to);
  else elastic_apply_kernel<TT, BPX_WARP_EDGE><<<blocks, 256, 0, s>>>(x, t, g, C, Ct, el, field, cval, xo, to);
}

// [a, a + na) and [b, b + nb) share a byte
bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

}  // namespace

extern "C" int bpx_elastic_draw(uint64_t seed, uint64_t thr, float alpha_lo, float alpha_hi, int B, const uint32_t* records_d, uint32_t* elastic_d,
                                bpx_stream_t stream) {
  const char* fn = "bpx_elastic_draw";
  BPX_CHECK(records_d && elastic_d, "%s: null pointer", fn);
  BPX_CHECK(B > 0, "%s: bad extents", fn);
  BPX_CHECK(((uintptr_t)elastic_d & 15) == 0 && ((uintptr_t)records_d & 3) == 0, "%s: elastic records must be 16-byte aligned", fn);
  BPX_CHECK(thr <= (1ull << 32), "%s: thr above 2^32", fn);
  BPX_CHECK(alpha_lo >= 0.f && alpha_lo <= alpha_hi && alpha_hi <= BPX_ELASTIC_ALPHA_MAX, "%s: the alpha range must satisfy 0 <= lo <= hi <= 1024", fn);
  elastic_draw_kernel<<<cdiv(B, 256), 256, 0, (hipStream_t)stream>>>(seed, thr, alpha_lo, alpha_hi, B, records_d, elastic_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_elastic_noise(uint64_t seed, int B, int Y, int X, const uint32_t* elastic_d, float* field_d, bpx_stream_t stream) {
  const char* fn = "bpx_elastic_noise";
  BPX_CHECK(elastic_d && field_d, "%s: null pointer", fn);
  BPX_CHECK(B > 0 && Y > 0 && X > 0, "%s: bad extents", fn);
  const int64_t n = 2 * (int64_t)Y * X;
  BPX_CHECK((int64_t)B * n < (1ll << 31), "%s: a field of %lld elements: 2^31 or more are not supported", fn, (long long)((int64_t)B * n));
  BPX_CHECK(((uintptr_t)field_d & 3) == 0 && ((uintptr_t)elastic_d & 3) == 0, "%s: the field must be 4-byte aligned", fn);
  const int64_t nq = cdiv64(n, 4);
  elastic_noise_kernel<<<(unsigned)cdiv64((int64_t)B * nq, 256), 256, 0, (hipStream_t)stream>>>(seed, B, n, nq, elastic_d, field_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_elastic_apply(const float* x_d, const void* t_d, int t_dtype, int B, int Z, int Y, int X, int C, int Ct, const uint32_t* elastic_d,
                                 const float* field_d, int mode, float cval, float* x_out_d, void* t_out_d, bpx_stream_t stream) {
  const char* fn = "bpx_elastic_apply";
  BPX_CHECK(x_d && t_d && elastic_d && field_d && x_out_d && t_out_d, "%s: null pointer", fn);
  BPX_CHECK(B > 0 && Z > 0 && Y > 0 && X > 0, "%s: bad extents", fn);
  const int64_t plane = (int64_t)Y * X, fe = 2 * (int64_t)B * plane;
  BPX_CHECK(fe < (1ll << 31), "%s: a field of %lld elements: 2^31 or more are not supported", fn, (long long)fe);
  BPX_CHECK(C >= 1 && C <= 16 && Ct >= 1 && Ct <= 8, "%s: 1..16 image channels and 1..8 target channels (got %d, %d)", fn, C, Ct);
  BPX_CHECK(t_dtype == BPX_F32 || t_dtype == BPX_U8, "%s: the target is float32 or uint8", fn);
  BPX_CHECK(mode == BPX_WARP_CONSTANT || mode == BPX_WARP_REFLECT || mode == BPX_WARP_EDGE, "%s: unknown border mode %d", fn, mode);
  BPX_CHECK(__builtin_isfinite(cval), "%s: cval must be finite", fn);
  const int64_t vox = (int64_t)B * Z * plane, xb = vox * C * 4, tb = vox * Ct * (int64_t)dtype_size(t_dtype);
  const struct { const void* p; int64_t n; } ins[4] = {{x_d, xb}, {t_d, tb}, {field_d, fe * 4}, {elastic_d, (int64_t)B * EREC * 4}};
  for (const auto& in : ins)
    BPX_CHECK(!overlap(x_out_d, xb, in.p, in.n) && !overlap(t_out_d, tb, in.p, in.n), "%s: out overlaps an input: the pass is a gather and cannot run in place", fn);
  BPX_CHECK(!overlap(x_out_d, xb, t_out_d, tb), "%s: the two outputs overlap", fn);
  ElasticGeom g;
  g.Z = Z; g.Y = Y; g.X = X;
  g.tiles_x = cdiv(X, ET); g.tiles_y = cdiv(Y, ET); g.zruns = cdiv(Z, EZ);
  const int64_t blocks = (int64_t)B * g.zruns * g.tiles_x * g.tiles_y;
  BPX_CHECK(blocks < (1ll << 31), "%s: %lld tiles exceed one launch", fn, (long long)blocks);
  if (t_dtype == BPX_F32)
    launch_elastic<float>(mode, (unsigned)blocks, (hipStream_t)stream, x_d, (const float*)t_d, g, C, Ct, elastic_d, field_d, cval, x_out_d, (float*)t_out_d);
  else
    launch_elastic<uint8_t>(mode, (unsigned)blocks, (hipStream_t)stream, x_d, (const uint8_t*)t_d, g, C, Ct, elastic_d, field_d, cval, x_out_d,
                            (uint8_t*)t_out_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
