// Dice and Dice + cross-entropy losses of heads with 2..8 channels (biapy_amd/losses.py states the definitions), as three streaming launches per
// loss call whatever N, batch_dice or the CE weight are:
//   sums   : grid (blocks, N); one softmax (class mode) or C sigmoids (channel mode) per voxel, I = sum p t, P = sum p, T = sum t per class plus the
//            CE / BCE sums and the count of labels outside [0, C); wave shuffle, four waves through LDS, ONE row per (sample, block); no atomics
//   finish : one workgroup; the rows in a fixed order in double -> the loss, the backward's coefficients a0 / a1 per class (or per sample and
//            class) and the CE normaliser, and the batch totals
//   bwd    : dlogits from the logits, the target, the coefficients and the upstream gradient, all read on the device
// Logits are planar fp32 (N, C, voxels) - what bpx_head_fwd writes.  Class mode: target (N, 1, voxels) class ids as floats, p = softmax over the
// channels; channel mode: target (N, C, voxels), p = sigmoid per channel.  The kernels are instantiated per channel count: the 3 C + 4 sums of a
// thread and the C loaded planes of a 4-voxel group are registers with compile-time indices (no scratch: profiles/kernel_resources.txt).
// The wave sum, the four-wave hand-over, the sigmoid / BCE terms, the finish's row sum and the block rule are loss_parts.h's, shared with the plain
// losses (seg, per-channel, softmax CE: plain_losses.hip) and the N2V loss (n2v.hip).
#include "loss_parts.h"

constexpr int DICE_MAXC = 8, DICE_ROW = 3 * DICE_MAXC + 4;
// columns of a row: I[8], P[8], T[8], {sum w nll | sum bce}, sum w, labels outside [0, C) other than ignore_index, counted voxels
constexpr int DR_I = 0, DR_P = DICE_MAXC, DR_T = 2 * DICE_MAXC, DR_CE = 3 * DICE_MAXC, DR_W = DR_CE + 1, DR_FAULT = DR_CE + 2, DR_CNT = DR_CE + 3;
// coefficients written by finish: coef[0] = w_ce / (sum w | numel) (0 when w_ce == 0), then per group g (one, or one per sample) at coef + 8 + 16 g:
// a0[8], a1[8], both times w_dice
constexpr int DICE_COEF_HEAD = 8, DICE_COEF_GROUP = 2 * DICE_MAXC;

template <int C> struct DiceAcc { float I[C], P[C], T[C], ce, w, faults, cnt; };

// softmax of one voxel: e[c] = exp(z[c] - max), returns (max, sum e)
template <int C> __device__ __forceinline__ void dice_softmax(const float (&z)[C], float (&e)[C], float& m, float& se) {
  m = z[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
  se = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) { e[c] = expf(z[c] - m); se += e[c]; }
}

template <int C>
__device__ __forceinline__ void dice_class_voxel(const float (&z)[C], float lab, int ignore_index, const float (&w)[C], bool with_ce, DiceAcc<C>& a) {
  const int y = (int)lab;
  const bool in_range = y >= 0 && y < C, counted = in_range && y != ignore_index;
  a.faults += (!in_range && y != ignore_index) ? 1.f : 0.f;
  a.cnt += counted ? 1.f : 0.f;
  float e[C], m, se;
  dice_softmax<C>(z, e, m, se);
  const float inv = 1.f / se;
  float zy = 0.f, wy = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float p = e[c] * inv;
    const bool is_y = counted && c == y;
    a.P[c] += counted ? p : 0.f;
    a.I[c] += is_y ? p : 0.f;
    a.T[c] += is_y ? 1.f : 0.f;
    zy = is_y ? z[c] : zy;
    wy = is_y ? w[c] : wy;
  }
  if (with_ce) {
    const float nll = (m + logf(se)) - zy;
    a.ce += counted ? wy * nll : 0.f;
    a.w += wy;                                  // 0 for an uncounted voxel
  }
}

template <int C>
__device__ __forceinline__ void dice_chan_voxel(const float (&z)[C], const float (&t)[C], bool with_ce, DiceAcc<C>& a) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float en;
    const float p = sigmoid_rcp(z[c], en);
    a.I[c] += p * t[c];
    a.P[c] += p;
    a.T[c] += t[c];
    if (with_ce) a.ce += bce_less_log(z[c], t[c]) + log1pf(en);
  }
}

// VEC: voxels % 4 == 0 and 16-byte aligned pointers - a thread walks groups of four voxels with one 16-byte load per plane; otherwise one voxel
// per step with dword loads (coalesced across the wave either way).  With voxels % 4 != 0 the planes of a sample start at different offsets modulo
// 16 bytes, so no 16-byte body exists that is aligned in every plane: such a tensor (a ragged patch) takes the dword path over ALL of its data -
// four load instructions where the other path issues one, the same bytes and the same full 256-byte lines per wave.  Its cost is not measured
// (scripts/dice_loss_timing.py times 128^3 patches, which take the 16-byte path); patch sizes of the reference's templates are multiples of 4.
template <int C, bool CLASS, bool VEC>
__global__ void __launch_bounds__(256) dice_sums_kernel(const float* __restrict__ z, const float* __restrict__ t, int64_t vox, int ignore_index,
                                                        const float* __restrict__ cw, int with_ce, float* __restrict__ part) {
  const int n = blockIdx.y;
  const float* zp = z + (size_t)n * C * vox;
  const float* tp = t + (size_t)n * (CLASS ? 1 : C) * vox;
  float w[C];
#pragma unroll
  for (int c = 0; c < C; ++c) w[c] = (CLASS && cw) ? cw[c] : 1.f;
  DiceAcc<C> a;
#pragma unroll
  for (int c = 0; c < C; ++c) a.I[c] = a.P[c] = a.T[c] = 0.f;
  a.ce = a.w = a.faults = a.cnt = 0.f;
  const bool ce = with_ce != 0;
  if (VEC) {
    const int64_t n4 = vox / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
      f32x4_t zv[C], tv[CLASS ? 1 : C];
#pragma unroll
      for (int c = 0; c < C; ++c) zv[c] = reinterpret_cast<const f32x4_t*>(zp + (size_t)c * vox)[i];
#pragma unroll
      for (int c = 0; c < (CLASS ? 1 : C); ++c) tv[c] = reinterpret_cast<const f32x4_t*>(tp + (size_t)c * vox)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float zc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) zc[c] = zv[c][e];
        if (CLASS) {
          dice_class_voxel<C>(zc, tv[0][e], ignore_index, w, ce, a);
        } else {
          float tc[C];
#pragma unroll
          for (int c = 0; c < C; ++c) tc[c] = tv[CLASS ? 0 : c][e];
          dice_chan_voxel<C>(zc, tc, ce, a);
        }
      }
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < vox; i += (int64_t)gridDim.x * 256) {
      float zc[C];
#pragma unroll
      for (int c = 0; c < C; ++c) zc[c] = zp[(size_t)c * vox + i];
      if (CLASS) {
        dice_class_voxel<C>(zc, tp[i], ignore_index, w, ce, a);
      } else {
        float tc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) tc[c] = tp[(size_t)c * vox + i];
        dice_chan_voxel<C>(zc, tc, ce, a);
      }
    }
  }
  __shared__ float red[4][DICE_ROW];
  float row[DICE_ROW];
#pragma unroll
  for (int c = 0; c < DICE_MAXC; ++c) {     // the columns of the channels beyond C are zeros
    row[DR_I + c] = row[DR_P + c] = row[DR_T + c] = 0.f;
    if (c < C) { row[DR_I + c] = wave_sum(a.I[c < C ? c : 0]); row[DR_P + c] = wave_sum(a.P[c < C ? c : 0]); row[DR_T + c] = wave_sum(a.T[c < C ? c : 0]); }
  }
  row[DR_CE] = wave_sum(a.ce); row[DR_W] = wave_sum(a.w); row[DR_FAULT] = wave_sum(a.faults); row[DR_CNT] = wave_sum(a.cnt);
  four_wave_hand_over(row, red);
  if (threadIdx.x < DICE_ROW) part[((size_t)n * gridDim.x + blockIdx.x) * DICE_ROW + threadIdx.x] = four_wave_sum_pairs(red, threadIdx.x);
}

// One workgroup.  Per sample: the sample's rows through rows_sum_8x32 (loss_parts.h) - a fixed order.  Dice per
// class from the batch totals (batch_dice) or from every sample's totals; M = the number of dice terms averaged.
//   a0 = w_dice (2 I + s) / (M (U + s)^2),  a1 = a0 - 2 w_dice / (M (U + s)),  U = P + T
//   loss = w_ce CE + w_dice (1 - sum dice / M), a term whose weight is 0 is not formed
__global__ void __launch_bounds__(256) dice_finish_kernel(const float* __restrict__ part, int N, int nb, int C, int class_mode, int batch_dice, double numel,
                                                          double w_ce, double w_dice, double smooth, double* __restrict__ sums, float* __restrict__ coef,
                                                          float* __restrict__ loss) {
  __shared__ double red[8][32];
  __shared__ double S[32];
  __shared__ double dsh[DICE_MAXC];
  const int tid = threadIdx.x;
  const double M = batch_dice ? (double)C : (double)N * C;
  double tot = 0., dice_sum = 0.;
  auto terms = [&](int g) {           // threads 0..C-1: the dice term and the coefficients of group g from S
    const double I = S[DR_I + tid], U = S[DR_P + tid] + S[DR_T + tid];
    const double num = 2. * I + smooth, den = U + smooth;
    const double a0 = w_dice * num / (M * den * den);
    float* cg = coef + DICE_COEF_HEAD + (size_t)g * DICE_COEF_GROUP;
    cg[tid] = (float)a0;
    cg[DICE_MAXC + tid] = (float)(a0 - 2. * w_dice / (M * den));
    dsh[tid] = num / den;
  };
  for (int n = 0; n < N; ++n) {
    const double v = rows_sum_8x32<DICE_ROW>(part + (size_t)n * nb * DICE_ROW, nb, red);
    if (tid < DICE_ROW) {
      S[tid] = v;
      tot += v;
    }
    __syncthreads();
    if (!batch_dice) {
      if (tid < C) terms(n);
      __syncthreads();
      if (tid == 0)
        for (int c = 0; c < C; ++c) dice_sum += dsh[c];
    }
  }
  __syncthreads();
  if (tid < DICE_ROW) { sums[tid] = tot; S[tid] = tot; }
  __syncthreads();
  if (batch_dice) {
    if (tid < C) terms(0);
    __syncthreads();
    if (tid == 0)
      for (int c = 0; c < C; ++c) dice_sum += dsh[c];
  }
  if (tid == 0) {
    double v = 0., kce = 0.;
    if (w_dice != 0.) v += w_dice * (1. - dice_sum / M);
    if (w_ce != 0.) {
      const double den = class_mode ? S[DR_W] : numel;       // every label ignored: 0 / 0 = NaN, as torch's mean reduction
      v += w_ce * S[DR_CE] / den;
      kce = w_ce / den;
    }
    coef[0] = (float)kce;
    *loss = (float)v;
  }
}

// class mode:   dz[c] = g (p_c (A_c - sum_k p_k A_k) + kce w[y] (p_c - [c == y])) on counted voxels, A_c = a1[c] where c == y and a0[c] elsewhere; 0 on the rest
// channel mode: dz[c] = g (A_c p_c (1 - p_c) + kce (p_c - t_c)),  A_c = a0[c] + t_c (a1[c] - a0[c])
template <int C>
__device__ __forceinline__ void dice_class_bwd_voxel(const float (&z)[C], float lab, int ignore_index, const float (&w)[C], const float (&a0)[C],
                                                     const float (&a1)[C], float kce, float g, float (&out)[C]) {
  const int y = (int)lab;
  const bool counted = y >= 0 && y < C && y != ignore_index;
  float e[C], m, se;
  dice_softmax<C>(z, e, m, se);
  const float inv = 1.f / se;
  float A[C], s = 0.f, wy = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    e[c] *= inv;
    A[c] = c == y ? a1[c] : a0[c];
    wy = c == y ? w[c] : wy;
    s += e[c] * A[c];
  }
  const float kc = kce * wy;
#pragma unroll
  for (int c = 0; c < C; ++c) out[c] = counted ? g * (e[c] * (A[c] - s) + kc * (e[c] - (c == y ? 1.f : 0.f))) : 0.f;
}

__device__ __forceinline__ float dice_chan_bwd(float z, float t, float a0, float a1, float kce, float g) {
  float en;
  const float p = sigmoid_rcp(z, en);
  const float A = a0 + t * (a1 - a0);
  return g * (A * (p * (1.f - p)) + kce * (p - t));
}

template <int C, bool CLASS, bool VEC>
__global__ void __launch_bounds__(256) dice_bwd_kernel(const float* __restrict__ z, const float* __restrict__ t, int64_t vox, int ignore_index,
                                                       const float* __restrict__ cw, const float* __restrict__ coef, int per_sample,
                                                       const float* __restrict__ gup, float* __restrict__ dz) {
  const int n = blockIdx.y;
  const float* zp = z + (size_t)n * C * vox;
  const float* tp = t + (size_t)n * (CLASS ? 1 : C) * vox;
  float* dp = dz + (size_t)n * C * vox;
  const float g = gup[0], kce = coef[0];
  const float* cg = coef + DICE_COEF_HEAD + (per_sample ? (size_t)n * DICE_COEF_GROUP : 0);
  float w[C], a0[C], a1[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { w[c] = (CLASS && cw) ? cw[c] : 1.f; a0[c] = cg[c]; a1[c] = cg[DICE_MAXC + c]; }
  if (VEC) {
    const int64_t n4 = vox / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
      f32x4_t zv[C], tv[CLASS ? 1 : C], ov[C];
#pragma unroll
      for (int c = 0; c < C; ++c) zv[c] = reinterpret_cast<const f32x4_t*>(zp + (size_t)c * vox)[i];
#pragma unroll
      for (int c = 0; c < (CLASS ? 1 : C); ++c) tv[c] = reinterpret_cast<const f32x4_t*>(tp + (size_t)c * vox)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (CLASS) {
          float zc[C], oc[C];
#pragma unroll
          for (int c = 0; c < C; ++c) zc[c] = zv[c][e];
          dice_class_bwd_voxel<C>(zc, tv[0][e], ignore_index, w, a0, a1, kce, g, oc);
#pragma unroll
          for (int c = 0; c < C; ++c) ov[c][e] = oc[c];
        } else {
#pragma unroll
          for (int c = 0; c < C; ++c) ov[c][e] = dice_chan_bwd(zv[c][e], tv[CLASS ? 0 : c][e], a0[c], a1[c], kce, g);
        }
      }
#pragma unroll
      for (int c = 0; c < C; ++c) reinterpret_cast<f32x4_t*>(dp + (size_t)c * vox)[i] = ov[c];
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < vox; i += (int64_t)gridDim.x * 256) {
      float zc[C], oc[C];
#pragma unroll
      for (int c = 0; c < C; ++c) zc[c] = zp[(size_t)c * vox + i];
      if (CLASS) {
        dice_class_bwd_voxel<C>(zc, tp[i], ignore_index, w, a0, a1, kce, g, oc);
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) oc[c] = dice_chan_bwd(zc[c], tp[(size_t)c * vox + i], a0[c], a1[c], kce, g);
      }
#pragma unroll
      for (int c = 0; c < C; ++c) dp[(size_t)c * vox + i] = oc[c];
    }
  }
}

// ---- C-ABI -----------------------------------------------------------------------------------------------------------------------------------------
static inline bool dice_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

#define DICE_ARGS_OK(fn)                                                                                                                      \
  BPX_CHECK(N > 0 && N <= 65535 && C >= 2 && C <= DICE_MAXC && voxels > 0, "%s: 2 <= C <= %d channels, 1 <= N <= 65535", fn, DICE_MAXC)

// KERNEL<C, CLASS, VEC> for the run-time (C, class_mode, vec)
#define DICE_DISPATCH_MODE(KERNEL, CC, ...)                                                       \
  do {                                                                                            \
    if (class_mode) { if (vec) KERNEL<CC, true, true> __VA_ARGS__; else KERNEL<CC, true, false> __VA_ARGS__; }     \
    else { if (vec) KERNEL<CC, false, true> __VA_ARGS__; else KERNEL<CC, false, false> __VA_ARGS__; }              \
  } while (0)
#define DICE_DISPATCH(KERNEL, ...)                                  \
  switch (C) {                                                      \
    case 2: DICE_DISPATCH_MODE(KERNEL, 2, __VA_ARGS__); break;      \
    case 3: DICE_DISPATCH_MODE(KERNEL, 3, __VA_ARGS__); break;      \
    case 4: DICE_DISPATCH_MODE(KERNEL, 4, __VA_ARGS__); break;      \
    case 5: DICE_DISPATCH_MODE(KERNEL, 5, __VA_ARGS__); break;      \
    case 6: DICE_DISPATCH_MODE(KERNEL, 6, __VA_ARGS__); break;      \
    case 7: DICE_DISPATCH_MODE(KERNEL, 7, __VA_ARGS__); break;      \
    default: DICE_DISPATCH_MODE(KERNEL, 8, __VA_ARGS__); break;     \
  }

extern "C" int bpx_dice_blocks(int64_t voxels) { return loss_blocks(voxels); }
extern "C" int bpx_dice_row(void) { return DICE_ROW; }

extern "C" int bpx_dice_sums(const float* logits_d, const float* target_d, int N, int C, int64_t voxels, int class_mode, int ignore_index,
                             const float* class_w_d, int with_ce, float* partials_d, bpx_stream_t stream) {
  const char* fn = "bpx_dice_sums";
  BPX_CHECK(logits_d && target_d && partials_d, "%s: null pointer", fn);
  DICE_ARGS_OK(fn);
  BPX_CHECK(class_mode || !class_w_d, "%s: class weights belong to the class mode's cross entropy", fn);
  const bool vec = voxels % 4 == 0 && dice_aligned16(logits_d) && dice_aligned16(target_d);
  dim3 grid((unsigned)bpx_dice_blocks(voxels), (unsigned)N);
  DICE_DISPATCH(dice_sums_kernel, <<<grid, 256, 0, (hipStream_t)stream>>>(logits_d, target_d, voxels, ignore_index, class_w_d, with_ce, partials_d));
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_dice_finish(const float* partials_d, int N, int C, int64_t voxels, int class_mode, int batch_dice, double w_ce, double w_dice,
                               double smooth, double* sums_d, float* coef_d, float* loss_d, bpx_stream_t stream) {
  const char* fn = "bpx_dice_finish";
  BPX_CHECK(partials_d && sums_d && coef_d && loss_d, "%s: null pointer", fn);
  DICE_ARGS_OK(fn);
  dice_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>(partials_d, N, bpx_dice_blocks(voxels), C, class_mode, batch_dice, (double)N * C * (double)voxels,
                                                         w_ce, w_dice, smooth, sums_d, coef_d, loss_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_dice_bwd(const float* logits_d, const float* target_d, int N, int C, int64_t voxels, int class_mode, int batch_dice, int ignore_index,
                            const float* class_w_d, const float* coef_d, const float* gup_d, float* dlogits_d, bpx_stream_t stream) {
  const char* fn = "bpx_dice_bwd";
  BPX_CHECK(logits_d && target_d && coef_d && gup_d && dlogits_d, "%s: null pointer", fn);
  DICE_ARGS_OK(fn);
  BPX_CHECK(class_mode || !class_w_d, "%s: class weights belong to the class mode's cross entropy", fn);
  const bool vec = voxels % 4 == 0 && dice_aligned16(logits_d) && dice_aligned16(target_d) && dice_aligned16(dlogits_d);
  const int64_t items = vec ? voxels / 4 : voxels;
  dim3 grid((unsigned)std::min<int64_t>(cdiv64(items, 256), 1024), (unsigned)N);
  const int per_sample = batch_dice ? 0 : 1;
  DICE_DISPATCH(dice_bwd_kernel, <<<grid, 256, 0, (hipStream_t)stream>>>(logits_d, target_d, voxels, ignore_index, class_w_d, coef_d, per_sample, gup_d,
                                                                          dlogits_d));
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
