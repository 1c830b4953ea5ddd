// The plain losses on fp32 logits (biapy_amd/losses.py states the definitions), each as streaming sums -> a one-workgroup finish in double -> backward:
//   seg        (bpx_seg_loss_*)    binary segmentation on the 1-channel head: BCE with logits, Dice and the IoU@0.5 counts from one row of six sums
//   chan       (bpx_chan_loss_*)   per-channel BCE / MSE / L1 of a multi-channel head behind its training-time activation, a weighted mean
//   softmax CE (bpx_softmax_ce_*)  multi-class cross entropy with ignore_index and class weights, and the per-class IoU counts
// No atomics: fp32 partials per block in a fixed order.  The shared pieces are in loss_parts.h; Dice / Dice + CE live in losses.hip.
#include "loss_parts.h"

// ------------------------------------------------------------------------------------------------
// Binary segmentation loss on the 1-channel head (metrics.py:493-586 CrossEntropyLoss_wrapper -> BCEWithLogits,
// :726-762 DiceLoss with batch_dice, :764-973 DiceCELoss) and the IoU@0.5 counts (:138-232), one streaming pass each way.
//   sums[b] = { sum bce, sum p*t, sum p, sum t, |P&T|, |P|T| }  per block b, p = sigmoid(z), P = p > 0.5, T = t > 0.5
//   backward: dz = a (p - t) - p (1 - p) (b t - c), (a, b, c) from the reduced sums (see losses.py)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) seg_loss_sums_kernel(const float* __restrict__ z, const float* __restrict__ t, int64_t n,
                                                            float* __restrict__ part) {
  float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const f32x4_t zv = reinterpret_cast<const f32x4_t*>(z)[i], tv = reinterpret_cast<const f32x4_t*>(t)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) seg_accumulate(zv[e], tv[e], s);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) seg_accumulate(z[n4 * 4 + threadIdx.x], t[n4 * 4 + threadIdx.x], s);  // tail
  __shared__ float red[4][6];
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = wave_sum(s[k]);
  four_wave_hand_over(s, red);
  if (threadIdx.x < 6) part[(size_t)blockIdx.x * 6 + threadIdx.x] = four_wave_sum_seq(red, threadIdx.x);
}

__global__ void __launch_bounds__(256) seg_loss_bwd_kernel(const float* __restrict__ z, const float* __restrict__ t, int64_t n,
                                                           const float* __restrict__ coef, float* __restrict__ dz) {
  const float a = coef[0], b = coef[1], c = coef[2];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dz[i] = seg_grad(z[i], t[i], a, b, c);
}

// The scalar tail of the loss on the device, in ONE block each way (round 3: it was ~25 float64 PyTorch element-wise launches inside the
// captured step).  finish: the partial rows are summed in a fixed order in double (thread k owns rows k, k + 256, ...; then a fixed-order
// combination of the 256 thread sums) -> sums[6] (double) and loss = w_ce * S0 / n + w_dice * (1 - (2 S1 + smooth) / (S2 + S3 + smooth)).
__global__ void __launch_bounds__(256) seg_loss_finish_kernel(const float* __restrict__ part, int blocks, double n, double w_ce, double w_dice,
                                                              double smooth, double* __restrict__ sums, float* __restrict__ loss) {
  __shared__ double red[256][6];
  double s[6] = {0., 0., 0., 0., 0., 0.};
  for (int b = threadIdx.x; b < blocks; b += 256)
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] += (double)part[(size_t)b * 6 + k];
#pragma unroll
  for (int k = 0; k < 6; ++k) red[threadIdx.x][k] = s[k];
  __syncthreads();
  // two levels (16 groups of 16 rows, then the 16 group sums): 32 dependent LDS reads instead of 256
  __shared__ double red2[16][6];
  if (threadIdx.x < 96) {
    const int gq = threadIdx.x / 6, k = threadIdx.x % 6;
    double a = 0.;
    for (int q = gq; q < 256; q += 16) a += red[q][k];
    red2[gq][k] = a;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    double a = 0.;
    for (int q = 0; q < 16; ++q) a += red2[q][threadIdx.x];
    red[0][threadIdx.x] = a;
    sums[threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double inter = red[0][1], uni = red[0][2] + red[0][3];
    *loss = (float)(w_ce * red[0][0] / n + w_dice * (1.0 - (2.0 * inter + smooth) / (uni + smooth)));
  }
}

// backward with the three coefficients formed in the kernel from the saved sums and the upstream gradient (a 0-d device tensor)
__global__ void __launch_bounds__(256) seg_loss_bwd_fused_kernel(const float* __restrict__ z, const float* __restrict__ t, int64_t n,
                                                                 const double* __restrict__ sums, const float* __restrict__ gup, double w_ce,
                                                                 double w_dice, double smooth, float* __restrict__ dz) {
  const double g = (double)gup[0], den = sums[2] + sums[3] + smooth;
  const float a = (float)(w_ce * g / (double)n), b = (float)(2.0 * w_dice * g / den), c = (float)(w_dice * g * (2.0 * sums[1] + smooth) / (den * den));
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const f32x4_t zv = reinterpret_cast<const f32x4_t*>(z)[i], tv = reinterpret_cast<const f32x4_t*>(t)[i];
    f32x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = seg_grad(zv[e], tv[e], a, b, c);
    reinterpret_cast<f32x4_t*>(dz)[i] = o;
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) {
    const int64_t i = n4 * 4 + threadIdx.x;
    dz[i] = seg_grad(z[i], t[i], a, b, c);
  }
}

// per-channel losses: loss = sum_c w_c * (sum of the channel's partial sums) / (N * vox), partials [N][C][nb]; fixed-order double sums
__global__ void __launch_bounds__(256) chan_loss_finish_kernel(const float* __restrict__ part, int N, int C, int nb, double inv_count,
                                                               const float* __restrict__ weights, float* __restrict__ loss) {
  __shared__ double red[1][256];
  double total = 0., a[1];
  for (int c = 0; c < C; ++c) {
    strided_sums_256(N * nb, [&](int, int q) { return part[((size_t)(q / nb) * C + c) * nb + q % nb]; }, red, a);
    if (threadIdx.x == 0) total += a[0] * inv_count * (double)weights[c];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)total;
}

// ---- per-channel losses of a multi-channel head (instance segmentation: B, C, D ... channels) -----------------------------------
// biapy/engine/metrics.py:1418-1810 (instance_segmentation_loss, plain channels: no masks / re-balancing / border weights) composed
// with the training-time head activation of the workflow (base_workflow.py:1403-1457: ce_* channels stay logits, the 'D' channel
// goes through tanh - instance_seg.py:405-409).  code[c] = kind | act << 2, kind: 0 BCE-with-logits, 1 MSE, 2 L1; act (applied to
// the logit before MSE / L1): 0 linear, 1 tanh, 2 sigmoid.  Planar fp32 tensors [N][C][vox].
__device__ __forceinline__ float chan_act(float z, int act, float& dact) {
  if (act == 1) { const float y = tanhf(z); dact = 1.f - y * y; return y; }
  if (act == 2) { float en; const float p = sigmoid_div(z, en); dact = p * (1.f - p); return p; }
  dact = 1.f;
  return z;
}
__device__ __forceinline__ float chan_loss_term(float z, float t, int code, float& dz) {
  const int kind = code & 3, act = (code >> 2) & 3;
  if (kind == 0) {
    float en;
    dz = sigmoid_div(z, en) - t;
    return bce_less_log(z, t) + log1pf(en);
  }
  float da;
  const float d = chan_act(z, act, da) - t;
  if (kind == 1) { dz = 2.f * d * da; return d * d; }
  dz = (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f) * da;
  return fabsf(d);
}

// grid (blocks, N*C): partial sum of the loss terms of plane (n, c) per block -> part[(n*C + c) * gridDim.x + blockIdx.x]
__global__ void __launch_bounds__(256) chan_loss_sums_kernel(const float* __restrict__ z, const float* __restrict__ t, int64_t vox, int C,
                                                             unsigned codes, float* __restrict__ part) {
  const int plane = blockIdx.y, c = plane % C;
  const int code = (codes >> (4 * c)) & 15;
  const float* zp = z + (size_t)plane * vox;
  const float* tp = t + (size_t)plane * vox;
  float s[1] = {0.f}, dz;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < vox; i += (int64_t)gridDim.x * 256) s[0] += chan_loss_term(zp[i], tp[i], code, dz);
  s[0] = wave_sum(s[0]);
  __shared__ float red[4][1];
  four_wave_hand_over(s, red);
  if (threadIdx.x == 0) part[(size_t)plane * gridDim.x + blockIdx.x] = four_wave_sum_seq(red, 0);
}

// dlogits[n][c][v] = coef[c] * d term / d logit;  gup != null: coef[c] holds the channel WEIGHT and the kernel forms
// weight * upstream gradient * inv_count itself (no element-wise launches on the host side)
__global__ void __launch_bounds__(256) chan_loss_bwd_kernel(const float* __restrict__ z, const float* __restrict__ t, int64_t vox, int C,
                                                            unsigned codes, const float* __restrict__ coef, float* __restrict__ dzo,
                                                            const float* __restrict__ gup = nullptr, float inv_count = 1.f) {
  const int plane = blockIdx.y, c = plane % C;
  const int code = (codes >> (4 * c)) & 15;
  const float k = gup ? gup[0] * coef[c] * inv_count : coef[c];
  const size_t off = (size_t)plane * vox;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < vox; i += (int64_t)gridDim.x * 256) {
    float dz;
    chan_loss_term(z[off + i], t[off + i], code, dz);
    dzo[off + i] = k * dz;
  }
}

// ---- multi-class cross entropy (metrics.py:493-586 CrossEntropyLoss_wrapper with num_classes > 2 -> torch.nn.CrossEntropyLoss(ignore_index, weight),
// mean reduction: sum_v w[y_v] * (logsumexp_c z[v][c] - z[v][y_v]) / sum_v w[y_v] over the voxels whose label is not ignore_index) and the per-class
// counts of the multi-class IoU (:138-232: argmax prediction against the label map).  logits are planar (N, C, voxels) fp32 - what bpx_head_fwd
// writes -, the label map (N, 1, voxels) holds class ids as floats.  Row of partials per (sample, block): {sum w * nll, sum w, tp[8], pred[8], tgt[8]}.
constexpr int SCE_MAXC = 8, SCE_ROW = 2 + 3 * SCE_MAXC;
__device__ __forceinline__ int sce_label(float t, int C, int ignore_index) {   // class id, or -1 = not counted (ignore_index / outside [0, C))
  const int y = (int)t;
  return (y == ignore_index || y < 0 || y >= C) ? -1 : y;
}
__global__ void __launch_bounds__(256) softmax_ce_sums_kernel(const float* __restrict__ z, const float* __restrict__ t, int C, int64_t vox, int ignore_index,
                                                              const float* __restrict__ cw, float* __restrict__ part) {
  const int n = blockIdx.y;
  const float* zp = z + (size_t)n * C * vox;
  const float* tp = t + (size_t)n * vox;
  float s_nll = 0.f, s_w = 0.f, cnt[3][SCE_MAXC];
#pragma unroll
  for (int c = 0; c < SCE_MAXC; ++c) cnt[0][c] = cnt[1][c] = cnt[2][c] = 0.f;
  float w[SCE_MAXC];
#pragma unroll
  for (int c = 0; c < SCE_MAXC; ++c) w[c] = (cw && c < C) ? cw[c] : 1.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < vox; i += (int64_t)gridDim.x * 256) {
    float zc[SCE_MAXC], m = -INFINITY;
    int am = 0;
#pragma unroll
    for (int c = 0; c < SCE_MAXC; ++c) {
      zc[c] = c < C ? zp[(size_t)c * vox + i] : -INFINITY;
      if (zc[c] > m) { m = zc[c]; am = c; }      // first maximum, as torch.argmax
    }
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < SCE_MAXC; ++c) se += c < C ? expf(zc[c] - m) : 0.f;
    const float lse = m + logf(se);
    const int y = sce_label(tp[i], C, ignore_index);
    if (y >= 0) {
#pragma unroll
      for (int c = 0; c < SCE_MAXC; ++c) {
        const bool is_y = c == y, is_p = c == am;
        if (is_y) { s_nll += w[c] * (lse - zc[c]); s_w += w[c]; }
        cnt[0][c] += (is_y && is_p) ? 1.f : 0.f; cnt[1][c] += is_p ? 1.f : 0.f; cnt[2][c] += is_y ? 1.f : 0.f;
      }
    }
  }
  __shared__ float red[4][SCE_ROW];
  float row[SCE_ROW] = {wave_sum(s_nll), wave_sum(s_w)};
#pragma unroll
  for (int k = 0; k < 3 * SCE_MAXC; ++k) row[2 + k] = wave_sum(cnt[k / SCE_MAXC][k % SCE_MAXC]);
  four_wave_hand_over(row, red);
  if (threadIdx.x < SCE_ROW) part[((size_t)n * gridDim.x + blockIdx.x) * SCE_ROW + threadIdx.x] = four_wave_sum_pairs(red, threadIdx.x);
}

// one workgroup: the rows summed in a fixed order in double; loss = sums[0] / sums[1] (NaN when every label is ignored, as torch's mean reduction)
__global__ void __launch_bounds__(256) softmax_ce_finish_kernel(const float* __restrict__ part, int rows, double* __restrict__ sums, float* __restrict__ loss) {
  __shared__ double red[8][SCE_ROW];
  const double v = rows_sum_8x32<SCE_ROW>(part, rows, red);        // 8 row lanes x 32 columns (26 used)
  if (threadIdx.x < SCE_ROW) {
    sums[threadIdx.x] = v;
    red[0][threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) *loss = (float)(red[0][0] / red[0][1]);
}

// dlogits[n][c][v] = gup * w[y] / sum_w * (softmax_c - [c == y]); 0 where the label is not counted
__global__ void __launch_bounds__(256) softmax_ce_bwd_kernel(const float* __restrict__ z, const float* __restrict__ t, int C, int64_t vox, int ignore_index,
                                                             const float* __restrict__ cw, const double* __restrict__ sums, const float* __restrict__ gup,
                                                             float* __restrict__ dz) {
  const int n = blockIdx.y;
  const float* zp = z + (size_t)n * C * vox;
  const float* tp = t + (size_t)n * vox;
  float* dp = dz + (size_t)n * C * vox;
  const float k0 = (float)((double)gup[0] / sums[1]);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < vox; i += (int64_t)gridDim.x * 256) {
    float zc[SCE_MAXC], m = -INFINITY;
#pragma unroll
    for (int c = 0; c < SCE_MAXC; ++c) {
      zc[c] = c < C ? zp[(size_t)c * vox + i] : -INFINITY;
      m = fmaxf(m, zc[c]);
    }
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < SCE_MAXC; ++c) { zc[c] = c < C ? expf(zc[c] - m) : 0.f; se += zc[c]; }
    const int y = sce_label(tp[i], C, ignore_index);
    const float k = y >= 0 ? k0 * (cw ? cw[y] : 1.f) : 0.f, inv = 1.f / se;
#pragma unroll
    for (int c = 0; c < SCE_MAXC; ++c)
      if (c < C) dp[(size_t)c * vox + i] = k * (zc[c] * inv - (c == y ? 1.f : 0.f));
  }
}

// ---- C-ABI -----------------------------------------------------------------------------------------------------------------------------------------
extern "C" int bpx_seg_loss_blocks(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>(1, cdiv64(n / 4, 256)), 2048); }

extern "C" int bpx_seg_loss_sums(const float* logits_d, const float* target_d, int64_t n, float* partials_d, bpx_stream_t stream) {
  const char* fn = "bpx_seg_loss_sums";
  BPX_CHECK(logits_d && target_d && partials_d, "%s: null pointer", fn);
  BPX_CHECK(n > 0, "%s: empty input", fn);
  BPX_CHECK((((uintptr_t)logits_d | (uintptr_t)target_d) & 15) == 0, "%s: logits and target must be 16-byte aligned", fn);
  seg_loss_sums_kernel<<<bpx_seg_loss_blocks(n), 256, 0, (hipStream_t)stream>>>(logits_d, target_d, n, partials_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_seg_loss_bwd(const float* logits_d, const float* target_d, int64_t n, const float* coef_d, float* dlogits_d,
                                bpx_stream_t stream) {
  const char* fn = "bpx_seg_loss_bwd";
  BPX_CHECK(logits_d && target_d && coef_d && dlogits_d, "%s: null pointer", fn);
  BPX_CHECK(n > 0, "%s: empty input", fn);
  seg_loss_bwd_kernel<<<grid_for(n), 256, 0, (hipStream_t)stream>>>(logits_d, target_d, n, coef_d, dlogits_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_seg_loss_finish(const float* partials_d, int blocks, int64_t n, float w_ce, float w_dice, float smooth, double* sums_d,
                                   float* loss_d, bpx_stream_t stream) {
  const char* fn = "bpx_seg_loss_finish";
  BPX_CHECK(partials_d && sums_d && loss_d && blocks > 0 && n > 0, "%s: bad arguments", fn);
  seg_loss_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>(partials_d, blocks, (double)n, (double)w_ce, (double)w_dice, (double)smooth, sums_d, loss_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_seg_loss_bwd_fused(const float* logits_d, const float* target_d, int64_t n, const double* sums_d, const float* gup_d, float w_ce,
                                      float w_dice, float smooth, float* dlogits_d, bpx_stream_t stream) {
  const char* fn = "bpx_seg_loss_bwd_fused";
  BPX_CHECK(logits_d && target_d && sums_d && gup_d && dlogits_d, "%s: null pointer", fn);
  BPX_CHECK(n > 0, "%s: empty input", fn);
  BPX_CHECK((((uintptr_t)logits_d | (uintptr_t)target_d | (uintptr_t)dlogits_d) & 15) == 0, "%s: tensors must be 16-byte aligned", fn);
  seg_loss_bwd_fused_kernel<<<grid_for(n / 4 + 1), 256, 0, (hipStream_t)stream>>>(logits_d, target_d, n, sums_d, gup_d, (double)w_ce, (double)w_dice,
                                                                                (double)smooth, dlogits_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_chan_loss_blocks(int64_t voxels) { return loss_blocks(voxels); }

extern "C" int bpx_chan_loss_sums(const float* logits_d, const float* target_d, int N, int C, int64_t voxels, unsigned codes, float* partials_d,
                                  bpx_stream_t stream) {
  const char* fn = "bpx_chan_loss_sums";
  BPX_CHECK(logits_d && target_d && partials_d, "%s: null pointer", fn);
  BPX_CHECK(N > 0 && C >= 1 && C <= 8 && voxels > 0, "%s: 1 <= C <= 8 channels", fn);
  for (int c = 0; c < C; ++c) BPX_CHECK(((codes >> (4 * c)) & 3) <= 2 && ((codes >> (4 * c + 2)) & 3) <= 2, "%s: bad code of channel %d", fn, c);
  dim3 grid((unsigned)loss_blocks(voxels), (unsigned)(N * C));
  chan_loss_sums_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(logits_d, target_d, voxels, C, codes, partials_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_chan_loss_bwd(const float* logits_d, const float* target_d, int N, int C, int64_t voxels, unsigned codes, const float* coef_d,
                                 float* dlogits_d, bpx_stream_t stream) {
  const char* fn = "bpx_chan_loss_bwd";
  BPX_CHECK(logits_d && target_d && coef_d && dlogits_d, "%s: null pointer", fn);
  BPX_CHECK(N > 0 && C >= 1 && C <= 8 && voxels > 0, "%s: 1 <= C <= 8 channels", fn);
  dim3 grid((unsigned)std::min<int64_t>(cdiv64(voxels, 256), 1024), (unsigned)(N * C));
  chan_loss_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(logits_d, target_d, voxels, C, codes, coef_d, dlogits_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_chan_loss_finish(const float* partials_d, int N, int C, int64_t voxels, const float* weights_d, float* loss_d, bpx_stream_t stream) {
  const char* fn = "bpx_chan_loss_finish";
  BPX_CHECK(partials_d && weights_d && loss_d && N > 0 && C > 0 && C <= 8, "%s: bad arguments", fn);
  chan_loss_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>(partials_d, N, C, loss_blocks(voxels), 1.0 / ((double)N * (double)voxels), weights_d, loss_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_chan_loss_bwd_fused(const float* logits_d, const float* target_d, int N, int C, int64_t voxels, unsigned codes, const float* weights_d,
                                       const float* gup_d, float* dlogits_d, bpx_stream_t stream) {
  const char* fn = "bpx_chan_loss_bwd_fused";
  BPX_CHECK(logits_d && target_d && weights_d && gup_d && dlogits_d, "%s: null pointer", fn);
  BPX_CHECK(N > 0 && C > 0 && C <= 8 && voxels > 0, "%s: bad shape", fn);
  dim3 grid((unsigned)loss_blocks(voxels), (unsigned)(N * C));
  chan_loss_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(logits_d, target_d, voxels, C, codes, weights_d, dlogits_d, gup_d,
                                                              (float)(1.0 / ((double)N * (double)voxels)));
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_softmax_ce_blocks(int64_t voxels) { return loss_blocks(voxels); }
extern "C" int bpx_softmax_ce_row(void) { return SCE_ROW; }

extern "C" int bpx_softmax_ce_sums(const float* logits_d, const float* target_d, int N, int C, int64_t voxels, int ignore_index, const float* class_w_d,
                                   float* partials_d, bpx_stream_t stream) {
  const char* fn = "bpx_softmax_ce_sums";
  BPX_CHECK(logits_d && target_d && partials_d, "%s: null pointer", fn);
  BPX_CHECK(N > 0 && N <= 65535 && C >= 2 && C <= SCE_MAXC && voxels > 0, "%s: 2 <= C <= %d classes, 1 <= N <= 65535", fn, SCE_MAXC);
  dim3 grid((unsigned)loss_blocks(voxels), (unsigned)N);
  softmax_ce_sums_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(logits_d, target_d, C, voxels, ignore_index, class_w_d, partials_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_softmax_ce_finish(const float* partials_d, int N, int64_t voxels, double* sums_d, float* loss_d, bpx_stream_t stream) {
  const char* fn = "bpx_softmax_ce_finish";
  BPX_CHECK(partials_d && sums_d && loss_d && N > 0 && voxels > 0, "%s: bad arguments", fn);
  softmax_ce_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>(partials_d, N * loss_blocks(voxels), sums_d, loss_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_softmax_ce_bwd(const float* logits_d, const float* target_d, int N, int C, int64_t voxels, int ignore_index, const float* class_w_d,
                                  const double* sums_d, const float* gup_d, float* dlogits_d, bpx_stream_t stream) {
  const char* fn = "bpx_softmax_ce_bwd";
  BPX_CHECK(logits_d && target_d && sums_d && gup_d && dlogits_d, "%s: null pointer", fn);
  BPX_CHECK(N > 0 && N <= 65535 && C >= 2 && C <= SCE_MAXC && voxels > 0, "%s: 2 <= C <= %d classes, 1 <= N <= 65535", fn, SCE_MAXC);
  dim3 grid((unsigned)std::min<int64_t>(cdiv64(voxels, 256), 1024), (unsigned)N);
  softmax_ce_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(logits_d, target_d, C, voxels, ignore_index, class_w_d, sums_d, gup_d, dlogits_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
