// The pieces the loss kernels share (plain_losses.hip: seg / chan / softmax CE; losses.hip: Dice; n2v.hip: masked MSE), each written once and
// inlined: no classes, no dispatch.  What differs between the families in the last bit stays apart under its own name: two sigmoid forms, two
// orders of the four-wave sum (block_sums.h); seg takes log(1 + en) from seg_log1p_unit, chan and Dice from log1pf.  Every kernel here runs 256
// threads.
#pragma once
#include <algorithm>

#include "block_sums.h"
#include "bpx_common.h"

// blocks per plane of the streaming sums kernels (chan, softmax CE, Dice, N2V): 1024 voxels per block, 512 blocks (= partial rows) at the most
static inline int loss_blocks(int64_t voxels) { return (int)std::min<int64_t>(std::max<int64_t>(1, cdiv64(voxels, 1024)), 512); }

// ---- per element: p = sigmoid(z) and en = exp(-|z|) with it; BCE with logits = max(z, 0) - z t + log(1 + en) ------------------------------
// one reciprocal, the negative side a product (seg sums, Dice) | a division on either side (seg backward, chan): they round differently
__device__ __forceinline__ float sigmoid_rcp(float z, float& en) {
  en = expf(-fabsf(z));
  const float r = 1.f / (1.f + en);
  return z >= 0.f ? r : en * r;
}
__device__ __forceinline__ float sigmoid_div(float z, float& en) {
  en = expf(-fabsf(z));
  return z >= 0.f ? 1.f / (1.f + en) : en / (1.f + en);
}
__device__ __forceinline__ float bce_less_log(float z, float t) { return fmaxf(z, 0.f) - z * t; }   // the caller adds its log(1 + en)

// log(1 + e) for e in [0, 1] (e = exp(-|z|)): v_log_f32 of the rounded sum.  Absolute error <= ~1e-7 per element (the rounding of 1 + e and one ulp of
// the hardware log2) against ocml's log1pf - three orders of magnitude below the fp32 summation that follows - at a tenth of its instructions: the
// kernel was VALU-bound at 40 us per step on ~150 instructions per element (a wave64 VALU instruction occupies its SIMD for four cycles), 67 MB of
// traffic need 13.
__device__ __forceinline__ float seg_log1p_unit(float e) { return __builtin_amdgcn_logf(1.f + e) * 0.69314718055994531f; }
// one element of the seg sums: s = { bce, p t, p, t, |P & T|, |P | T| }, P = p > 0.5, T = t > 0.5
__device__ __forceinline__ void seg_accumulate(float z, float t, float (&s)[6]) {
  float en;
  const float p = sigmoid_rcp(z, en);
  s[0] += bce_less_log(z, t) + seg_log1p_unit(en);
  s[1] += p * t; s[2] += p; s[3] += t;
  const bool P = p > 0.5f, T = t > 0.5f;
  s[4] += (P && T) ? 1.f : 0.f; s[5] += (P || T) ? 1.f : 0.f;
}
// one element of the seg backward: dz = a (p - t) - p (1 - p) (b t - c)
__device__ __forceinline__ float seg_grad(float z, float t, float a, float b, float c) {
  float en;
  const float p = sigmoid_div(z, en);
  return a * (p - t) - p * (1.f - p) * (b * t - c);
}

// ---- one-workgroup finish reductions of fp32 partials in double, every addition in a fixed order ----------------------------------------------
// Column threadIdx.x (< ROW <= 32) of `rows` rows of ROW partials: eight row lanes x 32 columns (lane l adds rows l, l + 8, ...), then the eight
// lanes in sequence.  The other threads return 0.  The caller sets a barrier before red is written again.
template <int ROW, int LD> __device__ __forceinline__ double rows_sum_8x32(const float* __restrict__ part, int rows, double (&red)[8][LD]) {
  const int k = threadIdx.x % 32, lr = threadIdx.x / 32;
  double a = 0., v = 0.;
  if (k < ROW)
    for (int r = lr; r < rows; r += 8) a += (double)part[(size_t)r * ROW + k];
  if (k < LD) red[lr][k] = a;
  __syncthreads();
  if (threadIdx.x < ROW)
    for (int q = 0; q < 8; ++q) v += red[q][threadIdx.x];
  return v;
}
// K sums of `count` terms each: thread t adds term(k, q) for q = t, t + 256, ...; then thread 0 adds the 256 thread sums in sequence -> out[k]
// (thread 0 only; 0 elsewhere).  Count: the callers' own index type.  The caller sets a barrier before red is written again.
template <int K, typename Count, class Term>
__device__ __forceinline__ void strided_sums_256(Count count, Term term, double (&red)[K][256], double (&out)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = 0.;
    for (Count q = threadIdx.x; q < count; q += 256) s += (double)term(k, q);
    red[k][threadIdx.x] = s;
    out[k] = 0.;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int q = 0; q < 256; ++q)
#pragma unroll
      for (int k = 0; k < K; ++k) out[k] += red[k][q];
}
