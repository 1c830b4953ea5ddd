// A 256-thread block's sum of one value per thread: wave shuffle, then the four waves through LDS.  Shared by the loss kernels (loss_parts.h), the
// kernels at the two ends of a network (ends.hip) and the rank-1 tail of the pool backward (elementwise.hip).  The two orders of the four-wave sum
// differ in the last bit of an fp32 total, so each stays under its own name and a call site keeps the one it has.
#pragma once
#include "bpx_common.h"

__device__ __forceinline__ float wave_sum(float v) {   // every lane receives the wave's total
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}
// lane 0 of each wave hands the wave's ROW sums over: red[wave][k] = v[k]; the block meets behind it
template <int ROW> __device__ __forceinline__ void four_wave_hand_over(const float (&v)[ROW], float (&red)[4][ROW]) {
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < ROW; ++k) red[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
}
// the four wave values of column k: left to right (seg, chan, N2V; head, rank-1 and up-sampling gradients) or in pairs (softmax CE, Dice; the
// pool backward's rank-1 tail) - fp32, the two differ in the last bit
template <int ROW> __device__ __forceinline__ float four_wave_sum_seq(const float (&red)[4][ROW], int k) { return red[0][k] + red[1][k] + red[2][k] + red[3][k]; }
template <int ROW> __device__ __forceinline__ float four_wave_sum_pairs(const float (&red)[4][ROW], int k) { return (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]); }
