// HBM-bound kernels around the convolutions: normalisation statistics and their finalizes (instance, group, batch norm), the norm backward,
// norm + activation with and without dropout, the channel affine, max-pooling, the attention gate and its MLP, weight packing, image packing,
// casts and a lane-layout self test.  The tensor kernels stream NDHWC tensors with 16-byte accesses along the channel axis.  The first layer, the
// SR "pre" up-sampling and the output head - tile and MFMA kernels - live in ends.hip.
#include <type_traits>

#include "block_sums.h"
#include "bpx_common.h"
#include "philox.h"

namespace {

template <typename T> __device__ __forceinline__ float elu_like(float u, int act) {
  return bpx_act_rt<std::is_same<T, float>::value>(u, act);
}

// ------------------------------------------------------------------------------------------------
// statistics
// ------------------------------------------------------------------------------------------------
// Partial arrays of the 128^3 levels have 4-16 K tiles per sample; one block per (sample, 16 channels) walking them is a
// latency chain (70 us for the transposed-conv statistics).  Above 1024 tiles a first pass with `nseg` blocks per
// (sample, channel group) sums `seg` consecutive tiles each, in double, and writes the result over the FIRST tile of its
// own segment (only that block reads the segment, so this is race-free and needs no scratch); the finalize kernels then
// read every seg-th tile.
__global__ void __launch_bounds__(1024) stats_compact_kernel(float* __restrict__ part, int tiles, int C, int seg) {
  __shared__ double red[2][64][16];
  const int n = blockIdx.y, c0 = blockIdx.x * 16, sg = blockIdx.z;
  const int c = threadIdx.x & 15, tl = threadIdx.x >> 4;
  const int t0 = sg * seg, t1 = min(tiles, t0 + seg);
  double s1 = 0.0, s2 = 0.0;
  if (c0 + c < C) {
    const float* pp = part + (size_t)n * tiles * 2 * C + c0 + c;
    for (int t = t0 + tl; t < t1; t += 64) {
      s1 += (double)pp[(size_t)t * 2 * C];
      s2 += (double)pp[(size_t)t * 2 * C + C];
    }
  }
  red[0][tl][c] = s1;
  red[1][tl][c] = s2;
  __syncthreads();   // every read of the segment is done
  // two levels, as lane_reduce below: eight lanes sum eight rows each, then 32 threads sum the eight (a chain of 16 dependent LDS reads instead of 64)
  double a = 0.0, b = 0.0;
  if (tl < 8)
    for (int t = tl; t < 64; t += 8) { a += red[0][t][c]; b += red[1][t][c]; }
  __syncthreads();
  if (tl < 8) { red[0][tl][c] = a; red[1][tl][c] = b; }
  __syncthreads();
  if (threadIdx.x < 32) {
    const int k = threadIdx.x >> 4, cc = threadIdx.x & 15;
    double s = 0.0;
    for (int t = 0; t < 8; ++t) s += red[k][t][cc];
    if (c0 + cc < C && t0 < tiles) part[((size_t)n * tiles + t0) * 2 * C + (size_t)k * C + c0 + cc] = (float)s;
  }
}

// returns the tile stride the finalize kernel has to use (1 = untouched)
static int compact_stats(float* part, int N, int tiles, int C, hipStream_t s) {
  if (tiles <= 1024) return 1;   // (1024 = LP_ROWS: the per-workgroup rows of the lean conv / fused backward kernels never need the extra pass)
  const int seg = cdiv(tiles, 32);
  dim3 grid((unsigned)cdiv(C, 16), (unsigned)N, (unsigned)cdiv(tiles, seg));
  stats_compact_kernel<<<grid, 1024, 0, s>>>(part, tiles, C, seg);
  return seg;
}

// part: [N][tiles][2][C].  One 1024-thread block per (n, CB-channel block): thread = (tile lane, channel); CB = 16, or the
// channels per group of a GroupNorm with wider groups (32 / 64), so that a group never straddles two blocks.
__device__ __forceinline__ void tile_sums(const float* __restrict__ pp, int C, int nt, size_t ts, int tl, int lanes, double& s1, double& s2) {
  // `lanes` tile lanes x 4 independent loads in flight per thread: the partial arrays have up to 16K tiles
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
  int t = tl;
  // (round 6) eight rows per lane requested at once where there are that many - the 64^3 levels have 1024 rows, 16 per lane: four dependent L2 round
  // trips with four rows in flight, two with eight.  The additions are those of two rounds of the four-row loop below, in the same order: same bits.
  for (; t + 7 * lanes < nt; t += 8 * lanes) {
    float c0, c1, c2, c3, d0, d1, d2, d3;
    a0 = pp[(size_t)t * ts]; b0 = pp[(size_t)t * ts + C];
    a1 = pp[(size_t)(t + lanes) * ts]; b1 = pp[(size_t)(t + lanes) * ts + C];
    a2 = pp[(size_t)(t + 2 * lanes) * ts]; b2 = pp[(size_t)(t + 2 * lanes) * ts + C];
    a3 = pp[(size_t)(t + 3 * lanes) * ts]; b3 = pp[(size_t)(t + 3 * lanes) * ts + C];
    c0 = pp[(size_t)(t + 4 * lanes) * ts]; d0 = pp[(size_t)(t + 4 * lanes) * ts + C];
    c1 = pp[(size_t)(t + 5 * lanes) * ts]; d1 = pp[(size_t)(t + 5 * lanes) * ts + C];
    c2 = pp[(size_t)(t + 6 * lanes) * ts]; d2 = pp[(size_t)(t + 6 * lanes) * ts + C];
    c3 = pp[(size_t)(t + 7 * lanes) * ts]; d3 = pp[(size_t)(t + 7 * lanes) * ts + C];
    s1 += ((double)a0 + (double)a1) + ((double)a2 + (double)a3);
    s2 += ((double)b0 + (double)b1) + ((double)b2 + (double)b3);
    s1 += ((double)c0 + (double)c1) + ((double)c2 + (double)c3);
    s2 += ((double)d0 + (double)d1) + ((double)d2 + (double)d3);
  }
  for (; t + 3 * lanes < nt; t += 4 * lanes) {
    a0 = pp[(size_t)t * ts]; b0 = pp[(size_t)t * ts + C];
    a1 = pp[(size_t)(t + lanes) * ts]; b1 = pp[(size_t)(t + lanes) * ts + C];
    a2 = pp[(size_t)(t + 2 * lanes) * ts]; b2 = pp[(size_t)(t + 2 * lanes) * ts + C];
    a3 = pp[(size_t)(t + 3 * lanes) * ts]; b3 = pp[(size_t)(t + 3 * lanes) * ts + C];
    s1 += ((double)a0 + (double)a1) + ((double)a2 + (double)a3);
    s2 += ((double)b0 + (double)b1) + ((double)b2 + (double)b3);
  }
  for (; t < nt; t += lanes) {
    s1 += (double)pp[(size_t)t * ts];
    s2 += (double)pp[(size_t)t * ts + C];
  }
}

// block-wide reduction over the tile lanes: red[k][0 .. cb) holds the channel totals afterwards (all barriers are uniform)
// Two levels (round 6): eight groups of tile lanes first (lane tl sums tl, tl + 8, ...), then the eight group sums.  One level - 2 cb threads walking
// all 64 lanes - was a chain of 64 dependent LDS reads, ~2.7 of the ~5 us these kernels take, and a training step launches 38 of them (a forward 21).
// Fixed order, fp64: the totals differ from the one-level sum in the last bit of a double at most.
__device__ __forceinline__ void lane_reduce(double (*red)[1024], int cb, int lanes, double s1, double s2) {
  red[0][threadIdx.x] = s1;
  red[1][threadIdx.x] = s2;
  __syncthreads();
  int rows = lanes;
  if (lanes >= 16) {                                      // (lanes = 1024 / cb: a power of two)
    constexpr int G = 8;
    const int tl = threadIdx.x / cb, c = threadIdx.x % cb;
    double a = 0.0, b = 0.0;
    if (tl < G)
      for (int t = tl; t < lanes; t += G) { a += red[0][t * cb + c]; b += red[1][t * cb + c]; }
    __syncthreads();                                      // every lane is read before rows 0 .. G - 1 are overwritten
    if (tl < G) { red[0][threadIdx.x] = a; red[1][threadIdx.x] = b; }
    __syncthreads();
    rows = G;
  }
  const bool mine = (int)threadIdx.x < 2 * cb;
  const int k = mine ? threadIdx.x / cb : 0, cc = mine ? threadIdx.x % cb : 0;
  double s = 0.0;
  if (mine)
    for (int t = 0; t < rows; ++t) s += red[k][t * cb + cc];
  __syncthreads();                                        // every total is read before any is overwritten
  if (mine) red[k][cc] = s;
  __syncthreads();
}

__global__ void __launch_bounds__(1024) norm_finalize_kernel(const float* __restrict__ part, int tiles, int tstride, int C, double inv_count,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                            int cpg /* channels per group */, int cb, bpx_norm_rec* __restrict__ out,
                                                            int out_ld, int out_off) {
  __shared__ double red[2][1024];
  const int lanes = 1024 / cb;
  const int n = blockIdx.y, c0 = blockIdx.x * cb;
  const int c = threadIdx.x % cb, tl = threadIdx.x / cb;
  double s1 = 0.0, s2 = 0.0;
  if (c0 + c < C)
    tile_sums(part + (size_t)n * tiles * 2 * C + c0 + c, C, (tiles + tstride - 1) / tstride, (size_t)tstride * 2 * C, tl, lanes, s1, s2);
  lane_reduce(red, cb, lanes, s1, s2);
  if ((int)threadIdx.x < cb && c0 + (int)threadIdx.x < C) {
    const int cc = threadIdx.x;
    double m, v;
    if (cpg == 1) {
      m = red[0][cc] * inv_count;
      v = red[1][cc] * inv_count - m * m;
    } else {  // GroupNorm: a group lies inside this block (cpg divides cb)
      const int gb = (cc / cpg) * cpg;
      double a = 0.0, b = 0.0;
      for (int q = 0; q < cpg; ++q) { a += red[0][gb + q]; b += red[1][gb + q]; }
      m = a * inv_count / cpg;
      v = b * inv_count / cpg - m * m;
    }
    if (v < 0.0) v = 0.0;
    float rstd = (float)(1.0 / sqrt(v + (double)eps));
    float ga = gamma ? gamma[c0 + cc] : 1.f, be = beta ? beta[c0 + cc] : 0.f;
    bpx_norm_rec r;
    r.mean = (float)m; r.rstd = rstd; r.scale = ga * rstd; r.shift = be - (float)m * ga * rstd;
    out[(size_t)n * out_ld + out_off + c0 + cc] = r;
  }
}

template <typename T>
__global__ void __launch_bounds__(64) tensor_stats_kernel(const T* __restrict__ x, int ld, int C, int64_t vps, int tiles,
                                                          float* __restrict__ part) {
  const int n = blockIdx.y, tile = blockIdx.x;
  const int64_t v0 = (int64_t)tile * 256, v1 = min(v0 + 256, vps);
  for (int c = threadIdx.x; c < C; c += 64) {
    float s1 = 0.f, s2 = 0.f;
    for (int64_t v = v0; v < v1; ++v) {
      float f = ElemTraits<T>::ld(x + ((size_t)n * vps + v) * ld + c);
      s1 += f; s2 += f * f;
    }
    part[(((size_t)n * tiles + tile) * 2 + 0) * C + c] = s1;
    part[(((size_t)n * tiles + tile) * 2 + 1) * C + c] = s2;
  }
}

// the same partials with 16-byte accesses: thread = (voxel slot, channel vector), the slots of a vector are summed through LDS in a
// fixed order.  The one-channel-per-lane kernel above keeps 16 of 64 lanes busy at C = 16 and walks its 256 voxels serially
// (0.24 ms for a 4 x 1000 x 256 tensor: 16 blocks of one wave); this one is 5-20x faster on the small tensors of ResUNet++.
template <typename T>
__global__ void __launch_bounds__(256) tensor_stats_vec_kernel(const T* __restrict__ x, int ld, int C, int64_t vps, int tiles,
                                                               float* __restrict__ part) {
  constexpr int VEC = ElemTraits<T>::KPL;
  __shared__ float red[2][256][VEC];
  const int n = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
  const int CV = C / VEC, slots = 256 / CV;
  const int cv = t % CV, vs = t / CV;
  const int64_t v0 = (int64_t)tile * 256, v1 = min(v0 + 256, vps);
  float s1[VEC], s2[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) s1[e] = s2[e] = 0.f;
  if (vs < slots)
    for (int64_t v = v0 + vs; v < v1; v += slots) {
      const u32x4_t raw = *reinterpret_cast<const u32x4_t*>(x + ((size_t)n * vps + v) * ld + cv * VEC);
      float f[VEC];
      unpack16<T>(raw, f);
#pragma unroll
      for (int e = 0; e < VEC; ++e) { s1[e] += f[e]; s2[e] += f[e] * f[e]; }
    }
#pragma unroll
  for (int e = 0; e < VEC; ++e) { red[0][t][e] = s1[e]; red[1][t][e] = s2[e]; }
  __syncthreads();
  for (int c = t; c < 2 * C; c += 256) {
    const int which = c / C, ch = c % C;
    float a = 0.f;
    for (int k = 0; k < slots; ++k) a += red[which][k * CV + ch / VEC][ch % VEC];
    part[(((size_t)n * tiles + tile) * 2 + which) * C + ch] = a;
  }
}

// InstanceNorm / GroupNorm backward finalize.  red: [N][tiles][2][C] partials of S1 = sum_v g, S2 = sum_v g*xhat per channel
// (g = dL/dy of the normalised tensor, xhat = (t - mean)*rstd with the GROUP's statistics).  With m1 = mean over the group of
// gamma*g and m2 = mean over the group of gamma*g*xhat (group = Cg channels x M voxels; Cg = 1 is InstanceNorm):
//   dx = rstd * (gamma*g - m1 - xhat*m2) = a*g + b*t + c0,  a = gamma*rstd, b = -rstd^2*m2, c0 = -rstd*m1 + rstd^2*mean*m2
//   dgamma[c] += sum_n S2[n][c], dbeta[c] += sum_n S1[n][c]
// One block per channel block walks the samples in order, so the two parameter gradients are sums in a FIXED order written by a
// single thread: deterministic, no atomics.
// Round 3: NB samples at a time - thread = (sample slot, tile lane, channel) - instead of one sample after the other: the four samples of a
// cfg-2 batch were four dependent rounds of tile_sums + two block reductions (10.5 us average over the step's 17 launches).  The
// per-sample totals still enter dgamma / dbeta in sample order.
__global__ void __launch_bounds__(1024) norm_bwd_finalize_kernel(const float* __restrict__ red_part, int N, int tiles, int tstride, int C,
                                                                double inv_count, const bpx_norm_rec* __restrict__ rec,
                                                                const float* __restrict__ gamma, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta, int cpg, int cb, int NB, bpx_nbwd_coef* __restrict__ coef) {
  __shared__ double red[2][1024];
  __shared__ double tot[2][16][64];                       // [S1 | S2][sample slot][channel of the block]
  const int lanes = 1024 / (cb * NB);
  const int c0 = blockIdx.x * cb;
  const int c = threadIdx.x % cb, tl = (threadIdx.x / cb) % lanes, ns = threadIdx.x / (cb * lanes);
  double dg = 0.0, db = 0.0;
  for (int n0 = 0; n0 < N; n0 += NB) {
    const int n = n0 + ns;
    double s1 = 0.0, s2 = 0.0;
    if (c0 + c < C && n < N)
      tile_sums(red_part + (size_t)n * tiles * 2 * C + c0 + c, C, (tiles + tstride - 1) / tstride, (size_t)tstride * 2 * C, tl, lanes, s1, s2);
    red[0][threadIdx.x] = s1;
    red[1][threadIdx.x] = s2;
    __syncthreads();
    if (tl < 2) {                                         // two threads per (slot, channel): one total each, lanes in a fixed order
      double a = 0.0;
      for (int q = 0; q < lanes; ++q) a += red[tl][(ns * lanes + q) * cb + c];
      tot[tl][ns][c] = a;
    }
    __syncthreads();
    if (tl == 0 && c0 + c < C && n < N) {
      const int cc = c0 + c;
      const double S1 = tot[0][ns][c], S2 = tot[1][ns][c];
      const bpx_norm_rec r = rec[(size_t)n * C + cc];
      const double ga = gamma ? (double)gamma[cc] : 1.0;
      double m1, m2;
      if (cpg == 1) {
        m1 = ga * S1 * inv_count;
        m2 = ga * S2 * inv_count;
      } else {
        const int gb = (c / cpg) * cpg;
        double a1 = 0.0, a2 = 0.0;
        for (int q = 0; q < cpg; ++q) {
          const double gq = gamma ? (double)gamma[c0 + gb + q] : 1.0;
          a1 += gq * tot[0][ns][gb + q];
          a2 += gq * tot[1][ns][gb + q];
        }
        m1 = a1 * inv_count / cpg;
        m2 = a2 * inv_count / cpg;
      }
      const double rs = (double)r.rstd;
      bpx_nbwd_coef k;
      k.a = (float)(ga * rs);
      k.b = (float)(-rs * rs * m2);
      k.c0 = (float)(-rs * m1 + rs * rs * (double)r.mean * m2);
      k.pad = 0.f;
      coef[(size_t)n * C + cc] = k;
    }
    if (ns == 0 && tl == 0 && c0 + c < C) {               // dgamma / dbeta: the samples of this pass in index order
      for (int q = 0; q < NB && n0 + q < N; ++q) {
        dg += (double)(float)tot[1][q][c];                // the per-sample terms enter as floats, as they did with the former atomics
        db += (double)(float)tot[0][q][c];
      }
    }
    __syncthreads();                                      // red / tot are rewritten by the next pass
  }
  if (ns == 0 && tl == 0 && c0 + c < C) {
    const int cc = c0 + c;
    if (dgamma) dgamma[cc] += (float)dg;
    if (dbeta) dbeta[cc] += (float)db;
  }
}

// Deferred form (round 4): one block per (channel block, SAMPLE) instead of one per channel block walking the samples - the 768-4096 partial rows of
// a sample are a latency chain, four of them in one block cost 8.6 us per launch (17 launches per cfg-2 step).  What needs every sample, dgamma /
// dbeta, leaves the kernel: the block overwrites the first partial row of ITS sample (its own columns; nobody else reads them) with the sample's
// totals as floats - [S2 total (the dgamma term) | S1 total (the dbeta term)] - and the sum over the samples, in sample order, is queued with the
// step's weight-gradient reductions (bpxred::reduce_rows; the caller keeps red_part alive until the flush).
__global__ void __launch_bounds__(1024) norm_bwd_finalize_ps_kernel(float* __restrict__ red_part, int tiles, int tstride, int C, double inv_count,
                                                                   const bpx_norm_rec* __restrict__ rec, const float* __restrict__ gamma, int cpg, int cb,
                                                                   bpx_nbwd_coef* __restrict__ coef) {
  __shared__ double red[2][1024];
  const int lanes = 1024 / cb;
  const int n = blockIdx.y, c0 = blockIdx.x * cb;
  const int c = threadIdx.x % cb, tl = threadIdx.x / cb;
  double s1 = 0.0, s2 = 0.0;
  float* pn = red_part + (size_t)n * tiles * 2 * C;
  if (c0 + c < C) tile_sums(pn + c0 + c, C, (tiles + tstride - 1) / tstride, (size_t)tstride * 2 * C, tl, lanes, s1, s2);
  lane_reduce(red, cb, lanes, s1, s2);                    // red[0][0 .. cb) = S1, red[1][0 .. cb) = S2 of this sample; every partial row has been read
  if ((int)threadIdx.x < cb && c0 + (int)threadIdx.x < C) {
    const int cl = threadIdx.x, cc = c0 + cl;
    const double S1 = red[0][cl], S2 = red[1][cl];
    const bpx_norm_rec r = rec[(size_t)n * C + cc];
    const double ga = gamma ? (double)gamma[cc] : 1.0;
    double m1, m2;
    if (cpg == 1) {
      m1 = ga * S1 * inv_count;
      m2 = ga * S2 * inv_count;
    } else {
      const int gb = (cl / cpg) * cpg;
      double a1 = 0.0, a2 = 0.0;
      for (int q = 0; q < cpg; ++q) {
        const double gq = gamma ? (double)gamma[c0 + gb + q] : 1.0;
        a1 += gq * red[0][gb + q];
        a2 += gq * red[1][gb + q];
      }
      m1 = a1 * inv_count / cpg;
      m2 = a2 * inv_count / cpg;
    }
    const double rs = (double)r.rstd;
    bpx_nbwd_coef k;
    k.a = (float)(ga * rs);
    k.b = (float)(-rs * rs * m2);
    k.c0 = (float)(-rs * m1 + rs * rs * (double)r.mean * m2);
    k.pad = 0.f;
    coef[(size_t)n * C + cc] = k;
    pn[cc] = (float)S2;                                   // first partial row of the sample: [dgamma terms | dbeta terms]
    pn[C + cc] = (float)S1;
  }
}

// ---- GroupNorm with ANY group width, over a tensor that may be the concatenation of two producers' outputs (round 3) -------------------
// The decoder's first norm sees torch.cat([up, skip], 1): with 8 groups over 3 fm channels a group is 6 / 12 / 24 / 48 channels wide and one of
// them straddles the concat boundary, i.e. draws its statistics from the partial sums of TWO producer kernels.  Two small steps replace
// norm_finalize there: every producer's partials -> per-channel totals in one (N, C, 2) array of doubles (its columns at out_off), then one
// block per sample forms the group statistics from the channel totals and writes all C records.  The backward mirrors it.
__global__ void __launch_bounds__(1024) chan_sums_kernel(const float* __restrict__ part, int tiles, int tstride, int C, double* __restrict__ sums,
                                                        int out_ld, int out_off) {
  __shared__ double red[2][1024];
  const int cb = 16, lanes = 1024 / cb;
  const int n = blockIdx.y, c0 = blockIdx.x * cb;
  const int c = threadIdx.x % cb, tl = threadIdx.x / cb;
  double s1 = 0.0, s2 = 0.0;
  if (c0 + c < C)
    tile_sums(part + (size_t)n * tiles * 2 * C + c0 + c, C, (tiles + tstride - 1) / tstride, (size_t)tstride * 2 * C, tl, lanes, s1, s2);
  lane_reduce(red, cb, lanes, s1, s2);
  if ((int)threadIdx.x < cb && c0 + (int)threadIdx.x < C) {
    double* o = sums + ((size_t)n * out_ld + out_off + c0 + threadIdx.x) * 2;
    o[0] = red[0][threadIdx.x]; o[1] = red[1][threadIdx.x];
  }
}

__global__ void __launch_bounds__(512) gn_finalize_kernel(const double* __restrict__ sums, int C, double inv_count, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, int cpg, bpx_norm_rec* __restrict__ out) {
  const int n = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const int gb = (c / cpg) * cpg;
    double a = 0.0, b = 0.0;
    for (int q = 0; q < cpg; ++q) { a += sums[((size_t)n * C + gb + q) * 2]; b += sums[((size_t)n * C + gb + q) * 2 + 1]; }   // fixed order
    const double m = a * inv_count / cpg;
    double v = b * inv_count / cpg - m * m;
    if (v < 0.0) v = 0.0;
    const float rstd = (float)(1.0 / sqrt(v + (double)eps));
    const float ga = gamma ? gamma[c] : 1.f, be = beta ? beta[c] : 0.f;
    bpx_norm_rec r;
    r.mean = (float)m; r.rstd = rstd; r.scale = ga * rstd; r.shift = be - (float)m * ga * rstd;
    out[(size_t)n * C + c] = r;
  }
}

// sums: per-channel totals {S1 = sum g, S2 = sum g * xhat}; same formulas as norm_bwd_finalize_kernel; one block, the samples in index
// order, so that dgamma / dbeta are fixed-order sums (deterministic)
__global__ void __launch_bounds__(512) gn_bwd_finalize_kernel(const double* __restrict__ sums, int N, int C, double inv_count,
                                                             const bpx_norm_rec* __restrict__ rec, const float* __restrict__ gamma,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta, int cpg,
                                                             bpx_nbwd_coef* __restrict__ coef) {
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const int gb = (c / cpg) * cpg;
    const double ga = gamma ? (double)gamma[c] : 1.0;
    double dg = 0.0, db = 0.0;
    for (int n = 0; n < N; ++n) {
      double a1 = 0.0, a2 = 0.0;
      for (int q = 0; q < cpg; ++q) {
        const double gq = gamma ? (double)gamma[gb + q] : 1.0;
        a1 += gq * sums[((size_t)n * C + gb + q) * 2];
        a2 += gq * sums[((size_t)n * C + gb + q) * 2 + 1];
      }
      const double m1 = a1 * inv_count / cpg, m2 = a2 * inv_count / cpg;
      const bpx_norm_rec r = rec[(size_t)n * C + c];
      const double rs = (double)r.rstd;
      bpx_nbwd_coef k;
      k.a = (float)(ga * rs);
      k.b = (float)(-rs * rs * m2);
      k.c0 = (float)(-rs * m1 + rs * rs * (double)r.mean * m2);
      k.pad = 0.f;
      coef[(size_t)n * C + c] = k;
      db += (double)(float)sums[((size_t)n * C + c) * 2];
      dg += (double)(float)sums[((size_t)n * C + c) * 2 + 1];
    }
    if (dgamma) dgamma[c] += (float)dg;
    if (dbeta) dbeta[c] += (float)db;
  }
}

// ---- BatchNorm3d: the statistics of a channel are over the whole batch ---------------------------------------------------------------------
// One 1024-thread block per 16 channels, thread = (tile lane, channel).  A lane walks its tiles of sample 0, then of sample 1, ... into the same
// fp64 accumulators, and lane_reduce sums the lanes in a fixed order: the batch totals have a fixed summation order (bit-reproducible).
__device__ __forceinline__ void batch_sums(const float* __restrict__ part, int N, int tiles, int tstride, int C, int c0, double (*red)[1024]) {
  constexpr int cb = 16, lanes = 1024 / cb;
  const int c = threadIdx.x % cb, tl = threadIdx.x / cb;
  double s1 = 0.0, s2 = 0.0;
  if (c0 + c < C)
    for (int n = 0; n < N; ++n)
      tile_sums(part + (size_t)n * tiles * 2 * C + c0 + c, C, (tiles + tstride - 1) / tstride, (size_t)tstride * 2 * C, tl, lanes, s1, s2);
  lane_reduce(red, cb, lanes, s1, s2);
}

__global__ void __launch_bounds__(1024) bn_finalize_kernel(const float* __restrict__ part, int N, int tiles, int tstride, int C, double inv_count,
                                                          double unbias, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                          float momentum, float* __restrict__ rmean, float* __restrict__ rvar,
                                                          int64_t* __restrict__ nbt, bpx_norm_rec* __restrict__ out, int out_ld, int out_off) {
  __shared__ double red[2][1024];
  const int c0 = blockIdx.x * 16;
  batch_sums(part, N, tiles, tstride, C, c0, red);
  if ((int)threadIdx.x < 16 && c0 + (int)threadIdx.x < C) {
    const int cc = c0 + threadIdx.x;
    const double m = red[0][threadIdx.x] * inv_count;
    double v = red[1][threadIdx.x] * inv_count - m * m;
    if (v < 0.0) v = 0.0;
    const float rstd = (float)(1.0 / sqrt(v + (double)eps));
    const float ga = gamma ? gamma[cc] : 1.f, be = beta ? beta[cc] : 0.f;
    bpx_norm_rec r;
    r.mean = (float)m; r.rstd = rstd; r.scale = ga * rstd; r.shift = be - (float)m * ga * rstd;
    for (int n = 0; n < N; ++n) out[(size_t)n * out_ld + out_off + cc] = r;
    const double mo = (double)momentum;
    if (rmean) rmean[cc] = (float)((1.0 - mo) * (double)rmean[cc] + mo * m);
    if (rvar) rvar[cc] = (float)((1.0 - mo) * (double)rvar[cc] + mo * v * unbias);
  }
  if (nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;
}

// the formulas of norm_bwd_finalize_kernel (cpg = 1) with the batch totals; the coefficients are the same for every sample
__global__ void __launch_bounds__(1024) bn_bwd_finalize_kernel(const float* __restrict__ red_part, int N, int tiles, int tstride, int C,
                                                              double inv_count, const bpx_norm_rec* __restrict__ rec, const float* __restrict__ gamma,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta, bpx_nbwd_coef* __restrict__ coef) {
  __shared__ double red[2][1024];
  const int c0 = blockIdx.x * 16;
  batch_sums(red_part, N, tiles, tstride, C, c0, red);
  if ((int)threadIdx.x < 16 && c0 + (int)threadIdx.x < C) {
    const int cc = c0 + threadIdx.x;
    const double S1 = red[0][threadIdx.x], S2 = red[1][threadIdx.x];
    const bpx_norm_rec r = rec[cc];
    const double ga = gamma ? (double)gamma[cc] : 1.0;
    const double m1 = ga * S1 * inv_count, m2 = ga * S2 * inv_count, rs = (double)r.rstd;
    bpx_nbwd_coef k;
    k.a = (float)(ga * rs);
    k.b = (float)(-rs * rs * m2);
    k.c0 = (float)(-rs * m1 + rs * rs * (double)r.mean * m2);
    k.pad = 0.f;
    for (int n = 0; n < N; ++n) coef[(size_t)n * C + cc] = k;
    if (dgamma) dgamma[cc] += (float)S2;
    if (dbeta) dbeta[cc] += (float)S1;
  }
}

// eval mode: one block per BN layer of the network (blockIdx.x = job), records from the running statistics replicated to the N rows
struct BnEvalBatch { bpx_bn_eval_job job[64]; };

__global__ void __launch_bounds__(256) bn_eval_records_kernel(const BnEvalBatch b, int N) {
  const bpx_bn_eval_job j = b.job[blockIdx.x];
  for (int c = threadIdx.x; c < j.C; c += blockDim.x) {
    const float rm = j.running_mean_d[c];
    const float rstd = (float)(1.0 / sqrt((double)j.running_var_d[c] + (double)j.eps));
    const float ga = j.gamma_d ? j.gamma_d[c] : 1.f, be = j.beta_d ? j.beta_d[c] : 0.f;
    bpx_norm_rec r;
    r.mean = rm; r.rstd = rstd; r.scale = ga * rstd; r.shift = be - rm * r.scale;
    for (int n = 0; n < N; ++n) j.out_d[(size_t)n * j.C + c] = r;
  }
}

// TT: element type of the activation tensor t (BPX_MIX16: fp16 beside bf16 gradients), else T
template <typename T, typename TT = T>
__global__ void __launch_bounds__(256) norm_bwd_apply_kernel(const T* __restrict__ g, int g_ld, const TT* __restrict__ t, int t_ld,
                                                             const bpx_nbwd_coef* __restrict__ coef, const T* __restrict__ addend,
                                                             int a_ld, T* __restrict__ dx, int dx_ld, int C, int64_t vps, int N) {
  // one sample per blockIdx.y; blockDim.x * gridDim.x is a multiple of G, so a thread keeps its channel group and holds its
  // 3 x KPL coefficients in registers (loading them per element made the kernel load-instruction bound: 2.2 TB/s)
  constexpr int KPL = ElemTraits<T>::KPL;
  const int G = C / KPL;
  const int n = blockIdx.y;
  const int64_t total = vps * G;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = (int)(first % G);
  float ka[KPL], kb[KPL], kc[KPL];
#pragma unroll
  for (int e = 0; e < KPL; ++e) {
    bpx_nbwd_coef k = coef[(size_t)n * C + cg * KPL + e];
    ka[e] = k.a; kb[e] = k.b; kc[e] = k.c0;
  }
  const size_t base = (size_t)n * vps;
  // the launchers make gridDim.x * 256 a multiple of G (na_blocks): a thread keeps its channel group and its voxel advances by a constant -
  // no 64-bit division per element
  const size_t vstep = (size_t)gridDim.x * blockDim.x / G;
  size_t vox = base + (size_t)(first / G);
  for (int64_t i = first; i < total; i += (int64_t)gridDim.x * blockDim.x, vox += vstep) {
    u32x4_t gv = *reinterpret_cast<const u32x4_t*>(g + vox * g_ld + cg * KPL);
    u32x4_t tv = *reinterpret_cast<const u32x4_t*>(t + vox * t_ld + cg * KPL);
    float gf[KPL], tf[KPL], of[KPL];
    unpack16<T>(gv, gf);
    unpack16<TT>(tv, tf);
#pragma unroll
    for (int e = 0; e < KPL; ++e) of[e] = ka[e] * gf[e] + kb[e] * tf[e] + kc[e];
    if (addend) {
      u32x4_t av = *reinterpret_cast<const u32x4_t*>(addend + vox * a_ld + cg * KPL);
      float af[KPL];
      unpack16<T>(av, af);
#pragma unroll
      for (int e = 0; e < KPL; ++e) of[e] += af[e];
    }
    *reinterpret_cast<u32x4_t*>(dx + vox * dx_ld + cg * KPL) = pack16<T>(of);
  }
}

// ------------------------------------------------------------------------------------------------
// Materialised InstanceNorm + activation (plain U-Net, biapy/models/blocks.py:154-166 Conv -> Norm -> Act, where the consumer
// is a pooling / transposed-conv / head kernel without a fused prologue) and its backward.
//   fwd: y = act(scale*x + shift)
//   bwd: g = dy * act'(scale*x + shift) (+ addend);  partial sums per (sample, block, channel) of S1 = sum g, S2 = sum g*xhat
//        over THIS kernel's product only (an addend brings its own partial sums), in the [N][tiles][2][C] layout
//        bpx_norm_bwd_finalize reads.  One sample per blockIdx.y; a thread keeps its channel group (see norm_bwd_apply).
// ------------------------------------------------------------------------------------------------
constexpr int NA_BLOCKS = 512;   // blocks (= partial-sum slots) per sample, upper bound

template <typename T>
__global__ void __launch_bounds__(256) norm_act_fwd_kernel(const T* __restrict__ x, int x_ld, const bpx_norm_rec* __restrict__ rec, int act,
                                                           T* __restrict__ y, int y_ld, int C, int64_t vps) {
  constexpr int KPL = ElemTraits<T>::KPL;
  const int G = C / KPL;
  const int n = blockIdx.y;
  const int64_t total = vps * G;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = (int)(first % G);
  float sc[KPL], sh[KPL];
#pragma unroll
  for (int e = 0; e < KPL; ++e) {
    bpx_norm_rec r = rec[(size_t)n * C + cg * KPL + e];
    sc[e] = r.scale; sh[e] = r.shift;
  }
  const size_t base = (size_t)n * vps;
  // the launchers make gridDim.x * 256 a multiple of G (na_blocks): a thread keeps its channel group and its voxel advances by a constant -
  // no 64-bit division per element
  const size_t vstep = (size_t)gridDim.x * blockDim.x / G;
  size_t vox = base + (size_t)(first / G);
  for (int64_t i = first; i < total; i += (int64_t)gridDim.x * blockDim.x, vox += vstep) {
    float f[KPL];
    unpack16<T>(*reinterpret_cast<const u32x4_t*>(x + vox * x_ld + cg * KPL), f);
#pragma unroll
    for (int e = 0; e < KPL; ++e) {
      float u = sc[e] * f[e] + sh[e];
      f[e] = bpx_act_rt<false>(u, act);
    }
    *reinterpret_cast<u32x4_t*>(y + vox * y_ld + cg * KPL) = pack16<T>(f);
  }
}

template <typename T, typename TT = T>   // TT: storage type of the activation tensor x (fp16 beside bf16 gradients in the mixed mode)
__global__ void __launch_bounds__(256) norm_act_bwd_kernel(const T* __restrict__ dy, int dy_ld, const TT* __restrict__ x, int x_ld,
                                                           const bpx_norm_rec* __restrict__ rec, int act, const T* __restrict__ addend,
                                                           int a_ld, T* __restrict__ g, int g_ld, int C, int64_t vps,
                                                           float* __restrict__ red_part) {
  constexpr int KPL = ElemTraits<T>::KPL;
  extern __shared__ float nred[];   // [256][2*KPL]
  const int G = C / KPL;
  const int n = blockIdx.y, tiles = gridDim.x;
  const int64_t total = vps * G;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = (int)(first % G);
  float sc[KPL], sh[KPL], mu[KPL], rs[KPL], s1[KPL], s2[KPL];
#pragma unroll
  for (int e = 0; e < KPL; ++e) {
    bpx_norm_rec r = rec[(size_t)n * C + cg * KPL + e];
    sc[e] = r.scale; sh[e] = r.shift; mu[e] = r.mean; rs[e] = r.rstd;
    s1[e] = s2[e] = 0.f;
  }
  const size_t base = (size_t)n * vps;
  // the launchers make gridDim.x * 256 a multiple of G (na_blocks): a thread keeps its channel group and its voxel advances by a constant -
  // no 64-bit division per element
  const size_t vstep = (size_t)gridDim.x * blockDim.x / G;
  size_t vox = base + (size_t)(first / G);
  for (int64_t i = first; i < total; i += (int64_t)gridDim.x * blockDim.x, vox += vstep) {
    float d[KPL], f[KPL], o[KPL];
    unpack16<T>(*reinterpret_cast<const u32x4_t*>(dy + vox * dy_ld + cg * KPL), d);
    unpack16<TT>(*reinterpret_cast<const u32x4_t*>(x + vox * x_ld + cg * KPL), f);
#pragma unroll
    for (int e = 0; e < KPL; ++e) {
      float u = sc[e] * f[e] + sh[e];
      float da = bpx_act_bwd_rt<false>(u, act);
      float gv = d[e] * da;
      s1[e] += gv;
      s2[e] += gv * ((f[e] - mu[e]) * rs[e]);
      o[e] = gv;
    }
    if (addend) {
      float af[KPL];
      unpack16<T>(*reinterpret_cast<const u32x4_t*>(addend + vox * a_ld + cg * KPL), af);
#pragma unroll
      for (int e = 0; e < KPL; ++e) o[e] += af[e];
    }
    *reinterpret_cast<u32x4_t*>(g + vox * g_ld + cg * KPL) = pack16<T>(o);
  }
#pragma unroll
  for (int e = 0; e < KPL; ++e) {
    nred[threadIdx.x * 2 * KPL + e] = s1[e];
    nred[threadIdx.x * 2 * KPL + KPL + e] = s2[e];
  }
  __syncthreads();
  // threads with equal (threadIdx.x % G) share a channel group (256 * blockIdx.x is a multiple of G by construction)
  for (int o = threadIdx.x; o < 2 * C; o += blockDim.x) {
    const int which = o / C, c = o % C, grp = c / KPL, e = c % KPL;
    const int lane0 = (int)(((int64_t)grp - (int64_t)blockIdx.x * blockDim.x % G + G) % G);
    float acc = 0.f;
    for (int t = lane0; t < (int)blockDim.x; t += G) acc += nred[t * 2 * KPL + which * KPL + e];
    red_part[(((size_t)n * tiles + blockIdx.x) * 2 + which) * C + c] = acc;
  }
}

// ------------------------------------------------------------------------------------------------
// Dropout of a residual block (biapy/models/blocks.py:163 `nn.Dropout(p)` after Conv -> Norm -> Act, i.e. on the activated tensor the block's
// second convolution reads).  With p > 0 that tensor is materialised (the fused prologue of the second convolution cannot carry a mask through
// its three consumers cheaply, and p = 0 - BiaPy's default - keeps the fused path):
//   fwd: y = act(scale * x + shift) * keep / (1 - p)
//   bwd: g = dy * keep / (1 - p) * act'(scale * x + shift), with the S1 / S2 partial sums of norm_act_bwd_kernel
// keep = Philox4x32-10(key = seed, counter = (element / 4, site, *counter_d)) >= p * 2^32, element = linear NDHWC index of the dense tensor: the mask
// is a function of (seed, step counter, site, element) only - forward and backward regenerate it, nothing is stored.  *counter_d is a DEVICE
// value the caller bumps once per forward (a captured graph then draws a new mask at every replay).  mask_io (tests): mode 1 = read the
// keep flags from it instead of drawing them, mode 2 = also write the drawn flags to it.
// ------------------------------------------------------------------------------------------------
// philox4x32_10: philox.h (shared with augment.hip)
struct DropArgs { float p; uint32_t thr; uint64_t seed; const uint64_t* counter; uint32_t site; uint8_t* mask; int mask_mode; };
// keep flags of the KPL consecutive elements starting at linear element index e0 (a multiple of 4)
template <int KPL>
__device__ __forceinline__ void drop_keep(const DropArgs& d, uint64_t ctr, uint64_t e0, bool (&keep)[KPL]) {
  if (d.mask_mode == 1) {
#pragma unroll
    for (int e = 0; e < KPL; ++e) keep[e] = d.mask[e0 + e] != 0;
    return;
  }
#pragma unroll
  for (int q = 0; q < KPL / 4; ++q) {
    const uint64_t blk = (e0 >> 2) + q;
    uint32_t r[4];
    philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), d.site, (uint32_t)ctr ^ ((uint32_t)(ctr >> 32) * 0x9E3779B9u), (uint32_t)d.seed, (uint32_t)(d.seed >> 32), r);
#pragma unroll
    for (int e = 0; e < 4; ++e) keep[q * 4 + e] = r[e] >= d.thr;
  }
  if (d.mask_mode == 2) {
#pragma unroll
    for (int e = 0; e < KPL; ++e) d.mask[e0 + e] = keep[e] ? 1 : 0;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) norm_act_drop_fwd_kernel(const T* __restrict__ x, int x_ld, const bpx_norm_rec* __restrict__ rec, int act,
                                                                T* __restrict__ y, int y_ld, int C, int64_t vps, const DropArgs d) {
  constexpr int KPL = ElemTraits<T>::KPL;
  const int G = C / KPL;
  const int n = blockIdx.y;
  const int64_t total = vps * G;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = (int)(first % G);
  float sc[KPL], sh[KPL];
#pragma unroll
  for (int e = 0; e < KPL; ++e) {
    bpx_norm_rec r = rec[(size_t)n * C + cg * KPL + e];
    sc[e] = r.scale; sh[e] = r.shift;
  }
  const uint64_t ctr = *d.counter;
  const float inv = 1.f / (1.f - d.p);
  const size_t base = (size_t)n * vps;
  const size_t vstep = (size_t)gridDim.x * blockDim.x / G;
  size_t vox = base + (size_t)(first / G);
  for (int64_t i = first; i < total; i += (int64_t)gridDim.x * blockDim.x, vox += vstep) {
    float f[KPL];
    bool keep[KPL];
    unpack16<T>(*reinterpret_cast<const u32x4_t*>(x + vox * x_ld + cg * KPL), f);
    drop_keep<KPL>(d, ctr, (uint64_t)vox * C + cg * KPL, keep);
#pragma unroll
    for (int e = 0; e < KPL; ++e) {
      const float u = sc[e] * f[e] + sh[e];
      f[e] = keep[e] ? bpx_act_rt<false>(u, act) * inv : 0.f;
    }
    *reinterpret_cast<u32x4_t*>(y + vox * y_ld + cg * KPL) = pack16<T>(f);
  }
}

// T: gradients (dy, g); TT: the activation tensor x (fp16 beside bf16 gradients in the mixed mode)
template <typename T, typename TT>
__global__ void __launch_bounds__(256) norm_act_drop_bwd_kernel(const T* __restrict__ dy, int dy_ld, const TT* __restrict__ x, int x_ld,
                                                                const bpx_norm_rec* __restrict__ rec, int act, T* __restrict__ g, int g_ld, int C,
                                                                int64_t vps, float* __restrict__ red_part, const DropArgs d) {
  constexpr int KPL = ElemTraits<T>::KPL;
  extern __shared__ float nred[];   // [256][2*KPL]
  const int G = C / KPL;
  const int n = blockIdx.y, tiles = gridDim.x;
  const int64_t total = vps * G;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = (int)(first % G);
  float sc[KPL], sh[KPL], mu[KPL], rs[KPL], s1[KPL], s2[KPL];
#pragma unroll
  for (int e = 0; e < KPL; ++e) {
    bpx_norm_rec r = rec[(size_t)n * C + cg * KPL + e];
    sc[e] = r.scale; sh[e] = r.shift; mu[e] = r.mean; rs[e] = r.rstd;
    s1[e] = s2[e] = 0.f;
  }
  const uint64_t ctr = *d.counter;
  const float inv = 1.f / (1.f - d.p);
  const size_t base = (size_t)n * vps;
  const size_t vstep = (size_t)gridDim.x * blockDim.x / G;
  size_t vox = base + (size_t)(first / G);
  for (int64_t i = first; i < total; i += (int64_t)gridDim.x * blockDim.x, vox += vstep) {
    float dv[KPL], f[KPL], o[KPL];
    bool keep[KPL];
    unpack16<T>(*reinterpret_cast<const u32x4_t*>(dy + vox * dy_ld + cg * KPL), dv);
    unpack16<TT>(*reinterpret_cast<const u32x4_t*>(x + vox * x_ld + cg * KPL), f);
    drop_keep<KPL>(d, ctr, (uint64_t)vox * C + cg * KPL, keep);
#pragma unroll
    for (int e = 0; e < KPL; ++e) {
      const float u = sc[e] * f[e] + sh[e];
      const float gv = keep[e] ? dv[e] * inv * bpx_act_bwd_rt<false>(u, act) : 0.f;
      s1[e] += gv;
      s2[e] += gv * ((f[e] - mu[e]) * rs[e]);
      o[e] = gv;
    }
    *reinterpret_cast<u32x4_t*>(g + vox * g_ld + cg * KPL) = pack16<T>(o);
  }
#pragma unroll
  for (int e = 0; e < KPL; ++e) {
    nred[threadIdx.x * 2 * KPL + e] = s1[e];
    nred[threadIdx.x * 2 * KPL + KPL + e] = s2[e];
  }
  __syncthreads();
  for (int o = threadIdx.x; o < 2 * C; o += blockDim.x) {
    const int which = o / C, c = o % C, grp = c / KPL, e = c % KPL;
    const int lane0 = (int)(((int64_t)grp - (int64_t)blockIdx.x * blockDim.x % G + G) % G);
    float acc = 0.f;
    for (int t = lane0; t < (int)blockDim.x; t += G) acc += nred[t * 2 * KPL + which * KPL + e];
    red_part[(((size_t)n * tiles + blockIdx.x) * 2 + which) * C + c] = acc;
  }
}

// ------------------------------------------------------------------------------------------------
// Channel attention of the RCAN trunk (biapy/models/rcan.py ChannelAttention / RCAB_rcan: x + h * sigmoid(MLP(avgpool(h)))):
//   channel_affine: y = [x +] s[n,c] * h [+ off[n,c]]     (forward: x + s*h ; backward: dh = s*dy + dmean/voxels)
//   dot_stats:      part[n][block][c] = sum over the block's voxels of a*b   (ds[n,c] = sum_v dy*h)
// Same thread mapping as norm_act_*: one sample per blockIdx.y, a thread keeps its channel group.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) channel_affine_kernel(const T* __restrict__ x, int x_ld, const T* __restrict__ h, int h_ld,
                                                             const float* __restrict__ sc, const float* __restrict__ off, T* __restrict__ y,
                                                             int y_ld, int C, int64_t vps) {
  constexpr int KPL = ElemTraits<T>::KPL;
  const int G = C / KPL;
  const int n = blockIdx.y;
  const int64_t total = vps * G;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = (int)(first % G);
  float ks[KPL], ko[KPL];
#pragma unroll
  for (int e = 0; e < KPL; ++e) {
    ks[e] = sc[(size_t)n * C + cg * KPL + e];
    ko[e] = off ? off[(size_t)n * C + cg * KPL + e] : 0.f;
  }
  const size_t base = (size_t)n * vps;
  // the launchers make gridDim.x * 256 a multiple of G (na_blocks): a thread keeps its channel group and its voxel advances by a constant -
  // no 64-bit division per element
  const size_t vstep = (size_t)gridDim.x * blockDim.x / G;
  size_t vox = base + (size_t)(first / G);
  for (int64_t i = first; i < total; i += (int64_t)gridDim.x * blockDim.x, vox += vstep) {
    float hf[KPL], o[KPL];
    unpack16<T>(*reinterpret_cast<const u32x4_t*>(h + vox * h_ld + cg * KPL), hf);
#pragma unroll
    for (int e = 0; e < KPL; ++e) o[e] = ks[e] * hf[e] + ko[e];
    if (x) {
      float xf[KPL];
      unpack16<T>(*reinterpret_cast<const u32x4_t*>(x + vox * x_ld + cg * KPL), xf);
#pragma unroll
      for (int e = 0; e < KPL; ++e) o[e] += xf[e];
    }
    *reinterpret_cast<u32x4_t*>(y + vox * y_ld + cg * KPL) = pack16<T>(o);
  }
}

template <typename T, typename TB = T>   // TB: storage type of b (the forward pass's fp16 tensor beside a bf16 gradient a in the mixed mode)
__global__ void __launch_bounds__(256) dot_stats_kernel(const T* __restrict__ a, int a_ld, const TB* __restrict__ b, int b_ld, int C,
                                                        int64_t vps, float* __restrict__ part) {
  constexpr int KPL = ElemTraits<T>::KPL;
  extern __shared__ float dred[];   // [256][KPL]
  const int G = C / KPL;
  const int n = blockIdx.y, tiles = gridDim.x;
  const int64_t total = vps * G;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = (int)(first % G);
  float s[KPL];
#pragma unroll
  for (int e = 0; e < KPL; ++e) s[e] = 0.f;
  const size_t base = (size_t)n * vps;
  // the launchers make gridDim.x * 256 a multiple of G (na_blocks): a thread keeps its channel group and its voxel advances by a constant -
  // no 64-bit division per element
  const size_t vstep = (size_t)gridDim.x * blockDim.x / G;
  size_t vox = base + (size_t)(first / G);
  for (int64_t i = first; i < total; i += (int64_t)gridDim.x * blockDim.x, vox += vstep) {
    float af[KPL], bf[KPL];
    unpack16<T>(*reinterpret_cast<const u32x4_t*>(a + vox * a_ld + cg * KPL), af);
    unpack16<TB>(*reinterpret_cast<const u32x4_t*>(b + vox * b_ld + cg * KPL), bf);
#pragma unroll
    for (int e = 0; e < KPL; ++e) s[e] += af[e] * bf[e];
  }
#pragma unroll
  for (int e = 0; e < KPL; ++e) dred[threadIdx.x * KPL + e] = s[e];
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const int grp = c / KPL, e = c % KPL;
    const int lane0 = (int)(((int64_t)grp - (int64_t)blockIdx.x * blockDim.x % G + G) % G);
    float acc = 0.f;
    for (int t = lane0; t < (int)blockDim.x; t += G) acc += dred[t * KPL + e];
    part[((size_t)n * tiles + blockIdx.x) * C + c] = acc;
  }
}

// ------------------------------------------------------------------------------------------------
// max pooling 2x2x2
// ------------------------------------------------------------------------------------------------
constexpr int POOL_IPT = 4;  // items (output voxel x 16-byte channel group) per thread

template <typename T>
__global__ void maxpool_fwd_kernel(const T* __restrict__ x, int x_ld, int x_cs, T* __restrict__ y, int y_ld, int C, int D, int H, int W, int sz,
                                   int tiles, float* __restrict__ part) {  // window (sz,2,2): sz = z_down of the level (1 or 2)
  constexpr int KPL = ElemTraits<T>::KPL;
  extern __shared__ float red[];  // [blockDim][2*KPL]
  const int G = C / KPL;
  const int Do = D / sz, Ho = H / 2, Wo = W / 2;
  const int64_t items = (int64_t)Do * Ho * Wo * G;
  const int n = blockIdx.y, tile = blockIdx.x;
  const int cg = threadIdx.x % G;
  const size_t xc = (size_t)((cg * KPL) >> 4) * x_cs + ((cg * KPL) & 15);   // x may be chunk-planar (x_cs: elements between 16-channel chunks)
  float s1[KPL], s2[KPL];
#pragma unroll
  for (int e = 0; e < KPL; ++e) s1[e] = s2[e] = 0.f;
  for (int it = 0; it < POOL_IPT; ++it) {
    int64_t i = ((int64_t)tile * POOL_IPT + it) * blockDim.x + threadIdx.x;
    if (i >= items) break;
    int64_t ov = i / G;
    int xo = (int)(ov % Wo), yo = (int)((ov / Wo) % Ho), zo = (int)(ov / ((int64_t)Wo * Ho));
    float m[KPL];
#pragma unroll
    for (int e = 0; e < KPL; ++e) m[e] = -INFINITY;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k >= 4 * sz) break;
      size_t vox = (((size_t)n * D + sz * zo + (k >> 2)) * H + 2 * yo + ((k >> 1) & 1)) * W + 2 * xo + (k & 1);
      u32x4_t v = *reinterpret_cast<const u32x4_t*>(x + vox * x_ld + xc);
      float f[KPL];
      unpack16<T>(v, f);
#pragma unroll
      for (int e = 0; e < KPL; ++e) m[e] = f[e] > m[e] ? f[e] : m[e];
    }
    size_t ovox = (size_t)n * Do * Ho * Wo + ov;
    *reinterpret_cast<u32x4_t*>(y + ovox * y_ld + cg * KPL) = pack16<T>(m);
#pragma unroll
    for (int e = 0; e < KPL; ++e) { s1[e] += m[e]; s2[e] += m[e] * m[e]; }
  }
  if (part) {
#pragma unroll
    for (int e = 0; e < KPL; ++e) { red[threadIdx.x * 2 * KPL + e] = s1[e]; red[threadIdx.x * 2 * KPL + KPL + e] = s2[e]; }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 2 * C; idx += blockDim.x) {
      int k = idx / C, c = idx % C;
      int g0 = c / KPL, e = c % KPL;
      float s = 0.f;
      for (int t = g0; t < (int)blockDim.x; t += G) s += red[t * 2 * KPL + k * KPL + e];
      part[(((size_t)n * tiles + tile) * 2 + k) * C + c] = s;
    }
  }
}

// TX: element type of the pooled layer's INPUT x (BPX_MIX16: fp16 beside bf16 gradients), else T.  SZ (z extent of the window) and the presence of the
// addend are template constants (round 6): with the run-time `if (k >= 4 sz) break` inside the unrolled window loops every load sat in its own basic
// block behind an `s_waitcnt vmcnt(0)` (12 such sites) - a wait for all stores issued so far (level 0: 3.8 TB/s).  Now a window's 4 SZ x loads, its dy
// load and its 4 SZ addend loads are requested together, then the arg-max, then the 4 SZ stores.
// R1 (round 6, level 0 of a one-channel-image network): the first block's rank-1 shortcut weight gradient dWsc[co] = sum_v img[v] * dx[v][co] rides along - dx
// is that block's output gradient and this kernel is what writes it; as a kernel of its own (rank1_wgrad_kernel) it read the 268 MB back (60 us).  C = 16:
// a thread keeps the 8 channels of its channel group (its parity) over its whole grid-stride walk; one row of 16 partial sums per workgroup.
template <typename T, typename TX, int SZ, bool ADD, bool R1 = false>
__global__ void __launch_bounds__(256) maxpool_bwd_kernel(const TX* __restrict__ x, int x_ld, int x_cs, const T* __restrict__ dy, int dy_ld,
                                                          const T* __restrict__ addend, int a_ld, T* __restrict__ dx, int dx_ld, int C,
                                                          int D, int H, int W, int N, const float* __restrict__ img = nullptr, float* __restrict__ r1part = nullptr) {
  constexpr int KPL = ElemTraits<T>::KPL, NW = 4 * SZ;
  float r1acc[R1 ? KPL : 1];
#pragma unroll
  for (int e = 0; e < (R1 ? KPL : 1); ++e) r1acc[e] = 0.f;
  const int G = C / KPL;
  const int Do = D / SZ, Ho = H / 2, Wo = W / 2;
  const int64_t total = (int64_t)N * Do * Ho * Wo * G;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int cg = (int)(i % G);
    const int64_t ov = i / G;
    const int xo = (int)(ov % Wo), yo = (int)((ov / Wo) % Ho), zo = (int)((ov / ((int64_t)Wo * Ho)) % Do), n = (int)(ov / ((int64_t)Wo * Ho * Do));
    const size_t v0 = (((size_t)n * D + SZ * zo) * H + 2 * yo) * W + 2 * xo;
    const size_t xoff = (size_t)((cg * KPL) >> 4) * x_cs + ((cg * KPL) & 15);
    u32x4_t vx[NW], va[ADD ? NW : 1];
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const size_t vox = v0 + ((size_t)(k >> 2) * H + ((k >> 1) & 1)) * W + (k & 1);
      vx[k] = *reinterpret_cast<const u32x4_t*>(x + vox * x_ld + xoff);
    }
    const u32x4_t vd = *reinterpret_cast<const u32x4_t*>(dy + (size_t)ov * dy_ld + cg * KPL);
    if (ADD) {
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        const size_t vox = v0 + ((size_t)(k >> 2) * H + ((k >> 1) & 1)) * W + (k & 1);
        va[k] = *reinterpret_cast<const u32x4_t*>(addend + vox * a_ld + cg * KPL);
      }
    }
    float m[KPL];
    int am[KPL];
#pragma unroll
    for (int e = 0; e < KPL; ++e) { m[e] = -INFINITY; am[e] = 0; }
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      float f[KPL];
      unpack16<TX>(vx[k], f);
#pragma unroll
      for (int e = 0; e < KPL; ++e)
        if (f[e] > m[e]) { m[e] = f[e]; am[e] = k; }  // strict >: first maximum wins, as in PyTorch
    }
    float d[KPL];
    unpack16<T>(vd, d);
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const size_t vox = v0 + ((size_t)(k >> 2) * H + ((k >> 1) & 1)) * W + (k & 1);
      float o[KPL];
      if (ADD) unpack16<T>(va[k], o);
      else {
#pragma unroll
        for (int e = 0; e < KPL; ++e) o[e] = 0.f;
      }
#pragma unroll
      for (int e = 0; e < KPL; ++e) o[e] += (am[e] == k) ? d[e] : 0.f;
      const u32x4_t po = pack16<T>(o);
      *reinterpret_cast<u32x4_t*>(dx + vox * dx_ld + cg * KPL) = po;
      if constexpr (R1) {                                       // the STORED (rounded) values, as the separate kernel read them
        const float iv = img[vox];
        float orr[KPL];
        unpack16<T>(po, orr);
#pragma unroll
        for (int e = 0; e < KPL; ++e) r1acc[e] = fmaf(iv, orr[e], r1acc[e]);
      }
    }
  }
  if constexpr (R1) {
    // C = 16 = two channel groups: thread parity = channel group (the grid stride is even).  Lanes of one parity, then the four waves, in a fixed order.
    __shared__ float r1red[4][2 * KPL];   // column = parity KPL + e: the channel
#pragma unroll
    for (int e = 0; e < KPL; ++e) {
      float a = r1acc[e];
#pragma unroll
      for (int m = 2; m < 64; m <<= 1) a += __shfl_xor(a, m, 64);
      if ((threadIdx.x & 63) < 2) r1red[threadIdx.x >> 6][(threadIdx.x & 1) * KPL + e] = a;
    }
    __syncthreads();
    if (threadIdx.x < 16) r1part[(size_t)blockIdx.x * 16 + threadIdx.x] = four_wave_sum_pairs(r1red, threadIdx.x);
  }
}

// ------------------------------------------------------------------------------------------------
// weight packing (see DESIGN.md "packed weights")
// ------------------------------------------------------------------------------------------------
enum { PK_K3 = 0, PK_K3_T = 1, PK_K1 = 2, PK_DENSE = 3, PK_DENSE_T = 4, PK_CT = 5, PK_CT_T = 6, PK_CT4 = 7, PK_CT4_T = 8 };

// element (chunk, k-group q, column, e) of a packed 3x3x3 operand
template <int KPL>
__device__ __forceinline__ float pack_k3_value(const float* __restrict__ w, int mode, int Cin, int chunk, int q, int col, int e) {
  constexpr int GPT = 16 / KPL, QTOT = 27 * GPT;
  int tap = (q < QTOT) ? q / GPT : -1;
  const int cgp = q % GPT;
  if (GPT == 2 && q < 56) tap = bpx_tap_order_bf16(q / GPT);  // paired tap order of the bf16 kernels
  if (tap < 0) return 0.f;
  const int kc = chunk * 16 + cgp * KPL + e;  // reduction channel
  return mode == PK_K3 ? w[((size_t)col * Cin + kc) * 27 + tap]                 // W[co][ci][tap]
                       : w[((size_t)kc * Cin + col) * 27 + (26 - tap)];         // W[co=kc][ci=col][mirrored tap]
}

template <typename T>
__device__ __forceinline__ void pack_one(const float* __restrict__ w, T* __restrict__ out, int mode, int Cin, int Cout, int64_t i) {
  constexpr int KPL = ElemTraits<T>::KPL, GPT = 16 / KPL;
  {
    // 32-bit index arithmetic (the launchers bound an operand below 2^31 elements): the divisions by run-time channel counts below are ~25
    // instructions each on 32 bits and ~120 on 64 - with 64-bit indices the transposed-conv and 1x1x1 operands alone cost the batched launch 20 us
    const unsigned iu = (unsigned)i;
    int e = (int)(iu % KPL);
    unsigned r = iu / KPL;
    float v = 0.f;
    if (mode == PK_K3 || mode == PK_K3_T) {
      constexpr int QTOT = 27 * GPT, QPAD = ((QTOT + 3) / 4) * 4;
      const int ncol = (mode == PK_K3) ? Cout : Cin;  // columns = output channels of the operator
      int col = (int)(r % ncol); r /= ncol;
      int q = (int)(r % QPAD);
      int chunk = (int)(r / QPAD);
      v = pack_k3_value<KPL>(w, mode, Cin, chunk, q, col, e);
    } else if (mode == PK_K1) {
      int col = (int)(r % Cout); r /= Cout;
      int q = (int)(r % 4);
      int chunk = (int)(r / 4);
      if (q < GPT) v = w[(size_t)col * Cin + chunk * 16 + q * KPL + e];
    } else if (mode == PK_DENSE || mode == PK_DENSE_T) {
      const int ncol = (mode == PK_DENSE) ? Cout : Cin, K = (mode == PK_DENSE) ? Cin : Cout;
      int col = (int)(r % ncol);
      int q = (int)(r / ncol);
      int kc = q * KPL + e;
      if (kc < K) v = (mode == PK_DENSE) ? w[(size_t)col * Cin + kc] : w[(size_t)kc * Cin + col];
    } else if (mode == PK_CT || mode == PK_CT4) {  // ConvTranspose (Cin,Cout,nsub): columns = sub*Cout+co, K = Cin
      const int nsub = (mode == PK_CT) ? 8 : 4;           // kernel (2,2,2) or (1,2,2)
      const int ncol = nsub * Cout;
      int col = (int)(r % ncol);
      int q = (int)(r / ncol);
      int kc = q * KPL + e;
      int sub = col / Cout, co = col % Cout;
      if (kc < Cin) v = w[((size_t)kc * Cout + co) * nsub + sub];
    } else {  // PK_CT_T / PK_CT4_T: columns = ci, K = sub*Cout+co
      const int nsub = (mode == PK_CT_T) ? 8 : 4;
      int col = (int)(r % Cin);
      int q = (int)(r / Cin);
      int kc = q * KPL + e;
      if (kc < nsub * Cout) { int sub = kc / Cout, co = kc % Cout; v = w[((size_t)col * Cout + co) * nsub + sub]; }
    }
    ElemTraits<T>::st(out + i, v);
  }
}

template <typename T>
__device__ __forceinline__ void pack_elems(const float* __restrict__ w, T* __restrict__ out, int mode, int Cin, int Cout, int64_t total,
                                           int64_t first, int64_t stride) {
  for (int64_t i = first; i < total; i += stride) pack_one<T>(w, out, mode, Cin, Cout, i);
}

// The 3x3x3 operands in COLUMN BLOCKS (round 6).  In the linear order a workgroup covers 32 columns of ONE k-group q, and the 27 taps of a source
// row (w[co][ci][27]: neighbouring reduction channels lie 108 bytes apart) are fetched by 27 different workgroups: every 128-byte line of the fp32
// weights crosses the L2 -> L1 path ~27 times (0.7 GB per training step, 50 us).  Here a workgroup owns 8 columns of one 16-channel chunk and walks
// ALL of its k-groups: the lines it touches are used completely while they sit in its L1, and every k-group's 8 columns x KPL elements are one
// 128-byte store.  The elements are the linear order's own (pack_one): same bits.
constexpr int PACK_COLS = 8;
__host__ __device__ inline bool pack_by_columns(int mode, int Cin, int Cout) {
  return (mode == PK_K3 && Cout % PACK_COLS == 0) || (mode == PK_K3_T && Cin % PACK_COLS == 0);
}
__host__ __device__ inline int pack_qpad(int kpl) { return ((27 * (16 / kpl) + 3) / 4) * 4; }
__host__ __device__ inline int pack_column_blocks(int mode, int Cin, int Cout) {   // chunks x column groups
  return mode == PK_K3 ? (Cin / 16) * (Cout / PACK_COLS) : (Cout / 16) * (Cin / PACK_COLS);
}
// `stage`: PACK_COLS * 16 * 27 floats of LDS.  The block's source is 8 runs of 432 contiguous floats (PK_K3: one run per column = output channel) or
// 16 runs of 216 (PK_K3_T: one per reduction channel): it is brought in with consecutive lanes on consecutive floats - gathering straight from
// global memory put each lane of a load on its own cache line, 64 lines per wave instruction, and that (not the arithmetic) was the kernel's 50 us -
// and gathered from LDS (stride 27 words: conflict-free).
constexpr int PACK_STAGE = PACK_COLS * 16 * 27;
template <typename T>
__device__ __forceinline__ void pack_column_block(const float* __restrict__ w, T* __restrict__ out, int mode, int Cin, int Cout, int blk, float* stage) {
  constexpr int KPL = ElemTraits<T>::KPL, GPT = 16 / KPL, QTOT = 27 * GPT, QPAD = ((QTOT + 3) / 4) * 4;
  const int ncol = mode == PK_K3 ? Cout : Cin, cgs = ncol / PACK_COLS;
  const int chunk = blk / cgs, c0 = (blk - chunk * cgs) * PACK_COLS;
  const bool fwd = mode == PK_K3;
  const int run = fwd ? 16 * 27 : PACK_COLS * 27;                                  // contiguous floats per source run
  const size_t base = fwd ? ((size_t)c0 * Cin + chunk * 16) * 27 : ((size_t)chunk * 16 * Cin + c0) * 27, rstride = (size_t)Cin * 27;
  // (every run starts at a multiple of 216 floats and Cin is a multiple of 4 wherever this path is taken: 16-byte loads when the tensor itself is aligned)
  const bool al = ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(out)) & 15) == 0 && (Cin & 3) == 0;
  if (al) {
    for (int l = threadIdx.x * 4; l < PACK_STAGE; l += blockDim.x * 4) {
      const int r = l / run, off = l - r * run;
      *reinterpret_cast<f32x4_t*>(stage + l) = *reinterpret_cast<const f32x4_t*>(w + base + (size_t)r * rstride + off);
    }
  } else {
    for (int l = threadIdx.x; l < PACK_STAGE; l += blockDim.x) {
      const int r = l / run, off = l - r * run;
      stage[l] = w[base + (size_t)r * rstride + off];
    }
  }
  __syncthreads();
  T* const o = out + ((size_t)chunk * QPAD * ncol + c0) * KPL;
  // the element function of pack_k3_value on the staged copy: w[co][ci][tap] sits at stage[(col_l * 16 + kc_l) * 27 + tap] (PK_K3),
  // w[co = kc][ci = col][tap] at stage[(kc_l * PACK_COLS + col_l) * 27 + tap] (PK_K3_T, read at the mirrored tap)
  auto value = [&](int q, int col_l, int e) -> float {
    int tap = (q < QTOT) ? q / GPT : -1;
    if (GPT == 2 && q < 56) tap = bpx_tap_order_bf16(q / GPT);
    const int kc_l = (q % GPT) * KPL + e;
    return tap < 0 ? 0.f : fwd ? stage[(col_l * 16 + kc_l) * 27 + tap] : stage[(kc_l * PACK_COLS + col_l) * 27 + (26 - tap)];
  };
  if (al) {   // one 16-byte piece (k-group q, column) per thread and round: KPL element conversions of ElemTraits<T>::st, one store
    for (int pz = threadIdx.x; pz < QPAD * PACK_COLS; pz += blockDim.x) {
      const int q = pz / PACK_COLS, col_l = pz % PACK_COLS;
      alignas(16) T tmp[KPL];
#pragma unroll
      for (int e = 0; e < KPL; ++e) ElemTraits<T>::st(&tmp[e], value(q, col_l, e));
      *reinterpret_cast<u32x4_t*>(o + ((size_t)q * ncol + col_l) * KPL) = *reinterpret_cast<const u32x4_t*>(tmp);
    }
  } else {
    for (int l = threadIdx.x; l < QPAD * PACK_COLS * KPL; l += blockDim.x) {
      const int q = l / (PACK_COLS * KPL), ce = l % (PACK_COLS * KPL);          // ce = column-in-block * KPL + e: contiguous in the packed operand
      ElemTraits<T>::st(o + (size_t)q * ncol * KPL + ce, value(q, ce / KPL, ce % KPL));
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256) pack_kernel(const float* __restrict__ w, T* __restrict__ out, int mode, int Cin, int Cout,
                                                   int64_t total) {
  pack_elems<T>(w, out, mode, Cin, Cout, total, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// One launch for up to 64 operands.  Job k owns the blocks [first_block[k], first_block[k + 1]), their number proportional to its size (round 6: with
// 256 blocks for EVERY job the 1.8 M-element operands of the bottom of the U took 27 elements per thread while most of the grid idled; four elements
// per thread now, and the 3x3x3 operands in column blocks - pack_column_block above).  Same per-element function: the packed bits do not change.
struct PackBatch { bpx_pack_job job[64]; int64_t total[64]; int first_block[65]; int count; };
constexpr int PACK_EPT = 4;
__device__ __forceinline__ int pack_job_of_block(const PackBatch& b, int blk) {   // block-uniform search
  int lo = 0, hi = b.count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blk >= b.first_block[mid]) lo = mid; else hi = mid;
  }
  return lo;
}
template <typename T>
__global__ void __launch_bounds__(256) pack_batch_kernel(const PackBatch b) {
  const int k = pack_job_of_block(b, (int)blockIdx.x);
  const bpx_pack_job j = b.job[k];
  const int nb = b.first_block[k + 1] - b.first_block[k], blk = (int)blockIdx.x - b.first_block[k];
  __shared__ float stage[PACK_STAGE];
  if (pack_by_columns(j.mode, j.Cin, j.Cout)) pack_column_block<T>(j.w_d, reinterpret_cast<T*>(j.packed_d), j.mode, j.Cin, j.Cout, blk, stage);
  else pack_elems<T>(j.w_d, reinterpret_cast<T*>(j.packed_d), j.mode, j.Cin, j.Cout, b.total[k], (int64_t)blk * blockDim.x + threadIdx.x, (int64_t)nb * blockDim.x);
}

// BPX_MIX16 (fp16 forward / bf16 backward training): the forward operators' weights are fp16, the transposed (backward) operators' bf16
__host__ __device__ inline bool mix_mode_is_bf16(int mode) { return mode == PK_K3_T || mode == PK_DENSE_T || mode == PK_CT_T || mode == PK_CT4_T; }
__global__ void __launch_bounds__(256) pack_batch_mix_kernel(const PackBatch b) {
  const int k = pack_job_of_block(b, (int)blockIdx.x);
  const bpx_pack_job j = b.job[k];
  const int nb = b.first_block[k + 1] - b.first_block[k], blk = (int)blockIdx.x - b.first_block[k];
  const int64_t first = (int64_t)blk * blockDim.x + threadIdx.x, step = (int64_t)nb * blockDim.x;
  __shared__ float stage[PACK_STAGE];
  if (pack_by_columns(j.mode, j.Cin, j.Cout)) {
    if (mix_mode_is_bf16(j.mode)) pack_column_block<uint16_t>(j.w_d, reinterpret_cast<uint16_t*>(j.packed_d), j.mode, j.Cin, j.Cout, blk, stage);
    else pack_column_block<f16_t>(j.w_d, reinterpret_cast<f16_t*>(j.packed_d), j.mode, j.Cin, j.Cout, blk, stage);
  } else if (mix_mode_is_bf16(j.mode)) pack_elems<uint16_t>(j.w_d, reinterpret_cast<uint16_t*>(j.packed_d), j.mode, j.Cin, j.Cout, b.total[k], first, step);
  else pack_elems<f16_t>(j.w_d, reinterpret_cast<f16_t*>(j.packed_d), j.mode, j.Cin, j.Cout, b.total[k], first, step);
}

inline int64_t packed_elems(int mode, int Cin, int Cout, int dtype) {
  const int KPL = dtype == BPX_F32 ? 4 : 8, GPT = 16 / KPL;
  const int QPAD3 = ((27 * GPT + 3) / 4) * 4;
  auto r4 = [](int64_t q) { return (q + 3) / 4 * 4; };
  switch (mode) {
    case PK_K3: return (int64_t)(Cin / 16) * QPAD3 * Cout * KPL;
    case PK_K3_T: return (int64_t)(Cout / 16) * QPAD3 * Cin * KPL;
    case PK_K1: return (int64_t)(Cin / 16) * 4 * Cout * KPL;
    case PK_DENSE: return r4(Cin / KPL) * Cout * KPL;
    case PK_DENSE_T: return r4(Cout / KPL) * Cin * KPL;
    case PK_CT: return r4(Cin / KPL) * 8 * Cout * KPL;
    case PK_CT_T: return r4((int64_t)8 * Cout / KPL) * Cin * KPL;
    case PK_CT4: return r4(Cin / KPL) * 4 * Cout * KPL;
    case PK_CT4_T: return r4((int64_t)4 * Cout / KPL) * Cin * KPL;
  }
  return -1;
}

template <typename TS, typename TD>
__global__ void __launch_bounds__(256) cast_kernel(const TS* __restrict__ s, TD* __restrict__ d, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    ElemTraits<TD>::st(d + i, ElemTraits<TS>::ld(s + i));
}

// ------------------------------------------------------------------------------------------------
// image of 1 .. 16 channels -> the first block's 16-channel NDHWC input (bpx_image_pack16)
// ------------------------------------------------------------------------------------------------
// One thread per 16-byte piece of a voxel's 16 output channels (two pieces in the 16-bit modes, four in f32): consecutive lanes store consecutive
// 16 bytes, so every store instruction fills whole 128-byte lines.  A piece above the image's channels is zeros and loads nothing.  blockIdx.y is the
// sample, the grid strides over the voxels of one sample; every offset is 64-bit.  The values round as cast_kernel's do (ElemTraits<T>::st).
template <typename T> __device__ __forceinline__ u32x4_t pack16_as_cast(const float* f) { return pack16<T>(f); }
template <> __device__ __forceinline__ u32x4_t pack16_as_cast<uint16_t>(const float* f) {
  u32x4_t v;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = (uint32_t)f32_to_bf16(f[2 * i]) | ((uint32_t)f32_to_bf16(f[2 * i + 1]) << 16);
  return v;
}

template <typename T>
__global__ void __launch_bounds__(256) image_pack16_kernel(const float* __restrict__ img, int64_t vox, int C, int64_t stride_n, int64_t stride_v,
                                                           int64_t stride_c, T* __restrict__ out) {
  constexpr int KPL = ElemTraits<T>::KPL, PPV = 16 / KPL, VPB = 256 / PPV;   // channels per piece, pieces per voxel, voxels per block and step
  const int q = threadIdx.x % PPV, c0 = q * KPL;
  const float* src = img + (int64_t)blockIdx.y * stride_n + (int64_t)c0 * stride_c;
  u32x4_t* dst = reinterpret_cast<u32x4_t*>(out + (int64_t)blockIdx.y * vox * 16) + q;
  const int64_t step = (int64_t)gridDim.x * VPB;
  for (int64_t v = (int64_t)blockIdx.x * VPB + threadIdx.x / PPV; v < vox; v += step) {
    float f[KPL];
#pragma unroll
    for (int e = 0; e < KPL; ++e) f[e] = c0 + e < C ? src[v * stride_v + (int64_t)e * stride_c] : 0.f;
    dst[v * PPV] = pack16_as_cast<T>(f);
  }
}

// ------------------------------------------------------------------------------------------------
// lane-layout self test (one wave)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) selftest_kernel(float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[32 * 16];
  const int l = threadIdx.x, i = l & 15, g = l >> 4;
  // (0) bf16 16x16x32: A[i][k] = ((3i+5k)%7)-3, B[k][j] = ((2k+7j)%5)-2
  {
    float a[8], b[8];
    for (int e = 0; e < 8; ++e) { int k = 8 * g + e; a[e] = (float)((3 * i + 5 * k) % 7 - 3); b[e] = (float)((2 * k + 7 * i) % 5 - 2); }
    u32x4_t av = pack16<uint16_t>(a), bv = pack16<uint16_t>(b);
    f32x4_t c = mfma_step<uint16_t>(av, bv, f32x4_t{0.f, 0.f, 0.f, 0.f});
    for (int r = 0; r < 4; ++r) out[(4 * g + r) * 16 + i] = c[r];
  }
  // (1) f32 16x16x4 x4 (K = 16): lane supplies k = 4*g' .. as mfma_step<float> does: element jj <-> k = 4*g + jj?
  //     mfma_step<float> issues 4 MFMAs; MFMA jj uses lane-group g as its k index, so the global reduction index
  //     of element jj in group g is any bijection - here k = 4*g + jj.
  {
    float a[4], b[4];
    for (int e = 0; e < 4; ++e) { int k = 4 * g + e; a[e] = (float)((3 * i + 5 * k) % 7 - 3); b[e] = (float)((2 * k + 7 * i) % 5 - 2); }
    u32x4_t av = pack16<float>(a), bv = pack16<float>(b);
    f32x4_t c = mfma_step<float>(av, bv, f32x4_t{0.f, 0.f, 0.f, 0.f});
    for (int r = 0; r < 4; ++r) out[256 + (4 * g + r) * 16 + i] = c[r];
  }
  // (2) ds_read_b64_tr_b16: LDS [32 voxels][16 ch] of raw u16 = voxel*16 + ch; each lane reads as the wgrad does.
  {
    for (int q = l; q < 32 * 16; q += 64) lds[q] = (uint16_t)q;
    __syncthreads();
    const unsigned char* base = reinterpret_cast<const unsigned char*>(lds) + g * 8 * 32 + (i >> 2) * 32 + (i & 3) * 8;
    s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(base));
    s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(base + 4 * 32));
    for (int e = 0; e < 4; ++e) { out[512 + l * 8 + e] = (float)(uint16_t)lo[e]; out[512 + l * 8 + 4 + e] = (float)(uint16_t)hi[e]; }
  }
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" int bpx_selftest_layouts(float* out_d, bpx_stream_t stream) {
  BPX_CHECK(out_d, "bpx_selftest_layouts: null");
  selftest_kernel<<<1, 64, 0, (hipStream_t)stream>>>(out_d);
  BPX_LAUNCH_CHECK("bpx_selftest_layouts");
  return 0;
}

extern "C" int bpx_norm_finalize(float* stats_part_d, int N, int tiles, int C, int64_t count_per_channel, const float* gamma_d,
                                 const float* beta_d, float eps, int groups, bpx_norm_rec* out_d, int out_ld, int out_off,
                                 bpx_stream_t stream) {
  const char* fn = "bpx_norm_finalize";
  BPX_CHECK(stats_part_d && out_d, "%s: null pointer", fn);
  BPX_CHECK(groups >= 1 && C % groups == 0, "%s: groups %d must divide C %d", fn, groups, C);
  int cpg = C / groups;
  BPX_CHECK(cpg == 1 || 16 % cpg == 0 || cpg == 32 || cpg == 64, "%s: channels per group %d unsupported (1, 2, 4, 8, 16, 32, 64)", fn, cpg);
  const int cb = cpg > 16 ? cpg : 16;
  dim3 grid((unsigned)cdiv(C, cb), (unsigned)N);
  const int tstride = compact_stats(stats_part_d, N, tiles, C, (hipStream_t)stream);   // consumes the partials
  norm_finalize_kernel<<<grid, 1024, 0, (hipStream_t)stream>>>(stats_part_d, tiles, tstride, C, 1.0 / (double)count_per_channel, gamma_d, beta_d, eps,
                                                              cpg, cb, out_d, out_ld, out_off);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_norm_channel_sums(float* stats_part_d, int N, int tiles, int C, double* sums_d, int out_ld, int out_off, bpx_stream_t stream) {
  const char* fn = "bpx_norm_channel_sums";
  BPX_CHECK(stats_part_d && sums_d, "%s: null pointer", fn);
  BPX_CHECK(C >= 1 && out_off >= 0 && out_off + C <= out_ld, "%s: columns [%d, %d) do not fit a row of %d", fn, out_off, out_off + C, out_ld);
  dim3 grid((unsigned)cdiv(C, 16), (unsigned)N);
  const int tstride = compact_stats(stats_part_d, N, tiles, C, (hipStream_t)stream);   // consumes the partials
  chan_sums_kernel<<<grid, 1024, 0, (hipStream_t)stream>>>(stats_part_d, tiles, tstride, C, sums_d, out_ld, out_off);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_groupnorm_finalize(const double* sums_d, int N, int C, int64_t count_per_channel, const float* gamma_d, const float* beta_d, float eps,
                                      int groups, bpx_norm_rec* out_d, bpx_stream_t stream) {
  const char* fn = "bpx_groupnorm_finalize";
  BPX_CHECK(sums_d && out_d, "%s: null pointer", fn);
  BPX_CHECK(groups >= 1 && C % groups == 0, "%s: groups %d must divide C %d", fn, groups, C);
  gn_finalize_kernel<<<(unsigned)N, 512, 0, (hipStream_t)stream>>>(sums_d, C, 1.0 / (double)count_per_channel, gamma_d, beta_d, eps, C / groups, out_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_groupnorm_bwd_finalize(const double* sums_d, int N, int C, int64_t count_per_channel, const bpx_norm_rec* rec_d, const float* gamma_d,
                                          float* dgamma_d, float* dbeta_d, int groups, bpx_nbwd_coef* coef_d, bpx_stream_t stream) {
  const char* fn = "bpx_groupnorm_bwd_finalize";
  BPX_CHECK(sums_d && rec_d && coef_d, "%s: null pointer", fn);
  BPX_CHECK(groups >= 1 && C % groups == 0, "%s: groups %d must divide C %d", fn, groups, C);
  gn_bwd_finalize_kernel<<<1, 512, 0, (hipStream_t)stream>>>(sums_d, N, C, 1.0 / (double)count_per_channel, rec_d, gamma_d, dgamma_d, dbeta_d, C / groups, coef_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_tensor_stats_tiles(int64_t voxels) { return (int)cdiv64(voxels, 256); }

extern "C" int bpx_tensor_stats(int dtype, int N, int64_t voxels, bpx_tensor x, float* stats_part_d, bpx_stream_t stream) {
  BPX_CHECK(x.cs == 0, "bpx_tensor_stats: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_tensor_stats";
  BPX_CHECK(x.ptr && stats_part_d, "%s: null pointer", fn);
  int tiles = (int)cdiv64(voxels, 256);
  dim3 grid((unsigned)tiles, (unsigned)N);
  const int vec = dtype == BPX_F32 ? 4 : 8;
  const bool wide = x.C % vec == 0 && x.ld % vec == 0 && x.C / vec <= 256 && ((uintptr_t)x.ptr & 15) == 0;
  if (dtype == BPX_BF16 && wide) tensor_stats_vec_kernel<uint16_t><<<grid, 256, 0, (hipStream_t)stream>>>((const uint16_t*)x.ptr, x.ld, x.C, voxels, tiles, stats_part_d);
  else if (dtype == BPX_F16 && wide) tensor_stats_vec_kernel<f16_t><<<grid, 256, 0, (hipStream_t)stream>>>((const f16_t*)x.ptr, x.ld, x.C, voxels, tiles, stats_part_d);
  else if (dtype == BPX_F16) tensor_stats_kernel<f16_t><<<grid, 64, 0, (hipStream_t)stream>>>((const f16_t*)x.ptr, x.ld, x.C, voxels, tiles, stats_part_d);
  else if (dtype == BPX_F32 && wide) tensor_stats_vec_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>((const float*)x.ptr, x.ld, x.C, voxels, tiles, stats_part_d);
  else if (dtype == BPX_BF16) tensor_stats_kernel<uint16_t><<<grid, 64, 0, (hipStream_t)stream>>>((const uint16_t*)x.ptr, x.ld, x.C, voxels, tiles, stats_part_d);
  else if (dtype == BPX_F32) tensor_stats_kernel<float><<<grid, 64, 0, (hipStream_t)stream>>>((const float*)x.ptr, x.ld, x.C, voxels, tiles, stats_part_d);
  else BPX_FAIL("%s: dtype must be BF16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

static int norm_bwd_finalize_impl(const char* fn, bool deferred, float* red_part_d, int N, int tiles, int C, int64_t count_per_channel,
                                  const bpx_norm_rec* rec_d, const float* gamma_d, float* dgamma_d, float* dbeta_d, int groups, bpx_nbwd_coef* coef_d,
                                  bpx_stream_t stream) {
  BPX_CHECK(red_part_d && rec_d && coef_d, "%s: null pointer", fn);
  BPX_CHECK(groups >= 1 && C % groups == 0, "%s: groups %d must divide C %d", fn, groups, C);
  const int cpg = C / groups;
  BPX_CHECK(cpg == 1 || 16 % cpg == 0 || cpg == 32 || cpg == 64, "%s: channels per group %d unsupported (1, 2, 4, 8, 16, 32, 64)", fn, cpg);
  const int cb = cpg > 16 ? cpg : 16;
  const int tstride = compact_stats(red_part_d, N, tiles, C, (hipStream_t)stream);     // consumes the partials
  if (deferred && bpxred::defer_active() && N > 1) {
    dim3 grid((unsigned)cdiv(C, cb), (unsigned)N);
    norm_bwd_finalize_ps_kernel<<<grid, 1024, 0, (hipStream_t)stream>>>(red_part_d, tiles, tstride, C, 1.0 / (double)count_per_channel, rec_d, gamma_d, cpg, cb, coef_d);
    BPX_LAUNCH_CHECK(fn);
    const int64_t stride = (int64_t)tiles * 2 * C;
    if (dgamma_d && dbeta_d == dgamma_d + C) return bpxred::reduce_rows(fn, red_part_d, N, stride, 2 * C, dgamma_d, (hipStream_t)stream);   // adjacent in the gradient slab: one job
    if (dgamma_d && bpxred::reduce_rows(fn, red_part_d, N, stride, C, dgamma_d, (hipStream_t)stream) != 0) return 1;
    if (dbeta_d && bpxred::reduce_rows(fn, red_part_d + C, N, stride, C, dbeta_d, (hipStream_t)stream) != 0) return 1;
    return 0;
  }
  int NB = 1;                                                                          // samples per pass: keep >= 8 tile lanes per sample
  while (NB * 2 <= N && NB * 2 <= 16 && 1024 / (cb * NB * 2) >= 8) NB *= 2;
  norm_bwd_finalize_kernel<<<(unsigned)cdiv(C, cb), 1024, 0, (hipStream_t)stream>>>(red_part_d, N, tiles, tstride, C, 1.0 / (double)count_per_channel,
                                                                                   rec_d, gamma_d, dgamma_d, dbeta_d, cpg, cb, NB, coef_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_norm_bwd_finalize(float* red_part_d, int N, int tiles, int C, int64_t count_per_channel, const bpx_norm_rec* rec_d,
                                     const float* gamma_d, float* dgamma_d, float* dbeta_d, int groups, bpx_nbwd_coef* coef_d,
                                     bpx_stream_t stream) {
  return norm_bwd_finalize_impl("bpx_norm_bwd_finalize", false, red_part_d, N, tiles, C, count_per_channel, rec_d, gamma_d, dgamma_d, dbeta_d, groups, coef_d, stream);
}
// The same between bpx_wgrad_defer_begin and bpx_wgrad_defer_flush: coef_d is complete when the call's kernel is, dgamma / dbeta take their sums at
// the flush, and red_part_d must stay untouched until then.  Outside a deferred window it is bpx_norm_bwd_finalize.
extern "C" int bpx_norm_bwd_finalize_deferred(float* red_part_d, int N, int tiles, int C, int64_t count_per_channel, const bpx_norm_rec* rec_d,
                                              const float* gamma_d, float* dgamma_d, float* dbeta_d, int groups, bpx_nbwd_coef* coef_d,
                                              bpx_stream_t stream) {
  return norm_bwd_finalize_impl("bpx_norm_bwd_finalize_deferred", true, red_part_d, N, tiles, C, count_per_channel, rec_d, gamma_d, dgamma_d, dbeta_d, groups, coef_d,
                                stream);
}

extern "C" int bpx_batchnorm_finalize(float* stats_part_d, int N, int tiles, int C, int64_t count_per_sample, const float* gamma_d, const float* beta_d,
                                      float eps, float momentum, float* running_mean_d, float* running_var_d, int64_t* num_batches_tracked_d,
                                      bpx_norm_rec* out_d, int out_ld, int out_off, bpx_stream_t stream) {
  const char* fn = "bpx_batchnorm_finalize";
  BPX_CHECK(stats_part_d && out_d, "%s: null pointer", fn);
  BPX_CHECK(N >= 1 && tiles >= 1 && C >= 1 && out_off >= 0 && out_off + C <= out_ld, "%s: bad shape N %d tiles %d C %d columns [%d, %d) of %d", fn, N, tiles, C,
            out_off, out_off + C, out_ld);
  const int64_t n = (int64_t)N * count_per_sample;
  BPX_CHECK(n > 1, "%s: expected more than 1 value per channel when training (N * voxels = %lld)", fn, (long long)n);
  const int tstride = compact_stats(stats_part_d, N, tiles, C, (hipStream_t)stream);   // consumes the partials
  bn_finalize_kernel<<<(unsigned)cdiv(C, 16), 1024, 0, (hipStream_t)stream>>>(stats_part_d, N, tiles, tstride, C, 1.0 / (double)n,
                                                                               (double)n / (double)(n - 1), gamma_d, beta_d, eps, momentum, running_mean_d,
                                                                               running_var_d, num_batches_tracked_d, out_d, out_ld, out_off);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_batchnorm_bwd_finalize(float* red_part_d, int N, int tiles, int C, int64_t count_per_sample, const bpx_norm_rec* rec_d,
                                          const float* gamma_d, float* dgamma_d, float* dbeta_d, int running_stats, bpx_nbwd_coef* coef_d,
                                          bpx_stream_t stream) {
  const char* fn = "bpx_batchnorm_bwd_finalize";
  BPX_CHECK(red_part_d && rec_d && coef_d, "%s: null pointer", fn);
  BPX_CHECK(N >= 1 && tiles >= 1 && C >= 1 && count_per_sample >= 1, "%s: bad shape N %d tiles %d C %d", fn, N, tiles, C);
  const int tstride = compact_stats(red_part_d, N, tiles, C, (hipStream_t)stream);     // consumes the partials
  // running statistics (eval-mode forward): the mean and variance do not depend on the input, their terms vanish (m1 = m2 = 0: b = c0 = 0)
  const double inv_count = running_stats ? 0.0 : 1.0 / ((double)N * (double)count_per_sample);
  bn_bwd_finalize_kernel<<<(unsigned)cdiv(C, 16), 1024, 0, (hipStream_t)stream>>>(red_part_d, N, tiles, tstride, C, inv_count, rec_d, gamma_d, dgamma_d, dbeta_d,
                                                                                   coef_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_batchnorm_eval_records(int count, const bpx_bn_eval_job* jobs, int N, bpx_stream_t stream) {
  const char* fn = "bpx_batchnorm_eval_records";
  BPX_CHECK(jobs && count >= 1 && count <= 64 && N >= 1, "%s: 1 ... 64 jobs and N >= 1 (got %d, N %d)", fn, count, N);
  BnEvalBatch b{};
  for (int i = 0; i < count; ++i) {
    const bpx_bn_eval_job& j = jobs[i];
    BPX_CHECK(j.running_mean_d && j.running_var_d && j.out_d && j.C >= 1, "%s: job %d: null pointer or C %d", fn, i, j.C);
    b.job[i] = j;
  }
  bn_eval_records_kernel<<<(unsigned)count, 256, 0, (hipStream_t)stream>>>(b, N);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

// ---- gate multiply of ResUNet++'s attention block (blocks.py:2168-2298: `out = conv_attn(...) * x2`, a 1-channel map times a
// C-channel tensor) and its two gradients.  a: channel `a_ch` of an NDHWC tensor with channel stride a.ld.
template <typename T>
__global__ void __launch_bounds__(256) gate_mul_fwd_kernel(const T* __restrict__ a, int a_ld, const T* __restrict__ x, int x_ld, T* __restrict__ y, int y_ld,
                                                           int C, int64_t total_vox) {
  constexpr int KPL = ElemTraits<T>::KPL;
  const int G = C / KPL;
  const int64_t total = total_vox * G;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t v = i / G;
    const int gidx = (int)(i - v * G);
    const float av = ElemTraits<T>::ld(a + v * a_ld);
    float f[8];
    unpack16<T>(*reinterpret_cast<const u32x4_t*>(x + v * x_ld + gidx * KPL), f);
#pragma unroll
    for (int e = 0; e < KPL; ++e) f[e] *= av;
    *reinterpret_cast<u32x4_t*>(y + v * y_ld + gidx * KPL) = pack16<T>(f);
  }
}

// dx = dy * a (C channels);  da[v] = sum_c dy[v][c] * x[v][c] written to channel 0 of a 16-channel tensor whose other channels are
// zeroed (it is the gradient of the zero-padded 16-output 1x1 convolution that produced the gate).  One wave-quarter (16 lanes) per
// voxel would waste lanes for small C; instead a thread owns one voxel and walks its channels (C * 2 B <= a few cache lines).
template <typename T, typename TT = T>   // TT: storage type of the forward tensors a, x (fp16 beside bf16 gradients in the mixed mode)
__global__ void __launch_bounds__(256) gate_mul_bwd_kernel(const T* __restrict__ dy, int dy_ld, const TT* __restrict__ a, int a_ld, const TT* __restrict__ x,
                                                           int x_ld, T* __restrict__ dx, int dx_ld, T* __restrict__ da16, int C, int64_t total_vox) {
  constexpr int KPL = ElemTraits<T>::KPL;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total_vox; v += (int64_t)gridDim.x * 256) {
    const float av = ElemTraits<TT>::ld(a + v * a_ld);
    float dot = 0.f;
    for (int c0 = 0; c0 < C; c0 += KPL) {
      float g[8], xv[8];
      unpack16<T>(*reinterpret_cast<const u32x4_t*>(dy + v * dy_ld + c0), g);
      unpack16<TT>(*reinterpret_cast<const u32x4_t*>(x + v * x_ld + c0), xv);
#pragma unroll
      for (int e = 0; e < KPL; ++e) { dot += g[e] * xv[e]; g[e] *= av; }
      *reinterpret_cast<u32x4_t*>(dx + v * dx_ld + c0) = pack16<T>(g);
    }
    float o[8] = {dot, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float zz[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<u32x4_t*>(da16 + v * 16) = pack16<T>(o);
#pragma unroll
    for (int q = 1; q < 16 / KPL; ++q) *reinterpret_cast<u32x4_t*>(da16 + v * 16 + q * KPL) = pack16<T>(zz);
  }
}

extern "C" int bpx_norm_bwd_apply(int dtype, int N, int64_t voxels, bpx_tensor g, bpx_tensor t, const bpx_nbwd_coef* coef_d,
                                  bpx_tensor addend, bpx_tensor dx, bpx_stream_t stream) {
  BPX_CHECK(g.cs == 0 && t.cs == 0 && addend.cs == 0 && dx.cs == 0, "bpx_norm_bwd_apply: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_norm_bwd_apply";
  BPX_CHECK(g.ptr && t.ptr && dx.ptr && coef_d, "%s: null pointer", fn);
  BPX_CHECK(g.C == t.C && g.C == dx.C && g.C % 16 == 0, "%s: channel mismatch", fn);
  int kpl = (dtype == BPX_BF16 || dtype == BPX_MIX16) ? 8 : 4;
  int64_t total = (int64_t)N * voxels * (g.C / kpl);
  if (total == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int G = g.C / kpl;                                   // 256 * blocks must be a multiple of G (a thread keeps its channel group)
  int odd = G;
  while ((odd & 1) == 0 && odd > 1) odd >>= 1;
  BPX_CHECK(G / odd <= 256, "%s: unsupported channel count %d", fn, g.C);
  int bx = (int)std::min<int64_t>(cdiv64(voxels * G, 256), std::max(1, 256 * 16 / N));
  bx = (bx + odd - 1) / odd * odd;
  dim3 grid((unsigned)bx, (unsigned)N);
  if (dtype == BPX_BF16)
    norm_bwd_apply_kernel<uint16_t><<<grid, 256, 0, s>>>((const uint16_t*)g.ptr, g.ld, (const uint16_t*)t.ptr, t.ld, coef_d,
                                                                    (const uint16_t*)addend.ptr, addend.ld, (uint16_t*)dx.ptr, dx.ld, g.C, voxels, N);
  else if (dtype == BPX_MIX16)   // t = the forward pass's fp16 tensor; g, addend, dx bf16
    norm_bwd_apply_kernel<uint16_t, f16_t><<<grid, 256, 0, s>>>((const uint16_t*)g.ptr, g.ld, (const f16_t*)t.ptr, t.ld, coef_d,
                                                                (const uint16_t*)addend.ptr, addend.ld, (uint16_t*)dx.ptr, dx.ld, g.C, voxels, N);
  else if (dtype == BPX_F32)
    norm_bwd_apply_kernel<float><<<grid, 256, 0, s>>>((const float*)g.ptr, g.ld, (const float*)t.ptr, t.ld, coef_d,
                                                                 (const float*)addend.ptr, addend.ld, (float*)dx.ptr, dx.ld, g.C, voxels, N);
  else BPX_FAIL("%s: dtype must be BF16, F32 or MIX16", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

static int na_blocks(int64_t voxels, int C, int kpl) {
  const int G = C / kpl;
  int odd = G;
  while ((odd & 1) == 0 && odd > 1) odd >>= 1;
  int bx = (int)std::min<int64_t>(cdiv64(voxels * G, 256), NA_BLOCKS);
  return (bx + odd - 1) / odd * odd;   // 256 * bx is a multiple of G: a thread keeps its channel group
}

extern "C" int bpx_norm_act_tiles(int dtype, int64_t voxels, int C) { return na_blocks(voxels, C, dtype == BPX_F32 ? 4 : 8); }

extern "C" int bpx_norm_act_fwd(int dtype, int N, int64_t voxels, bpx_tensor x, const bpx_norm_rec* rec_d, int act, bpx_tensor y,
                                bpx_stream_t stream) {
  BPX_CHECK(x.cs == 0 && y.cs == 0, "bpx_norm_act_fwd: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_norm_act_fwd";
  BPX_CHECK(x.ptr && y.ptr && rec_d, "%s: null pointer", fn);
  BPX_CHECK(x.C == y.C && x.C % 16 == 0 && x.C <= 2048, "%s: channels must match and be a multiple of 16", fn);
  BPX_CHECK(act >= 0 && act <= BPX_ACT_LAST, "%s: unknown activation %d", fn, act);
  if ((int64_t)N * voxels == 0) return 0;
  const int kpl = dtype == BPX_F32 ? 4 : 8;
  dim3 grid((unsigned)na_blocks(voxels, x.C, kpl), (unsigned)N);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == BPX_BF16)
    norm_act_fwd_kernel<uint16_t><<<grid, 256, 0, s>>>((const uint16_t*)x.ptr, x.ld, rec_d, act, (uint16_t*)y.ptr, y.ld, x.C, voxels);
  else if (dtype == BPX_F16)
    norm_act_fwd_kernel<f16_t><<<grid, 256, 0, s>>>((const f16_t*)x.ptr, x.ld, rec_d, act, (f16_t*)y.ptr, y.ld, x.C, voxels);
  else if (dtype == BPX_F32)
    norm_act_fwd_kernel<float><<<grid, 256, 0, s>>>((const float*)x.ptr, x.ld, rec_d, act, (float*)y.ptr, y.ld, x.C, voxels);
  else BPX_FAIL("%s: dtype must be BF16, F16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_norm_act_bwd(int dtype, int N, int64_t voxels, bpx_tensor dy, bpx_tensor x, const bpx_norm_rec* rec_d, int act,
                                bpx_tensor addend, bpx_tensor g, float* red_part_d, bpx_stream_t stream) {
  BPX_CHECK(dy.cs == 0 && x.cs == 0 && addend.cs == 0 && g.cs == 0, "bpx_norm_act_bwd: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_norm_act_bwd";
  BPX_CHECK(dy.ptr && x.ptr && g.ptr && rec_d && red_part_d, "%s: null pointer", fn);
  BPX_CHECK(x.C == dy.C && x.C == g.C && x.C % 16 == 0 && x.C <= 2048, "%s: channels must match and be a multiple of 16", fn);
  BPX_CHECK(act >= 0 && act <= BPX_ACT_LAST, "%s: unknown activation %d", fn, act);
  if ((int64_t)N * voxels == 0) return 0;
  const int kpl = dtype == BPX_F32 ? 4 : 8;
  dim3 grid((unsigned)na_blocks(voxels, x.C, kpl), (unsigned)N);
  const size_t shm = (size_t)256 * 2 * kpl * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == BPX_BF16)
    norm_act_bwd_kernel<uint16_t><<<grid, 256, shm, s>>>((const uint16_t*)dy.ptr, dy.ld, (const uint16_t*)x.ptr, x.ld, rec_d, act,
                                                         (const uint16_t*)addend.ptr, addend.ld, (uint16_t*)g.ptr, g.ld, x.C, voxels, red_part_d);
  else if (dtype == BPX_MIX16)   // x = the forward pass's fp16 tensor; dy, addend, g bf16
    norm_act_bwd_kernel<uint16_t, f16_t><<<grid, 256, shm, s>>>((const uint16_t*)dy.ptr, dy.ld, (const f16_t*)x.ptr, x.ld, rec_d, act,
                                                                (const uint16_t*)addend.ptr, addend.ld, (uint16_t*)g.ptr, g.ld, x.C, voxels, red_part_d);
  else if (dtype == BPX_F32)
    norm_act_bwd_kernel<float><<<grid, 256, shm, s>>>((const float*)dy.ptr, dy.ld, (const float*)x.ptr, x.ld, rec_d, act,
                                                      (const float*)addend.ptr, addend.ld, (float*)g.ptr, g.ld, x.C, voxels, red_part_d);
  else BPX_FAIL("%s: dtype must be BF16, MIX16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

static int drop_args(const char* fn, float p, uint64_t seed, const uint64_t* counter_d, int site, uint8_t* mask_io_d, int mask_mode, DropArgs& d) {
  BPX_CHECK(p >= 0.f && p < 1.f, "%s: dropout probability %g outside [0, 1)", fn, (double)p);
  BPX_CHECK(counter_d != nullptr, "%s: the step counter is null", fn);
  BPX_CHECK(mask_mode >= 0 && mask_mode <= 2 && (mask_mode == 0 || mask_io_d != nullptr), "%s: mask mode %d needs a mask buffer", fn, mask_mode);
  d.p = p; d.thr = (uint32_t)std::min<double>(4294967295.0, (double)p * 4294967296.0); d.seed = seed; d.counter = counter_d; d.site = (uint32_t)site;
  d.mask = mask_io_d; d.mask_mode = mask_mode;
  return 0;
}

extern "C" int bpx_norm_act_dropout_fwd(int dtype, int N, int64_t voxels, bpx_tensor x, const bpx_norm_rec* rec_d, int act, float p, uint64_t seed,
                                        const uint64_t* counter_d, int site, uint8_t* mask_io_d, int mask_mode, bpx_tensor y, bpx_stream_t stream) {
  const char* fn = "bpx_norm_act_dropout_fwd";
  BPX_CHECK(x.cs == 0 && y.cs == 0 && x.ld == x.C && y.ld == y.C, "%s: dense tensors only", fn);
  BPX_CHECK(x.ptr && y.ptr && rec_d, "%s: null pointer", fn);
  BPX_CHECK(x.C == y.C && x.C % 16 == 0 && x.C <= 2048, "%s: channels must match and be a multiple of 16", fn);
  BPX_CHECK(act >= 0 && act <= BPX_ACT_LAST, "%s: unknown activation %d", fn, act);
  DropArgs d{};
  if (drop_args(fn, p, seed, counter_d, site, mask_io_d, mask_mode, d)) return 1;
  if ((int64_t)N * voxels == 0) return 0;
  const int kpl = dtype == BPX_F32 ? 4 : 8;
  dim3 grid((unsigned)na_blocks(voxels, x.C, kpl), (unsigned)N);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == BPX_BF16) norm_act_drop_fwd_kernel<uint16_t><<<grid, 256, 0, s>>>((const uint16_t*)x.ptr, x.ld, rec_d, act, (uint16_t*)y.ptr, y.ld, x.C, voxels, d);
  else if (dtype == BPX_F16) norm_act_drop_fwd_kernel<f16_t><<<grid, 256, 0, s>>>((const f16_t*)x.ptr, x.ld, rec_d, act, (f16_t*)y.ptr, y.ld, x.C, voxels, d);
  else if (dtype == BPX_F32) norm_act_drop_fwd_kernel<float><<<grid, 256, 0, s>>>((const float*)x.ptr, x.ld, rec_d, act, (float*)y.ptr, y.ld, x.C, voxels, d);
  else BPX_FAIL("%s: dtype must be BF16, F16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_norm_act_dropout_tiles(int dtype, int64_t voxels, int C) { return na_blocks(voxels, C, dtype == BPX_F32 ? 4 : 8); }

extern "C" int bpx_norm_act_dropout_bwd(int dtype, int N, int64_t voxels, bpx_tensor dy, bpx_tensor x, const bpx_norm_rec* rec_d, int act, float p,
                                        uint64_t seed, const uint64_t* counter_d, int site, uint8_t* mask_io_d, int mask_mode, bpx_tensor g,
                                        float* red_part_d, bpx_stream_t stream) {
  const char* fn = "bpx_norm_act_dropout_bwd";
  BPX_CHECK(dy.cs == 0 && x.cs == 0 && g.cs == 0 && x.ld == x.C && dy.ld == dy.C && g.ld == g.C, "%s: dense tensors only", fn);
  BPX_CHECK(dy.ptr && x.ptr && g.ptr && rec_d && red_part_d, "%s: null pointer", fn);
  BPX_CHECK(x.C == dy.C && x.C == g.C && x.C % 16 == 0 && x.C <= 2048, "%s: channels must match and be a multiple of 16", fn);
  BPX_CHECK(act >= 0 && act <= BPX_ACT_LAST, "%s: unknown activation %d", fn, act);
  DropArgs d{};
  if (drop_args(fn, p, seed, counter_d, site, mask_io_d, mask_mode == 2 ? 0 : mask_mode, d)) return 1;   // (the backward never writes the mask)
  if ((int64_t)N * voxels == 0) return 0;
  const int kpl = dtype == BPX_F32 ? 4 : 8;
  dim3 grid((unsigned)na_blocks(voxels, x.C, kpl), (unsigned)N);
  const size_t shm = (size_t)256 * 2 * kpl * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == BPX_BF16)
    norm_act_drop_bwd_kernel<uint16_t, uint16_t><<<grid, 256, shm, s>>>((const uint16_t*)dy.ptr, dy.ld, (const uint16_t*)x.ptr, x.ld, rec_d, act, (uint16_t*)g.ptr, g.ld, x.C, voxels, red_part_d, d);
  else if (dtype == BPX_MIX16)
    norm_act_drop_bwd_kernel<uint16_t, f16_t><<<grid, 256, shm, s>>>((const uint16_t*)dy.ptr, dy.ld, (const f16_t*)x.ptr, x.ld, rec_d, act, (uint16_t*)g.ptr, g.ld, x.C, voxels, red_part_d, d);
  else if (dtype == BPX_F32)
    norm_act_drop_bwd_kernel<float, float><<<grid, 256, shm, s>>>((const float*)dy.ptr, dy.ld, (const float*)x.ptr, x.ld, rec_d, act, (float*)g.ptr, g.ld, x.C, voxels, red_part_d, d);
  else BPX_FAIL("%s: dtype must be BF16, MIX16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_channel_affine(int dtype, int N, int64_t voxels, bpx_tensor x, bpx_tensor h, const float* scale_d, const float* offset_d,
                                  bpx_tensor y, bpx_stream_t stream) {
  BPX_CHECK(x.cs == 0 && h.cs == 0 && y.cs == 0, "bpx_channel_affine: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_channel_affine";
  BPX_CHECK(h.ptr && y.ptr && scale_d, "%s: null pointer", fn);
  BPX_CHECK(h.C == y.C && h.C % 16 == 0 && h.C <= 2048 && (x.ptr == nullptr || x.C == h.C), "%s: channels must match and be a multiple of 16", fn);
  if ((int64_t)N * voxels == 0) return 0;
  const int kpl = (dtype == BPX_BF16 || dtype == BPX_F16) ? 8 : 4;
  dim3 grid((unsigned)na_blocks(voxels, h.C, kpl) * 4, (unsigned)N);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == BPX_BF16)
    channel_affine_kernel<uint16_t><<<grid, 256, 0, s>>>((const uint16_t*)x.ptr, x.ld, (const uint16_t*)h.ptr, h.ld, scale_d, offset_d, (uint16_t*)y.ptr,
                                                         y.ld, h.C, voxels);
  else if (dtype == BPX_F16)     // fp16 storage (the super-resolution trunk's inference mode, cfg 5)
    channel_affine_kernel<f16_t><<<grid, 256, 0, s>>>((const f16_t*)x.ptr, x.ld, (const f16_t*)h.ptr, h.ld, scale_d, offset_d, (f16_t*)y.ptr, y.ld, h.C,
                                                      voxels);
  else if (dtype == BPX_F32)
    channel_affine_kernel<float><<<grid, 256, 0, s>>>((const float*)x.ptr, x.ld, (const float*)h.ptr, h.ld, scale_d, offset_d, (float*)y.ptr, y.ld, h.C,
                                                      voxels);
  else BPX_FAIL("%s: dtype must be BF16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The gate of channel attention / squeeze-excite on the pooled (N, C) vector (biapy/models/rcan.py ChannelAttention,
// blocks.py:1119-1191 SqExBlock): a few hundred FLOPs that were ~8 PyTorch launches each way - one block per sample forward,
// one block for the whole batch backward (the sums over samples run in a fixed order: deterministic).
//   m[c] = sum_tiles part[n][t][0][c] / voxels;  u1 = W1 m + b1;  a1 = act(u1);  s = sigmoid(W2 a1 + b2)
// saved[n] = { m[C], u1[R], a1[R] }.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gate_act(float u, int act) {
  return bpx_act_rt<true>(u, act);
}
__device__ __forceinline__ float gate_act_bwd(float u, int act) {
  return bpx_act_bwd_rt<true>(u, act);
}

// sum over the tiles of one (sample, channel) column, 256 / C lanes per channel, combined through LDS in lane order
__device__ __forceinline__ float gate_column_sum(const float* col, int tiles, size_t tstride, int C, double* red /* [256] */) {
  const int c = threadIdx.x % C, l = threadIdx.x / C, lanes = 256 / C;
  double a = 0.0;
  if (l < lanes) {
    double a1 = 0.0, a2 = 0.0, a3 = 0.0;                  // four accumulators; the kernel is one latency chain of L2 reads otherwise, so
    int t = l;                                            // sixteen loads are issued before the first add (the adds keep the order of the 4-row loop below: same bits)
    for (; t + 15 * lanes < tiles; t += 16 * lanes) {
      float v[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) v[k] = col[(size_t)(t + k * lanes) * tstride + c];
#pragma unroll
      for (int k = 0; k < 16; k += 4) { a += (double)v[k]; a1 += (double)v[k + 1]; a2 += (double)v[k + 2]; a3 += (double)v[k + 3]; }
    }
    for (; t + 3 * lanes < tiles; t += 4 * lanes) {
      a += (double)col[(size_t)t * tstride + c];
      a1 += (double)col[(size_t)(t + lanes) * tstride + c];
      a2 += (double)col[(size_t)(t + 2 * lanes) * tstride + c];
      a3 += (double)col[(size_t)(t + 3 * lanes) * tstride + c];
    }
    for (; t < tiles; t += lanes) a += (double)col[(size_t)t * tstride + c];
    a = (a + a1) + (a2 + a3);
  }
  red[threadIdx.x] = a;
  __syncthreads();
  double tot = 0.0;
  if ((int)threadIdx.x < C)
    for (int q = 0; q < lanes; ++q) tot += red[q * C + threadIdx.x];
  __syncthreads();
  return (float)tot;                                      // valid in threads < C
}

__global__ void __launch_bounds__(256) gate_mlp_fwd_kernel(const float* __restrict__ part, int tiles, int C, float inv_vox, const float* __restrict__ w1,
                                                           const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2, int R,
                                                           int act, float* __restrict__ s_out, float* __restrict__ saved) {
  __shared__ double red[256];
  __shared__ float m[256], a1[64];
  const int n = blockIdx.x, t = threadIdx.x;
  const float tot = gate_column_sum(part + (size_t)n * tiles * 2 * C, tiles, (size_t)2 * C, C, red);
  float* sv = saved + (size_t)n * (C + 2 * R);
  if (t < C) { m[t] = tot * inv_vox; sv[t] = m[t]; }
  __syncthreads();
  if (t < R) {
    float u = b1 ? b1[t] : 0.f;
    for (int c = 0; c < C; ++c) u += w1[(size_t)t * C + c] * m[c];
    const float a = gate_act(u, act);
    a1[t] = a;
    sv[C + t] = u; sv[C + R + t] = a;
  }
  __syncthreads();
  if (t < C) {
    float u = b2 ? b2[t] : 0.f;
    for (int r = 0; r < R; ++r) u += w2[(size_t)t * R + r] * a1[r];
    s_out[(size_t)n * C + t] = 1.f / (1.f + expf(-u));
  }
}

__global__ void __launch_bounds__(256) gate_mlp_bwd_kernel(const float* __restrict__ dpart, int N, int tiles, int C, float inv_vox, const float* __restrict__ s_in,
                                                           const float* __restrict__ saved, const float* __restrict__ w1, const float* __restrict__ w2, int R,
                                                           int act, float* __restrict__ dw1, float* __restrict__ db1, float* __restrict__ dw2,
                                                           float* __restrict__ db2, float* __restrict__ off) {
  __shared__ double red[256];
  __shared__ float du2[256], du1[64];
  const int t = threadIdx.x;
  float aw1[64], aw2[64];                                 // this thread's column of dW1 ([r][c = t]) and row of dW2 ([c = t][r]); R <= 64
  float ab2 = 0.f, ab1 = 0.f;
#pragma unroll
  for (int r = 0; r < 64; ++r) aw1[r] = aw2[r] = 0.f;
  for (int n = 0; n < N; ++n) {
    const float ds = gate_column_sum(dpart + (size_t)n * tiles * C, tiles, (size_t)C, C, red);
    const float* sv = saved + (size_t)n * (C + 2 * R);
    if (t < C) {
      const float sg = s_in[(size_t)n * C + t];
      du2[t] = ds * sg * (1.f - sg);
    }
    __syncthreads();
    if (t < R) {
      float a = 0.f;
      for (int c = 0; c < C; ++c) a += du2[c] * w2[(size_t)c * R + t];
      a *= gate_act_bwd(sv[C + t], act);
      du1[t] = a;
      ab1 += a;
    }
    __syncthreads();
    if (t < C) {
      const float d2 = du2[t], mc = sv[t];
      ab2 += d2;
      float dm = 0.f;
#pragma unroll
      for (int r = 0; r < 64; ++r)
        if (r < R) {
          aw2[r] += d2 * sv[C + R + r];
          aw1[r] += du1[r] * mc;
          dm += du1[r] * w1[(size_t)r * C + t];
        }
      off[(size_t)n * C + t] = dm * inv_vox;
    }
    __syncthreads();
  }
  if (t < C) {
#pragma unroll
    for (int r = 0; r < 64; ++r)
      if (r < R) {
        dw2[(size_t)t * R + r] += aw2[r];
        dw1[(size_t)r * C + t] += aw1[r];
      }
    if (db2) db2[t] += ab2;
  }
  if (t < R && db1) db1[t] += ab1;
}

extern "C" int bpx_gate_mlp_fwd(const float* part_d, int N, int tiles, int C, int64_t voxels, const float* w1_d, const float* b1_d, const float* w2_d,
                                const float* b2_d, int R, int act, float* s_d, float* saved_d, bpx_stream_t stream) {
  const char* fn = "bpx_gate_mlp_fwd";
  BPX_CHECK(part_d && w1_d && w2_d && s_d && saved_d, "%s: null pointer", fn);
  BPX_CHECK(N >= 0 && tiles > 0 && voxels > 0, "%s: bad extents", fn);
  BPX_CHECK(C >= 1 && C <= 256 && R >= 1 && R <= 64 && R <= C, "%s: C must be <= 256 and R <= 64 (got C=%d R=%d)", fn, C, R);
  BPX_CHECK(act >= 0 && act <= BPX_ACT_LAST, "%s: unknown activation %d", fn, act);
  if (N == 0) return 0;
  gate_mlp_fwd_kernel<<<(unsigned)N, 256, 0, (hipStream_t)stream>>>(part_d, tiles, C, (float)(1.0 / (double)voxels), w1_d, b1_d, w2_d, b2_d, R, act, s_d, saved_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_gate_mlp_bwd(const float* dpart_d, int N, int tiles, int C, int64_t voxels, const float* s_d, const float* saved_d, const float* w1_d,
                                const float* w2_d, int R, int act, float* dw1_d, float* db1_d, float* dw2_d, float* db2_d, float* off_d,
                                bpx_stream_t stream) {
  const char* fn = "bpx_gate_mlp_bwd";
  BPX_CHECK(dpart_d && s_d && saved_d && w1_d && w2_d && dw1_d && dw2_d && off_d, "%s: null pointer", fn);
  BPX_CHECK(N >= 0 && tiles > 0 && voxels > 0, "%s: bad extents", fn);
  BPX_CHECK(C >= 1 && C <= 256 && R >= 1 && R <= 64 && R <= C, "%s: C must be <= 256 and R <= 64 (got C=%d R=%d)", fn, C, R);
  BPX_CHECK(act >= 0 && act <= BPX_ACT_LAST, "%s: unknown activation %d", fn, act);
  if (N == 0) return 0;
  gate_mlp_bwd_kernel<<<1, 256, 0, (hipStream_t)stream>>>(dpart_d, N, tiles, C, (float)(1.0 / (double)voxels), s_d, saved_d, w1_d, w2_d, R, act, dw1_d, db1_d,
                                                          dw2_d, db2_d, off_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_dot_stats(int dtype, int N, int64_t voxels, bpx_tensor a, bpx_tensor b, float* part_d, bpx_stream_t stream) {
  BPX_CHECK(a.cs == 0 && b.cs == 0, "bpx_dot_stats: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_dot_stats";
  BPX_CHECK(a.ptr && b.ptr && part_d, "%s: null pointer", fn);
  BPX_CHECK(a.C == b.C && a.C % 16 == 0 && a.C <= 2048, "%s: channels must match and be a multiple of 16", fn);
  if ((int64_t)N * voxels == 0) return 0;
  const int kpl = dtype == BPX_F32 ? 4 : 8;
  dim3 grid((unsigned)na_blocks(voxels, a.C, kpl), (unsigned)N);
  const size_t shm = (size_t)256 * kpl * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == BPX_BF16) dot_stats_kernel<uint16_t><<<grid, 256, shm, s>>>((const uint16_t*)a.ptr, a.ld, (const uint16_t*)b.ptr, b.ld, a.C, voxels, part_d);
  else if (dtype == BPX_MIX16) dot_stats_kernel<uint16_t, f16_t><<<grid, 256, shm, s>>>((const uint16_t*)a.ptr, a.ld, (const f16_t*)b.ptr, b.ld, a.C, voxels, part_d);   // a bf16 gradient, b fp16 activation
  else if (dtype == BPX_F32) dot_stats_kernel<float><<<grid, 256, shm, s>>>((const float*)a.ptr, a.ld, (const float*)b.ptr, b.ld, a.C, voxels, part_d);
  else BPX_FAIL("%s: dtype must be BF16, MIX16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

static int pool_block(int C, int kpl) { int G = C / kpl; return (256 / G) * G; }

extern "C" int bpx_maxpool3d_stats_tiles(int dtype, int D, int H, int W, int sz, int C) {
  int kpl = dtype == BPX_F32 ? 4 : 8;
  int bd = pool_block(C, kpl);
  int64_t items = (int64_t)(D / (sz == 1 ? 1 : 2)) * (H / 2) * (W / 2) * (C / kpl);
  return (int)cdiv64(items, (int64_t)bd * POOL_IPT);
}

extern "C" int bpx_maxpool3d_fwd(int dtype, int N, int D, int H, int W, int sz, bpx_tensor x, bpx_tensor y, float* stats_part_d,
                                 bpx_stream_t stream) {
  BPX_CHECK(y.cs == 0, "bpx_maxpool3d_fwd: only x may be chunk-planar");
  BPX_CHECK(x.cs == 0 || (x.cs % 8 == 0 && x.cs >= ((int64_t)N * D * H * W - 1) * x.ld + 16), "bpx_maxpool3d_fwd: x has chunk stride %lld", (long long)x.cs);
  const int xcs = x.cs ? (int)x.cs : 16;
  const char* fn = "bpx_maxpool3d_fwd";
  BPX_CHECK(x.ptr && y.ptr, "%s: null pointer", fn);
  BPX_CHECK(sz == 1 || sz == 2, "%s: z stride must be 1 or 2 (got %d)", fn, sz);
  BPX_CHECK(D % sz == 0 && H % 2 == 0 && W % 2 == 0, "%s: extents must be divisible by the window (%d,2,2) (got %d,%d,%d)", fn, sz, D, H, W);
  BPX_CHECK(x.C == y.C && x.C % 16 == 0 && x.C <= 2048, "%s: channels must match and be a multiple of 16", fn);
  int kpl = dtype == BPX_F32 ? 4 : 8;
  int bd = pool_block(x.C, kpl);
  int tiles = bpx_maxpool3d_stats_tiles(dtype, D, H, W, sz, x.C);
  dim3 grid((unsigned)tiles, (unsigned)N);
  size_t shm = (size_t)bd * 2 * kpl * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == BPX_BF16)
    maxpool_fwd_kernel<uint16_t><<<grid, bd, shm, s>>>((const uint16_t*)x.ptr, x.ld, xcs, (uint16_t*)y.ptr, y.ld, x.C, D, H, W, sz, tiles, stats_part_d);
  else if (dtype == BPX_F16)
    maxpool_fwd_kernel<f16_t><<<grid, bd, shm, s>>>((const f16_t*)x.ptr, x.ld, xcs, (f16_t*)y.ptr, y.ld, x.C, D, H, W, sz, tiles, stats_part_d);
  else if (dtype == BPX_F32)
    maxpool_fwd_kernel<float><<<grid, bd, shm, s>>>((const float*)x.ptr, x.ld, xcs, (float*)y.ptr, y.ld, x.C, D, H, W, sz, tiles, stats_part_d);
  else BPX_FAIL("%s: dtype must be BF16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_maxpool3d_bwd(int dtype, int N, int D, int H, int W, int sz, bpx_tensor x, bpx_tensor dy, bpx_tensor addend, bpx_tensor dx,
                                 bpx_stream_t stream) {
  BPX_CHECK(dy.cs == 0 && addend.cs == 0 && dx.cs == 0, "bpx_maxpool3d_bwd: only x may be chunk-planar");
  BPX_CHECK(x.cs == 0 || (x.cs % 8 == 0 && x.cs >= ((int64_t)N * D * H * W - 1) * x.ld + 16), "bpx_maxpool3d_bwd: x has chunk stride %lld", (long long)x.cs);
  const int xcs = x.cs ? (int)x.cs : 16;
  const char* fn = "bpx_maxpool3d_bwd";
  BPX_CHECK(x.ptr && dy.ptr && dx.ptr, "%s: null pointer", fn);
  BPX_CHECK(sz == 1 || sz == 2, "%s: z stride must be 1 or 2 (got %d)", fn, sz);
  // (the kernel walks whole windows: a trailing plane / row / column would keep whatever dx held and lose the addend there)
  BPX_CHECK(D % sz == 0 && H % 2 == 0 && W % 2 == 0, "%s: extents must be divisible by the window (%d,2,2) (got %d,%d,%d)", fn, sz, D, H, W);
  BPX_CHECK(x.C == dy.C && x.C == dx.C && x.C % 16 == 0, "%s: channel mismatch", fn);
  int kpl = (dtype == BPX_BF16 || dtype == BPX_MIX16) ? 8 : 4;
  int64_t total = (int64_t)N * (D / sz) * (H / 2) * (W / 2) * (x.C / kpl);
  if (total == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const bool add = addend.ptr != nullptr;
#define MPB(T_, TX_)                                                                                                                                        \
  do {                                                                                                                                                      \
    const TX_* xp = (const TX_*)x.ptr; const T_* dyp = (const T_*)dy.ptr; const T_* ap = (const T_*)addend.ptr; T_* dxp = (T_*)dx.ptr;                     \
    if (sz == 2 && add) maxpool_bwd_kernel<T_, TX_, 2, true><<<grid_for(total), 256, 0, s>>>(xp, x.ld, xcs, dyp, dy.ld, ap, addend.ld, dxp, dx.ld, x.C, D, H, W, N);   \
    else if (sz == 2) maxpool_bwd_kernel<T_, TX_, 2, false><<<grid_for(total), 256, 0, s>>>(xp, x.ld, xcs, dyp, dy.ld, ap, addend.ld, dxp, dx.ld, x.C, D, H, W, N);    \
    else if (add) maxpool_bwd_kernel<T_, TX_, 1, true><<<grid_for(total), 256, 0, s>>>(xp, x.ld, xcs, dyp, dy.ld, ap, addend.ld, dxp, dx.ld, x.C, D, H, W, N);         \
    else maxpool_bwd_kernel<T_, TX_, 1, false><<<grid_for(total), 256, 0, s>>>(xp, x.ld, xcs, dyp, dy.ld, ap, addend.ld, dxp, dx.ld, x.C, D, H, W, N);                 \
  } while (0)
  if (dtype == BPX_BF16) MPB(uint16_t, uint16_t);
  else if (dtype == BPX_MIX16) MPB(uint16_t, f16_t);   // x = the forward pass's fp16 tensor; dy, addend, dx bf16
  else if (dtype == BPX_F32) MPB(float, float);
  else BPX_FAIL("%s: dtype must be BF16, F32 or MIX16", fn);
#undef MPB
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

// bpx_maxpool3d_bwd (with addend) + the rank-1 shortcut weight gradient of the block whose output gradient it writes (maxpool_bwd_kernel<.., R1 = true>)
extern "C" int64_t bpx_maxpool3d_bwd_r1_workspace(int dtype, int N, int D, int H, int W, int sz, int C) {
  static const bool on = getenv("BPX_POOL_R1") == nullptr || atoi(getenv("BPX_POOL_R1")) != 0;   // A/B: BPX_POOL_R1=0 = the two separate kernels
  if (!on || (dtype != BPX_BF16 && dtype != BPX_MIX16) || C != 16 || (sz != 1 && sz != 2) || D % sz || H % 2 || W % 2) return 0;
  const int64_t total = (int64_t)N * (D / sz) * (H / 2) * (W / 2) * 2;
  if (total < 65536) return 0;
  return (int64_t)grid_for(total) * 16 * 4;
}
extern "C" int bpx_maxpool3d_bwd_r1(int dtype, int N, int D, int H, int W, int sz, bpx_tensor x, bpx_tensor dy, bpx_tensor addend, bpx_tensor dx,
                                    const float* img_d, float* dw_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  const char* fn = "bpx_maxpool3d_bwd_r1";
  BPX_CHECK(dy.cs == 0 && addend.cs == 0 && dx.cs == 0, "%s: only x may be chunk-planar", fn);
  BPX_CHECK(x.cs == 0 || (x.cs % 8 == 0 && x.cs >= ((int64_t)N * D * H * W - 1) * x.ld + 16), "%s: x has chunk stride %lld", fn, (long long)x.cs);
  const int xcs = x.cs ? (int)x.cs : 16;
  BPX_CHECK(x.ptr && dy.ptr && dx.ptr && addend.ptr && img_d && dw_d && ws_d, "%s: null pointer", fn);
  BPX_CHECK(x.C == dy.C && x.C == dx.C && x.C == addend.C, "%s: channel mismatch", fn);
  BPX_CHECK(sz == 1 || sz == 2, "%s: z stride must be 1 or 2 (got %d)", fn, sz);
  BPX_CHECK(D % sz == 0 && H % 2 == 0 && W % 2 == 0, "%s: extents must be divisible by the window (%d,2,2) (got %d,%d,%d)", fn, sz, D, H, W);
  const int64_t need = bpx_maxpool3d_bwd_r1_workspace(dtype, N, D, H, W, sz, x.C);
  BPX_CHECK(need > 0, "%s: unsupported here (16 channels, 16-bit storage): use bpx_maxpool3d_bwd and bpx_conv1x1_c1_wgrad", fn);
  BPX_CHECK(ws_bytes >= need, "%s: workspace too small (%lld < %lld bytes)", fn, (long long)ws_bytes, (long long)need);
  const int64_t total = (int64_t)N * (D / sz) * (H / 2) * (W / 2) * 2;
  const int blocks = grid_for(total);
  hipStream_t s = (hipStream_t)stream;
  float* pw = reinterpret_cast<float*>(ws_d);
  const uint16_t* dyp = (const uint16_t*)dy.ptr; const uint16_t* ap = (const uint16_t*)addend.ptr; uint16_t* dxp = (uint16_t*)dx.ptr;
#define MPR(TX_)                                                                                                                                                          \
  do {                                                                                                                                                                    \
    if (sz == 2) maxpool_bwd_kernel<uint16_t, TX_, 2, true, true><<<blocks, 256, 0, s>>>((const TX_*)x.ptr, x.ld, xcs, dyp, dy.ld, ap, addend.ld, dxp, dx.ld, x.C, D, H, W, N, img_d, pw); \
    else maxpool_bwd_kernel<uint16_t, TX_, 1, true, true><<<blocks, 256, 0, s>>>((const TX_*)x.ptr, x.ld, xcs, dyp, dy.ld, ap, addend.ld, dxp, dx.ld, x.C, D, H, W, N, img_d, pw);         \
  } while (0)
  if (dtype == BPX_MIX16) MPR(f16_t); else MPR(uint16_t);
#undef MPR
  BPX_LAUNCH_CHECK(fn);
  return bpxred::reduce_partials(fn, pw, dw_d, blocks, 1, 1, 16, 0, 1, 0, nullptr, nullptr, 0, true, s);
}

extern "C" int64_t bpx_packed_weight_elems(int mode, int Cin, int Cout, int dtype) { return packed_elems(mode, Cin, Cout, dtype); }

extern "C" int bpx_pack_weight(int mode, const float* w_d, int Cin, int Cout, int dtype, void* packed_d, bpx_stream_t stream) {
  const char* fn = "bpx_pack_weight";
  BPX_CHECK(w_d && packed_d, "%s: null pointer", fn);
  BPX_CHECK(mode >= PK_K3 && mode <= PK_CT4_T, "%s: bad mode %d", fn, mode);
  BPX_CHECK(dtype == BPX_BF16 || dtype == BPX_F32 || dtype == BPX_F16 || dtype == BPX_MIX16, "%s: dtype must be BF16, F16, F32 or MIX16", fn);
  if (dtype == BPX_MIX16) dtype = mix_mode_is_bf16(mode) ? BPX_BF16 : BPX_F16;   // forward operators fp16, transposed (backward) operators bf16
  if (mode <= PK_K1) BPX_CHECK(Cin % 16 == 0 && Cout % 16 == 0, "%s: Cin/Cout must be multiples of 16", fn);
  if (mode == PK_K3_T) BPX_CHECK(Cout % 16 == 0, "%s: Cout must be a multiple of 16", fn);
  int64_t total = packed_elems(mode, Cin, Cout, dtype);
  BPX_CHECK(total < (1ll << 31), "%s: an operand of %lld elements is beyond the 32-bit index range of the pack kernels", fn, (long long)total);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == BPX_BF16) pack_kernel<uint16_t><<<grid_for(total), 256, 0, s>>>(w_d, (uint16_t*)packed_d, mode, Cin, Cout, total);
  else if (dtype == BPX_F16) pack_kernel<f16_t><<<grid_for(total), 256, 0, s>>>(w_d, (f16_t*)packed_d, mode, Cin, Cout, total);
  else pack_kernel<float><<<grid_for(total), 256, 0, s>>>(w_d, (float*)packed_d, mode, Cin, Cout, total);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_pack_weights_batched(int dtype, int count, const bpx_pack_job* jobs, bpx_stream_t stream) {
  const char* fn = "bpx_pack_weights_batched";
  BPX_CHECK(dtype == BPX_BF16 || dtype == BPX_F32 || dtype == BPX_F16 || dtype == BPX_MIX16, "%s: dtype must be BF16, F16, F32 or MIX16", fn);
  BPX_CHECK(count >= 0 && (count == 0 || jobs != nullptr), "%s: bad job list", fn);
  hipStream_t s = (hipStream_t)stream;
  for (int base = 0; base < count; base += 64) {
    PackBatch b{};
    const int n = std::min(64, count - base);
    int blocks = 0;
    b.count = n;
    for (int k = 0; k < n; ++k) {
      const bpx_pack_job& j = jobs[base + k];
      BPX_CHECK(j.w_d && j.packed_d, "%s: job %d has a null pointer", fn, base + k);
      BPX_CHECK(j.mode >= PK_K3 && j.mode <= PK_CT4_T, "%s: job %d: unknown mode %d", fn, base + k, j.mode);
      BPX_CHECK(j.Cin >= 1 && j.Cout >= 1, "%s: job %d: bad channel counts", fn, base + k);
      if (j.mode == PK_K3 || j.mode == PK_K1) BPX_CHECK(j.Cin % 16 == 0, "%s: job %d: Cin must be a multiple of 16", fn, base + k);
      if (j.mode == PK_K3_T) BPX_CHECK(j.Cout % 16 == 0, "%s: job %d: Cout must be a multiple of 16", fn, base + k);
      b.job[k] = j;
      b.total[k] = packed_elems(j.mode, j.Cin, j.Cout, dtype);
      BPX_CHECK(b.total[k] < (1ll << 31), "%s: job %d: an operand of %lld elements is beyond the 32-bit index range of the pack kernels", fn, base + k, (long long)b.total[k]);
      b.first_block[k] = blocks;
      blocks += pack_by_columns(j.mode, j.Cin, j.Cout) ? pack_column_blocks(j.mode, j.Cin, j.Cout) : (int)std::max<int64_t>(1, cdiv64(b.total[k], 256 * PACK_EPT));
    }
    b.first_block[n] = blocks;
    const unsigned grid = (unsigned)blocks;
    if (dtype == BPX_BF16) pack_batch_kernel<uint16_t><<<grid, 256, 0, s>>>(b);
    else if (dtype == BPX_MIX16) pack_batch_mix_kernel<<<grid, 256, 0, s>>>(b);
    else if (dtype == BPX_F16) pack_batch_kernel<f16_t><<<grid, 256, 0, s>>>(b);
    else pack_batch_kernel<float><<<grid, 256, 0, s>>>(b);
    BPX_LAUNCH_CHECK(fn);
  }
  return 0;
}

extern "C" int bpx_cast(int src_dtype, const void* src_d, int dst_dtype, void* dst_d, int64_t n, bpx_stream_t stream) {
  const char* fn = "bpx_cast";
  BPX_CHECK(src_d && dst_d, "%s: null pointer", fn);
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (src_dtype == BPX_F32 && dst_dtype == BPX_BF16) cast_kernel<float, uint16_t><<<grid_for(n), 256, 0, s>>>((const float*)src_d, (uint16_t*)dst_d, n);
  else if (src_dtype == BPX_F32 && dst_dtype == BPX_F16) cast_kernel<float, f16_t><<<grid_for(n), 256, 0, s>>>((const float*)src_d, (f16_t*)dst_d, n);
  else if (src_dtype == BPX_BF16 && dst_dtype == BPX_F32) cast_kernel<uint16_t, float><<<grid_for(n), 256, 0, s>>>((const uint16_t*)src_d, (float*)dst_d, n);
  else BPX_FAIL("%s: unsupported conversion %d -> %d", fn, src_dtype, dst_dtype);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_image_pack16(int dtype, int N, int64_t voxels, int C, const float* img_d, int64_t stride_n, int64_t stride_v, int64_t stride_c,
                                void* out16_d, bpx_stream_t stream) {
  const char* fn = "bpx_image_pack16";
  BPX_CHECK(img_d && out16_d, "%s: null pointer", fn);
  BPX_CHECK(C >= 1 && C <= 16, "%s: 1 <= C <= 16 channels (got %d)", fn, C);
  BPX_CHECK(N >= 0 && N <= 65535 && voxels >= 0, "%s: bad shape (N = %d, voxels = %lld)", fn, N, (long long)voxels);
  BPX_CHECK(stride_n >= 0 && stride_v >= 0 && stride_c >= 0, "%s: negative stride", fn);
  BPX_CHECK(((uintptr_t)out16_d & 15) == 0 && ((uintptr_t)img_d & 3) == 0, "%s: the output must be 16-byte aligned, the image 4-byte", fn);
  if (N == 0 || voxels == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int ppv = dtype == BPX_F32 ? 4 : 2;   // 16-byte pieces per voxel
  dim3 grid((unsigned)std::min<int64_t>(cdiv64(voxels * ppv, 256), std::max<int64_t>(1, 256 * 16 / N)), (unsigned)N);
  if (dtype == BPX_F32) image_pack16_kernel<float><<<grid, 256, 0, s>>>(img_d, voxels, C, stride_n, stride_v, stride_c, (float*)out16_d);
  else if (dtype == BPX_BF16) image_pack16_kernel<uint16_t><<<grid, 256, 0, s>>>(img_d, voxels, C, stride_n, stride_v, stride_c, (uint16_t*)out16_d);
  else if (dtype == BPX_F16) image_pack16_kernel<f16_t><<<grid, 256, 0, s>>>(img_d, voxels, C, stride_n, stride_v, stride_c, (f16_t*)out16_d);
  else BPX_FAIL("%s: unsupported storage dtype %d", fn, dtype);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_gate_mul_fwd(int dtype, int64_t total_voxels, bpx_tensor a, bpx_tensor x, bpx_tensor y, bpx_stream_t stream) {
  BPX_CHECK(a.cs == 0 && x.cs == 0 && y.cs == 0, "bpx_gate_mul_fwd: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_gate_mul_fwd";
  BPX_CHECK(a.ptr && x.ptr && y.ptr, "%s: null pointer", fn);
  const int kpl = dtype == BPX_F32 ? 4 : 8;
  BPX_CHECK(x.C == y.C && x.C % kpl == 0 && x.ld % kpl == 0 && y.ld % kpl == 0, "%s: channel counts / strides must be multiples of %d", fn, kpl);
  if (total_voxels == 0) return 0;
  const int blocks = grid_for(total_voxels * (x.C / kpl));
  if (dtype == BPX_BF16) gate_mul_fwd_kernel<uint16_t><<<blocks, 256, 0, (hipStream_t)stream>>>((const uint16_t*)a.ptr, a.ld, (const uint16_t*)x.ptr, x.ld, (uint16_t*)y.ptr, y.ld, x.C, total_voxels);
  else if (dtype == BPX_F16) gate_mul_fwd_kernel<f16_t><<<blocks, 256, 0, (hipStream_t)stream>>>((const f16_t*)a.ptr, a.ld, (const f16_t*)x.ptr, x.ld, (f16_t*)y.ptr, y.ld, x.C, total_voxels);
  else if (dtype == BPX_F32) gate_mul_fwd_kernel<float><<<blocks, 256, 0, (hipStream_t)stream>>>((const float*)a.ptr, a.ld, (const float*)x.ptr, x.ld, (float*)y.ptr, y.ld, x.C, total_voxels);
  else BPX_FAIL("%s: dtype must be BF16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_gate_mul_bwd(int dtype, int64_t total_voxels, bpx_tensor dy, bpx_tensor a, bpx_tensor x, bpx_tensor dx, void* da16_d, bpx_stream_t stream) {
  BPX_CHECK(dy.cs == 0 && a.cs == 0 && x.cs == 0 && dx.cs == 0, "bpx_gate_mul_bwd: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_gate_mul_bwd";
  BPX_CHECK(dy.ptr && a.ptr && x.ptr && dx.ptr && da16_d, "%s: null pointer", fn);
  const int kpl = dtype == BPX_F32 ? 4 : 8;
  BPX_CHECK(x.C == dy.C && x.C == dx.C && x.C % kpl == 0 && x.ld % kpl == 0 && dy.ld % kpl == 0 && dx.ld % kpl == 0,
            "%s: channel counts / strides must be multiples of %d", fn, kpl);
  if (total_voxels == 0) return 0;
  const int blocks = grid_for(total_voxels);
  if (dtype == BPX_BF16) gate_mul_bwd_kernel<uint16_t><<<blocks, 256, 0, (hipStream_t)stream>>>((const uint16_t*)dy.ptr, dy.ld, (const uint16_t*)a.ptr, a.ld, (const uint16_t*)x.ptr, x.ld, (uint16_t*)dx.ptr, dx.ld, (uint16_t*)da16_d, x.C, total_voxels);
  else if (dtype == BPX_MIX16) gate_mul_bwd_kernel<uint16_t, f16_t><<<blocks, 256, 0, (hipStream_t)stream>>>((const uint16_t*)dy.ptr, dy.ld, (const f16_t*)a.ptr, a.ld, (const f16_t*)x.ptr, x.ld, (uint16_t*)dx.ptr, dx.ld, (uint16_t*)da16_d, x.C, total_voxels);
  else if (dtype == BPX_F32) gate_mul_bwd_kernel<float><<<blocks, 256, 0, (hipStream_t)stream>>>((const float*)dy.ptr, dy.ld, (const float*)a.ptr, a.ld, (const float*)x.ptr, x.ld, (float*)dx.ptr, dx.ld, (float*)da16_d, x.C, total_voxels);
  else BPX_FAIL("%s: dtype must be BF16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
