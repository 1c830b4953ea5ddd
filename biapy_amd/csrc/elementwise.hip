// HBM-bound kernels around the convolutions: normalisation statistics, InstanceNorm backward,
// max-pooling, the 1x1x1 output head, the Cin=1 first layer, weight packing, casts and a lane-layout
// self test.  All of them stream NDHWC tensors with 16-byte accesses along the channel axis.
#include <type_traits>

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
    __shared__ float r1red[4][2][KPL];
#pragma unroll
    for (int e = 0; e < KPL; ++e) {
      float a = r1acc[e];
#pragma unroll
      for (int m = 2; m < 64; m <<= 1) a += __shfl_xor(a, m, 64);
      if ((threadIdx.x & 63) < 2) r1red[threadIdx.x >> 6][threadIdx.x & 1][e] = a;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
      const int par = threadIdx.x >> 3, e = threadIdx.x & 7;
      r1part[(size_t)blockIdx.x * 16 + threadIdx.x] = (r1red[0][par][e] + r1red[1][par][e]) + (r1red[2][par][e] + r1red[3][par][e]);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// output head (1x1x1 conv to <= 8 fp32 channels, planar output) and its backward
// ------------------------------------------------------------------------------------------------
// COUT is a template parameter (one instance per channel count 1..8): every channel loop unrolls and a[] stays in registers.  The arithmetic is
// that of the former run-time-Cout kernel, operation for operation (same fmaf chain per channel, same softmax order), so Cout <= 4 is bit-identical.
template <typename T, int CIN, int COUT>
__global__ void __launch_bounds__(256) head_fwd_kernel(const T* __restrict__ x, int x_ld, const float* __restrict__ w,
                                                       const float* __restrict__ b, int act, float* __restrict__ out,
                                                       int64_t sn, int64_t sc, int64_t vps, int N) {
  constexpr int KPL = ElemTraits<T>::KPL;
  __shared__ float ws[COUT * CIN + COUT];
  for (int i = threadIdx.x; i < COUT * CIN; i += blockDim.x) ws[i] = w[i];
  if (threadIdx.x < COUT) ws[COUT * CIN + threadIdx.x] = b ? b[threadIdx.x] : 0.f;
  __syncthreads();
  // per-channel codes, 4 bits each (channel 0 in the low nibble): 0 linear, 1 sigmoid, 2 tanh, 3 softmax - consecutive
  // softmax channels form ONE group (apply_model_activations, base_workflow.py:1403-1457); a head may hold several groups.
  // gend[co]: last channel of the softmax group that starts at co, or -1 (no group starts there)
  int gend[COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
    gend[co] = -1;
    if (((act >> (4 * co)) & 15) == 3 && (co == 0 || ((act >> (4 * (co - 1))) & 15) != 3)) {
      int e = co;
      while (e + 1 < COUT && ((act >> (4 * (e + 1))) & 15) == 3) ++e;
      gend[co] = e;
    }
  }
  const int64_t total = (int64_t)N * vps;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    // the weights are re-read from LDS in every iteration: hoisted out of the loop (the channel loops are unrolled) they took up to
    // COUT * CIN VGPRs - occupancy 8 -> 4 at Cout 4 and AGPR spills at CIN 32
    asm volatile("" ::: "memory");
    float f[CIN];
#pragma unroll
    for (int q = 0; q < CIN / KPL; ++q) unpack16<T>(*reinterpret_cast<const u32x4_t*>(x + (size_t)i * x_ld + q * KPL), f + q * KPL);
    int n = (int)(i / vps);
    int64_t v = i - (int64_t)n * vps;
    float a[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
      a[co] = ws[COUT * CIN + co];
#pragma unroll
      for (int c = 0; c < CIN; ++c) a[co] = fmaf(f[c], ws[co * CIN + c], a[co]);
    }
    // channel order, as before; a group's members are addressed with compile-time indices under the run-time bound e = gend[co]
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
      const int code = (act >> (4 * co)) & 15;
      if (code == 1) a[co] = 1.f / (1.f + expf(-a[co]));
      else if (code == 2) a[co] = tanhf(a[co]);
      else if (gend[co] >= 0) {
        const int e = gend[co];
        float m = a[co];
#pragma unroll
        for (int k = co + 1; k < COUT; ++k) if (k <= e) m = fmaxf(m, a[k]);
        float ssum = 0.f;
#pragma unroll
        for (int k = co; k < COUT; ++k) if (k <= e) { a[k] = expf(a[k] - m); ssum += a[k]; }
#pragma unroll
        for (int k = co; k < COUT; ++k) if (k <= e) a[k] /= ssum;
      }
    }
#pragma unroll
    for (int co = 0; co < COUT; ++co) out[n * sn + co * sc + v] = a[co];
  }
}

// TX: element type of the head's input x (BPX_MIX16: fp16 beside the bf16 gradient dx), else T
template <typename T, int CIN, int COUT, typename TX = T>
__global__ void __launch_bounds__(256) head_bwd_kernel(const TX* __restrict__ x, int x_ld, const float* __restrict__ w, int Cout,
                                                       const float* __restrict__ dout, int64_t sn, int64_t sc, T* __restrict__ dx,
                                                       int dx_ld, float* __restrict__ dw, float* __restrict__ db, int64_t vps, int N) {
  constexpr int KPL = ElemTraits<T>::KPL;
  __shared__ float ws[COUT * CIN];
  for (int i = threadIdx.x; i < Cout * CIN; i += blockDim.x) ws[i] = w[i];
  __syncthreads();
  float dwl[COUT][CIN];
  float dbl[COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
    dbl[co] = 0.f;
#pragma unroll
    for (int c = 0; c < CIN; ++c) dwl[co][c] = 0.f;
  }
  const int64_t total = (int64_t)N * vps;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    float f[CIN], o[CIN];
#pragma unroll
    for (int q = 0; q < CIN / KPL; ++q) unpack16<TX>(*reinterpret_cast<const u32x4_t*>(x + (size_t)i * x_ld + q * KPL), f + q * KPL);
#pragma unroll
    for (int c = 0; c < CIN; ++c) o[c] = 0.f;
    int n = (int)(i / vps);
    int64_t v = i - (int64_t)n * vps;
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
      {
        float d = dout[n * sn + co * sc + v];
        dbl[co] += d;
#pragma unroll
        for (int c = 0; c < CIN; ++c) { o[c] = fmaf(d, ws[co * CIN + c], o[c]); dwl[co][c] = fmaf(d, f[c], dwl[co][c]); }
      }
    }
#pragma unroll
    for (int q = 0; q < CIN / KPL; ++q) *reinterpret_cast<u32x4_t*>(dx + (size_t)i * dx_ld + q * KPL) = pack16<T>(o + q * KPL);
  }
  // block reduction (wave shuffles, then LDS across the 4 waves) -> one partial per value per block
  __shared__ float redh[4][COUT * CIN + COUT];
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
#pragma unroll
    for (int c = 0; c < CIN; ++c) {
      float a = dwl[co][c];
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) a += __shfl_xor(a, m, 64);
      if (ln == 0) redh[wv][co * CIN + c] = a;
    }
    float a = dbl[co];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) a += __shfl_xor(a, m, 64);
    if (ln == 0) redh[wv][COUT * CIN + co] = a;
  }
  __syncthreads();
  // one row of partials per workgroup ([blocks][COUT*CIN] and [blocks][COUT]); bpxred::reduce_partials sums the rows in a fixed order
  for (int i = threadIdx.x; i < COUT * CIN + COUT; i += blockDim.x) {
    float sum = redh[0][i] + redh[1][i] + redh[2][i] + redh[3][i];
    if (i < COUT * CIN) dw[(size_t)blockIdx.x * (COUT * CIN) + i] = sum;
    else if (db) db[(size_t)blockIdx.x * COUT + (i - COUT * CIN)] = sum;
  }
}

// Cout 5..8: the input channels are split into 16-channel slices, one workgroup each (the accumulators of head_bwd_kernel would not fit: COUT = 4 at
// CIN = 32 already takes 256 VGPRs).  Slice s reads every dout channel but only x[:, s] and w[:, s]; it writes dx[:, s] (no cross-slice sum) and
// the dW[:, s] columns of its workgroup column's partial row.  Per thread: dwl[COUT][16] + o[16] + f[16].  The numerics are head_bwd_kernel's: fp32
// dout, per-thread fmaf chains in channel order, wave shuffles, the four waves in a fixed order, then bpxred::reduce_partials over the rows.
// 1-D grid of ncol * (Cin / 16) workgroups: the slices of one column are 8 workgroups apart - the same XCD (workgroups go round-robin over the
// eight), dispatched together - so the halves of one x row are read, and the halves of one dx row written, at about the same time.  With the slice
// in blockIdx.y every column of slice 0 ran before slice 1 began: each x line came from HBM twice and dx went out in half lines (Cin 32, Cout 8:
// 775 us at 4 x 128^3).
template <typename T, int COUT, typename TX = T>
__global__ void __launch_bounds__(256) head_bwd_slice_kernel(const TX* __restrict__ x, int x_ld, const float* __restrict__ w, int Cin,
                                                             const float* __restrict__ dout, int64_t sn, int64_t sc, T* __restrict__ dx,
                                                             int dx_ld, float* __restrict__ dw, float* __restrict__ db, int64_t vps, int N) {
  constexpr int KPL = ElemTraits<T>::KPL, CS = 16;
  static_assert(ElemTraits<TX>::KPL == KPL, "x and dx: the same element size");
  const int nsl = Cin / CS, ncol = (int)gridDim.x / nsl;
  const int sl = (int)(blockIdx.x >> 3) % nsl, col = (int)(blockIdx.x / (8 * nsl)) * 8 + (int)(blockIdx.x & 7);
  const int c0 = sl * CS;
  __shared__ float ws[COUT * CS];
  for (int i = threadIdx.x; i < COUT * CS; i += blockDim.x) ws[i] = w[(i / CS) * Cin + c0 + i % CS];
  __syncthreads();
  float dwl[COUT][CS];
  float dbl[COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
    dbl[co] = 0.f;
#pragma unroll
    for (int c = 0; c < CS; ++c) dwl[co][c] = 0.f;
  }
  const int64_t total = (int64_t)N * vps;
  for (int64_t i = (int64_t)col * blockDim.x + threadIdx.x; i < total; i += (int64_t)ncol * blockDim.x) {
    asm volatile("" ::: "memory");   // w[:, s] from LDS in every iteration (see head_fwd_kernel): the accumulators need the registers
    float f[CS], o[CS];
#pragma unroll
    for (int q = 0; q < CS / KPL; ++q) unpack16<TX>(*reinterpret_cast<const u32x4_t*>(x + (size_t)i * x_ld + c0 + q * KPL), f + q * KPL);
#pragma unroll
    for (int c = 0; c < CS; ++c) o[c] = 0.f;
    int n = (int)(i / vps);
    int64_t v = i - (int64_t)n * vps;
    float d[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) d[co] = dout[n * sn + co * sc + v];
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
      dbl[co] += d[co];
#pragma unroll
      for (int c = 0; c < CS; ++c) { o[c] = fmaf(d[co], ws[co * CS + c], o[c]); dwl[co][c] = fmaf(d[co], f[c], dwl[co][c]); }
    }
#pragma unroll
    for (int q = 0; q < CS / KPL; ++q) *reinterpret_cast<u32x4_t*>(dx + (size_t)i * dx_ld + c0 + q * KPL) = pack16<T>(o + q * KPL);
  }
  __shared__ float redh[4][COUT * CS + COUT];
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
#pragma unroll
    for (int c = 0; c < CS; ++c) {
      float a = dwl[co][c];
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) a += __shfl_xor(a, m, 64);
      if (ln == 0) redh[wv][co * CS + c] = a;
    }
    float a = dbl[co];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) a += __shfl_xor(a, m, 64);
    if (ln == 0) redh[wv][COUT * CS + co] = a;
  }
  __syncthreads();
  // this slice's columns of the workgroup-column's partial row ([blocks][COUT][Cin]); the bias row ([blocks][COUT]) from slice 0
  for (int i = threadIdx.x; i < COUT * CS + COUT; i += blockDim.x) {
    float sum = redh[0][i] + redh[1][i] + redh[2][i] + redh[3][i];
    if (i < COUT * CS) dw[(size_t)col * (COUT * Cin) + (i / CS) * Cin + c0 + i % CS] = sum;
    else if (db && sl == 0) db[(size_t)col * COUT + (i - COUT * CS)] = sum;
  }
}

// ------------------------------------------------------------------------------------------------
// first layer: Cin = 1, k = 3, fp32 image -> 16 output channels per blockIdx.y
// ------------------------------------------------------------------------------------------------
// Implicit GEMM with K = 27 taps (padded to 32 / 28): the image halo tile sits in LDS as fp32, a lane gathers the taps
// of its voxel straight from it.  bf16 storage: the fp32 image value is split into hi + lo bf16 parts (two MFMAs) so the
// raw input keeps ~16 mantissa bits; the weights are rounded to bf16 like every other layer in that mode.
// BUF (round 5): image and output move through BUFFER instructions - a halo voxel outside the volume / a tile beyond the launch's range / an output
// voxel outside the volume uses an out-of-range offset (loads return the zero padding, stores are dropped) instead of a predicate.  With predicated
// loads the compiler's wait at the loop head for the prefetched halo was `s_waitcnt vmcnt(0)` (its wait-count pass gives up at the joins of the
// bounds tests), i.e. a wait for the previous tile's 8 stores as well - what the prefetch-before-the-stores order was meant to avoid; now the
// wait is a counted one that leaves the stores in flight.  The launcher takes BUF when image and output lie within 32-bit byte offsets.
template <typename T, bool BUF>
__global__ void __launch_bounds__(256) conv_c1_fwd_kernel(const float* __restrict__ img, const float* __restrict__ w /* (Cout,1,27) */,
                                                          const float* __restrict__ bias, T* __restrict__ y, int y_ld, int Cout, int D,
                                                          int H, int W, int tilesY, int tilesX, int tilesPerSample, float* __restrict__ part, int totalTiles,
                                                          uint32_t img_bytes, uint32_t y_bytes) {
  constexpr bool BF = sizeof(T) == 2;   // 16-bit storage (bf16 bits or fp16): hi + lo split of the fp32 image, two MFMAs
  constexpr int TZ = 4, TY = 8, TX = 16, HZ = TZ + 2, HY = TY + 2, HX = TX + 2, HV = HZ * HY * HX, MS = 8;
  __shared__ float simg[HV];
  __shared__ float red[4][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int cb = blockIdx.y * 16;
  // Round 4: persistent workgroups.  As one workgroup per tile the kernel was bound by the LIFE of a workgroup - image load latency, 16 MFMAs,
  // then its stores' write acknowledgements before the slot frees - at 2.1 TB/s written (0.144 ms at 4 x 128^3).  The image halo of the NEXT tile
  // is requested into registers (five floats per thread) BEFORE this tile's stores: a wave's VMEM operations retire in order, so the wait for
  // those loads then leaves the stores outstanding; weights / tap offsets / bias are set up once.
  constexpr int NI = (HV + 255) / 256;
  float pi[NI];
  const __amdgpu_buffer_rsrc_t rs_img = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(img), 0, (int)img_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc(y, 0, (int)y_bytes, 0x00020000);
  // BUF: the halo voxel (hz, hy, hx) a thread stages is the same for every tile - its coordinates (one packed word per piece) and its offset
  // relative to the tile's first voxel are set up once; a tile costs three unsigned range tests and one add per piece.  (As written for the
  // pointer-addressed instance - the divisions by HX / HY inside the tile loop - the five requests were 200 of the loop's 1060 instructions, and
  // the kernel is bound by instruction issue: ~1000 instructions per tile and wave = the 105 us it takes.)
  uint32_t hpk[BUF ? NI : 1];
  int hrel[BUF ? NI : 1];
  if constexpr (BUF) {
#pragma unroll
    for (int u = 0; u < NI; ++u) {
      const int i = u * 256 + tid;
      const int hx = i % HX, hy = (i / HX) % HY, hz = i / (HX * HY);
      hpk[u] = i < HV ? (uint32_t)(hz | (hy << 8) | (hx << 16)) : 0xFFFFFFFFu;
      hrel[u] = ((hz - 1) * H + (hy - 1)) * W + (hx - 1);
    }
  }
  auto issue = [&](int tt) {
    const int n_ = tt / tilesPerSample, tile_ = tt - n_ * tilesPerSample;
    const int x0_ = (tile_ % tilesX) * TX, y0_ = ((tile_ / tilesX) % tilesY) * TY, z0_ = (tile_ / (tilesX * tilesY)) * TZ;
    if constexpr (BUF) {
      const int base = ((n_ * D + z0_) * H + y0_) * W + x0_;
      const bool live = tt < totalTiles;
#pragma unroll
      for (int u = 0; u < NI; ++u) {
        // z0 + hz - 1 in [0, D) <=> (unsigned)(z0 - 1 + hz) < D; a piece beyond the halo has hz = 255: out of every volume the launcher admits
        const uint32_t z = (uint32_t)(z0_ - 1) + (hpk[u] & 255u), yy = (uint32_t)(y0_ - 1) + ((hpk[u] >> 8) & 255u), x = (uint32_t)(x0_ - 1) + (hpk[u] >> 16);
        const bool in = live && hpk[u] != 0xFFFFFFFFu && z < (uint32_t)D && yy < (uint32_t)H && x < (uint32_t)W;
        pi[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_img, (int)(in ? (uint32_t)(base + hrel[u]) * 4u : 0xFFFFFFF0u), 0, 0));
      }
    } else {
#pragma unroll
      for (int u = 0; u < NI; ++u) {
        const int i = u * 256 + tid;
        const int hx = i % HX, hy = (i / HX) % HY, hz = i / (HX * HY);
        const int z = z0_ + hz - 1, yy = y0_ + hy - 1, x = x0_ + hx - 1;
        pi[u] = (i < HV && z >= 0 && z < D && yy >= 0 && yy < H && x >= 0 && x < W) ? img[(((size_t)n_ * D + z) * H + yy) * W + x] : 0.f;
      }
    }
  };
  if (BUF || (int)blockIdx.x < totalTiles) issue(blockIdx.x);
  // weight operand of this lane: output channel cb + j, taps 8g..8g+7 (bf16) or 4s+g (f32)
  u32x4_t wa = u32x4_t{0u, 0u, 0u, 0u};
  float wf32[7];
  int toff[BF ? 8 : 7];
  if constexpr (BF) {
    float wv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int t = 8 * g + e;
      wv[e] = t < 27 ? w[(size_t)(cb + j) * 27 + t] : 0.f;
      int tc = t < 27 ? t : 26;
      toff[e] = ((tc / 9) * HY + (tc / 3) % 3) * HX + tc % 3;
    }
    wa = pack16<T>(wv);
  } else {
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      int t = 4 * s + g;
      wf32[s] = t < 27 ? w[(size_t)(cb + j) * 27 + t] : 0.f;
      int tc = t < 27 ? t : 26;
      toff[s] = ((tc / 9) * HY + (tc / 3) % 3) * HX + tc % 3;
    }
  }
  float bsv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bsv[r] = bias ? bias[cb + 4 * g + r] : 0.f;
  for (int tt = blockIdx.x; tt < totalTiles; tt += gridDim.x) {
  const int n = tt / tilesPerSample, tile = tt - n * tilesPerSample;
  const int x0 = (tile % tilesX) * TX, y0 = ((tile / tilesX) % tilesY) * TY, z0 = (tile / (tilesX * tilesY)) * TZ;
  __syncthreads();                                   // the previous tile's reads of simg / red are done
  // 16-bit storage (round 5): the hi + lo split happens HERE, once per halo voxel (5 values per thread), and LDS holds the pair as one word
  // (hi in the low half); the gather below then builds the two MFMA operands with two byte permutes per pair of taps.  Before, every lane split
  // the 8 gathered taps of each of its 8 voxels itself: 24 conversions / subtractions per m-subtile, ~40 % of the kernel's VALU work.  Same
  // conversions of the same values: same bits.
#pragma unroll
  for (int u = 0; u < NI; ++u)
    if (u * 256 + tid < HV) {
      if constexpr (BF) {
        const float f = pi[u];
        const float hf = lo16<T>(pk16<T>(f, 0.f));
        simg[u * 256 + tid] = __uint_as_float(pk16<T>(f, f - hf));
      } else {
        simg[u * 256 + tid] = pi[u];
      }
    }
  __syncthreads();
  if (BUF || tt + (int)gridDim.x < totalTiles) issue(tt + gridDim.x);   // (BUF: a tile beyond the range requests nothing - every lane out of range)
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  const uint32_t ybase = ((uint32_t)(((n * D + z0 + wave) * H + y0) * W + x0 + j) * (uint32_t)y_ld + (uint32_t)(cb + 4 * g)) * (uint32_t)sizeof(T);
  const uint32_t yrowb = (uint32_t)(W * y_ld) * (uint32_t)sizeof(T);
  const bool full = z0 + TZ <= D && y0 + TY <= H && x0 + TX <= W;       // (uniform)
  f32x2_t p1[2] = {f32x2_t{0.f, 0.f}, f32x2_t{0.f, 0.f}}, p2[2] = {f32x2_t{0.f, 0.f}, f32x2_t{0.f, 0.f}};   // BUF: s1 / s2 as pairs
#pragma unroll
  for (int ms = 0; ms < MS; ++ms) {
    int t = (wave * MS + ms) * 16 + j;
    int tz = t / (TY * TX), ty = (t / TX) % TY, tx = t % TX;
    const float* base = simg + (tz * HY + ty) * HX + tx;
    f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if constexpr (BF) {
      uint32_t v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = __float_as_uint(base[toff[e]]);
      u32x4_t hi, lov;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        hi[k] = __builtin_amdgcn_perm(v[2 * k + 1], v[2 * k], 0x05040100u);    // the low halves (hi parts) of taps 2k, 2k + 1
        lov[k] = __builtin_amdgcn_perm(v[2 * k + 1], v[2 * k], 0x07060302u);   // the high halves (lo parts)
      }
      acc = mfma_step<T>(wa, hi, acc);
      acc = mfma_step<T>(wa, lov, acc);
    } else {
#pragma unroll
      for (int s = 0; s < 7; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf32[s], base[toff[s]], acc, 0, 0, 0);
    }
    int z = z0 + tz, yy = y0 + ty, x = x0 + tx;
    const bool inside = z < D && yy < H && x < W;
    if constexpr (BUF) {
      // (packed fp32 pairs: the same additions / multiplications, half the instructions; the outside-the-volume select only on a partial tile)
      const f32x2_t va = f32x2_t{acc[0], acc[1]} + f32x2_t{bsv[0], bsv[1]}, vb = f32x2_t{acc[2], acc[3]} + f32x2_t{bsv[2], bsv[3]};
      const float v4[4] = {va[0], va[1], vb[0], vb[1]};
      f32x2_t sa = va, sb = vb;
      if (!full && !inside) sa = sb = f32x2_t{0.f, 0.f};
      p1[0] = p1[0] + sa; p1[1] = p1[1] + sb;
      p2[0] = p2[0] + sa * sa; p2[1] = p2[1] + sb * sb;
      // (t = (wave MS + ms) 16 + j: tz = wave, ty = ms, tx = j - the voxel's offset is the m-subtile-0 offset of this lane + ms rows)
      const uint32_t off = inside ? ybase + (uint32_t)ms * yrowb : 0xFFFFFFF0u;
      if constexpr (BF) __builtin_amdgcn_raw_buffer_store_b64(u32x2_t{pk16s<T>(v4[0], v4[1]), pk16s<T>(v4[2], v4[3])}, rs_y, (int)off, 0, 0);
      else __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{__float_as_uint(v4[0]), __float_as_uint(v4[1]), __float_as_uint(v4[2]), __float_as_uint(v4[3])}, rs_y, (int)off, 0, 0);
    } else if (inside) {
      float v4[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) { v4[r] = acc[r] + bsv[r]; s1[r] += v4[r]; s2[r] += v4[r] * v4[r]; }
      T* yp = y + ((((size_t)n * D + z) * H + yy) * W + x) * (size_t)y_ld + cb + 4 * g;
      if constexpr (BF) *reinterpret_cast<u32x2_t*>(yp) = u32x2_t{pk16s<T>(v4[0], v4[1]), pk16s<T>(v4[2], v4[3])};
      else *reinterpret_cast<f32x4_t*>(yp) = f32x4_t{v4[0], v4[1], v4[2], v4[3]};
    }
  }
  if (part) {
    if constexpr (BUF) {
      const f32x2_t q0 = p1[0], q1 = p1[1], q2 = p2[0], q3 = p2[1];   // (copies first: elements of an array of vectors, see bpx_common.h)
      s1[0] = q0[0]; s1[1] = q0[1]; s1[2] = q1[0]; s1[3] = q1[1];
      s2[0] = q2[0]; s2[1] = q2[1]; s2[2] = q3[0]; s2[3] = q3[1];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // (row16_sum pairs lanes as the xor butterfly it replaces did - 1, 2, then the other quad of the half, then the other half - the same
      //  additions of the same values: same bits; four DPP adds instead of four cross-lane shuffles each)
      const float a = row16_sum(s1[r]), b = row16_sum(s2[r]);
      if (j == 0) { red[wave][4 * g + r] = a; red[wave][16 + 4 * g + r] = b; }
    }
    __syncthreads();
    if (tid < 32) {
      int k = tid >> 4, c = tid & 15;
      float s = red[0][k * 16 + c] + red[1][k * 16 + c] + red[2][k * 16 + c] + red[3][k * 16 + c];
      part[(((size_t)n * tilesPerSample + tile) * 2 + k) * Cout + cb + c] = s;
    }
  }
  }   // tiles of this workgroup
}

// dW[co][tap] += sum_v img[v+tap]*dy[v][co]; thread = (tap, voxel subset), 16 co in registers.
template <typename T>
__global__ void __launch_bounds__(256) conv_c1_wgrad_kernel(const float* __restrict__ img, const T* __restrict__ dy, int dy_ld,
                                                            int D, int H, int W, int N, int totalTiles, float* __restrict__ dw,
                                                            float* __restrict__ db) {
  constexpr int TZ = 4, TY = 8, TX = 8, HZ = TZ + 2, HY = TY + 2, HX = TX + 2;
  __shared__ float simg[HZ * HY * HX];
  __shared__ __attribute__((aligned(16))) float sdy[TZ * TY * TX][16];
  __shared__ float sred[9][27 + 1][16];
  const int cb = blockIdx.y * 16;
  const int tap = threadIdx.x % 27, sub = threadIdx.x / 27;  // sub 0..8 active (243 threads)
  const bool worker = threadIdx.x < 243;
  const int toff = ((tap / 9) * HY + (tap / 3) % 3) * HX + tap % 3;
  float acc[16], bs[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) { acc[c] = 0.f; bs[c] = 0.f; }
  const int tilesX = cdiv(W, TX), tilesY = cdiv(H, TY), tilesZ = cdiv(D, TZ);
  const int tps = tilesX * tilesY * tilesZ;
  for (int tt = blockIdx.x; tt < totalTiles; tt += gridDim.x) {
    const int n = tt / tps, tile = tt % tps;
    const int x0 = (tile % tilesX) * TX, y0 = ((tile / tilesX) % tilesY) * TY, z0 = (tile / (tilesX * tilesY)) * TZ;
    __syncthreads();
    for (int i = threadIdx.x; i < HZ * HY * HX; i += 256) {
      int hx = i % HX, hy = (i / HX) % HY, hz = i / (HX * HY);
      int z = z0 + hz - 1, y = y0 + hy - 1, x = x0 + hx - 1;
      simg[i] = (z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W) ? img[(((size_t)n * D + z) * H + y) * W + x] : 0.f;
    }
    {  // dy tile -> fp32 in LDS, moved as 16-byte pieces (KPL channels per piece)
      constexpr int KPL = ElemTraits<T>::KPL, PPV = 16 / KPL;
#pragma unroll
      for (int u = 0; u < TZ * TY * TX * PPV / 256; ++u) {
        const int i = u * 256 + threadIdx.x, t = i / PPV, sp = i % PPV;
        const int x = x0 + t % TX, y = y0 + (t / TX) % TY, z = z0 + t / (TX * TY);
        float f[KPL];
#pragma unroll
        for (int e = 0; e < KPL; ++e) f[e] = 0.f;
        if (z < D && y < H && x < W)
          unpack16<T>(*reinterpret_cast<const u32x4_t*>(dy + ((((size_t)n * D + z) * H + y) * W + x) * dy_ld + cb + sp * KPL), f);
#pragma unroll
        for (int q = 0; q < KPL / 4; ++q)
          *reinterpret_cast<f32x4_t*>(&sdy[t][sp * KPL + q * 4]) = f32x4_t{f[q * 4], f[q * 4 + 1], f[q * 4 + 2], f[q * 4 + 3]};
      }
    }
    __syncthreads();
    if (worker) {
      for (int t = sub; t < TZ * TY * TX; t += 9) {
        int tx = t % TX, ty = (t / TX) % TY, tz = t / (TX * TY);
        float iv = simg[(tz * HY + ty) * HX + tx + toff];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4_t d = *reinterpret_cast<const f32x4_t*>(&sdy[t][q * 4]);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[q * 4 + e] = fmaf(iv, d[e], acc[q * 4 + e]);
            if (tap == 0) bs[q * 4 + e] += d[e];
          }
        }
      }
    }
  }
  __syncthreads();
  if (worker) {
#pragma unroll
    for (int c = 0; c < 16; ++c) { sred[sub][tap][c] = acc[c]; if (tap == 0) sred[sub][27][c] = bs[c]; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 28 * 16; i += 256) {
    int t = i / 16, c = i % 16;
    float s = 0.f;
    for (int q = 0; q < 9; ++q) s += sred[q][t][c];
    // partial slab of this workgroup column: dw = [gridDim.x][27][Cout], db = [gridDim.x][Cout] (Cout = 16 * gridDim.y)
    const int Cout = 16 * gridDim.y;
    if (t < 27) dw[((size_t)blockIdx.x * 27 + t) * Cout + cb + c] = s;
    else if (db) db[(size_t)blockIdx.x * Cout + cb + c] = s;
  }
}


// The same on the matrix cores (bf16 dy): D[tap][co] += sum_v A[tap][v] * G[v][co] with K = 32 voxels per MFMA step.
// A = image patches (fp32 in LDS, split hi + lo into two bf16 operands exactly like conv_c1_fwd_kernel, so the image keeps
// ~16 mantissa bits), two 16-row blocks for the 27 taps; row 27 is all ones -> D[27][co] = sum_v dy = the bias gradient.
// G = dy^T fragments through ds_read_b64_tr_b16.  Wave w owns K-chunks {2w, 2w+1} of every 4x4x16 tile.
// NB (round 4): dy is not read but formed on the way into LDS from the InstanceNorm-backward operands of the layer's output,
//   dy = a[n,c] * g + b[n,c] * t + c0[n,c]   (bpx_norm_bwd_finalize's coefficients; t = the conv's raw output, TT = fp16 in the mixed mode)
// in the arithmetic of norm_bwd_apply_kernel and rounded to bf16 as that kernel's store would: the pass that wrote dy (3 tensor units of
// traffic at 128^3, 139 us per cfg-2 step) is gone and this kernel reads two units instead of one.
// BUF (round 5): image, dy and t arrive through buffer loads with out-of-range offsets for voxels outside the volume and for tiles beyond the
// launch, requested unconditionally.  With predicated loads every wait for a staged tile was `s_waitcnt vmcnt(0)` (the wait-count pass gives up at
// the joins of the bounds tests): the wait for tile i also waited for tile i + 1's requests, issued later - the two-tiles-ahead staging ran one
// tile ahead.  The sample's coefficients are re-read behind a SCALAR branch (they were re-loaded for every tile: 8 more 16-byte loads per thread,
// as many VMEM instructions as the tile's own operands).
template <typename TT, bool NB, bool BUF>
__global__ void __launch_bounds__(256) conv_c1_wgrad_mfma_kernel(const float* __restrict__ img, const uint16_t* __restrict__ dy, int dy_ld,
                                                                 int D, int H, int W, int N, int totalTiles, float* __restrict__ dw,
                                                                 float* __restrict__ db, const TT* __restrict__ tsrc, int t_ld,
                                                                 const bpx_nbwd_coef* __restrict__ coef, uint32_t img_bytes, uint32_t dy_bytes,
                                                                 uint32_t t_bytes) {
  constexpr int TZ = 4, TY = 4, TX = 16, TV = TZ * TY * TX, HZ = TZ + 2, HY = TY + 2, HX = TX + 2, HV = HZ * HY * HX;
  constexpr int VBG = 32;
  __shared__ float simg[HV + 8];
  __shared__ __attribute__((aligned(16))) unsigned char sG[TV * VBG];
  __shared__ float sred[4][2][64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int cb = blockIdx.y * 16;
  f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
  // this lane's two taps (rows i and 16 + i) as float offsets into the halo image; row 27 = ones, rows 28..31 unused
  int toff[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int tap = b * 16 + i;
    toff[b] = tap < 27 ? ((tap / 9) * HY + (tap / 3) % 3) * HX + tap % 3 : -1;
  }
  const int tilesX = cdiv(W, TX), tilesY = cdiv(H, TY), tilesZ = cdiv(D, TZ);
  const int tps = tilesX * tilesY * tilesZ;
  // register-prefetched staging, TWO tiles ahead (round 4; one tile ahead until then): the MFMA part is tiny, the kernel is pure load latency - with
  // the operands of one tile in flight per workgroup an iteration was a full memory latency (3.3 TB/s with the folded IN-backward operands)
  constexpr int NI = (HV + 255) / 256;
  struct Stage { float pi[NI]; u32x4_t pg[2]; u32x4_t pt[NB ? 2 : 1]; };
  Stage st0, st1;
  f32x4_t ck[NB ? 8 : 1];   // {a, b, c0, -} of this thread's 8 channels in the current sample
  int cur_n = -1;
  const __amdgpu_buffer_rsrc_t rs_img = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(img), 0, (int)img_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_dy = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(dy), 0, (int)dy_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_t = __builtin_amdgcn_make_buffer_rsrc(const_cast<TT*>(tsrc), 0, (int)t_bytes, 0x00020000);
  // BUF: this thread's halo voxels (packed coordinates, offset relative to the tile's first voxel) and tile voxels are the same for every tile
  uint32_t hpk[BUF ? NI : 1];
  int hrel[BUF ? NI : 1];
  if constexpr (BUF) {
#pragma unroll
    for (int u = 0; u < NI; ++u) {
      const int q = u * 256 + tid;
      const int hx = q % HX, hy = (q / HX) % HY, hz = q / (HX * HY);
      hpk[u] = q < HV ? (uint32_t)(hz | (hy << 8) | (hx << 16)) : 0xFFFFFFFFu;
      hrel[u] = ((hz - 1) * H + (hy - 1)) * W + (hx - 1);
    }
  }
  auto issue = [&](int tt, Stage& sg) {
    const int n = tt / tps, tile = tt % tps;
    const int x0 = (tile % tilesX) * TX, y0 = ((tile / tilesX) % tilesY) * TY, z0 = (tile / (tilesX * tilesY)) * TZ;
    if constexpr (BUF) {
      const bool live = tt < totalTiles;
      const int base = ((n * D + z0) * H + y0) * W + x0;
#pragma unroll
      for (int u = 0; u < NI; ++u) {
        const uint32_t z = (uint32_t)(z0 - 1) + (hpk[u] & 255u), y = (uint32_t)(y0 - 1) + ((hpk[u] >> 8) & 255u), x = (uint32_t)(x0 - 1) + (hpk[u] >> 16);
        const bool in = live && hpk[u] != 0xFFFFFFFFu && z < (uint32_t)D && y < (uint32_t)H && x < (uint32_t)W;
        sg.pi[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_img, (int)(in ? (uint32_t)(base + hrel[u]) * 4u : 0xFFFFFFF0u), 0, 0));
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int q = u * 256 + tid, t = q >> 1;
        const int x = x0 + (t & 15), y = y0 + ((t >> 4) & 3), z = z0 + (t >> 6);
        const bool in = live && z < D && y < H && x < W;
        const uint32_t v = (uint32_t)(((n * D + z) * H + y) * W + x);
        sg.pg[u] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rs_dy, (int)(in ? (v * (uint32_t)dy_ld + (uint32_t)(cb + (q & 1) * 8)) * 2u : 0xFFFFFFF0u), 0, 0));
        if (NB) sg.pt[NB ? u : 0] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rs_t, (int)(in ? (v * (uint32_t)t_ld + (uint32_t)(cb + (q & 1) * 8)) * 2u : 0xFFFFFFF0u), 0, 0));
      }
    } else {
#pragma unroll
      for (int u = 0; u < NI; ++u) {
        const int q = u * 256 + tid;
        const int hx = q % HX, hy = (q / HX) % HY, hz = q / (HX * HY);
        const int z = z0 + hz - 1, y = y0 + hy - 1, x = x0 + hx - 1;
        sg.pi[u] = (q < HV && z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W) ? img[(((size_t)n * D + z) * H + y) * W + x] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int q = u * 256 + tid, t = q >> 1;
        const int x = x0 + (t & 15), y = y0 + ((t >> 4) & 3), z = z0 + (t >> 6);
        sg.pg[u] = u32x4_t{0u, 0u, 0u, 0u};
        if (NB) sg.pt[NB ? u : 0] = u32x4_t{0u, 0u, 0u, 0u};
        if (z < D && y < H && x < W) {
          const size_t v = (((size_t)n * D + z) * H + y) * W + x;
          sg.pg[u] = *reinterpret_cast<const u32x4_t*>(dy + v * dy_ld + cb + (q & 1) * 8);
          if (NB) sg.pt[NB ? u : 0] = *reinterpret_cast<const u32x4_t*>(tsrc + v * t_ld + cb + (q & 1) * 8);
        }
      }
    }
  };
  // the staged dy piece: as loaded, or a * g + b * t + c0 (out-of-volume voxels stay zero: their operands were never loaded)
  auto piece = [&](int u, int tt, const Stage& sg) -> u32x4_t {
    if (!NB) return sg.pg[u];
    const int q = u * 256 + tid, t = q >> 1;
    const int tile = tt % tps;
    const int x = (tile % tilesX) * TX + (t & 15), y = ((tile / tilesX) % tilesY) * TY + ((t >> 4) & 3), z = (tile / (tilesX * tilesY)) * TZ + (t >> 6);
    const bool inside = z < D && y < H && x < W;
    if (!BUF && !inside) return u32x4_t{0u, 0u, 0u, 0u};
    float gf[8], tf[8], of[8];
    unpack16<uint16_t>(sg.pg[u], gf);
    unpack16<TT>(sg.pt[NB ? u : 0], tf);
#pragma unroll
    for (int e = 0; e < 8; ++e) { const f32x4_t k = ck[NB ? e : 0]; of[e] = k[0] * gf[e] + k[1] * tf[e] + k[2]; }
    const u32x4_t r = pack16<uint16_t>(of);
    if (BUF) return inside ? r : u32x4_t{0u, 0u, 0u, 0u};          // (a select: no branch between the staged loads and their consumers)
    return r;
  };
  const int step = gridDim.x;
  if (BUF || (int)blockIdx.x < totalTiles) issue(blockIdx.x, st0);
  if (BUF || (int)blockIdx.x + step < totalTiles) issue(blockIdx.x + step, st1);
  auto body = [&](int tt, Stage& sg) {
    if (NB) {
      const int n = BUF ? __builtin_amdgcn_readfirstlane(tt / tps) : tt / tps;
      if (n != (BUF ? __builtin_amdgcn_readfirstlane(cur_n) : cur_n)) {   // (a handful of times per workgroup; BUF: a scalar branch)
        cur_n = n;
        if constexpr (BUF) {
          // through the SCALAR cache (uniform addresses, lgkmcnt): as vector loads they would be the youngest VMEM operations at the staged tile's first
          // use, and the wait for them - on every path, the counts are static - a wait for the prefetched tiles behind them
          const f32x4_t* kp = reinterpret_cast<const f32x4_t*>(coef + (size_t)n * (16 * gridDim.y) + cb);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const f32x4_t lo = kp[e], hi = kp[8 + e];
            ck[NB ? e : 0] = (tid & 1) ? hi : lo;
          }
        } else {
          const f32x4_t* kp = reinterpret_cast<const f32x4_t*>(coef + (size_t)n * (16 * gridDim.y) + cb + (tid & 1) * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) ck[NB ? e : 0] = kp[e];
        }
      }
    }
    __syncthreads();
    // (round 5) the hi + lo bf16 split once per halo voxel, the pair as one LDS word (hi in the low half) - see conv_c1_fwd_kernel
#pragma unroll
    for (int u = 0; u < NI; ++u)
      if (u * 256 + tid < HV) {
        const float f = sg.pi[u];
        simg[u * 256 + tid] = __uint_as_float(cvt_pk_bf16(f, f - bf16lo(cvt_pk_bf16(f, 0.f))));
      }
#pragma unroll
    for (int u = 0; u < 2; ++u) *reinterpret_cast<u32x4_t*>(sG + (size_t)(u * 256 + tid) * 16) = piece(u, tt, sg);
    __syncthreads();
    if (BUF || tt + 2 * step < totalTiles) issue(tt + 2 * step, sg);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int kc = wave * 2 + kk;
      const int t0 = kc * 32 + g * 8;                       // 8 consecutive x voxels of one row
      const int hb = (((t0 >> 6) + 0) * HY + ((t0 >> 4) & 3)) * HX + (t0 & 15);
      u32x4_t gf;
      {
        const unsigned char* q = sG + (t0 + (i >> 2)) * VBG + (i & 3) * 8;
        s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(q));
        s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(q + 4 * VBG));
        u32x2_t l2 = __builtin_bit_cast(u32x2_t, lo), h2 = __builtin_bit_cast(u32x2_t, hi);
        gf = u32x4_t{l2[0], l2[1], h2[0], h2[1]};
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        uint32_t f[8];   // {hi | lo << 16} words; the ones row: bf16(1) = 0x3F80 with lo part 0
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = toff[b] >= 0 ? __float_as_uint(simg[hb + toff[b] + k]) : ((b == 1 && i == 11) ? 0x3F80u : 0u);
        u32x4_t ah, al;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          ah[k] = __builtin_amdgcn_perm(f[2 * k + 1], f[2 * k], 0x05040100u);
          al[k] = __builtin_amdgcn_perm(f[2 * k + 1], f[2 * k], 0x07060302u);
        }
        acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ah), __builtin_bit_cast(bf16x8_t, gf), acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, al), __builtin_bit_cast(bf16x8_t, gf), acc[b], 0, 0, 0);
      }
    }
  };
  if constexpr (BUF) {
    // pairs of tiles in a loop whose every trip runs both bodies, the odd last tile behind it: with the second body under a test inside the loop
    // there is a static path on which stage 1 was not refilled, and the first body's waits are counted for THAT path (vmcnt(6 .. 0): a wait for
    // stage 1's requests as well)
    int tt = blockIdx.x;
    for (; tt + step < totalTiles; tt += 2 * step) {
      body(tt, st0);
      body(tt + step, st1);
    }
    if (tt < totalTiles) body(tt, st0);
  } else {
    for (int tt = blockIdx.x; tt < totalTiles; tt += 2 * step) {
      body(tt, st0);
      if (tt + step < totalTiles) body(tt + step, st1);
    }
  }
  // lane holds D[row = 4g + r][co = i] of each block: sum the four waves, then one partial per (tap, co) and workgroup
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) sred[wave][b][lane][r] = acc[b][r];
  __syncthreads();
  for (int q = tid; q < 2 * 64 * 4; q += 256) {
    const int r = q & 3, ln = (q >> 2) & 63, b = q >> 8;
    const float sum = sred[0][b][ln][r] + sred[1][b][ln][r] + sred[2][b][ln][r] + sred[3][b][ln][r];
    const int row = b * 16 + 4 * (ln >> 4) + r, co = ln & 15;
    const int Cout = 16 * gridDim.y;
    if (row < 27) dw[((size_t)blockIdx.x * 27 + row) * Cout + cb + co] = sum;
    else if (row == 27 && db) db[(size_t)blockIdx.x * Cout + cb + co] = sum;
  }
}

// shortcut of the first block (Conv3d 1 -> Cout, k = 1): dW[co] += sum_v img[v]*dy[v][co]; 16 channels per blockIdx.y
template <typename T>
__global__ void __launch_bounds__(256) rank1_wgrad_kernel(const float* __restrict__ img, const T* __restrict__ dy, int dy_ld, int64_t total,
                                                          float* __restrict__ dw) {
  constexpr int KPL = ElemTraits<T>::KPL;
  const int cb = blockIdx.y * 16;
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.f;
  // four voxels in flight per thread: with one, the 32 iterations of a thread were a chain of memory latencies (138 us for
  // 268 MB); the order of the additions into acc[] is unchanged
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; v + 3 * stride < total; v += 4 * stride) {
    float iv[4];
    u32x4_t raw[4][16 / KPL];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      iv[u] = img[v + u * stride];
#pragma unroll
      for (int q = 0; q < 16 / KPL; ++q) raw[u][q] = *reinterpret_cast<const u32x4_t*>(dy + (size_t)(v + u * stride) * dy_ld + cb + q * KPL);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float f[16];
#pragma unroll
      for (int q = 0; q < 16 / KPL; ++q) unpack16<T>(raw[u][q], f + q * KPL);
#pragma unroll
      for (int c = 0; c < 16; ++c) acc[c] = fmaf(iv[u], f[c], acc[c]);
    }
  }
  for (; v < total; v += stride) {
    float iv = img[v], f[16];
#pragma unroll
    for (int q = 0; q < 16 / KPL; ++q) unpack16<T>(*reinterpret_cast<const u32x4_t*>(dy + (size_t)v * dy_ld + cb + q * KPL), f + q * KPL);
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = fmaf(iv, f[c], acc[c]);
  }
  __shared__ float redr[4][16];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    float a = acc[c];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) a += __shfl_xor(a, m, 64);
    if ((threadIdx.x & 63) == 0) redr[threadIdx.x >> 6][c] = a;
  }
  __syncthreads();
  if (threadIdx.x < 16)   // partial row of this workgroup column: [gridDim.x][Cout]
    dw[(size_t)blockIdx.x * (16 * gridDim.y) + cb + threadIdx.x] = redr[0][threadIdx.x] + redr[1][threadIdx.x] + redr[2][threadIdx.x] + redr[3][threadIdx.x];
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

// ---- super-resolution "pre" up-sampling of the 1-channel input image (biapy/models/resunet.py:206-213, :368-369):
// ConvTranspose3d(1, 1, kernel = stride = (fz, fy, fx)), out[n, fz*z+a, fy*y+b, fx*x+c] = img[n,z,y,x] * w[a][b][c] + bias, written as
// channel 0 of a 16-channel NDHWC tensor of the storage dtype (channels 1..15 = 0): the first residual block then runs on the
// generic 16-channel kernels (its 1-input-channel weights zero-padded), which also yield the gradient of the up-sampled image.
template <typename T>
__global__ void __launch_bounds__(256) upsample_c1_fwd_kernel(const float* __restrict__ img, const float* __restrict__ w, const float* __restrict__ b,
                                                              T* __restrict__ out16, int D, int H, int W, int fz, int fy, int fx, int64_t total) {
  constexpr int KPL = ElemTraits<T>::KPL;
  const int Ho = H * fy, Wo = W * fx, Do = D * fz;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    int64_t r = v;
    const int xo = (int)(r % Wo); r /= Wo;
    const int yo = (int)(r % Ho); r /= Ho;
    const int zo = (int)(r % Do);
    const int64_t n = r / Do;
    const int z = zo / fz, a = zo - z * fz, y = yo / fy, bb = yo - y * fy, x = xo / fx, c = xo - x * fx;
    const float val = img[((n * D + z) * H + y) * (int64_t)W + x] * w[(a * fy + bb) * fx + c] + b[0];
    float f[8] = {val, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float zz[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<u32x4_t*>(out16 + v * 16) = pack16<T>(f);
#pragma unroll
    for (int q = 1; q < 16 / KPL; ++q) *reinterpret_cast<u32x4_t*>(out16 + v * 16 + q * KPL) = pack16<T>(zz);
  }
}

// gradients of the layer above: grid (blocks, taps): block (bx, t) sums img * g and g over its share of the INPUT voxels for tap
// t = (a*fy + b)*fx + c, g = channel 0 of dx16 at the tap's output voxel -> part[(t*gridDim.x + bx)*2 + {0,1}] (deterministic).
template <typename T>
__global__ void __launch_bounds__(256) upsample_c1_bwd_kernel(const float* __restrict__ img, const T* __restrict__ dx16, int D, int H, int W, int fz,
                                                              int fy, int fx, int64_t total_in, float* __restrict__ part) {
  const int t = blockIdx.y;
  const int c = t % fx, bb = (t / fx) % fy, a = t / (fx * fy);
  const int Ho = H * fy, Wo = W * fx, Do = D * fz;
  float sw = 0.f, sg = 0.f;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total_in; v += (int64_t)gridDim.x * 256) {
    int64_t r = v;
    const int x = (int)(r % W); r /= W;
    const int y = (int)(r % H); r /= H;
    const int z = (int)(r % D);
    const int64_t n = r / D;
    const int64_t vo = ((n * Do + (int64_t)z * fz + a) * Ho + (int64_t)y * fy + bb) * Wo + (int64_t)x * fx + c;
    const float g = ElemTraits<T>::ld(dx16 + vo * 16);
    sw += img[v] * g;
    sg += g;
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) { sw += __shfl_xor(sw, m, 64); sg += __shfl_xor(sg, m, 64); }
  __shared__ float red[4][2];
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = sw; red[threadIdx.x >> 6][1] = sg; }
  __syncthreads();
  if (threadIdx.x < 2) part[((size_t)t * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
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

extern "C" int bpx_head_fwd(int dtype, int64_t vps, int N, bpx_tensor x, const float* w_d, const float* b_d, int Cout, int head_act,
                            float* out_d, int64_t sn, int64_t sc, bpx_stream_t stream) {
  BPX_CHECK(x.cs == 0, "bpx_head_fwd: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_head_fwd";
  BPX_CHECK(x.ptr && w_d && out_d, "%s: null pointer", fn);
  BPX_CHECK(Cout >= 1 && Cout <= 8, "%s: Cout must be 1..8 (got %d)", fn, Cout);
  BPX_CHECK(x.C == 16 || x.C == 32, "%s: Cin must be 16 or 32 (got %d)", fn, x.C);
  int64_t total = (int64_t)N * vps;
  hipStream_t s = (hipStream_t)stream;
#define HL2(T, CIN, CO) head_fwd_kernel<T, CIN, CO><<<grid_for(total), 256, 0, s>>>((const T*)x.ptr, x.ld, w_d, b_d, head_act, out_d, sn, sc, vps, N)
#define HL(T, CIN)                                                                                                      \
  do {                                                                                                                  \
    switch (Cout) {                                                                                                     \
      case 1: HL2(T, CIN, 1); break; case 2: HL2(T, CIN, 2); break; case 3: HL2(T, CIN, 3); break; case 4: HL2(T, CIN, 4); break; \
      case 5: HL2(T, CIN, 5); break; case 6: HL2(T, CIN, 6); break; case 7: HL2(T, CIN, 7); break; default: HL2(T, CIN, 8); break; \
    }                                                                                                                   \
  } while (0)
  if (dtype == BPX_BF16) { if (x.C == 16) HL(uint16_t, 16); else HL(uint16_t, 32); }
  else if (dtype == BPX_F16) { if (x.C == 16) HL(f16_t, 16); else HL(f16_t, 32); }
  else if (dtype == BPX_F32) { if (x.C == 16) HL(float, 16); else HL(float, 32); }
  else BPX_FAIL("%s: dtype must be BF16, F16 or F32", fn);
#undef HL2
#undef HL
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

// scratch of the per-workgroup partials (the kernels launch at most 1024 workgroup columns; Cout 5..8: one row per column, its Cin / 16 slices
// write disjoint parts of it)
extern "C" int64_t bpx_head_bwd_workspace(int Cin, int Cout) { return (int64_t)1024 * ((int64_t)Cout * Cin + Cout) * 4; }
extern "C" int64_t bpx_conv3d_c1_wgrad_workspace(int Cout) { return (int64_t)1024 * 28 * Cout * 4; }
extern "C" int64_t bpx_conv1x1_c1_wgrad_workspace(int Cout) { return (int64_t)1024 * Cout * 4; }

extern "C" int bpx_head_bwd(int dtype, int64_t vps, int N, bpx_tensor x, const float* w_d, int Cout, const float* dout_d, int64_t sn,
                            int64_t sc, bpx_tensor dx, float* dw_d, float* db_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  BPX_CHECK(x.cs == 0 && dx.cs == 0, "bpx_head_bwd: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_head_bwd";
  BPX_CHECK(x.ptr && w_d && dout_d && dx.ptr && dw_d, "%s: null pointer", fn);
  BPX_CHECK(Cout >= 1 && Cout <= 8, "%s: Cout must be 1..8 (got %d)", fn, Cout);
  BPX_CHECK(x.C == 16 || x.C == 32, "%s: Cin must be 16 or 32 (got %d)", fn, x.C);
  BPX_CHECK(ws_d && ws_bytes >= bpx_head_bwd_workspace(x.C, Cout), "%s: workspace too small (%lld bytes)", fn, (long long)ws_bytes);
  int64_t total = (int64_t)N * vps;
  int blocks = (int)std::min<int64_t>(cdiv64(total, 256), 1024);
  if (Cout > 4 && x.C > 16) blocks = (blocks + 7) & ~7;   // the sliced kernel pairs columns 8 workgroups apart (<= 1024 still)
  hipStream_t s = (hipStream_t)stream;
  float* pw = reinterpret_cast<float*>(ws_d);
  float* pb = db_d ? pw + (size_t)blocks * Cout * x.C : nullptr;
#define HL2(T, CIN, CO, TX) head_bwd_kernel<T, CIN, CO, TX><<<blocks, 256, 0, s>>>((const TX*)x.ptr, x.ld, w_d, Cout, dout_d, sn, sc, (T*)dx.ptr, dx.ld, pw, pb, vps, N)
#define HS2(T, CO, TX) head_bwd_slice_kernel<T, CO, TX><<<blocks * (x.C / 16), 256, 0, s>>>((const TX*)x.ptr, x.ld, w_d, x.C, dout_d, sn, sc, (T*)dx.ptr, dx.ld, pw, pb, vps, N)
#define HL(T, CIN, TX)                                                                                                        \
  do {                                                                                                                        \
    switch (Cout) {                                                                                                           \
      case 1: HL2(T, CIN, 1, TX); break; case 2: HL2(T, CIN, 2, TX); break; case 3: HL2(T, CIN, 3, TX); break; case 4: HL2(T, CIN, 4, TX); break; \
      case 5: HS2(T, 5, TX); break; case 6: HS2(T, 6, TX); break; case 7: HS2(T, 7, TX); break; default: HS2(T, 8, TX); break;              \
    }                                                                                                                         \
  } while (0)
  if (dtype == BPX_BF16) { if (x.C == 16) HL(uint16_t, 16, uint16_t); else HL(uint16_t, 32, uint16_t); }
  else if (dtype == BPX_MIX16) { if (x.C == 16) HL(uint16_t, 16, f16_t); else HL(uint16_t, 32, f16_t); }   // x fp16, dx bf16
  else if (dtype == BPX_F32) { if (x.C == 16) HL(float, 16, float); else HL(float, 32, float); }
  else BPX_FAIL("%s: dtype must be BF16, F32 or MIX16", fn);
#undef HL2
#undef HS2
#undef HL
  BPX_LAUNCH_CHECK(fn);
  // dw[co][ci] flat = one "tap", one "input channel", Cout*Cin outputs; bias rows of Cout values
  return bpxred::reduce_partials(fn, pw, dw_d, blocks, 1, 1, Cout * x.C, 0, 1, 0, pb, db_d, Cout, false, s);
}

static int g_c1_persist = 2048;   // persistent workgroups of the first-layer forward (bpx_debug_set_c1_persist; 0 = one workgroup per tile, as until round 3)
static int g_c1_nobuf = 0;        // bit 30 of the hook's argument: the pointer-addressed instance (tests / A-B of the buffer-addressed one)
extern "C" int bpx_debug_set_c1_persist(int wgs) { g_c1_nobuf = (wgs >> 30) & 1; g_c1_persist = wgs & 0x3FFFFFFF; return 0; }
extern "C" int bpx_conv3d_c1_stats_tiles(int D, int H, int W) { return cdiv(D, 4) * cdiv(H, 8) * cdiv(W, 16); }

extern "C" int bpx_conv3d_c1_fwd(int dtype, int N, int D, int H, int W, const float* img_d, const float* w_d, const float* bias_d,
                                 bpx_tensor y, float* stats_part_d, bpx_stream_t stream) {
  BPX_CHECK(y.cs == 0, "bpx_conv3d_c1_fwd: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_conv3d_c1_fwd";
  BPX_CHECK(img_d && w_d && y.ptr, "%s: null pointer", fn);
  BPX_CHECK(y.C % 16 == 0, "%s: Cout must be a multiple of 16", fn);
  int tiles = bpx_conv3d_c1_stats_tiles(D, H, W);
  int tY = cdiv(H, 8), tX = cdiv(W, 16);
  const int total = tiles * N;
  dim3 grid((unsigned)std::min(total, g_c1_persist > 0 ? g_c1_persist : total), (unsigned)(y.C / 16));   // persistent: 8 workgroups per CU
  hipStream_t s = (hipStream_t)stream;
  BPX_CHECK(dtype == BPX_BF16 || dtype == BPX_F16 || dtype == BPX_F32, "%s: dtype must be BF16, F16 or F32", fn);
  // the buffer-addressed instance when image and output lie within 32-bit byte offsets of their bases (A/B and tests: bpx_debug_set_c1_persist bit 30 clears it)
  const int64_t vox = (int64_t)N * D * H * W;
  const int64_t ib = vox * 4, yb = vox * y.ld * (int64_t)dtype_size(dtype);
  const bool buf = !g_c1_nobuf && ib < 0xFFFFFF00ll && yb < 0xFFFFFF00ll;
#define C1F(T_, B_) conv_c1_fwd_kernel<T_, B_><<<grid, 256, 0, s>>>(img_d, w_d, bias_d, (T_*)y.ptr, y.ld, y.C, D, H, W, tY, tX, tiles, stats_part_d, total, (uint32_t)ib, (uint32_t)yb)
  if (dtype == BPX_BF16) { if (buf) C1F(uint16_t, true); else C1F(uint16_t, false); }
  else if (dtype == BPX_F16) { if (buf) C1F(f16_t, true); else C1F(f16_t, false); }
  else { if (buf) C1F(float, true); else C1F(float, false); }
#undef C1F
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

static int c1_wgrad_impl(const char* fn, int dtype, int N, int D, int H, int W, const float* img_d, bpx_tensor dy, bpx_tensor t,
                         const bpx_nbwd_coef* coef_d, float* dw_d, float* db_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  BPX_CHECK(dy.cs == 0, "%s: chunk-planar tensors (cs != 0) are not accepted here", fn);
  BPX_CHECK(img_d && dy.ptr && dw_d, "%s: null pointer", fn);
  BPX_CHECK(dy.C % 16 == 0, "%s: Cout must be a multiple of 16", fn);
  BPX_CHECK(ws_d && ws_bytes >= bpx_conv3d_c1_wgrad_workspace(dy.C), "%s: workspace too small (%lld bytes)", fn, (long long)ws_bytes);
  const bool nb = coef_d != nullptr, mix = dtype == BPX_MIX16;
  if (mix) dtype = BPX_BF16;
  int totalTiles = N * cdiv(D, 4) * cdiv(H, 8) * cdiv(W, 8);
  dim3 grid((unsigned)std::min(totalTiles, 1024), (unsigned)(dy.C / 16));
  hipStream_t s = (hipStream_t)stream;
  int groups = (int)grid.x;
  float* pw = reinterpret_cast<float*>(ws_d);
  const bool mfma_ok = dtype == BPX_BF16 && W > 8 && ((uintptr_t)dy.ptr & 15) == 0 && (dy.ld & 7) == 0;
  if (nb)
    BPX_CHECK(mfma_ok && t.ptr && t.cs == 0 && t.C == dy.C && ((uintptr_t)t.ptr & 15) == 0 && (t.ld & 7) == 0 && ((uintptr_t)coef_d & 15) == 0,
              "%s: needs bf16 gradients (BF16 / MIX16), W > 8 and 16-byte aligned dense g / t (bpx_conv3d_c1_wgrad_nb_supported)", fn);
  if (mfma_ok) {
    const int tiles = N * cdiv(D, 4) * cdiv(H, 4) * cdiv(W, 16);
    // 768 workgroups (3 per CU), each looping over its share of the tiles
    dim3 gm((unsigned)std::min(std::min(tiles, 768), g_c1_persist > 0 ? g_c1_persist : tiles), (unsigned)(dy.C / 16));   // (tests cap the workgroups through bpx_debug_set_c1_persist)
    groups = (int)gm.x;
    float* pb = db_d ? pw + (size_t)groups * 27 * dy.C : nullptr;
    // the buffer-addressed instances when the three operands lie within 32-bit byte offsets (bpx_debug_set_c1_persist bit 30 clears it: tests / A-B)
    const int64_t vox = (int64_t)N * D * H * W;
    const int64_t ib = vox * 4, gb = vox * dy.ld * 2, tb = nb ? vox * t.ld * 2 : 16;
    const bool buf = !g_c1_nobuf && ib < 0xFFFFFF00ll && gb < 0xFFFFFF00ll && tb < 0xFFFFFF00ll;
#define C1W(TT_, NB_, B_, tp_, tld_, cf_) conv_c1_wgrad_mfma_kernel<TT_, NB_, B_><<<gm, 256, 0, s>>>(img_d, (const uint16_t*)dy.ptr, dy.ld, D, H, W, N, tiles, pw, pb, tp_, tld_, cf_, (uint32_t)ib, (uint32_t)gb, (uint32_t)tb)
    if (nb && mix) { if (buf) C1W(f16_t, true, true, (const f16_t*)t.ptr, t.ld, coef_d); else C1W(f16_t, true, false, (const f16_t*)t.ptr, t.ld, coef_d); }
    else if (nb) { if (buf) C1W(uint16_t, true, true, (const uint16_t*)t.ptr, t.ld, coef_d); else C1W(uint16_t, true, false, (const uint16_t*)t.ptr, t.ld, coef_d); }
    else { if (buf) C1W(uint16_t, false, true, (const uint16_t*)nullptr, 0, (const bpx_nbwd_coef*)nullptr); else C1W(uint16_t, false, false, (const uint16_t*)nullptr, 0, (const bpx_nbwd_coef*)nullptr); }
#undef C1W
  } else {
    float* pb = db_d ? pw + (size_t)groups * 27 * dy.C : nullptr;
    if (dtype == BPX_BF16) conv_c1_wgrad_kernel<uint16_t><<<grid, 256, 0, s>>>(img_d, (const uint16_t*)dy.ptr, dy.ld, D, H, W, N, totalTiles, pw, pb);
    else if (dtype == BPX_F32) conv_c1_wgrad_kernel<float><<<grid, 256, 0, s>>>(img_d, (const float*)dy.ptr, dy.ld, D, H, W, N, totalTiles, pw, pb);
    else BPX_FAIL("%s: dtype must be BF16 or F32", fn);
  }
  BPX_LAUNCH_CHECK(fn);
  // partials [groups][27][1][Cout] -> dw (Cout,1,3,3,3): index = co*27 + tap
  return bpxred::reduce_partials(fn, pw, dw_d, groups, 27, 1, dy.C, 0, 27, 1, pw + (size_t)groups * 27 * dy.C, db_d, 0, true, s);
}

extern "C" int bpx_conv3d_c1_wgrad(int dtype, int N, int D, int H, int W, const float* img_d, bpx_tensor dy, float* dw_d, float* db_d,
                                   void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  BPX_CHECK(dtype == BPX_BF16 || dtype == BPX_F32, "bpx_conv3d_c1_wgrad: dtype must be BF16 or F32");
  return c1_wgrad_impl("bpx_conv3d_c1_wgrad", dtype, N, D, H, W, img_d, dy, bpx_tensor{nullptr, 0, 0}, nullptr, dw_d, db_d, ws_d, ws_bytes, stream);
}

// The same with dy = a * g + b * t + c0 formed inside the kernel (the InstanceNorm backward of the first layer's output: bpx_norm_bwd_apply folded
// into its only consumer - the first layer has no input gradient).  dtype BF16 (g, t bf16) or MIX16 (t fp16); W > 8.
extern "C" int bpx_conv3d_c1_wgrad_nb_supported(int dtype, int W) { return (dtype == BPX_BF16 || dtype == BPX_MIX16) && W > 8 ? 1 : 0; }
extern "C" int bpx_conv3d_c1_wgrad_nb(int dtype, int N, int D, int H, int W, const float* img_d, bpx_tensor g, bpx_tensor t, const bpx_nbwd_coef* coef_d,
                                      float* dw_d, float* db_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  const char* fn = "bpx_conv3d_c1_wgrad_nb";
  BPX_CHECK(dtype == BPX_BF16 || dtype == BPX_MIX16, "%s: dtype must be BF16 or MIX16", fn);
  BPX_CHECK(coef_d != nullptr, "%s: coefficients are null", fn);
  return c1_wgrad_impl(fn, dtype, N, D, H, W, img_d, g, t, coef_d, dw_d, db_d, ws_d, ws_bytes, stream);
}

extern "C" int bpx_conv1x1_c1_wgrad(int dtype, int64_t voxels_total, const float* img_d, bpx_tensor dy, float* dw_d, void* ws_d, int64_t ws_bytes,
                                    bpx_stream_t stream) {
  BPX_CHECK(dy.cs == 0, "bpx_conv1x1_c1_wgrad: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_conv1x1_c1_wgrad";
  BPX_CHECK(img_d && dy.ptr && dw_d, "%s: null pointer", fn);
  BPX_CHECK(dy.C % 16 == 0, "%s: Cout must be a multiple of 16", fn);
  BPX_CHECK(ws_d && ws_bytes >= bpx_conv1x1_c1_wgrad_workspace(dy.C), "%s: workspace too small (%lld bytes)", fn, (long long)ws_bytes);
  dim3 grid((unsigned)std::min<int64_t>(cdiv64(voxels_total, 256), 1024), (unsigned)(dy.C / 16));
  hipStream_t s = (hipStream_t)stream;
  float* pw = reinterpret_cast<float*>(ws_d);
  if (dtype == BPX_BF16) rank1_wgrad_kernel<uint16_t><<<grid, 256, 0, s>>>(img_d, (const uint16_t*)dy.ptr, dy.ld, voxels_total, pw);
  else if (dtype == BPX_F32) rank1_wgrad_kernel<float><<<grid, 256, 0, s>>>(img_d, (const float*)dy.ptr, dy.ld, voxels_total, pw);
  else BPX_FAIL("%s: dtype must be BF16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return bpxred::reduce_partials(fn, pw, dw_d, (int)grid.x, 1, 1, dy.C, 0, 1, 0, nullptr, nullptr, 0, true, s);
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

extern "C" int bpx_upsample_c1_fwd(int dtype, int N, int D, int H, int W, int fz, int fy, int fx, const float* img_d, const float* w_d, const float* bias_d,
                                   void* out16_d, bpx_stream_t stream) {
  const char* fn = "bpx_upsample_c1_fwd";
  BPX_CHECK(img_d && w_d && bias_d && out16_d, "%s: null pointer", fn);
  BPX_CHECK(fz >= 1 && fy >= 1 && fx >= 1 && fz * fy * fx <= 512, "%s: bad factors (%d,%d,%d)", fn, fz, fy, fx);
  const int64_t total = (int64_t)N * D * fz * H * fy * W * fx;
  if (total == 0) return 0;
  if (dtype == BPX_BF16) upsample_c1_fwd_kernel<uint16_t><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(img_d, w_d, bias_d, (uint16_t*)out16_d, D, H, W, fz, fy, fx, total);
  else if (dtype == BPX_F16) upsample_c1_fwd_kernel<f16_t><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(img_d, w_d, bias_d, (f16_t*)out16_d, D, H, W, fz, fy, fx, total);
  else if (dtype == BPX_F32) upsample_c1_fwd_kernel<float><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(img_d, w_d, bias_d, (float*)out16_d, D, H, W, fz, fy, fx, total);
  else BPX_FAIL("%s: dtype must be BF16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_upsample_c1_blocks(int64_t voxels_in) { return (int)std::min<int64_t>(std::max<int64_t>(1, cdiv64(voxels_in, 2048)), 256); }

extern "C" int bpx_upsample_c1_bwd(int dtype, int N, int D, int H, int W, int fz, int fy, int fx, const float* img_d, const void* dx16_d, float* partials_d,
                                   bpx_stream_t stream) {
  const char* fn = "bpx_upsample_c1_bwd";
  BPX_CHECK(img_d && dx16_d && partials_d, "%s: null pointer", fn);
  BPX_CHECK(fz >= 1 && fy >= 1 && fx >= 1 && fz * fy * fx <= 512, "%s: bad factors (%d,%d,%d)", fn, fz, fy, fx);
  const int64_t total_in = (int64_t)N * D * H * W;
  if (total_in == 0) return 0;
  dim3 grid((unsigned)bpx_upsample_c1_blocks(total_in), (unsigned)(fz * fy * fx));
  if (dtype == BPX_BF16) upsample_c1_bwd_kernel<uint16_t><<<grid, 256, 0, (hipStream_t)stream>>>(img_d, (const uint16_t*)dx16_d, D, H, W, fz, fy, fx, total_in, partials_d);
  else if (dtype == BPX_F32) upsample_c1_bwd_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>(img_d, (const float*)dx16_d, D, H, W, fz, fy, fx, total_in, partials_d);
  else BPX_FAIL("%s: dtype must be BF16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

