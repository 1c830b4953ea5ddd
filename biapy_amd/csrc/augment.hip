// Training-time augmentation on the device (biapy_amd/augment.py states the semantics, include/biapy_amd.h the record layout): flips, rot90 over
// (Y, X), contrast, brightness, Gaussian noise and cutout of a float32 (B,Z,Y,X,C) batch and its float32 / uint8 target in ONE gather pass.
// The affine warp (rotation, zoom, shear, shift: step 0, a pass of its own in front of that one) is the last section of the file; the elastic
// deformation (step 0b) is elastic.hip, which shares augment_core.h with the warp.
//
// Random numbers: Philox4x32-10 (philox.h), key = the augmenter's 64-bit seed, counter words = (sample, stream, counter low, counter high) with the
// augmenter's own device counter, one value per call.  Streams of the draw kernel, r = the four output words:
//   0      fires: r0 rot90, r1 zflip, r2 vflip, r3 hflip                  ("fires": (uint64) r < floor(da_prob * 2^32))
//   1      r0 >> 30 = k of rot90; fires: r1 contrast, r2 brightness, r3 noise
//   2      uniforms: r0 contrast c (a = 1 + c), r1 brightness b, r2 noise s; r3: cutout fires
//   3      r0: number of boxes = box_lo + ((uint64) r0 * (box_hi - box_lo + 1) >> 32)
//   4 + i  box i, extents: r0, r1, r2 = fractions of Z, Y, X (uniform in the size range), extent = clamp(floor(f * dim), 1, dim)
//   8 + i  box i, origin:  z0 = (uint64) r0 * (Z - dz + 1) >> 32, y0 from r1, x0 from r2
// A uniform is min(lo + u * (hi - lo), hi) in fp32 with u = (r >> 8) * 2^-24.
// The noise of the apply kernel uses the key (seed low ^ 0x4E4F4953, seed high) - no draw stream shares it - and the counter words
// (q low, q high ^ (sample << 8), counter low, counter high), q = element / 4, element = linear (z,y,x,c) index of the OUTPUT within its sample
// (below 2^42, fewer than 2^24 samples): a function of (seed, counter value, sample, element) only.  One Philox call serves the four
// consecutive elements 4q .. 4q+3 as two Box-Muller pairs (noise4).
#include "bpx_common.h"
#include "philox.h"
#include "augment_core.h"   // aug_uniform, warp_clamp, warp_tap, warp_lerp: shared with elastic.hip

namespace {

constexpr int REC = BPX_AUG_REC_WORDS;

__device__ __forceinline__ int aug_extent(uint32_t r, float lo, float hi, int dim) {
  const int e = (int)floorf(__fmul_rn(aug_uniform(r, lo, hi), (float)dim));
  return min(max(e, 1), dim);
}
__device__ __forceinline__ int aug_below(uint32_t r, int n) { return (int)(((uint64_t)r * (uint64_t)n) >> 32); }   // uniform in [0, n)

__global__ void __launch_bounds__(256) aug_draw_kernel(const bpx_aug_cfg cfg, int B, int Z, int Y, int X, uint64_t* __restrict__ state,
                                                       uint32_t* __restrict__ rec) {
  const uint64_t ctr = state[0];
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) {
    const uint32_t k0 = (uint32_t)cfg.seed, k1 = (uint32_t)(cfg.seed >> 32), cl = (uint32_t)ctr, ch = (uint32_t)(ctr >> 32);
    uint32_t w[REC];
#pragma unroll
    for (int i = 0; i < REC; ++i) w[i] = 0;
    uint32_t r[4], q[4];
    uint32_t flags = 0;
    auto fires = [&](uint32_t v, uint32_t en) { return (cfg.enable & en) && (uint64_t)v < cfg.thr; };
    philox4x32_10((uint32_t)b, 0u, cl, ch, k0, k1, r);
    philox4x32_10((uint32_t)b, 1u, cl, ch, k0, k1, q);
    if (fires(r[0], BPX_AUG_EN_ROT90)) flags |= (q[0] >> 30) << BPX_AUG_K_SHIFT;
    if (Z > 1 && fires(r[1], BPX_AUG_EN_ZFLIP)) flags |= BPX_AUG_F_ZFLIP;
    if (fires(r[2], BPX_AUG_EN_VFLIP)) flags |= BPX_AUG_F_VFLIP;
    if (fires(r[3], BPX_AUG_EN_HFLIP)) flags |= BPX_AUG_F_HFLIP;
    if (fires(q[1], BPX_AUG_EN_CONTRAST)) flags |= BPX_AUG_F_CONTRAST;
    if (fires(q[2], BPX_AUG_EN_BRIGHTNESS)) flags |= BPX_AUG_F_BRIGHTNESS;
    if (fires(q[3], BPX_AUG_EN_NOISE)) flags |= BPX_AUG_F_NOISE;
    philox4x32_10((uint32_t)b, 2u, cl, ch, k0, k1, r);
    if (cfg.enable & BPX_AUG_EN_CONTRAST) w[BPX_AUG_W_A] = __float_as_uint(__fadd_rn(1.f, aug_uniform(r[0], cfg.c_lo, cfg.c_hi)));
    if (cfg.enable & BPX_AUG_EN_BRIGHTNESS) w[BPX_AUG_W_B] = __float_as_uint(aug_uniform(r[1], cfg.b_lo, cfg.b_hi));
    if (cfg.enable & BPX_AUG_EN_NOISE) w[BPX_AUG_W_S] = __float_as_uint(aug_uniform(r[2], cfg.s_lo, cfg.s_hi));
    if (fires(r[3], BPX_AUG_EN_CUTOUT)) {
      philox4x32_10((uint32_t)b, 3u, cl, ch, k0, k1, q);
      const int nb = cfg.box_lo + aug_below(q[0], cfg.box_hi - cfg.box_lo + 1);
      flags |= (uint32_t)nb << BPX_AUG_NBOX_SHIFT;
#pragma unroll
      for (int i = 0; i < BPX_AUG_MAX_BOXES; ++i) {
        if (i < nb) {
          philox4x32_10((uint32_t)b, 4u + i, cl, ch, k0, k1, r);
          philox4x32_10((uint32_t)b, 8u + i, cl, ch, k0, k1, q);
          const int dz = aug_extent(r[0], cfg.f_lo, cfg.f_hi, Z), dy = aug_extent(r[1], cfg.f_lo, cfg.f_hi, Y), dx = aug_extent(r[2], cfg.f_lo, cfg.f_hi, X);
          uint32_t* bx = w + BPX_AUG_W_BOX + 6 * i;
          bx[0] = (uint32_t)aug_below(q[0], Z - dz + 1); bx[1] = (uint32_t)aug_below(q[1], Y - dy + 1); bx[2] = (uint32_t)aug_below(q[2], X - dx + 1);
          bx[3] = (uint32_t)dz; bx[4] = (uint32_t)dy; bx[5] = (uint32_t)dx;
        }
      }
    }
    w[BPX_AUG_W_FLAGS] = flags;
    w[BPX_AUG_W_CTR] = cl; w[BPX_AUG_W_CTR + 1] = ch;
    u32x4_t* dst = reinterpret_cast<u32x4_t*>(rec + (size_t)b * REC);
#pragma unroll
    for (int i = 0; i < REC / 4; ++i) dst[i] = u32x4_t{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
  }
  // the counter advances once, after every block has read it: the blocks count themselves on state[1], the last one to arrive bumps state[0]
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    const unsigned long long t = atomicAdd(reinterpret_cast<unsigned long long*>(state + 1), 1ull);
    if (t == (unsigned long long)gridDim.x - 1) {
      state[1] = 0;
      state[0] = ctr + 1;
    }
  }
}

// ---- per-sample mean: fp64 partials per block, then one block per sample adds them in a fixed order ---------------------------------------
constexpr int MEAN_MAX_BLOCKS = 256;

__global__ void __launch_bounds__(256) aug_mean_partial_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ part) {
  const float* xs = x + (size_t)blockIdx.y * n;
  double s = 0.0;
  const int64_t n4 = (((uintptr_t)xs & 15) == 0) ? n / 4 : 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const f32x4_t v = reinterpret_cast<const f32x4_t*>(xs)[i];
    s += ((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3]);
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) s += (double)xs[i];
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
  __shared__ double r[4];
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
}

__global__ void __launch_bounds__(MEAN_MAX_BLOCKS) aug_mean_final_kernel(const double* __restrict__ part, int blocks, int64_t n, uint32_t* __restrict__ rec) {
  __shared__ double sh[MEAN_MAX_BLOCKS];
  sh[threadIdx.x] = (int)threadIdx.x < blocks ? part[(size_t)blockIdx.x * blocks + threadIdx.x] : 0.0;
  __syncthreads();
  for (int m = MEAN_MAX_BLOCKS / 2; m > 0; m >>= 1) {
    if ((int)threadIdx.x < m) sh[threadIdx.x] += sh[threadIdx.x + m];
    __syncthreads();
  }
  if (threadIdx.x == 0) rec[(size_t)blockIdx.x * REC + BPX_AUG_W_M] = __float_as_uint((float)(sh[0] / (double)n));
}

int mean_blocks(int64_t n) { return (int)std::min<int64_t>(MEAN_MAX_BLOCKS, std::max<int64_t>(1, cdiv64(n, 256 * 16))); }

// ---- the gather pass ---------------------------------------------------------------------------------------------------------------------
// One workgroup = one (sample, z, T x T tile of (Y, X)) of the OUTPUT, never two samples: the orientation is uniform over the workgroup.  The tile's
// source rectangle (a T x T tile of the source plane, its rows along the source's X whatever k is) is read row by row - full lines - into LDS with
// a row pitch == C (mod 32) words, image and target side by side, and after ONE barrier the output rows are formed from LDS: for an odd k consecutive
// lanes walk a source COLUMN, which the pitch spreads over consecutive banks (ds_read_b32: 32 banks per 32-lane half).  Where X * C is a multiple
// of 4 (and the pointers are aligned) every lane moves 16 bytes of the image / of a float32 target, or 4 bytes of a uint8 target, per access.
struct AugGeom { int Z, Y, X, T, tiles_x, tiles_y; };

struct TileMap {
  int k, vf, hf, Y, X;
  // source (ys, xs) of output (yo, xo):  v = rot90(src, k) over (Y, X), then the flips
  __device__ __forceinline__ void src(int yo, int xo, int& ys, int& xs) const {
    const int yv = vf ? Y - 1 - yo : yo, xv = hf ? X - 1 - xo : xo;
    switch (k) {
      case 0: ys = yv; xs = xv; break;
      case 1: ys = xv; xs = X - 1 - yv; break;
      case 2: ys = Y - 1 - yv; xs = X - 1 - xv; break;
      default: ys = Y - 1 - xv; xs = yv; break;
    }
  }
};

// LDS word of channel 0 of output voxel (row r, column xl) of the tile: a0 + r * dy + xl * dx (the map is affine)
struct LdsMap { int a0, dy, dx; };
__device__ __forceinline__ LdsMap lds_map(const TileMap& tm, int yo0, int xo0, int ys0, int xs0, int pitch, int C) {
  int ya, xa, yb, xb, yc, xc;
  tm.src(yo0, xo0, ya, xa);
  tm.src(yo0 + 1, xo0, yb, xb);          // differences only: the neighbours may lie outside the plane
  tm.src(yo0, xo0 + 1, yc, xc);
  LdsMap m;
  m.a0 = (ya - ys0) * pitch + (xa - xs0) * C;
  m.dy = (yb - ya) * pitch + (xb - xa) * C;
  m.dx = (yc - ya) * pitch + (xc - xa) * C;
  return m;
}

// V consecutive elements of a row <-> 32-bit words (a uint8 target is held one value per word)
template <typename T, int V> struct Vec;
template <> struct Vec<float, 1> {
  static __device__ __forceinline__ void ld(const float* p, uint32_t* w) { w[0] = __float_as_uint(*p); }
  static __device__ __forceinline__ void st(float* p, const uint32_t* w) { *p = __uint_as_float(w[0]); }
};
template <> struct Vec<float, 4> {
  static __device__ __forceinline__ void ld(const float* p, uint32_t* w) {
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(p);
    w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
  }
  static __device__ __forceinline__ void st(float* p, const uint32_t* w) { *reinterpret_cast<u32x4_t*>(p) = u32x4_t{w[0], w[1], w[2], w[3]}; }
};
template <> struct Vec<uint8_t, 1> {
  static __device__ __forceinline__ void ld(const uint8_t* p, uint32_t* w) { w[0] = *p; }
  static __device__ __forceinline__ void st(uint8_t* p, const uint32_t* w) { *p = (uint8_t)w[0]; }
};
template <> struct Vec<uint8_t, 4> {
  static __device__ __forceinline__ void ld(const uint8_t* p, uint32_t* w) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
    w[0] = v & 255u; w[1] = (v >> 8) & 255u; w[2] = (v >> 16) & 255u; w[3] = v >> 24;
  }
  static __device__ __forceinline__ void st(uint8_t* p, const uint32_t* w) {
    *reinterpret_cast<uint32_t*>(p) = (w[0] & 255u) | ((w[1] & 255u) << 8) | ((w[2] & 255u) << 16) | (w[3] << 24);
  }
};

// rows of the source rectangle -> LDS (row r at r * pitch): the workgroup's threads walk the rectangle's V-element items row after row, so a
// wave covers several short rows at once and every lane is busy
template <typename T, int V>
__device__ __forceinline__ void tile_load(const T* __restrict__ plane, int X, int C, int ys0, int xs0, int nys, int nxs, int pitch, uint32_t* lds) {
  const int ipr = nxs * C / V, items = nys * ipr;               // V == 4: the row holds a multiple of 4 elements
  const float rcp = 1.f / (float)ipr;
  for (int i = threadIdx.x; i < items; i += 256) {
    const int r = small_div(i, rcp), c = (i - r * ipr) * V;
    uint32_t w[V];
    Vec<T, V>::ld(plane + ((int64_t)(ys0 + r) * X + xs0) * C + c, w);
#pragma unroll
    for (int j = 0; j < V; ++j) lds[r * pitch + c + j] = w[j];
  }
}

struct BoxSet { int n; int z0[BPX_AUG_MAX_BOXES], y0[BPX_AUG_MAX_BOXES], x0[BPX_AUG_MAX_BOXES], z1[BPX_AUG_MAX_BOXES], y1[BPX_AUG_MAX_BOXES], x1[BPX_AUG_MAX_BOXES]; };
__device__ __forceinline__ bool in_boxes(const BoxSet& bs, int z, int y, int x) {
  bool in = false;
#pragma unroll
  for (int i = 0; i < BPX_AUG_MAX_BOXES; ++i)
    if (i < bs.n) in |= z >= bs.z0[i] && z < bs.z1[i] && y >= bs.y0[i] && y < bs.y1[i] && x >= bs.x0[i] && x < bs.x1[i];
  return in;
}

// N(0,1) of the output elements 4q .. 4q+3 of a sample: one Philox block, two Box-Muller pairs (cosine for the even element, sine for the odd one)
__device__ __forceinline__ void noise4(uint64_t seed, uint32_t cl, uint32_t ch, uint32_t sample, uint64_t q, float (&n)[4]) {
  uint32_t r[4];
  philox4x32_10((uint32_t)q, (uint32_t)(q >> 32) ^ (sample << 8), cl, ch, (uint32_t)seed ^ 0x4E4F4953u, (uint32_t)(seed >> 32), r);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = (float)((r[2 * p] >> 8) + 1u) * 5.9604644775390625e-8f;     // (0, 1]: no logarithm of zero
    const float u2 = (float)(r[2 * p + 1] >> 8) * 5.9604644775390625e-8f;        // [0, 1)
    const float rad = sqrtf(-2.f * logf(u1)), ang = 6.283185307179586f * u2;
    n[2 * p] = rad * cosf(ang);
    n[2 * p + 1] = rad * sinf(ang);
  }
}

template <typename TT, int VX, int VT>
__global__ void __launch_bounds__(256) aug_apply_kernel(const float* __restrict__ x, const TT* __restrict__ t, AugGeom g, int C, int Ct, int pitch_x,
                                                        int pitch_t, const uint32_t* __restrict__ rec, uint64_t seed, float cval, int mask_too,
                                                        float* __restrict__ xo, TT* __restrict__ to) {
  extern __shared__ uint32_t lds[];
  uint32_t* lds_x = lds;
  uint32_t* lds_t = lds + g.T * pitch_x;
  const int tiles = g.tiles_x * g.tiles_y;
  const int64_t per_sample = (int64_t)g.Z * tiles;
  const int b = (int)((int64_t)blockIdx.x / per_sample);
  const int rest = (int)((int64_t)blockIdx.x - (int64_t)b * per_sample);
  const int zo = rest / tiles, tile = rest % tiles;
  const int yo0 = (tile / g.tiles_x) * g.T, xo0 = (tile % g.tiles_x) * g.T;
  const int nyo = min(g.T, g.Y - yo0), nxo = min(g.T, g.X - xo0);

  const uint32_t* rc = rec + (size_t)b * REC;
  const uint32_t flags = rc[BPX_AUG_W_FLAGS];
  TileMap tm;
  tm.k = (int)((flags >> BPX_AUG_K_SHIFT) & 3u);
  if (g.Y != g.X) tm.k &= 2;                                   // an odd k needs a square plane
  tm.vf = (flags & BPX_AUG_F_VFLIP) != 0; tm.hf = (flags & BPX_AUG_F_HFLIP) != 0; tm.Y = g.Y; tm.X = g.X;
  const int zs = (flags & BPX_AUG_F_ZFLIP) ? g.Z - 1 - zo : zo;
  int ysa, xsa, ysb, xsb;
  tm.src(yo0, xo0, ysa, xsa);
  tm.src(yo0 + nyo - 1, xo0 + nxo - 1, ysb, xsb);
  const int ys0 = min(ysa, ysb), xs0 = min(xsa, xsb), nys = abs(ysa - ysb) + 1, nxs = abs(xsa - xsb) + 1;   // <= T each

  const int64_t plane_vox = (int64_t)g.Y * g.X;
  const int64_t src_plane = ((int64_t)b * g.Z + zs) * plane_vox, dst_plane = ((int64_t)b * g.Z + zo) * plane_vox;
  tile_load<float, VX>(x + src_plane * C, g.X, C, ys0, xs0, nys, nxs, pitch_x, lds_x);
  tile_load<TT, VT>(t + src_plane * Ct, g.X, Ct, ys0, xs0, nys, nxs, pitch_t, lds_t);

  const bool contrast = flags & BPX_AUG_F_CONTRAST, bright = flags & BPX_AUG_F_BRIGHTNESS, noise = flags & BPX_AUG_F_NOISE;
  const float a = __uint_as_float(rc[BPX_AUG_W_A]), bb = __uint_as_float(rc[BPX_AUG_W_B]), s = __uint_as_float(rc[BPX_AUG_W_S]);
  const float m = __uint_as_float(rc[BPX_AUG_W_M]);
  const uint32_t cl = rc[BPX_AUG_W_CTR], ch = rc[BPX_AUG_W_CTR + 1];
  // the boxes that meet this tile (uniform over the workgroup)
  BoxSet bs;
  bs.n = 0;
  const int nb = min((int)((flags >> BPX_AUG_NBOX_SHIFT) & 7u), BPX_AUG_MAX_BOXES);
#pragma unroll
  for (int i = 0; i < BPX_AUG_MAX_BOXES; ++i) {
    bs.z0[i] = bs.y0[i] = bs.x0[i] = bs.z1[i] = bs.y1[i] = bs.x1[i] = 0;
  }
#pragma unroll
  for (int i = 0; i < BPX_AUG_MAX_BOXES; ++i) {
    if (i < nb) {
      const int* bx = reinterpret_cast<const int*>(rc + BPX_AUG_W_BOX + 6 * i);
      const int z0 = bx[0], y0 = bx[1], x0 = bx[2];
      const int z1 = z0 + max(bx[3], 0), y1 = y0 + max(bx[4], 0), x1 = x0 + max(bx[5], 0);
      if (zo >= z0 && zo < z1 && y0 < yo0 + nyo && y1 > yo0 && x0 < xo0 + nxo && x1 > xo0) {
        const int j = bs.n++;
        bs.z0[j] = z0; bs.y0[j] = y0; bs.x0[j] = x0; bs.z1[j] = z1; bs.y1[j] = y1; bs.x1[j] = x1;
      }
    }
  }
  const LdsMap mx = lds_map(tm, yo0, xo0, ys0, xs0, pitch_x, C), mt = lds_map(tm, yo0, xo0, ys0, xs0, pitch_t, Ct);
  const float rcp_c = 1.f / (float)C, rcp_ct = 1.f / (float)Ct;
  __syncthreads();

  // ---- image ----
  {
    const int ipr = nxo * C / VX, items = nyo * ipr;
    const float rcp = 1.f / (float)ipr;
    for (int i = threadIdx.x; i < items; i += 256) {
      const int r = small_div(i, rcp), e = (i - r * ipr) * VX;
      const int yo = yo0 + r, base = mx.a0 + r * mx.dy;
      const int64_t row_vox = dst_plane + (int64_t)yo * g.X + xo0;
      float* row = xo + row_vox * C;
      {
        uint32_t w[VX];
        float nz[4];
        if (noise) {                                             // element index within the sample; a vector never straddles a Philox block
          const uint64_t el = (uint64_t)(row_vox - (int64_t)b * g.Z * plane_vox) * C + e;
          noise4(seed, cl, ch, (uint32_t)b, el >> 2, nz);
          if (VX == 1) nz[0] = nz[el & 3];
        }
#pragma unroll
        for (int j = 0; j < VX; ++j) {
          const int ee = e + j;
          const int xl = C == 1 ? ee : small_div(ee, rcp_c);
          const int c = ee - xl * C;
          float v = __uint_as_float(lds_x[base + xl * mx.dx + c]);
          if (contrast) v = __fadd_rn(__fmul_rn(__fsub_rn(v, m), a), m);
          if (bright) v = __fadd_rn(v, bb);
          if (noise) v = __fadd_rn(v, __fmul_rn(s, nz[j]));
          if (bs.n && in_boxes(bs, zo, yo, xo0 + xl)) v = cval;
          w[j] = __float_as_uint(v);
        }
        Vec<float, VX>::st(row + e, w);
      }
    }
  }
  // ---- target ----
  {
    const int ipr = nxo * Ct / VT, items = nyo * ipr;
    const float rcp = 1.f / (float)ipr;
    const bool cut = mask_too && bs.n;
    for (int i = threadIdx.x; i < items; i += 256) {
      const int r = small_div(i, rcp), e = (i - r * ipr) * VT;
      const int yo = yo0 + r, base = mt.a0 + r * mt.dy;
      TT* row = to + (dst_plane + (int64_t)yo * g.X + xo0) * Ct;
      {
        uint32_t w[VT];
#pragma unroll
        for (int j = 0; j < VT; ++j) {
          const int ee = e + j;
          const int xl = Ct == 1 ? ee : small_div(ee, rcp_ct);
          const int c = ee - xl * Ct;
          w[j] = lds_t[base + xl * mt.dx + c];
          if (cut && in_boxes(bs, zo, yo, xo0 + xl)) w[j] = 0;
        }
        Vec<TT, VT>::st(row + e, w);
      }
    }
  }
}

int tile_pitch(int T, int C) { return T * C + C + (32 - (T * C) % 32) % 32; }   // == C (mod 32)
// the largest tile edge whose image and target tiles fit 64 KB of LDS together
int tile_edge(int C, int Ct) {
  for (int T = 64; T > 16; T >>= 1)
    if ((size_t)T * (tile_pitch(T, C) + tile_pitch(T, Ct)) * 4 <= 65536) return T;
  return 16;
}

template <typename TT>
void launch_apply(int vx, int vt, unsigned blocks, size_t lds, hipStream_t s, const float* x, const TT* t, AugGeom g, int C, int Ct, int pitch_x, int pitch_t,
                  const uint32_t* rec, uint64_t seed, float cval, int mask_too, float* xo, TT* to) {
  if (vx && vt) aug_apply_kernel<TT, 4, 4><<<blocks, 256, lds, s>>>(x, t, g, C, Ct, pitch_x, pitch_t, rec, seed, cval, mask_too, xo, to);
  else if (vx) aug_apply_kernel<TT, 4, 1><<<blocks, 256, lds, s>>>(x, t, g, C, Ct, pitch_x, pitch_t, rec, seed, cval, mask_too, xo, to);
  else if (vt) aug_apply_kernel<TT, 1, 4><<<blocks, 256, lds, s>>>(x, t, g, C, Ct, pitch_x, pitch_t, rec, seed, cval, mask_too, xo, to);
  else aug_apply_kernel<TT, 1, 1><<<blocks, 256, lds, s>>>(x, t, g, C, Ct, pitch_x, pitch_t, rec, seed, cval, mask_too, xo, to);
}

// ---- the affine warp (step 0): one 2x3 matrix per sample, bilinear image, nearest target ---------------------------------------------------
// Streams 16-18 of the draw key and counter words (the call's counter value is read back out of the sample's augmentation record):
//   16     fires: r0 rotation, r1 zoom, r2 shear, r3 shift
//   17     uniforms: r0 theta (degrees), r1 zoom, r2 phi (degrees)
//   18     uniforms: r0 ty, r1 tx (fractions of Y and X)
constexpr int WREC = BPX_WARP_REC_WORDS;

__global__ void __launch_bounds__(256) warp_draw_kernel(const bpx_warp_cfg cfg, int B, int Y, int X, const uint32_t* __restrict__ rec,
                                                        uint32_t* __restrict__ warp) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint32_t k0 = (uint32_t)cfg.seed, k1 = (uint32_t)(cfg.seed >> 32);
  const uint32_t cl = rec[(size_t)b * REC + BPX_AUG_W_CTR], ch = rec[(size_t)b * REC + BPX_AUG_W_CTR + 1];
  uint32_t f[4], u[4], v[4];
  philox4x32_10((uint32_t)b, 16u, cl, ch, k0, k1, f);
  philox4x32_10((uint32_t)b, 17u, cl, ch, k0, k1, u);
  philox4x32_10((uint32_t)b, 18u, cl, ch, k0, k1, v);
  auto fires = [&](uint32_t r, uint32_t en) { return (cfg.enable & en) && (uint64_t)r < cfg.thr; };
  uint32_t flags = 0;
  float th = 0.f, zm = 1.f, ph = 0.f, ty = 0.f, tx = 0.f;
  if (fires(f[0], BPX_WARP_F_ROT)) { flags |= BPX_WARP_F_ROT; th = aug_uniform(u[0], cfg.rot_lo, cfg.rot_hi); }
  if (fires(f[1], BPX_WARP_F_ZOOM)) { flags |= BPX_WARP_F_ZOOM; zm = aug_uniform(u[1], cfg.zoom_lo, cfg.zoom_hi); }
  if (fires(f[2], BPX_WARP_F_SHEAR)) { flags |= BPX_WARP_F_SHEAR; ph = aug_uniform(u[2], cfg.shear_lo, cfg.shear_hi); }
  if (fires(f[3], BPX_WARP_F_SHIFT)) {
    flags |= BPX_WARP_F_SHIFT;
    ty = aug_uniform(v[0], cfg.shift_lo, cfg.shift_hi);
    tx = aug_uniform(v[1], cfg.shift_lo, cfg.shift_hi);
  }
  // A = (1/z) [[c, s], [-s, c]] [[1, 0], [t, 1]] = (1/z) [[c + s t, s], [c t - s, c]]
  const float d2r = 0.017453292519943295f;
  const float ra = __fmul_rn(th, d2r), rp = __fmul_rn(ph, d2r);
  const float c = cosf(ra), s = sinf(ra), t = tanf(rp), iz = __fdiv_rn(1.f, zm);
  const float cy = (float)(Y - 1) * 0.5f, cx = (float)(X - 1) * 0.5f;
  const float m00 = __fmul_rn(iz, __fadd_rn(c, __fmul_rn(s, t))), m01 = __fmul_rn(iz, s);
  const float m10 = __fmul_rn(iz, __fsub_rn(__fmul_rn(c, t), s)), m11 = __fmul_rn(iz, c);
  const float m02 = __fsub_rn(cy, __fmul_rn(ty, (float)Y)), m12 = __fsub_rn(cx, __fmul_rn(tx, (float)X));
  u32x4_t* dst = reinterpret_cast<u32x4_t*>(warp + (size_t)b * WREC);
  dst[0] = u32x4_t{flags, __float_as_uint(m00), __float_as_uint(m01), __float_as_uint(m02)};
  dst[1] = u32x4_t{__float_as_uint(m10), __float_as_uint(m11), __float_as_uint(m12), 0u};
  dst[2] = u32x4_t{__float_as_uint(th), __float_as_uint(zm), __float_as_uint(ph), __float_as_uint(ty)};
  dst[3] = u32x4_t{__float_as_uint(tx), 0u, 0u, 0u};
}

// One workgroup = one (sample, z, WT x WT tile of (Y, X)) of the OUTPUT, never two samples: flags and matrix are uniform over it.  Its source
// footprint is a parallelogram of one z plane, read with plain loads - consecutive lanes walk consecutive output elements of a row, so their
// taps step by one matrix column through the source and the four taps of neighbouring lanes share cache lines.
constexpr int WT = 32;
struct WarpGeom { int Z, Y, X, tiles_x, tiles_y; };

// warp_tap<MODE>, the border rule of an integer tap index, warp_clamp and warp_lerp: augment_core.h
struct WarpMap {
  float m00, m01, m02, m10, m11, m12, cy, cx;
  __device__ __forceinline__ void src(int y, int x, float& fy, float& fx) const {
    const float dy = __fsub_rn((float)y, cy), dx = __fsub_rn((float)x, cx);
    fy = __fadd_rn(__fadd_rn(__fmul_rn(m00, dy), __fmul_rn(m01, dx)), m02);
    fx = __fadd_rn(__fadd_rn(__fmul_rn(m10, dy), __fmul_rn(m11, dx)), m12);
    fy = warp_clamp(fy);
    fx = warp_clamp(fx);
  }
};

template <typename TT, int MODE>
__global__ void __launch_bounds__(256) warp_apply_kernel(const float* __restrict__ x, const TT* __restrict__ t, WarpGeom g, int C, int Ct,
                                                         const uint32_t* __restrict__ warp, float cval, float* __restrict__ xo, TT* __restrict__ to) {
  const int tiles = g.tiles_x * g.tiles_y;
  const int64_t per_sample = (int64_t)g.Z * tiles;
  const int b = (int)((int64_t)blockIdx.x / per_sample);
  const int rest = (int)((int64_t)blockIdx.x - (int64_t)b * per_sample);
  const int z = rest / tiles, tile = rest % tiles;
  const int yo0 = (tile / g.tiles_x) * WT, xo0 = (tile % g.tiles_x) * WT;
  const int nyo = min(WT, g.Y - yo0), nxo = min(WT, g.X - xo0);
  const int Y = g.Y, X = g.X;
  const int py = max(2 * Y - 2, 1), px = max(2 * X - 2, 1);

  const uint32_t* rc = warp + (size_t)b * WREC;
  const uint32_t flags = rc[BPX_WARP_W_FLAGS];
  WarpMap wm;
  wm.m00 = __uint_as_float(rc[BPX_WARP_W_M]); wm.m01 = __uint_as_float(rc[BPX_WARP_W_M + 1]); wm.m02 = __uint_as_float(rc[BPX_WARP_W_M + 2]);
  wm.m10 = __uint_as_float(rc[BPX_WARP_W_M + 3]); wm.m11 = __uint_as_float(rc[BPX_WARP_W_M + 4]); wm.m12 = __uint_as_float(rc[BPX_WARP_W_M + 5]);
  wm.cy = (float)(Y - 1) * 0.5f; wm.cx = (float)(X - 1) * 0.5f;

  const int64_t plane = ((int64_t)b * g.Z + z) * Y * X;           // the sample's z plane, in voxels: source and destination alike
  const float* xs = x + plane * C;
  const TT* ts = t + plane * Ct;
  const float rcp_c = 1.f / (float)C, rcp_ct = 1.f / (float)Ct;

  // ---- image ----
  {
    const int ipr = nxo * C, items = nyo * ipr;                    // < 2^15 items, rows of at most 2^9 elements: small_div is exact
    const float rcp = 1.f / (float)ipr;
    for (int i = threadIdx.x; i < items; i += 256) {
      const int r = small_div(i, rcp), e = i - r * ipr;
      const int xl = C == 1 ? e : small_div(e, rcp_c), c = e - xl * C;
      const int yo = yo0 + r, xv = xo0 + xl;
      const int64_t dst = ((int64_t)yo * X + xv) * C + c;
      float out;
      if (!flags) {
        out = xs[dst];
      } else {
        float fy, fx;
        wm.src(yo, xv, fy, fx);
        const float fy0 = floorf(fy), fx0 = floorf(fx);
        const float wy = __fsub_rn(fy, fy0), wx = __fsub_rn(fx, fx0);
        const int y0 = (int)fy0, x0 = (int)fx0;
        bool iy0, iy1, ix0, ix1;
        const int64_t ra = (int64_t)warp_tap<MODE>(y0, Y, py, iy0) * X, rb = (int64_t)warp_tap<MODE>(y0 + 1, Y, py, iy1) * X;
        const int xa = warp_tap<MODE>(x0, X, px, ix0), xb = warp_tap<MODE>(x0 + 1, X, px, ix1);
        float v00 = xs[(ra + xa) * C + c], v01 = xs[(ra + xb) * C + c], v10 = xs[(rb + xa) * C + c], v11 = xs[(rb + xb) * C + c];
        if constexpr (MODE == BPX_WARP_CONSTANT) {
          v00 = iy0 && ix0 ? v00 : cval; v01 = iy0 && ix1 ? v01 : cval;
          v10 = iy1 && ix0 ? v10 : cval; v11 = iy1 && ix1 ? v11 : cval;
        }
        out = warp_lerp(v00, v01, v10, v11, wx, wy);
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
      const int yo = yo0 + r, xv = xo0 + xl;
      const int64_t dst = ((int64_t)yo * X + xv) * Ct + c;
      TT out;
      if (!flags) {
        out = ts[dst];
      } else {
        float fy, fx;
        wm.src(yo, xv, fy, fx);
        bool iy, ix;
        const int ya = warp_tap<MODE>((int)floorf(__fadd_rn(fy, 0.5f)), Y, py, iy), xa = warp_tap<MODE>((int)floorf(__fadd_rn(fx, 0.5f)), X, px, ix);
        out = ts[((int64_t)ya * X + xa) * Ct + c];
        if constexpr (MODE == BPX_WARP_CONSTANT) out = iy && ix ? out : (TT)0;
      }
      to[plane * Ct + dst] = out;
    }
  }
}

template <typename TT>
void launch_warp(int mode, unsigned blocks, hipStream_t s, const float* x, const TT* t, WarpGeom g, int C, int Ct, const uint32_t* warp, float cval,
                 float* xo, TT* to) {
  if (mode == BPX_WARP_CONSTANT) warp_apply_kernel<TT, BPX_WARP_CONSTANT><<<blocks, 256, 0, s>>>(x, t, g, C, Ct, warp, cval, xo, to);
  else if (mode == BPX_WARP_REFLECT) warp_apply_kernel<TT, BPX_WARP_REFLECT><<<blocks, 256, 0, s>>>(x, t, g, C, Ct, warp, cval, xo, to);
  else warp_apply_kernel<TT, BPX_WARP_EDGE><<<blocks, 256, 0, s>>>(x, t, g, C, Ct, warp, cval, xo, to);
}

}  // namespace

extern "C" int bpx_aug_draw(const bpx_aug_cfg* cfg, int B, int Z, int Y, int X, uint64_t* state_d, uint32_t* records_d, bpx_stream_t stream) {
  const char* fn = "bpx_aug_draw";
  BPX_CHECK(cfg && state_d && records_d, "%s: null pointer", fn);
  BPX_CHECK(B > 0 && Z > 0 && Y > 0 && X > 0, "%s: bad extents", fn);
  BPX_CHECK(((uintptr_t)records_d & 15) == 0 && ((uintptr_t)state_d & 7) == 0, "%s: records must be 16-byte aligned, the state 8-byte aligned", fn);
  BPX_CHECK(cfg->thr <= (1ull << 32), "%s: thr above 2^32", fn);
  if (cfg->enable & BPX_AUG_EN_CUTOUT) {
    BPX_CHECK(cfg->box_lo >= 1 && cfg->box_lo <= cfg->box_hi && cfg->box_hi <= BPX_AUG_MAX_BOXES, "%s: box count range outside 1..%d", fn, BPX_AUG_MAX_BOXES);
    BPX_CHECK(cfg->f_lo > 0.f && cfg->f_lo <= cfg->f_hi && cfg->f_hi <= 1.f, "%s: box size fractions outside (0, 1]", fn);
  }
  aug_draw_kernel<<<cdiv(B, 256), 256, 0, (hipStream_t)stream>>>(*cfg, B, Z, Y, X, state_d, records_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_aug_mean_blocks(int64_t n) { return n > 0 ? mean_blocks(n) : 0; }

extern "C" int bpx_aug_mean(const float* x_d, int B, int64_t n, double* ws_d, uint32_t* records_d, bpx_stream_t stream) {
  const char* fn = "bpx_aug_mean";
  BPX_CHECK(x_d && ws_d && records_d, "%s: null pointer", fn);
  BPX_CHECK(B > 0 && B <= 65535 && n > 0, "%s: bad extents", fn);
  const int blocks = mean_blocks(n);
  aug_mean_partial_kernel<<<dim3(blocks, B), 256, 0, (hipStream_t)stream>>>(x_d, n, ws_d);
  BPX_LAUNCH_CHECK(fn);
  aug_mean_final_kernel<<<B, MEAN_MAX_BLOCKS, 0, (hipStream_t)stream>>>(ws_d, blocks, n, records_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_aug_apply(const float* x_d, const void* t_d, int t_dtype, int B, int Z, int Y, int X, int C, int Ct, const uint32_t* records_d,
                             uint64_t seed, float cval, int mask_too, float* x_out_d, void* t_out_d, bpx_stream_t stream) {
  const char* fn = "bpx_aug_apply";
  BPX_CHECK(x_d && t_d && records_d && x_out_d && t_out_d, "%s: null pointer", fn);
  BPX_CHECK(B > 0 && Z > 0 && Y > 0 && X > 0, "%s: bad extents", fn);
  BPX_CHECK(C >= 1 && C <= 16 && Ct >= 1 && Ct <= 8, "%s: 1..16 image channels and 1..8 target channels (got %d, %d)", fn, C, Ct);
  BPX_CHECK(t_dtype == BPX_F32 || t_dtype == BPX_U8, "%s: the target is float32 or uint8", fn);
  BPX_CHECK((const void*)x_d != (const void*)x_out_d && t_d != t_out_d, "%s: the pass is a gather and cannot run in place", fn);
  AugGeom g;
  g.Z = Z; g.Y = Y; g.X = X;
  g.T = tile_edge(C, Ct);
  g.tiles_x = cdiv(X, g.T); g.tiles_y = cdiv(Y, g.T);
  const int64_t blocks = (int64_t)B * Z * g.tiles_x * g.tiles_y;
  BPX_CHECK(blocks < (1ll << 31), "%s: %lld tiles exceed one launch", fn, (long long)blocks);
  const int pitch_x = tile_pitch(g.T, C), pitch_t = tile_pitch(g.T, Ct);
  const size_t lds = (size_t)g.T * (pitch_x + pitch_t) * 4;
  BPX_CHECK(lds <= 65536, "%s: internal: %zu bytes of LDS", fn, lds);
  // vector accesses: every row segment of a tile then starts and ends on a multiple of 4 elements (tile edges are multiples of 16 voxels, the
  // plane's rows hold a multiple of 4 elements; an odd k has Y == X) - 16 bytes of fp32, 4 bytes of uint8
  const auto aligned = [](const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; };
  const int vx = ((int64_t)X * C) % 4 == 0 && aligned(x_d, 16) && aligned(x_out_d, 16);
  const size_t ta = t_dtype == BPX_F32 ? 16 : 4;
  const int vt = ((int64_t)X * Ct) % 4 == 0 && aligned(t_d, ta) && aligned(t_out_d, ta);
  if (t_dtype == BPX_F32)
    launch_apply<float>(vx, vt, (unsigned)blocks, lds, (hipStream_t)stream, x_d, (const float*)t_d, g, C, Ct, pitch_x, pitch_t, records_d, seed, cval,
                        mask_too, x_out_d, (float*)t_out_d);
  else
    launch_apply<uint8_t>(vx, vt, (unsigned)blocks, lds, (hipStream_t)stream, x_d, (const uint8_t*)t_d, g, C, Ct, pitch_x, pitch_t, records_d, seed, cval,
                          mask_too, x_out_d, (uint8_t*)t_out_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_warp_draw(const bpx_warp_cfg* cfg, int B, int Y, int X, const uint32_t* records_d, uint32_t* warp_d, bpx_stream_t stream) {
  const char* fn = "bpx_warp_draw";
  BPX_CHECK(cfg && records_d && warp_d, "%s: null pointer", fn);
  BPX_CHECK(B > 0 && Y > 0 && X > 0, "%s: bad extents", fn);
  BPX_CHECK(((uintptr_t)warp_d & 15) == 0 && ((uintptr_t)records_d & 3) == 0, "%s: warp records must be 16-byte aligned", fn);
  BPX_CHECK(cfg->thr <= (1ull << 32), "%s: thr above 2^32", fn);
  BPX_CHECK((cfg->enable & ~0xFu) == 0, "%s: unknown enable bits", fn);
  BPX_CHECK(cfg->rot_lo <= cfg->rot_hi && cfg->shear_lo <= cfg->shear_hi && cfg->shift_lo <= cfg->shift_hi, "%s: a range has lo > hi", fn);
  if (cfg->enable & BPX_WARP_F_ZOOM) BPX_CHECK(cfg->zoom_lo > 0.f && cfg->zoom_lo <= cfg->zoom_hi, "%s: the zoom range must be positive with lo <= hi", fn);
  warp_draw_kernel<<<cdiv(B, 256), 256, 0, (hipStream_t)stream>>>(*cfg, B, Y, X, records_d, warp_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_warp_apply(const float* x_d, const void* t_d, int t_dtype, int B, int Z, int Y, int X, int C, int Ct, const uint32_t* warp_d, int mode,
                              float cval, float* x_out_d, void* t_out_d, bpx_stream_t stream) {
  const char* fn = "bpx_warp_apply";
  BPX_CHECK(x_d && t_d && warp_d && x_out_d && t_out_d, "%s: null pointer", fn);
  BPX_CHECK(B > 0 && Z > 0 && Y > 0 && X > 0, "%s: bad extents", fn);
  BPX_CHECK(C >= 1 && C <= 16 && Ct >= 1 && Ct <= 8, "%s: 1..16 image channels and 1..8 target channels (got %d, %d)", fn, C, Ct);
  BPX_CHECK(t_dtype == BPX_F32 || t_dtype == BPX_U8, "%s: the target is float32 or uint8", fn);
  BPX_CHECK(mode == BPX_WARP_CONSTANT || mode == BPX_WARP_REFLECT || mode == BPX_WARP_EDGE, "%s: unknown border mode %d", fn, mode);
  BPX_CHECK((const void*)x_d != (const void*)x_out_d && t_d != t_out_d, "%s: the pass is a gather and cannot run in place", fn);
  BPX_CHECK(Y <= (1 << 24) && X <= (1 << 24), "%s: a plane axis above 2^24 voxels", fn);      // (Y-1)/2 and every y - cy stay exact in fp32
  WarpGeom g;
  g.Z = Z; g.Y = Y; g.X = X;
  g.tiles_x = cdiv(X, WT); g.tiles_y = cdiv(Y, WT);
  const int64_t blocks = (int64_t)B * Z * g.tiles_x * g.tiles_y;
  BPX_CHECK(blocks < (1ll << 31), "%s: %lld tiles exceed one launch", fn, (long long)blocks);
  if (t_dtype == BPX_F32)
    launch_warp<float>(mode, (unsigned)blocks, (hipStream_t)stream, x_d, (const float*)t_d, g, C, Ct, warp_d, cval, x_out_d, (float*)t_out_d);
  else
    launch_warp<uint8_t>(mode, (unsigned)blocks, (hipStream_t)stream, x_d, (const uint8_t*)t_d, g, C, Ct, warp_d, cval, x_out_d, (uint8_t*)t_out_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
