// Random training patches from device-resident volumes (biapy_amd/sampler.py states the semantics, include/biapy_amd.h the origin record, the
// descriptors and the two draw modes): bpx_patch_draw fills one (v, z0, y0, x0) record per sample, bpx_patch_gather copies the windows.
//
// Random numbers: Philox4x32-10 (philox.h), key = the sampler's 64-bit seed, counter words = (sample, stream, counter low, counter high) with the
// sampler's own device counter, one value per call - the augmenter's keying (augment.hip).  Streams of the draw kernel, r = the four output words:
//   0      r64 = (uint64) r0 << 32 | r1: the origin (uniform mode) or the voxel of the drawn class (class mode); r2 >> 8: the class; r3 unused
// Every quantity that decides an origin is an integer, except the one fp32 compare of u = (r2 >> 8) * 2^-24 with the running class sums.
//
// Draw kernel: one wave per sample.  Philox and the binary searches are wave-uniform (every lane computes the same values); the search inside the
// drawn row of a class map is the wave's: 64 voxels per step, a ballot of the voxels of the class, population counts.  Every loop is bounded by 64
// binary-search steps or by ceil(X / 64); no thread waits on another, apart from the ticket's single atomicAdd.
//
// Gather kernel: one workgroup = a share of one (sample, z) plane of the OUTPUT, whose Py rows of L = Px * C elements are contiguous.  Where L is a
// multiple of the elements in 16 bytes of output (and the output is 16-byte aligned) every lane moves one 16-byte output piece per step, four steps
// in flight: ONE load of its source elements (16 bytes of a float32 image or target, 8 / 4 bytes of a uint16 / uint8 image, 16 bytes of a uint8
// target) at the source's element alignment - a row starts x0 * C elements into its line, wherever that is; global loads of gfx950 take any
// address - and one 16-byte store.  FALLBACK where L is no such multiple, or the output is not aligned: element by element.
#include "bpx_common.h"
#include "philox.h"

namespace {

// the last i in [0, n) with at(i) <= k, for a non-decreasing at with at(0) <= k: at most 64 steps
template <typename F>
__device__ __forceinline__ int64_t last_le(F at, int64_t n, int64_t k) {
  int64_t lo = 0, hi = n;
  for (int s = 0; s < 64 && hi - lo > 1; ++s) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (at(mid) <= k) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return max(lo, min(v, hi)); }

__global__ void __launch_bounds__(256) patch_draw_kernel(const bpx_patch_cfg cfg, const bpx_patch_vol* __restrict__ vols, const int64_t* __restrict__ cum,
                                                         const int64_t* __restrict__ rowcum, int64_t R, int B, uint64_t* __restrict__ state,
                                                         int32_t* __restrict__ origins) {
  const uint64_t ctr = state[0];
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);          // wave-uniform
  if (b < B) {
    uint32_t r[4];
    philox4x32_10((uint32_t)b, 0u, (uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)cfg.seed, (uint32_t)(cfg.seed >> 32), r);
    const uint64_t r64 = ((uint64_t)r[0] << 32) | r[1];
    int v, z0, y0, x0;
    if (cfg.K == 0) {
      const int64_t k = (int64_t)__umul64hi(r64, (uint64_t)cum[cfg.V]);
      v = (int)last_le([&](int64_t i) { return cum[i]; }, cfg.V, k);
      int64_t rest = k - cum[v];
      const int64_t nx = vols[v].X - cfg.Px + 1, ny = vols[v].Y - cfg.Py + 1;
      x0 = (int)(rest % nx); rest /= nx;
      y0 = (int)(rest % ny);
      z0 = (int)(rest / ny);
    } else {
      const float u = (float)(r[2] >> 8) * 5.9604644775390625e-8f;   // 2^-24, exact
      int c = cfg.K - 1;
#pragma unroll
      for (int i = 7; i >= 0; --i)
        if (i < cfg.K && u < cfg.class_cum[i]) c = i;                // the first class whose running sum exceeds u
      const int64_t* rc = rowcum + (int64_t)c * (R + 1);
      const int64_t k = (int64_t)__umul64hi(r64, (uint64_t)rc[R]);
      const int64_t row = last_le([&](int64_t i) { return rc[i]; }, R, k);
      int64_t j = k - rc[row];
      v = (int)last_le([&](int64_t i) { return vols[i].row0; }, cfg.V, row);
      const bpx_patch_vol vol = vols[v];
      const int64_t rin = row - vol.row0;                            // z * Y + y
      const int z = (int)(rin / vol.Y), y = (int)(rin - (int64_t)z * vol.Y);
      const uint8_t* line = vol.cls + rin * vol.X;
      int x = 0;
      for (int base = 0; base < vol.X; base += 64) {                 // wave-uniform: j, the mask and its count are the same in every lane
        const int xi = base + lane;
        const bool hit = xi < vol.X && line[xi] == (uint8_t)c;
        const unsigned long long mask = __ballot(hit);
        const int64_t cnt = __popcll(mask);
        if (j < cnt) {                                               // the (j+1)-th set bit of the mask
          const bool mine = hit && __popcll(mask & ((1ull << lane) - 1ull)) == (int)j;
          x = base + (__ffsll((long long)__ballot(mine)) - 1);
          break;
        }
        j -= cnt;
      }
      z0 = clampi(z - cfg.Pz / 2, 0, vol.Z - cfg.Pz);
      y0 = clampi(y - cfg.Py / 2, 0, vol.Y - cfg.Py);
      x0 = clampi(x - cfg.Px / 2, 0, vol.X - cfg.Px);
    }
    if (lane == 0) *reinterpret_cast<u32x4_t*>(origins + (size_t)b * 4) = u32x4_t{(uint32_t)v, (uint32_t)z0, (uint32_t)y0, (uint32_t)x0};
  }
  // the counter advances once, after every block has read it (the ticket scheme of aug_draw_kernel)
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

// ---- the gather pass ---------------------------------------------------------------------------------------------------------------------
struct GatherGeom { int V, Pz, Py, Px, C, Ct; };
constexpr int FLIGHT = 4;                                               // 16-byte pieces a lane has in flight
// a volume's pointer comes out of a descriptor in memory: say that it is global memory (global_load instead of flat_load)
template <typename T> using global_ptr = const __attribute__((address_space(1))) T*;

// one output element of the image: exact conversion, then the optional fp32 multiply; float32 travels as its bits
template <typename TS> __device__ __forceinline__ uint32_t image_word(TS s, bool use_scale, float scale) {
  const float f = (float)s;
  return __float_as_uint(use_scale ? __fmul_rn(f, scale) : f);
}
template <> __device__ __forceinline__ uint32_t image_word<uint32_t>(uint32_t s, bool use_scale, float scale) {
  return use_scale ? __float_as_uint(__fmul_rn(__uint_as_float(s), scale)) : s;
}

// the Py rows of L elements of one output plane <- rows `pitch` elements apart in the source; 16-byte pieces of 4 output words
template <typename TS>
__device__ __forceinline__ void image_plane(const TS* __restrict__ src, int64_t pitch, int Py, int L, uint32_t* __restrict__ dst, bool fast, bool use_scale,
                                            float scale) {
  if (fast) {
    const int ppr = L / 4, pieces = Py * ppr;
    const global_ptr<TS> gsrc = (global_ptr<TS>)src;
    for (int i0 = blockIdx.y * (256 * FLIGHT) + threadIdx.x; i0 < pieces; i0 += gridDim.y * (256 * FLIGHT)) {
      TS s[FLIGHT][4];
#pragma unroll
      for (int u = 0; u < FLIGHT; ++u) {                              // FLIGHT loads in flight, then their stores
        const int i = i0 + u * 256;
        if (i < pieces) {
          const int y = i / ppr, e = (i - y * ppr) * 4;
          __builtin_memcpy(s[u], gsrc + (int64_t)y * pitch + e, sizeof(s[u]));
        }
      }
#pragma unroll
      for (int u = 0; u < FLIGHT; ++u) {
        const int i = i0 + u * 256;
        if (i < pieces)
          *reinterpret_cast<u32x4_t*>(dst + (int64_t)i * 4) = u32x4_t{image_word(s[u][0], use_scale, scale), image_word(s[u][1], use_scale, scale),
                                                                     image_word(s[u][2], use_scale, scale), image_word(s[u][3], use_scale, scale)};
      }
    }
  } else {
    const int n = Py * L;
    for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256) {
      const int y = i / L, e = i - y * L;
      dst[i] = image_word(src[(int64_t)y * pitch + e], use_scale, scale);
    }
  }
}

// the same for the target, bit for bit: 16-byte pieces of 16 / sizeof(T) elements
template <typename T>
__device__ __forceinline__ void target_plane(const T* __restrict__ src, int64_t pitch, int Py, int L, T* __restrict__ dst, bool fast) {
  constexpr int VEC = 16 / (int)sizeof(T);
  if (fast) {
    const int ppr = L / VEC, pieces = Py * ppr;
    const global_ptr<T> gsrc = (global_ptr<T>)src;
    for (int i0 = blockIdx.y * (256 * FLIGHT) + threadIdx.x; i0 < pieces; i0 += gridDim.y * (256 * FLIGHT)) {
      u32x4_t w[FLIGHT];
#pragma unroll
      for (int u = 0; u < FLIGHT; ++u) {
        const int i = i0 + u * 256;
        if (i < pieces) {
          const int y = i / ppr, e = (i - y * ppr) * VEC;
          __builtin_memcpy(&w[u], gsrc + (int64_t)y * pitch + e, 16);
        }
      }
#pragma unroll
      for (int u = 0; u < FLIGHT; ++u) {
        const int i = i0 + u * 256;
        if (i < pieces) *reinterpret_cast<u32x4_t*>(dst + (int64_t)i * VEC) = w[u];
      }
    }
  } else {
    const int n = Py * L;
    for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256) {
      const int y = i / L, e = i - y * L;
      dst[i] = src[(int64_t)y * pitch + e];
    }
  }
}

// TI: uint32_t (the bits of a float32 image), uint16_t or uint8_t; TT: uint32_t (the bits of a float32 target) or uint8_t
template <typename TI, typename TT>
__global__ void __launch_bounds__(256) patch_gather_kernel(const bpx_patch_vol* __restrict__ vols, const GatherGeom g, const int32_t* __restrict__ origins,
                                                           int fast_x, int fast_t, int use_scale, float scale, uint32_t* __restrict__ xo, TT* __restrict__ to) {
  const int b = blockIdx.x / g.Pz, z = blockIdx.x - b * g.Pz;
  const u32x4_t o = *reinterpret_cast<const u32x4_t*>(origins + (size_t)b * 4);
  const bpx_patch_vol vol = vols[clampi((int)o[0], 0, g.V - 1)];
  // an origin outside its volume is moved inside: no record, whatever wrote it, makes the pass read outside the volumes
  const int z0 = clampi((int)o[1], 0, vol.Z - g.Pz), y0 = clampi((int)o[2], 0, vol.Y - g.Py), x0 = clampi((int)o[3], 0, vol.X - g.Px);
  const int64_t vox0 = ((int64_t)(z0 + z) * vol.Y + y0) * vol.X + x0;      // 64 bits: a volume may hold more than 2^31 voxels
  const int64_t plane = (int64_t)blockIdx.x * g.Py * g.Px;                  // output voxels ahead of this plane
  image_plane<TI>(reinterpret_cast<const TI*>(vol.img) + vox0 * g.C, (int64_t)vol.X * g.C, g.Py, g.Px * g.C, xo + plane * g.C, fast_x != 0, use_scale != 0,
                  scale);
  target_plane<TT>(reinterpret_cast<const TT*>(vol.tgt) + vox0 * g.Ct, (int64_t)vol.X * g.Ct, g.Py, g.Px * g.Ct, to + plane * g.Ct, fast_t != 0);
}

int check_vols(const char* fn, const bpx_patch_vol* vols_h, int V, int Pz, int Py, int Px, bool need_data, bool need_cls) {
  BPX_CHECK(V >= 1, "%s: no volume", fn);
  BPX_CHECK(Pz >= 1 && Py >= 1 && Px >= 1, "%s: bad patch %d x %d x %d", fn, Pz, Py, Px);
  int64_t rows = 0;
  for (int v = 0; v < V; ++v) {
    const bpx_patch_vol& w = vols_h[v];
    BPX_CHECK(w.Z >= 1 && w.Y >= 1 && w.X >= 1, "%s: volume %d has bad extents", fn, v);
    BPX_CHECK(Pz <= w.Z && Py <= w.Y && Px <= w.X, "%s: the patch %d x %d x %d is larger than volume %d (%d x %d x %d)", fn, Pz, Py, Px, v, w.Z, w.Y, w.X);
    BPX_CHECK(!need_data || (w.img && w.tgt), "%s: null pointer (volume %d)", fn, v);
    BPX_CHECK(!need_cls || w.cls, "%s: null pointer (class map of volume %d)", fn, v);
    BPX_CHECK(w.row0 == rows, "%s: volume %d starts at row %lld, not at %lld", fn, v, (long long)w.row0, (long long)rows);
    rows += (int64_t)w.Z * w.Y;
  }
  return 0;
}

template <typename TI, typename TT>
void launch_gather(dim3 grid, hipStream_t s, const bpx_patch_vol* vols, const GatherGeom& g, const int32_t* origins, int fast_x, int fast_t, int use_scale,
                   float scale, float* xo, void* to) {
  patch_gather_kernel<TI, TT><<<grid, 256, 0, s>>>(vols, g, origins, fast_x, fast_t, use_scale, scale, reinterpret_cast<uint32_t*>(xo), reinterpret_cast<TT*>(to));
}

}  // namespace

extern "C" int bpx_patch_draw(const bpx_patch_cfg* cfg, const bpx_patch_vol* vols_h, const bpx_patch_vol* vols_d, const int64_t* cum_d,
                              const int64_t* rowcum_d, int64_t R, int B, uint64_t* state_d, int32_t* origins_d, bpx_stream_t stream) {
  const char* fn = "bpx_patch_draw";
  BPX_CHECK(cfg && vols_h && vols_d && state_d && origins_d, "%s: null pointer", fn);
  BPX_CHECK(B >= 1, "%s: B must be at least 1 (got %d)", fn, B);
  BPX_CHECK(cfg->K >= 0 && cfg->K <= 8, "%s: 1..8 classes, or 0 for the uniform mode (got %d)", fn, cfg->K);
  BPX_CHECK(((uintptr_t)origins_d & 15) == 0 && ((uintptr_t)state_d & 7) == 0, "%s: origins must be 16-byte aligned, the state 8-byte aligned", fn);
  if (check_vols(fn, vols_h, cfg->V, cfg->Pz, cfg->Py, cfg->Px, false, cfg->K > 0)) return 1;
  if (cfg->K == 0) {
    BPX_CHECK(cum_d, "%s: null pointer (cum_d, uniform mode)", fn);
  } else {
    BPX_CHECK(rowcum_d, "%s: null pointer (rowcum_d, class mode)", fn);
    const bpx_patch_vol& last = vols_h[cfg->V - 1];
    BPX_CHECK(R == last.row0 + (int64_t)last.Z * last.Y, "%s: R = %lld is not the number of rows of the volumes", fn, (long long)R);
    float prev = 0.f;
    for (int c = 0; c < cfg->K; ++c) {
      BPX_CHECK(cfg->class_cum[c] >= prev && cfg->class_cum[c] <= 1.f, "%s: class_cum must be non-decreasing within [0, 1]", fn);
      prev = cfg->class_cum[c];
    }
    BPX_CHECK(prev == 1.f, "%s: the last class_cum must be 1", fn);
  }
  patch_draw_kernel<<<cdiv(B, 4), 256, 0, (hipStream_t)stream>>>(*cfg, vols_d, cum_d, rowcum_d, R, B, state_d, origins_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_patch_gather(const bpx_patch_vol* vols_h, const bpx_patch_vol* vols_d, int V, int img_dtype, int C, int tgt_dtype, int Ct, int Pz, int Py,
                                int Px, const int32_t* origins_d, int B, int use_scale, float scale, float* x_out_d, void* t_out_d, bpx_stream_t stream) {
  const char* fn = "bpx_patch_gather";
  BPX_CHECK(vols_h && vols_d && origins_d && x_out_d && t_out_d, "%s: null pointer", fn);
  BPX_CHECK(B >= 1, "%s: B must be at least 1 (got %d)", fn, B);
  BPX_CHECK(C >= 1 && C <= 16 && Ct >= 1 && Ct <= 8, "%s: 1..16 image channels and 1..8 target channels (got %d, %d)", fn, C, Ct);
  BPX_CHECK(img_dtype == BPX_F32 || img_dtype == BPX_U8 || img_dtype == BPX_U16, "%s: the image is float32, uint8 or uint16", fn);
  BPX_CHECK(tgt_dtype == BPX_F32 || tgt_dtype == BPX_U8, "%s: the target is float32 or uint8", fn);
  if (check_vols(fn, vols_h, V, Pz, Py, Px, true, false)) return 1;
  BPX_CHECK(((uintptr_t)origins_d & 15) == 0, "%s: origins must be 16-byte aligned", fn);
  BPX_CHECK(((uintptr_t)x_out_d & 3) == 0 && (tgt_dtype == BPX_U8 || ((uintptr_t)t_out_d & 3) == 0), "%s: outputs must be aligned to their elements", fn);
  BPX_CHECK((int64_t)Py * Px * 16 < (1ll << 31), "%s: a plane of %d x %d voxels exceeds one launch", fn, Py, Px);
  BPX_CHECK((int64_t)B * Pz < (1ll << 31), "%s: %lld planes exceed one launch", fn, (long long)B * Pz);
  const GatherGeom g{V, Pz, Py, Px, C, Ct};
  const int vt = tgt_dtype == BPX_U8 ? 16 : 4;
  const int fast_x = (Px * C) % 4 == 0 && ((uintptr_t)x_out_d & 15) == 0;
  const int fast_t = (Px * Ct) % vt == 0 && ((uintptr_t)t_out_d & 15) == 0;
  // a lane's steps: 16-byte pieces on the fast paths, elements otherwise; four steps per lane and workgroup
  const int64_t steps_x = (int64_t)Py * Px * C / (fast_x ? 4 : 1), steps_t = (int64_t)Py * Px * Ct / (fast_t ? vt : 1);
  const dim3 grid((unsigned)(B * Pz), (unsigned)std::min<int64_t>(65535, std::max<int64_t>(1, cdiv64(std::max(steps_x, steps_t), 256 * FLIGHT))));
  const hipStream_t s = (hipStream_t)stream;
  const bool t8 = tgt_dtype == BPX_U8;
  if (img_dtype == BPX_F32) {
    if (t8) launch_gather<uint32_t, uint8_t>(grid, s, vols_d, g, origins_d, fast_x, fast_t, use_scale, scale, x_out_d, t_out_d);
    else launch_gather<uint32_t, uint32_t>(grid, s, vols_d, g, origins_d, fast_x, fast_t, use_scale, scale, x_out_d, t_out_d);
  } else if (img_dtype == BPX_U16) {
    if (t8) launch_gather<uint16_t, uint8_t>(grid, s, vols_d, g, origins_d, fast_x, fast_t, use_scale, scale, x_out_d, t_out_d);
    else launch_gather<uint16_t, uint32_t>(grid, s, vols_d, g, origins_d, fast_x, fast_t, use_scale, scale, x_out_d, t_out_d);
  } else {
    if (t8) launch_gather<uint8_t, uint8_t>(grid, s, vols_d, g, origins_d, fast_x, fast_t, use_scale, scale, x_out_d, t_out_d);
    else launch_gather<uint8_t, uint32_t>(grid, s, vols_d, g, origins_d, fast_x, fast_t, use_scale, scale, x_out_d, t_out_d);
  }
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
