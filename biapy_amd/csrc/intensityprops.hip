// Intensity properties of an int32 label volume (Z, Y, X) and an image of the same shape (float32, uint8 or uint16) on the device: for every
// label l in 1..n_max its voxel count, the smallest and the largest image value, the EXACT sum of its image values as int64 limbs, that sum
// rounded once to float64, the mean, and the counts of NaN / +inf / -inf voxels - scikit-image's intensity_min / intensity_max /
// intensity_mean, scipy.ndimage's minimum / maximum / sum_labels / mean with an index.  The one per-label measurement with a second
// volume-sized operand: the reference copies both volumes to the host for it.
//
// LAUNCHES, fixed by (Z, Y, X, n_max, dtype): init (count, limbs and counters 0, the keys at their initial values), accumulate, finish (keys
// decoded, limbs rounded, the non-finite rule, the division; row 0 and the labels no voxel carries zeros with a NaN mean).  The outputs are the
// accumulators: no workspace.  Global memory sees relaxed, agent-scope integer atomics only (uint32 / int64 add, uint32 min / max): a float sum
// would depend on the order, the limbs of intensityprops_core.h do not - the same bits every run.  Nothing is read back, capturable; every loop
// is bounded by a launch parameter or a constant, none by what another thread does.
//
// THE ACCUMULATE PASS walks the volume as regionprops.hip does: a WAVE owns a span of OVL_SPAN = 8192 voxels and takes it in trips of 256, lane
// l holding the voxels 4 l .. 4 l + 3 of the labels and of the image (16-byte loads of the labels and a float32 image, 8-byte of uint16, 4-byte
// of uint8 where the pointer is so aligned, element loads otherwise and at the ragged end - the same bits either way; the next trip's loads are
// issued before this trip is worked on).  A voxel's contribution is not closed form, so there are no runs: each lane first merges those of its
// four voxels that share a label and a limb (ip_fits / ip_absorb: count, the two keys, the two limb sums, the counters) and sends one
// accumulator where four voxels agree.  The block's four waves meet in a table of 256 records keyed by label in LDS (regionprops_core.h's slot
// scheme; 25 600 bytes for float32), which is merged into the global arrays once per occupied slot at the block's end, zero limbs and counters
// skipped; what the table does not take goes to global directly.
// TWO FORMS, the same bits: (a) the lane merge alone; (b) in addition a trip whose 256 voxels carry ONE label (a ballot), all finite and with
// pieces for one limb pair, is reduced across the wave - count 256, the two keys, two int64 sums - and lane 0 sends it: an object wider than a
// trip otherwise sends 64 accumulators to one slot's words, which LDS serialises.  Form (a) is the default: on labelled instances few trips
// are uniform and the test, the reductions' registers (96 VGPRs against 70: five waves per SIMD against the six the table's LDS allows) cost
// more than they save (float32 balls at 1024^3: 2.56 ms against 2.95 ms, uint8: 1.39 against 1.51).  Form (b) stays selectable because it wins on
// one measured input, one label over the whole volume (1024^3: 2.57 ms against 4.45 ms).  bpx_debug_set_intensityprops_wave picks the form
// (environment: BPX_INTENSITYPROPS_WAVE); figures: profiles/intensityprops_timing.json, DESIGN.md section 4.
#include "bpx_common.h"
#include "intensityprops_core.h"
#include "label_walk.h"

namespace {

template <int NL> struct IpDev {     // the global per-label arrays, the atomics at the memory side
  unsigned* area_p;
  unsigned* kmin_p;
  unsigned* kmax_p;
  long long* limbs_p;
  unsigned* nonf_p;
  __device__ __forceinline__ void count(uint32_t r, uint32_t c) const { __hip_atomic_fetch_add(area_p + r, c, LW_RLX_AGENT); }
  __device__ __forceinline__ void kmin(uint32_t r, uint32_t k) const { __hip_atomic_fetch_min(kmin_p + r, k, LW_RLX_AGENT); }
  __device__ __forceinline__ void kmax(uint32_t r, uint32_t k) const { __hip_atomic_fetch_max(kmax_p + r, k, LW_RLX_AGENT); }
  __device__ __forceinline__ void limb(uint32_t r, int j, int64_t v) const { __hip_atomic_fetch_add(limbs_p + (int64_t)r * NL + j, (long long)v, LW_RLX_AGENT); }
  __device__ __forceinline__ void nonf(uint32_t r, int k, uint32_t c) const { __hip_atomic_fetch_add(nonf_p + (int64_t)r * 3 + k, c, LW_RLX_AGENT); }
};

template <int NL> struct IpLds : LwKeysLds {     // the block's table in LDS
  unsigned* count_p;
  unsigned* kmin_p;
  unsigned* kmax_p;
  long long* limbs_p;
  unsigned* nonf_p;
  __device__ __forceinline__ void count(uint32_t s, uint32_t c) const { __hip_atomic_fetch_add(count_p + s, c, LW_RLX_WG); }
  __device__ __forceinline__ void kmin(uint32_t s, uint32_t k) const { __hip_atomic_fetch_min(kmin_p + s, k, LW_RLX_WG); }
  __device__ __forceinline__ void kmax(uint32_t s, uint32_t k) const { __hip_atomic_fetch_max(kmax_p + s, k, LW_RLX_WG); }
  __device__ __forceinline__ void limb(uint32_t s, int j, int64_t v) const { __hip_atomic_fetch_add(limbs_p + s * NL + j, (long long)v, LW_RLX_WG); }
  __device__ __forceinline__ void nonf(uint32_t s, int k, uint32_t c) const { __hip_atomic_fetch_add(nonf_p + s * 3 + k, c, LW_RLX_WG); }
  __device__ __forceinline__ uint32_t count_of(uint32_t s) const { return count_p[s]; }
  __device__ __forceinline__ uint32_t kmin_of(uint32_t s) const { return kmin_p[s]; }
  __device__ __forceinline__ uint32_t kmax_of(uint32_t s) const { return kmax_p[s]; }
  __device__ __forceinline__ int64_t limb_of(uint32_t s, int j) const { return limbs_p[s * NL + j]; }
  __device__ __forceinline__ uint32_t nonf_of(uint32_t s, int k) const { return nonf_p[s * 3 + k]; }
};

// the image's voxels i .. i + 3 as 32-bit words (the float's bits, the integer widened): one load of 4 elements where `vec`
template <int DT> __device__ __forceinline__ void load4_image(const void* __restrict__ image, int64_t i, int64_t end, bool vec, uint32_t b[OVL_VPL]) {
  if constexpr (DT == BPX_F32) {
    const uint32_t* x = static_cast<const uint32_t*>(image);
    if (i + OVL_VPL <= end) {
      if (vec) {
        const u32x4_t w = *reinterpret_cast<const u32x4_t*>(x + i);
        b[0] = w[0]; b[1] = w[1]; b[2] = w[2]; b[3] = w[3];
      } else {
        b[0] = x[i]; b[1] = x[i + 1]; b[2] = x[i + 2]; b[3] = x[i + 3];
      }
    } else {
#pragma unroll
      for (int e = 0; e < OVL_VPL; ++e) b[e] = (i + e < end) ? x[i + e] : 0u;
    }
  } else if constexpr (DT == BPX_U16) {
    const uint16_t* x = static_cast<const uint16_t*>(image);
    if (i + OVL_VPL <= end) {
      if (vec) {
        const u32x2_t w = *reinterpret_cast<const u32x2_t*>(x + i);
        b[0] = w[0] & 0xffffu; b[1] = w[0] >> 16; b[2] = w[1] & 0xffffu; b[3] = w[1] >> 16;
      } else {
        b[0] = x[i]; b[1] = x[i + 1]; b[2] = x[i + 2]; b[3] = x[i + 3];
      }
    } else {
#pragma unroll
      for (int e = 0; e < OVL_VPL; ++e) b[e] = (i + e < end) ? (uint32_t)x[i + e] : 0u;
    }
  } else {
    const uint8_t* x = static_cast<const uint8_t*>(image);
    if (i + OVL_VPL <= end) {
      if (vec) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(x + i);
        b[0] = w & 0xffu; b[1] = (w >> 8) & 0xffu; b[2] = (w >> 16) & 0xffu; b[3] = w >> 24;
      } else {
        b[0] = x[i]; b[1] = x[i + 1]; b[2] = x[i + 2]; b[3] = x[i + 3];
      }
    } else {
#pragma unroll
      for (int e = 0; e < OVL_VPL; ++e) b[e] = (i + e < end) ? (uint32_t)x[i + e] : 0u;
    }
  }
}

// reductions over the 64 lanes of a wave, every lane receives the result.  LOOP BOUND: 6 steps
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int o = OVL_LANES / 2; o; o >>= 1) { const uint32_t t = __shfl_xor(v, o, OVL_LANES); v = t < v ? t : v; }
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = OVL_LANES / 2; o; o >>= 1) { const uint32_t t = __shfl_xor(v, o, OVL_LANES); v = t > v ? t : v; }
  return v;
}
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
  for (int o = OVL_LANES / 2; o; o >>= 1) v += (int64_t)__shfl_xor((long long)v, o, OVL_LANES);
  return v;
}

// init / finish: thread t takes the rows t, t + T ...  LOOP BOUND: ceil(rows / T) trips, fixed by the launch
template <int NL> __global__ void __launch_bounds__(256) ip_init_kernel(uint32_t* __restrict__ area, uint32_t* __restrict__ kmin, uint32_t* __restrict__ kmax,
                                                                        int64_t* __restrict__ limbs, uint32_t* __restrict__ nonf, int64_t rows) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256)
    ip_init_row<NL>(area + r, kmin + r, kmax + r, limbs + r * NL, nonf + r * 3);
}
template <int NL, bool F32> __global__ void __launch_bounds__(256) ip_finish_kernel(const uint32_t* __restrict__ area, uint32_t* __restrict__ kmin,
                                                                                   uint32_t* __restrict__ kmax, const int64_t* __restrict__ limbs,
                                                                                   const uint32_t* __restrict__ nonf, double* __restrict__ sum,
                                                                                   double* __restrict__ mean, int64_t rows) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256)
    ip_finish_row<NL, F32>(r, area + r, kmin + r, kmax + r, limbs + r * NL, nonf + r * 3, sum + r, mean + r);
}

// accumulate: wave w of the grid owns the voxels [w * OVL_SPAN, (w + 1) * OVL_SPAN) below n.  LOOP BOUND: OVL_SPAN / OVL_TRIP = 32 trips; the clear
// and the flush of the block's table IP_LOCAL_SLOTS / 256 = 1 trip.  Every wave reaches both barriers, with or without voxels.
template <int DT, bool WAVE>
__global__ void __launch_bounds__(64 * OVL_WAVES) ip_accumulate_kernel(IpDev<DT == BPX_F32 ? IP_NL_F32 : IP_NL_INT> m, const int* __restrict__ labels,
                                                                       const void* __restrict__ image, int64_t n, int n_max) {
  constexpr bool F32 = DT == BPX_F32;
  constexpr int NL = F32 ? IP_NL_F32 : IP_NL_INT;
  __shared__ int lkeys[IP_LOCAL_SLOTS];
  __shared__ unsigned lcount[IP_LOCAL_SLOTS];
  __shared__ unsigned lkmin[IP_LOCAL_SLOTS];
  __shared__ unsigned lkmax[IP_LOCAL_SLOTS];
  __shared__ long long llimbs[IP_LOCAL_SLOTS * NL];
  __shared__ unsigned lnonf[IP_LOCAL_SLOTS * 3];
  __shared__ unsigned lclaimed;
  const IpLds<NL> loc{{lkeys, &lclaimed}, lcount, lkmin, lkmax, llimbs, lnonf};
  for (int s = threadIdx.x; s < IP_LOCAL_SLOTS; s += 64 * OVL_WAVES) {
    lkeys[s] = 0;
    lcount[s] = 0;
    lkmin[s] = IP_KMIN_INIT;
    lkmax[s] = IP_KMAX_INIT;
#pragma unroll
    for (int j = 0; j < NL; ++j) llimbs[s * NL + j] = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) lnonf[s * 3 + k] = 0;
  }
  if (threadIdx.x == 0) lclaimed = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t begin = ((int64_t)blockIdx.x * OVL_WAVES + (threadIdx.x >> 6)) * OVL_SPAN;
  if (begin < n) {                                                      // the whole wave
    const int64_t end = begin + OVL_SPAN < n ? begin + OVL_SPAN : n;
    // spans start at multiples of 8192 voxels and a lane at a multiple of 4: aligned as the pointers are
    const bool lvec = lw_aligned16(labels);
    const bool ivec = ((uintptr_t)image & (F32 ? 15 : DT == BPX_U16 ? 7 : 3)) == 0;
    int v[OVL_VPL], nv[OVL_VPL] = {0, 0, 0, 0};
    uint32_t b[OVL_VPL], nb[OVL_VPL] = {0, 0, 0, 0};
    lw_load4(labels, begin + OVL_VPL * lane, end, lvec, v);
    load4_image<DT>(image, begin + OVL_VPL * lane, end, ivec, b);
    for (int64_t t = begin; t < end; t += OVL_TRIP) {
      if (t + OVL_TRIP < end) {                                         // on their way while this trip is worked on
        lw_load4(labels, t + OVL_TRIP + OVL_VPL * lane, end, lvec, nv);
        load4_image<DT>(image, t + OVL_TRIP + OVL_VPL * lane, end, ivec, nb);
      }
      int32_t lab[OVL_VPL];
      IpVoxel vx[OVL_VPL];
#pragma unroll
      for (int e = 0; e < OVL_VPL; ++e) {
        lab[e] = rp_label(v[e], n_max);                                 // 0 past the end of the span: contributes nothing
        vx[e] = ip_voxel<F32>(b[e]);
      }
      bool sent = false;
      if constexpr (WAVE) {
        const int32_t l0 = __builtin_amdgcn_readfirstlane(lab[0]);     // uniform
        if (l0 > 0) {
          IpAcc a = ip_acc(l0);
          bool ok = true;
#pragma unroll
          for (int e = 0; e < OVL_VPL; ++e) {
            ok = ok && vx[e].cls == IP_FINITE && ip_fits(a, lab[e], vx[e]);
            if (ok) ip_absorb(a, vx[e]);
          }
          if (__ballot(ok) == ~0ull) {                                  // 256 finite voxels of label l0, every lane within one limb pair
            const int32_t limb = (int32_t)wave_max((uint32_t)(a.limb + 1)) - 1;       // -1 when no lane holds a nonzero piece
            if (__ballot(a.limb < 0 || a.limb == limb) == ~0ull) {      // and the same pair in every lane
              a.count = OVL_TRIP;
              a.kmin = wave_min(a.kmin);
              a.kmax = wave_max(a.kmax);
              a.limb = limb;
              a.lo = wave_sum(a.lo);
              a.hi = wave_sum(a.hi);
              if (lane == 0) ip_emit<NL>(loc, m, a);
              sent = true;
            }
          }
        }
      }
      if (!sent) {
        IpAcc a = ip_acc(lab[0]);
#pragma unroll
        for (int e = 0; e < OVL_VPL; ++e) {
          if (!ip_fits(a, lab[e], vx[e])) { ip_emit<NL>(loc, m, a); a = ip_acc(lab[e]); }
          if (lab[e] > 0) ip_absorb(a, vx[e]);
        }
        ip_emit<NL>(loc, m, a);
      }
#pragma unroll
      for (int e = 0; e < OVL_VPL; ++e) { v[e] = nv[e]; b[e] = nb[e]; }
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < IP_LOCAL_SLOTS; s += 64 * OVL_WAVES) ip_merge<NL>(loc, (uint32_t)s, m);   // the flush: every label of the block once
}

constexpr int IP_DEFAULT_WAVE = 0;
int g_intensityprops_wave = IP_DEFAULT_WAVE;   // bpx_debug_set_intensityprops_wave: 1 = form (b), uniform trips reduced across the wave; 0 = form (a), the lane merge alone; same bits

template <int DT> void launch(const int32_t* labels_d, const void* image_d, int64_t n, int n_max, int32_t* area_d, void* min_d, void* max_d, int64_t* limbs_d,
                              int32_t* nonfinite_d, double* sum_d, double* mean_d, hipStream_t s) {
  constexpr bool F32 = DT == BPX_F32;
  constexpr int NL = F32 ? IP_NL_F32 : IP_NL_INT;
  const int64_t rows = (int64_t)n_max + 1;
  uint32_t* area = reinterpret_cast<uint32_t*>(area_d);
  uint32_t* kmin = static_cast<uint32_t*>(min_d);
  uint32_t* kmax = static_cast<uint32_t*>(max_d);
  uint32_t* nonf = reinterpret_cast<uint32_t*>(nonfinite_d);
  const IpDev<NL> m{area, kmin, kmax, reinterpret_cast<long long*>(limbs_d), nonf};
  const unsigned blocks = lw_span_blocks(n);
  ip_init_kernel<NL><<<lw_rows_grid(rows), 256, 0, s>>>(area, kmin, kmax, limbs_d, nonf, rows);
  if (g_intensityprops_wave) ip_accumulate_kernel<DT, true><<<blocks, 64 * OVL_WAVES, 0, s>>>(m, labels_d, image_d, n, n_max);
  else ip_accumulate_kernel<DT, false><<<blocks, 64 * OVL_WAVES, 0, s>>>(m, labels_d, image_d, n, n_max);
  ip_finish_kernel<NL, F32><<<lw_rows_grid(rows), 256, 0, s>>>(area, kmin, kmax, limbs_d, nonf, sum_d, mean_d, rows);
}

}  // namespace

extern "C" int bpx_debug_set_intensityprops_wave(int on) { g_intensityprops_wave = on < 0 ? IP_DEFAULT_WAVE : on ? 1 : 0; return 0; }   // negative: back to the default

extern "C" int bpx_intensity_props(const int32_t* labels_d, const void* image_d, int image_dtype, int Z, int Y, int X, int n_max, int32_t* area_d,
                                   void* min_d, void* max_d, int64_t* limbs_d, int32_t* nonfinite_d, double* sum_d, double* mean_d, bpx_stream_t stream) {
  const char* fn = "bpx_intensity_props";
  BPX_CHECK(labels_d && image_d && area_d && min_d && max_d && limbs_d && nonfinite_d && sum_d && mean_d, "%s: null pointer", fn);
  LW_CHECK_VOLUME(fn, Z, Y, X, n_max);
  BPX_CHECK(image_dtype == BPX_F32 || image_dtype == BPX_U8 || image_dtype == BPX_U16, "%s: image dtype must be BPX_F32, BPX_U8 or BPX_U16 (got %d)", fn,
            image_dtype);
  const uintptr_t esize = image_dtype == BPX_F32 ? 4 : image_dtype == BPX_U16 ? 2 : 1;
  BPX_CHECK((((uintptr_t)labels_d | (uintptr_t)area_d | (uintptr_t)min_d | (uintptr_t)max_d | (uintptr_t)nonfinite_d) & 3) == 0 &&
                (((uintptr_t)limbs_d | (uintptr_t)sum_d | (uintptr_t)mean_d) & 7) == 0 && ((uintptr_t)image_d & (esize - 1)) == 0,
            "%s: labels, area, min, max and nonfinite must be 4-byte aligned, limbs, sum and mean 8-byte aligned, the image to its element size", fn);
  hipStream_t s = (hipStream_t)stream;
  if (image_dtype == BPX_F32) launch<BPX_F32>(labels_d, image_d, n, n_max, area_d, min_d, max_d, limbs_d, nonfinite_d, sum_d, mean_d, s);
  else if (image_dtype == BPX_U16) launch<BPX_U16>(labels_d, image_d, n, n_max, area_d, min_d, max_d, limbs_d, nonfinite_d, sum_d, mean_d, s);
  else launch<BPX_U8>(labels_d, image_d, n, n_max, area_d, min_d, max_d, limbs_d, nonfinite_d, sum_d, mean_d, s);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

// The core steps on host memory, for the CPU suite: nothing is launched.
extern "C" int bpx_intensity_pieces_host(uint32_t bits, int* limb, int64_t* lo, int64_t* hi) {
  BPX_CHECK(limb && lo && hi, "bpx_intensity_pieces_host: null pointer");
  const IpVoxel v = ip_voxel_f32(bits);
  *limb = v.limb;                           // -1: NaN or an infinity, no pieces
  *lo = v.lo;
  *hi = v.hi;
  return 0;
}
extern "C" int bpx_intensity_round_host(const int64_t* limbs, int nl, double* out) {
  BPX_CHECK(limbs && out, "bpx_intensity_round_host: null pointer");
  BPX_CHECK(nl == IP_NL_F32 || nl == IP_NL_INT, "bpx_intensity_round_host: nl must be %d (float32, unit 2^-149) or %d (integers, unit 1) (got %d)", IP_NL_F32,
            IP_NL_INT, nl);
  *out = ip_f64(nl == IP_NL_F32 ? ip_round_bits<IP_NL_F32>(limbs, IP_UNIT_F32) : ip_round_bits<IP_NL_INT>(limbs, 0));
  return 0;
}
