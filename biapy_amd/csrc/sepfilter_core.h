// What decides a result of the separable filter (sepfilter.hip): the border fold of each mode, the tile a block owns for a radius
// (sepfilter_plan), how a block stages its tile and halo (sepfilter_stage_lanes / sepfilter_stage_rows), and the per-output accumulation from a
// register window (sepfilter_window).  Compiles for the device (sepfilter.hip) and for the host (scripts/sepfilter_cpu_check.cpp runs whole
// blocks with the same text under ASan / UBSan, against a literal fold and the same-order float loop).
//
// THE RULE, along one axis of n voxels with 2 r + 1 float32 weights w[0 .. 2r]:
//     acc = w[0] * v[f(i - r)];   acc = acc + w[j] * v[f(i + j - r)]  for j = 1 .. 2r in that order;   out[i] = acc
// every * and + one IEEE float32 operation, round to nearest: no FMA (the library builds with -ffp-contract=off and nothing here calls
// fmaf), no folding of symmetric taps, no sum across lanes, denormals kept.  The first tap is a product alone, not 0 + product: -0.0 stays.
// THE BORDER f: "reflect" d c b a | a b c d (period 2 n), "mirror" d c b | a b c d (period 2 n - 2, n = 1 maps to 0), "nearest" clamps,
// "constant" answers -1 and the element is float32(cval); all fold over as many periods as r needs (an axis of 3 voxels with r = 8 is legal).
// A PASS sees the volume as (outer, n, inner): the filtered axis has n voxels `inner` elements apart.  z: (1, Z, Y X); y: (Z, Y, X); x: (Z Y, X, 1).
//   inner > 1 (z, y), "lanes": a block of 256 threads owns TA x 64 outputs, 64 consecutive elements of `inner` on the lanes (coalesced rows of
//   256 bytes) and TA = 32 G voxels of the axis; it stages the (TA + 2 r) x 64 slab, wave w the slab rows w, w + 4, ... with the fold resolved
//   once per row.  After the barrier lane l of wave w produces, for g = 0 .. G - 1, the 8 consecutive outputs 8 (4 g + w) .. + 7 of column l.
//   inner = 1 (x), "rows": a block owns 8 rows x 256 outputs; it stages 8 x (256 + 2 r) elements, consecutive along x across a wave, into
//   rows skewed by one word per 8 (element c at c + c / 8), so that the 32 threads of a row, which start 8 elements apart, read 32 banks.
// THE WINDOW: a thread holds 8 staged values in registers, adds tap j to its 8 accumulators, and replaces the one value no later tap needs by
// the next staged one: 8 + 2 r LDS reads for 8 outputs, not 8 (2 r + 1).  The slot of a value is fixed after unrolling (no register moves).
// No atomics, no workspace of its own, nothing read back; every loop runs to a constant or a launch parameter.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SEPFILTER_HD __host__ __device__ __forceinline__
#else
#define SEPFILTER_HD inline
#endif

constexpr int SEPFILTER_MAX_RADIUS = 32;              // per axis: 65 taps
constexpr int SEPFILTER_MAX_TAPS = 2 * SEPFILTER_MAX_RADIUS + 1;
constexpr int SEPFILTER_REFLECT = 0, SEPFILTER_MIRROR = 1, SEPFILTER_NEAREST = 2, SEPFILTER_CONSTANT = 3;
constexpr int SEPFILTER_THREADS = 256, SEPFILTER_WAVES = 4, SEPFILTER_LANES = 64;
constexpr int SEPFILTER_T = 8;                        // consecutive outputs of a thread along the filtered axis: the register window
constexpr int SEPFILTER_ROWS = 8, SEPFILTER_ROW_TX = 256;            // the x pass: 8 rows of 32 threads, 8 outputs each
// LDS per block.  The halo costs 2 r / TA of a pass's reads, so a larger r wants a longer tile; 40 KiB lets r = 32 stage 96 + 64 slab rows and
// keeps 4 blocks (16 waves) on the 160 KiB of a CU, and the small radii of everyday sigmas need 10 to 12 KiB (the register count then decides).
constexpr int SEPFILTER_LDS_BUDGET = 40960;

// ---- the border: index i of an axis of n voxels, any i; -1 is the constant ---------------------------------------------------------------------
SEPFILTER_HD int sepfilter_fold(int mode, int64_t i, int n) {
  if (i >= 0 && i < n) return (int)i;
  if (mode == SEPFILTER_CONSTANT) return -1;
  if (mode == SEPFILTER_NEAREST || n == 1) return i < 0 ? 0 : n - 1;
  if (mode == SEPFILTER_REFLECT) {
    const int64_t period = 2 * (int64_t)n;            // the axis and its mirror image, repeated
    int64_t r = i % period;
    if (r < 0) r += period;
    return (int)(r < n ? r : period - 1 - r);
  }
  const int64_t period = 2 * (int64_t)n - 2;          // mirror: the end voxels are not repeated
  int64_t r = i % period;
  if (r < 0) r += period;
  return (int)(r < n ? r : period - r);
}

// ---- the tile -------------------------------------------------------------------------------------------------------------------------------------
struct SepfilterPlan {
  int TA;                                             // outputs of a block along the filtered axis
  int G;                                              // lanes pass: groups of 8 outputs per thread (TA = 32 G); rows pass: 1
  int HA;                                             // TA + 2 r staged along the axis
  int pitch;                                          // rows pass: words between the staged rows (skewed); lanes pass: 64
  int lds_bytes;
};
SEPFILTER_HD int sepfilter_skew(int c) { return c + (c >> 3); }
// lanes pass: the smallest TA = 32 G that is at least twice the halo (4 r), or the largest that the budget holds; rows pass: 8 x 256.
// LOOP BOUND: 8.
SEPFILTER_HD SepfilterPlan sepfilter_plan(int r, bool rows) {
  if (rows) {
    const int ha = SEPFILTER_ROW_TX + 2 * r, pitch = sepfilter_skew(ha) + 1;
    return SepfilterPlan{SEPFILTER_ROW_TX, 1, ha, pitch, SEPFILTER_ROWS * pitch * 4};
  }
  int g = 1;
  for (; g < 8; ++g) {
    const int ta = SEPFILTER_WAVES * SEPFILTER_T * g;
    if (ta >= 4 * r) break;
    if ((ta + SEPFILTER_WAVES * SEPFILTER_T + 2 * r) * SEPFILTER_LANES * 4 > SEPFILTER_LDS_BUDGET) break;    // the next one would not fit
  }
  const int ta = SEPFILTER_WAVES * SEPFILTER_T * g;
  return SepfilterPlan{ta, g, ta + 2 * r, SEPFILTER_LANES, (ta + 2 * r) * SEPFILTER_LANES * 4};
}

// what a launch is told; the weights travel by value, so nothing is allocated, copied or read back
struct SepfilterArgs {
  const float* in;                                    // (outer, n, inner) float32
  float* out;                                         // the same, another buffer
  int64_t inner;                                      // elements between neighbours along the filtered axis
  int outer, n;
  int r, mode;
  float cval;
  int tiles_a, tiles_i;                               // block b owns tile (b / tiles_i / tiles_a, b / tiles_i % tiles_a, b % tiles_i)
  int wide;                                           // rows pass: out and the row pitch allow 16-byte stores
  SepfilterPlan p;
  float w[SEPFILTER_MAX_TAPS];
};

// ---- the window: 8 consecutive outputs from the staged values src[at(0)] .. src[at(7 + 2 r)] ------------------------------------------------------------
// at(m) = m * stride, or the skewed m + m / 8 of the rows pass (its base is a multiple of 8 elements, so base and m skew apart).
// Tap t needs v[t + k] for output k; it lives in slot (t + k) % 8.  LOOP BOUNDS: 2 r + 1 taps in chunks of 8; 8.
template <bool SKEW> SEPFILTER_HD int sepfilter_at(int m, int stride) { return SKEW ? m + (m >> 3) : m * stride; }
template <bool SKEW> SEPFILTER_HD void sepfilter_window(const float* src, int stride, const float* w, int r, float* acc) {
  constexpr int T = SEPFILTER_T;
  const int taps = 2 * r + 1;
  float win[T];
#pragma unroll
  for (int k = 0; k < T; ++k) win[k] = src[sepfilter_at<SKEW>(k, stride)];
  const float w0 = w[0];
#pragma unroll
  for (int k = 0; k < T; ++k) acc[k] = w0 * win[k];
  for (int t0 = 1; t0 < taps; t0 += T) {
#pragma unroll
    for (int s = 0; s < T; ++s) {
      const int t = t0 + s;
      if (t < taps) {                                 // the same for every lane
        win[s] = src[sepfilter_at<SKEW>(t + T - 1, stride)];         // v[t - 1] leaves slot (t - 1) % 8 = s, v[t + 7] takes it
        const float wt = w[t];
#pragma unroll
        for (int k = 0; k < T; ++k) acc[k] = acc[k] + wt * win[(k + s + 1) % T];
      }
    }
  }
}

// ---- the lanes pass (z, y): tile (o, a0, i0) --------------------------------------------------------------------------------------------------------------
// LOOP BOUNDS: HA <= 160 slab rows.
SEPFILTER_HD void sepfilter_stage_lanes(const SepfilterArgs& a, float* slab, int o, int a0, int64_t i0, int wave, int lane) {
  const int64_t i = i0 + lane;
  const bool col = i < a.inner;
  const float* base = a.in + (int64_t)o * a.n * a.inner;
  for (int h = wave; h < a.p.HA; h += SEPFILTER_WAVES) {
    const int src = sepfilter_fold(a.mode, (int64_t)a0 - a.r + h, a.n);
    float v = a.cval;
    if (!col) v = 0.f;                                // a column past the end: staged so that the slab is defined, never stored
    else if (src >= 0) v = base[(int64_t)src * a.inner + i];
    slab[h * SEPFILTER_LANES + lane] = v;
  }
}
// LOOP BOUNDS: G <= 3 groups; 8 outputs.
SEPFILTER_HD void sepfilter_lane(const SepfilterArgs& a, const float* slab, int o, int a0, int64_t i0, int wave, int lane) {
  const int64_t i = i0 + lane;
  float* base = a.out + (int64_t)o * a.n * a.inner;
  for (int g = 0; g < a.p.G; ++g) {
    const int first = SEPFILTER_T * (SEPFILTER_WAVES * g + wave);    // the group's first output within the tile
    if (a0 + first >= a.n) continue;                  // a ragged tile: the whole wave skips the group
    float acc[SEPFILTER_T];
    sepfilter_window<false>(slab + first * SEPFILTER_LANES + lane, SEPFILTER_LANES, a.w, a.r, acc);
    if (i < a.inner) {
#pragma unroll
      for (int k = 0; k < SEPFILTER_T; ++k)
        if (a0 + first + k < a.n) base[(int64_t)(a0 + first + k) * a.inner + i] = acc[k];
    }
  }
}

// ---- the rows pass (x): tile of rows row0 .. row0 + 7, outputs x0 .. x0 + 255 ----------------------------------------------------------------------------
// LOOP BOUNDS: 8 rows x (256 + 2 r) / 64 <= 5 columns per lane.
SEPFILTER_HD void sepfilter_stage_rows(const SepfilterArgs& a, float* img, int64_t row0, int x0, int wave, int lane) {
  for (int rr = wave; rr < SEPFILTER_ROWS; rr += SEPFILTER_WAVES) {
    const int64_t row = row0 + rr;
    const bool live = row < a.outer;
    const float* base = a.in + (live ? row : 0) * (int64_t)a.n;
    for (int c = lane; c < a.p.HA; c += SEPFILTER_LANES) {
      const int src = sepfilter_fold(a.mode, (int64_t)x0 - a.r + c, a.n);
      float v = a.cval;
      if (!live) v = 0.f;                             // a row past the end: staged, never stored
      else if (src >= 0) v = base[src];
      img[rr * a.p.pitch + sepfilter_skew(c)] = v;
    }
  }
}
struct __attribute__((may_alias, aligned(16))) sepfilter_f4 { float a, b, c, d; };     // one 16-byte store
// thread `tid` of the block: row tid / 32 of the tile, outputs 8 (tid % 32) .. + 7 of it
SEPFILTER_HD void sepfilter_row(const SepfilterArgs& a, const float* img, int64_t row0, int x0, int tid) {
  const int rr = tid >> 5, seg = tid & 31;
  const int64_t row = row0 + rr;
  const int x = x0 + SEPFILTER_T * seg;
  if (row >= a.outer || x >= a.n) return;
  float acc[SEPFILTER_T];
  sepfilter_window<true>(img + rr * a.p.pitch + sepfilter_skew(SEPFILTER_T * seg), 1, a.w, a.r, acc);
  float* dst = a.out + row * (int64_t)a.n + x;
  if (a.wide && x + SEPFILTER_T <= a.n) {             // 16-byte stores where out, the row length and x allow them
    sepfilter_f4* wide = reinterpret_cast<sepfilter_f4*>(dst);
    wide[0] = sepfilter_f4{acc[0], acc[1], acc[2], acc[3]};
    wide[1] = sepfilter_f4{acc[4], acc[5], acc[6], acc[7]};
  } else {
#pragma unroll
    for (int k = 0; k < SEPFILTER_T; ++k)
      if (x + k < a.n) dst[k] = acc[k];
  }
}
