// What decides a result of the median filter (median.hip): the order-preserving key of a voxel, the per-axis index map of each border mode, the
// tile a block owns for a size triple (median_plan), how a block stages its tile and halo as keys (median_stage), the selection network
// (median_select) and the lane that walks its windows through it (median_lane).  Compiles for the device (median.hip) and for the host
// (scripts/median_cpu_check.cpp runs whole blocks with the same code under ASan / UBSan, against a brute-force sort of every window).
//
// THE KEY of a voxel is an order-preserving uint32: float32 through peaks_core.h's peaks_okey (bits | 0x80000000 for a clear sign bit, ~bits
// otherwise: -0.0 < +0.0, negative-sign NaNs below -inf, positive-sign NaNs above +inf), uint8 the value itself.  The result at a voxel is the
// value whose key has rank W / 2 among the W = sz * sy * sx keys of its window, bits and all; nothing is computed, so nothing is flushed.
// THE BORDER is resolved per axis when an element is staged: "reflect" (d c b a | a b c d | d c b a, over as many periods as it takes) and
// "nearest" map an index outside the axis to one inside, "constant" answers -1 and the element is the key of cval.
// A BLOCK of 256 threads owns TZ x TY x 64 output voxels (median_plan) and stages them with their halo, (TZ + sz - 1)(TY + sy - 1)(64 + sx - 1)
// keys, into LDS: wave w takes the image's rows w, w + 4, ..., lane l the columns l and l + 64 of each, so a row's (z, y) is mapped once per
// wave and a column's x once per lane.  After the barrier lane l of wave w owns column l of the tile's rows w, w + 4, ... (TZ * TY / 4 <= 8
// outputs) and reads each window from LDS at consecutive addresses across the wave; the window's offsets are the same for every lane.
// THE SELECTION is forgetful: with m = W / 2, hold m + 2 keys, move the minimum and the maximum of the live set to its ends and drop both
// (neither can be the median: m + 1 elements lie on one side of each), take in the next window element, until none is left and one key
// remains.  Only min / max of uint32, every index a constant after unrolling.  The network is a template of the window COUNT, not of the size
// triple; MEDIAN_INSTANCES lists the counts that have one, and any other W runs on the next larger instance WI padded with (WI - W) / 2 keys
// 0x00000000 and as many 0xFFFFFFFF, which leaves the median where it was.  No atomics, no workspace; every loop runs to a constant or a
// launch parameter.
#pragma once
#include <stdint.h>

#include "peaks_core.h"                                // peaks_okey / peaks_unokey: the float32 key map, used and not copied

#if defined(__HIPCC__)
#define MEDIAN_HD __host__ __device__ __forceinline__
#else
#define MEDIAN_HD inline
#endif

constexpr int MEDIAN_MAX_SIZE = 15;                   // per axis
constexpr int MEDIAN_MAX_WINDOW = 125;                // sz * sy * sx
constexpr int MEDIAN_REFLECT = 0, MEDIAN_NEAREST = 1, MEDIAN_CONSTANT = 2;
constexpr int MEDIAN_THREADS = 256, MEDIAN_WAVES = 4, MEDIAN_TX = 64;
constexpr int MEDIAN_MAX_ROWS = 32;                   // TZ * TY: at most 8 outputs per thread
// LDS per block: the smallest tile of the flattest admissible windows (9 x 13 x 1, 11 x 11 x 1) needs 35 to 36 KiB; 4 blocks fit the
// 160 KiB of a CU, so the register count of an instance decides its occupancy (never below 2 blocks per CU)
constexpr int MEDIAN_LDS_BUDGET = 40960;
// the window counts with a network of their own; every admissible W runs on the smallest of them that is >= W
constexpr int MEDIAN_NUM_INSTANCES = 10;
constexpr int MEDIAN_INSTANCES[MEDIAN_NUM_INSTANCES] = {3, 5, 7, 9, 15, 25, 27, 49, 75, 125};

typedef uint32_t __attribute__((may_alias)) median_u32;

// ---- the key ------------------------------------------------------------------------------------------------------------------------------------
MEDIAN_HD uint32_t median_key(uint32_t bits, bool is_f32) { return is_f32 ? peaks_okey(bits, true) : bits; }
MEDIAN_HD uint32_t median_unkey(uint32_t k, bool is_f32) { return is_f32 ? peaks_unokey(k, true) : k; }
// the key of the constant border: cval as the volume's type holds it (the caller has checked that it is finite / an integer in 0..255)
MEDIAN_HD uint32_t median_cval_key(double cval, bool is_f32) {
  if (!is_f32) return (uint32_t)(int)cval;
  const float f = (float)cval;
  uint32_t bits;
  __builtin_memcpy(&bits, &f, 4);
  return median_key(bits, true);
}
MEDIAN_HD uint32_t median_load_key(const void* in, bool is_f32, int64_t at) {
  return is_f32 ? median_key(static_cast<const median_u32*>(in)[at], true) : (uint32_t) static_cast<const uint8_t*>(in)[at];
}
MEDIAN_HD void median_store_key(void* out, bool is_f32, int64_t at, uint32_t k) {
  if (is_f32) static_cast<median_u32*>(out)[at] = median_unkey(k, true);
  else static_cast<uint8_t*>(out)[at] = (uint8_t)k;
}

// ---- the border: index i of an axis of n voxels, any i --------------------------------------------------------------------------------------------
// (64-bit: a tile's halo at the end of an axis of almost 2^31 voxels lies past INT32_MAX; the division is met in border tiles only)
MEDIAN_HD int median_src(int mode, int64_t i, int n) {
  if (i >= 0 && i < n) return (int)i;
  if (mode == MEDIAN_CONSTANT) return -1;
  if (mode == MEDIAN_NEAREST) return i < 0 ? 0 : n - 1;
  const int64_t period = 2 * (int64_t)n;              // reflect: the axis and its mirror image, repeated
  int64_t r = i % period;
  if (r < 0) r += period;
  return (int)(r < n ? r : period - 1 - r);
}

// ---- the tile -------------------------------------------------------------------------------------------------------------------------------------
struct MedianPlan {
  int TZ, TY, TX;                                     // output voxels of a block
  int HZ, HY, HX;                                     // the staged image: tile plus halo
  int R;                                              // outputs per thread: TZ * TY / 4
  int lds_bytes;
};
// Of the tiles TZ x TY x 64 with TZ in 1, 2, 4, 8, TY in 1 .. 32 (powers of two), TZ * TY a multiple of 4 and at most 32, whose image fits the
// budget: the one that stages the fewest keys per output, among equals the smallest.  A window of one plane gets a tile of one plane.
// LOOP BOUNDS: 4 x 6.
MEDIAN_HD MedianPlan median_plan(int sz, int sy, int sx) {
  MedianPlan best{0, 0, MEDIAN_TX, 0, 0, 0, 0, 0};
  int64_t best_elems = 0, best_rows = 0;
  for (int tz = 1; tz <= 8; tz *= 2) {
    if (sz == 1 && tz > 1) break;
    for (int ty = 1; ty <= 32; ty *= 2) {
      const int rows = tz * ty;
      if (rows % MEDIAN_WAVES != 0 || rows > MEDIAN_MAX_ROWS) continue;
      const int64_t elems = (int64_t)(tz + sz - 1) * (ty + sy - 1) * (MEDIAN_TX + sx - 1);
      if (elems * 4 > MEDIAN_LDS_BUDGET) continue;
      if (best_rows == 0 || elems * best_rows < best_elems * rows) {       // elems / rows < best_elems / best_rows
        best = MedianPlan{tz, ty, MEDIAN_TX, tz + sz - 1, ty + sy - 1, MEDIAN_TX + sx - 1, rows / MEDIAN_WAVES, (int)elems * 4};
        best_elems = elems;
        best_rows = rows;
      }
    }
  }
  return best;
}
// the smallest instance that holds W keys (W <= MEDIAN_MAX_WINDOW).  LOOP BOUND: 10.
MEDIAN_HD int median_instance(int W) {
  for (int i = 0; i < MEDIAN_NUM_INSTANCES; ++i)
    if (MEDIAN_INSTANCES[i] >= W) return MEDIAN_INSTANCES[i];
  return 0;
}

// what a launch is told
struct MedianArgs {
  const void* in;                                     // (Z, Y, X) float32 or uint8
  void* out;                                          // the same
  int Z, Y, X;
  int sz, sy, sx;
  int mode;
  int is_f32;
  uint32_t ckey;                                      // median_cval_key
  int W;                                              // sz * sy * sx
  int tiles_y, tiles_x;                               // block b owns tile (b / tiles_x / tiles_y, b / tiles_x % tiles_y, b % tiles_x)
  MedianPlan p;
};

// ---- staging: rows wave, wave + 4, ... and columns lane, lane + 64 of the image of the tile at (z0, y0, x0) ----------------------------------------------
// LOOP BOUNDS: HZ * HY <= 128 rows; 2 columns.
MEDIAN_HD void median_stage(const MedianArgs& a, uint32_t* img, int z0, int y0, int x0, int wave, int lane) {
  const MedianPlan& p = a.p;
  const bool is_f32 = a.is_f32 != 0;
  int xs[2];                                          // the source x of the lane's columns: -1 is the constant, -2 no such column
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int hx = lane + MEDIAN_TX * c;
    xs[c] = hx < p.HX ? median_src(a.mode, (int64_t)x0 - a.sx / 2 + hx, a.X) : -2;
  }
  const int rows = p.HZ * p.HY;
  for (int r = wave; r < rows; r += MEDIAN_WAVES) {
    const int hz = r / p.HY, hy = r - hz * p.HY;
    const int zs = median_src(a.mode, (int64_t)z0 - a.sz / 2 + hz, a.Z), ys = median_src(a.mode, (int64_t)y0 - a.sy / 2 + hy, a.Y);
    const bool row_in = zs >= 0 && ys >= 0;
    const int64_t base = row_in ? ((int64_t)zs * a.Y + ys) * a.X : 0;
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if (xs[c] != -2) img[r * p.HX + lane + MEDIAN_TX * c] = (row_in && xs[c] >= 0) ? median_load_key(a.in, is_f32, base + xs[c]) : a.ckey;
  }
}

// ---- the window of one output, element by element ---------------------------------------------------------------------------------------------------
struct MedianWalk {
  const uint32_t* p;                                  // the lane's column of the image
  int off;                                            // the next element's offset: the same for every lane
  int i, dx, dy;
  int W, sx, sy, row_skip, plane_skip;
};
MEDIAN_HD MedianWalk median_walk(const MedianArgs& a, const uint32_t* column, int first) {
  return MedianWalk{column, first, 0, 0, 0, a.W, a.sx, a.sy, a.p.HX - a.sx, (a.p.HY - a.sy) * a.p.HX};
}
// element i of the window in raster order, then the padding keys of an instance larger than the window: 0, 0xFFFFFFFF, 0, ...
MEDIAN_HD uint32_t median_next(MedianWalk& w) {
  const bool real = w.i < w.W;
  const uint32_t v = w.p[real ? w.off : 0];
  const uint32_t k = real ? v : (((w.i - w.W) & 1) ? 0xFFFFFFFFu : 0u);
  ++w.i;
  ++w.off;
  if (++w.dx == w.sx) {
    w.dx = 0;
    w.off += w.row_skip;
    if (++w.dy == w.sy) {
      w.dy = 0;
      w.off += w.plane_skip;
    }
  }
  return k;
}

// ---- the network ---------------------------------------------------------------------------------------------------------------------------------
MEDIAN_HD void median_cx(uint32_t& lo, uint32_t& hi) {
  const uint32_t a = lo < hi ? lo : hi, b = lo < hi ? hi : lo;
  lo = a;
  hi = b;
}
// the minimum of a[0 .. N-1] to a[0], the maximum to a[N-1], the multiset kept: pair i with N-1-i (the minimum is then in the lower half or
// the middle, the maximum in the upper half or the middle), then one chain each.  3 N / 2 exchanges.  LOOP BOUNDS: N.
template <int N> MEDIAN_HD void median_ends(uint32_t* a) {
#pragma unroll
  for (int i = 0; i < N / 2; ++i) median_cx(a[i], a[N - 1 - i]);
#pragma unroll
  for (int i = 1; i < (N + 1) / 2; ++i) median_cx(a[0], a[i]);
#pragma unroll
  for (int i = N / 2; i < N - 1; ++i) median_cx(a[i], a[N - 1]);
}
// a live set of N keys in a[0 .. N-1] with N - 3 window elements still to come: drop both ends, take the next element into a[0]
template <int N> MEDIAN_HD uint32_t median_shrink(uint32_t* a, MedianWalk& w) {
  median_ends<N>(a);
  if constexpr (N == 3) {
    return a[1];
  } else {
    a[0] = median_next(w);
    return median_shrink<N - 1>(a, w);
  }
}
// the key of rank WI / 2 among the next WI keys of the walk
template <int WI> MEDIAN_HD uint32_t median_select(MedianWalk& w) {
  static_assert(WI >= 3 && WI % 2 == 1 && WI <= MEDIAN_MAX_WINDOW, "an odd window count");
  constexpr int N = WI / 2 + 2;
  uint32_t a[N];
#pragma unroll
  for (int i = 0; i < N; ++i) a[i] = median_next(w);
  return median_shrink<N>(a, w);
}

// ---- the lane: column `lane` of the tile's rows wave, wave + 4, ... ----------------------------------------------------------------------------------------
// LOOP BOUND: R <= 8 outputs.
template <int WI> MEDIAN_HD void median_lane(const MedianArgs& a, const uint32_t* img, int z0, int y0, int x0, int wave, int lane) {
  const MedianPlan& p = a.p;
  const int x = x0 + lane;
  for (int j = 0; j < p.R; ++j) {
    const int row = wave + MEDIAN_WAVES * j;
    const int tz = row / p.TY, ty = row - tz * p.TY;
    const int z = z0 + tz, y = y0 + ty;
    if (z >= a.Z || y >= a.Y) continue;               // a ragged tile: the whole wave skips the row
    MedianWalk w = median_walk(a, img + lane, (tz * p.HY + ty) * p.HX);
    const uint32_t k = median_select<WI>(w);
    if (x < a.X) median_store_key(a.out, a.is_f32 != 0, ((int64_t)z * a.Y + y) * a.X + x, k);
  }
}
