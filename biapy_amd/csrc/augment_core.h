// What decides a value of the augmenter's two resampling passes (augment.hip: the affine warp; elastic.hip: the elastic deformation), apart from
// where the source coordinate comes from: the uniform map of a Philox word, the clamp of a coordinate, the border rule of an integer tap index,
// the four bilinear taps with their weights, the nearest tap, and the association of the interpolation.  Compiles for the device and for the
// host (scripts/elastic_cpu_check.cpp walks adversarial fields through elastic_voxel under ASan / UBSan and asserts every tap inside its plane).
//
// Every * + - below is one IEEE float32 operation, round to nearest: the library builds with -ffp-contract=off and nothing here calls fmaf.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/biapy_amd.h"

#if defined(__HIPCC__)
#define AUG_HD __host__ __device__ __forceinline__
#else
#define AUG_HD inline
#endif

// min(lo + u (hi - lo), hi) with u = (r >> 8) * 2^-24
AUG_HD float aug_uniform(uint32_t r, float lo, float hi) {
  const float u = (float)(r >> 8) * 5.9604644775390625e-8f;   // 2^-24, exact
  return fminf(lo + u * (hi - lo), hi);
}

// i / n for 0 <= i < 2^15 and 1 <= n <= 2^10 by one multiplication (exact: (i + 0.5) / n is at least 0.5 / n away from every integer)
AUG_HD int small_div(int i, float rcp_n) { return (int)(((float)i + 0.5f) * rcp_n); }

// a source coordinate, clamped to [-2^30, 2^30]; a NaN becomes the lower bound: every index below is finite
AUG_HD float warp_clamp(float f) { return fminf(fmaxf(f, -1073741824.f), 1073741824.f); }

// the source index of tap i on an axis of n voxels (p = max(2n - 2, 1), the reflect period); `in`: whether a constant-mode tap reads the plane
template <int MODE>
AUG_HD int warp_tap(int i, int n, int p, bool& in) {
  if constexpr (MODE == BPX_WARP_REFLECT) {
    int r = i % p;
    r += r < 0 ? p : 0;
    in = true;
    return r < n ? r : p - r;
  } else {
    in = MODE == BPX_WARP_EDGE || (unsigned)i < (unsigned)n;
    const int lo = i > 0 ? i : 0;
    return lo < n - 1 ? lo : n - 1;
  }
}

// out = top (1 - wy) + bot wy, top = v00 (1 - wx) + v01 wx, bot = v10 (1 - wx) + v11 wx
AUG_HD float warp_lerp(float v00, float v01, float v10, float v11, float wx, float wy) {
  const float ux = 1.f - wx, uy = 1.f - wy;
  const float top = v00 * ux + v01 * wx;
  const float bot = v10 * ux + v11 * wx;
  return top * uy + bot * wy;
}

// ---- the elastic deformation: what one output voxel (y, x) of a (Y, X) plane reads ------------------------------------------------------
// fy = y + alpha sy, fx = x + alpha sx, clamped; then the warp's rules.  o00 o01 o10 o11 / on: voxel indices WITHIN THE PLANE (row * X +
// column, below Y X whatever the field holds) of the bilinear taps (y0, x0) (y0, x0+1) (y0+1, x0) (y0+1, x0+1) and of the nearest voxel
// (floor(fy + 0.5), floor(fx + 0.5)); mask bits 0-3: that bilinear tap reads the plane, bit 4: the nearest one does (constant mode; else all set).
constexpr uint32_t ELASTIC_IN_NEAREST = 16u;
struct ElasticTaps {
  int o00, o01, o10, o11, on;
  float wx, wy;
  uint32_t mask;
};

template <int MODE>
AUG_HD ElasticTaps elastic_voxel(int y, int x, float alpha, float sy, float sx, int Y, int X, int py, int px) {
  const float fy = warp_clamp((float)y + alpha * sy), fx = warp_clamp((float)x + alpha * sx);
  const float fy0 = floorf(fy), fx0 = floorf(fx);
  const int y0 = (int)fy0, x0 = (int)fx0;
  bool iy0, iy1, ix0, ix1, iy, ix;
  const int ra = warp_tap<MODE>(y0, Y, py, iy0) * X, rb = warp_tap<MODE>(y0 + 1, Y, py, iy1) * X;
  const int xa = warp_tap<MODE>(x0, X, px, ix0), xb = warp_tap<MODE>(x0 + 1, X, px, ix1);
  const int yn = warp_tap<MODE>((int)floorf(fy + 0.5f), Y, py, iy), xn = warp_tap<MODE>((int)floorf(fx + 0.5f), X, px, ix);
  ElasticTaps t;
  t.o00 = ra + xa; t.o01 = ra + xb; t.o10 = rb + xa; t.o11 = rb + xb;
  t.on = yn * X + xn;
  t.wx = fx - fx0; t.wy = fy - fy0;
  t.mask = (iy0 && ix0 ? 1u : 0u) | (iy0 && ix1 ? 2u : 0u) | (iy1 && ix0 ? 4u : 0u) | (iy1 && ix1 ? 8u : 0u) | (iy && ix ? ELASTIC_IN_NEAREST : 0u);
  return t;
}
