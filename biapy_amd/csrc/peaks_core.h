// What decides a result of the local-maximum search (peaks.hip): the 64-bit key of a voxel, the passes a set of radii needs, how a lane fetches
// and stores its voxels, the windowed maximum of one lane, the final test, and the decoding of a key into value and coordinates.  Compiles for
// the device (peaks.hip) and for the host (scripts/peaks_cpu_check.cpp replays the launch sequence thread by thread with the same code under
// ASan / UBSan, against a brute-force search of every voxel's box).
//
// THE KEY of voxel v is  (k(v) << 32) | (0xFFFFFFFF - linear_index(v)),  k the order-preserving uint32 image of the value that the watershed uses
// (int32: v + 2^31; float32: the sign-flip map, -0.0 < +0.0, NaN unspecified).  A larger key is a larger value, and among equal values the
// raster-first voxel; the keys of a volume are distinct, so "the maximum of the box" names ONE voxel, and a value-only filter cannot.  No voxel
// of a volume under 2^31 voxels carries key 0 (the low word is at least 2^31): 0 is "nothing" - a voxel outside the row, an unused slot.
// THE BOX [z-rz, z+rz] x [y-ry, y+ry] x [x-rx, x+rx] is clipped to the volume and searched one axis at a time (the maximum is separable): one
// pass per axis with a nonzero radius, X then Y then Z; the first pass forms the keys from the image, the last compares each voxel's box
// maximum with its own key (formed again from the image), applies the threshold and the border margin and writes 0 / 1; the passes between
// write the running maxima as key volumes.  Every radius zero: one pass that is first and last.
// A LANE owns PEAKS_V = 4 voxels of one row from x0 = 4 * chunk: 16 bytes of the image, 32 of a key volume, fetched by 16-byte accesses where
// the address allows and by 4-byte (image) or 8-byte (keys) accesses otherwise and in the row's ragged last chunk - the same bits either way.
// Along X it fetches the chunks chunk - ceil(r / 4) .. chunk + ceil(r / 4) of its row and lets each of their voxels meet each of its four
// windows (registers only, no index that is not a constant after unrolling); along Y / Z it fetches its own chunk from the rows
// pos - r .. pos + r inside the volume.  At most 2 r + 4 (X) or 2 r + 1 (Y, Z) voxels per voxel and axis, never the box.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PEAKS_HD __host__ __device__ __forceinline__
#else
#define PEAKS_HD inline
#endif

constexpr int PEAKS_V = 4;                            // voxels per lane
constexpr int PEAKS_MAX_RADIUS = 64;
constexpr int PEAKS_AXIS_Z = 0, PEAKS_AXIS_Y = 1, PEAKS_AXIS_X = 2;

typedef uint32_t __attribute__((may_alias)) peaks_u32;                        // a voxel of either image type
typedef uint32_t __attribute__((vector_size(16), may_alias)) peaks_u32x4;      // four of them in one access
typedef uint64_t __attribute__((may_alias)) peaks_u64;
typedef uint64_t __attribute__((vector_size(16), may_alias)) peaks_u64x2;      // two keys in one access

struct PeaksChunk { uint64_t k[PEAKS_V]; };           // the keys of a lane's four voxels; 0 past the row's end

// ---- the key ------------------------------------------------------------------------------------------------------------------------------------
PEAKS_HD uint32_t peaks_okey(uint32_t bits, bool is_f32) {
  return is_f32 ? ((bits & 0x80000000u) ? ~bits : (bits | 0x80000000u)) : (bits ^ 0x80000000u);
}
PEAKS_HD uint32_t peaks_unokey(uint32_t k, bool is_f32) { return (!is_f32 || (k & 0x80000000u)) ? (k ^ 0x80000000u) : ~k; }
PEAKS_HD uint64_t peaks_key(uint32_t bits, bool is_f32, uint32_t index) { return (uint64_t)peaks_okey(bits, is_f32) << 32 | (0xFFFFFFFFu - index); }
PEAKS_HD double peaks_value(uint32_t bits, bool is_f32) {          // exact for both types
  if (is_f32) {
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return (double)f;
  }
  return (double)(int32_t)bits;
}
// a key back into the voxel's bits and coordinates
PEAKS_HD void peaks_decode(uint64_t key, bool is_f32, int Y, int X, uint32_t* bits, int* z, int* y, int* x) {
  const uint32_t index = 0xFFFFFFFFu - (uint32_t)key;
  *bits = peaks_unokey((uint32_t)(key >> 32), is_f32);
  *x = (int)(index % (uint32_t)X);
  *y = (int)(index / (uint32_t)X % (uint32_t)Y);
  *z = (int)(index / (uint32_t)X / (uint32_t)Y);
}

// ---- the passes ---------------------------------------------------------------------------------------------------------------------------------
struct PeaksStep {
  int axis, r;
  int src, dst;                                       // -1: the image (src) / the results (dst); 0, 1: the key volumes of the workspace
};
// the passes of (rz, ry, rx) on a (Z, Y, X) volume into steps[3]; returns how many (1 .. 3).  A radius along an axis of one voxel asks for nothing.
PEAKS_HD int peaks_plan(int Z, int Y, int X, int rz, int ry, int rx, PeaksStep* steps) {
  int n = 0;
  if (rx > 0 && X > 1) steps[n++] = PeaksStep{PEAKS_AXIS_X, rx, 0, 0};
  if (ry > 0 && Y > 1) steps[n++] = PeaksStep{PEAKS_AXIS_Y, ry, 0, 0};
  if (rz > 0 && Z > 1) steps[n++] = PeaksStep{PEAKS_AXIS_Z, rz, 0, 0};
  if (n == 0) steps[n++] = PeaksStep{PEAKS_AXIS_X, 0, 0, 0};
  for (int i = 0; i < n; ++i) {                       // LOOP BOUND: 3
    steps[i].src = i - 1;                             // -1, 0, 1
    steps[i].dst = i == n - 1 ? -1 : i;
  }
  return n;
}

// what one pass is told
struct PeaksPass {
  const void* img;                                    // (Z, Y, X) float32 or int32, 4-byte aligned
  const void* src;                                    // key volume read (unused by the first pass)
  void* dst;                                          // key volume written (unused by the last pass)
  uint8_t* mask;                                      // last pass: 0 / 1 per voxel, or null
  int Z, Y, X;
  int axis, r;
  int is_f32;
  int thr_none;                                       // threshold == -inf: no threshold
  double thr;
  int bz, by, bx;
};

// ---- a lane's voxels to and from memory ---------------------------------------------------------------------------------------------------------------
// The image bits of the n (1 .. 4) voxels from linear index `at`; nothing past them is touched.  LOOP BOUNDS: 4.
PEAKS_HD void peaks_load_bits(const void* img, int64_t at, int n, uint32_t* w) {
  const peaks_u32* p = static_cast<const peaks_u32*>(img) + at;
  if (n == PEAKS_V && ((uintptr_t)p & 15) == 0) {
    const peaks_u32x4 v = *reinterpret_cast<const peaks_u32x4*>(p);
    w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
    return;
  }
#pragma unroll
  for (int e = 0; e < PEAKS_V; ++e) w[e] = e < n ? p[e] : 0u;
}
PEAKS_HD PeaksChunk peaks_keys_of_image(const void* img, int64_t at, int n, bool is_f32) {
  uint32_t w[PEAKS_V];
  peaks_load_bits(img, at, n, w);
  PeaksChunk c;
#pragma unroll
  for (int e = 0; e < PEAKS_V; ++e) c.k[e] = e < n ? peaks_key(w[e], is_f32, (uint32_t)(at + e)) : 0;
  return c;
}
PEAKS_HD PeaksChunk peaks_load_keys(const void* vol, int64_t at, int n) {
  const peaks_u64* p = static_cast<const peaks_u64*>(vol) + at;
  PeaksChunk c;
  if (n == PEAKS_V && ((uintptr_t)p & 15) == 0) {
    const peaks_u64x2 a = reinterpret_cast<const peaks_u64x2*>(p)[0], b = reinterpret_cast<const peaks_u64x2*>(p)[1];
    c.k[0] = a[0]; c.k[1] = a[1]; c.k[2] = b[0]; c.k[3] = b[1];
    return c;
  }
#pragma unroll
  for (int e = 0; e < PEAKS_V; ++e) c.k[e] = e < n ? p[e] : 0;
  return c;
}
PEAKS_HD void peaks_store_keys(void* vol, int64_t at, int n, const PeaksChunk& c) {
  peaks_u64* p = static_cast<peaks_u64*>(vol) + at;
  if (n == PEAKS_V && ((uintptr_t)p & 15) == 0) {
    const peaks_u64x2 a = {c.k[0], c.k[1]}, b = {c.k[2], c.k[3]};
    reinterpret_cast<peaks_u64x2*>(p)[0] = a;
    reinterpret_cast<peaks_u64x2*>(p)[1] = b;
    return;
  }
#pragma unroll
  for (int e = 0; e < PEAKS_V; ++e)
    if (e < n) p[e] = c.k[e];
}
template <bool SRC_IMG> PEAKS_HD PeaksChunk peaks_fetch(const PeaksPass& p, int64_t at, int n) {
  if constexpr (SRC_IMG) return peaks_keys_of_image(p.img, at, n, p.is_f32 != 0);
  else return peaks_load_keys(p.src, at, n);
}

// ---- the windowed maximum of one lane ---------------------------------------------------------------------------------------------------------------
PEAKS_HD uint64_t peaks_max(uint64_t a, uint64_t b) { return b > a ? b : a; }
// Along X: the chunk `k` starts `off` voxels from the lane's own (a multiple of 4, negative to the left); its voxel j meets the window of the
// lane's voxel e when |off + j - e| <= r.  LOOP BOUNDS: 4 x 4.
PEAKS_HD void peaks_window_max(PeaksChunk& best, const PeaksChunk& k, int off, int r) {
#pragma unroll
  for (int j = 0; j < PEAKS_V; ++j)
#pragma unroll
    for (int e = 0; e < PEAKS_V; ++e) {
      const int d = off + j - e;
      if (d <= r && -d <= r) best.k[e] = peaks_max(best.k[e], k.k[j]);
    }
}
// Along Y / Z: voxel for voxel.
PEAKS_HD void peaks_column_max(PeaksChunk& best, const PeaksChunk& k) {
#pragma unroll
  for (int e = 0; e < PEAKS_V; ++e) best.k[e] = peaks_max(best.k[e], k.k[e]);
}

// ---- the final test -----------------------------------------------------------------------------------------------------------------------------
// `box` is the maximum of the keys in the voxel's box, `bits` the voxel's own value, `index` its linear index
PEAKS_HD bool peaks_test(uint64_t box, uint32_t bits, uint32_t index, const PeaksPass& p, int z, int y, int x) {
  return box == peaks_key(bits, p.is_f32 != 0, index) && (p.thr_none || peaks_value(bits, p.is_f32 != 0) > p.thr) && z >= p.bz && z < p.Z - p.bz &&
         y >= p.by && y < p.Y - p.by && x >= p.bx && x < p.X - p.bx;
}

// ---- the lane -----------------------------------------------------------------------------------------------------------------------------------
// Chunk `chunk` of row (z, y) in one pass.  Not FINAL: the running maxima go to p.dst and 0 is returned.  FINAL: bit e of the result says that
// voxel x0 + e is a peak, own[e] is then its key, and the 0 / 1 bytes go to p.mask when that is given.
// LOOP BOUNDS: 2 * ceil(r / 4) + 1 <= 33 chunks along X; 2 r + 1 <= 129 rows along Y / Z; 4 voxels.
template <bool SRC_IMG, bool FINAL>
PEAKS_HD uint32_t peaks_lane(const PeaksPass& p, int z, int y, int chunk, uint64_t* own) {
  const int x0 = chunk * PEAKS_V;
  const int n = p.X - x0 < PEAKS_V ? p.X - x0 : PEAKS_V;               // 1 .. 4 voxels inside the row
  const int64_t row = ((int64_t)z * p.Y + y) * p.X, at = row + x0;
  PeaksChunk best{{0, 0, 0, 0}};
  if (p.axis == PEAKS_AXIS_X) {
    const int reach = (p.r + PEAKS_V - 1) / PEAKS_V, chunks = (p.X + PEAKS_V - 1) / PEAKS_V;
    const int lo = chunk - reach < 0 ? 0 : chunk - reach, hi = chunk + reach > chunks - 1 ? chunks - 1 : chunk + reach;
    for (int c = lo; c <= hi; ++c) {
      const int xs = c * PEAKS_V;
      const PeaksChunk k = peaks_fetch<SRC_IMG>(p, row + xs, p.X - xs < PEAKS_V ? p.X - xs : PEAKS_V);
      peaks_window_max(best, k, xs - x0, p.r);
    }
  } else {
    const bool along_y = p.axis == PEAKS_AXIS_Y;
    const int64_t stride = along_y ? (int64_t)p.X : (int64_t)p.Y * p.X;
    const int pos = along_y ? y : z, extent = along_y ? p.Y : p.Z;
    const int lo = pos - p.r < 0 ? 0 : pos - p.r, hi = pos + p.r > extent - 1 ? extent - 1 : pos + p.r;
    for (int j = lo; j <= hi; ++j) peaks_column_max(best, peaks_fetch<SRC_IMG>(p, at + (int64_t)(j - pos) * stride, n));
  }
  if constexpr (!FINAL) {
    peaks_store_keys(p.dst, at, n, best);
    return 0;
  } else {
    uint32_t w[PEAKS_V];
    peaks_load_bits(p.img, at, n, w);
    uint32_t found = 0;
#pragma unroll
    for (int e = 0; e < PEAKS_V; ++e) {
      own[e] = 0;
      if (e < n && peaks_test(best.k[e], w[e], (uint32_t)(at + e), p, z, y, x0 + e)) {
        found |= 1u << e;
        own[e] = best.k[e];
      }
    }
    if (p.mask) {
      uint8_t* m = p.mask + at;
      if (n == PEAKS_V && ((uintptr_t)m & 3) == 0) {
        *reinterpret_cast<peaks_u32*>(m) = (found & 1u) | (found & 2u) << 7 | (found & 4u) << 14 | (found & 8u) << 21;
      } else {
#pragma unroll
        for (int e = 0; e < PEAKS_V; ++e)
          if (e < n) m[e] = (uint8_t)(found >> e & 1u);
      }
    }
    return found;
  }
}
