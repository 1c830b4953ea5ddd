// What decides a result of the morphology pass (morph.hip): which rows of the 3 x 3 (x 3) neighbourhood belong to the structuring element and how
// wide each is, what an out-of-volume neighbour counts as, the byte-packed shifts of the binary path, the per-element combine of the grey paths,
// how a lane's 16 bytes are fetched and stored, and the lane itself (morph_lane).  Compiles for the device (morph.hip) and for the host
// (scripts/morph_cpu_check.cpp walks volumes lane by lane with the same code under ASan / UBSan, against a brute-force loop over the element).
//
// THE ELEMENT is scipy.ndimage.generate_binary_structure(ndim, connectivity), in closed form per row (dz, dy) of the neighbourhood, k = |dz| + |dy|:
// the row belongs to it when k <= connectivity (in 2-D only the rows with dz = 0), and contributes x - 1, x, x + 1 when k + 1 <= connectivity,
// x alone otherwise.
// THE BORDER: an out-of-volume neighbour is IGNORED (SciPy's grey filters in mode="reflect" for these elements, binary erosion with
// border_value=1, binary dilation with border_value=0), or, on the binary path only, counts as the ABSORBING value (0 for erosion, 1 for
// dilation: SciPy's border_value=0 erosion and border_value=1 dilation).  On the binary path both are one rule: such a neighbour is the byte
// morph_fill() - the identity of AND / OR when ignored, the absorbing value otherwise.  On the grey paths an out-of-volume row is skipped and an
// out-of-row x is clamped into the row: x itself always belongs to a row that x - 1 / x + 1 belong to, so the clamped neighbour adds nothing.
// A LANE owns MORPH_BYTES = 16 bytes of one row: 16 uint8 or 4 int32 / float32 voxels from x0 = chunk * V.  It fetches them from every row of the
// element by one 16-byte load where the address allows, 4-byte loads where only that is aligned, single bytes otherwise and in the row's
// ragged last chunk (the same bits either way), and the two voxels x0 - 1 and x0 + V of a wide row on their own: an overlapping load, no lane
// needs another's registers.  No atomics, no workspace; every loop runs to a constant.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MORPH_HD __host__ __device__ __forceinline__
#else
#define MORPH_HD inline
#endif

constexpr int MORPH_BYTES = 16;                       // per lane and row
constexpr int MORPH_ERODE = 0, MORPH_DILATE = 1, MORPH_BOUNDARY = 2;                       // op: the minimum, the maximum, or "they differ"
constexpr int MORPH_BINARY = 1, MORPH_ABSORB = 2, MORPH_INNER = 4, MORPH_FLAGS = 7;         // flags

typedef uint32_t __attribute__((may_alias)) morph_u32;                       // a word of voxels of any of the three types
typedef uint32_t __attribute__((vector_size(16), may_alias)) morph_u32x4;     // one 16-byte access

struct MorphChunk { uint32_t w[4]; };                 // a lane's 16 bytes of one row, little endian: byte i is w[i / 4] >> 8 (i % 4)

// ---- the row rule ------------------------------------------------------------------------------------------------------------------------------
MORPH_HD int morph_abs(int v) { return v < 0 ? -v : v; }
MORPH_HD bool morph_row_in(int ndim, int connectivity, int dz, int dy) {
  return (ndim == 3 || dz == 0) && morph_abs(dz) + morph_abs(dy) <= connectivity;
}
MORPH_HD bool morph_row_wide(int connectivity, int dz, int dy) { return morph_abs(dz) + morph_abs(dy) + 1 <= connectivity; }

// ---- the border rule of the binary path: the 0 / 1 byte an out-of-volume neighbour counts as -----------------------------------------------------
MORPH_HD uint32_t morph_fill(bool is_max, bool absorb) { return (is_max == absorb) ? 1u : 0u; }      // min: ignored 1, absorbing 0; max: ignored 0, absorbing 1

// ---- 0 / 1 bytes packed four to a word ----------------------------------------------------------------------------------------------------------
// every nonzero byte to 1: bit 7 of ((b & 0x7f) + 0x7f) | b is set exactly when b != 0, and no byte carries into the next
MORPH_HD uint32_t morph_norm01(uint32_t w) { return (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) >> 7 & 0x01010101u; }
// the voxels x - 1 (x + 1) of the four voxels of w: a byte funnel shift with the word before (after) it
MORPH_HD uint32_t morph_left(uint32_t w, uint32_t before) { return w << 8 | before >> 24; }
MORPH_HD uint32_t morph_right(uint32_t w, uint32_t after) { return w >> 8 | after << 24; }
MORPH_HD uint32_t morph_join(uint32_t a, uint32_t b, bool is_max) { return is_max ? a | b : a & b; }

// ---- the per-element combine of the grey paths (float32: equal as values; which of -0.0 / +0.0 wins and NaN are unspecified) ------------------------
template <class T> MORPH_HD T morph_pick(T a, T b, bool is_max) { return is_max ? (b > a ? b : a) : (b < a ? b : a); }
template <class T> MORPH_HD bool morph_is_background(T v, int background);
template <> MORPH_HD bool morph_is_background<uint8_t>(uint8_t v, int background) { return (int)v == background; }
template <> MORPH_HD bool morph_is_background<int32_t>(int32_t v, int background) { return v == background; }
template <> MORPH_HD bool morph_is_background<float>(float v, int background) { return v == (float)background; }

// ---- element e of a chunk ------------------------------------------------------------------------------------------------------------------------
template <class T> MORPH_HD T morph_get(const MorphChunk& c, int e);
template <> MORPH_HD uint8_t morph_get<uint8_t>(const MorphChunk& c, int e) { return (uint8_t)(c.w[e >> 2] >> 8 * (e & 3)); }
template <> MORPH_HD int32_t morph_get<int32_t>(const MorphChunk& c, int e) { return (int32_t)c.w[e]; }
template <> MORPH_HD float morph_get<float>(const MorphChunk& c, int e) {
  float f;
  __builtin_memcpy(&f, &c.w[e], 4);
  return f;
}
MORPH_HD uint32_t morph_bits(uint8_t v) { return v; }
MORPH_HD uint32_t morph_bits(int32_t v) { return (uint32_t)v; }
MORPH_HD uint32_t morph_bits(float v) {
  uint32_t u;
  __builtin_memcpy(&u, &v, 4);
  return u;
}

// ---- a lane's 16 bytes (or 4: the boundary bytes of four 4-byte voxels) to and from memory ----------------------------------------------------------
// The first `valid` of the MORPH_BYTES bytes at p, the others 0.  p .. p + valid - 1 lie inside the row; nothing else is touched.
// LOOP BOUNDS: 4 words, 16 bytes.
MORPH_HD MorphChunk morph_load(const uint8_t* p, int valid) {
  MorphChunk c{{0, 0, 0, 0}};
  const uintptr_t a = (uintptr_t)p;
  if (valid == MORPH_BYTES && (a & 15) == 0) {
    const morph_u32x4 v = *reinterpret_cast<const morph_u32x4*>(p);
    c.w[0] = v[0]; c.w[1] = v[1]; c.w[2] = v[2]; c.w[3] = v[3];
    return c;
  }
  const int words = (a & 3) == 0 ? valid >> 2 : 0;       // whole aligned words first, single bytes for the rest
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < words) c.w[i] = reinterpret_cast<const morph_u32*>(p)[i];
#pragma unroll
  for (int i = 0; i < MORPH_BYTES; ++i)
    if (i >= 4 * words && i < valid) c.w[i >> 2] |= (uint32_t)p[i] << 8 * (i & 3);
  return c;
}
// The first `valid` of the `bytes` (16 or 4) bytes of c to p.
MORPH_HD void morph_store(uint8_t* p, int bytes, int valid, const MorphChunk& c) {
  const uintptr_t a = (uintptr_t)p;
  if (bytes == MORPH_BYTES && valid == MORPH_BYTES && (a & 15) == 0) {
    const morph_u32x4 v = {c.w[0], c.w[1], c.w[2], c.w[3]};
    *reinterpret_cast<morph_u32x4*>(p) = v;
    return;
  }
  const int words = (a & 3) == 0 ? valid >> 2 : 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < words) reinterpret_cast<morph_u32*>(p)[i] = c.w[i];
#pragma unroll
  for (int i = 0; i < MORPH_BYTES; ++i)
    if (i >= 4 * words && i < valid) p[i] = (uint8_t)(c.w[i >> 2] >> 8 * (i & 3));
}

// the chunk x0 .. x0 + V - 1 of a row of X voxels; the voxels from X on read as the row's last one (clamp) or as `pad`
template <class T> MORPH_HD MorphChunk morph_load_row(const T* row, int x0, int X, bool clamp, T pad) {
  constexpr int V = MORPH_BYTES / (int)sizeof(T);
  const int n = X - x0 < V ? X - x0 : V;                 // 1 .. V voxels inside the row
  MorphChunk c = morph_load(reinterpret_cast<const uint8_t*>(row + x0), n * (int)sizeof(T));
  if (n < V) {
    const uint32_t bits = morph_bits(clamp ? row[X - 1] : pad);
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (e >= n) c.w[e * (int)sizeof(T) >> 2] |= bits << 8 * (e * (int)sizeof(T) & 3);
  }
  return c;
}
// voxel x of the row, x = -1 and x = X included: clamped into the row (clamp), or `pad`
template <class T> MORPH_HD T morph_edge(const T* row, int x, int X, bool clamp, T pad) {
  if (x >= 0 && x < X) return row[x];
  return clamp ? row[x < 0 ? 0 : X - 1] : pad;
}

// ---- the lane -----------------------------------------------------------------------------------------------------------------------------------
// Chunk `chunk` of row (z, y): the minimum (MORPH_ERODE), the maximum (MORPH_DILATE) or "they differ" (MORPH_BOUNDARY; with MORPH_INNER: and the
// voxel is not `background`) over the element, written to `out` (T, or uint8 for the boundary).  BINARY (uint8 only, erode / dilate): every
// nonzero byte is 1, the work is done on packed words and 0 / 1 is written.  LOOP BOUNDS: 9 rows, V voxels, 4 words.
template <class T, int OP, bool BINARY>
MORPH_HD void morph_lane(const T* in, void* out, int Z, int Y, int X, int ndim, int connectivity, int flags, int background, int z, int y, int chunk) {
  constexpr int V = MORPH_BYTES / (int)sizeof(T);
  constexpr bool want_min = OP != MORPH_DILATE, want_max = OP != MORPH_ERODE;
  const int x0 = chunk * V;
  const int n = X - x0 < V ? X - x0 : V;
  const int64_t at = ((int64_t)z * Y + y) * X;
  MorphChunk res;
  if constexpr (BINARY) {
    constexpr bool is_max = OP == MORPH_DILATE;
    const uint32_t fill = morph_fill(is_max, (flags & MORPH_ABSORB) != 0), fill4 = fill * 0x01010101u;
    uint32_t acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = is_max ? 0u : 0x01010101u;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz) {
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        if (!morph_row_in(ndim, connectivity, dz, dy)) continue;
        const bool wide = morph_row_wide(connectivity, dz, dy);
        const bool inside = z + dz >= 0 && z + dz < Z && y + dy >= 0 && y + dy < Y;
        MorphChunk c{{fill4, fill4, fill4, fill4}};
        uint32_t before = fill, after = fill;
        if (inside) {
          const T* row = in + at + ((int64_t)dz * Y + dy) * X;
          c = morph_load_row<T>(row, x0, X, false, (T)fill);
#pragma unroll
          for (int i = 0; i < 4; ++i) c.w[i] = morph_norm01(c.w[i]);
          if (wide) {
            before = morph_edge<T>(row, x0 - 1, X, false, (T)fill) != 0;
            after = morph_edge<T>(row, x0 + V, X, false, (T)fill) != 0;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          uint32_t m = c.w[i];
          if (wide) {
            m = morph_join(m, morph_left(c.w[i], i ? c.w[i - 1] : before << 24), is_max);
            m = morph_join(m, morph_right(c.w[i], i < 3 ? c.w[i + 1] : after), is_max);
          }
          acc[i] = morph_join(acc[i], m, is_max);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) res.w[i] = acc[i];
    morph_store(reinterpret_cast<uint8_t*>(out) + at + x0, MORPH_BYTES, n, res);
  } else {
    const MorphChunk centre = morph_load_row<T>(in + at, x0, X, true, T(0));
    T lo[V], hi[V];
#pragma unroll
    for (int e = 0; e < V; ++e) lo[e] = hi[e] = morph_get<T>(centre, e);
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz) {
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        if (!morph_row_in(ndim, connectivity, dz, dy)) continue;
        const bool wide = morph_row_wide(connectivity, dz, dy);
        if (!(z + dz >= 0 && z + dz < Z && y + dy >= 0 && y + dy < Y)) continue;          // an out-of-volume row is ignored
        if (dz == 0 && dy == 0 && !wide) continue;                                        // the centre alone: lo and hi start from it
        const T* row = in + at + ((int64_t)dz * Y + dy) * X;
        const MorphChunk c = (dz == 0 && dy == 0) ? centre : morph_load_row<T>(row, x0, X, true, T(0));
        T before = T(0), after = T(0);
        if (wide) {
          before = morph_edge<T>(row, x0 - 1, X, true, T(0));
          after = morph_edge<T>(row, x0 + V, X, true, T(0));
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const T v = morph_get<T>(c, e);
          const T l = e ? morph_get<T>(c, e ? e - 1 : 0) : before, r = e < V - 1 ? morph_get<T>(c, e < V - 1 ? e + 1 : e) : after;
          if (want_min) { lo[e] = morph_pick(lo[e], v, false); if (wide) lo[e] = morph_pick(morph_pick(lo[e], l, false), r, false); }
          if (want_max) { hi[e] = morph_pick(hi[e], v, true); if (wide) hi[e] = morph_pick(morph_pick(hi[e], l, true), r, true); }
        }
      }
    }
    res = MorphChunk{{0, 0, 0, 0}};
    if constexpr (OP == MORPH_BOUNDARY) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const bool edge = lo[e] != hi[e] && !((flags & MORPH_INNER) && morph_is_background<T>(morph_get<T>(centre, e), background));
        res.w[e >> 2] |= (edge ? 1u : 0u) << 8 * (e & 3);
      }
      morph_store(reinterpret_cast<uint8_t*>(out) + at + x0, V, n, res);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) res.w[e * (int)sizeof(T) >> 2] |= morph_bits(OP == MORPH_DILATE ? hi[e] : lo[e]) << 8 * (e * (int)sizeof(T) & 3);
      morph_store(reinterpret_cast<uint8_t*>(reinterpret_cast<T*>(out) + at + x0), MORPH_BYTES, n * (int)sizeof(T), res);
    }
  }
}
