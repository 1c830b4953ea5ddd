// Host run of the morphology pass of biapy_amd/csrc/morph.hip: the same code (csrc/morph_core.h: the row rule, the border rule, the byte-packed
// shifts, the per-element combine, the 16-byte / 4-byte / single-byte loads and stores, and the lane itself, morph_lane) walked lane by lane as
// the kernel's threads do - thread t owns chunk t % chunks of row t / chunks - against a brute-force loop over the structuring element in its
// textbook form (|dz| + |dy| + |dx| <= connectivity, dz = 0 in 2-D), which knows nothing of rows.
// Cases, for uint8, int32 and float32: X = 1, 2 and one below, at and above the lane span (16 voxels of uint8, 4 of the 4-byte types) and the
// wave span (1024 / 256); volumes of one, two and three rows and planes, axes of one voxel; every base misalignment of the input (0..15 bytes for
// uint8, 0 / 4 / 8 / 12 for the 4-byte types) with another one for the output; connectivity 1..3 in 3-D and 1..2 in 2-D; erode, dilate, boundary
// and inner boundary, and on uint8 the binary path under both border rules.  Input and output lie between poisoned guard bytes, so that a load or
// store one byte outside the volume stops the run.  A development aid for finding an off-by-one at a row's or the volume's end before the
// kernel runs:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I biapy_amd/csrc scripts/morph_cpu_check.cpp -o morph_cpu_check
//   ./morph_cpu_check
// Prints one line per dtype and exits nonzero on the first mismatch.  Not loaded into Python, not part of the test suite.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "morph_core.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

constexpr int GUARD = 32;

// `bytes` bytes that start `mis` bytes past a 16-byte boundary, poisoned on both sides
struct Guarded {
  uint8_t* raw;
  uint8_t* p;
  size_t total;
  Guarded(size_t bytes, int mis) : total(GUARD + 16 + bytes + GUARD) {
    raw = static_cast<uint8_t*>(aligned_alloc(16, (total + 15) / 16 * 16));
    p = raw + GUARD + mis;
    POISON(raw, p - raw);
    POISON(p + bytes, raw + total - (p + bytes));
  }
  ~Guarded() {
    UNPOISON(raw, total);
    free(raw);
  }
};

template <class T> static T draw(std::mt19937& rng, int kind);
template <> uint8_t draw<uint8_t>(std::mt19937& rng, int kind) {
  static const uint8_t vals[] = {0, 1, 2, 128, 255};
  const unsigned r = rng() % 100;
  if (kind == 0) return r < 40 ? 0 : vals[1 + rng() % 4];          // a mask with other nonzero bytes than 1
  return r < 30 ? 0 : (uint8_t)(1 + rng() % 3);                     // few labels, so that neighbours tie and differ
}
template <> int32_t draw<int32_t>(std::mt19937& rng, int) {
  static const int32_t vals[] = {-2147483647 - 1, -7, 0, 0, 1, 2, 3, 70000, 2147483647};
  return vals[rng() % 9];
}
template <> float draw<float>(std::mt19937& rng, int) {
  static const float vals[] = {-3.e38f, -1.5f, 0.f, 0.f, 0.25f, 1.f, 2.f, 3.e38f};
  return vals[rng() % 8];
}

// the element in its textbook form, voxel by voxel
template <class T>
static void brute(const T* in, uint8_t* out_bytes, int Z, int Y, int X, int ndim, int conn, int op, int flags, int background) {
  const bool binary = flags & MORPH_BINARY, absorb = flags & MORPH_ABSORB;
  for (int z = 0; z < Z; ++z)
    for (int y = 0; y < Y; ++y)
      for (int x = 0; x < X; ++x) {
        const size_t at = ((size_t)z * Y + y) * X + x;
        const T centre = binary ? (T)(in[at] != 0) : in[at];
        T lo = centre, hi = centre;
        for (int dz = -1; dz <= 1; ++dz)
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              if (abs(dz) + abs(dy) + abs(dx) > conn || (ndim == 2 && dz != 0)) continue;
              const int zz = z + dz, yy = y + dy, xx = x + dx;
              T v;
              if (zz < 0 || zz >= Z || yy < 0 || yy >= Y || xx < 0 || xx >= X) {
                if (!absorb) continue;
                v = (T)(op == MORPH_DILATE ? 1 : 0);
              } else {
                v = in[((size_t)zz * Y + yy) * X + xx];
                if (binary) v = (T)(v != 0);
              }
              if (v < lo) lo = v;
              if (v > hi) hi = v;
            }
        if (op == MORPH_BOUNDARY) {
          bool is_bg;
          if constexpr (sizeof(T) == 1) is_bg = (int)centre == background;
          else is_bg = centre == (T)background;
          out_bytes[at] = lo != hi && !((flags & MORPH_INNER) && is_bg);
        } else {
          const T r = op == MORPH_DILATE ? hi : lo;
          memcpy(out_bytes + at * sizeof(T), &r, sizeof(T));
        }
      }
}

template <class T, int OP, bool BINARY>
static void walk(const T* in, void* out, int Z, int Y, int X, int ndim, int conn, int flags, int background) {
  constexpr int V = MORPH_BYTES / (int)sizeof(T);
  const uint32_t chunks = (uint32_t)((X + V - 1) / V), total = (uint32_t)Z * Y * chunks;
  for (uint32_t t = 0; t < total; ++t) {                 // the kernel's thread t
    const uint32_t row = t / chunks;
    morph_lane<T, OP, BINARY>(in, out, Z, Y, X, ndim, conn, flags, background, (int)(row / (uint32_t)Y), (int)(row % (uint32_t)Y), (int)(t - row * chunks));
  }
}

template <class T> static void lanes(const T* in, void* out, int Z, int Y, int X, int ndim, int conn, int op, int flags, int background) {
  if constexpr (sizeof(T) == 1) {
    if (flags & MORPH_BINARY) {
      if (op == MORPH_ERODE) walk<T, MORPH_ERODE, true>(in, out, Z, Y, X, ndim, conn, flags, background);
      else walk<T, MORPH_DILATE, true>(in, out, Z, Y, X, ndim, conn, flags, background);
      return;
    }
  }
  if (op == MORPH_ERODE) walk<T, MORPH_ERODE, false>(in, out, Z, Y, X, ndim, conn, flags, background);
  else if (op == MORPH_DILATE) walk<T, MORPH_DILATE, false>(in, out, Z, Y, X, ndim, conn, flags, background);
  else walk<T, MORPH_BOUNDARY, false>(in, out, Z, Y, X, ndim, conn, flags, background);
}

struct Mode { int op, flags; };

template <class T> static long run_dtype(const char* name) {
  constexpr int V = MORPH_BYTES / (int)sizeof(T);
  std::mt19937 rng(1234);
  std::vector<Mode> modes = {{MORPH_ERODE, 0}, {MORPH_DILATE, 0}, {MORPH_BOUNDARY, 0}, {MORPH_BOUNDARY, MORPH_INNER}};
  if (sizeof(T) == 1)
    for (int op : {MORPH_ERODE, MORPH_DILATE})
      for (int f : {MORPH_BINARY, MORPH_BINARY | MORPH_ABSORB}) modes.push_back({op, f});
  const int small_x[] = {1, 2, V - 1, V, V + 1, 2 * V + 1}, big_x[] = {64 * V - 1, 64 * V, 64 * V + 1};
  const int small_zy[][2] = {{1, 1}, {1, 3}, {2, 3}, {3, 1}, {3, 2}, {3, 3}}, big_zy[][2] = {{1, 2}, {2, 3}};
  long cases = 0;
  for (int big = 0; big < 2; ++big)
    for (int xi = 0; xi < (big ? 3 : 6); ++xi)
      for (int zi = 0; zi < (big ? 2 : 6); ++zi)
        for (int mis = 0; mis < 16; mis += (int)sizeof(T)) {
          if (big && sizeof(T) == 1 && !(mis == 0 || mis == 1 || mis == 3 || mis == 4 || mis == 8 || mis == 12 || mis == 15)) continue;
          const int X = big ? big_x[xi] : small_x[xi], Z = big ? big_zy[zi][0] : small_zy[zi][0], Y = big ? big_zy[zi][1] : small_zy[zi][1];
          const size_t n = (size_t)Z * Y * X;
          for (int ndim = 2; ndim <= 3; ++ndim) {
            if (ndim == 2 && Z != 1) continue;
            for (int conn = 1; conn <= ndim; ++conn)
              for (const Mode& m : modes) {
                const bool boundary = m.op == MORPH_BOUNDARY;
                const size_t out_es = boundary ? 1 : sizeof(T);
                const int out_mis = out_es == 1 ? (mis * 5 + 3) & 15 : (mis + 4) & 15;
                Guarded gin(n * sizeof(T), mis), gout(n * out_es, out_mis);
                T* in = reinterpret_cast<T*>(gin.p);
                for (size_t i = 0; i < n; ++i) in[i] = draw<T>(rng, (m.flags & MORPH_BINARY) ? 0 : 1);
                memset(gout.p, 0xAB, n * out_es);
                const int background = boundary ? (int)(rng() % 3) : 0;
                std::vector<uint8_t> want(n * out_es);
                brute<T>(in, want.data(), Z, Y, X, ndim, conn, m.op, m.flags, background);
                lanes<T>(in, gout.p, Z, Y, X, ndim, conn, m.op, m.flags, background);
                if (memcmp(gout.p, want.data(), n * out_es) != 0) {
                  size_t i = 0;
                  while (gout.p[i] == want[i]) ++i;
                  printf("MISMATCH %s: %d x %d x %d, ndim %d, connectivity %d, op %d, flags %d, input %d and output %d bytes past a 16-byte boundary: "
                         "byte %zu is %d, expected %d\n", name, Z, Y, X, ndim, conn, m.op, m.flags, mis, out_mis, i, gout.p[i], want[i]);
                  exit(1);
                }
                ++cases;
              }
          }
        }
  printf("%s: %ld cases agree with the brute-force loop\n", name, cases);
  return cases;
}

int main() {
  // the packed helpers on every byte value and on the carries between bytes
  for (uint32_t b = 0; b < 256; ++b)
    for (int k = 0; k < 4; ++k) {
      const uint32_t w = b << 8 * k | 0xff000000u >> 8 * k;
      uint32_t want = 0;
      for (int j = 0; j < 4; ++j) want |= (uint32_t)((w >> 8 * j & 0xff) != 0) << 8 * j;
      if (morph_norm01(w) != want) { printf("MISMATCH morph_norm01(%08x)\n", w); return 1; }
    }
  if (morph_left(0x04030201u, 0xaa000000u) != 0x030201aau || morph_right(0x04030201u, 0x000000bbu) != 0xbb040302u) { printf("MISMATCH byte shifts\n"); return 1; }
  long cases = run_dtype<uint8_t>("uint8") + run_dtype<int32_t>("int32") + run_dtype<float>("float32");
  printf("morph_cpu_check: all %ld cases agree\n", cases);
  return 0;
}
