// Host run of the local-maximum search of biapy_amd/csrc/peaks.hip: the same code (csrc/peaks_core.h: the key, the plan of passes, the 16-byte /
// 8-byte / 4-byte loads and stores, the windowed maximum of a lane, the final test, the decoding of a key) with the launch sequence replayed
// thread by thread as the kernels run it - thread t owns chunk t % chunks of row t / chunks, pass after pass through the two key volumes of
// the workspace - against a brute-force search of every voxel's clipped box that knows nothing of passes or lanes.
// Cases, for float32 and int32: X = 1 .. 9 and one below, at and above 64 and 300; volumes of one, two, three and seven rows and planes; every
// combination of the radii 0, 1, 2, 3, 5, 8, 64 that the sizes make worthwhile, isotropic and not; images of few values (ties everywhere),
// with -0.0 / +0.0, the infinities and INT32_MIN / INT32_MAX; thresholds none, inside the range and above it; border margins 0, 1 and beyond
// half an extent; the image at 0 / 4 / 8 / 12 bytes past a 16-byte boundary, the workspace at 0 / 8, the mask at any byte.  Image, workspace,
// mask and key array lie between poisoned guard bytes, so that a load or store one byte outside them stops the run.  A development aid for
// finding an off-by-one at a row's or the volume's end before the kernel runs:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I biapy_amd/csrc scripts/peaks_cpu_check.cpp -o peaks_cpu_check
//   ./peaks_cpu_check
// Prints one line per dtype and exits nonzero on the first mismatch.  Not loaded into Python, not part of the test suite.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "peaks_core.h"

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

static uint32_t fbits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
static uint32_t draw(std::mt19937& rng, bool is_f32, int kind) {
  if (kind == 2) return is_f32 ? fbits((float)(rng() % 100000) / 7.f - 5000.f) : (uint32_t)(int32_t)(rng() % 200001 - 100000);      // few ties
  if (is_f32) {
    static const float vals[] = {-INFINITY, -3.e38f, -1.5f, -0.f, 0.f, 0.f, 0.25f, 1.f, 1.f, 2.f, 3.e38f, INFINITY};
    return fbits(kind == 0 ? vals[rng() % 12] : vals[3 + rng() % 3]);                   // kind 1: zeros of both signs
  }
  static const int32_t vals[] = {-2147483647 - 1, -7, 0, 0, 1, 1, 2, 3, 70000, 2147483647};
  return (uint32_t)(kind == 0 ? vals[rng() % 10] : vals[2 + rng() % 3]);
}

// the definition, voxel by voxel: the keys of the clipped box, compared as (value key, then raster-first index)
static void brute(const uint32_t* img, bool is_f32, int Z, int Y, int X, int rz, int ry, int rx, double thr, int bz, int by, int bx,
                  std::vector<uint8_t>& mask, std::vector<uint64_t>& keys) {
  keys.clear();
  for (int z = 0; z < Z; ++z)
    for (int y = 0; y < Y; ++y)
      for (int x = 0; x < X; ++x) {
        const size_t at = ((size_t)z * Y + y) * X + x;
        const uint32_t mine = peaks_okey(img[at], is_f32);
        bool peak = true;
        for (int zz = std::max(z - rz, 0); zz <= std::min(z + rz, Z - 1) && peak; ++zz)
          for (int yy = std::max(y - ry, 0); yy <= std::min(y + ry, Y - 1) && peak; ++yy)
            for (int xx = std::max(x - rx, 0); xx <= std::min(x + rx, X - 1); ++xx) {
              const size_t o = ((size_t)zz * Y + yy) * X + xx;
              const uint32_t other = peaks_okey(img[o], is_f32);
              if (other > mine || (other == mine && o < at)) { peak = false; break; }
            }
        double v;
        if (is_f32) { float f; memcpy(&f, &img[at], 4); v = f; } else v = (int32_t)img[at];
        if (!(thr == -INFINITY || v > thr)) peak = false;
        if (z < bz || z >= Z - bz || y < by || y >= Y - by || x < bx || x >= X - bx) peak = false;
        mask[at] = peak;
        if (peak) keys.push_back((uint64_t)mine << 32 | (0xFFFFFFFFu - (uint32_t)at));
      }
}

// the launch sequence of bpx_peak_local_max, thread by thread
template <bool SRC_IMG, bool FINAL>
static void walk(const PeaksPass& p, uint64_t* keys, int max_peaks, int* num) {
  const uint32_t chunks = (uint32_t)((p.X + PEAKS_V - 1) / PEAKS_V), total = (uint32_t)p.Z * p.Y * chunks;
  for (uint32_t t = 0; t < total; ++t) {                 // the kernel's thread t
    const uint32_t row = t / chunks;
    uint64_t own[PEAKS_V];
    const uint32_t found = peaks_lane<SRC_IMG, FINAL>(p, (int)(row / (uint32_t)p.Y), (int)(row % (uint32_t)p.Y), (int)(t - row * chunks), own);
    for (int e = 0; e < PEAKS_V; ++e)
      if (found >> e & 1u) {
        const int slot = (*num)++;
        if (keys && slot < max_peaks) keys[slot] = own[e];
      }
  }
}
static void replay(const void* img, bool is_f32, int Z, int Y, int X, int rz, int ry, int rx, double thr, int bz, int by, int bx, uint8_t* mask,
                   uint64_t* keys, int max_peaks, int* num, uint8_t* ws) {
  *num = 0;
  for (int i = 0; keys && i < max_peaks; ++i) keys[i] = 0;
  PeaksStep steps[3];
  const int passes = peaks_plan(Z, Y, X, rz, ry, rx, steps);
  PeaksPass p{};
  p.img = img; p.mask = mask; p.Z = Z; p.Y = Y; p.X = X; p.is_f32 = is_f32; p.thr_none = thr == -INFINITY; p.thr = thr; p.bz = bz; p.by = by; p.bx = bx;
  uint8_t* vol[2] = {ws, ws + (size_t)Z * Y * X * 8};
  for (int i = 0; i < passes; ++i) {
    const bool first = steps[i].src < 0, last = steps[i].dst < 0;
    p.axis = steps[i].axis; p.r = steps[i].r;
    p.src = first ? nullptr : vol[steps[i].src];
    p.dst = last ? nullptr : vol[steps[i].dst];
    if (first && last) walk<true, true>(p, keys, max_peaks, num);
    else if (first) walk<true, false>(p, keys, max_peaks, num);
    else if (last) walk<false, true>(p, keys, max_peaks, num);
    else walk<false, false>(p, keys, max_peaks, num);
  }
}

static long run_dtype(const char* name, bool is_f32) {
  std::mt19937 rng(4321);
  const int xs[] = {1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 300}, zys[][2] = {{1, 1}, {1, 3}, {2, 3}, {3, 1}, {3, 2}, {7, 7}, {1, 70}, {70, 2}};
  const int radii[][3] = {{0, 0, 0}, {1, 1, 1}, {2, 2, 2}, {1, 2, 3}, {3, 0, 0}, {0, 3, 0}, {0, 0, 3}, {0, 5, 1}, {5, 0, 2}, {8, 8, 8}, {64, 64, 64}, {0, 0, 64}, {0, 1, 4}};
  long cases = 0;
  int which = 0;
  for (int X : xs)
    for (auto& zy : zys)
      for (auto& r : radii) {
        const int Z = zy[0], Y = zy[1];
        if ((size_t)Z * Y * X > 6000 && r[0] + r[1] + r[2] > 30) continue;           // the brute-force box at radius 64 on the larger volumes
        ++which;
        const int kind = which % 3, mis = which % 4 * 4, ws_mis = which / 4 % 2 * 8, mask_mis = which * 5 % 16;
        const size_t n = (size_t)Z * Y * X;
        Guarded gimg(n * 4, mis), gws(n * 16, ws_mis), gmask(n, mask_mis);
        uint32_t* img = reinterpret_cast<uint32_t*>(gimg.p);
        for (size_t i = 0; i < n; ++i) img[i] = draw(rng, is_f32, kind);
        std::vector<uint32_t> before(img, img + n);
        const double thrs[] = {-INFINITY, 0.5, 1.e39};
        const int b = which / 3 % 3;                                                  // 0, 1, and beyond half of a small extent
        const int bz = b == 2 ? 2 : (Z > 1 ? b : 0), by = b == 2 ? 4 : b, bx = b == 2 ? 3 : b;
        const double thr = thrs[which / 2 % 3];
        std::vector<uint8_t> want(n);
        std::vector<uint64_t> want_keys;
        brute(img, is_f32, Z, Y, X, r[0], r[1], r[2], thr, bz, by, bx, want, want_keys);
        const int max_peaks = which % 5 == 0 ? std::max<int>(1, (int)want_keys.size() / 2) : (int)n;
        Guarded gkeys((size_t)max_peaks * 8, 8);
        uint64_t* keys = reinterpret_cast<uint64_t*>(gkeys.p);
        memset(gmask.p, 0xAB, n);
        memset(gws.p, 0xCD, n * 16);
        int num = -5;
        const bool with_mask = which % 7 != 0, with_keys = !with_mask || which % 2;
        replay(img, is_f32, Z, Y, X, r[0], r[1], r[2], thr, bz, by, bx, with_mask ? gmask.p : nullptr, with_keys ? keys : nullptr, max_peaks, &num, gws.p);
        bool ok = num == (int)want_keys.size() && memcmp(img, before.data(), n * 4) == 0;
        if (ok && with_mask) ok = memcmp(gmask.p, want.data(), n) == 0;
        if (ok && with_keys) {
          std::vector<uint64_t> got(keys, keys + max_peaks);
          std::sort(got.begin(), got.end(), std::greater<uint64_t>());
          std::sort(want_keys.begin(), want_keys.end(), std::greater<uint64_t>());
          if (num <= max_peaks) {
            for (int i = 0; i < max_peaks && ok; ++i) ok = got[i] == (i < num ? want_keys[i] : 0);
          } else {                                                                   // saturated: some max_peaks of the peaks, each once
            for (int i = 0; i < max_peaks && ok; ++i)
              ok = std::binary_search(want_keys.begin(), want_keys.end(), got[i], std::greater<uint64_t>()) && (i == 0 || got[i] != got[i - 1]);
          }
          for (int i = 0; i < std::min(num, max_peaks) && ok; ++i) {                  // a key decodes into its voxel
            uint32_t bits;
            int z, y, x;
            peaks_decode(got[i], is_f32, Y, X, &bits, &z, &y, &x);
            ok = z >= 0 && z < Z && y >= 0 && y < Y && x >= 0 && x < X && img[((size_t)z * Y + y) * X + x] == bits && want[((size_t)z * Y + y) * X + x];
          }
        }
        if (!ok) {
          printf("MISMATCH %s: %d x %d x %d, radii (%d, %d, %d), threshold %g, border (%d, %d, %d), values of kind %d, image %d bytes past a 16-byte "
                 "boundary: %d peaks, expected %zu\n", name, Z, Y, X, r[0], r[1], r[2], thr, bz, by, bx, kind, mis, num, want_keys.size());
          exit(1);
        }
        ++cases;
      }
  printf("%s: %ld cases agree with the brute-force search\n", name, cases);
  return cases;
}

int main() {
  // the order-preserving map and its inverse
  const float fs[] = {-INFINITY, -3.e38f, -1.f, -1.e-45f, -0.f, 0.f, 1.e-45f, 1.f, 3.e38f, INFINITY};
  for (int i = 0; i < 10; ++i) {
    if (i && !(peaks_okey(fbits(fs[i - 1]), true) < peaks_okey(fbits(fs[i]), true))) { printf("MISMATCH float order at %d\n", i); return 1; }
    if (peaks_unokey(peaks_okey(fbits(fs[i]), true), true) != fbits(fs[i])) { printf("MISMATCH float inverse at %d\n", i); return 1; }
  }
  const int32_t is[] = {-2147483647 - 1, -2, -1, 0, 1, 2147483647};
  for (int i = 0; i < 6; ++i) {
    if (i && !(peaks_okey((uint32_t)is[i - 1], false) < peaks_okey((uint32_t)is[i], false))) { printf("MISMATCH int order at %d\n", i); return 1; }
    if (peaks_unokey(peaks_okey((uint32_t)is[i], false), false) != (uint32_t)is[i]) { printf("MISMATCH int inverse at %d\n", i); return 1; }
  }
  if (peaks_key(0, false, 0x7FFFFFFEu) == 0 || peaks_key(fbits(-INFINITY), true, 0x7FFFFFFEu) == 0) { printf("MISMATCH key 0\n"); return 1; }
  // the plan: one pass per axis that has a radius and more than one voxel, the first from the image, the last into the results
  PeaksStep st[3];
  if (peaks_plan(4, 5, 6, 1, 2, 3, st) != 3 || st[0].axis != PEAKS_AXIS_X || st[0].r != 3 || st[0].src != -1 || st[0].dst != 0 || st[1].axis != PEAKS_AXIS_Y ||
      st[1].src != 0 || st[1].dst != 1 || st[2].axis != PEAKS_AXIS_Z || st[2].r != 1 || st[2].src != 1 || st[2].dst != -1 ||
      peaks_plan(4, 5, 6, 0, 0, 0, st) != 1 || st[0].r != 0 || st[0].src != -1 || st[0].dst != -1 || peaks_plan(1, 1, 300, 64, 64, 64, st) != 1 ||
      st[0].axis != PEAKS_AXIS_X || st[0].r != 64 || peaks_plan(1, 9, 9, 5, 0, 2, st) != 1 || peaks_plan(3, 9, 1, 5, 0, 2, st) != 1 || st[0].axis != PEAKS_AXIS_Z) {
    printf("MISMATCH plan\n");
    return 1;
  }
  long cases = run_dtype("float32", true) + run_dtype("int32", false);
  printf("peaks_cpu_check: all %ld cases agree\n", cases);
  return 0;
}
