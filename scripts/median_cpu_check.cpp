// Host run of the median filter of biapy_amd/csrc/median.hip: the same code (csrc/median_core.h: the keys, the per-axis index map of each border
// mode, the plan of tiles, the staging of a block's image, the selection network and the lane) against statements that know nothing of it.
//   1. the network of every instance, and the padding rule for every odd W <= 125 on the smallest instance that holds it, against
//      std::nth_element on random, constant, two-valued and all-extreme vectors;
//   2. the index maps of the three modes against a literal statement (fold the index back at the ends until it is inside / clamp / outside),
//      for extents 1 .. 9 and offsets several periods out, and at the end of an axis of 2^31 - 1 voxels;
//   3. median_plan for every admissible size triple: the image fits the LDS budget, the rows divide among the four waves, the image is the
//      tile plus its halo, and no tile with fewer staged keys per output was passed over;
//   4. whole blocks as the kernel runs them - median_stage by every (wave, lane), then median_lane by every (wave, lane) on the instance the
//      launcher picks - on tiny volumes of both dtypes, volumes smaller than the halo among them, against a brute-force sort of every window.
//      Input and output lie between poisoned guard bytes and the image is exactly lds_bytes long, so a load or store outside them stops the run.
// A development aid for finding an off-by-one before the kernel runs:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I biapy_amd/csrc scripts/median_cpu_check.cpp -o median_cpu_check
//   ./median_cpu_check
// Prints one line per part and exits nonzero on the first mismatch.  Host only: not loaded into Python, not part of the test suite.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "median_core.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

constexpr int GUARD = 32;

struct Guarded {                                      // `bytes` bytes that start `mis` bytes past a 16-byte boundary, poisoned on both sides
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

#define REQUIRE(cond, ...)            \
  do {                                \
    if (!(cond)) {                    \
      printf("FAILED: " __VA_ARGS__); \
      printf("\n");                   \
      exit(1);                        \
    }                                 \
  } while (0)

static uint32_t fbits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

// the instance of the launcher's switch, by the same rule
template <class F> static void with_instance(int WI, F&& f) {
  switch (WI) {
    case 3: f(std::integral_constant<int, 3>()); break;
    case 5: f(std::integral_constant<int, 5>()); break;
    case 7: f(std::integral_constant<int, 7>()); break;
    case 9: f(std::integral_constant<int, 9>()); break;
    case 15: f(std::integral_constant<int, 15>()); break;
    case 25: f(std::integral_constant<int, 25>()); break;
    case 27: f(std::integral_constant<int, 27>()); break;
    case 49: f(std::integral_constant<int, 49>()); break;
    case 75: f(std::integral_constant<int, 75>()); break;
    case 125: f(std::integral_constant<int, 125>()); break;
    default: REQUIRE(false, "no instance %d", WI);
  }
}

// ---- 1. the network and the padding rule ------------------------------------------------------------------------------------------------------------
static long check_network() {
  std::mt19937 rng(1234);
  long cases = 0;
  for (int i = 0; i < MEDIAN_NUM_INSTANCES; ++i) REQUIRE(median_instance(MEDIAN_INSTANCES[i]) == MEDIAN_INSTANCES[i], "instance %d", MEDIAN_INSTANCES[i]);
  for (int W = 1; W <= MEDIAN_MAX_WINDOW; W += 2) {
    const int WI = median_instance(W);
    REQUIRE(WI >= W && WI >= 3 && (WI - W) % 2 == 0, "instance of %d", W);
    for (int i = 0; i < MEDIAN_NUM_INSTANCES; ++i) REQUIRE(MEDIAN_INSTANCES[i] < W || MEDIAN_INSTANCES[i] >= WI, "instance of %d is not the smallest", W);
    for (int kind = 0; kind < 6; ++kind) {
      for (int rep = 0; rep < (kind == 0 ? 40 : 8); ++rep) {
        std::vector<uint32_t> v(W);
        const uint32_t c = rng();
        for (auto& e : v) {
          switch (kind) {
            case 0: e = rng(); break;                                            // no ties
            case 1: e = c; break;                                                // constant
            case 2: e = (rng() & 1) ? c : ~c; break;                             // two values
            case 3: e = rng() % 5; break;                                        // heavy ties
            case 4: e = (rng() & 1) ? 0u : 0xFFFFFFFFu; break;                   // the padding keys themselves
            default: e = rng() % 3 == 0 ? 0u : (rng() % 2 ? 0xFFFFFFFFu : rng()); break;
          }
        }
        std::vector<uint32_t> s(v);
        std::nth_element(s.begin(), s.begin() + W / 2, s.end());
        uint32_t got = 0;
        with_instance(WI, [&](auto wi) {
          MedianWalk w{v.data(), 0, 0, 0, 0, W, W, 1, 0, 0};                     // a window of one row of W
          got = median_select<decltype(wi)::value>(w);
        });
        REQUIRE(got == s[W / 2], "network: W %d on instance %d, kind %d: got %08x, expected %08x", W, WI, kind, got, s[W / 2]);
        ++cases;
      }
    }
  }
  return cases;
}

// ---- 2. the index maps ---------------------------------------------------------------------------------------------------------------------------------
static int literal_src(int mode, long long i, long long n) {
  if (mode == MEDIAN_CONSTANT) return i >= 0 && i < n ? (int)i : -1;
  if (mode == MEDIAN_NEAREST) return (int)(i < 0 ? 0 : i >= n ? n - 1 : i);
  while (i < 0 || i >= n) i = i < 0 ? -1 - i : 2 * n - 1 - i;                    // d c b a | a b c d | d c b a: mirror at the face that was crossed
  return (int)i;
}
static long check_maps() {
  long cases = 0;
  for (int mode = 0; mode < 3; ++mode) {
    for (int n = 1; n <= 9; ++n)
      for (int i = -5 * n - 9; i <= 6 * n + 9; ++i, ++cases)
        REQUIRE(median_src(mode, i, n) == literal_src(mode, i, n), "map: mode %d, n %d, i %d: %d != %d", mode, n, i, median_src(mode, i, n), literal_src(mode, i, n));
    const int big = 2147483647;
    for (long long i = (long long)big - 80; i <= (long long)big + 80; ++i, ++cases)
      REQUIRE(median_src(mode, i, big) == literal_src(mode, i, big), "map: mode %d at the end of 2^31 - 1 voxels, i %lld", mode, i);
    for (long long i = -80; i <= 80; ++i, ++cases) REQUIRE(median_src(mode, i, big) == literal_src(mode, i, big), "map: mode %d at the start, i %lld", mode, i);
  }
  // the example of the definition: a b c d
  const int want[12] = {3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0};
  for (int i = 0; i < 12; ++i) REQUIRE(median_src(MEDIAN_REFLECT, i - 4, 4) == want[i], "reflect is d c b a | a b c d | d c b a");
  return cases;
}

// ---- 3. the plan ---------------------------------------------------------------------------------------------------------------------------------------
static long check_plan() {
  long cases = 0;
  for (int sz = 1; sz <= MEDIAN_MAX_SIZE; sz += 2)
    for (int sy = 1; sy <= MEDIAN_MAX_SIZE; sy += 2)
      for (int sx = 1; sx <= MEDIAN_MAX_SIZE; sx += 2) {
        if (sz * sy * sx > MEDIAN_MAX_WINDOW) continue;
        const MedianPlan p = median_plan(sz, sy, sx);
        REQUIRE(p.TX == MEDIAN_TX && p.TZ >= 1 && p.TY >= 1, "plan %d %d %d: no tile", sz, sy, sx);
        REQUIRE(p.TZ * p.TY % MEDIAN_WAVES == 0 && p.R == p.TZ * p.TY / MEDIAN_WAVES && p.R >= 1 && p.R * MEDIAN_WAVES <= MEDIAN_MAX_ROWS, "plan %d %d %d: rows", sz, sy, sx);
        REQUIRE(p.HZ == p.TZ + sz - 1 && p.HY == p.TY + sy - 1 && p.HX == p.TX + sx - 1, "plan %d %d %d: halo", sz, sy, sx);
        REQUIRE(p.HX <= 2 * MEDIAN_TX, "plan %d %d %d: a lane stages two columns at most", sz, sy, sx);
        REQUIRE(p.lds_bytes == 4 * p.HZ * p.HY * p.HX && p.lds_bytes <= MEDIAN_LDS_BUDGET, "plan %d %d %d: %d bytes of LDS", sz, sy, sx, p.lds_bytes);
        REQUIRE(2 * p.lds_bytes <= 160 * 1024, "plan %d %d %d: two blocks per CU", sz, sy, sx);
        REQUIRE(sz > 1 || p.TZ == 1, "plan %d %d %d: a window of one plane owns one plane", sz, sy, sx);
        for (int tz = 1; tz <= 8; tz *= 2)                                        // no admissible tile stages fewer keys per output
          for (int ty = 1; ty <= 32; ty *= 2) {
            const long long e = (long long)(tz + sz - 1) * (ty + sy - 1) * (MEDIAN_TX + sx - 1);
            if (tz * ty % 4 || tz * ty > MEDIAN_MAX_ROWS || e * 4 > MEDIAN_LDS_BUDGET || (sz == 1 && tz > 1)) continue;
            REQUIRE(e * (p.TZ * p.TY) >= (long long)(p.lds_bytes / 4) * (tz * ty), "plan %d %d %d: tile %d x %d stages less", sz, sy, sx, tz, ty);
          }
        ++cases;
      }
  const MedianPlan p = median_plan(5, 5, 5);
  printf("  5 x 5 x 5: tile %d x %d x %d, %d keys staged for %d outputs (%.2f per output), %d bytes\n", p.TZ, p.TY, p.TX, p.lds_bytes / 4, p.TZ * p.TY * p.TX,
         p.lds_bytes / 4.0 / (p.TZ * p.TY * p.TX), p.lds_bytes);
  return cases;
}

// ---- 4. whole blocks -----------------------------------------------------------------------------------------------------------------------------------
static uint32_t draw(std::mt19937& rng, bool is_f32, int kind) {
  if (!is_f32) return kind == 0 ? rng() % 256 : kind == 1 ? rng() % 2 : rng() % 3 * 127;
  if (kind == 0) return fbits((float)(rng() % 1000003) / 977.f - 500.f);
  if (kind == 1) return fbits((float)(rng() % 4) * 0.25f);
  static const uint32_t vals[] = {0xFF800000u, 0x7F800000u, 0x80000000u, 0u, 0x00000001u, 0x80000001u, 0x7FC00000u, 0xFFC00001u, 0x3F800000u, 0xBF800000u, 0x7F7FFFFFu};
  return vals[rng() % (sizeof(vals) / sizeof(vals[0]))];
}

static void run_blocks(const MedianArgs& a) {
  const MedianPlan& p = a.p;
  const int tiles_z = (a.Z + p.TZ - 1) / p.TZ;
  std::vector<uint32_t> img(p.lds_bytes / 4);                                    // exactly the launch's LDS
  for (int b = 0; b < tiles_z * a.tiles_y * a.tiles_x; ++b) {
    const int x0 = b % a.tiles_x * p.TX, y0 = b / a.tiles_x % a.tiles_y * p.TY, z0 = b / a.tiles_x / a.tiles_y * p.TZ;
    std::fill(img.begin(), img.end(), 0xDEADBEEFu);
    for (int t = 0; t < MEDIAN_THREADS; ++t) median_stage(a, img.data(), z0, y0, x0, t >> 6, t & 63);
    with_instance(median_instance(a.W), [&](auto wi) {
      for (int t = 0; t < MEDIAN_THREADS; ++t) median_lane<decltype(wi)::value>(a, img.data(), z0, y0, x0, t >> 6, t & 63);
    });
  }
}

static long check_blocks() {
  std::mt19937 rng(99);
  long cases = 0;
  const int shapes[][3] = {{1, 1, 1}, {2, 3, 1}, {1, 2, 5}, {3, 4, 5}, {1, 9, 70}, {5, 6, 7}, {9, 5, 3}, {2, 33, 66}, {6, 1, 66}};
  const int sizes[][3] = {{1, 1, 1}, {1, 3, 3}, {3, 3, 3}, {1, 5, 5}, {5, 1, 1}, {1, 1, 15}, {3, 1, 5}, {1, 3, 7}, {3, 3, 5}, {1, 7, 7}, {15, 1, 1}, {1, 11, 11}, {5, 5, 5}};
  for (const auto& shape : shapes)
    for (const auto& size : sizes)
      for (int is_f32 = 0; is_f32 < 2; ++is_f32)
        for (int mode = 0; mode < 3; ++mode) {
          const int Z = shape[0], Y = shape[1], X = shape[2], sz = size[0], sy = size[1], sx = size[2], W = sz * sy * sx;
          const int kind = (int)(cases % 3), es = is_f32 ? 4 : 1;
          const size_t n = (size_t)Z * Y * X;
          Guarded in(n * es, is_f32 ? 4 * (int)(cases % 4) : (int)(cases % 7)), out(n * es, is_f32 ? 4 * (int)(cases % 3) : (int)(cases % 5));
          for (size_t i = 0; i < n; ++i) {
            const uint32_t v = draw(rng, is_f32, kind);
            if (is_f32) memcpy(in.p + 4 * i, &v, 4);
            else in.p[i] = (uint8_t)v;
          }
          memset(out.p, 0xA5, n * es);
          const double cval = is_f32 ? (cases % 2 ? 0.25 : 0.0) : (cases % 2 ? 255.0 : 1.0);
          MedianArgs a{};
          a.in = in.p; a.out = out.p;
          a.Z = Z; a.Y = Y; a.X = X;
          a.sz = sz; a.sy = sy; a.sx = sx;
          a.mode = mode;
          a.is_f32 = is_f32;
          a.ckey = median_cval_key(cval, is_f32);
          a.W = W;
          a.p = median_plan(sz, sy, sx);
          a.tiles_x = (X + a.p.TX - 1) / a.p.TX;
          a.tiles_y = (Y + a.p.TY - 1) / a.p.TY;
          run_blocks(a);
          // brute force: the values of the window through the literal border, their keys sorted
          const float cf = (float)cval;
          const uint32_t cbits = is_f32 ? fbits(cf) : (uint32_t)cval;
          std::vector<uint32_t> keys(W);
          for (int z = 0; z < Z; ++z)
            for (int y = 0; y < Y; ++y)
              for (int x = 0; x < X; ++x) {
                int k = 0;
                for (int dz = -(sz / 2); dz <= sz / 2; ++dz)
                  for (int dy = -(sy / 2); dy <= sy / 2; ++dy)
                    for (int dx = -(sx / 2); dx <= sx / 2; ++dx) {
                      const int zs = literal_src(mode, z + dz, Z), ys = literal_src(mode, y + dy, Y), xs = literal_src(mode, x + dx, X);
                      uint32_t bits = cbits;
                      if (zs >= 0 && ys >= 0 && xs >= 0) {
                        const size_t at = ((size_t)zs * Y + ys) * X + xs;
                        if (is_f32) memcpy(&bits, in.p + 4 * at, 4);
                        else bits = in.p[at];
                      }
                      keys[k++] = is_f32 ? ((bits & 0x80000000u) ? ~bits : (bits | 0x80000000u)) : bits;       // the key, stated again
                    }
                std::sort(keys.begin(), keys.end());
                const uint32_t key = keys[W / 2], want = is_f32 ? ((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key) : key;
                const size_t at = ((size_t)z * Y + y) * X + x;
                uint32_t got = 0;
                if (is_f32) memcpy(&got, out.p + 4 * at, 4);
                else got = out.p[at];
                REQUIRE(got == want, "blocks: %d x %d x %d, size %d %d %d, %s, mode %d at (%d, %d, %d): got %08x, expected %08x", Z, Y, X, sz, sy, sx,
                        is_f32 ? "float32" : "uint8", mode, z, y, x, got, want);
              }
          ++cases;
        }
  return cases;
}

int main() {
  printf("network: %ld vectors agree with std::nth_element\n", check_network());
  printf("index maps: %ld indices agree with the literal statement\n", check_maps());
  printf("plan: %ld size triples\n", check_plan());
  printf("blocks: %ld volumes agree with the brute-force sort\n", check_blocks());
  printf("median_cpu_check: all parts agree\n");
  return 0;
}
