// Host run of the separable filter of biapy_amd/csrc/sepfilter.hip: the same code (csrc/sepfilter_core.h: the border fold of each mode, the plan
// of tiles, the staging of a block's tile and halo, the register window and the lane / row that store its outputs) against statements that
// know nothing of it.
//   1. sepfilter_fold of the four modes against a literal statement (walk the index back at the ends, one step at a time, until it is inside /
//      clamp / outside), for extents 1 .. 80 and offsets of up to 32 + a tile beyond either end, and at the end of an axis of 2^31 - 1 voxels;
//   2. sepfilter_plan for every radius 0 .. 32: the slab fits the LDS budget, the tile is whole groups of 8 outputs per wave, the tile is at
//      least twice the halo unless the next larger one would not fit, the skewed rows of the x pass do not overlap;
//   3. sepfilter_window alone, both addressings, every radius, against the same-order float loop, bit for bit;
//   4. whole blocks as the kernels run them - the staging by every (wave, lane), then sepfilter_lane / sepfilter_row by every thread - for
//      every mode, radii 0 .. 32 and extents 1 .. 80 along the filtered axis, as a z, a y and an x pass (aligned and 4 bytes past alignment),
//      against the literal fold and the same-order float loop, bit for bit; values include denormals and signed zeros.  Input and output lie
//      between poisoned guard bytes and the staged image is exactly lds_bytes long, so a load or store outside them stops the run.
// A development aid for finding an off-by-one before the kernel runs:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I biapy_amd/csrc scripts/sepfilter_cpu_check.cpp -o sepfilter_cpu_check
//   ./sepfilter_cpu_check
// Prints one line per part and exits nonzero on the first mismatch.  Host only: not loaded into Python, not part of the test suite.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "sepfilter_core.h"

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
  float* f() { return reinterpret_cast<float*>(p); }
};

#define REQUIRE(cond, ...)            \
  do {                                \
    if (!(cond)) {                    \
      printf("FAILED: " __VA_ARGS__); \
      printf("\n");                   \
      exit(1);                        \
    }                                 \
  } while (0)

static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

// the literal border: step back inside, one voxel at a time
static int literal_fold(int mode, long long i, int n) {
  if (mode == SEPFILTER_CONSTANT) return (i < 0 || i >= n) ? -1 : (int)i;
  if (mode == SEPFILTER_NEAREST) return i < 0 ? 0 : (i >= n ? n - 1 : (int)i);
  if (n == 1) return 0;
  while (i < 0 || i >= n) {
    if (mode == SEPFILTER_REFLECT) i = i < 0 ? -1 - i : 2LL * n - 1 - i;       // d c b a | a b c d
    else i = i < 0 ? -i : 2LL * (n - 1) - i;                                   // d c b | a b c d
  }
  return (int)i;
}

static long long check_fold() {
  long long count = 0;
  for (int mode = 0; mode < 4; ++mode) {
    for (int n = 1; n <= 80; ++n)
      for (long long i = -400; i <= n + 400; ++i, ++count)
        REQUIRE(sepfilter_fold(mode, i, n) == literal_fold(mode, i, n), "fold mode %d n %d i %lld: %d", mode, n, i, sepfilter_fold(mode, i, n));
    const int big = 2147483647;
    for (long long d = -300; d <= 300; ++d, ++count) {
      const long long i = (long long)big - 1 + d;
      int want;
      if (i < big) want = (int)i;
      else if (mode == SEPFILTER_CONSTANT) want = -1;
      else if (mode == SEPFILTER_NEAREST) want = big - 1;
      else if (mode == SEPFILTER_REFLECT) want = (int)(2LL * big - 1 - i);
      else want = (int)(2LL * (big - 1) - i);
      REQUIRE(sepfilter_fold(mode, i, big) == want, "fold mode %d at the end of 2^31 - 1 voxels, i %lld", mode, i);
    }
  }
  return count;
}

static int check_plan() {
  int gmax = 0;
  for (int r = 0; r <= SEPFILTER_MAX_RADIUS; ++r) {
    const SepfilterPlan p = sepfilter_plan(r, false);
    REQUIRE(p.G >= 1 && p.TA == SEPFILTER_WAVES * SEPFILTER_T * p.G && p.HA == p.TA + 2 * r && p.pitch == SEPFILTER_LANES, "lanes plan r %d", r);
    REQUIRE(p.lds_bytes == p.HA * SEPFILTER_LANES * 4 && p.lds_bytes <= SEPFILTER_LDS_BUDGET, "lanes plan r %d: %d bytes", r, p.lds_bytes);
    const int next = (p.TA + SEPFILTER_WAVES * SEPFILTER_T + 2 * r) * SEPFILTER_LANES * 4;
    REQUIRE(p.TA >= 4 * r || next > SEPFILTER_LDS_BUDGET, "lanes plan r %d: a tile of %d is under twice the halo and the next one fits", r, p.TA);
    REQUIRE(p.G == 1 || p.TA - SEPFILTER_WAVES * SEPFILTER_T < 4 * r, "lanes plan r %d: a tile of %d is longer than it needs", r, p.TA);
    gmax = p.G > gmax ? p.G : gmax;
    const SepfilterPlan q = sepfilter_plan(r, true);
    REQUIRE(q.TA == SEPFILTER_ROW_TX && q.G == 1 && q.HA == q.TA + 2 * r && q.pitch > sepfilter_skew(q.HA - 1), "rows plan r %d", r);
    REQUIRE(q.lds_bytes == SEPFILTER_ROWS * q.pitch * 4 && q.lds_bytes <= SEPFILTER_LDS_BUDGET, "rows plan r %d: %d bytes", r, q.lds_bytes);
  }
  REQUIRE(gmax == 3, "the largest group count is %d", gmax);
  return SEPFILTER_MAX_RADIUS + 1;
}

static float value(std::mt19937& rng) {
  switch (rng() % 8) {
    case 0: return -0.0f;
    case 1: return 0.0f;
    case 2: { uint32_t u = (rng() % 9000) | ((rng() & 1u) << 31); float f; memcpy(&f, &u, 4); return f; }   // denormal
    case 3: return std::ldexp((float)(rng() % 2000) - 1000.f, -140);                                        // products underflow
    default: return std::ldexp((float)(int)(rng() % 200001) - 100000.f, -12);
  }
}

static void weights(std::mt19937& rng, int r, float* w) {
  for (int j = 0; j < 2 * r + 1; ++j) w[j] = std::ldexp((float)(int)(rng() % 4001) - 2000.f, -11) * (j % 3 == 0 ? 1.f : 0.37f);
}

// the rule, stated once more with nothing of the tiles
static float rule(const float* v, long long stride, int n, int i, const float* w, int r, int mode, float cval) {
  auto at = [&](int j) {
    const int s = literal_fold(mode, (long long)i + j - r, n);
    return s < 0 ? cval : v[s * stride];
  };
  float acc = w[0] * at(0);
  for (int j = 1; j <= 2 * r; ++j) acc = acc + w[j] * at(j);
  return acc;
}

static long long check_window(std::mt19937& rng) {
  long long count = 0;
  for (int r = 0; r <= SEPFILTER_MAX_RADIUS; ++r) {
    float w[SEPFILTER_MAX_TAPS];
    weights(rng, r, w);
    const int m = SEPFILTER_T + 2 * r;
    for (int skew = 0; skew < 2; ++skew) {
      const int stride = skew ? 1 : 3;
      const size_t len = skew ? (size_t)sepfilter_skew(m - 1) + 1 : (size_t)(m - 1) * stride + 1;
      Guarded g(len * 4, 0);
      std::vector<float> v(m);
      for (int i = 0; i < m; ++i) v[i] = value(rng);
      for (size_t i = 0; i < len; ++i) g.f()[i] = 12345.f;
      for (int i = 0; i < m; ++i) g.f()[skew ? sepfilter_skew(i) : i * stride] = v[i];
      float acc[SEPFILTER_T];
      if (skew) sepfilter_window<true>(g.f(), 1, w, r, acc);
      else sepfilter_window<false>(g.f(), stride, w, r, acc);
      for (int k = 0; k < SEPFILTER_T; ++k, ++count) {
        float want = w[0] * v[k];
        for (int j = 1; j <= 2 * r; ++j) want = want + w[j] * v[k + j];
        REQUIRE(bits(acc[k]) == bits(want), "window r %d skew %d output %d: %a, the loop gives %a", r, skew, k, acc[k], want);
      }
    }
  }
  return count;
}

// one pass over (outer, n, inner) as the launcher sets it up and the kernels run it
static void run_pass(const float* in, float* out, int outer, int n, long long inner, const float* w, int r, int mode, float cval) {
  SepfilterArgs a{};
  a.in = in;
  a.out = out;
  a.inner = inner;
  a.outer = outer;
  a.n = n;
  a.r = r;
  a.mode = mode;
  a.cval = cval;
  for (int j = 0; j < 2 * r + 1; ++j) a.w[j] = w[j];
  const bool rows = inner == 1;
  a.p = sepfilter_plan(r, rows);
  Guarded img((size_t)a.p.lds_bytes, 0);
  if (rows) {
    a.tiles_a = (n + SEPFILTER_ROW_TX - 1) / SEPFILTER_ROW_TX;
    a.tiles_i = 1;
    a.wide = ((uintptr_t)out & 15) == 0 && n % 4 == 0;
    const int blocks = (outer + SEPFILTER_ROWS - 1) / SEPFILTER_ROWS * a.tiles_a;
    for (int b = 0; b < blocks; ++b) {
      const int by_x = b / a.tiles_a, x0 = (b - by_x * a.tiles_a) * SEPFILTER_ROW_TX;
      const long long row0 = (long long)by_x * SEPFILTER_ROWS;
      for (int t = 0; t < SEPFILTER_THREADS; ++t) sepfilter_stage_rows(a, img.f(), row0, x0, t >> 6, t & 63);
      for (int t = 0; t < SEPFILTER_THREADS; ++t) sepfilter_row(a, img.f(), row0, x0, t);
    }
  } else {
    a.tiles_a = (n + a.p.TA - 1) / a.p.TA;
    a.tiles_i = (int)((inner + SEPFILTER_LANES - 1) / SEPFILTER_LANES);
    const int blocks = outer * a.tiles_a * a.tiles_i;
    for (int b = 0; b < blocks; ++b) {
      const int by_i = b / a.tiles_i;
      const long long i0 = (long long)(b - by_i * a.tiles_i) * SEPFILTER_LANES;
      const int o = by_i / a.tiles_a, a0 = by_i % a.tiles_a * a.p.TA;
      for (int t = 0; t < SEPFILTER_THREADS; ++t) sepfilter_stage_lanes(a, img.f(), o, a0, i0, t >> 6, t & 63);
      for (int t = 0; t < SEPFILTER_THREADS; ++t) sepfilter_lane(a, img.f(), o, a0, i0, t >> 6, t & 63);
    }
  }
}

static long long check_blocks(std::mt19937& rng) {
  long long count = 0;
  // (outer, inner) around the filtered axis: a z pass with 70 and 3 columns, a y pass of 2 planes, x passes of 3 and 9 rows
  const int shapes[5][2] = {{1, 70}, {1, 3}, {2, 65}, {3, 1}, {9, 1}};
  for (int mode = 0; mode < 4; ++mode)
    for (int r = 0; r <= SEPFILTER_MAX_RADIUS; ++r) {
      float w[SEPFILTER_MAX_TAPS];
      weights(rng, r, w);
      for (int n = 1; n <= 80; ++n)
        for (int sh = 0; sh < 5; ++sh) {
          if ((n + r + sh) % 3 != 0 && n > 12 && n != 64 && n != 80) continue;                 // a third of the long extents per shape
          const int outer = shapes[sh][0], inner = shapes[sh][1];
          const size_t vox = (size_t)outer * n * inner;
          const int mis = (n + r) % 2 ? 4 : 0;
          Guarded in(vox * 4, mis), out(vox * 4, mis);
          for (size_t i = 0; i < vox; ++i) in.f()[i] = value(rng), out.f()[i] = -777.f;
          const float cval = mode == SEPFILTER_CONSTANT ? 0.25f : 99.f;
          run_pass(in.f(), out.f(), outer, n, inner, w, r, mode, cval);
          for (int o = 0; o < outer; ++o)
            for (int i = 0; i < n; ++i)
              for (int c = 0; c < inner; ++c, ++count) {
                const float want = rule(in.f() + (size_t)o * n * inner + c, inner, n, i, w, r, mode, cval);
                const float got = out.f()[((size_t)o * n + i) * inner + c];
                REQUIRE(bits(got) == bits(want), "mode %d r %d n %d outer %d inner %d at (%d, %d, %d): %a, the rule gives %a", mode, r, n, outer, inner,
                        o, i, c, got, want);
              }
        }
    }
  // long rows: two and three tiles along x, ragged, wide and narrow stores
  for (int mode = 0; mode < 4; ++mode)
    for (int r : {0, 4, 32})
      for (int n : {256, 257, 300, 512, 700}) {
        float w[SEPFILTER_MAX_TAPS];
        weights(rng, r, w);
        const int outer = 9;
        const size_t vox = (size_t)outer * n;
        for (int mis : {0, 4}) {
          Guarded in(vox * 4, mis), out(vox * 4, mis);
          for (size_t i = 0; i < vox; ++i) in.f()[i] = value(rng), out.f()[i] = -777.f;
          run_pass(in.f(), out.f(), outer, n, 1, w, r, mode, 0.25f);
          for (int o = 0; o < outer; ++o)
            for (int i = 0; i < n; ++i, ++count) {
              const float want = rule(in.f() + (size_t)o * n, 1, n, i, w, r, mode, 0.25f);
              REQUIRE(bits(out.f()[(size_t)o * n + i]) == bits(want), "long row mode %d r %d n %d mis %d at (%d, %d)", mode, r, n, mis, o, i);
            }
        }
      }
  // a long z axis: several tiles of every group count
  for (int r : {1, 9, 20, 32}) {
    float w[SEPFILTER_MAX_TAPS];
    weights(rng, r, w);
    const int n = 301, inner = 67;
    const size_t vox = (size_t)n * inner;
    Guarded in(vox * 4, 4), out(vox * 4, 0);
    for (size_t i = 0; i < vox; ++i) in.f()[i] = value(rng), out.f()[i] = -777.f;
    run_pass(in.f(), out.f(), 1, n, inner, w, r, SEPFILTER_MIRROR, 0.f);
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < inner; ++c, ++count) {
        const float want = rule(in.f() + c, inner, n, i, w, r, SEPFILTER_MIRROR, 0.f);
        REQUIRE(bits(out.f()[(size_t)i * inner + c]) == bits(want), "long axis r %d at (%d, %d)", r, i, c);
      }
  }
  return count;
}

int main() {
  std::mt19937 rng(20261020);
  printf("1. border fold: %lld indices agree with the literal statement\n", check_fold());
  printf("2. tile plan: %d radii within the LDS budget of %d bytes\n", check_plan(), SEPFILTER_LDS_BUDGET);
  printf("3. register window: %lld outputs equal the same-order float loop bit for bit\n", check_window(rng));
  printf("4. whole blocks: %lld voxels equal the rule bit for bit\n", check_blocks(rng));
  printf("sepfilter_cpu_check: all parts passed\n");
  return 0;
}
