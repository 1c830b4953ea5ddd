// Host run of the per-voxel arithmetic of the elastic deformation (biapy_amd/csrc/elastic.hip): the same code (csrc/augment_core.h:
// elastic_voxel - coordinate, clamp, border rule of every tap, weights - and warp_lerp) over adversarial fields, against statements that know
// nothing of it.
//   1. warp_tap of the three modes against a literal statement (walk the index back from the ends one step at a time / clamp / outside), for
//      extents 1 .. 40 and indices of several periods beyond either end, and at +-2^30 and +-(2^30 + 1);
//   2. elastic_voxel, every mode, planes 1 x 1 .. 37 x 41: for every voxel and every (alpha, displacement) of a list that holds zeros, exact
//      half-integers, several extents, +-1e30, +-inf, NaN, denormals and +-FLT_MAX, every tap index is inside [0, Y X) and the weights are in
//      [0, 1]; the gather then reads a plane that lies between poisoned guard bytes through those indices (ASan stops a load outside), and
//      the result is finite for a finite plane;
//   3. a constant integer displacement is an exact shift (weights 0, the tap of the literal fold) and alpha = 0 the identity.
// A development aid for finding an index out of range before the kernel runs:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I biapy_amd/csrc scripts/elastic_cpu_check.cpp -o elastic_cpu_check
//   ./elastic_cpu_check
// Prints one line per part and exits nonzero on the first mismatch.  Host only: not loaded into Python, not part of the test suite.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "augment_core.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

#define REQUIRE(cond, ...)            \
  do {                                \
    if (!(cond)) {                    \
      printf("FAILED: " __VA_ARGS__); \
      printf("\n");                   \
      exit(1);                        \
    }                                 \
  } while (0)

constexpr int GUARD = 64;

// the border rule, literally: -1 = a constant-mode tap outside
static int literal_tap(int mode, long long i, int n) {
  if (mode == BPX_WARP_CONSTANT) return i >= 0 && i < n ? (int)i : -1;
  if (mode == BPX_WARP_EDGE) return i < 0 ? 0 : i >= n ? n - 1 : (int)i;
  if (n == 1) return 0;
  const long long p = 2LL * n - 2;
  i = ((i % p) + p) % p;                               // d c b | a b c d | c b a: position within the period
  return (int)(i < n ? i : p - i);
}

template <int MODE>
static void check_taps() {
  long long checked = 0;
  for (int n = 1; n <= 40; ++n) {
    const int p = 2 * n - 2 > 1 ? 2 * n - 2 : 1;
    std::vector<long long> idx;
    for (long long i = -5LL * p - 3; i <= n + 5LL * p + 3; ++i) idx.push_back(i);
    for (long long i : {-(1LL << 30) - 1, -(1LL << 30), (1LL << 30), (1LL << 30) + 1}) idx.push_back(i);
    for (long long i : idx) {
      bool in = false;
      const int got = warp_tap<MODE>((int)i, n, p, in);
      const int want = literal_tap(MODE, i, n);
      REQUIRE(got >= 0 && got < n, "warp_tap<%d>(%lld, %d) = %d leaves the axis", MODE, i, n, got);
      if (want < 0) REQUIRE(!in, "warp_tap<%d>(%lld, %d): a tap outside reads the plane", MODE, i, n);
      else REQUIRE(in && got == want, "warp_tap<%d>(%lld, %d) = %d, the literal rule gives %d", MODE, i, n, got, want);
      ++checked;
    }
  }
  printf("1. warp_tap<%d>: %lld indices equal the literal rule\n", MODE, checked);
}

static std::vector<float> adversarial() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  return {0.f, -0.f, 0.5f, -0.5f, 1.5f, -2.5f, 0.25f, 0.49999997f, 0.50000006f, 1.f, -1.f, 3.f, -7.f, 40.f, -41.f, 123.f, -150.75f, 1e5f, -1e5f,
          1073741824.f, -1073741824.f, 1073741952.f, 2147483648.f, -2147483648.f, 4294967296.f, 1e30f, -1e30f, FLT_MAX, -FLT_MAX, inf, -inf, nan,
          1e-40f, -1e-40f, FLT_MIN};
}

template <int MODE>
static void check_voxels() {
  const std::vector<float> vals = adversarial();
  const std::vector<float> alphas = {0.f, 1.f, 12.5f, 1024.f, -3.f, 1e30f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
  const int planes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {5, 3}, {24, 20}, {37, 41}};
  long long checked = 0;
  for (const auto& pl : planes) {
    const int Y = pl[0], X = pl[1], py = 2 * Y - 2 > 1 ? 2 * Y - 2 : 1, px = 2 * X - 2 > 1 ? 2 * X - 2 : 1;
    const size_t bytes = (size_t)Y * X * sizeof(float), total = GUARD + bytes + GUARD;
    uint8_t* raw = static_cast<uint8_t*>(aligned_alloc(16, (total + 15) / 16 * 16));
    float* plane = reinterpret_cast<float*>(raw + GUARD);
    for (int i = 0; i < Y * X; ++i) plane[i] = (float)(i % 13) - 6.f;
    POISON(raw, GUARD);
    POISON(raw + GUARD + bytes, GUARD);
    for (int y = 0; y < Y; ++y)
      for (int x = 0; x < X; ++x)
        for (float alpha : alphas)
          for (float sy : vals)
            for (float sx : vals) {
              const ElasticTaps t = elastic_voxel<MODE>(y, x, alpha, sy, sx, Y, X, py, px);
              for (int o : {t.o00, t.o01, t.o10, t.o11, t.on})
                REQUIRE(o >= 0 && o < Y * X, "elastic_voxel<%d>(%d, %d, alpha %g, s (%g, %g)) on %d x %d: tap %d outside the plane", MODE, y, x, alpha, sy, sx, Y, X, o);
              REQUIRE(t.wx >= 0.f && t.wx <= 1.f && t.wy >= 0.f && t.wy <= 1.f, "weights (%g, %g) outside [0, 1]", t.wx, t.wy);
              if (MODE != BPX_WARP_CONSTANT) REQUIRE(t.mask == 31u, "mask %u: every tap of this mode reads the plane", t.mask);
              float v00 = plane[t.o00], v01 = plane[t.o01], v10 = plane[t.o10], v11 = plane[t.o11];      // ASan: inside the guards
              if (MODE == BPX_WARP_CONSTANT) {
                v00 = t.mask & 1u ? v00 : 0.75f; v01 = t.mask & 2u ? v01 : 0.75f; v10 = t.mask & 4u ? v10 : 0.75f; v11 = t.mask & 8u ? v11 : 0.75f;
              }
              const float out = warp_lerp(v00, v01, v10, v11, t.wx, t.wy), near = plane[t.on];
              REQUIRE(std::isfinite(out) && std::fabs(out) <= 6.001f && std::isfinite(near), "a finite plane gave %g", out);
              ++checked;
            }
    // 3. a constant integer displacement is an exact shift, alpha = 0 the identity
    for (int y = 0; y < Y; ++y)
      for (int x = 0; x < X; ++x)
        for (int dy : {-50, -3, 0, 1, 44})
          for (int dx : {-41, -1, 0, 2, 60}) {
            const ElasticTaps t = elastic_voxel<MODE>(y, x, 4.f, (float)dy * 0.25f, (float)dx * 0.25f, Y, X, py, px);
            const int wy = literal_tap(MODE, (long long)y + dy, Y), wx = literal_tap(MODE, (long long)x + dx, X);
            REQUIRE(t.wx == 0.f && t.wy == 0.f, "an integer displacement has weights (%g, %g)", t.wx, t.wy);
            if (wy >= 0 && wx >= 0) REQUIRE((t.mask & 1u) && (t.mask & ELASTIC_IN_NEAREST) && t.o00 == wy * X + wx && t.on == t.o00, "shift (%d, %d) at (%d, %d): tap %d, expected %d", dy, dx, y, x, t.o00, wy * X + wx);
            else REQUIRE(!(t.mask & 1u) && !(t.mask & ELASTIC_IN_NEAREST), "shift (%d, %d) at (%d, %d) leaves the plane but reads it", dy, dx, y, x);
            const ElasticTaps id = elastic_voxel<MODE>(y, x, 0.f, (float)dy * 1e3f, (float)dx, Y, X, py, px);
            REQUIRE(id.o00 == y * X + x && id.on == id.o00 && id.wx == 0.f && id.wy == 0.f && (id.mask & 17u) == 17u, "alpha 0 is not the identity at (%d, %d)", y, x);
          }
    UNPOISON(raw, total);
    free(raw);
  }
  printf("2-3. elastic_voxel<%d>: %lld adversarial voxels keep every tap inside its plane; integer shifts and alpha 0 are exact\n", MODE, checked);
}

int main() {
  check_taps<BPX_WARP_CONSTANT>();
  check_taps<BPX_WARP_REFLECT>();
  check_taps<BPX_WARP_EDGE>();
  check_voxels<BPX_WARP_CONSTANT>();
  check_voxels<BPX_WARP_REFLECT>();
  check_voxels<BPX_WARP_EDGE>();
  printf("elastic_cpu_check: all parts passed\n");
  return 0;
}
