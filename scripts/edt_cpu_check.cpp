// Host run of the distance transform of biapy_amd/csrc/edt.hip: the same one-dimensional pieces (csrc/edt_core.h: run start / end from a
// chunk's boundary bits with the carry across chunks, the envelope build and query, the integer and fp64 metrics) in the same order of
// passes (row, Y columns, Z columns, in place) over whole small volumes, in binary and in label mode, checked against a brute-force O(n^2)
// minimum - exactly on the integer path, to 1e-12 relative on the fp64 path.  The stacks are sized as the library sizes them (one entry per
// column position), so an entry too many is an out-of-bounds write the sanitizer sees.  A development aid:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I biapy_amd/csrc scripts/edt_cpu_check.cpp -o edt_cpu_check
//   ./edt_cpu_check
// Prints one line per volume and exits nonzero on the first mismatch.  Not loaded into Python, not part of the test suite.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "edt_core.h"

struct Vol {
  int Z, Y, X;
  std::vector<int> k;     // keys
  Vol(int z, int y, int x) : Z(z), Y(y), X(x), k((size_t)z * y * x, 0) {}
  size_t n() const { return (size_t)Z * Y * X; }
  int& at(int z, int y, int x) { return k[((size_t)z * Y + y) * X + x]; }
};

template <class V> struct HostStack {     // exactly n entries: an overrun is the sanitizer's
  std::vector<int> pos, t;
  std::vector<V> h;
  explicit HostStack(int n) : pos(n), t(n), h(n) {}
  void put(int q, int p, int tt, V hh) { pos.at(q) = p; t.at(q) = tt; h.at(q) = hh; }
  void get(int q, int& p, int& tt, V& hh) const { p = pos.at(q); tt = t.at(q); hh = h.at(q); }
};

// the row pass of edt_row_kernel, the wave's 64 lanes one after the other
template <class M> static void row_pass(const M& m, const int* key, int X, typename M::val* val) {
  typedef typename M::val V;
  const int chunks = (X + 63) / 64;
  int64_t carry = 0;
  for (int c = 0; c < chunks; ++c) {
    const int64_t base = (int64_t)c * 64;
    uint64_t bnd = 0;
    for (int l = 0; l < 64; ++l) {
      const int64_t x = base + l;
      if (x < X && x > 0 && key[x] != key[x - 1]) bnd |= 1ull << l;
    }
    for (int l = 0; l < 64 && base + l < X; ++l) val[base + l] = (V)edt_left_steps(base + l, edt_run_start(bnd, l, base, carry));
    if (bnd) carry = base + 63 - __builtin_clzll(bnd);
  }
  carry = X - 1;
  for (int c = chunks - 1; c >= 0; --c) {
    const int64_t base = (int64_t)c * 64;
    uint64_t bnd = 0;
    for (int l = 0; l < 64; ++l) {
      const int64_t x = base + l;
      if (x < X - 1 && key[x] != key[x + 1]) bnd |= 1ull << l;
    }
    for (int l = 0; l < 64 && base + l < X; ++l) {
      const int64_t x = base + l, dl = (int64_t)val[x], dr = edt_right_steps(x, edt_run_end(bnd, l, base, carry), X);
      const int64_t d = dl == 0 ? dr : (dr == 0 ? dl : std::min(dl, dr));
      val[x] = key[x] == 0 ? (V)0 : (d == 0 ? M::inf() : m.steps(d));
    }
    if (bnd) carry = base + __builtin_ctzll(bnd);
  }
}

template <class M> static std::vector<typename M::val> transform(const Vol& v, const M& mz, const M& my, const M& mx) {
  typedef typename M::val V;
  std::vector<V> val(v.n());
  for (int r = 0; r < v.Z * v.Y; ++r) row_pass(mx, v.k.data() + (size_t)r * v.X, v.X, val.data() + (size_t)r * v.X);
  auto columns = [&](const M& m, int64_t cols, int len, int64_t inner, int64_t outer, int64_t stride) {
    HostStack<V> st(len);
    for (int64_t c = 0; c < cols; ++c) {
      const int64_t base = (c / inner) * outer + c % inner;
      edt_column(
          m, st, len, [&](int i) { return v.k[base + i * stride]; }, [&](int i) { return val[base + i * stride]; },
          [&](int i, V x) { val[base + i * stride] = x; }, false);
    }
  };
  const int64_t plane = (int64_t)v.Y * v.X;
  columns(my, (int64_t)v.Z * v.X, v.Y, v.X, plane, v.X);
  columns(mz, plane, v.Z, plane, 0, plane);
  return val;
}

static int failures = 0;

static void check(const std::string& name, const Vol& v) {
  const double w[3] = {2.0, 1.0, 0.5};
  const std::vector<int32_t> gi = transform(v, EdtInt{}, EdtInt{}, EdtInt{});
  const std::vector<double> gd = transform(v, EdtF64{w[0]}, EdtF64{w[1]}, EdtF64{w[2]});
  int bad = 0;
  int64_t largest = 0;
  for (int z = 0; z < v.Z; ++z)
    for (int y = 0; y < v.Y; ++y)
      for (int x = 0; x < v.X; ++x) {
        const size_t i = ((size_t)z * v.Y + y) * v.X + x;
        int64_t bi = EDT_INF;
        double bd = INFINITY;
        if (v.k[i] == 0) { bi = 0; bd = 0; }
        else
          for (int c = 0; c < v.Z; ++c)
            for (int b = 0; b < v.Y; ++b)
              for (int a = 0; a < v.X; ++a)
                if (v.k[((size_t)c * v.Y + b) * v.X + a] != v.k[i]) {
                  const int64_t dz = c - z, dy = b - y, dx = a - x;
                  bi = std::min(bi, dz * dz + dy * dy + dx * dx);
                  bd = std::min(bd, w[0] * w[0] * dz * dz + w[1] * w[1] * dy * dy + w[2] * w[2] * dx * dx);
                }
        if (bi != EDT_INF) largest = std::max(largest, bi);
        const bool ok_i = gi[i] == bi;
        const bool ok_d = std::isinf(bd) ? std::isinf(gd[i]) : std::fabs(gd[i] - bd) <= 1e-12 * bd;
        if (!ok_i || !ok_d) {
          if (++bad <= 3) std::printf("  at (%d,%d,%d) key %d: int %d, expected %lld; fp64 %.17g, expected %.17g\n", z, y, x, v.k[i], gi[i], (long long)bi, gd[i], bd);
        }
      }
  if (bad) ++failures;
  std::printf("%-34s %2d x %3d x %3d  largest squared distance %lld  %s\n", name.c_str(), v.Z, v.Y, v.X, (long long)largest, bad ? "MISMATCH" : "ok");
}

int main() {
  std::mt19937 rng(0);
  std::uniform_real_distribution<float> uni(0.f, 1.f);
  const int shapes[][3] = {{5, 9, 70}, {3, 17, 130}, {1, 13, 66}, {5, 1, 1}, {1, 1, 200}, {1, 150, 2}, {90, 2, 3}, {7, 8, 64}};
  for (const auto& s : shapes) {
    for (float p : {0.5f, 0.9f, 0.99f}) {
      Vol v(s[0], s[1], s[2]);
      for (auto& b : v.k) b = uni(rng) < p ? 1 : 0;
      check("binary p=" + std::to_string(p).substr(0, 4), v);
    }
    { Vol v(s[0], s[1], s[2]); check("all zero", v); }
    { Vol v(s[0], s[1], s[2]); std::fill(v.k.begin(), v.k.end(), 1); check("all one (sentinel)", v); }
    { Vol v(s[0], s[1], s[2]); std::fill(v.k.begin(), v.k.end(), 1); v.k[0] = 0; check("single zero at the first corner", v); }
    { Vol v(s[0], s[1], s[2]); std::fill(v.k.begin(), v.k.end(), 1); v.k.back() = 0; check("single zero at the last corner", v); }
    { Vol v(s[0], s[1], s[2]); std::fill(v.k.begin(), v.k.end(), 7); v.at(s[0] / 2, s[1] / 2, s[2] / 2) = 9; check("one foreign label in the middle", v); }
    { Vol v(s[0], s[1], s[2]);
      for (int z = 0; z < s[0]; ++z) for (int y = 0; y < s[1]; ++y) for (int x = 0; x < s[2]; ++x) v.at(z, y, x) = (x + y + z) % 11 != 0;
      check("diagonal zero planes", v); }
    { Vol v(s[0], s[1], s[2]);
      for (int z = 0; z < s[0]; ++z) for (int y = 0; y < s[1]; ++y) for (int x = 0; x < s[2]; ++x) v.at(z, y, x) = (x + y + z) & 1;
      check("checkerboard", v); }
    for (int labels : {3, 40}) {
      Vol v(s[0], s[1], s[2]);
      std::vector<int> block(1040);                                   // 4 x 4 x 4 blocks of one label each, ids 2^30 + k, 0 = background
      for (auto& b : block) b = (int)(rng() % (labels + 1));
      for (int z = 0; z < s[0]; ++z) for (int y = 0; y < s[1]; ++y) for (int x = 0; x < s[2]; ++x) {
        const int b = block[((z / 4) * 7 + (y / 4)) * 13 % 1000 + (x / 4) % 40];
        v.at(z, y, x) = b ? b + (1 << 30) : 0;
      }
      check("touching blocks of " + std::to_string(labels) + " labels", v);
    }
    { Vol v(s[0], s[1], s[2]);
      for (auto& b : v.k) b = (int)(rng() % 4);
      check("random labels 0..3", v); }
  }
  if (failures) std::printf("FAILED: %d volumes disagree with the brute force\n", failures);
  else std::printf("all volumes agree with the brute force\n");
  return failures ? 1 : 0;
}
