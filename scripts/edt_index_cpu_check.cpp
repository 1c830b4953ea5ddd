// Host run of the nearest-source transform of biapy_amd/csrc/edt_index.hip: the same one-dimensional pieces (csrc/edt_core.h: run start / end
// from a chunk's boundary bits, edt_row_steps / edt_row_site, edt_column_sites with the index carried in the stack entry, the integer and fp64
// metrics) in the same order of passes (row, Y columns, Z columns, values and indices in place) over whole small volumes, plain and inverted,
// checked against the brute-force rule "nearest source, smallest linear index among the nearest": on the integer path value AND index exactly -
// which is the tie behaviour of the envelope (equal costs keep the earlier site) confirmed, not assumed - and on the fp64 path the value to
// 1e-12 relative and the index as a source whose true distance is within 1e-12 relative of the least.  The stacks are sized as the library
// sizes them (one entry per column position), so an entry too many is an out-of-bounds write the sanitizer sees.  A development aid:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I biapy_amd/csrc scripts/edt_index_cpu_check.cpp -o edt_index_cpu_check
//   ./edt_index_cpu_check
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
  std::vector<int> v;     // values
  Vol(int z, int y, int x) : Z(z), Y(y), X(x), v((size_t)z * y * x, 0) {}
  size_t n() const { return (size_t)Z * Y * X; }
  int& at(int z, int y, int x) { return v[((size_t)z * Y + y) * X + x]; }
};

template <class V> struct HostSiteStack {     // exactly n entries: an overrun is the sanitizer's
  std::vector<int> pos, t, ix;
  std::vector<V> h;
  int cur = -1, top = -1;
  explicit HostSiteStack(int n) : pos(n), t(n), ix(n), h(n) {}
  void put(int q, int p, int tt, V hh) { pos.at(q) = p; t.at(q) = tt; h.at(q) = hh; ix.at(q) = cur; top = cur; }
  void get(int q, int& p, int& tt, V& hh) { p = pos.at(q); tt = t.at(q); hh = h.at(q); top = ix.at(q); }
};

// the row pass of edt_index_row_kernel, the wave's 64 lanes one after the other; key: 0 = a source
template <class M> static void row_pass(const M& m, const int* key, int64_t row, int X, typename M::val* val, int32_t* idx) {
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
      const int64_t d = edt_row_steps(dl, dr);
      val[x] = key[x] == 0 ? (V)0 : (d == 0 ? M::inf() : m.steps(d));
      idx[x] = key[x] == 0 ? (int32_t)(row + x) : edt_row_site(row + x, dl, dr);
    }
    if (bnd) carry = base + __builtin_ctzll(bnd);
  }
}

template <class M>
static void transform(const Vol& v, const std::vector<int>& key, const M& mz, const M& my, const M& mx, std::vector<typename M::val>& val, std::vector<int32_t>& idx) {
  typedef typename M::val V;
  val.assign(v.n(), V());
  idx.assign(v.n(), 0);
  for (int r = 0; r < v.Z * v.Y; ++r) row_pass(mx, key.data() + (size_t)r * v.X, (int64_t)r * v.X, v.X, val.data() + (size_t)r * v.X, idx.data() + (size_t)r * v.X);
  auto columns = [&](const M& m, int64_t cols, int len, int64_t inner, int64_t outer, int64_t stride) {
    HostSiteStack<V> st(len);
    for (int64_t c = 0; c < cols; ++c) {
      const int64_t base = (c / inner) * outer + c % inner;
      edt_column_sites(
          m, st, len, [&](int i) { return key[base + i * stride]; }, [&](int i) { return val[base + i * stride]; },
          [&](int i) { return (int)idx[base + i * stride]; },
          [&](int i, V x, int site) { val[base + i * stride] = x; idx[base + i * stride] = site; }, false);
    }
  };
  const int64_t plane = (int64_t)v.Y * v.X;
  columns(my, (int64_t)v.Z * v.X, v.Y, v.X, plane, v.X);
  columns(mz, plane, v.Z, plane, 0, plane);
}

static int failures = 0;

static void check(const std::string& name, const Vol& v, int invert) {
  const double w[3] = {2.0, 1.0, 0.5};
  std::vector<int> key(v.n());
  for (size_t i = 0; i < v.n(); ++i) key[i] = (v.v[i] != 0) != (invert != 0);
  std::vector<int32_t> gi, ii, id;
  std::vector<double> gd;
  transform(v, key, EdtInt{}, EdtInt{}, EdtInt{}, gi, ii);
  transform(v, key, EdtF64{w[0]}, EdtF64{w[1]}, EdtF64{w[2]}, gd, id);
  auto dist64 = [&](size_t i, int32_t u) {
    const int64_t X = v.X, Y = v.Y;
    const int64_t dz = (int64_t)(u / (X * Y)) - (int64_t)(i / (X * Y)), dy = (int64_t)(u / X % Y) - (int64_t)(i / X % Y), dx = (int64_t)(u % X) - (int64_t)(i % X);
    return w[0] * w[0] * dz * dz + w[1] * w[1] * dy * dy + w[2] * w[2] * dx * dx;
  };
  int bad = 0, ties = 0;
  for (int z = 0; z < v.Z; ++z)
    for (int y = 0; y < v.Y; ++y)
      for (int x = 0; x < v.X; ++x) {
        const size_t i = ((size_t)z * v.Y + y) * v.X + x;
        int64_t bi = EDT_INF, bu = -1;
        int nearest = 0;
        double bd = INFINITY;
        for (int c = 0; c < v.Z; ++c)                                 // raster order: the first of equal minima is the smallest linear index
          for (int b = 0; b < v.Y; ++b)
            for (int a = 0; a < v.X; ++a) {
              const size_t u = ((size_t)c * v.Y + b) * v.X + a;
              if (key[u] != 0) continue;
              const int64_t dz = c - z, dy = b - y, dx = a - x, d = dz * dz + dy * dy + dx * dx;
              if (d < bi) { bi = d; bu = (int64_t)u; nearest = 1; }
              else if (d == bi) ++nearest;
              bd = std::min(bd, w[0] * w[0] * dz * dz + w[1] * w[1] * dy * dy + w[2] * w[2] * dx * dx);
            }
        if (nearest > 1) ++ties;
        const bool ok_i = gi[i] == bi && ii[i] == bu;
        bool ok_d = std::isinf(bd) ? (std::isinf(gd[i]) && id[i] == -1) : std::fabs(gd[i] - bd) <= 1e-12 * bd;
        if (ok_d && !std::isinf(bd)) ok_d = id[i] >= 0 && (size_t)id[i] < v.n() && key[id[i]] == 0 && std::fabs(dist64(i, id[i]) - bd) <= 1e-12 * bd;
        if (!ok_i || !ok_d) {
          if (++bad <= 3)
            std::printf("  at (%d,%d,%d): int %d at %d, expected %lld at %lld; fp64 %.17g at %d, expected %.17g\n", z, y, x, gi[i], ii[i], (long long)bi,
                        (long long)bu, gd[i], id[i], bd);
        }
      }
  if (bad) ++failures;
  std::printf("%-40s %2d x %3d x %3d  voxels with several nearest sources %6d  %s\n", (name + (invert ? " (inverted)" : "")).c_str(), v.Z, v.Y, v.X, ties,
              bad ? "MISMATCH" : "ok");
}

int main() {
  std::mt19937 rng(0);
  std::uniform_real_distribution<float> uni(0.f, 1.f);
  const int shapes[][3] = {{5, 9, 70}, {3, 17, 130}, {1, 13, 66}, {5, 1, 1}, {1, 1, 200}, {1, 150, 2}, {90, 2, 3}, {7, 8, 64}};
  for (const auto& s : shapes) {
    for (float p : {0.5f, 0.9f, 0.99f}) {
      Vol v(s[0], s[1], s[2]);
      for (auto& b : v.v) b = uni(rng) < p ? 1 : 0;
      check("binary p=" + std::to_string(p).substr(0, 4), v, 0);
    }
    { Vol v(s[0], s[1], s[2]); check("all zero (every voxel a source)", v, 0); check("all zero (no source)", v, 1); }
    { Vol v(s[0], s[1], s[2]); std::fill(v.v.begin(), v.v.end(), 1); v.v[0] = 0; check("single source at the first corner", v, 0); }
    { Vol v(s[0], s[1], s[2]); std::fill(v.v.begin(), v.v.end(), 1); v.v.back() = 0; check("single source at the last corner", v, 0); }
    { Vol v(s[0], s[1], s[2]); v.at(s[0] / 2, s[1] / 2, s[2] / 2) = 9; check("single label in the middle", v, 1); }
    { Vol v(s[0], s[1], s[2]);
      for (int z = 0; z < s[0]; ++z) for (int y = 0; y < s[1]; ++y) for (int x = 0; x < s[2]; ++x) v.at(z, y, x) = (x + y + z) % 11 != 0;
      check("diagonal source planes", v, 0); }
    { Vol v(s[0], s[1], s[2]);
      for (int z = 0; z < s[0]; ++z) for (int y = 0; y < s[1]; ++y) for (int x = 0; x < s[2]; ++x) v.at(z, y, x) = (x + y + z) & 1;
      check("checkerboard", v, 0); check("checkerboard", v, 1); }
    { Vol v(s[0], s[1], s[2]);
      for (int z = 0; z < s[0]; ++z) for (int y = 0; y < s[1]; ++y) for (int x = 0; x < s[2]; ++x) v.at(z, y, x) = x != s[2] / 3;
      check("source plane across the rows", v, 0); }                 // every row's g is equal along Y: every site survives in the envelope
    { Vol v(s[0], s[1], s[2]);
      for (int z = 0; z < s[0]; ++z) for (int y = 0; y < s[1]; ++y) for (int x = 0; x < s[2]; ++x) v.at(z, y, x) = ((x / 4 + y / 4 + z / 4) % 3) ? 0 : 1 + (x / 4) % 5;
      check("sparse 4 x 4 x 4 label blocks", v, 1); }
    { Vol v(s[0], s[1], s[2]);
      for (auto& b : v.v) b = (int)(rng() % 4);
      check("random labels 0..3", v, 1); }
  }
  if (failures) std::printf("FAILED: %d volumes disagree with the brute force\n", failures);
  else std::printf("all volumes agree with the brute force\n");
  return failures ? 1 : 0;
}
