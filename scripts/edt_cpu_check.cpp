// Host run of the distance transform of biapy_amd/csrc/edt.hip and edt_index.hip: the same one-dimensional pieces (csrc/edt_core.h: run start /
// end from a chunk's boundary bits with the carry across chunks, edt_row_steps / edt_row_site, the envelope build and query of edt_column -
// without a payload and with the index carried in the stack entry -, the integer and fp64 metrics) in the same order of passes (row, Y
// columns, Z columns, values and indices in place) over whole small volumes, checked against a brute-force O(n^2) minimum.  Every volume is
// keyed three ways - by its labels, by "nonzero" and by "zero" - and each distinct keying runs without indices; the two binary keyings (the
// plain and the inverted call of edt_index.hip: key 0 = a source) run with indices too.  Distances: exactly on the integer path, to 1e-12
// relative on the fp64 path.  Indices, against the rule "nearest source, smallest linear index among the nearest": exactly on the integer path
// - which is the tie behaviour of the envelope (equal costs keep the earlier site) confirmed, not assumed - and on the fp64 path as a source
// whose true distance is within 1e-12 relative of the least.  The stacks are sized as the library sizes them (one entry per column position),
// so an entry too many is an out-of-bounds write the sanitizer sees.  A development aid:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I biapy_amd/csrc scripts/edt_cpu_check.cpp -o edt_cpu_check
//   ./edt_cpu_check
// Prints one line per volume and keying and exits nonzero after a mismatch.  Not loaded into Python, not part of the test suite.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <type_traits>
#include <vector>

#include "edt_core.h"

struct Vol {
  int Z, Y, X;
  std::vector<int> v;     // values
  Vol(int z, int y, int x) : Z(z), Y(y), X(x), v((size_t)z * y * x, 0) {}
  size_t n() const { return (size_t)Z * Y * X; }
  int& at(int z, int y, int x) { return v[((size_t)z * Y + y) * X + x]; }
};

struct NoPayload {};
struct Payload {
  std::vector<int> ix;
  int cur = -1, top = -1;
};
template <class V, bool WITH_SITES> struct HostStack : std::conditional_t<WITH_SITES, Payload, NoPayload> {     // exactly n entries: an overrun is the sanitizer's
  static constexpr bool SITES = WITH_SITES;
  std::vector<int> pos, t;
  std::vector<V> h;
  explicit HostStack(int n) : pos(n), t(n), h(n) {
    if constexpr (SITES) this->ix.resize(n);
  }
  void put(int q, int p, int tt, V hh) {
    pos.at(q) = p; t.at(q) = tt; h.at(q) = hh;
    if constexpr (SITES) { this->ix.at(q) = this->cur; this->top = this->cur; }
  }
  void get(int q, int& p, int& tt, V& hh) {
    p = pos.at(q); tt = t.at(q); hh = h.at(q);
    if constexpr (SITES) this->top = this->ix.at(q);
  }
};

// the row pass of edt_row_kernel, the wave's 64 lanes one after the other; idx: with the index only
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
      if (idx) idx[x] = key[x] == 0 ? (int32_t)(row + x) : edt_row_site(row + x, dl, dr);
    }
    if (bnd) carry = base + __builtin_ctzll(bnd);
  }
}

template <class M, bool SITES>
static void transform(const Vol& v, const std::vector<int>& key, const M& mz, const M& my, const M& mx, std::vector<typename M::val>& val, std::vector<int32_t>& idx) {
  typedef typename M::val V;
  val.assign(v.n(), V());
  idx.assign(SITES ? v.n() : 0, 0);
  for (int r = 0; r < v.Z * v.Y; ++r) {
    const size_t row = (size_t)r * v.X;
    row_pass(mx, key.data() + row, (int64_t)row, v.X, val.data() + row, SITES ? idx.data() + row : nullptr);
  }
  auto columns = [&](const M& m, int64_t cols, int len, int64_t inner, int64_t outer, int64_t stride) {
    HostStack<V, SITES> st(len);
    for (int64_t c = 0; c < cols; ++c) {
      const int64_t base = (c / inner) * outer + c % inner;
      auto k = [&](int i) { return key[base + i * stride]; };
      auto load = [&](int i) { return val[base + i * stride]; };
      auto store = [&](int i, V x, int site) {
        val[base + i * stride] = x;
        if constexpr (SITES) idx[base + i * stride] = site;
      };
      if constexpr (SITES) edt_column(m, st, len, k, load, store, false, [&](int i) { return (int)idx[base + i * stride]; });
      else edt_column(m, st, len, k, load, store, false);
    }
  };
  const int64_t plane = (int64_t)v.Y * v.X;
  columns(my, (int64_t)v.Z * v.X, v.Y, v.X, plane, v.X);
  columns(mz, plane, v.Z, plane, 0, plane);
}

static int failures = 0;

// one keying of one volume: without indices and, where the keys are binary, with them, against one brute-force loop
static void check_keys(const std::string& name, const Vol& v, const std::vector<int>& key) {
  const double w[3] = {2.0, 1.0, 0.5};
  const bool sites = *std::max_element(key.begin(), key.end()) <= 1;
  std::vector<int32_t> gi, si, ii, id, none;
  std::vector<double> gd, sd;
  transform<EdtInt, false>(v, key, EdtInt{}, EdtInt{}, EdtInt{}, gi, none);
  transform<EdtF64, false>(v, key, EdtF64{w[0]}, EdtF64{w[1]}, EdtF64{w[2]}, gd, none);
  if (sites) {
    transform<EdtInt, true>(v, key, EdtInt{}, EdtInt{}, EdtInt{}, si, ii);
    transform<EdtF64, true>(v, key, EdtF64{w[0]}, EdtF64{w[1]}, EdtF64{w[2]}, sd, id);
  }
  auto dist64 = [&](size_t i, int32_t u) {
    const int64_t X = v.X, Y = v.Y;
    const int64_t dz = (int64_t)(u / (X * Y)) - (int64_t)(i / (X * Y)), dy = (int64_t)(u / X % Y) - (int64_t)(i / X % Y), dx = (int64_t)(u % X) - (int64_t)(i % X);
    return w[0] * w[0] * dz * dz + w[1] * w[1] * dy * dy + w[2] * w[2] * dx * dx;
  };
  int bad = 0, ties = 0;
  int64_t largest = 0;
  for (int z = 0; z < v.Z; ++z)
    for (int y = 0; y < v.Y; ++y)
      for (int x = 0; x < v.X; ++x) {
        const size_t i = ((size_t)z * v.Y + y) * v.X + x;
        int64_t bi = EDT_INF, bu = -1;
        int nearest = 0;
        double bd = INFINITY;
        if (key[i] == 0) { bi = 0; bu = (int64_t)i; bd = 0; }
        else
          for (int c = 0; c < v.Z; ++c)                               // raster order: the first of equal minima is the smallest linear index
            for (int b = 0; b < v.Y; ++b)
              for (int a = 0; a < v.X; ++a) {
                const size_t u = ((size_t)c * v.Y + b) * v.X + a;
                if (key[u] == key[i]) continue;
                const int64_t dz = c - z, dy = b - y, dx = a - x, d = dz * dz + dy * dy + dx * dx;
                if (d < bi) { bi = d; bu = (int64_t)u; nearest = 1; }
                else if (d == bi) ++nearest;
                bd = std::min(bd, w[0] * w[0] * dz * dz + w[1] * w[1] * dy * dy + w[2] * w[2] * dx * dx);
              }
        if (nearest > 1) ++ties;
        if (bi != EDT_INF) largest = std::max(largest, bi);
        auto near = [&](double g) { return std::isinf(bd) ? std::isinf(g) : std::fabs(g - bd) <= 1e-12 * bd; };
        bool ok = gi[i] == bi && near(gd[i]);
        if (sites) {
          ok = ok && si[i] == bi && ii[i] == bu && near(sd[i]);
          if (std::isinf(bd)) ok = ok && id[i] == -1;
          else ok = ok && id[i] >= 0 && (size_t)id[i] < v.n() && key[id[i]] == 0 && std::fabs(dist64(i, id[i]) - bd) <= 1e-12 * bd;
        }
        if (!ok && ++bad <= 3) {
          std::printf("  at (%d,%d,%d) key %d: int %d, expected %lld; fp64 %.17g, expected %.17g\n", z, y, x, key[i], gi[i], (long long)bi, gd[i], bd);
          if (sites) std::printf("    with indices: int %d at %d, expected at %lld; fp64 %.17g at %d\n", si[i], ii[i], (long long)bu, sd[i], id[i]);
        }
      }
  if (bad) ++failures;
  std::printf("%-46s %2d x %3d x %3d  %-12s largest squared distance %6lld  several nearest %6d  %s\n", name.c_str(), v.Z, v.Y, v.X,
              sites ? "with indices" : "", (long long)largest, ties, bad ? "MISMATCH" : "ok");
}

// label mode, binary mode / the plain call with indices, the inverted call with indices
static void check(const std::string& name, const Vol& v) {
  std::vector<int> bin(v.n()), inv(v.n());
  for (size_t i = 0; i < v.n(); ++i) { bin[i] = v.v[i] != 0; inv[i] = v.v[i] == 0; }
  if (bin != v.v) check_keys(name + " (labels)", v, v.v);
  check_keys(name, v, bin);
  check_keys(name + " (inverted)", v, inv);
}

int main() {
  std::mt19937 rng(0);
  std::uniform_real_distribution<float> uni(0.f, 1.f);
  const int shapes[][3] = {{5, 9, 70}, {3, 17, 130}, {1, 13, 66}, {5, 1, 1}, {1, 1, 200}, {1, 150, 2}, {90, 2, 3}, {7, 8, 64}};
  for (const auto& s : shapes) {
    auto fill = [&](auto&& f) {
      Vol v(s[0], s[1], s[2]);
      for (int z = 0; z < s[0]; ++z) for (int y = 0; y < s[1]; ++y) for (int x = 0; x < s[2]; ++x) v.at(z, y, x) = f(z, y, x);
      return v;
    };
    for (float p : {0.5f, 0.9f, 0.99f}) check("binary p=" + std::to_string(p).substr(0, 4), fill([&](int, int, int) { return uni(rng) < p ? 1 : 0; }));
    check("all zero", Vol(s[0], s[1], s[2]));                          // every voxel a source; inverted: no source, the sentinel and -1
    { Vol v = fill([](int, int, int) { return 1; }); v.v[0] = 0; check("single zero at the first corner", v); }
    { Vol v = fill([](int, int, int) { return 1; }); v.v.back() = 0; check("single zero at the last corner", v); }
    { Vol v = fill([](int, int, int) { return 7; }); v.at(s[0] / 2, s[1] / 2, s[2] / 2) = 9; check("one foreign label in the middle", v); }
    { Vol v(s[0], s[1], s[2]); v.at(s[0] / 2, s[1] / 2, s[2] / 2) = 9; check("single label in the middle", v); }
    check("diagonal zero planes", fill([](int z, int y, int x) { return (x + y + z) % 11 != 0; }));
    check("checkerboard", fill([](int z, int y, int x) { return (x + y + z) & 1; }));
    check("zero plane across the rows", fill([&](int, int, int x) { return x != s[2] / 3; }));   // every row's g is equal along Y: every site survives in the envelope
    for (int labels : {3, 40}) {
      std::vector<int> block(1040);                                   // 4 x 4 x 4 blocks of one label each, ids 2^30 + k, 0 = background
      for (auto& b : block) b = (int)(rng() % (labels + 1));
      check("touching blocks of " + std::to_string(labels) + " labels", fill([&](int z, int y, int x) {
              const int b = block[((z / 4) * 7 + (y / 4)) * 13 % 1000 + (x / 4) % 40];
              return b ? b + (1 << 30) : 0;
            }));
    }
    check("sparse 4 x 4 x 4 label blocks", fill([](int z, int y, int x) { return ((x / 4 + y / 4 + z / 4) % 3) ? 0 : 1 + (x / 4) % 5; }));
    check("random labels 0..3", fill([&](int, int, int) { return (int)(rng() % 4); }));
  }
  if (failures) std::printf("FAILED: %d runs disagree with the brute force\n", failures);
  else std::printf("all volumes agree with the brute force\n");
  return failures ? 1 : 0;
}
