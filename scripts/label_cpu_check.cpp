// Host run of the labelling algorithm of biapy_amd/csrc/label.hip: the same find / unite / neighbour enumeration (csrc/label_uf.h) and the same
// sequence of steps (merge in both forms, flatten + count, scan, rank, map) over structured and random masks, sequentially and with the
// union phase spread over std::threads on std::atomic<int>, checked against a plain flood fill that numbers components in raster order of
// their first voxel.  A development aid for finding an unbounded loop or an off-by-one at a volume or tile edge before the kernels run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -I biapy_amd/csrc scripts/label_cpu_check.cpp -o label_cpu_check
//   ./label_cpu_check
// Prints one line per mask and exits nonzero on the first mismatch.  Not loaded into Python, not part of the test suite.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "label_uf.h"

struct HostMem {
  std::atomic<int>* p;
  int load(int i) const { return p[i].load(std::memory_order_relaxed); }
  int amin(int i, int v) const {
    int cur = p[i].load(std::memory_order_relaxed);
    while (v < cur && !p[i].compare_exchange_weak(cur, v, std::memory_order_relaxed)) {}
    return cur;
  }
};

struct Vol {
  int Z, Y, X;
  std::vector<uint8_t> m;
  Vol(int z, int y, int x) : Z(z), Y(y), X(x), m((size_t)z * y * x, 0) {}
  int n() const { return Z * Y * X; }
  uint8_t& at(int z, int y, int x) { return m[((size_t)z * Y + y) * X + x]; }
};

static std::vector<int> flood_fill(const Vol& v, int conn, int* num) {
  std::vector<int> lab(v.n(), 0), stack;
  int next = 0;
  for (int s = 0; s < v.n(); ++s) {
    if (!v.m[s] || lab[s]) continue;
    lab[s] = ++next;                        // raster-first voxel of a new component
    stack.push_back(s);
    while (!stack.empty()) {
      const int i = stack.back();
      stack.pop_back();
      const int x = i % v.X, y = (i / v.X) % v.Y, z = i / v.X / v.Y;
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int k = (dz != 0) + (dy != 0) + (dx != 0);
            if (k == 0 || k > conn) continue;
            const int nz = z + dz, ny = y + dy, nx = x + dx;
            if (nz < 0 || nz >= v.Z || ny < 0 || ny >= v.Y || nx < 0 || nx >= v.X) continue;
            const int j = (nz * v.Y + ny) * v.X + nx;
            if (v.m[j] && !lab[j]) { lab[j] = next; stack.push_back(j); }
          }
    }
  }
  *num = next;
  return lab;
}

static void parallel_for(int threads, int count, const std::function<void(int)>& f) {   // item q runs on thread q % threads: neighbours on different threads
  if (threads <= 1) { for (int q = 0; q < count; ++q) f(q); return; }
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([=, &f] { for (int q = t; q < count; q += threads) f(q); });
  for (auto& th : pool) th.join();
}

// the launch sequence of bpx_label_u8, step for step
static std::vector<int> label_host(const Vol& v, int conn, bool tiled, int threads, bool map_backwards, int* num) {
  const int n = v.n(), Z = v.Z, Y = v.Y, X = v.X;
  std::unique_ptr<std::atomic<int>[]> parent(new std::atomic<int>[n]);
  const HostMem g{parent.get()};
  auto cross_or_all = [&](int i, bool cross) {
    const int x = i % X, zy = i / X, y = zy % Y, z = zy / Y;
    const int lz = z % LBL_TZ, ly = y % LBL_TY, lx = x % LBL_TX;
    if (cross && !(lz == 0 || ly == 0 || ly == LBL_TY - 1 || lx == 0 || lx == LBL_TX - 1)) return;
    if (!v.m[i]) return;
    auto at = [&](int dz, int dy, int dx) { return ((z + dz) * Y + (y + dy)) * X + (x + dx); };
    lbl_for_backward(
        conn,
        [&](int dz, int dy, int dx) {
          const int nz = z + dz, ny = y + dy, nx = x + dx;
          return nz >= 0 && ny >= 0 && ny < Y && nx >= 0 && nx < X && v.m[at(dz, dy, dx)] != 0;
        },
        [&](int dz, int dy, int dx) {
          if (!cross || lbl_leaves_tile(lz, ly, lx, dz, dy, dx)) lbl_unite(g, i, at(dz, dy, dx));
        });
  };
  if (tiled) {
    const int ntx = (X + LBL_TX - 1) / LBL_TX, nty = (Y + LBL_TY - 1) / LBL_TY, ntz = (Z + LBL_TZ - 1) / LBL_TZ;
    parallel_for(threads, ntx * nty * ntz, [&](int b) {
      std::unique_ptr<std::atomic<int>[]> P(new std::atomic<int>[LBL_TV]);
      std::vector<uint8_t> M(LBL_TV);
      const HostMem m{P.get()};
      const int x0 = (b % ntx) * LBL_TX, y0 = ((b / ntx) % nty) * LBL_TY, z0 = (b / ntx / nty) * LBL_TZ;
      for (int l = 0; l < LBL_TV; ++l) {
        const int lx = l % LBL_TX, ly = (l / LBL_TX) % LBL_TY, lz = l / (LBL_TX * LBL_TY);
        const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
        M[l] = (z < Z && y < Y && x < X && v.m[((size_t)z * Y + y) * X + x]) ? 1 : 0;
        P[l].store(M[l] ? l : LBL_BG);
      }
      for (int l = 0; l < LBL_TV; ++l) {
        if (!M[l]) continue;
        const int lx = l % LBL_TX, ly = (l / LBL_TX) % LBL_TY, lz = l / (LBL_TX * LBL_TY);
        lbl_for_backward(
            conn, [&](int dz, int dy, int dx) { return !lbl_leaves_tile(lz, ly, lx, dz, dy, dx) && M[l + (dz * LBL_TY + dy) * LBL_TX + dx] != 0; },
            [&](int dz, int dy, int dx) { lbl_unite(m, l, l + (dz * LBL_TY + dy) * LBL_TX + dx); });
      }
      for (int l = 0; l < LBL_TV; ++l) {
        const int lx = l % LBL_TX, ly = (l / LBL_TX) % LBL_TY, lz = l / (LBL_TX * LBL_TY);
        const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
        if (z >= Z || y >= Y || x >= X) continue;
        int out = LBL_BG;
        if (M[l]) {
          const int r = lbl_find(m, l);
          out = ((z0 + r / (LBL_TX * LBL_TY)) * Y + (y0 + (r / LBL_TX) % LBL_TY)) * X + (x0 + r % LBL_TX);
        }
        parent[(z * Y + y) * X + x].store(out);
      }
    });
    parallel_for(threads, n, [&](int i) { cross_or_all(i, true); });
  } else {
    for (int i = 0; i < n; ++i) parent[i].store(v.m[i] ? i : LBL_BG);
    parallel_for(threads, n, [&](int i) { cross_or_all(i, false); });
  }
  // flatten + count
  const int chunks = (int)lbl_chunks(n);
  std::vector<int> counts(chunks, 0);
  parallel_for(threads, chunks, [&](int c) {
    for (int i = c * LBL_CHUNK; i < n && i < (c + 1) * LBL_CHUNK; ++i) {
      const int p = g.load(i);
      if (p < 0) continue;
      if (p == i) { ++counts[c]; continue; }
      const int r = lbl_find(g, p);
      if (r != p) parent[i].store(r, std::memory_order_relaxed);
    }
  });
  int total = 0;                                                     // scan
  for (int c = 0; c < chunks; ++c) { const int k = counts[c]; counts[c] = total; total += k; }
  *num = total;
  for (int c = 0; c < chunks; ++c) {                                 // rank
    int k = counts[c];
    for (int i = c * LBL_CHUNK; i < n && i < (c + 1) * LBL_CHUNK; ++i)
      if (g.load(i) == i) parent[i].store(-(++k));
  }
  std::vector<int> lab(n);                                           // map, in place, in either order
  for (int q = 0; q < n; ++q) {
    const int i = map_backwards ? n - 1 - q : q;
    const int val = g.load(i);
    int out;
    if (val == LBL_BG) out = 0;
    else if (val < 0) out = -val;
    else { const int r = g.load(val); out = r < 0 ? -r : r; }
    parent[i].store(out);
  }
  for (int i = 0; i < n; ++i) lab[i] = g.load(i);
  return lab;
}

static int failures = 0;

static void check(const std::string& name, const Vol& v) {
  for (int conn = 1; conn <= 3; ++conn) {
    int want_n = 0;
    const std::vector<int> want = flood_fill(v, conn, &want_n);
    for (int tiled = 0; tiled <= 1; ++tiled)
      for (int threads : {1, 4}) {
        int got_n = -1;
        const std::vector<int> got = label_host(v, conn, tiled != 0, threads, threads == 4, &got_n);
        if (got_n != want_n || got != want) {
          ++failures;
          std::printf("MISMATCH %s conn %d tiled %d threads %d: N %d, expected %d\n", name.c_str(), conn, tiled, threads, got_n, want_n);
        }
      }
    std::printf("%-28s %2d x %3d x %3d  conn %d  N = %d\n", name.c_str(), v.Z, v.Y, v.X, conn, want_n);
  }
}

static Vol snake(int Z, int Y, int X) {   // a one-voxel-wide path through the whole volume: boustrophedon rows in the even planes, joined at alternating ends
  Vol v(Z, Y, X);
  const int R = (Y - 1) / 2;
  for (int z = 0; z < Z; z += 2) {
    for (int r = 0; r <= R; ++r) {
      for (int x = 0; x < X; ++x) v.at(z, 2 * r, x) = 1;
      if (r < R) v.at(z, 2 * r + 1, r % 2 == 0 ? X - 1 : 0) = 1;
    }
    if (z + 2 < Z) {
      if ((z / 2) % 2 == 0) v.at(z + 1, 2 * R, R % 2 == 0 ? X - 1 : 0) = 1;   // at the path's end
      else v.at(z + 1, 0, 0) = 1;                                             // at its start
    }
  }
  return v;
}

int main() {
  const int Z = 20, Y = 43, X = 150;      // two full 8 x 8 x 64 tiles and a partial one on every axis
  { Vol v(Z, Y, X); check("all zero", v); }
  { Vol v(Z, Y, X); std::fill(v.m.begin(), v.m.end(), 255); check("all one", v); }
  { Vol v(Z, Y, X); v.m.back() = 2; check("last voxel", v); }
  { Vol v(Z, Y, X); for (int z = 0; z < Z; ++z) for (int y = 0; y < Y; ++y) for (int x = 0; x < X; ++x) v.at(z, y, x) = (z + y + x) & 1; check("checkerboard", v); }
  check("boustrophedon", snake(Z, Y, X));
  { Vol v(Z, Y, X);
    for (int z = 0; z < Z; ++z) {
      for (int x = 0; x < X; ++x) { v.at(z, 0, x) = 1; v.at(z, Y - 1, x) = 1; }
      for (int x = 0; x < X; x += 4) for (int y = 0; y <= Y - 3; ++y) v.at(z, y, x) = 1;
      for (int x = 2; x < X; x += 4) for (int y = 2; y < Y; ++y) v.at(z, y, x) = 1;
    }
    check("interleaved combs", v); }
  { Vol v(Z, Y, X);
    v.at(7, 7, 10) = v.at(8, 8, 10) = 1;        // edge pair across a tile edge (z, y)
    v.at(15, 3, 63) = v.at(16, 3, 64) = 1;      // edge pair across a tile edge (z, x)
    v.at(15, 30, 64) = v.at(16, 30, 63) = 1;    // the same, other diagonal
    v.at(8, 24, 5) = v.at(9, 23, 5) = 1;        // edge pair leaving the tile upwards in y from its inside in z
    v.at(3, 15, 100) = v.at(3, 16, 101) = 1;    // edge pair (y, x) inside one z
    v.at(7, 15, 63) = v.at(8, 16, 64) = 1;      // corner pair across a tile corner
    v.at(7, 32, 64) = v.at(8, 31, 63) = 1;      // corner pair, other diagonals
    v.at(15, 39, 127) = v.at(16, 40, 128) = 1;
    check("pairs across tile borders", v); }
  std::mt19937 rng(0);
  std::uniform_real_distribution<float> uni(0.f, 1.f);
  const int shapes[][3] = {{9, 21, 37}, {2, 64, 128}, {17, 16, 200}, {1, 33, 70}, {5, 1, 1}, {1, 1, 300}};
  for (const auto& s : shapes)
    for (float p : {0.1f, 0.25f, 0.32f, 0.5f, 0.9f}) {
      Vol v(s[0], s[1], s[2]);
      for (auto& b : v.m) b = uni(rng) < p ? 1 : 0;
      check("random p=" + std::to_string(p).substr(0, 4), v);
    }
  if (failures) std::printf("FAILED: %d mismatches\n", failures);
  else std::printf("all masks agree with the flood fill\n");
  return failures ? 1 : 0;
}
