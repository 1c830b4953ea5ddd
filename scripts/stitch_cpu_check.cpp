// Host run of the label stitching of biapy_amd/csrc/stitch.hip, rule "touch": the same shell enumeration, neighbour lookup and unions
// (csrc/stitch_core.h over csrc/label_uf.h) and the same sequence of steps (offsets, first voxels, shell unions, resolve, rank by key, apply)
// over structured and random masks cut by ragged grids, blocks one voxel thick included, at every connectivity, sequentially and with the
// union phase spread over std::threads on std::atomic<int>, checked against a plain flood fill of the WHOLE volume that numbers components in
// raster order of their first voxel.  The per-block labels come from the same flood fill run on each block alone.  The shell enumeration is
// checked on its own too: every shell voxel once, nothing else.  A development aid for finding an off-by-one at a block edge or an
// out-of-bounds neighbour before the kernels run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -I biapy_amd/csrc scripts/stitch_cpu_check.cpp -o stitch_cpu_check
//   ./stitch_cpu_check
// Prints one line per mask and grid and exits nonzero on the first mismatch.  Not loaded into Python, not part of the test suite.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <functional>
#include <memory>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "label_uf.h"
#include "stitch_core.h"

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
  uint8_t get(int z, int y, int x) const { return m[((size_t)z * Y + y) * X + x]; }
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

static void parallel_for(int threads, int64_t count, const std::function<void(int64_t)>& f) {   // item q runs on thread q % threads
  if (threads <= 1) { for (int64_t q = 0; q < count; ++q) f(q); return; }
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([=, &f] { for (int64_t q = t; q < count; q += threads) f(q); });
  for (auto& th : pool) th.join();
}

static int failures = 0;

static void check_shell(int ez, int ey, int ex) {
  std::vector<int> seen((size_t)ez * ey * ex, 0);
  const int64_t n = stitch_shell_count(ez, ey, ex);
  for (int64_t t = 0; t < n; ++t) {
    int z = -1, y = -1, x = -1;
    stitch_shell_voxel(t, ez, ey, ex, z, y, x);
    if (z < 0 || z >= ez || y < 0 || y >= ey || x < 0 || x >= ex) { ++failures; std::printf("SHELL %d x %d x %d: entry %lld leaves the block\n", ez, ey, ex, (long long)t); return; }
    ++seen[((size_t)z * ey + y) * ex + x];
  }
  for (int z = 0; z < ez; ++z)
    for (int y = 0; y < ey; ++y)
      for (int x = 0; x < ex; ++x) {
        const bool shell = z == 0 || z == ez - 1 || y == 0 || y == ey - 1 || x == 0 || x == ex - 1;
        if (seen[((size_t)z * ey + y) * ex + x] != (shell ? 1 : 0)) { ++failures; std::printf("SHELL %d x %d x %d: voxel (%d, %d, %d) seen %d times\n", ez, ey, ex, z, y, x, seen[((size_t)z * ey + y) * ex + x]); return; }
      }
}

// the launch sequence of LabelStitcher.resolve() + apply(), step for step; t_max below T exercises the guards (the result is then refused)
static bool stitch_host(const Vol& v, int bz, int by, int bx, int conn, int threads, int t_slack, std::vector<int>& out, int* num) {
  const StitchGrid g = stitch_grid(v.Z, v.Y, v.X, bz, by, bx);
  const int nb = (int)stitch_blocks(g);
  std::vector<std::vector<int32_t>> labels(nb);
  std::vector<StitchBlock> blocks(nb);
  std::vector<int32_t> nums(nb);
  for (int b = 0; b < nb; ++b) {                                   // every block labelled on its own
    const int i = b / (g.nby * g.nbx), j = (b / g.nbx) % g.nby, k = b % g.nbx;
    const int ez = stitch_extent(i, bz, v.Z), ey = stitch_extent(j, by, v.Y), ex = stitch_extent(k, bx, v.X);
    Vol part(ez, ey, ex);
    for (int z = 0; z < ez; ++z)
      for (int y = 0; y < ey; ++y)
        for (int x = 0; x < ex; ++x) part.at(z, y, x) = v.get(i * bz + z, j * by + y, k * bx + x);
    int n = 0;
    const std::vector<int> lab = flood_fill(part, conn, &n);
    labels[b].assign(lab.begin(), lab.end());
    nums[b] = n;
    blocks[b] = StitchBlock{labels[b].data(), i * bz, j * by, k * bx, ez, ey, ex};
  }
  std::vector<int64_t> offs(nb + 1, 0);                            // begin
  for (int b = 0; b < nb; ++b) offs[b + 1] = offs[b] + std::max(nums[b], 0);
  const int64_t T = offs[nb];
  const int t_max = (int)std::max<int64_t>(1, T + t_slack);
  const bool overflow = T > t_max;
  std::unique_ptr<std::atomic<int>[]> parent(new std::atomic<int>[t_max + 1]);
  std::vector<int64_t> first(t_max + 1, ST_NONE), key(t_max + 1, ST_NONE);
  for (int q = 0; q <= t_max; ++q) parent[q].store(q);
  const HostMem m{parent.get()};
  const StitchView view{blocks.data(), nums.data(), offs.data(), t_max};
  for (int b = 0; b < nb; ++b) {                                   // first: run heads only
    const StitchBlock& B = blocks[b];
    for (int z = 0; z < B.ez; ++z)
      for (int y = 0; y < B.ey; ++y)
        for (int x = 0; x < B.ex; ++x) {
          const int l = B.labels[((size_t)z * B.ey + y) * B.ex + x];
          if (x > 0 && l == B.labels[((size_t)z * B.ey + y) * B.ex + x - 1]) continue;
          const int gid = stitch_gid(view, b, l);
          if (gid) first[gid] = std::min(first[gid], ((int64_t)(B.z0 + z) * v.Y + (B.y0 + y)) * v.X + (B.x0 + x));
        }
  }
  const int64_t shell = stitch_shell_count(std::min(bz, v.Z), std::min(by, v.Y), std::min(bx, v.X));   // shell: the kernel's thread grid
  parallel_for(threads, shell * nb, [&](int64_t q) {
    const int b = (int)(q / shell);
    const int64_t t = q % shell;
    const StitchBlock& B = blocks[b];
    if (t >= stitch_shell_count(B.ez, B.ey, B.ex)) return;
    int z, y, x;
    stitch_shell_voxel(t, B.ez, B.ey, B.ex, z, y, x);
    stitch_touch_voxel(m, g, view, conn, b, z, y, x);
  });
  const int top = (int)std::min<int64_t>(T, t_max);                // resolve
  parallel_for(threads, top, [&](int64_t q) {
    const int gid = (int)q + 1;
    const int r = lbl_find(m, gid);
    if (r != gid) parent[gid].store(r, std::memory_order_relaxed);
  });
  for (int gid = 1; gid <= top; ++gid)
    if (first[gid] != ST_NONE) key[m.load(gid)] = std::min(key[m.load(gid)], first[gid]);
  std::vector<int> order(t_max + 1), map(t_max + 1, 0);            // rank the roots by key
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b]; });
  int M = 0;
  for (int q = 0; q <= t_max; ++q)
    if (key[order[q]] != ST_NONE) map[order[q]] = ++M;
  for (int gid = 1; gid <= top; ++gid) map[gid] = map[m.load(gid)];      // a root reads its own entry
  *num = overflow ? -1 : M;
  out.assign(v.n(), 0);
  for (int b = 0; b < nb; ++b) {                                   // apply, written back to the whole volume
    const StitchBlock& B = blocks[b];
    for (int z = 0; z < B.ez; ++z)
      for (int y = 0; y < B.ey; ++y)
        for (int x = 0; x < B.ex; ++x) {
          const int l = B.labels[((size_t)z * B.ey + y) * B.ex + x];
          const int gid = stitch_gid(view, b, l);
          out[((size_t)(B.z0 + z) * v.Y + (B.y0 + y)) * v.X + (B.x0 + x)] = overflow ? l : (gid ? map[gid] : 0);
        }
  }
  return !overflow;
}

static void check(const std::string& name, const Vol& v, const std::vector<std::vector<int>>& grids) {
  for (int conn = 1; conn <= 3; ++conn) {
    int want_n = 0;
    const std::vector<int> want = flood_fill(v, conn, &want_n);
    for (const auto& b : grids)
      for (int threads : {1, 4}) {
        int got_n = -2;
        std::vector<int> got;
        stitch_host(v, b[0], b[1], b[2], conn, threads, 0, got, &got_n);
        if (got_n != want_n || got != want) {
          ++failures;
          std::printf("MISMATCH %s conn %d blocks %d x %d x %d threads %d: M %d, expected %d\n", name.c_str(), conn, b[0], b[1], b[2], threads, got_n, want_n);
        }
        if (want_n > 1 && threads == 4) {                          // one id too many for the table: refused, and no guard lets an index past t_max through
          if (stitch_host(v, b[0], b[1], b[2], conn, threads, -1, got, &got_n) || got_n != -1) {
            ++failures;
            std::printf("MISMATCH %s conn %d blocks %d x %d x %d: the overflow was not reported\n", name.c_str(), conn, b[0], b[1], b[2]);
          }
        }
      }
    std::printf("%-28s %2d x %3d x %3d  conn %d  M = %d\n", name.c_str(), v.Z, v.Y, v.X, conn, want_n);
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
      if ((z / 2) % 2 == 0) v.at(z + 1, 2 * R, R % 2 == 0 ? X - 1 : 0) = 1;
      else v.at(z + 1, 0, 0) = 1;
    }
  }
  return v;
}

int main() {
  for (int ez : {1, 2, 3, 5})
    for (int ey : {1, 2, 4})
      for (int ex : {1, 2, 3, 7}) check_shell(ez, ey, ex);
  const int Z = 13, Y = 21, X = 70;
  const std::vector<std::vector<int>> grids = {{5, 8, 33}, {1, 8, 33}, {4, 21, 70}, {13, 21, 70}, {13, 1, 70}, {5, 8, 1}, {6, 7, 35}, {100, 100, 100}};
  { Vol v(Z, Y, X); check("all zero", v, grids); }
  { Vol v(Z, Y, X); std::fill(v.m.begin(), v.m.end(), 255); check("all one", v, grids); }
  { Vol v(Z, Y, X); v.m.back() = 2; check("last voxel", v, grids); }
  { Vol v(Z, Y, X); for (int z = 0; z < Z; ++z) for (int y = 0; y < Y; ++y) for (int x = 0; x < X; ++x) v.at(z, y, x) = (z + y + x) & 1; check("checkerboard", v, grids); }
  check("boustrophedon", snake(Z, Y, X), grids);
  { Vol v(Z, Y, X);
    v.at(4, 7, 32) = v.at(5, 8, 33) = 1;        // corner pair across a block corner of 5 x 8 x 33
    v.at(4, 15, 10) = v.at(5, 16, 10) = 1;      // edge pair across a block edge (z, y)
    v.at(3, 7, 33) = v.at(3, 8, 32) = 1;        // edge pair whose backward neighbour (0, -1, +1) leaves through the high x face
    v.at(9, 3, 65) = v.at(10, 3, 66) = 1;       // edge pair (z, x)
    v.at(9, 12, 66) = v.at(10, 12, 65) = 1;     // the same, other diagonal
    v.at(9, 16, 33) = v.at(10, 15, 32) = 1;     // corner pair, other diagonals
    check("pairs across block borders", v, grids); }
  { Vol v(Z, Y, X);                             // first voxel in a later block than the smallest id
    for (int x = 30; x <= 33; ++x) v.at(0, 8, x) = 1;
    v.at(1, 8, 33) = v.at(1, 7, 33) = v.at(0, 0, 0) = v.at(0, 8, 5) = v.at(0, 9, 0) = v.at(0, 20, 5) = v.at(1, 0, 50) = 1;
    check("first voxel in later block", v, grids); }
  std::mt19937 rng(0);
  std::uniform_real_distribution<float> uni(0.f, 1.f);
  const int shapes[][3] = {{13, 21, 70}, {3, 70, 300}, {1, 33, 70}, {5, 1, 1}, {1, 1, 300}};
  const std::vector<std::vector<int>> small = {{5, 8, 33}, {2, 33, 130}, {1, 8, 33}, {1, 1, 7}};
  for (const auto& s : shapes)
    for (float p : {0.2f, 0.32f, 0.5f, 0.7f}) {
      Vol v(s[0], s[1], s[2]);
      for (auto& b : v.m) b = uni(rng) < p ? 1 : 0;
      check("random p=" + std::to_string(p).substr(0, 4), v, small);
    }
  if (failures) std::printf("FAILED: %d mismatches\n", failures);
  else std::printf("all masks agree with the flood fill\n");
  return failures ? 1 : 0;
}
