// Host run of the seeded watershed of biapy_amd/csrc/watershed.hip: the same steps (csrc/watershed_core.h: init, pick, resolve, unite, flatten, last) on
// the same union-find (csrc/label_uf.h) in the launch sequence of bpx_watershed - R = ws_rounds(n) rounds whatever the data - sequentially and with
// every pass spread over std::threads on std::atomic, checked against the statement of the contract: Kruskal over the edges sorted by (weight,
// raster-first endpoint, rank of the forward offset), joining two trees unless they are the same or both seeded.  Random volumes with heavy ties
// (1, 2, 4 and 1000 image levels), both dtypes, masks, repeated labels, long one-voxel-wide paths.  A development aid for finding an unbounded
// loop, an off-by-one at a volume edge or a round bound that does not hold before the kernels run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -I biapy_amd/csrc scripts/watershed_cpu_check.cpp -o watershed_cpu_check
//   ./watershed_cpu_check
// Prints one line per volume and exits nonzero on the first mismatch.  Not loaded into Python, not part of the test suite.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "watershed_core.h"

struct HostMem {
  std::atomic<int>* P;
  std::atomic<uint64_t>* best;
  std::atomic<int>* out;
  std::atomic<int>* act;
  int load(int i) const { return P[i].load(std::memory_order_relaxed); }
  int amin(int i, int v) const {
    int cur = P[i].load(std::memory_order_relaxed);
    while (v < cur && !P[i].compare_exchange_weak(cur, v, std::memory_order_relaxed)) {}
    return cur;
  }
  void pstore(int i, int v) const { P[i].store(v, std::memory_order_relaxed); }
  uint64_t bload(int i) const { return best[i].load(std::memory_order_relaxed); }
  void bmin(int i, uint64_t k) const {
    uint64_t cur = best[i].load(std::memory_order_relaxed);
    while (k < cur && !best[i].compare_exchange_weak(cur, k, std::memory_order_relaxed)) {}
  }
  void bstore(int i, uint64_t k) const { best[i].store(k, std::memory_order_relaxed); }
  int oload(int i) const { return out[i].load(std::memory_order_relaxed); }
  void ostore(int i, int v) const { out[i].store(v, std::memory_order_relaxed); }
  bool flagged(int r) const { return act[r].load(std::memory_order_relaxed) != 0; }
  void flag(int r) const { act[r].store(1, std::memory_order_relaxed); }
};

struct Vol {
  int Z, Y, X, f32;
  std::vector<uint32_t> img;       // the 32 bits of the float32 / int32 values
  std::vector<int> markers;
  std::vector<uint8_t> mask;
  Vol(int z, int y, int x, int f) : Z(z), Y(y), X(x), f32(f), img((size_t)z * y * x, 0), markers(img.size(), 0), mask(img.size(), 1) {}
  int n() const { return Z * Y * X; }
};

static uint32_t bits_of(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

static void parallel_for(int threads, int count, const std::function<void(int)>& f) {   // item q runs on thread q % threads: neighbours on different threads
  if (threads <= 1) { for (int q = 0; q < count; ++q) f(q); return; }
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([=, &f] { for (int q = t; q < count; q += threads) f(q); });
  for (auto& th : pool) th.join();
}

// the launch sequence of bpx_watershed, step for step
static std::vector<int> watershed_host(const Vol& v, int conn, int threads, int* rounds) {
  const int n = v.n(), R = ws_rounds(n);
  std::unique_ptr<std::atomic<int>[]> P(new std::atomic<int>[n]), out(new std::atomic<int>[n]), act(new std::atomic<int>[R + 2]);
  std::unique_ptr<std::atomic<uint64_t>[]> best(new std::atomic<uint64_t>[n]);
  const HostMem m{P.get(), best.get(), out.get(), act.get()};
  const WsGeom g{v.Z, v.Y, v.X, conn};
  const WsImage img{v.img.data(), v.f32};
  for (int r = 0; r <= R + 1; ++r) act[r].store(0);
  parallel_for(threads, n, [&](int i) { ws_init(m, i, v.mask[i] != 0, v.markers[i]); });
  for (int r = 0; r < R; ++r) {
    if (m.flagged(r)) parallel_for(threads, n, [&](int i) { ws_pick(m, g, img, i, r); });
    if (!m.flagged(r + 1)) continue;
    parallel_for(threads, n, [&](int i) { ws_resolve(m, g, img, i); });
    parallel_for(threads, n, [&](int i) { ws_unite(m, i); });
    parallel_for(threads, n, [&](int i) { ws_flatten(m, i); });
  }
  // one more pick must find nothing: R rounds sufficed
  if (m.flagged(R)) {
    for (int i = 0; i < n; ++i) ws_pick(m, g, img, i, R);               // flag R + 1: the spare entry
    if (m.flagged(R + 1)) { std::printf("ROUND BOUND: a tree still picks after R = %d rounds\n", R); *rounds = -1; return {}; }
  }
  *rounds = ws_rounds_used(m, R);
  parallel_for(threads, n, [&](int i) { ws_last(m, i); });
  std::vector<int> lab(n);
  for (int i = 0; i < n; ++i) lab[i] = m.oload(i);
  return lab;
}

// the statement: Kruskal in the strict order, joining unless the trees are the same or both seeded
static std::vector<int> kruskal(const Vol& v, int conn) {
  const int n = v.n();
  const WsGeom g{v.Z, v.Y, v.X, conn};
  const WsImage img{v.img.data(), v.f32};
  std::vector<std::tuple<uint32_t, int, int, int>> edges;     // weight, u, rank, other endpoint
  for (int u = 0; u < n; ++u) {
    if (!v.mask[u]) continue;
    const int x = u % v.X, y = (u / v.X) % v.Y, z = u / v.X / v.Y;
    int rank = 0;
    ws_for_forward(conn, [&](int dz, int dy, int dx) {
      const int nb = ws_neighbour(g, z, y, x, dz, dy, dx);
      if (nb >= 0 && v.mask[nb]) edges.emplace_back(std::max(img.key(u), img.key(nb)), u, rank, nb);
      ++rank;
      return false;
    });
  }
  std::sort(edges.begin(), edges.end());
  std::vector<int> parent(n), label(n, 0);
  for (int i = 0; i < n; ++i) { parent[i] = i; label[i] = (v.mask[i] && v.markers[i] > 0) ? v.markers[i] : 0; }
  auto find = [&](int i) { while (parent[i] != i) { parent[i] = parent[parent[i]]; i = parent[i]; } return i; };
  for (const auto& e : edges) {
    const int a = find(std::get<1>(e)), b = find(std::get<3>(e));
    if (a == b || (label[a] && label[b])) continue;
    parent[a] = b;
    if (label[a]) label[b] = label[a];
  }
  std::vector<int> lab(n, 0);
  for (int i = 0; i < n; ++i) if (v.mask[i]) lab[i] = label[find(i)];
  return lab;
}

static int failures = 0;

static void check(const std::string& name, const Vol& v, int max_conn = 3) {
  for (int conn = 1; conn <= max_conn; ++conn) {
    const std::vector<int> want = kruskal(v, conn);
    int used = 0;
    for (int threads : {1, 4}) {
      int rounds = 0;
      const std::vector<int> got = watershed_host(v, conn, threads, &rounds);
      if (got != want || rounds < 0 || rounds > ws_rounds(v.n())) {
        ++failures;
        std::printf("MISMATCH %s conn %d threads %d (rounds %d)\n", name.c_str(), conn, threads, rounds);
      }
      used = rounds;
    }
    int assigned = 0;
    for (int l : want) assigned += l != 0;
    std::printf("%-34s %2d x %3d x %3d  conn %d  rounds %2d of %2d  %d voxels labelled\n", name.c_str(), v.Z, v.Y, v.X, conn, used, ws_rounds(v.n()), assigned);
  }
}

// a one-voxel-wide boustrophedon path through plane 0: the long chain for the round bound
static Vol snake(int Y, int X, int f32, std::vector<int>* order) {
  Vol v(1, Y, X, f32);
  std::fill(v.mask.begin(), v.mask.end(), 0);
  const int rows = (Y - 1) / 2;
  for (int r = 0; r <= rows; ++r) {
    for (int q = 0; q < X; ++q) order->push_back((2 * r) * X + (r % 2 == 0 ? q : X - 1 - q));
    if (r < rows) order->push_back((2 * r + 1) * X + (r % 2 == 0 ? X - 1 : 0));
  }
  for (int i : *order) v.mask[i] = 1;
  return v;
}

int main() {
  std::mt19937 rng(0);
  std::uniform_real_distribution<float> uni(0.f, 1.f);
  const int shapes[][3] = {{9, 21, 37}, {8, 16, 64}, {1, 33, 70}, {5, 1, 1}, {1, 1, 300}, {3, 4, 5}, {6, 6, 6}};
  for (const auto& s : shapes)
    for (int levels : {1, 2, 4, 1000})
      for (int f32 = 0; f32 <= 1; ++f32)
        for (float keep : {0.6f, 0.9f, 1.0f})
          for (float seeds : {0.01f, 0.1f}) {
            Vol v(s[0], s[1], s[2], f32);
            for (int i = 0; i < v.n(); ++i) {
              const int q = (int)(uni(rng) * levels) - levels / 2;
              v.img[i] = f32 ? bits_of(0.25f * (float)q) : (uint32_t)q;
              v.mask[i] = uni(rng) < keep ? 1 : 0;
              v.markers[i] = uni(rng) < seeds ? 1 + (int)(uni(rng) * 5) : (uni(rng) < 0.02f ? -3 : 0);     // repeated labels, some negative
            }
            check("random L" + std::to_string(levels) + (f32 ? " f32" : " i32") + " m" + std::to_string(keep).substr(0, 3) + " s" + std::to_string(seeds).substr(0, 4), v);
          }
  { Vol v(4, 9, 11, 0); check("no marker", v); }
  { Vol v(4, 9, 11, 0); v.markers[17] = 7; check("one marker", v); }
  { Vol v(4, 9, 11, 1); for (int i = 0; i < v.n(); ++i) v.markers[i] = 1 + i % 3; check("every voxel a marker", v); }
  { Vol v(1, 1, 21, 0); v.markers[0] = 1; v.markers[20] = 2; check("flat line, seeds at the ends", v, 1); }
  { Vol v(1, 1, 21, 1);
    v.img = {bits_of(-0.0f), bits_of(0.0f), bits_of(-INFINITY), bits_of(INFINITY), bits_of(1e-45f), bits_of(-1e-45f), bits_of(0.0f), bits_of(-0.0f), bits_of(1e-40f),
             bits_of(0.0f), bits_of(-0.0f), bits_of(-0.0f), bits_of(0.0f), bits_of(3.f), bits_of(-3.f), bits_of(0.f), bits_of(-0.f), bits_of(1e-45f), bits_of(0.f),
             bits_of(-0.f), bits_of(0.f)};
    v.markers[0] = 1; v.markers[20] = 2; v.markers[10] = 3;
    check("signed zeros, infinities, denormals", v, 1); }
  for (int f32 = 0; f32 <= 1; ++f32) {
    std::vector<int> order;
    Vol v = snake(41, 150, f32, &order);
    v.markers[order.back()] = 4;
    check("path, one seed at its end", v, 1);
    const int len = (int)order.size();
    for (int q = 0; q < len; ++q) {
      const int h = q < len / 2 ? q : len - 1 - q;                        // strictly up to the middle, strictly down after it
      v.img[order[q]] = f32 ? bits_of((float)h) : (uint32_t)h;
    }
    v.markers[order.front()] = 9;
    check("path, a seed at each end, a peak", v, 1);
  }
  if (failures) std::printf("FAILED: %d mismatches\n", failures);
  else std::printf("all volumes agree with Kruskal\n");
  return failures ? 1 : 0;
}
