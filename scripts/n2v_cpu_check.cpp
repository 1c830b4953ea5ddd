// Host run of the per-box arithmetic of the Noise2Void masker (biapy_amd/csrc/n2v.hip): the same code (csrc/n2v_core.h: n2v_box) over every box
// of adversarial shapes - axes of 1, extents below the box edge, radii above the extent, box edge 64, ragged last boxes - for the four
// manipulators, several samples, channels and counter values on both sides of 2^32.  For every box it asserts that
//   * coord and source are both -1 or both inside [0, Z Y X), and coord lies inside its own box;
//   * the source lies inside the clipped window around coord; uniform_withoutCP never picks coord; identity / normal_additive pick coord;
//   * the masked voxels of one (sample, channel) are distinct (a byte map of the sample between poisoned guard bytes is written through coord
//     and read through source: ASan stops an access outside);
//   * n2v_philox gives the Philox4x32-10 known answers of the Random123 test vectors.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I biapy_amd/csrc scripts/n2v_cpu_check.cpp -o n2v_cpu_check
//   ./n2v_cpu_check
// Prints one line per part and exits nonzero on the first mismatch.  Host only: never loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "n2v_core.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

#define REQUIRE(cond, ...)                       \
  do {                                           \
    if (!(cond)) {                               \
      std::fprintf(stderr, "FAILED: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");                \
      std::exit(1);                              \
    }                                            \
  } while (0)

static N2VGeom geom(int Z, int Y, int X, int s, int r, int manip) {
  N2VGeom g;
  g.Z = Z; g.Y = Y; g.X = X;
  g.sz = Z == 1 ? 1 : s; g.sy = Y == 1 ? 1 : s; g.sx = X == 1 ? 1 : s;
  g.rz = Z == 1 ? 0 : r; g.ry = Y == 1 ? 0 : r; g.rx = X == 1 ? 0 : r;
  g.nz = (Z + g.sz - 1) / g.sz; g.ny = (Y + g.sy - 1) / g.sy; g.nx = (X + g.sx - 1) / g.sx;
  g.manip = manip;
  return g;
}

int main() {
  {  // Random123's known answers of philox4x32_10
    uint32_t r[4];
    n2v_philox(0, 0, 0, 0, 0, 0, r);
    REQUIRE(r[0] == 0x6627e8d5u && r[1] == 0xe169c58du && r[2] == 0xbc57ac4cu && r[3] == 0x9b00dbd8u, "philox(0)");
    n2v_philox(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, r);
    REQUIRE(r[0] == 0x408f276du && r[1] == 0x41c83b0eu && r[2] == 0xa20bc7c6u && r[3] == 0x6d5451fdu, "philox(~0)");
    n2v_philox(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, r);
    REQUIRE(r[0] == 0xd16cfe09u && r[1] == 0x94fdccebu && r[2] == 0x5001e420u && r[3] == 0x24126ea1u, "philox(pi)");
    std::printf("philox: 3 known answers\n");
  }
  const int shapes[][3] = {{1, 1, 1}, {1, 1, 9}, {1, 7, 1}, {5, 1, 1}, {1, 45, 50}, {3, 5, 7}, {2, 2, 2}, {13, 22, 37}, {6, 7, 9}, {8, 8, 8}, {65, 3, 130}, {1, 64, 129}};
  const int edges[] = {1, 2, 3, 4, 8, 22, 63, 64};
  const int radii[] = {0, 1, 2, 5, 15};
  const uint64_t counters[] = {0ull, 1ull, 0xFFFFFFFFull, 0x100000000ull, 0xFFFFFFFFFFFFFFFFull};
  const size_t GUARD = 64;
  long long walked = 0, masked = 0;
  for (const auto& sh : shapes) {
    const int Z = sh[0], Y = sh[1], X = sh[2];
    const int64_t V = (int64_t)Z * Y * X;
    std::vector<unsigned char> buf(V + 2 * GUARD, 0);
    unsigned char* map = buf.data() + GUARD;
    POISON(buf.data(), GUARD);
    POISON(map + V, GUARD);
    for (int s : edges)
      for (int r : radii)
        for (int manip = 0; manip < 4; ++manip) {
          const N2VGeom g = geom(Z, Y, X, s, r, manip);
          const int64_t boxes = (int64_t)g.nz * g.ny * g.nx;
          for (int rep = 0; rep < 3; ++rep) {
            const uint64_t q = counters[(rep + s + r) % 5], seed = 0x9E3779B97F4A7C15ull * (uint64_t)(rep + 1) + (uint64_t)s;
            const uint32_t b = rep == 2 ? (1u << 24) - 1u : (uint32_t)rep, c = (uint32_t)((rep * 7) % 8);
            std::memset(map, 0, (size_t)V);
            for (int64_t i = 0; i < boxes; ++i) {
              const N2VPick pk = n2v_box(g, (uint32_t)seed ^ N2V_KEY_XOR, (uint32_t)(seed >> 32), (uint32_t)q, (uint32_t)(q >> 32), b, c, (uint32_t)i);
              ++walked;
              REQUIRE((pk.coord < 0) == (pk.source < 0), "coord %lld / source %lld disagree", (long long)pk.coord, (long long)pk.source);
              if (pk.coord < 0) {
                REQUIRE(pk.coord == -1 && pk.source == -1, "an unmasked box must report -1, -1");
                continue;
              }
              ++masked;
              REQUIRE(pk.coord < V && pk.source < V, "index out of the sample: %lld %lld of %lld", (long long)pk.coord, (long long)pk.source, (long long)V);
              const int pz = (int)(pk.coord / ((int64_t)Y * X)), py = (int)(pk.coord / X % Y), px = (int)(pk.coord % X);
              const int qz = (int)(pk.source / ((int64_t)Y * X)), qy = (int)(pk.source / X % Y), qx = (int)(pk.source % X);
              const int iz = (int)(i / ((int64_t)g.ny * g.nx)), iy = (int)(i / g.nx % g.ny), ix = (int)(i % g.nx);
              REQUIRE(pz / g.sz == iz && py / g.sy == iy && px / g.sx == ix, "the masked voxel left its box");
              REQUIRE(std::abs(qz - pz) <= g.rz && std::abs(qy - py) <= g.ry && std::abs(qx - px) <= g.rx, "the source left its window");
              if (manip == N2V_UNIFORM_WITHOUT_CP) REQUIRE(pk.source != pk.coord, "uniform_withoutCP picked the centre");
              if (manip >= N2V_IDENTITY) REQUIRE(pk.source == pk.coord, "identity / normal_additive must pick the voxel itself");
              REQUIRE(map[pk.coord] == 0, "one voxel masked twice");
              const volatile unsigned char* vmap = map;
              (void)vmap[pk.source];                                            // the read through source: ASan checks it
              map[pk.coord] = 1;
            }
            if (Z % g.sz == 0 && Y % g.sy == 0 && X % g.sx == 0 && !(manip == N2V_UNIFORM_WITHOUT_CP && r == 0)) {
              int64_t n = 0;
              for (int64_t v = 0; v < V; ++v) n += map[v];
              if (manip != N2V_UNIFORM_WITHOUT_CP || (V > 1)) {
                bool one_voxel_window = manip == N2V_UNIFORM_WITHOUT_CP && (g.rz == 0 || Z == 1) && (g.ry == 0 || Y == 1) && (g.rx == 0 || X == 1);
                if (!one_voxel_window) REQUIRE(n == boxes, "a divisible shape masks one voxel per box: %lld of %lld", (long long)n, (long long)boxes);
              }
            }
          }
        }
    UNPOISON(buf.data(), GUARD);
    UNPOISON(map + V, GUARD);
  }
  std::printf("n2v_box: %lld boxes walked, %lld masked, every index in range\n", walked, masked);
  return 0;
}
