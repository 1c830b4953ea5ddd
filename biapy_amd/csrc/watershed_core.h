// The steps of the seeded watershed (watershed.hip): the order-preserving keys, the enumeration of a voxel's forward neighbours, and one function
// per launch - init, pick, resolve, unite, flatten, last - each the work of ONE voxel.  Compiles for the device (watershed.hip wraps each in a
// kernel) and for the host (scripts/watershed_cpu_check.cpp runs the same code sequentially and on std::atomic under std::thread).  Find and unite
// are label_uf.h's, with their termination arguments.  The memory is reached through a policy `M`:
//   int      load(int i) / amin(int i, int v) / pstore(int i, int v)     the parents P (load and amin as label_uf.h asks for them)
//   uint64_t bload(int i) / bmin(int i, uint64_t k) / bstore(int i, k)    best[i]: relaxed read, atomic min (value before not needed), store
//   int      oload(int i) / ostore(int i, int v)                         out[i]: the label a root carries, at the end the result
//   bool     flagged(int r) / flag(int r)                                the round flags
// and the image through `I` with  uint32_t key(int i)  - the order-preserving key of voxel i's value.
//
// THE CONTRACT (include/biapy_amd.h, prepost.watershed): nodes = voxels inside the mask; edges = pairs of nodes that are neighbours at the
// connectivity; weight = max(key(u), key(v)); strict total order of the edges = (weight, linear index of the raster-first endpoint u, rank of the
// offset among u's forward offsets in (dz, dy, dx) lexicographic order); a voxel with marker > 0 inside the mask is SEEDED.  The result is the
// unique minimum spanning forest in which no tree holds two seeded voxels' groups: Kruskal over the edges in that order, joining two trees unless
// they are the same or both hold a seed.  Every voxel takes the marker of its tree's seed, 0 when the tree has none or the voxel is masked out.
//
// STATE: P parents (flat - every entry a root - between rounds; LBL_BG outside the mask, so no pass but init reads the mask); out[root] the label of
// the root's tree, 0 while it has none (a nonzero entry of ANY voxel equals its tree's label, because trees with different labels never join:
// refreshing a root's label is a plain store on whose value every writer agrees); best[root] the tree's pick, key = weight << 31 | u < 2^63.
// ROUND r (Boruvka): pick - every voxel of an unseeded tree offers its cheapest edge into another tree, one 64-bit atomic min per voxel that has one;
// resolve - the root decodes (weight, u) and walks u's forward offsets for the first edge of that weight that leaves its tree (the rank, which the
// key does not hold); unite; flatten - P[v] = root, the label moves to the new root, best is reset.  A seeded tree never picks, an unseeded tree
// picks one edge: following the picks ends at a seeded tree or at a mutual pair, so a group that joins holds at most one seed, and every edge
// picked is the cheapest across a cut, hence an edge of the forest.  The unseeded trees that still have a way out at least halve per round:
// ws_rounds(n) = ceil(log2(max(n, 2))) + 1 rounds always suffice.  Round r's pick sets flag r + 1 when it picked anything; a round whose
// predecessor picked nothing has nothing to do.  Flag 0 says that the volume holds a seed at all (without one every voxel is 0: no round runs).
#pragma once
#include "label_uf.h"

#define WS_NONE (~(uint64_t)0)     // best[i]: no pick.  Above every key (keys are below 2^63) and every root index

struct WsGeom { int Z, Y, X, conn; };

LBL_HD uint32_t ws_okey_i32(uint32_t bits) { return bits ^ 0x80000000u; }                                     // v + 2^31
LBL_HD uint32_t ws_okey_f32(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }    // -0.0 < +0.0; NaN unspecified

struct WsImage {       // float32 and int32 values are both read as their 32 bits
  const uint32_t* bits;
  int is_f32;
  LBL_HD uint32_t key(int i) const { return is_f32 ? ws_okey_f32(bits[i]) : ws_okey_i32(bits[i]); }
};

// ceil(log2(max(n, 2))) + 1.  LOOP BOUND: b < 31 steps for n < 2^31.
LBL_HD int ws_rounds(int64_t n) {
  int b = 1;
  while (((int64_t)1 << b) < n) ++b;
  return b + 1;
}

// The FORWARD half of a voxel's neighbourhood at connectivity `conn`, in (dz, dy, dx) lexicographic order: (0,0,1), (0,1,-1), (0,1,0), (0,1,1),
// (1,-1,-1) ... (1,1,1) - the order that ranks the edges of one raster-first endpoint.  f returns true to stop.  LOOP BOUND: 13 calls.
template <class F> LBL_HD void ws_for_forward(int conn, F&& f) {
  for (int dz = 0; dz <= 1; ++dz)
    for (int dy = dz ? -1 : 0; dy <= 1; ++dy)
      for (int dx = (dz || dy) ? -1 : 1; dx <= 1; ++dx) {
        if ((dz != 0) + (dy != 0) + (dx != 0) > conn) continue;
        if (f(dz, dy, dx)) return;
      }
}

// linear index of the neighbour of (z, y, x) at the offset, -1 outside the volume
LBL_HD int ws_neighbour(const WsGeom& g, int z, int y, int x, int dz, int dy, int dx) {
  const int nz = z + dz, ny = y + dy, nx = x + dx;
  if ((uint32_t)nz >= (uint32_t)g.Z || (uint32_t)ny >= (uint32_t)g.Y || (uint32_t)nx >= (uint32_t)g.X) return -1;
  return (nz * g.Y + ny) * g.X + nx;        // a voxel of the volume: < n < 2^31
}

template <class M> LBL_HD void ws_init(const M& m, int v, bool masked, int marker) {
  const int l = (masked && marker > 0) ? marker : 0;
  m.pstore(v, masked ? v : LBL_BG);
  m.ostore(v, l);
  m.bstore(v, WS_NONE);
  if (l && !m.flagged(0)) m.flag(0);                    // one store per wave or so, not one per seeded voxel on a single address
}

// pick, round `round`: P is flat and nobody writes it.  Reads the flag of the round before outside (the kernel's early return).
template <class M, class I> LBL_HD void ws_pick(const M& m, const WsGeom& g, const I& img, int v, int round) {
  const int r = m.load(v);
  if (r < 0 || m.oload(r) != 0) return;                 // outside the mask, or the tree has its seed
  const int x = v % g.X, zy = v / g.X, y = zy % g.Y, z = zy / g.Y;
  const uint32_t kv = img.key(v);
  uint64_t best = WS_NONE;
  auto see = [&](int dz, int dy, int dx) {
    const int nb = ws_neighbour(g, z, y, x, dz, dy, dx);
    if (nb < 0) return false;
    const int pn = m.load(nb);
    if (pn < 0 || pn == r) return false;                // masked out, or the same tree
    const uint32_t kn = img.key(nb);
    const uint64_t key = ((uint64_t)(kv > kn ? kv : kn) << 31) | (uint32_t)(v < nb ? v : nb);
    if (key < best) best = key;
    return false;
  };
  ws_for_forward(g.conn, see);
  ws_for_forward(g.conn, [&](int dz, int dy, int dx) { return see(-dz, -dy, -dx); });
  if (best == WS_NONE) return;
  if (best < m.bload(r)) m.bmin(r, best);               // best[r] only falls during the pass: a stale read costs an atomic, never a pick
  if (!m.flagged(round + 1)) m.flag(round + 1);         // as in init: a flag that is up is not stored again
}

// resolve: reads P only, so every root it sees is the root as of the round's start.  best[r]: the key -> the root to unite with.
template <class M, class I> LBL_HD void ws_resolve(const M& m, const WsGeom& g, const I& img, int r) {
  const uint64_t key = m.bload(r);
  if (key == WS_NONE) return;                           // only the roots of unseeded trees that picked hold anything else
  const uint32_t w = (uint32_t)(key >> 31);
  const int u = (int)(key & 0x7fffffffu);
  const int x = u % g.X, zy = u / g.X, y = zy % g.Y, z = zy / g.Y;
  const uint32_t ku = img.key(u);
  const int pu = m.load(u);
  uint64_t target = WS_NONE;
  ws_for_forward(g.conn, [&](int dz, int dy, int dx) {
    const int nb = ws_neighbour(g, z, y, x, dz, dy, dx);
    if (nb < 0) return false;
    const int pn = m.load(nb);
    if (pn < 0) return false;
    const uint32_t kn = img.key(nb);
    if ((ku > kn ? ku : kn) != w || (pu == r) == (pn == r)) return false;     // another weight, or not an edge that leaves the tree
    target = (uint32_t)(pu == r ? pn : pu);
    return true;
  });
  m.bstore(r, target);
}

// unite: decided by best alone (P changes under this pass's feet).  Mutual picks unite twice, harmlessly.
template <class M> LBL_HD void ws_unite(const M& m, int v) {
  const uint64_t t = m.bload(v);
  if (t != WS_NONE) lbl_unite(m, v, (int)t);
}

// flatten: entries change under other threads' feet only from an ancestor to the root itself, and roots do not change, so every find ends at
// the true root (label_uf.h: the bound of the walk)
template <class M> LBL_HD void ws_flatten(const M& m, int v) {
  const int p = m.load(v);
  if (p < 0) return;
  const int r = lbl_find(m, v);
  if (r != p) m.pstore(v, r);
  const int l = m.oload(v);
  if (l != 0 && r != v && m.oload(r) == 0) m.ostore(r, l);     // every writer of out[r] writes this same label
  if (m.bload(v) != WS_NONE) m.bstore(v, WS_NONE);
}

// the last pass: every voxel writes its own entry only; a root rewrites its own label
template <class M> LBL_HD void ws_last(const M& m, int v) {
  const int p = m.load(v);
  m.ostore(v, p < 0 ? 0 : m.oload(p));
}

// number of rounds that picked anything
template <class M> LBL_HD int ws_rounds_used(const M& m, int R) {
  int used = 0;
  for (int r = 1; r <= R; ++r) used += m.flagged(r) ? 1 : 0;     // LOOP BOUND: R <= 32
  return used;
}
