// Union-find over linear voxel indices for connected-component labelling (label.hip): find, unite and the enumeration of the backward half
// of a voxel's neighbourhood.  Compiles for the device (label.hip) and for the host (scripts/label_cpu_check.cpp runs the same code
// sequentially and on std::atomic<int> under std::thread) - the memory is reached through a policy `M` with
//   int  load(int i)          relaxed read of parent[i]
//   int  amin(int i, int v)   atomic parent[i] = min(parent[i], v), returns the value before
//
// INVARIANT: parent[i] <= i at all times for every foreground voxel (it starts as i and is only ever lowered, by amin), parent[i] < 0 for
// background.  A read may be stale (another compute die's cache): a stale value is an EARLIER value of parent[i], which also is <= i and
// also lies in i's component, so stale reads cost retries and never a wrong answer - the decision itself is taken by the atomic, on the
// one true value.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LBL_HD __host__ __device__ __forceinline__
#else
#define LBL_HD inline
#endif

#define LBL_BG INT32_MIN          // parent / label of a background voxel until the last pass writes 0
constexpr int LBL_TZ = 8, LBL_TY = 8, LBL_TX = 64;   // the tile of the tiled merge: X innermost, one 64-byte mask row per wave load
constexpr int LBL_TV = LBL_TZ * LBL_TY * LBL_TX;
constexpr int LBL_CHUNK = 4096;   // voxels per numbering chunk (roots are counted, scanned and ranked per chunk)

// Root of i.  TERMINATION: the loop continues only while 0 <= p < i, so i strictly decreases over non-negative integers: at most
// (start index) steps whatever the other threads do and whatever is read (a root p == i, a background marker p < 0 and a value p > i
// that the invariant excludes all end it).
template <class M> LBL_HD int lbl_find(const M& m, int i) {
  int p = m.load(i);
  while ((uint32_t)p < (uint32_t)i) {
    i = p;
    p = m.load(i);
  }
  return i;
}

// Joins the sets of a and b: the larger root is hung under the smaller with one atomic min.  `old == a` says that a still was a root and
// now points at b: done.  Otherwise another thread had lowered parent[a] to old < a before us; the min has left parent[a] = min(old, b),
// which keeps a joined to the smaller of the two, and what remains to be recorded is old ~ b: continue with that pair.  (When old > b
// the entry of the NON-root a moves from old to b; the link a ~ old it held is restored by the pair the loop goes on with.)
// TERMINATION: each retry replaces a = max(a, b) by old < a while b < a stays, so max(a, b) strictly decreases over non-negative
// integers: at most max(a, b) retries whatever the interleaving.  `old >= a` (as unsigned: a negative value too) ends the loop, so a
// value the invariant excludes cannot keep it alive.
template <class M> LBL_HD void lbl_unite(const M& m, int a, int b) {
  a = lbl_find(m, a);
  b = lbl_find(m, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = m.amin(a, b);
    if ((uint32_t)old >= (uint32_t)a) break;
    a = old;
  }
}

// The BACKWARD half of a voxel's neighbourhood - the neighbours of connectivity `conn` (1 faces, 2 + edges, 3 + corners) that come before
// the voxel in raster order: 3 / 9 / 13 offsets.  A voxel united with these alone is united with every neighbour, because the forward
// ones do it from their side.  fg(dz, dy, dx) says whether that neighbour exists and is foreground; f(dz, dy, dx) is called for the
// neighbours to unite with.  The offsets form three groups, each around a face neighbour: the row (0, 0, -1); the row above, around
// (0, -1, 0); the plane below, around (-1, 0, 0).  WHEN A GROUP'S CENTRE IS FOREGROUND, THE CENTRE ALONE IS TAKEN: every other member of
// the group is a neighbour of the centre (at the same connectivity) inside a SIMPLER group of the later of the two - a member of the
// plane group sits in the centre's row-above group or row, a member of the row-above group in the centre's row - so that pair is united
// from there, the chain of reliances ends at the one-member row group, and the components are the same.  In solid regions this turns 13
// unions per voxel into 3.
// The plane below goes first: its members have the smallest indices, and a voxel hung under a far-away small root first keeps the trees flat
// (measured: row first cost the global-only merge 20 % at connectivity 1).
template <class FG, class F> LBL_HD void lbl_for_backward(int conn, FG&& fg, F&& f) {
  if (fg(-1, 0, 0)) f(-1, 0, 0);
  else if (conn >= 2) {
    if (fg(-1, -1, 0)) f(-1, -1, 0);
    if (fg(-1, 0, -1)) f(-1, 0, -1);
    if (fg(-1, 0, 1)) f(-1, 0, 1);
    if (fg(-1, 1, 0)) f(-1, 1, 0);
    if (conn >= 3) {
      if (fg(-1, -1, -1)) f(-1, -1, -1);
      if (fg(-1, -1, 1)) f(-1, -1, 1);
      if (fg(-1, 1, -1)) f(-1, 1, -1);
      if (fg(-1, 1, 1)) f(-1, 1, 1);
    }
  }
  if (fg(0, -1, 0)) f(0, -1, 0);
  else if (conn >= 2) {
    if (fg(0, -1, -1)) f(0, -1, -1);
    if (fg(0, -1, 1)) f(0, -1, 1);
  }
  if (fg(0, 0, -1)) f(0, 0, -1);
}

// does the neighbour at offset (dz, dy, dx) of the voxel at tile-local (lz, ly, lx) lie in another tile?
LBL_HD bool lbl_leaves_tile(int lz, int ly, int lx, int dz, int dy, int dx) {
  return (uint32_t)(lz + dz) >= (uint32_t)LBL_TZ || (uint32_t)(ly + dy) >= (uint32_t)LBL_TY || (uint32_t)(lx + dx) >= (uint32_t)LBL_TX;
}

LBL_HD int64_t lbl_chunks(int64_t n) { return (n + LBL_CHUNK - 1) / LBL_CHUNK; }
