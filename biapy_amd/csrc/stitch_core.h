// Stitching of per-block label volumes (stitch.hip): the grid of blocks, the enumeration of a block's shell, the lookup of a neighbour by global
// coordinate and the two uniting rules, over a union-find on LABEL IDS (label_uf.h, unchanged) instead of voxels.  Compiles for the device
// (stitch.hip) and for the host (scripts/stitch_cpu_check.cpp runs the same code sequentially and on std::atomic<int> under std::thread).
//
// A volume (Z, Y, X) is cut by a regular grid of blocks (bz, by, bx), the last block of an axis may be ragged; block (i, j, k) covers
// [i bz, min((i + 1) bz, Z)) and likewise in y and x; blocks are numbered in raster order of (i, j, k).  Block b is a contiguous int32 array of
// its own with local labels 1..n_b (a label <= 0 or > n_b is background); off_b is the exclusive prefix sum of the n_b; the GLOBAL ID of (b, l)
// is off_b + l, in 1..T; the table parent[0..t_max] starts as the identity and keeps parent[g] <= g (lbl_unite hangs the larger root under the
// smaller by an atomic min), so label_uf.h's reasoning on stale reads holds as it stands.  An id above t_max takes part in nothing (the
// overflow flag is up then, and nothing is written back).
#pragma once
#include <stdint.h>

#include "label_uf.h"

#define ST_HD LBL_HD
#define ST_NONE INT64_MAX   // first[] / key[] of an id that no voxel carries

struct StitchGrid { int Z, Y, X, bz, by, bx, nbz, nby, nbx; };
struct StitchBlock { const int32_t* labels; int32_t z0, y0, x0, ez, ey, ex; };                    // the layout of bpx_stitch_block
struct StitchView { const StitchBlock* blocks; const int32_t* nums; const int64_t* offs; int t_max; };

ST_HD int stitch_cdiv(int a, int b) { return (int)(((int64_t)a + b - 1) / b); }
ST_HD StitchGrid stitch_grid(int Z, int Y, int X, int bz, int by, int bx) {
  return StitchGrid{Z, Y, X, bz, by, bx, stitch_cdiv(Z, bz), stitch_cdiv(Y, by), stitch_cdiv(X, bx)};
}
ST_HD int64_t stitch_blocks(const StitchGrid& g) { return (int64_t)g.nbz * g.nby * g.nbx; }
ST_HD int stitch_extent(int i, int b, int N) {        // extent of the i-th block of an axis of N voxels cut every b
  const int64_t lo = (int64_t)i * b, hi = lo + b;
  return (int)((hi < N ? hi : (int64_t)N) - lo);
}
ST_HD int stitch_block_of(const StitchGrid& g, int z, int y, int x) { return ((z / g.bz) * g.nby + y / g.by) * g.nbx + x / g.bx; }

// 0 for background and for an id past t_max, the global id otherwise
ST_HD int stitch_gid(const StitchView& v, int b, int l) {
  if (l <= 0 || l > v.nums[b]) return 0;
  const int64_t g = v.offs[b] + l;
  return g <= v.t_max ? (int)g : 0;
}
ST_HD int stitch_gid_at(const StitchView& v, int b, int z, int y, int x) {   // (z, y, x) GLOBAL, inside block b
  const StitchBlock B = v.blocks[b];
  return stitch_gid(v, b, B.labels[((int64_t)(z - B.z0) * B.ey + (y - B.y0)) * B.ex + (x - B.x0)]);
}

// The shell of a block of extents (ez, ey, ex): every voxel with a coordinate at 0 or at the extent - 1, each once.  Both z planes first, then
// for every inner z both y rows, then for every inner z and y both x ends.  A block one voxel thick along an axis is all shell.
ST_HD int64_t stitch_shell_count(int ez, int ey, int ex) {
  const int64_t nzf = ez < 2 ? ez : 2, nyf = ey < 2 ? ey : 2, nxf = ex < 2 ? ex : 2, mz = ez > 2 ? ez - 2 : 0, my = ey > 2 ? ey - 2 : 0;
  return nzf * ey * ex + mz * (nyf * ex + my * nxf);
}
ST_HD void stitch_shell_voxel(int64_t t, int ez, int ey, int ex, int& z, int& y, int& x) {
  const int64_t nzf = ez < 2 ? ez : 2, nyf = ey < 2 ? ey : 2, nxf = ex < 2 ? ex : 2, my = ey > 2 ? ey - 2 : 0, plane = (int64_t)ey * ex;
  if (t < nzf * plane) {
    const int64_t r = t % plane;
    z = t / plane ? ez - 1 : 0; y = (int)(r / ex); x = (int)(r % ex);
    return;
  }
  t -= nzf * plane;
  const int64_t per = nyf * ex + my * nxf;
  int64_t r = t % per;
  z = 1 + (int)(t / per);
  if (r < nyf * ex) { y = r / ex ? ey - 1 : 0; x = (int)(r % ex); return; }
  r -= nyf * ex;
  y = 1 + (int)(r / nxf);
  x = r % nxf ? ex - 1 : 0;
}

// every backward neighbour at connectivity conn (the 3 / 9 / 13 offsets of lbl_for_backward, WITHOUT its "centre alone" shortcut: its chain
// of reliances is not proven across blocks here, and only shell voxels come this way, so every cross-block backward neighbour is taken)
template <class F> ST_HD void stitch_for_backward_all(int conn, F&& f) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int o = 0; o < 13; ++o) {                       // offsets 0..12 of the 27 in (dz, dy, dx) raster order come before the centre (13)
    const int dz = o / 9 - 1, dy = (o / 3) % 3 - 1, dx = o % 3 - 1;
    if ((dz != 0) + (dy != 0) + (dx != 0) <= conn) f(dz, dy, dx);
  }
}

// "touch": the voxel at LOCAL (z, y, x) of block b is united with every labelled backward neighbour that lies inside the volume in ANOTHER block
template <class M> ST_HD void stitch_touch_voxel(const M& m, const StitchGrid& g, const StitchView& v, int conn, int b, int z, int y, int x) {
  const StitchBlock B = v.blocks[b];
  const int ga = stitch_gid(v, b, B.labels[((int64_t)z * B.ey + y) * B.ex + x]);
  if (!ga) return;
  stitch_for_backward_all(conn, [&](int dz, int dy, int dx) {
    const int lz = z + dz, ly = y + dy, lx = x + dx;
    if ((uint32_t)lz < (uint32_t)B.ez && (uint32_t)ly < (uint32_t)B.ey && (uint32_t)lx < (uint32_t)B.ex) return;   // the block's own labelling joined these
    const int gz = B.z0 + lz, gy = B.y0 + ly, gx = B.x0 + lx;
    if ((uint32_t)gz >= (uint32_t)g.Z || (uint32_t)gy >= (uint32_t)g.Y || (uint32_t)gx >= (uint32_t)g.X) return;
    const int gb = stitch_gid_at(v, stitch_block_of(g, gz, gy, gx), gz, gy, gx);
    if (gb) lbl_unite(m, ga, gb);
  });
}

// "contact": the in-plane positions of all pairs of face-adjacent blocks, axis by axis (z, y, x); position t of axis a is one voxel of the low
// block's last plane (za, ya, xa) and its partner in the high block's first plane, one step further along the axis.
ST_HD int64_t stitch_face_count(const StitchGrid& g, int axis) {
  return axis == 0 ? (int64_t)(g.nbz - 1) * g.Y * g.X : axis == 1 ? (int64_t)(g.nby - 1) * g.Z * g.X : (int64_t)(g.nbx - 1) * g.Z * g.Y;
}
struct StitchVoxel { int z, y, x; };
ST_HD StitchVoxel stitch_face_voxel(const StitchGrid& g, int axis, int64_t t) {   // the LOW side's voxel, global
  const int64_t plane = axis == 0 ? (int64_t)g.Y * g.X : axis == 1 ? (int64_t)g.Z * g.X : (int64_t)g.Z * g.Y;
  const int inner = axis == 2 ? g.Y : g.X;                                          // the faster of the two in-plane axes
  const int64_t r = t % plane;
  const int last = (int)((t / plane + 1) * (axis == 0 ? g.bz : axis == 1 ? g.by : g.bx) - 1), u = (int)(r / inner), w = (int)(r % inner);
  return axis == 0 ? StitchVoxel{last, u, w} : axis == 1 ? StitchVoxel{u, last, w} : StitchVoxel{u, w, last};
}
// a and b are united iff c(a, b) q >= p min(s_A(a), s_B(b)): c the positions where both planes hold the pair, s the positions that hold the label
ST_HD bool stitch_contact_joins(int c, int sa, int sb, int p, int q) { return (int64_t)c * q >= (int64_t)p * (sa < sb ? sa : sb); }
// the block that owns global id gid >= 1: the last b with offs[b] < gid
ST_HD int stitch_block_of_id(const int64_t* offs, int nblocks, int gid) {
  int lo = 0, hi = nblocks - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offs[mid] < gid) lo = mid; else hi = mid - 1;
  }
  return lo;
}
ST_HD int stitch_axis_between(const StitchGrid& g, int ba, int bb) {   // the axis along which two face-adjacent blocks differ
  if (ba / (g.nby * g.nbx) != bb / (g.nby * g.nbx)) return 0;
  return (ba / g.nbx) % g.nby != (bb / g.nbx) % g.nby ? 1 : 2;
}
