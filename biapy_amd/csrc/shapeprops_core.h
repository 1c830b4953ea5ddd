// The steps of the per-label shape properties (shapeprops.hip): the closed-form second-order coordinate sums of a run, the bound under which they
// fit 64 bits, the exact covariance numerator and the written-down float sequence that follows it, the face rule, the per-lane counter that sums
// a lane's faces (or perimeter classes) before any atomic, the border and weight-class rules of the 2-D perimeter, and the block's table of three
// counters keyed by label.  Compiles for the device (shapeprops.hip) and for the host (scripts/shapeprops_cpu_check.cpp replays the same code
// sequentially and on std::atomic under std::thread).  The label clamp, the head rule, the coordinate stepping, the carry step and the slot
// search of the block's table are those of regionprops_core.h, which this header includes.
//
// MOMENTS.  The record of a label: 6 x uint64, the sums of zz, yy, xx, zy, zx, yx over its voxels, reached through a policy `M`:
//   void mom(r, int k, uint64_t v)     mom[r][k] += v              (the block's table adds  uint64_t mom_of(s, k)  and the key policy of rp_local_slot)
// COUNTERS (faces per axis z, y, x; perimeter classes 0, 1, 2): 3 integers per label, reached through
//   void cnt(r, int k, uint32_t v)     cnt[r][k] += v              (the block's table adds  uint32_t cnt_of(s, k)  and the key policy)
// A block's share of one counter is at most 2 * 32768 (two faces of each of its voxels): uint32 in LDS, the global rows as wide as the entry says.
// Every field is an integer reached by a commutative add: the result does not depend on the order or on the route a contribution takes.
#pragma once
#include <stdint.h>

#include "regionprops_core.h"

#define SP_HD RP_HD

constexpr int SP_MOMENTS = 6;               // zz, yy, xx, zy, zx, yx
constexpr int SP_COUNTERS = 3;

// ---- the moments bound ---------------------------------------------------------------------------------------------------------------------------
// n (Emax - 1)^2 < 2^63, n the voxel count and Emax the largest extent: a coordinate product is at most (Emax - 1)^2 and a label has at most n
// voxels, so every sum fits int64.  The closed forms stay below 2^64 as well: with L <= Emax <= n the largest intermediate is
// (L - 1) L (2 L - 1) < 2 L^3, and L (L - 1)^2 < 2^63 admits L <= 2^21, where it is (2^21 - 1) 2^21 (2^22 - 1) < 2^64.
// n (Emax - 1)^2 <= 2^63 - 1  <=>  n <= floor((2^63 - 1) / (Emax - 1)^2): no 128-bit product needed.  n < 2^31, Emax < 2^31.
SP_HD bool sp_moments_fit(int64_t n, int64_t emax) {
  const uint64_t sq = (uint64_t)(emax - 1) * (uint64_t)(emax - 1);
  return sq == 0 || (uint64_t)n <= (uint64_t)INT64_MAX / sq;
}

// ---- the closed-form contribution of the run x0 .. x0 + L - 1 of row (z, y) to the moments of record r --------------------------------------------
//   sum x  = L x0 + L (L - 1) / 2                                   sum zz = L z^2, sum yy = L y^2, sum zy = L z y
//   sum xx = L x0^2 + x0 L (L - 1) + (L - 1) L (2 L - 1) / 6        sum zx = z sum x, sum yx = y sum x
// A term that is 0 (z = 0 in every 2-D image) is not sent.
template <class M> SP_HD void sp_apply_moments(const M& m, uint32_t r, int32_t z, int32_t y, int32_t x0, uint32_t L) {
  const uint64_t l = L, a = (uint64_t)x0, zz = (uint64_t)z, yy = (uint64_t)y;
  const uint64_t pairs = l * (l - 1);                                   // even
  const uint64_t sx = l * a + pairs / 2;
  const uint64_t v[SP_MOMENTS] = {l * zz * zz, l * yy * yy, l * a * a + a * pairs + pairs * (2 * l - 1) / 6, l * zz * yy, zz * sx, yy * sx};
#pragma unroll
  for (int k = 0; k < SP_MOMENTS; ++k)                                  // LOOP BOUND: 6
    if (v[k]) m.mom(r, k, v[k]);
}

// one finished run of a label > 0: into the block's table when that takes it, else straight to the global rows
template <class ML, class MG> SP_HD void sp_emit_moments(const ML& local, const MG& global, int32_t label, int32_t z, int32_t y, int32_t x0, uint32_t L) {
  const int s = rp_local_slot(local, label);
  if (s >= 0) sp_apply_moments(local, (uint32_t)s, z, y, x0, L);
  else sp_apply_moments(global, (uint32_t)label, z, y, x0, L);
}
template <class ML, class MG> SP_HD void sp_merge_moments(const ML& local, uint32_t s, const MG& global) {
  const int32_t label = local.kload(s);
  if (label == 0) return;
  for (int k = 0; k < SP_MOMENTS; ++k) {                                // LOOP BOUND: 6
    const uint64_t v = local.mom_of(s, k);
    if (v) global.mom((uint32_t)label, k, v);
  }
}

// ---- the finish pass: covariance from area A, coordinate sums S and moments M --------------------------------------------------------------------
// cov_ab = M_ab / A - (S_a / A) (S_b / A) = (A M_ab - S_a S_b) / A^2.  The numerator is formed exactly: A < 2^31, M_ab < 2^63, S_a < 2^62, so both
// products are below 2^94 and need 128 bits (unsigned __int128: a 64 x 64 -> 128 multiply and a subtraction, no division).  THE FLOAT SEQUENCE,
// repeated by tests/shapeprops_ref.py with Python ints for the numerator:
//   1. N = A M_ab - S_a S_b, sign s and magnitude |N| = hi 2^64 + lo
//   2. d = double(hi) * 2^64 + double(lo)      double(hi) and the product are exact (hi < 2^30); double(lo) rounds to nearest even, the sum rounds
//   3. d = s d;  cov = (d / double(A)) / double(A)                      two roundings; double(A) is exact
// Four roundings at most: |cov - exact| <= ((1 + 2^-53)^4 - 1) |exact|.
struct SpWide { uint64_t hi, lo; bool neg; };
SP_HD SpWide sp_cov_numerator(uint64_t A, uint64_t Mab, uint64_t Sa, uint64_t Sb) {
  const unsigned __int128 p = (unsigned __int128)A * Mab, q = (unsigned __int128)Sa * Sb;
  const bool neg = q > p;
  const unsigned __int128 mag = neg ? q - p : p - q;
  return SpWide{(uint64_t)(mag >> 64), (uint64_t)mag, neg};
}
SP_HD double sp_cov_entry(uint64_t A, uint64_t Mab, uint64_t Sa, uint64_t Sb) {
  const SpWide n = sp_cov_numerator(A, Mab, Sa, Sb);
  double d = (double)n.hi * 18446744073709551616.0 + (double)n.lo;
  if (n.neg) d = -d;
  const double a = (double)A;
  return d / a / a;
}
// which coordinate sums belong to moment k (zz, yy, xx, zy, zx, yx)
SP_HD int sp_axis_a(int k) { return k < 3 ? k : k == 5 ? 1 : 0; }
SP_HD int sp_axis_b(int k) { return k < 3 ? k : k == 3 ? 1 : 2; }
SP_HD void sp_finish_row(const int32_t* area, const int64_t* sums, const int64_t* mom, double* cov) {
  const uint64_t A = (uint64_t)(uint32_t)*area;
  for (int k = 0; k < SP_MOMENTS; ++k)                                  // LOOP BOUND: 6
    cov[k] = A == 0 ? 0.0 : sp_cov_entry(A, (uint64_t)mom[k], (uint64_t)sums[sp_axis_a(k)], (uint64_t)sums[sp_axis_b(k)]);
}

// ---- faces ---------------------------------------------------------------------------------------------------------------------------------------
// The neighbour of a voxel of label l > 0 in one direction is given as its label after rp_label, or SP_OUTSIDE when it lies outside the volume:
// the pair is a face when the two differ.  Where a run was cut (trip, span, lane) plays no part: only labels are compared.
constexpr int32_t SP_OUTSIDE = -1;          // no label equals it (rp_label is never negative)
SP_HD uint32_t sp_face(int32_t label, int32_t neighbour) { return neighbour != label ? 1u : 0u; }

// The counter a lane carries over its consecutive voxels: contributions to one label are summed and go out once, when the label changes and at
// the lane's end (sp_count_flush); background and all-zero counts are dropped.
struct SpCount { int32_t label; uint32_t c[SP_COUNTERS]; };
template <class ML, class MG> SP_HD void sp_count_flush(const ML& local, const MG& global, const SpCount& a) {
  if (a.label <= 0 || (a.c[0] | a.c[1] | a.c[2]) == 0) return;
  const int s = rp_local_slot(local, a.label);
#pragma unroll
  for (int k = 0; k < SP_COUNTERS; ++k) {                               // LOOP BOUND: 3
    if (a.c[k] == 0) continue;
    if (s >= 0) local.cnt((uint32_t)s, k, a.c[k]);
    else global.cnt((uint32_t)a.label, k, a.c[k]);
  }
}
template <class ML, class MG> SP_HD void sp_count_step(const ML& local, const MG& global, SpCount& a, int32_t label, uint32_t c0, uint32_t c1, uint32_t c2) {
  if (label != a.label) {
    sp_count_flush(local, global, a);
    a = SpCount{label, {0, 0, 0}};
  }
  a.c[0] += c0; a.c[1] += c1; a.c[2] += c2;
}
// the faces of a lane's four consecutive voxels (labels `lab`, positions `pos`; a voxel past the end has label 0): `left` / `right` are the
// labels before the first and after the last of them, ym / yp / zm / zp those in the rows and planes beside them or SP_OUTSIDE; the volume's
// ends along x follow from the position
template <class ML, class MG> SP_HD void sp_lane_faces(const ML& local, const MG& global, const int32_t lab[OVL_VPL], const RpPos pos[OVL_VPL], int32_t left,
                                                       int32_t right, const int32_t ym[OVL_VPL], const int32_t yp[OVL_VPL], const int32_t zm[OVL_VPL],
                                                       const int32_t zp[OVL_VPL], int32_t X) {
  SpCount acc{0, {0, 0, 0}};
#pragma unroll
  for (int e = 0; e < OVL_VPL; ++e) {                                   // LOOP BOUND: 4
    const int32_t l = lab[e];
    if (l <= 0) { sp_count_step(local, global, acc, 0, 0, 0, 0); continue; }
    const int32_t xm = pos[e].x == 0 ? SP_OUTSIDE : e ? lab[e - 1] : left;
    const int32_t xp = pos[e].x == X - 1 ? SP_OUTSIDE : e < OVL_VPL - 1 ? lab[e + 1] : right;
    sp_count_step(local, global, acc, l, sp_face(l, zm[e]) + sp_face(l, zp[e]), sp_face(l, ym[e]) + sp_face(l, yp[e]), sp_face(l, xm) + sp_face(l, xp));
  }
  sp_count_flush(local, global, acc);
}

template <class ML, class MG> SP_HD void sp_merge_counts(const ML& local, uint32_t s, const MG& global) {
  const int32_t label = local.kload(s);
  if (label == 0) return;
  for (int k = 0; k < SP_COUNTERS; ++k) {                               // LOOP BOUND: 3
    const uint32_t v = local.cnt_of(s, k);
    if (v) global.cnt((uint32_t)label, k, v);
  }
}

// ---- the 2-D perimeter: scikit-image's perimeter(label == l, neighborhood=4) for every label at once ----------------------------------------------
// A BORDER pixel carries a label > 0 and has a 4-neighbour that differs from it (outside the image counts as background 0, which differs).  For a
// border pixel of label l, k4 / kd count its 4- / diagonal neighbours that are border pixels of l; code = 1 + 2 k4 + 10 kd picks the weight class:
// 0 (weight 1), 1 (sqrt 2), 2 ((1 + sqrt 2) / 2), or none (-1).
SP_HD bool sp_is_border(int32_t l, int32_t up, int32_t down, int32_t left, int32_t right) { return l > 0 && (up != l || down != l || left != l || right != l); }
SP_HD int sp_perimeter_class(int code) {
  switch (code) {
    case 5: case 7: case 15: case 17: case 25: case 27: return 0;
    case 21: case 33: return 1;
    case 13: case 23: return 2;
    default: return -1;
  }
}
// the tile of one block: SP_TY x SP_TX pixels, their labels with a halo of 2 and their border flags with a halo of 1
constexpr int SP_TY = 16, SP_TX = 64;
constexpr int SP_LW = SP_TX + 4, SP_LH = SP_TY + 4;       // the label tile
constexpr int SP_BW = SP_TX + 2, SP_BH = SP_TY + 2;       // the border tile: (r, c) is pixel (r + 1, c + 1) of the label tile
// class of tile pixel (ty, tx) from the two tiles, -1 when it counts nothing; `lab` and `bor` are indexable (LDS on the device, vectors on the host)
template <class LT, class BT> SP_HD int sp_pixel_class(const LT& lab, const BT& bor, int ty, int tx) {
  const int br = ty + 1, bc = tx + 1;
  if (!bor[br * SP_BW + bc]) return -1;
  const int32_t l = lab[(ty + 2) * SP_LW + tx + 2];
  int k4 = 0, kd = 0;
  for (int dy = -1; dy <= 1; ++dy)                                      // LOOP BOUND: 3 x 3
    for (int dx = -1; dx <= 1; ++dx) {
      if (dy == 0 && dx == 0) continue;
      const bool same = bor[(br + dy) * SP_BW + bc + dx] && lab[(ty + 2 + dy) * SP_LW + tx + 2 + dx] == l;
      if (same) { if (dy == 0 || dx == 0) ++k4; else ++kd; }
    }
  return sp_perimeter_class(1 + 2 * k4 + 10 * kd);
}
