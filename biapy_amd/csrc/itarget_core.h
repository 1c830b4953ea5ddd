// The steps of the instance-segmentation training targets (itarget.hip; biapy_amd/targets.py states the semantics): the id a voxel's value
// counts for, the per-instance record and what a run of voxels contributes to it, the finish of a record, and the value of every channel at a
// voxel.  Compiles for the device (itarget.hip) and for the host (scripts/itarget_cpu_check.cpp replays the same code sequentially and on
// std::atomic under std::thread).  Built on regionprops_core.h: the run, the head rule, the block's table and its key policy are that header's.
//
// THE RECORD of an instance (sample b, id l; row b (n_max + 1) + l): regionprops_core.h's record - area (uint32), the coordinate sums
// (3 x uint64: z, y, x), the INCLUSIVE box (6 x int32) - and two maxima kept as the uint32 BITS of a non-negative float32, whose order the bits
// preserve (+inf, 0x7F800000, above every finite value): dmax, the largest distance d of the instance, and rcmax, the largest centroid distance
// rc.  Every field is an integer reached by a commutative atomic (add, min, max): the same bits whatever the order or the route.  The policy `M`
// of regionprops_core.h gains
//   void umax(r, int k, uint32_t bits)      maxima[k][r] = max(maxima[k][r], bits), k = IT_DMAX / IT_RCMAX
// and a table's policy  uint32_t umax_of(s, k).
// THE FINISH turns the three sums of a present instance into its centroid, c_a = double(S_a) / double(A), stored as the double's bits in the
// sum's place: the pack pass and the rcmax pass read centroids, not sums.
#pragma once
#include <math.h>
#include <stdint.h>

#include "regionprops_core.h"

#define IT_HD RP_HD

// ---- channel codes, four bits each in a code word, channel i at bits 4 i .. 4 i + 3 (BPX_ITARGET_* of include/biapy_amd.h) ----------------------
constexpr int IT_F = 1, IT_C = 2, IT_D = 3, IT_DC = 4, IT_H = 5, IT_V = 6, IT_Z = 7;
constexpr int IT_MAX_CHANNELS = 8;
constexpr int32_t IT_ID_LIMIT = 1 << 24;          // n_max < 2^24: a float32 holds every id exactly
constexpr int IT_FLAG_F_EXCLUDES_C = 1, IT_FLAG_D_RAW = 2, IT_FLAG_D_CLIP = 4;      // the pack pass's flags
constexpr int IT_MODE_THICK = 0, IT_MODE_INNER = 1;
constexpr int IT_DMAX = 0, IT_RCMAX = 1;
constexpr uint32_t IT_INF_BITS = 0x7F800000u;

IT_HD int it_code(uint32_t codes, int i) { return (int)((codes >> (4 * i)) & 15u); }
IT_HD bool it_has(uint32_t codes, int channels, int code) {
  for (int i = 0; i < channels && i < IT_MAX_CHANNELS; ++i)       // LOOP BOUND: 8
    if (it_code(codes, i) == code) return true;
  return false;
}
IT_HD uint32_t it_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
IT_HD float it_float(uint32_t u) { return __builtin_bit_cast(float, u); }
IT_HD double it_double(uint64_t u) { return __builtin_bit_cast(double, u); }
IT_HD uint64_t it_bits64(double d) { return __builtin_bit_cast(uint64_t, d); }

// ---- the id a value counts for: itself when it is an integer in 0..n_max, else background 0 and a fault ----------------------------------------
// NaN fails both comparisons, +-inf one of them; -0.0 is the integer 0.  (float)n_max is exact below 2^24.
IT_HD int32_t it_id_f32(float v, int32_t n_max, uint32_t& fault) {
  const bool ok = v >= 0.f && v <= (float)n_max && v == truncf(v);
  fault = ok ? 0u : 1u;
  return ok ? (int32_t)v : 0;
}
IT_HD int32_t it_id_i32(int32_t v, int32_t n_max, uint32_t& fault) {
  const bool ok = v >= 0 && v <= n_max;
  fault = ok ? 0u : 1u;
  return ok ? v : 0;
}

// ---- what the run x0 .. x0 + L - 1 of row (z, y) contributes to record r: regionprops' closed form and the run's largest distance ---------------
// the largest of the L distances from `d` on, as bits.  LOOP BOUND: L, at most a row's X voxels.  KNOWN LIMIT: the loop is serial in the one lane
// that holds the run's head (lane 0 for a run carried across trips) while the wave's other lanes wait.  At training patches a run is at most
// the patch's X (80, 128) voxels and the records are 2 to 6 % of a call (profiles/itarget_timing.json); on a whole volume whose rows lie inside
// one id for thousands of voxels a wave reads up to its span's 8192 distances through one lane.  Not measured at such rows; a per-trip form
// (each lane the maximum of its own 4 voxels, a segmented reduction over the trip's heads) is the follow-up.
IT_HD uint32_t it_run_max(const uint32_t* d, uint32_t L) {
  uint32_t m = 0;
  for (uint32_t i = 0; i < L; ++i) m = d[i] > m ? d[i] : m;
  return m;
}
template <class M> IT_HD void it_apply(const M& m, uint32_t r, int32_t z, int32_t y, int32_t x0, uint32_t L, uint32_t dmax_bits) {
  rp_apply(m, r, z, y, x0, L);
  m.umax(r, IT_DMAX, dmax_bits);
}
// one finished run: into the block's table when that takes the label, to the global row `base + label` otherwise (the overflow route)
template <class ML, class MG>
IT_HD void it_emit(const ML& local, const MG& global, uint32_t base, int32_t label, int32_t z, int32_t y, int32_t x0, uint32_t L, uint32_t dmax_bits) {
  const int s = rp_local_slot(local, label);
  if (s >= 0) it_apply(local, (uint32_t)s, z, y, x0, L, dmax_bits);
  else it_apply(global, base + (uint32_t)label, z, y, x0, L, dmax_bits);
}
// the flush of slot s into the global row of its label
template <class ML, class MG> IT_HD void it_merge(const ML& local, uint32_t s, const MG& global, uint32_t base) {
  const int32_t label = local.kload(s);
  if (label == 0) return;
  const uint32_t r = base + (uint32_t)label;
  global.area(r, local.area_of(s));
  for (int k = 0; k < 3; ++k) {             // LOOP BOUND: 3
    global.sum(r, k, local.sum_of(s, k));
    global.lo(r, k, local.lo_of(s, k));
    global.hi(r, k, local.hi_of(s, k));
  }
  global.umax(r, IT_DMAX, local.umax_of(s, IT_DMAX));
}
// the same two steps of the rcmax pass: only that maximum moves
template <class ML, class MG> IT_HD void it_emit_rc(const ML& local, const MG& global, uint32_t base, int32_t label, uint32_t rc_bits) {
  const int s = rp_local_slot(local, label);
  if (s >= 0) local.umax((uint32_t)s, IT_RCMAX, rc_bits);
  else global.umax(base + (uint32_t)label, IT_RCMAX, rc_bits);
}
template <class ML, class MG> IT_HD void it_merge_rc(const ML& local, uint32_t s, const MG& global, uint32_t base) {
  const int32_t label = local.kload(s);
  if (label != 0) global.umax(base + (uint32_t)label, IT_RCMAX, local.umax_of(s, IT_RCMAX));
}

// ---- the init and finish of a row ------------------------------------------------------------------------------------------------------------
IT_HD void it_init_row(uint32_t* area, uint64_t* sums, int32_t* box, uint32_t* dmax, uint32_t* rcmax) {
  *area = 0; *dmax = 0; *rcmax = 0;
  for (int k = 0; k < 3; ++k) { sums[k] = 0; box[k] = RP_LO_INIT; box[3 + k] = RP_HI_INIT; }      // LOOP BOUND: 3
}
// sums -> centroids (the doubles' bits); a row without voxels becomes zeros with an empty box at 0
IT_HD void it_finish_row(const uint32_t* area, uint64_t* sums, int32_t* box) {
  const uint32_t A = *area;
  for (int k = 0; k < 3; ++k) {             // LOOP BOUND: 3
    if (A == 0) { sums[k] = 0; box[k] = 0; box[3 + k] = 0; }
    else sums[k] = it_bits64((double)sums[k] / (double)A);
  }
}

// ---- the channels ------------------------------------------------------------------------------------------------------------------------------
// rc = float32(sqrt(((dz sz)^2 + (dy sy)^2) + (dx sx)^2)) in fp64, in this order; the translation units are built without contraction (no FMA)
IT_HD float it_rc(const double c[3], int32_t z, int32_t y, int32_t x, const double s[3]) {
  const double dz = ((double)z - c[0]) * s[0], dy = ((double)y - c[1]) * s[1], dx = ((double)x - c[2]) * s[2];
  return (float)sqrt((dz * dz + dy * dy) + dx * dx);
}
// Along a row rc does not decrease with |x - c_x| (every step above is monotone and rounding keeps the order), so a run's largest rc is at one of its ends.
IT_HD uint32_t it_run_rc_max(const double c[3], int32_t z, int32_t y, int32_t x0, uint32_t L, const double s[3]) {
  const uint32_t a = it_bits(it_rc(c, z, y, x0, s)), b = it_bits(it_rc(c, z, y, x0 + (int32_t)L - 1, s));
  return a > b ? a : b;
}
IT_HD float it_dc(float rc, float rcmax) { return rcmax == 0.f ? 1.f : 1.f - rc / rcmax; }
// the offset of coordinate p from the centroid c, scaled by the box's extent on p's side: float32(o / e), 0 when e == 0
IT_HD float it_offset(int32_t p, double c, int32_t lo, int32_t hi) {
  const double o = (double)p - c;
  const double e = o >= 0.0 ? (double)hi - c : c - (double)lo;
  return e == 0.0 ? 0.f : (float)(o / e);
}
// D: d / dmax, 1 at the +inf sentinel (an instance that fills its sample); raw: d, or min(d, clip)
IT_HD float it_d(float d, float dmax, int flags, float clip) {
  if (flags & IT_FLAG_D_RAW) return (flags & IT_FLAG_D_CLIP) ? (d < clip ? d : clip) : d;
  return it_bits(d) == IT_INF_BITS ? 1.f : d / dmax;
}
// does an in-volume neighbour of (z, y, x) within the element generate_binary_structure(ndim, conn) carry another id than l?  ids: one sample's
// (Z, Y, X).  LOOP BOUND: 27
IT_HD bool it_differs(const int32_t* ids, int32_t Z, int32_t Y, int32_t X, int32_t z, int32_t y, int32_t x, int ndim, int conn, int32_t l) {
  bool any = false;
  for (int dz = (ndim == 3 ? -1 : 0); dz <= (ndim == 3 ? 1 : 0); ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int k = (dz != 0) + (dy != 0) + (dx != 0);
        const int32_t zz = z + dz, yy = y + dy, xx = x + dx;
        if (k == 0 || k > conn || zz < 0 || zz >= Z || yy < 0 || yy >= Y || xx < 0 || xx >= X) continue;
        any |= ids[((int64_t)zz * Y + yy) * X + xx] != l;
      }
  return any;
}

// the finished records of a batch as the pack pass reads them: row r = b (n_max + 1) + l
struct ItRecords {
  const uint64_t* cen;      // [rows][3] the centroids' bits
  const int32_t* box;       // [rows][6] inclusive
  const uint32_t* dmax;     // [rows]
  const uint32_t* rcmax;    // [rows]
};
struct ItPack {
  uint32_t codes;
  int32_t channels, ndim, conn, mode, flags;
  float clip;
  double s[3];
};
IT_HD bool it_needs_contour(const ItPack& p) { return it_has(p.codes, p.channels, IT_C) || ((p.flags & IT_FLAG_F_EXCLUDES_C) && it_has(p.codes, p.channels, IT_F)); }

// the value of the channel `code` at voxel (z, y, x) of id l (row r of the records), `edge` = it_differs there, d its distance
IT_HD float it_value(int code, const ItPack& p, const ItRecords& rec, uint32_t r, int32_t l, bool edge, float d, int32_t z, int32_t y, int32_t x) {
  const bool contour = edge && (p.mode == IT_MODE_THICK || l > 0);
  if (code == IT_C) return contour ? 1.f : 0.f;
  if (l <= 0) return 0.f;
  switch (code) {
    case IT_F: return ((p.flags & IT_FLAG_F_EXCLUDES_C) && contour) ? 0.f : 1.f;
    case IT_D: return it_d(d, it_float(rec.dmax[r]), p.flags, p.clip);
    case IT_DC: {
      const double c[3] = {it_double(rec.cen[(int64_t)r * 3]), it_double(rec.cen[(int64_t)r * 3 + 1]), it_double(rec.cen[(int64_t)r * 3 + 2])};
      return it_dc(it_rc(c, z, y, x, p.s), it_float(rec.rcmax[r]));
    }
    case IT_H: return it_offset(x, it_double(rec.cen[(int64_t)r * 3 + 2]), rec.box[(int64_t)r * 6 + 2], rec.box[(int64_t)r * 6 + 5]);
    case IT_V: return it_offset(y, it_double(rec.cen[(int64_t)r * 3 + 1]), rec.box[(int64_t)r * 6 + 1], rec.box[(int64_t)r * 6 + 4]);
    case IT_Z: return it_offset(z, it_double(rec.cen[(int64_t)r * 3]), rec.box[(int64_t)r * 6], rec.box[(int64_t)r * 6 + 3]);
    default: return 0.f;
  }
}
