// The steps of the per-label intensity properties (intensityprops.hip): what one voxel of the image adds to its label's record, how a lane merges
// its voxels before it touches memory, the record's policy, the block's table, and the finish pass - the normalisation of the limbs, the one
// rounding to float64, the non-finite rule and the division.  Everything that decides a result is here and compiles for the device
// (intensityprops.hip) and for the host (bpx_intensity_pieces_host / bpx_intensity_round_host, scripts/intensityprops_cpu_check.cpp).  The order
// preserving uint32 key is peaks_core.h's (peaks_okey / peaks_unokey), the slot search of the block's table regionprops_core.h's (rp_local_slot).
//
// THE EXACT SUM.  A finite float32 is an integer m < 2^24 times 2^(q - 149): with E = (bits >> 23) & 255 and f = bits & 0x7fffff,
// (m, q) = (f, 0) for E == 0 (zero, denormals) and (f | 0x800000, E - 1) otherwise, q in 0..253.  The fixed-point line of 254 + 23 = 277 bits
// above 2^-149 is cut into IP_NL_F32 = 9 windows of 32 bits, one int64 LIMB each: w = m << (q & 31) is below 2^55, its low 32 bits go to limb
// q >> 5 and its high bits (below 2^23) to limb (q >> 5) + 1 <= 8; both are negated for a negative voxel.  A voxel adds at most one piece,
// below 2^32 in magnitude, to any limb, so fewer than 2^31 voxels keep every limb below 2^63: no limb wraps.  Integer adds commute, so the
// limbs are the same bits whatever the order and whatever is summed first in registers or in LDS, and sum_j limb[j] * 2^(32 j - 149) is the
// exact real sum of the label's finite voxels.  uint8 / uint16 images: IP_NL_INT = 1 limb of unit 1, the plain integer sum.
// THE RECORD of a label: count (uint32), the smallest and the largest key (uint32; IP_KMIN_INIT / IP_KMAX_INIT while no voxel that is not NaN
// was seen - no such voxel carries either key), the limbs (NL x int64) and the counts of NaN, +inf and -inf voxels (3 x uint32).  It is reached
// through a policy `M`, `r` the row (the label in the global arrays, the slot in a block's table):
//   void count(r, uint32_t c) / void kmin(r, uint32_t k) / void kmax(r, uint32_t k) / void limb(r, int j, int64_t v) / void nonf(r, int k, uint32_t c)
// the table's policy adds kload / kcas / nclaimed / claim (regionprops_core.h) and the plain reads count_of / kmin_of / kmax_of / limb_of / nonf_of.
#pragma once
#include <stdint.h>

#include "peaks_core.h"
#include "regionprops_core.h"

#define IP_HD OVL_HD

constexpr int IP_NL_F32 = 9;                // limbs of a float32 image, unit 2^-149
constexpr int IP_NL_INT = 1;                // of a uint8 / uint16 image, unit 1
constexpr int IP_UNIT_F32 = -149;
constexpr uint32_t IP_KMIN_INIT = 0xFFFFFFFFu;      // the keys of NaN bit patterns: no voxel that takes part in min / max carries them
constexpr uint32_t IP_KMAX_INIT = 0u;
constexpr int IP_FINITE = 0, IP_NAN = 1, IP_PINF = 2, IP_NINF = 3;      // a voxel's class; class - 1 is its column of `nonfinite`
constexpr uint32_t IP_F32_NAN = 0x7fc00000u;                    // min = max of a label whose voxels are all NaN
constexpr uint64_t IP_F64_NAN = 0x7ff8000000000000ull, IP_F64_INF = 0x7ff0000000000000ull, IP_F64_SIGN = 0x8000000000000000ull;
// 256 slots of 28 + 8 NL bytes (key 4, count 4, keys 8, limbs 8 NL, non-finite 12): 25 600 bytes of LDS for float32 images, six blocks per CU
// by LDS where the 32 waves of a CU allow eight; 9 216 bytes for the integer images.
constexpr int IP_LOCAL_SLOTS = RP_LOCAL_SLOTS;

// ---- one voxel ----------------------------------------------------------------------------------------------------------------------------------
struct IpVoxel {
  uint32_t key;       // order preserving: -0.0 < +0.0
  int32_t cls;        // IP_FINITE ...
  int32_t limb;       // q >> 5 of a finite voxel, -1 otherwise
  int64_t lo, hi;     // the pieces for limb and limb + 1; both 0 for a zero and for a voxel that is not finite
};

IP_HD IpVoxel ip_voxel_f32(uint32_t bits) {
  const uint32_t E = (bits >> 23) & 255u, f = bits & 0x7fffffu;
  const bool neg = (bits >> 31) != 0;
  IpVoxel v{peaks_okey(bits, true), IP_FINITE, -1, 0, 0};
  if (E == 255u) { v.cls = f ? IP_NAN : neg ? IP_NINF : IP_PINF; return v; }
  const uint32_t m = E ? (f | 0x800000u) : f, q = E ? E - 1u : 0u;
  const uint64_t w = (uint64_t)m << (q & 31u);
  const int64_t lo = (int64_t)(w & 0xffffffffull), hi = (int64_t)(w >> 32);
  v.limb = (int32_t)(q >> 5);
  v.lo = neg ? -lo : lo;
  v.hi = neg ? -hi : hi;
  return v;
}
// an integer image's voxel (uint8 / uint16, widened): limb 0 is the plain sum
IP_HD IpVoxel ip_voxel_int(uint32_t value) { return IpVoxel{peaks_okey(value, false), IP_FINITE, 0, (int64_t)value, 0}; }
template <bool F32> IP_HD IpVoxel ip_voxel(uint32_t bits) { return F32 ? ip_voxel_f32(bits) : ip_voxel_int(bits); }

// ---- the lane merge: what voxels of one label add, summed in registers before anything is issued -------------------------------------------------
// `limb` is the limb of lo (hi belongs to limb + 1), -1 while no voxel with a nonzero piece was taken.  A voxel fits when it carries the
// accumulator's label and its pieces, if it has any, belong to the accumulator's limbs; one that does not fit sends the accumulator out first.
struct IpAcc {
  int32_t label;
  uint32_t count, kmin, kmax;
  int32_t limb;
  int64_t lo, hi;
  uint32_t nan, pinf, ninf;
};
IP_HD IpAcc ip_acc(int32_t label) { return IpAcc{label, 0, IP_KMIN_INIT, IP_KMAX_INIT, -1, 0, 0, 0, 0, 0}; }
IP_HD bool ip_has_pieces(const IpVoxel& v) { return (v.lo | v.hi) != 0; }
IP_HD bool ip_fits(const IpAcc& a, int32_t label, const IpVoxel& v) {
  return a.label == label && (!ip_has_pieces(v) || a.limb < 0 || a.limb == v.limb);
}
IP_HD void ip_absorb(IpAcc& a, const IpVoxel& v) {
  a.count += 1;
  if (v.cls != IP_NAN) {
    a.kmin = v.key < a.kmin ? v.key : a.kmin;
    a.kmax = v.key > a.kmax ? v.key : a.kmax;
  }
  if (ip_has_pieces(v)) { a.limb = v.limb; a.lo += v.lo; a.hi += v.hi; }
  a.nan += v.cls == IP_NAN;
  a.pinf += v.cls == IP_PINF;
  a.ninf += v.cls == IP_NINF;
}

// one accumulator into record r: zero limbs, zero counters and untouched keys are skipped.  hi is nonzero only below the last limb.
template <int NL, class M> IP_HD void ip_apply(const M& m, uint32_t r, const IpAcc& a) {
  m.count(r, a.count);
  if (a.kmin != IP_KMIN_INIT) { m.kmin(r, a.kmin); m.kmax(r, a.kmax); }
  if (a.limb >= 0) {
    if (a.lo != 0) m.limb(r, a.limb, a.lo);
    if (a.hi != 0 && a.limb + 1 < NL) m.limb(r, a.limb + 1, a.hi);
  }
  if (a.nan) m.nonf(r, 0, a.nan);
  if (a.pinf) m.nonf(r, 1, a.pinf);
  if (a.ninf) m.nonf(r, 2, a.ninf);
}

// an accumulator of a label > 0 that covers voxels: into the block's table when that takes the label, else to the global arrays
template <int NL, class ML, class MG> IP_HD void ip_emit(const ML& local, const MG& global, const IpAcc& a) {
  if (a.label <= 0 || a.count == 0) return;
  const int s = rp_local_slot(local, a.label);
  if (s >= 0) ip_apply<NL>(local, (uint32_t)s, a);
  else ip_apply<NL>(global, (uint32_t)a.label, a);
}

// the flush: slot s of the block's table into the global record of its label, once; empty slots are skipped.  LOOP BOUND: NL
template <int NL, class ML, class MG> IP_HD void ip_merge(const ML& local, uint32_t s, const MG& global) {
  const int32_t label = local.kload(s);
  if (label == 0) return;
  const uint32_t r = (uint32_t)label;
  global.count(r, local.count_of(s));
  if (local.kmin_of(s) != IP_KMIN_INIT) { global.kmin(r, local.kmin_of(s)); global.kmax(r, local.kmax_of(s)); }
  for (int j = 0; j < NL; ++j) {
    const int64_t v = local.limb_of(s, j);
    if (v != 0) global.limb(r, j, v);
  }
  for (int k = 0; k < 3; ++k) {             // LOOP BOUND: 3
    const uint32_t c = local.nonf_of(s, k);
    if (c) global.nonf(r, k, c);
  }
}

// ---- the finish pass ------------------------------------------------------------------------------------------------------------------------------
// The float64 nearest (ties to even) to sum_j limbs[j] * 2^(32 j + unit), as its bits.  The limbs are first normalised into NL + 1 digits of 32
// bits and a sign: the carry out of a limb is at most 2^31 in magnitude (a limb is below 2^63), so the magnitude is below 2^(32 NL + 32) -
// 2^319 for nine limbs minus the unit.  The digits are then read from the top: the first 54 bits from the leading one are the 53 of the result
// and the guard bit, everything below is sticky.  Every index is a constant after unrolling: registers, no addresses.  An exact zero is +0.0;
// with unit >= -149 and fewer than 2^31 voxels the result is a normal number, neither overflow nor underflow.  LOOP BOUNDS: NL, NL + 1.
template <int NL> IP_HD uint64_t ip_round_bits(const int64_t* limbs, int unit) {
  uint32_t d[NL + 1];
  int64_t carry = 0;
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int64_t t = limbs[j] + carry;
    d[j] = (uint32_t)(uint64_t)t;
    carry = t >> 32;                        // floor: the digits are those of the two's complement
  }
  const bool neg = carry < 0;
  d[NL] = (uint32_t)(uint64_t)carry;
  if (neg) {                                // the magnitude: two's complement negation over the NL + 1 digits
    uint64_t c = 1;
#pragma unroll
    for (int j = 0; j <= NL; ++j) {
      const uint64_t x = (uint64_t)(uint32_t)~d[j] + c;
      d[j] = (uint32_t)x;
      c = x >> 32;
    }
  }
  uint64_t acc = 0;
  int have = 0, top = 0;
  bool sticky = false;
#pragma unroll
  for (int j = NL; j >= 0; --j) {
    const uint32_t x = d[j];
    if (have == 0) {
      if (x) { have = 32 - __builtin_clz(x); acc = x; top = 32 * j + have - 1; }
    } else if (have < 54) {
      const int take = 54 - have < 32 ? 54 - have : 32;         // 1..32
      acc = (acc << take) | (uint64_t)(x >> (32 - take));
      sticky = sticky || (x & ((1u << (32 - take)) - 1u)) != 0;
      have += take;
    } else {
      sticky = sticky || x != 0;
    }
  }
  if (have == 0) return 0;
  uint64_t mant;
  if (have == 54) {
    mant = acc >> 1;
    if ((acc & 1) && (sticky || (mant & 1))) mant += 1;         // to nearest, ties to even; 2^53 carries into the exponent below
  } else {
    mant = acc << (53 - have);                                  // fewer than 54 bits in all: exact
  }
  const uint64_t e = (uint64_t)(top + unit + 1023);             // the biased exponent of 2^top units
  return ((e - 1) << 52) + mant | (neg ? IP_F64_SIGN : 0);
}

// the non-finite rule: a NaN voxel, or infinities of both signs, make the sum NaN; infinities of one sign make it that infinity
IP_HD uint64_t ip_sum_rule(uint64_t rounded, uint32_t nan, uint32_t pinf, uint32_t ninf) {
  if (nan || (pinf && ninf)) return IP_F64_NAN;
  if (pinf) return IP_F64_INF;
  if (ninf) return IP_F64_INF | IP_F64_SIGN;
  return rounded;
}

IP_HD double ip_f64(uint64_t bits) { double v; __builtin_memcpy(&v, &bits, 8); return v; }

// what the init pass writes into a row: the record before any voxel
template <int NL> IP_HD void ip_init_row(uint32_t* area, uint32_t* kmin, uint32_t* kmax, int64_t* limbs, uint32_t* nonf) {
  *area = 0; *kmin = IP_KMIN_INIT; *kmax = IP_KMAX_INIT;
  for (int j = 0; j < NL; ++j) limbs[j] = 0;                    // LOOP BOUND: NL
  for (int k = 0; k < 3; ++k) nonf[k] = 0;                      // LOOP BOUND: 3
}

// one row after the accumulate pass: the keys decoded in place (min / max share their memory with the keys), sum and mean formed; row 0 and a
// label that no voxel carries hold zeros and a NaN mean.  mean = sum / area is a second rounding.
template <int NL, bool F32> IP_HD void ip_finish_row(int64_t row, const uint32_t* area, uint32_t* kmin, uint32_t* kmax, const int64_t* limbs,
                                                    const uint32_t* nonf, double* sum, double* mean) {
  if (row == 0 || *area == 0) {             // row 0 is never accumulated into: absent either way, stated for the reader
    *kmin = 0; *kmax = 0; *sum = 0.0; *mean = ip_f64(IP_F64_NAN);
    return;
  }
  if (*kmin == IP_KMIN_INIT) { *kmin = IP_F32_NAN; *kmax = IP_F32_NAN; }      // every voxel NaN (float32 only)
  else { *kmin = peaks_unokey(*kmin, F32); *kmax = peaks_unokey(*kmax, F32); }
  const uint64_t s = ip_sum_rule(ip_round_bits<NL>(limbs, F32 ? IP_UNIT_F32 : 0), nonf[0], nonf[1], nonf[2]);
  *sum = ip_f64(s);
  *mean = ip_f64(s) / (double)*area;
}
