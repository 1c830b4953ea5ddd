// The steps of the per-label region properties (regionprops.hip): which voxels of a trip are run heads, the coordinates a lane walks along, the
// step that carries the run left open at the end of a trip into the next one, the closed-form contribution of a run to its label's record, and
// the block's own table keyed by label.  Compiles for the device (regionprops.hip) and for the host (scripts/regionprops_cpu_check.cpp replays the
// same code sequentially and on std::atomic under std::thread).  The span, the trip and the head masks are those of overlap_core.h (OVL_SPAN,
// OVL_TRIP, ovl_first_head / ovl_last_head / ovl_next_head), which this header includes.
//
// THE RECORD of a label: area (uint32), the coordinate sums (3 x uint64: z, y, x) and the box (6 x int32: the minima z y x, then the maxima,
// INCLUSIVE until the finish pass).  Every field is an integer reached by a commutative atomic (add, min, max), so the result does not depend on
// the order or on the route a run takes.  A record is reached through a policy `M`, `r` the row (the label in the global arrays, the slot in a
// block's table):
//   void area(r, uint32_t c)           area[r] += c
//   void sum(r, int k, uint64_t v)     sums[r][k] += v
//   void lo(r, int k, int32_t v)       box[r][k] = min(box[r][k], v)
//   void hi(r, int k, int32_t v)       box[r][3 + k] = max(box[r][3 + k], v)
// A HEAD is a voxel whose label differs from the voxel's before it OR that starts a row (x == 0): every run lies inside one row (z, y) and covers
// x0 .. x0 + L - 1, so its whole contribution is closed form (rp_apply).  A label <= 0 or > n_max is background 0 (rp_label); runs of
// background are dropped where they end and cost nothing.
// THE BLOCK'S OWN TABLE: RP_LOCAL_SLOTS records in LDS with a key (the label, 0 = empty) per slot, claimed by a 32-bit compare-and-swap, linear
// probing from rp_hash(label), at most RP_LOCAL_PROBES probes and RP_LOCAL_LABELS claimed slots; a run that finds no slot goes to the global
// arrays directly, and at the block's end every occupied slot is merged into the global arrays once (rp_merge).  The table's policy adds
//   int32_t kload(s) / int32_t kcas(s, label) (the value BEFORE) / uint32_t nclaimed() / void claim()
//   uint32_t area_of(s) / uint64_t sum_of(s, k) / int32_t lo_of(s, k) / int32_t hi_of(s, k)        plain reads, after the block's barrier
#pragma once
#include <stdint.h>

#include "overlap_core.h"

#define RP_HD OVL_HD

// 256 slots of 56 bytes (key 4, area 4, sums 24, box 24) are 14 KB of LDS: eleven blocks fit a CU's 160 KB, more than the eight that 32 waves
// per CU allow, so the occupancy is left to the registers.  512 slots (28 KB) would hold it to five blocks, five waves per SIMD.  A block's 32768
// contiguous voxels (32 rows at 1024^3) meet a few dozen labels.
constexpr int RP_LOCAL_SLOTS = 256;
constexpr int RP_LOCAL_LABELS = RP_LOCAL_SLOTS / 2;
constexpr int RP_LOCAL_PROBES = 16;
constexpr int32_t RP_NO_LABEL = -1;         // the carried run before the span's first voxel: no label equals it (rp_label is never negative)

// the label a voxel counts for: itself inside 1..n_max, else background 0 (the convention of bpx_label_sizes and bpx_watershed)
RP_HD int32_t rp_label(int32_t v, int32_t n_max) { return v > 0 && v <= n_max ? v : 0; }

// ---- the coordinates a lane walks along -----------------------------------------------------------------------------------------------------
struct RpPos { int32_t z, y, x; };

// How far OVL_TRIP voxels move a position: by (dz, dy, dx) with dx < X and dy < Y, found once on the host.
struct RpStride { int32_t dz, dy, dx; };
RP_HD RpStride rp_stride(int32_t Y, int32_t X) {
  const int32_t rows = OVL_TRIP / X;
  return RpStride{rows / Y, rows % Y, OVL_TRIP % X};
}

// the position of flat index i (two 32-bit divisions: once per lane and span)
RP_HD RpPos rp_pos_of(uint32_t i, int32_t Y, int32_t X) {
  const uint32_t row = i / (uint32_t)X;
  return RpPos{(int32_t)(row / (uint32_t)Y), (int32_t)(row % (uint32_t)Y), (int32_t)(i % (uint32_t)X)};
}
// one voxel on / one trip on, without a division: x < X and y < Y before and after
RP_HD void rp_step(RpPos& p, int32_t Y, int32_t X) {
  if (++p.x == X) { p.x = 0; if (++p.y == Y) { p.y = 0; ++p.z; } }
}
RP_HD void rp_advance(RpPos& p, const RpStride& s, int32_t Y, int32_t X) {
  p.x += s.dx;
  int32_t carry = 0;
  if (p.x >= X) { p.x -= X; carry = 1; }
  p.y += s.dy + carry;                      // at most 2 Y - 1
  carry = 0;
  if (p.y >= Y) { p.y -= Y; carry = 1; }
  p.z += s.dz + carry;
}

// the head rule: a label change or a row start
RP_HD bool rp_is_head(int32_t label, int32_t prev, int32_t x) { return label != prev || x == 0; }

// ---- the closed-form contribution of the run x0 .. x0 + L - 1 of row (z, y) to record r ---------------------------------------------------------
template <class M> RP_HD void rp_apply(const M& m, uint32_t r, int32_t z, int32_t y, int32_t x0, uint32_t L) {
  const uint64_t l = L;
  m.area(r, L);
  m.sum(r, 0, l * (uint64_t)z);
  m.sum(r, 1, l * (uint64_t)y);
  m.sum(r, 2, l * (uint64_t)x0 + l * (l - 1) / 2);
  // The box: six atomics that return nothing.  Reading the box first and issuing only the atomics that would change it was measured and
  // dropped: the wave waits for the reads, and form (b) got slower (balls at 512^3: 0.495 ms against 0.437 ms, at 1024^3: 2.86 against 2.34).
  m.lo(r, 0, z); m.lo(r, 1, y); m.lo(r, 2, x0);
  m.hi(r, 0, z); m.hi(r, 1, y); m.hi(r, 2, x0 + (int32_t)L - 1);
}

// ---- the block's table ------------------------------------------------------------------------------------------------------------------------
// consecutive labels (the numbering of label()) to slots far apart: Fibonacci hashing, the top bits of the product
RP_HD uint32_t rp_hash(int32_t label) { return ((uint32_t)label * 0x9E3779B1u) >> 24 & (uint32_t)(RP_LOCAL_SLOTS - 1); }

// the slot of `label` (> 0) in the block's table, claimed if need be; -1 when the table does not take it.  LOOP BOUND: RP_LOCAL_PROBES probes,
// whatever the other threads do.  The counter may pass RP_LOCAL_LABELS by the threads that claim at the same moment (256 at the most - the table's
// other half), never the slot count: a claim needs an empty slot.
template <class ML> RP_HD int rp_local_slot(const ML& t, int32_t label) {
  uint32_t slot = rp_hash(label);
  for (int probe = 0; probe < RP_LOCAL_PROBES; ++probe) {
    int32_t k = t.kload(slot);
    if (k == 0) {
      if (t.nclaimed() >= (uint32_t)RP_LOCAL_LABELS) return -1;
      k = t.kcas(slot, label);
      if (k == 0) { t.claim(); k = label; }           // ours
    }
    if (k == label) return (int)slot;
    slot = (slot + 1) & (uint32_t)(RP_LOCAL_SLOTS - 1);
  }
  return -1;
}

// one finished run of a label > 0: form (a) straight to the global arrays, form (b) into the block's table when that takes it
template <class MG> RP_HD void rp_emit(const MG& global, int32_t label, int32_t z, int32_t y, int32_t x0, uint32_t L) {
  rp_apply(global, (uint32_t)label, z, y, x0, L);
}
template <class ML, class MG> RP_HD void rp_emit(const ML& local, const MG& global, int32_t label, int32_t z, int32_t y, int32_t x0, uint32_t L) {
  const int s = rp_local_slot(local, label);
  if (s >= 0) rp_apply(local, (uint32_t)s, z, y, x0, L);
  else rp_apply(global, (uint32_t)label, z, y, x0, L);
}

// what a cleared slot holds besides key 0, area 0 and sums 0: a box that any voxel shrinks (also the init pass's value for the global rows)
constexpr int32_t RP_LO_INIT = INT32_MAX;
constexpr int32_t RP_HI_INIT = -1;

// the flush: slot s of the block's table into the global record of its label, once; empty slots are skipped
template <class ML, class MG> RP_HD void rp_merge(const ML& local, uint32_t s, const MG& global) {
  const int32_t label = local.kload(s);
  if (label == 0) return;
  const uint32_t r = (uint32_t)label;
  global.area(r, local.area_of(s));
  for (int k = 0; k < 3; ++k) {             // LOOP BOUND: 3
    global.sum(r, k, local.sum_of(s, k));
    global.lo(r, k, local.lo_of(s, k));
    global.hi(r, k, local.hi_of(s, k));
  }
}

// ---- the run a wave carries in registers from trip to trip ------------------------------------------------------------------------------------
// The label of the last voxel seen, how many voxels the run has covered since its head, and where the head lies.  Starts as {RP_NO_LABEL, 0}:
// the span's first voxel is a head.  A row start is a head, so the run never leaves row (z, y).
struct RpRun { int32_t label; uint32_t count; int32_t z, y, x0; };

// The carry step, after a trip's heads are known.  Without a head the trip's `valid` voxels all continue the carried run.  With one, the carried
// run ends at the first head: `done` receives it, and the run from the LAST head (label last_label, at `last_pos`) to the end of the trip
// becomes the carried one; the heads before the last were complete runs inside the trip and went out from the lanes that hold them.  Returns
// whether `done` is to be sent: it covers voxels (not the span's start) and its label is not background.
RP_HD bool rp_carry_step(RpRun& run, RpRun& done, bool any_head, uint32_t first_head, uint32_t last_head, int32_t last_label, const RpPos& last_pos,
                         uint32_t valid) {
  if (!any_head) { run.count += valid; return false; }
  done = run;
  done.count = run.count + first_head;
  run = RpRun{last_label, valid - last_head, last_pos.z, last_pos.y, last_pos.x};
  return done.count != 0 && done.label > 0;
}

// ---- the init and finish passes, one row ---------------------------------------------------------------------------------------------------------
RP_HD void rp_init_row(int32_t* area, int64_t* sums, int32_t* box) {
  *area = 0;
  for (int k = 0; k < 3; ++k) { sums[k] = 0; box[k] = RP_LO_INIT; box[3 + k] = RP_HI_INIT; }      // LOOP BOUND: 3
}
// maxima made exclusive; the background row and the labels no voxel carries are all zeros
RP_HD void rp_finish_row(int64_t row, const int32_t* area, int64_t* sums, int32_t* box) {
  const bool absent = row == 0 || *area == 0;           // row 0 is never accumulated into: absent either way, stated for the reader
  for (int k = 0; k < 3; ++k) {                         // LOOP BOUND: 3
    if (absent) { sums[k] = 0; box[k] = 0; box[3 + k] = 0; }
    else box[3 + k] += 1;
  }
}
