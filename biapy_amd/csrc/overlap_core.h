// The steps of the sparse label-overlap table (overlap.hip): the key of a voxel pair, the hash, the bounded insert into the open-addressing table,
// the positions of the run heads of one trip of a wave, and the step that carries the run left open at the end of a trip into the next one.
// Compiles for the device (overlap.hip) and for the host (scripts/overlap_cpu_check.cpp replays the same code sequentially and on std::atomic
// under std::thread).  The table is reached through a policy `M`:
//   uint64_t kload(uint32_t s)                 relaxed read of the key of slot s
//   uint64_t kcas(uint32_t s, uint64_t key)    atomic "if the slot is OVL_EMPTY, it now holds key"; returns the value BEFORE (64-bit compare-and-swap)
//   void     cadd(uint32_t s, uint32_t c)      atomic count[s] += c (value before not needed)
//   uint32_t nclaimed() / void claim()         relaxed read of / atomic + 1 on the counter of claimed slots
//
// THE TABLE: `slots` = ovl_slots(max_pairs) entries, a power of two >= 2 * max_pairs, linear probing from ovl_hash(key) & (slots - 1).  A key, once in
// a slot, never leaves it or changes, so a reader that sees it may add to the slot's count without any ordering: the count array is zeroed by the
// clear pass, and the compact pass runs after the count pass has ended.  The counter of claimed slots is raised by the one thread whose
// compare-and-swap took the slot, so after the count pass it is exactly the number of occupied slots.
// THE BLOCK'S OWN TABLE: the waves of a block first count into a table of OVL_LOCAL_SLOTS slots in LDS, of the same form and reached through the same
// policy and the same ovl_insert; what it cannot take (more than OVL_LOCAL_PAIRS distinct pairs in the block's voxels) goes straight to the global
// table, and at the block's end every occupied local slot is added to the global table once (ovl_count / the flush in overlap.hip).  A pair's
// voxels may so be split between the two routes; the global count is their sum either way.
// OVERFLOW: more than max_pairs distinct pairs.  A thread that is about to claim a slot while the counter already exceeds max_pairs gives up, and so
// does one that has probed 64 slots in a row; the counter then stays above max_pairs and the compact pass reports -1.  While the counter is at most
// max_pairs the table is at most half full and every insert ends at its key or at an empty slot.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OVL_HD __host__ __device__ __forceinline__
#else
#define OVL_HD inline
#endif

#define OVL_EMPTY ((uint64_t)INT64_MAX)     // no key: above every key (a key is at most 0x7fffffff7fffffff); also the filler of keys_d past K

constexpr int OVL_LANES = 64;               // a wave
constexpr int OVL_VPL = 4;                  // voxels per lane and trip: one 16-byte load per input
constexpr int OVL_TRIP = OVL_LANES * OVL_VPL;
// Voxels per wave.  One table update per uniform span: at 1024^3 an all-background pair sends 2^30 / 8192 = 131072 adds to one address where one
// per voxel would send 2^30, and 32 trips amortise the flush at the span's end.  Not longer: a 256^3 volume (2^24 voxels) then still gives 2048
// waves, eight per CU, which a memory-bound pass needs to keep enough loads in flight.  A power of two above 4, so that a span starts 16-byte
// aligned whenever the volume does.
constexpr int OVL_SPAN = 8192;
constexpr int OVL_WAVES = 4;                // waves (spans) per block: one local table per 32768 voxels
// The local table: a block's 32768 contiguous voxels (half a plane at 256^3) meet a few dozen pairs in instance volumes; 512 slots of 12 bytes are
// 6 KB of LDS, which leaves the occupancy to the registers.
constexpr int OVL_LOCAL_SLOTS = 512;
constexpr int OVL_LOCAL_PAIRS = OVL_LOCAL_SLOTS / 2;

// a label <= 0 is background 0 (as the markers of the watershed); key = a << 32 | b, below 2^63
OVL_HD uint64_t ovl_key(int32_t a, int32_t b) { return ((uint64_t)(uint32_t)(a > 0 ? a : 0) << 32) | (uint32_t)(b > 0 ? b : 0); }

// slot count for max_pairs: the power of two >= 2 * max_pairs; 0 when max_pairs < 1 or the count would pass 2^31.  LOOP BOUND: 31 steps.
OVL_HD int64_t ovl_slots(int64_t max_pairs) {
  if (max_pairs < 1 || max_pairs > ((int64_t)1 << 30)) return 0;
  int64_t s = 2;
  while (s < 2 * max_pairs) s <<= 1;
  return s;
}

// the finaliser of MurmurHash3 (a bijection of 64 bits: keys that differ in one label spread over the whole table), folded to 32 bits
OVL_HD uint32_t ovl_hash(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (uint32_t)(k ^ (k >> 32));
}

// count[key] += count; false when the key is not in the table and was not put there (overflow).  LOOP BOUND: `mask + 1` probes, the slot count,
// whatever the other threads do; every 64th probe looks at the overflow counter, so once overflow is decided no insert costs more than 64 probes (a
// full table of a small max_pairs otherwise costs every voxel a walk over all of it).
template <class M> OVL_HD bool ovl_insert(const M& m, uint64_t key, uint32_t count, uint32_t mask, uint32_t max_pairs) {
  uint32_t slot = ovl_hash(key) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    uint64_t k = m.kload(slot);
    if (k == OVL_EMPTY) {
      if (m.nclaimed() > max_pairs) return false;     // overflow is decided: the table's contents no longer matter
      k = m.kcas(slot, key);
      if (k == OVL_EMPTY) { m.claim(); k = key; }     // ours
    }
    if (k == key) { m.cadd(slot, count); return true; }
    if ((probe & 63u) == 63u && m.nclaimed() > max_pairs) return false;
    slot = (slot + 1) & mask;
  }
  return false;                                       // every slot holds another key: claimed = slots > max_pairs
}

// one run of a wave: into the block's table, into the global one when that takes no more.  The local counter may pass OVL_LOCAL_PAIRS by the
// threads that claim at the same moment (256 at the most, which the spare half of the slots takes); a local table that is full to the last slot
// still answers within 64 probes.
template <class ML, class MG> OVL_HD void ovl_count(const ML& local, const MG& global, uint64_t key, uint32_t count, uint32_t mask, uint32_t max_pairs) {
  if (!ovl_insert(local, key, count, (uint32_t)(OVL_LOCAL_SLOTS - 1), (uint32_t)OVL_LOCAL_PAIRS)) ovl_insert(global, key, count, mask, max_pairs);
}

// ---- one trip of a wave: OVL_TRIP consecutive voxels, lane l holds the voxels 4 l .. 4 l + 3, of which the first `valid` exist -------------------
// A voxel is a HEAD when its key differs from the voxel's before it (for voxel 0: from the key of the run carried into the trip).  H[e] has bit l
// set when voxel 4 l + e is a head; heads lie below `valid`.  A run reaches from its head to the next head, or to `valid`.

// position of the first head after voxel 4 * lane + e, `valid` when there is none
OVL_HD uint32_t ovl_next_head(const uint64_t H[OVL_VPL], int lane, int e, uint32_t valid) {
  for (int f = e + 1; f < OVL_VPL; ++f)
    if ((H[f] >> lane) & 1) return (uint32_t)(OVL_VPL * lane + f);
  const uint64_t any = H[0] | H[1] | H[2] | H[3];
  const uint64_t later = lane >= OVL_LANES - 1 ? 0 : any >> (lane + 1);
  if (!later) return valid;
  const int l2 = lane + 1 + __builtin_ctzll(later);
  for (int f = 0; f < OVL_VPL - 1; ++f)
    if ((H[f] >> l2) & 1) return (uint32_t)(OVL_VPL * l2 + f);
  return (uint32_t)(OVL_VPL * l2 + OVL_VPL - 1);
}

// position of the first / last head of the trip; only when there is one (H[0] | H[1] | H[2] | H[3] != 0)
OVL_HD uint32_t ovl_first_head(const uint64_t H[OVL_VPL]) {
  const int l = __builtin_ctzll(H[0] | H[1] | H[2] | H[3]);
  for (int f = 0; f < OVL_VPL - 1; ++f)
    if ((H[f] >> l) & 1) return (uint32_t)(OVL_VPL * l + f);
  return (uint32_t)(OVL_VPL * l + OVL_VPL - 1);
}
OVL_HD uint32_t ovl_last_head(const uint64_t H[OVL_VPL]) {
  const int l = 63 - __builtin_clzll(H[0] | H[1] | H[2] | H[3]);
  for (int f = OVL_VPL - 1; f > 0; --f)
    if ((H[f] >> l) & 1) return (uint32_t)(OVL_VPL * l + f);
  return (uint32_t)(OVL_VPL * l);
}

// The run a wave carries in registers from trip to trip: the key of the last voxel seen and how many voxels it has covered since its head.
// Starts as {OVL_EMPTY, 0}: no key equals OVL_EMPTY, so the span's first voxel is a head.
struct OvlRun { uint64_t key; uint32_t count; };

// The carry step, after a trip's heads are known.  Without a head the trip's `valid` voxels all continue the carried run.  With one, the carried
// run ends at the first head: `done` receives it (the caller sends it to the table unless its count is 0 - the span's start) and the run from
// the LAST head, of key last_key, to the end of the trip becomes the carried one; the heads before the last were complete runs inside the trip and
// went to the table from the lanes that hold them.  Returns whether `done` was filled.
OVL_HD bool ovl_carry_step(OvlRun& run, OvlRun& done, bool any_head, uint32_t first_head, uint32_t last_head, uint64_t last_key, uint32_t valid) {
  if (!any_head) { run.count += valid; return false; }
  done.key = run.key;
  done.count = run.count + first_head;
  run.key = last_key;
  run.count = valid - last_head;
  return done.count != 0;
}
