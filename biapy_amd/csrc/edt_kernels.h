// The kernels and the launch of the exact Euclidean distance transform, once for both of its forms: distances alone (edt.hip) and distances
// with the nearest source (edt_index.hip), told apart at compile time by INDEX.  Included by those two files and by nothing else; each
// instantiates its own form and keeps its entry points.  The one-dimensional pieces both forms are made of: edt_core.h.
//
// THREE LAUNCHES, fixed by the shape and the path alone; no atomics, no data-dependent waiting, every loop bounded by an extent:
//   row pass     one wave per row, lanes along X (coalesced).  A forward sweep over the row's 64-voxel chunks finds every voxel's run start from
//                a ballot of the key changes (the last start carried across chunks) and stores the steps to the left foreign voxel; a backward
//                sweep finds the run end the same way and stores g = min(left, right)^2 - with INDEX also the index of that source, the left
//                one on a tie; a source stores its own index, a row without a source -1.
//   column pass  (Y, then Z) one thread per column, consecutive lanes on consecutive x, so every load and store of a wave is one contiguous
//                row segment.  Per run of equal nonzero keys: the lower envelope of the run's parabolas and of the foreign voxel on each side
//                (edt_core.h), built on the way up, queried on the way back.  A persistent grid of T threads loops over the columns; a thread's
//                stack keeps its first 32 (fp64: 16) entries in LDS and owns slab entries [q * T + t] of the workspace beyond, q < the column
//                length.  With INDEX every site enters the stack with the index the pass before left at its position, and the query writes
//                the winning entry's index beside the value.
// INTEGER PATH (sampling == NULL): int32 values in place in the caller's output; the Z pass overwrites each int32 with its final int32 or
// float32.  64-bit candidate sums; Z^2 + Y^2 + X^2 < 2^31 - 1 is required so that every finite value is below the sentinel (positions then fit
// 16 bits).  FP64 PATH (sampling given): fp64 values in an 8-byte array in the workspace; the Z pass writes float32(value) or float32(sqrt(value)).
#pragma once
#include <algorithm>
#include <cmath>

#include "bpx_common.h"
#include "edt_core.h"

namespace {

// The input volume: uint8 or int32.  Without INDEX `mode` = binary: every nonzero value is the same key, else the value is the key (labels).
// With INDEX `mode` = invert: key 0 = a source - a zero voxel, inverted a nonzero one -, 1 = any other voxel.
template <bool INDEX> struct EdtKeys {
  const void* p;
  int i32, mode;
  __device__ __forceinline__ int at(int64_t i) const {
    const int v = i32 ? reinterpret_cast<const int*>(p)[i] : (int)reinterpret_cast<const uint8_t*>(p)[i];
    if constexpr (INDEX) return (v != 0) != (mode != 0);
    else return mode ? (v != 0) : v;
  }
};

// What a stack entry carries beside position, first winning position and height: nothing, or the index of the site's source (edt_core.h).
template <bool SITES> struct EdtPayload {};
template <> struct EdtPayload<true> {
  typedef __attribute__((address_space(3))) int32_t lds_ix_t;
  lds_ix_t* lix;
  int cur, top;             // the payload of the next put / of the envelope's top
  int32_t* ix;              // last, next to pt, h and T: what a kernel reads of its stack argument stays one contiguous load
};

// Thread-private stack.  The first LDS_DEPTH entries live in LDS at [q * 64 + lane] (a column pass runs one wave per workgroup), where the
// pushes and pops of nearly every run stay; deeper entries go to the workspace slab, entry q of thread t at [q * T + t] (the lanes of a wave
// at one depth are contiguous).  PT: position and t packed into its two halves; H: the height.
template <class PT, class H, int LDS_DEPTH, bool WITH_SITES> struct EdtStack : EdtPayload<WITH_SITES> {
  static constexpr int DEPTH = LDS_DEPTH;
  static constexpr bool SITES = WITH_SITES;
  static constexpr int ENTRY_BYTES = sizeof(PT) + sizeof(H) + (SITES ? 4 : 0);     // 8 / 12 on the integer path, 16 / 20 on the fp64 path
  typedef PT pt_t;
  typedef __attribute__((address_space(3))) PT lds_pt_t;     // typed as LDS: through generic pointers the compiler folds the two branches below
  typedef __attribute__((address_space(3))) H lds_h_t;       // into one FLAT access of a selected address, which waits on the memory counter too
  PT* pt;
  H* h;
  int64_t T, tid;
  lds_pt_t* lpt;            // LDS, already at the lane
  lds_h_t* lh;
  // the slab of `entries` entries at `base`: the packed positions, the heights, then the payloads
  static EdtStack carve(void* base, int64_t entries) {
    EdtStack st{};
    st.pt = reinterpret_cast<PT*>(base);
    st.h = reinterpret_cast<H*>(st.pt + entries);
    if constexpr (SITES) st.ix = reinterpret_cast<int32_t*>(st.h + entries);
    return st;
  }
  static __device__ __forceinline__ PT pack(int pos, int t) { return (PT)(uint32_t)pos | ((PT)(uint32_t)t << (sizeof(PT) * 4)); }   // integer path: both <= 46340
  __device__ __forceinline__ void put(int q, int pos, int t, H hh) {
    const PT w = pack(pos, t);
    if constexpr (SITES) this->top = this->cur;
    if (q < LDS_DEPTH) {
      lpt[q * 64] = w; lh[q * 64] = hh;
      if constexpr (SITES) this->lix[q * 64] = this->cur;
    } else {
      const int64_t i = (int64_t)q * T + tid;
      pt[i] = w; h[i] = hh;
      if constexpr (SITES) this->ix[i] = this->cur;
    }
  }
  __device__ __forceinline__ void get(int q, int& pos, int& t, H& hh) {
    PT w;
    if (q < LDS_DEPTH) {
      w = lpt[q * 64]; hh = lh[q * 64];
      if constexpr (SITES) this->top = this->lix[q * 64];
    } else {
      const int64_t i = (int64_t)q * T + tid;
      w = pt[i]; hh = h[i];
      if constexpr (SITES) this->top = this->ix[i];
    }
    pos = (int)(w & (((PT)1 << (sizeof(PT) * 4)) - 1));
    t = (int)(w >> (sizeof(PT) * 4));
  }
};
// 16 KiB of LDS per wave without INDEX either way: 8 waves per CU at 131072 threads in flight.  With INDEX 24 KiB (fp64: 20 KiB): 6 waves fit
// a CU's 160 KiB, 98304 threads in flight.
template <bool INDEX> using EdtStackInt = EdtStack<uint32_t, int32_t, 32, INDEX>;
template <bool INDEX> using EdtStackF64 = EdtStack<uint64_t, double, 16, INDEX>;
template <bool INDEX> constexpr int EDT_MAX_THREADS = INDEX ? 98304 : 131072;   // threads in flight of a column pass: 384 / 512 per CU

// One wave per row (grid-stride over the rows).  val[] takes the steps to the left foreign voxel first, then g; with INDEX idx[] takes the index
// of the nearer source.
template <class M, bool INDEX>
__global__ void __launch_bounds__(256) edt_row_kernel(EdtKeys<INDEX> keys, M m, int64_t rows, int X, typename M::val* __restrict__ val, int32_t* __restrict__ idx) {
  typedef typename M::val V;
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * 4;
  const int chunks = (int)(((int64_t)X + 63) / 64);
  for (int64_t r = wave; r < rows; r += waves) {           // wave-uniform
    const int64_t row = r * X;
    int64_t carry = 0;
    int edge = 0;                                          // the key next to the chunk, from the chunk before
    for (int c = 0; c < chunks; ++c) {
      const int64_t base = (int64_t)c * 64, x = base + lane;
      const bool in = x < X;
      const int k = in ? keys.at(row + x) : 0;
      const int up = __shfl_up(k, 1, 64);                  // every lane takes part: a shuffle inside the conditional would read lane 0 while it is masked off
      const int left = lane ? up : edge;
      const unsigned long long bnd = __ballot(in && x > 0 && k != left);
      const int64_t start = edt_run_start(bnd, lane, base, carry);
      if (in) val[row + x] = (V)edt_left_steps(x, start);
      if (bnd) carry = base + 63 - __builtin_clzll(bnd);
      edge = __shfl(k, 63, 64);
    }
    carry = (int64_t)X - 1;
    for (int c = chunks - 1; c >= 0; --c) {
      const int64_t base = (int64_t)c * 64, x = base + lane;
      const bool in = x < X;
      const int k = in ? keys.at(row + x) : 0;
      const int down = __shfl_down(k, 1, 64);
      const int right = lane < 63 ? down : edge;
      const unsigned long long bnd = __ballot(in && x < (int64_t)X - 1 && k != right);
      const int64_t end = edt_run_end(bnd, lane, base, carry);
      if (in) {
        const int64_t dl = (int64_t)val[row + x], dr = edt_right_steps(x, end, X);     // the lane's own store of the forward sweep
        const int64_t d = edt_row_steps(dl, dr);
        val[row + x] = k == 0 ? (V)0 : (d == 0 ? M::inf() : m.steps(d));
        if constexpr (INDEX) idx[row + x] = k == 0 ? (int32_t)(row + x) : edt_row_site(row + x, dl, dr);
      }
      if (bnd) carry = base + __builtin_ctzll(bnd);
      edge = __shfl(k, 0, 64);
    }
  }
}

// One thread per column, T threads looping over `cols` columns.  Column c: `len` positions from (c / inner) * outer + c % inner, `stride` apart
// (Y pass: inner = X, outer = Y * X, stride = X; Z pass: inner = Y * X, outer = 0, stride = Y * X).  Values - and with S::SITES indices - in place.
// FINAL = 0: in place in val.  FINAL = 1: the last pass, which writes the distances as the caller wants them: the integer path in place (an
// int32, or the bits of a float32, over the int32 just read), the fp64 path to outf - or, with S::SITES and dist == 0, not at all (indices
// only).  idx and dist are read with S::SITES only.
template <class M, class S, int FINAL>
__global__ void __launch_bounds__(64) edt_column_kernel(EdtKeys<S::SITES> keys, M m, S slab, int64_t cols, int len, int64_t inner, int64_t outer, int64_t stride,
                                                        typename M::val* val, int32_t* idx, float* outf, int squared, int dist) {
  typedef typename M::val V;
  constexpr bool FP64 = sizeof(V) == 8;
  __shared__ typename S::pt_t lds_pt[S::DEPTH * 64];
  __shared__ V lds_h[S::DEPTH * 64];
  S st = slab;
  st.tid = (int64_t)blockIdx.x * 64 + threadIdx.x;
  st.lpt = (typename S::lds_pt_t*)lds_pt + threadIdx.x;
  st.lh = (typename S::lds_h_t*)lds_h + threadIdx.x;
  bool write_bg = FINAL && FP64;
  if constexpr (S::SITES) {
    __shared__ int32_t lds_ix[S::DEPTH * 64];
    st.lix = (typename S::lds_ix_t*)lds_ix + threadIdx.x;
    st.cur = st.top = -1;
    write_bg = write_bg && dist;
  }
  for (int64_t c = st.tid; c < cols; c += st.T) {
    const int64_t base = (c / inner) * outer + c % inner;
    edt_column(
        m, st, len, [&](int i) { return keys.at(base + (int64_t)i * stride); }, [&](int i) { return val[base + (int64_t)i * stride]; },
        [&](int i, V v, int site) {
          const int64_t o = base + (int64_t)i * stride;
          if constexpr (S::SITES) idx[o] = site;
          if (!FINAL) val[o] = v;
          else if (S::SITES && !dist) return;
          else if (FP64) outf[o] = (float)(squared ? (double)v : sqrt((double)v));
          else if (squared) val[o] = v;
          else val[o] = (V)__float_as_int(v == M::inf() ? INFINITY : (float)sqrt((double)v));
        },
        write_bg, [&](int i) { return (int)idx[base + (int64_t)i * stride]; });
  }
}

// ---- the host side --------------------------------------------------------------------------------------------------------------------
inline int64_t edt_voxels(int Z, int Y, int X) { return (Z < 1 || Y < 1 || X < 1) ? 0 : (int64_t)Z * Y * X; }
inline bool edt_sq_limit_ok(int Z, int Y, int X) { return (int64_t)Z * Z + (int64_t)Y * Y + (int64_t)X * X < EDT_SQ_LIMIT; }

// threads in flight of a column pass over `cols` columns: a quarter of them, in whole waves, at most EDT_MAX_THREADS
template <bool INDEX> int64_t edt_threads(int64_t cols) { return std::min<int64_t>(EDT_MAX_THREADS<INDEX>, cdiv64(cdiv64(cols, 4), 64) * 64); }
// stack entries of the workspace: the larger of the two column passes' (threads x column length)
template <bool INDEX> int64_t edt_entries(int Z, int Y, int X) {
  return std::max(edt_threads<INDEX>((int64_t)Z * X) * Y, edt_threads<INDEX>((int64_t)Y * X) * Z);
}
// bytes of workspace: the stacks, on the fp64 path after 8 bytes per voxel of values; -1 for a shape the call refuses
template <bool INDEX> int64_t edt_workspace(int Z, int Y, int X, int fp64_path) {
  const int64_t n = edt_voxels(Z, Y, X);
  if (n < 1 || n >= ((int64_t)1 << 31)) return -1;
  if (!fp64_path && !edt_sq_limit_ok(Z, Y, X)) return -1;
  const int64_t entries = edt_entries<INDEX>(Z, Y, X);
  return fp64_path ? n * 8 + entries * EdtStackF64<INDEX>::ENTRY_BYTES : entries * EdtStackInt<INDEX>::ENTRY_BYTES;
}

// what both entry points refuse alike, in the name of the one called
inline int edt_check_args(const char* fn, int key_dtype, int Z, int Y, int X, const double* sampling) {
  BPX_CHECK(key_dtype == BPX_U8 || key_dtype == BPX_I32, "%s: keys must be BPX_U8 or BPX_I32 (got dtype %d)", fn, key_dtype);
  BPX_CHECK(Z >= 1 && Y >= 1 && X >= 1, "%s: extents must be at least 1 (got %d x %d x %d)", fn, Z, Y, X);
  const int64_t n = edt_voxels(Z, Y, X);
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels: volumes of 2^31 voxels or more are not supported (int32 indices)", fn, (long long)n);
  if (sampling) {
    for (int a = 0; a < 3; ++a)
      BPX_CHECK(std::isfinite(sampling[a]) && sampling[a] > 0.0, "%s: sampling must be positive and finite (got %g, %g, %g)", fn, sampling[0],
                sampling[1], sampling[2]);
  } else {
    BPX_CHECK(edt_sq_limit_ok(Z, Y, X), "%s: %d x %d x %d: Z^2 + Y^2 + X^2 must stay below 2^31 - 1 on the integer path (the squared distance would reach the sentinel)",
              fn, Z, Y, X);
  }
  return 0;
}

template <class M, class S>
void edt_launch_path(const EdtKeys<S::SITES>& keys, const double* w, int Z, int Y, int X, typename M::val* val, void* stacks, int32_t* idx, float* outf,
                     int squared, int dist, hipStream_t s) {
  constexpr bool INDEX = S::SITES;
  const int64_t rows = (int64_t)Z * Y, plane = (int64_t)Y * X;
  M mx, my, mz;
  if constexpr (sizeof(typename M::val) == 8) { mx.w = w[2]; my.w = w[1]; mz.w = w[0]; }
  edt_row_kernel<M, INDEX><<<(unsigned)std::min<int64_t>(cdiv64(rows, 4), 1 << 16), 256, 0, s>>>(keys, mx, rows, X, val, idx);
  S st = S::carve(stacks, edt_entries<INDEX>(Z, Y, X));
  st.T = edt_threads<INDEX>((int64_t)Z * X);
  edt_column_kernel<M, S, 0><<<(unsigned)(st.T / 64), 64, 0, s>>>(keys, my, st, (int64_t)Z * X, Y, (int64_t)X, plane, (int64_t)X, val, idx, outf, squared, dist);
  st.T = edt_threads<INDEX>(plane);
  edt_column_kernel<M, S, 1><<<(unsigned)(st.T / 64), 64, 0, s>>>(keys, mz, st, plane, Z, plane, 0, plane, val, idx, outf, squared, dist);
}

// The three launches of a checked call.  `val`: the values' home - int32 on the integer path (the Z pass leaves the result there), fp64 with
// `sampling` (the Z pass writes float32 to outf); `stacks`: edt_entries<INDEX> stack entries.  idx, dist: with INDEX only.
template <bool INDEX>
void edt_launch(const EdtKeys<INDEX>& keys, const double* sampling, int Z, int Y, int X, void* val, void* stacks, int32_t* idx, float* outf, int squared,
                int dist, hipStream_t s) {
  if (sampling) edt_launch_path<EdtF64, EdtStackF64<INDEX>>(keys, sampling, Z, Y, X, reinterpret_cast<double*>(val), stacks, idx, outf, squared, dist, s);
  else edt_launch_path<EdtInt, EdtStackInt<INDEX>>(keys, nullptr, Z, Y, X, reinterpret_cast<int32_t*>(val), stacks, idx, nullptr, squared, dist, s);
}

}  // namespace
