// The exact Euclidean distance transform with the nearest source (biapy_amd/prepost.py: distance_transform_edt(return_indices=...),
// expand_labels, voronoi_on_mask).  A voxel is a SOURCE when its value is 0 (with `invert`: when it is nonzero).  index(v) = the linear index
// (int32, C order over (Z,Y,X)) of the source u with the least |u - v|^2, among equally near ones the smallest linear index - the raster-first
// source; a source's index is its own; -1 everywhere where the volume holds no source, beside the distance sentinel of edt.hip (INT32_MAX /
// +inf).  The distances are those of bpx_edt on the same mask, bit for bit.  The rule's separable form and its tie behaviour: edt_core.h.
//
// THREE LAUNCHES as in edt.hip, fixed by the shape and the path alone; no atomics, no data-dependent waiting, every loop bounded by an extent:
//   row pass     one wave per row.  The run start and end of every voxel from the ballots of the key changes; g = min(left, right)^2 and the
//                index of that source, the left one on a tie; a source stores its own index, a row without a source -1.
//   column pass  (Y, then Z) one thread per column, consecutive lanes on consecutive x.  Per run of non-source voxels the lower envelope of the
//                run's parabolas and of the source on each side; every site enters the stack WITH the index the pass before left at its
//                position, and the query writes the winning entry's index beside the value.
// THE INDEX TRAVELS IN THE STACK ENTRY (a fourth field), not through a second index volume.  A column pass cannot gather from the index volume
// it writes - the query walks a run from its end to its start while sites anywhere in the run are still to be read - so the alternative is a
// ping-pong volume of 4 bytes per voxel in the workspace and one per-lane gather per voxel.  Carried in the stack, both values and indices
// are updated in place (a position is loaded before anything at or beyond it is stored) and each column pass adds one coalesced 4-byte read
// and one coalesced 4-byte write per voxel to the traffic of edt.hip.  The price is LDS: the 32 (fp64: 16) entries a thread keeps there are
// 12 (fp64: 20) bytes each, 24 KiB (20 KiB) per wave where edt.hip has 16, so 6 waves fit a CU's 160 KiB where edt.hip runs 8.  The persistent
// grid is sized to that residency: 98304 threads in flight (6 waves x 256 CUs), both paths.  Entries beyond the LDS depth go to the workspace
// slab, entry q of thread t at [q * T + t], as in edt.hip.  Which of the two designs is faster has not been measured against each other; what
// this one costs beside the distance-only call is in profiles/edt_index_timing.json.
// INTEGER PATH (sampling == NULL): int32 values in place in dist_d - or, when dist_d is NULL, in 4 more bytes per voxel of workspace; the Z
// pass overwrites each with its final int32 or float32.  FP64 PATH: fp64 values in the workspace, the Z pass writes float32 to dist_d if given.
// WORKSPACE: E = max(T(Z * X) * Y, T(Y * X) * Z) stack entries with T(columns) = min(98304, a quarter of the columns rounded up to 64):
// 12 * E bytes on the integer path (1.125 GiB at 1024^3), 8 bytes per voxel + 20 * E on the fp64 path.
#include <algorithm>
#include <cmath>

#include "bpx_common.h"
#include "edt_core.h"

namespace {

constexpr int EDTI_MAX_THREADS = 98304;   // threads in flight of a column pass: 6 waves per CU, what 24 KiB of LDS per wave admit

struct Sources {            // the input volume: uint8 or int32; key 0 = a source, 1 = any other voxel
  const void* p;
  int i32, invert;
  __device__ __forceinline__ int at(int64_t i) const {
    const int v = i32 ? reinterpret_cast<const int*>(p)[i] : (int)reinterpret_cast<const uint8_t*>(p)[i];
    return (v != 0) != (invert != 0);
  }
};

// Thread-private stack of (position, first winning position, height, index of the site's source): the Stack of edt.hip with the payload
// edt_column_sites asks for.  First LDS_DEPTH entries in LDS at [q * 64 + lane], deeper ones in the slab at [q * T + tid].
template <class PT, class H, int LDS_DEPTH> struct SiteStack {
  static constexpr int DEPTH = LDS_DEPTH;
  typedef PT pt_t;
  typedef __attribute__((address_space(3))) PT lds_pt_t;     // typed as LDS: through generic pointers the compiler folds the two branches below
  typedef __attribute__((address_space(3))) H lds_h_t;       // into one FLAT access of a selected address, which waits on the memory counter too
  typedef __attribute__((address_space(3))) int32_t lds_ix_t;
  PT* pt;
  H* h;
  int32_t* ix;
  int64_t T, tid;
  lds_pt_t* lpt;            // LDS, already at the lane
  lds_h_t* lh;
  lds_ix_t* lix;
  int cur, top;             // the payload of the next put / of the envelope's top
  static __device__ __forceinline__ PT pack(int pos, int t) { return (PT)(uint32_t)pos | ((PT)(uint32_t)t << (sizeof(PT) * 4)); }   // integer path: both <= 46340
  __device__ __forceinline__ void put(int q, int pos, int t, H hh) {
    const PT w = pack(pos, t);
    top = cur;
    if (q < LDS_DEPTH) { lpt[q * 64] = w; lh[q * 64] = hh; lix[q * 64] = cur; }
    else { const int64_t i = (int64_t)q * T + tid; pt[i] = w; h[i] = hh; ix[i] = cur; }
  }
  __device__ __forceinline__ void get(int q, int& pos, int& t, H& hh) {
    PT w;
    if (q < LDS_DEPTH) { w = lpt[q * 64]; hh = lh[q * 64]; top = lix[q * 64]; }
    else { const int64_t i = (int64_t)q * T + tid; w = pt[i]; hh = h[i]; top = ix[i]; }
    pos = (int)(w & (((PT)1 << (sizeof(PT) * 4)) - 1));
    t = (int)(w >> (sizeof(PT) * 4));
  }
};
typedef SiteStack<uint32_t, int32_t, 32> SiteStackInt;   // 24 KiB of LDS per wave
typedef SiteStack<uint64_t, double, 16> SiteStackF64;    // 20 KiB

// One wave per row (grid-stride over the rows).  val[] takes the steps to the left source first, then g; idx[] the index of the nearer source.
template <class M>
__global__ void __launch_bounds__(256) edt_index_row_kernel(Sources keys, M m, int64_t rows, int X, typename M::val* __restrict__ val, int32_t* __restrict__ idx) {
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
      const int up = __shfl_up(k, 1, 64);                  // every lane takes part: shuffles and ballots stay outside the conditionals
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
        idx[row + x] = k == 0 ? (int32_t)(row + x) : edt_row_site(row + x, dl, dr);
      }
      if (bnd) carry = base + __builtin_ctzll(bnd);
      edge = __shfl(k, 0, 64);
    }
  }
}

// One thread per column, T threads looping over `cols` columns, laid out as in edt.hip's edt_column_kernel.  Values and indices in place.
// FINAL = 1: the last pass, which writes the distances as the caller wants them - the integer path in place (an int32, or the bits of a
// float32), the fp64 path to outf - or not at all (dist == 0: indices only).
template <class M, class S, int FINAL>
__global__ void __launch_bounds__(64) edt_index_column_kernel(Sources keys, M m, S slab, int64_t cols, int len, int64_t inner, int64_t outer, int64_t stride,
                                                              typename M::val* val, int32_t* idx, float* outf, int squared, int dist) {
  typedef typename M::val V;
  constexpr bool FP64 = sizeof(V) == 8;
  __shared__ typename S::pt_t lds_pt[S::DEPTH * 64];
  __shared__ V lds_h[S::DEPTH * 64];
  __shared__ int32_t lds_ix[S::DEPTH * 64];
  const int64_t tid = (int64_t)blockIdx.x * 64 + threadIdx.x;
  S st{slab.pt, slab.h, slab.ix, slab.T, tid, (typename S::lds_pt_t*)lds_pt + threadIdx.x, (typename S::lds_h_t*)lds_h + threadIdx.x,
       (typename S::lds_ix_t*)lds_ix + threadIdx.x, -1, -1};
  for (int64_t c = tid; c < cols; c += st.T) {
    const int64_t base = (c / inner) * outer + c % inner;
    edt_column_sites(
        m, st, len, [&](int i) { return keys.at(base + (int64_t)i * stride); }, [&](int i) { return val[base + (int64_t)i * stride]; },
        [&](int i) { return (int)idx[base + (int64_t)i * stride]; },
        [&](int i, V v, int site) {
          const int64_t o = base + (int64_t)i * stride;
          idx[o] = site;
          if (!FINAL) val[o] = v;
          else if (!dist) return;
          else if (FP64) outf[o] = (float)(squared ? (double)v : sqrt((double)v));
          else if (squared) val[o] = v;
          else val[o] = (V)__float_as_int(v == M::inf() ? INFINITY : (float)sqrt((double)v));
        },
        FINAL && FP64 && dist);
  }
}

int64_t voxels_of(int Z, int Y, int X) { return (Z < 1 || Y < 1 || X < 1) ? 0 : (int64_t)Z * Y * X; }

// threads in flight of a column pass over `cols` columns: a quarter of them, in whole waves, at most EDTI_MAX_THREADS
int64_t edti_threads(int64_t cols) { return std::min<int64_t>(EDTI_MAX_THREADS, cdiv64(cdiv64(cols, 4), 64) * 64); }
// stack entries of the workspace: the larger of the two column passes' (threads x column length)
int64_t edti_entries(int Z, int Y, int X) { return std::max(edti_threads((int64_t)Z * X) * Y, edti_threads((int64_t)Y * X) * Z); }

bool sq_limit_ok(int Z, int Y, int X) { return (int64_t)Z * Z + (int64_t)Y * Y + (int64_t)X * X < EDT_SQ_LIMIT; }

template <class M, class S>
void launch_columns(const Sources& keys, const double* w, S st /* T per pass */, int Z, int Y, int X, typename M::val* val, int32_t* idx, float* outf, int squared,
                    int dist, hipStream_t s) {
  const int64_t plane = (int64_t)Y * X;
  M my, mz;
  if constexpr (sizeof(typename M::val) == 8) { my.w = w[1]; mz.w = w[0]; }
  st.T = edti_threads((int64_t)Z * X);
  edt_index_column_kernel<M, S, 0><<<(unsigned)(st.T / 64), 64, 0, s>>>(keys, my, st, (int64_t)Z * X, Y, (int64_t)X, plane, (int64_t)X, val, idx, outf, squared, dist);
  st.T = edti_threads(plane);
  edt_index_column_kernel<M, S, 1><<<(unsigned)(st.T / 64), 64, 0, s>>>(keys, mz, st, plane, Z, plane, 0, plane, val, idx, outf, squared, dist);
}

}  // namespace

extern "C" int64_t bpx_edt_index_workspace(int Z, int Y, int X, int fp64_path) {
  const int64_t n = voxels_of(Z, Y, X);
  if (n < 1 || n >= ((int64_t)1 << 31)) return -1;
  if (!fp64_path && !sq_limit_ok(Z, Y, X)) return -1;
  const int64_t entries = edti_entries(Z, Y, X);
  return fp64_path ? n * 8 + entries * 20 : entries * 12;
}

extern "C" int bpx_edt_index(const void* key_d, int key_dtype, int invert, int Z, int Y, int X, const double* sampling, int squared, void* dist_d,
                             int32_t* index_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  const char* fn = "bpx_edt_index";
  BPX_CHECK(key_d && index_d && ws_d, "%s: null pointer", fn);
  BPX_CHECK(key_dtype == BPX_U8 || key_dtype == BPX_I32, "%s: keys must be BPX_U8 or BPX_I32 (got dtype %d)", fn, key_dtype);
  BPX_CHECK(Z >= 1 && Y >= 1 && X >= 1, "%s: extents must be at least 1 (got %d x %d x %d)", fn, Z, Y, X);
  const int64_t n = voxels_of(Z, Y, X);
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels: volumes of 2^31 voxels or more are not supported (int32 indices)", fn, (long long)n);
  if (sampling) {
    for (int a = 0; a < 3; ++a)
      BPX_CHECK(std::isfinite(sampling[a]) && sampling[a] > 0.0, "%s: sampling must be positive and finite (got %g, %g, %g)", fn, sampling[0],
                sampling[1], sampling[2]);
  } else {
    BPX_CHECK(sq_limit_ok(Z, Y, X), "%s: %d x %d x %d: Z^2 + Y^2 + X^2 must stay below 2^31 - 1 on the integer path (the squared distance would reach the sentinel)",
              fn, Z, Y, X);
  }
  const int fp64 = sampling ? 1 : 0, dist = dist_d ? 1 : 0;
  const int64_t need = bpx_edt_index_workspace(Z, Y, X, fp64) + ((fp64 || dist) ? 0 : n * 4);
  BPX_CHECK(ws_bytes >= need, "%s: workspace too small (%lld bytes; bpx_edt_index_workspace%s says %lld)", fn, (long long)ws_bytes,
            (fp64 || dist) ? "" : " + 4 bytes per voxel for the values of a call without dist_d", (long long)need);
  BPX_CHECK(((uintptr_t)dist_d & 3) == 0 && ((uintptr_t)index_d & 3) == 0 && ((uintptr_t)ws_d & 7) == 0 && (key_dtype != BPX_I32 || ((uintptr_t)key_d & 3) == 0),
            "%s: dist, index and int32 keys must be 4-byte aligned, the workspace 8-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  const Sources keys{key_d, key_dtype == BPX_I32 ? 1 : 0, invert ? 1 : 0};
  const int64_t rows = (int64_t)Z * Y, entries = edti_entries(Z, Y, X);
  const unsigned row_blocks = (unsigned)std::min<int64_t>(cdiv64(rows, 4), 1 << 16);
  if (fp64) {
    double* val = reinterpret_cast<double*>(ws_d);
    double* h = val + n + entries;
    const SiteStackF64 st{reinterpret_cast<uint64_t*>(val + n), h, reinterpret_cast<int32_t*>(h + entries), 0, 0, nullptr, nullptr, nullptr, -1, -1};
    edt_index_row_kernel<EdtF64><<<row_blocks, 256, 0, s>>>(keys, EdtF64{sampling[2]}, rows, X, val, index_d);
    launch_columns<EdtF64, SiteStackF64>(keys, sampling, st, Z, Y, X, val, index_d, reinterpret_cast<float*>(dist_d), squared, dist, s);
  } else {
    int32_t* w = reinterpret_cast<int32_t*>(ws_d);
    int32_t* val = dist ? reinterpret_cast<int32_t*>(dist_d) : w + 3 * entries;      // the values' home when the caller wants none
    const SiteStackInt st{reinterpret_cast<uint32_t*>(w), w + entries, w + 2 * entries, 0, 0, nullptr, nullptr, nullptr, -1, -1};
    edt_index_row_kernel<EdtInt><<<row_blocks, 256, 0, s>>>(keys, EdtInt{}, rows, X, val, index_d);
    launch_columns<EdtInt, SiteStackInt>(keys, nullptr, st, Z, Y, X, val, index_d, nullptr, squared, dist, s);
  }
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
