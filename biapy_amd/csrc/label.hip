// Connected-component labelling of a binary (Z,Y,X) uint8 volume on the device - scipy.ndimage.label(mask, generate_binary_structure(ndim, c))
// bit for bit: int32 labels, background 0, components numbered 1..N in raster order of each component's first voxel.  What follows the
// binarisation of prepost.hip in every segmentation workflow (seed maps, blobs, object counts, small-object removal).
//
// ALGORITHM: union-find over linear voxel indices with labels_out itself as the parent array (label_uf.h: find, unite, the termination
// arguments).  Every union hangs the larger root under the smaller, so a component's root is its raster-first voxel.
//   merge, form 1 (global only)  init: parent[i] = i / LBL_BG; one thread per voxel unites it with the foreground voxels among the backward
//                                half of its neighbourhood (3 / 9 / 13), every union on global memory.
//   merge, form 2 (tiled)        a workgroup resolves an 8 x 8 x 64 tile entirely in LDS (16 KB of int32 parents + 4 KB of mask) and writes
//                                each voxel's tile-local root as a global index; a second kernel unites only the pairs that cross a tile
//                                face, edge or corner.  Same final labels by construction (the components do not depend on the order of
//                                the unions, the numbering only on the components).  bpx_debug_set_label_tiled / BPX_LABEL_TILED choose;
//                                form 1 is the default (the measurement that decided it).
//   flatten + count              every foreground voxel points at its root; roots (parent[i] == i) are counted per chunk of 4096 voxels.
//   scan                         exclusive scan of the chunk counts (one workgroup), the total is N -> *num_d.
//   rank                         root i takes -(its 1-based rank in raster order) IN PLACE.
//   map                          the last pass, one thread per voxel writing its own entry: LBL_BG -> 0; a root -r -> r; a non-root, whose
//                                entry still is its root's index, -> |entry of the root|, which is -r or r depending on whether the root's
//                                thread has flipped it yet - the same value either way.
// ENCODING of labels_out between the kernels: LBL_BG (INT32_MIN) background; >= 0 a parent index (<= the voxel's own); in (LBL_BG, 0) the
// negated final id of a root; after the map pass the final labels.  No second voxel-sized buffer: the workspace is one int32 per chunk.
// The launch sequence (6 launches) depends on (Z, Y, X, connectivity) and the chosen form alone; nothing is read back; integer atomics
// only, so two runs give the same bits; capturable.  Volumes of 2^31 voxels or more are refused (int32 indices).
// Companions: bpx_label_sizes (voxel count per label), bpx_label_filter (small-object removal, optional renumbering).
#include <algorithm>

#include "bpx_common.h"
#include "label_uf.h"

namespace {

#define LBL_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define LBL_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

struct GlobalMem {   // parents in global memory: relaxed agent-scope loads (never register-cached), the min at the memory side
  int* p;
  __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, LBL_RLX_AGENT); }
  __device__ __forceinline__ int amin(int i, int v) const { return __hip_atomic_fetch_min(p + i, v, LBL_RLX_AGENT); }
};
struct LdsMem {      // parents of one tile in LDS
  int* p;
  __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, LBL_RLX_WG); }
  __device__ __forceinline__ int amin(int i, int v) const { return __hip_atomic_fetch_min(p + i, v, LBL_RLX_WG); }
};

struct Geom { int Z, Y, X, conn; int64_t n; };

__global__ void __launch_bounds__(256) label_init_kernel(const uint8_t* __restrict__ mask, int64_t n, int* __restrict__ parent) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) parent[i] = mask[i] ? (int)i : LBL_BG;
}

// one thread per voxel: unite with the backward neighbours.  CROSS = false: all of them (form 1).  CROSS = true: only those in another
// tile (form 2, after label_tile_kernel); a voxel that is not on its tile's surface returns before it reads anything.
template <bool CROSS> __global__ void __launch_bounds__(256) label_merge_kernel(const uint8_t* __restrict__ mask, Geom g, int* parent) {
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i64 >= g.n) return;
  const int i = (int)i64;
  const int x = i % g.X, zy = i / g.X, y = zy % g.Y, z = zy / g.Y;
  const int lz = z % LBL_TZ, ly = y % LBL_TY, lx = x % LBL_TX;
  // backward offsets have dz <= 0 and, at dz = 0, dy <= 0: the tile is left downwards in z, either way in y (dy = +1 comes with dz = -1) and x
  if (CROSS && !(lz == 0 || ly == 0 || ly == LBL_TY - 1 || lx == 0 || lx == LBL_TX - 1)) return;
  if (!mask[i]) return;
  const GlobalMem m{parent};
  auto at = [&](int dz, int dy, int dx) { return ((z + dz) * g.Y + (y + dy)) * g.X + (x + dx); };   // a voxel of the volume where fg says so: < n < 2^31
  lbl_for_backward(
      g.conn,
      [&](int dz, int dy, int dx) {
        const int nz = z + dz, ny = y + dy, nx = x + dx;
        return nz >= 0 && ny >= 0 && ny < g.Y && nx >= 0 && nx < g.X && mask[at(dz, dy, dx)] != 0;
      },
      [&](int dz, int dy, int dx) {
        if (!CROSS || lbl_leaves_tile(lz, ly, lx, dz, dy, dx)) lbl_unite(m, i, at(dz, dy, dx));   // a pair inside one tile is united already
      });
}

// form 2, first kernel: one workgroup per tile; parents are tile-local indices (z, y, x order, the order of the global indices restricted
// to the tile, so the local root is the tile's raster-first voxel of the component); voxels outside the volume are background
__global__ void __launch_bounds__(256) label_tile_kernel(const uint8_t* __restrict__ mask, Geom g, int ntx, int nty, int* __restrict__ parent) {
  __shared__ int P[LBL_TV];
  __shared__ uint8_t M[LBL_TV];
  const int b = blockIdx.x;
  const int x0 = (b % ntx) * LBL_TX, y0 = ((b / ntx) % nty) * LBL_TY, z0 = (b / ntx / nty) * LBL_TZ;
  constexpr int PER = LBL_TV / 256;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int l = k * 256 + threadIdx.x;
    const int lx = l % LBL_TX, ly = (l / LBL_TX) % LBL_TY, lz = l / (LBL_TX * LBL_TY);
    const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
    uint8_t v = 0;
    if (z < g.Z && y < g.Y && x < g.X) v = mask[((int64_t)z * g.Y + y) * g.X + x] ? 1 : 0;
    M[l] = v;
    P[l] = v ? l : LBL_BG;
  }
  __syncthreads();
  const LdsMem m{P};
  for (int k = 0; k < PER; ++k) {
    const int l = k * 256 + threadIdx.x;
    if (!M[l]) continue;
    const int lx = l % LBL_TX, ly = (l / LBL_TX) % LBL_TY, lz = l / (LBL_TX * LBL_TY);
    // a neighbour in another tile counts as absent here: the group's other members are then taken, and the pair that crosses is the next kernel's
    lbl_for_backward(
        g.conn, [&](int dz, int dy, int dx) { return !lbl_leaves_tile(lz, ly, lx, dz, dy, dx) && M[l + (dz * LBL_TY + dy) * LBL_TX + dx] != 0; },
        [&](int dz, int dy, int dx) { lbl_unite(m, l, l + (dz * LBL_TY + dy) * LBL_TX + dx); });
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int l = k * 256 + threadIdx.x;
    const int lx = l % LBL_TX, ly = (l / LBL_TX) % LBL_TY, lz = l / (LBL_TX * LBL_TY);
    const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
    if (z >= g.Z || y >= g.Y || x >= g.X) continue;
    int out = LBL_BG;
    if (M[l]) {
      const int r = lbl_find(m, l);                      // nothing writes P any more
      const int rx = r % LBL_TX, ry = (r / LBL_TX) % LBL_TY, rz = r / (LBL_TX * LBL_TY);
      out = (int)(((int64_t)(z0 + rz) * g.Y + (y0 + ry)) * g.X + (x0 + rx));
    }
    parent[((int64_t)z * g.Y + y) * g.X + x] = out;
  }
}

// one workgroup per chunk: parent[i] = root(i) for the foreground voxels, counts[chunk] = number of roots in the chunk.  Entries change
// under other threads' feet only from an ancestor to the root itself, and roots do not change at all, so every find ends at the true root.
__global__ void __launch_bounds__(256) label_flatten_count_kernel(int* parent, int64_t n, int* __restrict__ counts) {
  __shared__ int wsum[4];
  const GlobalMem m{parent};
  const int64_t base = (int64_t)blockIdx.x * LBL_CHUNK;
  int roots = 0;
  for (int k = 0; k < LBL_CHUNK / 256; ++k) {
    const int64_t i64 = base + k * 256 + threadIdx.x;
    if (i64 >= n) break;
    const int i = (int)i64;
    const int p = m.load(i);
    if (p < 0) continue;
    if (p == i) { ++roots; continue; }
    const int r = lbl_find(m, p);
    if (r != p) __hip_atomic_store(parent + i, r, LBL_RLX_AGENT);
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) roots += __shfl_xor(roots, s, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = roots;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// Single-workgroup exclusive scan in place over data[0 .. n), 4096 elements per round with a running carry; *total = the sum.
//   MODE 0  plain: the chunk counts of the numbering
//   MODE 1  bpx_label_filter, ids kept : data[l] = sizes[l] -> (survives ? l : 0)
//   MODE 2  bpx_label_filter, relabel  : data[l] = sizes[l] -> (survives ? its 1-based rank among the survivors : 0)
// survives: l >= 1 and sizes[l] >= max(min_size, 1) (an id that no voxel carries is no component)
template <int MODE> __global__ void __launch_bounds__(1024) label_scan_kernel(int* data, int64_t n, int min_size, int* total) {
  __shared__ int wtot[16];
  __shared__ int carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t base = 0; base < n; base += 4096) {
    const int64_t i0 = base + (int64_t)threadIdx.x * 4;
    int v[4], s = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int x = (i0 + e < n) ? data[i0 + e] : 0;
      if (MODE != 0) x = (i0 + e >= 1 && i0 + e < n && x >= min_size && x >= 1) ? 1 : 0;
      v[e] = x;
      s += x;
    }
    int inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    int before = carry_s, all = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (q < w) before += wtot[q];
      all += wtot[q];
    }
    int run = before + inc - s;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (i0 + e < n) data[i0 + e] = MODE == 0 ? run : (v[e] ? (MODE == 1 ? (int)(i0 + e) : run + 1) : 0);
      run += v[e];
    }
    __syncthreads();
    if (threadIdx.x == 0) carry_s += all;
    __syncthreads();
  }
  if (threadIdx.x == 0 && total) *total = carry_s;
}

// one workgroup per chunk: the k-th root of the volume in raster order (k from 1) takes -k
__global__ void __launch_bounds__(256) label_rank_kernel(int* parent, int64_t n, const int* __restrict__ offsets) {
  constexpr int PER = LBL_CHUNK / 256;
  __shared__ int cnt[PER * 4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * LBL_CHUNK;
  uint32_t isroot = 0;
  int below[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    const bool r = i < n && parent[i] == (int)i;
    const unsigned long long bal = __ballot(r);
    below[k] = __popcll(bal & ((1ull << lane) - 1ull));
    if (r) isroot |= 1u << k;
    if (lane == 0) cnt[k * 4 + w] = __popcll(bal);
  }
  __syncthreads();
  if (threadIdx.x < 64) {          // exclusive scan of the 64 (round, wave) counts by one wave
    const int c = cnt[threadIdx.x];
    int inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    cnt[threadIdx.x] = inc - c;
  }
  __syncthreads();
  const int off = offsets[blockIdx.x];
#pragma unroll
  for (int k = 0; k < PER; ++k)
    if (isroot & (1u << k)) parent[base + k * 256 + threadIdx.x] = -(off + cnt[k * 4 + w] + below[k] + 1);
}
static_assert(LBL_CHUNK / 256 * 4 == 64, "label_rank_kernel scans its (round, wave) counts with one wave");

// the last pass (see the header): every thread writes its own entry only, and reads its root's through an atomic load
__global__ void __launch_bounds__(256) label_map_kernel(int* labels, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int v = labels[i];
  int out;
  if (v == LBL_BG) out = 0;
  else if (v < 0) out = -v;
  else {
    const int r = __hip_atomic_load(labels + v, LBL_RLX_AGENT);     // v < i is a root: -id, or id once its thread has been here
    out = r < 0 ? -r : r;
  }
  __hip_atomic_store(labels + i, out, LBL_RLX_AGENT);
}

__global__ void __launch_bounds__(256) label_zero_kernel(int* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0;
}

// sizes[l] += number of voxels with label l, 0 <= l <= n_max.  The lanes of a wave that hold the same label add once, together.
__global__ void __launch_bounds__(256) label_sizes_kernel(const int* __restrict__ labels, int64_t n, int n_max, int* sizes) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = ((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63)); base < n; base += (int64_t)gridDim.x * 256) {   // wave-uniform
    const int64_t i = base + lane;
    const int l = i < n ? labels[i] : -1;
    const bool valid = l >= 0 && l <= n_max;
    unsigned long long todo = __ballot(valid);
    while (todo) {                                     // one round per distinct label among the wave's 64: at most 64 rounds
      const int leader = __ffsll((long long)todo) - 1;
      const int ll = __shfl(l, leader, 64);
      const unsigned long long same = __ballot(valid && l == ll);
      if (lane == leader) atomicAdd(&sizes[ll], __popcll(same));
      todo &= ~same;
    }
  }
}

__global__ void __launch_bounds__(256) label_apply_map_kernel(int* labels, int64_t n, int n_max, const int* __restrict__ map) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int l = labels[i];
    if (l == 0) continue;
    const int o = (l > 0 && l <= n_max) ? map[l] : 0;
    if (o != l) labels[i] = o;
  }
}

int g_label_tiled = 0;   // bpx_debug_set_label_tiled / BPX_LABEL_TILED: 0 (default) = global-only merge, 1 = tiled merge; same bits.  The default is the
                         // form that measured faster on the realistic mask at 1024^3 (scripts/label_timing.py, profiles/label_timing.json)

int64_t voxels_of(int Z, int Y, int X) { return (Z < 1 || Y < 1 || X < 1) ? 0 : (int64_t)Z * Y * X; }
int stream_blocks(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>(1, (n + 255) / 256), 8192); }

}  // namespace

extern "C" int bpx_debug_set_label_tiled(int on) { g_label_tiled = on ? 1 : 0; return 0; }

extern "C" int64_t bpx_label_workspace(int Z, int Y, int X) {
  const int64_t n = voxels_of(Z, Y, X);
  if (n < 1 || n >= ((int64_t)1 << 31)) return -1;
  return lbl_chunks(n) * 4;
}

extern "C" int bpx_label_u8(const uint8_t* mask_d, int Z, int Y, int X, int connectivity, int32_t* labels_d, int32_t* num_d, void* ws_d,
                            int64_t ws_bytes, bpx_stream_t stream) {
  const char* fn = "bpx_label_u8";
  BPX_CHECK(mask_d && labels_d && num_d && ws_d, "%s: null pointer", fn);
  BPX_CHECK(Z >= 1 && Y >= 1 && X >= 1, "%s: extents must be at least 1 (got %d x %d x %d)", fn, Z, Y, X);
  BPX_CHECK(connectivity >= 1 && connectivity <= 3, "%s: connectivity must be 1, 2 or 3 (got %d)", fn, connectivity);
  const int64_t n = voxels_of(Z, Y, X);
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels: volumes of 2^31 voxels or more are not supported (int32 indices)", fn, (long long)n);
  BPX_CHECK(ws_bytes >= bpx_label_workspace(Z, Y, X), "%s: workspace too small (%lld bytes, bpx_label_workspace says %lld)", fn,
            (long long)ws_bytes, (long long)bpx_label_workspace(Z, Y, X));
  BPX_CHECK((((uintptr_t)labels_d | (uintptr_t)num_d | (uintptr_t)ws_d) & 3) == 0, "%s: labels, num and the workspace must be 4-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  const Geom g{Z, Y, X, connectivity, n};
  int* counts = reinterpret_cast<int*>(ws_d);
  const unsigned vb = (unsigned)((n + 255) / 256), chunks = (unsigned)lbl_chunks(n);
  if (g_label_tiled) {
    const int ntx = cdiv(X, LBL_TX), nty = cdiv(Y, LBL_TY), ntz = cdiv(Z, LBL_TZ);
    const int64_t tiles = (int64_t)ntx * nty * ntz;       // <= n < 2^31
    label_tile_kernel<<<(unsigned)tiles, 256, 0, s>>>(mask_d, g, ntx, nty, labels_d);
    label_merge_kernel<true><<<vb, 256, 0, s>>>(mask_d, g, labels_d);
  } else {
    label_init_kernel<<<vb, 256, 0, s>>>(mask_d, n, labels_d);
    label_merge_kernel<false><<<vb, 256, 0, s>>>(mask_d, g, labels_d);
  }
  label_flatten_count_kernel<<<chunks, 256, 0, s>>>(labels_d, n, counts);
  label_scan_kernel<0><<<1, 1024, 0, s>>>(counts, (int64_t)chunks, 0, num_d);
  label_rank_kernel<<<chunks, 256, 0, s>>>(labels_d, n, counts);
  label_map_kernel<<<vb, 256, 0, s>>>(labels_d, n);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_label_sizes(const int32_t* labels_d, int64_t n, int n_max, int32_t* sizes_d, bpx_stream_t stream) {
  const char* fn = "bpx_label_sizes";
  BPX_CHECK(labels_d && sizes_d, "%s: null pointer", fn);
  BPX_CHECK(n >= 1, "%s: extents must be at least 1 (got %lld voxels)", fn, (long long)n);
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels: volumes of 2^31 voxels or more are not supported", fn, (long long)n);
  BPX_CHECK(n_max >= 0 && n_max < INT32_MAX, "%s: n_max must be in [0, 2^31 - 1) (got %d)", fn, n_max);
  hipStream_t s = (hipStream_t)stream;
  label_zero_kernel<<<stream_blocks((int64_t)n_max + 1), 256, 0, s>>>(sizes_d, (int64_t)n_max + 1);
  label_sizes_kernel<<<stream_blocks(n), 256, 0, s>>>(labels_d, n, n_max, sizes_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_label_filter(int32_t* labels_d, int64_t n, int n_max, int32_t* sizes_d, int min_size, int relabel, int32_t* num_out_d,
                                bpx_stream_t stream) {
  const char* fn = "bpx_label_filter";
  BPX_CHECK(labels_d && sizes_d, "%s: null pointer", fn);
  BPX_CHECK(n >= 1, "%s: extents must be at least 1 (got %lld voxels)", fn, (long long)n);
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels: volumes of 2^31 voxels or more are not supported", fn, (long long)n);
  BPX_CHECK(n_max >= 0 && n_max < INT32_MAX, "%s: n_max must be in [0, 2^31 - 1) (got %d)", fn, n_max);
  hipStream_t s = (hipStream_t)stream;
  if (relabel) label_scan_kernel<2><<<1, 1024, 0, s>>>(sizes_d, (int64_t)n_max + 1, min_size, num_out_d);
  else label_scan_kernel<1><<<1, 1024, 0, s>>>(sizes_d, (int64_t)n_max + 1, min_size, num_out_d);
  label_apply_map_kernel<<<stream_blocks(n), 256, 0, s>>>(labels_d, n, n_max, sizes_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
