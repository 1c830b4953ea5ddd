// Stitching of per-block label volumes on the device: what joins the results of several bpx_label_u8 / bpx_watershed calls into the labels of
// the whole volume, so that labelling is no longer bound to one call's 2^31 voxels (biapy_amd/prepost.py: LabelStitcher, label_blocks).
//
// stitch_core.h states the grid, the global ids and the two uniting rules; the union-find is label_uf.h's over the id table parent[0..t_max]
// (integer atomic min only).  The passes, all fixed by the grid:
//   begin     off_b = exclusive prefix sum of max(n_b, 0) (one wave, int64, nothing read back); parent = identity; first = key = ST_NONE; flag = 0.
//   first     per block, at volume rate: first[g] = the smallest GLOBAL linear index (z Y + y) X + x among g's voxels, by a native 64-bit atomic
//             min that only RUN HEADS issue (a row start, or a label that differs from its left neighbour), and only when a relaxed load of the
//             slot still reads a larger index (a stale value is an earlier, larger one: one redundant atomic, never a wrong answer).
//   shell     "touch": one thread per shell voxel of every block unites it with its labelled backward neighbours in other blocks, found by
//             global coordinate through the descriptor table.
//   contact   "contact": the last / first planes of every pair of face-adjacent blocks as two arrays of global ids, their per-label position
//             counts by integer atomic add, the pair counts by bpx_label_overlap, and one thread per pair uniting by the stated ratio.
//   resolve   parent[g] = root(g); key[root] = min of first over the set (64-bit atomic min); flag raised when T > t_max.  Ranking the roots by
//             key is one sort over t_max + 1 entries on the caller's side (prepost.py), as label_overlap does.
//   apply     per block, at volume rate, in place: labels[i] = map[off_b + labels[i]] (0 for background), nothing written when the flag is up.
// No float arithmetic, no float atomics: the same bits every run.  Nothing is read back.  int64 wherever a global index can pass 2^31; a single
// block stays below 2^31 voxels.
#include <algorithm>

#include "bpx_common.h"
#include "stitch_core.h"

static_assert(sizeof(bpx_stitch_block) == 32 && sizeof(StitchBlock) == 32, "the descriptor is 32 bytes on both sides");

namespace {

#define ST_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct IdMem {   // the id table in global memory: relaxed agent-scope loads (never register-cached), the min at the memory side
  int* p;
  __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, ST_RLX_AGENT); }
  __device__ __forceinline__ int amin(int i, int v) const { return __hip_atomic_fetch_min(p + i, v, ST_RLX_AGENT); }
};

// slot = min(slot, v) for int64 slots; the relaxed load in front removes the atomic whenever the slot is already as small
__device__ __forceinline__ void min64(int64_t* slot, int64_t v) {
  if (__hip_atomic_load(slot, ST_RLX_AGENT) > v) __hip_atomic_fetch_min(slot, v, ST_RLX_AGENT);
}

// one wave: offs[b] = sum of max(nums[b'], 0) over b' < b, offs[nblocks] = T
__global__ void __launch_bounds__(64) stitch_offsets_kernel(const int* __restrict__ nums, int nblocks, int64_t* __restrict__ offs, int* __restrict__ flag) {
  const int lane = threadIdx.x;
  int64_t carry = 0;
  for (int base = 0; base < nblocks; base += 64) {
    const int b = base + lane;
    const int64_t v = b < nblocks ? (int64_t)std::max(nums[b], 0) : 0;
    int64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    if (b < nblocks) offs[b] = carry + inc - v;
    carry += __shfl(inc, 63, 64);
  }
  if (lane == 0) { offs[nblocks] = carry; *flag = 0; }
}

__global__ void __launch_bounds__(256) stitch_init_kernel(int t_max, int* __restrict__ parent, int64_t* __restrict__ first, int64_t* __restrict__ key) {
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g <= t_max; g += (int64_t)gridDim.x * 256) {
    parent[g] = (int)g;
    first[g] = ST_NONE;
    key[g] = ST_NONE;
  }
}

struct FirstGeom { int ez, ey, ex, z0, y0, x0, Y, X; int64_t n; };

// four consecutive voxels per thread; VEC: one 16-byte load where all four exist (the block's base is 16-byte aligned then)
template <bool VEC> __global__ void __launch_bounds__(256) stitch_first_kernel(const int* __restrict__ labels, FirstGeom g, const int* __restrict__ num_d,
                                                                             const int64_t* __restrict__ off_d, int t_max, int64_t* first) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= g.n) return;
  const int nb = *num_d;
  const int64_t off = *off_d;
  int v[4];
  if (VEC && i + 3 < g.n) {
    const u32x4_t w = *reinterpret_cast<const u32x4_t*>(labels + i);
    v[0] = (int)w[0]; v[1] = (int)w[1]; v[2] = (int)w[2]; v[3] = (int)w[3];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = i + e < g.n ? labels[i + e] : 0;
  }
  int x = (int)(i % g.ex);
  const int64_t zy = i / g.ex;
  int y = (int)(zy % g.ey), z = (int)(zy / g.ey);
  int prev = x > 0 ? labels[i - 1] : 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int l = v[e];
    if (i + e < g.n && l > 0 && l <= nb && (x == 0 || l != prev) && off + l <= t_max)
      min64(first + (off + l), ((int64_t)(g.z0 + z) * g.Y + (g.y0 + y)) * g.X + (g.x0 + x));
    prev = l;
    if (++x == g.ex) { x = 0; if (++y == g.ey) { y = 0; ++z; } }
  }
}

// "touch": thread t of block b's slice of the grid takes the t-th shell voxel of block b
__global__ void __launch_bounds__(256) stitch_shell_kernel(StitchGrid g, StitchView v, int conn, int per_block, int* parent) {
  const int b = blockIdx.x / per_block;
  const int64_t t = (int64_t)(blockIdx.x % per_block) * 256 + threadIdx.x;
  const StitchBlock B = v.blocks[b];
  if (t >= stitch_shell_count(B.ez, B.ey, B.ex)) return;
  int z, y, x;
  stitch_shell_voxel(t, B.ez, B.ey, B.ex, z, y, x);
  stitch_touch_voxel(IdMem{parent}, g, v, conn, b, z, y, x);
}

struct ContactWs { int* pa; int* pb; int* s; int64_t* keys; int* counts; int* num; void* ows; int64_t ows_bytes; int64_t faces, total; };

__global__ void __launch_bounds__(256) stitch_zero_kernel(int* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0;
}

// "contact", first step: the two sides of every in-plane position as global ids, and s[axis][g] / s[3 + axis][g], the positions of the low
// block's last / the high block's first plane along the axis that hold g
__global__ void __launch_bounds__(256) stitch_faces_kernel(StitchGrid g, StitchView v, int64_t n0, int64_t n1, int64_t n, int* __restrict__ pa,
                                                           int* __restrict__ pb, int* s) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int axis = t < n0 ? 0 : t < n0 + n1 ? 1 : 2;
  const StitchVoxel lo = stitch_face_voxel(g, axis, t - (axis == 0 ? 0 : axis == 1 ? n0 : n0 + n1));
  const int z = lo.z, y = lo.y, x = lo.x;
  const int z2 = z + (axis == 0), y2 = y + (axis == 1), x2 = x + (axis == 2);
  const int a = stitch_gid_at(v, stitch_block_of(g, z, y, x), z, y, x), c = stitch_gid_at(v, stitch_block_of(g, z2, y2, x2), z2, y2, x2);
  pa[t] = a;
  pb[t] = c;
  const int64_t row = (int64_t)v.t_max + 1;
  if (a) __hip_atomic_fetch_add(s + axis * row + a, 1, ST_RLX_AGENT);
  if (c) __hip_atomic_fetch_add(s + (3 + axis) * row + c, 1, ST_RLX_AGENT);
}

// "contact", last step: one thread per distinct pair of the overlap table
__global__ void __launch_bounds__(256) stitch_contact_kernel(StitchGrid g, const int64_t* __restrict__ offs, int nblocks, int t_max, int p, int q,
                                                             const int64_t* __restrict__ keys, const int* __restrict__ counts,
                                                             const int* __restrict__ num, int64_t max_pairs, const int* __restrict__ s, int* parent,
                                                             int* flag) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n = *num;
  if (n < 0) {                                    // more distinct pairs than the table holds: the result would be wrong, so it is refused
    if (k == 0) *flag = 1;
    return;
  }
  if (k >= n || k >= max_pairs) return;
  const int64_t key = keys[k];
  const int a = (int)(key >> 32), b = (int)(key & 0xFFFFFFFF);
  if (a <= 0 || b <= 0 || a > t_max || b > t_max) return;
  const int axis = stitch_axis_between(g, stitch_block_of_id(offs, nblocks, a), stitch_block_of_id(offs, nblocks, b));
  const int64_t row = (int64_t)t_max + 1;
  if (stitch_contact_joins(counts[k], s[axis * row + a], s[(3 + axis) * row + b], p, q)) lbl_unite(IdMem{parent}, a, b);
}

// Entries change under other threads' feet only from an ancestor to the root itself, and roots do not change at all (nothing unites any more),
// so every find ends at the true root.
__global__ void __launch_bounds__(256) stitch_resolve_kernel(int* parent, const int64_t* __restrict__ first, int64_t* key, const int64_t* __restrict__ total,
                                                             int t_max, int* flag) {
  const int64_t T = *total;
  if (blockIdx.x == 0 && threadIdx.x == 0 && T > t_max) *flag = 1;
  const int64_t top = std::min<int64_t>(T, t_max);
  const IdMem m{parent};
  for (int64_t g64 = (int64_t)blockIdx.x * 256 + threadIdx.x + 1; g64 <= top; g64 += (int64_t)gridDim.x * 256) {
    const int g = (int)g64;
    const int r = lbl_find(m, g);
    if (r != g) __hip_atomic_store(parent + g, r, ST_RLX_AGENT);
    const int64_t f = first[g];
    if (f != ST_NONE) min64(key + r, f);
  }
}

template <bool VEC> __global__ void __launch_bounds__(256) stitch_apply_kernel(int* labels, int64_t n, const int* __restrict__ num_d,
                                                                             const int64_t* __restrict__ off_d, int t_max, const int* __restrict__ map,
                                                                             const int* __restrict__ flag) {
  if (*flag) return;
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  const int nb = *num_d;
  const int64_t off = *off_d;
  auto out = [&](int l) { return (l > 0 && l <= nb && off + l <= t_max) ? map[off + l] : 0; };
  if (VEC && i + 3 < n) {
    u32x4_t w = *reinterpret_cast<const u32x4_t*>(labels + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = (uint32_t)out((int)w[e]);
    *reinterpret_cast<u32x4_t*>(labels + i) = w;
  } else {
    for (int e = 0; e < 4 && i + e < n; ++e) labels[i + e] = out(labels[i + e]);
  }
}

int stream_blocks(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>(1, (n + 255) / 256), 8192); }
int64_t up16(int64_t b) { return (b + 15) & ~(int64_t)15; }

// the checks every entry point with a grid shares, in this order; fills g
int check_grid(const char* fn, int Z, int Y, int X, int bz, int by, int bx, StitchGrid& g) {
  BPX_CHECK(Z >= 1 && Y >= 1 && X >= 1, "%s: extents must be at least 1 (got %d x %d x %d)", fn, Z, Y, X);
  BPX_CHECK(bz >= 1 && by >= 1 && bx >= 1, "%s: block extents must be at least 1 (got %d x %d x %d)", fn, bz, by, bx);
  const int64_t bv = (int64_t)std::min(bz, Z) * std::min(by, Y) * std::min(bx, X);
  BPX_CHECK(bv < ((int64_t)1 << 31), "%s: %lld voxels per block: blocks of 2^31 voxels or more are not supported (int32 indices)", fn, (long long)bv);
  g = stitch_grid(Z, Y, X, bz, by, bx);
  BPX_CHECK(stitch_blocks(g) < ((int64_t)1 << 20), "%s: %lld blocks: grids of 2^20 blocks or more are not supported", fn, (long long)stitch_blocks(g));
  return 0;
}

// layout of bpx_stitch_contact's workspace; false when a size is refused
bool contact_layout(const StitchGrid& g, int t_max, int64_t max_pairs, void* ws, ContactWs& w) {
  w.faces = stitch_face_count(g, 0) + stitch_face_count(g, 1) + stitch_face_count(g, 2);
  if (w.faces >= ((int64_t)1 << 31) || t_max < 1 || max_pairs < 1) return false;
  w.ows_bytes = w.faces ? bpx_overlap_workspace(max_pairs) : 0;
  if (w.ows_bytes < 0) return false;
  char* p = reinterpret_cast<char*>(ws);
  int64_t at = 0;
  auto take = [&](int64_t bytes) { char* r = p ? p + at : nullptr; at += up16(bytes); return r; };
  w.pa = reinterpret_cast<int*>(take(w.faces * 4));
  w.pb = reinterpret_cast<int*>(take(w.faces * 4));
  w.s = reinterpret_cast<int*>(take(6 * ((int64_t)t_max + 1) * 4));
  w.keys = reinterpret_cast<int64_t*>(take(max_pairs * 8));
  w.counts = reinterpret_cast<int*>(take(max_pairs * 4));
  w.num = reinterpret_cast<int*>(take(4));
  w.ows = take(w.ows_bytes);
  w.total = at;
  return true;
}

}  // namespace

extern "C" int bpx_stitch_begin(const int32_t* nums_d, int nblocks, int t_max, int64_t* offs_d, int32_t* parent_d, int64_t* first_d, int64_t* key_d,
                                int32_t* flag_d, bpx_stream_t stream) {
  const char* fn = "bpx_stitch_begin";
  BPX_CHECK(nums_d && offs_d && parent_d && first_d && key_d && flag_d, "%s: null pointer", fn);
  BPX_CHECK(nblocks >= 1 && nblocks < (1 << 20), "%s: the number of blocks must be in [1, 2^20) (got %d)", fn, nblocks);
  BPX_CHECK(t_max >= 1 && t_max < INT32_MAX, "%s: t_max must be in [1, 2^31 - 1) (got %d)", fn, t_max);
  BPX_CHECK((((uintptr_t)nums_d | (uintptr_t)parent_d | (uintptr_t)flag_d) & 3) == 0 && (((uintptr_t)offs_d | (uintptr_t)first_d | (uintptr_t)key_d) & 7) == 0,
            "%s: nums, parent and flag must be 4-byte aligned, offs, first and key 8-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  stitch_offsets_kernel<<<1, 64, 0, s>>>(nums_d, nblocks, offs_d, flag_d);
  stitch_init_kernel<<<stream_blocks((int64_t)t_max + 1), 256, 0, s>>>(t_max, parent_d, first_d, key_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_stitch_first(const int32_t* labels_d, int ez, int ey, int ex, int z0, int y0, int x0, int Y, int X, const int32_t* num_d,
                                const int64_t* off_d, int t_max, int64_t* first_d, bpx_stream_t stream) {
  const char* fn = "bpx_stitch_first";
  BPX_CHECK(labels_d && num_d && off_d && first_d, "%s: null pointer", fn);
  BPX_CHECK(ez >= 1 && ey >= 1 && ex >= 1, "%s: block extents must be at least 1 (got %d x %d x %d)", fn, ez, ey, ex);
  const int64_t n = (int64_t)ez * ey * ex;
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels per block: blocks of 2^31 voxels or more are not supported (int32 indices)", fn, (long long)n);
  BPX_CHECK(z0 >= 0 && y0 >= 0 && x0 >= 0, "%s: the block's origin must not be negative (got %d, %d, %d)", fn, z0, y0, x0);
  BPX_CHECK(Y >= 1 && X >= 1 && (int64_t)y0 + ey <= Y && (int64_t)x0 + ex <= X, "%s: the block leaves the volume's %d x %d planes (origin %d, %d, extents %d x %d)", fn,
            Y, X, y0, x0, ey, ex);
  BPX_CHECK(t_max >= 1 && t_max < INT32_MAX, "%s: t_max must be in [1, 2^31 - 1) (got %d)", fn, t_max);
  BPX_CHECK((((uintptr_t)labels_d | (uintptr_t)num_d) & 3) == 0 && (((uintptr_t)off_d | (uintptr_t)first_d) & 7) == 0,
            "%s: labels and num must be 4-byte aligned, off and first 8-byte aligned", fn);
  const FirstGeom g{ez, ey, ex, z0, y0, x0, Y, X, n};
  const unsigned blocks = (unsigned)((n + 1023) / 1024);
  hipStream_t s = (hipStream_t)stream;
  if (((uintptr_t)labels_d & 15) == 0) stitch_first_kernel<true><<<blocks, 256, 0, s>>>(labels_d, g, num_d, off_d, t_max, first_d);
  else stitch_first_kernel<false><<<blocks, 256, 0, s>>>(labels_d, g, num_d, off_d, t_max, first_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_stitch_shell(const bpx_stitch_block* blocks_d, int Z, int Y, int X, int bz, int by, int bx, int connectivity, const int32_t* nums_d,
                                const int64_t* offs_d, int t_max, int32_t* parent_d, bpx_stream_t stream) {
  const char* fn = "bpx_stitch_shell";
  BPX_CHECK(blocks_d && nums_d && offs_d && parent_d, "%s: null pointer", fn);
  StitchGrid g;
  if (check_grid(fn, Z, Y, X, bz, by, bx, g)) return 1;
  BPX_CHECK(connectivity >= 1 && connectivity <= 3, "%s: connectivity must be 1, 2 or 3 (got %d)", fn, connectivity);
  BPX_CHECK(t_max >= 1 && t_max < INT32_MAX, "%s: t_max must be in [1, 2^31 - 1) (got %d)", fn, t_max);
  BPX_CHECK((((uintptr_t)nums_d | (uintptr_t)parent_d) & 3) == 0 && (((uintptr_t)blocks_d | (uintptr_t)offs_d) & 7) == 0,
            "%s: nums and parent must be 4-byte aligned, the descriptors and offs 8-byte aligned", fn);
  const int64_t nblocks = stitch_blocks(g);
  if (nblocks == 1) return 0;                       // nothing crosses a face
  const int64_t shell = stitch_shell_count(std::min(bz, Z), std::min(by, Y), std::min(bx, X));   // the largest block's
  const int64_t per = (shell + 255) / 256;
  BPX_CHECK(per * nblocks < ((int64_t)1 << 31), "%s: %lld shell voxels: more than one launch covers", fn, (long long)(shell * nblocks));
  const StitchView v{reinterpret_cast<const StitchBlock*>(blocks_d), nums_d, offs_d, t_max};
  stitch_shell_kernel<<<(unsigned)(per * nblocks), 256, 0, (hipStream_t)stream>>>(g, v, connectivity, (int)per, parent_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int64_t bpx_stitch_contact_workspace(int Z, int Y, int X, int bz, int by, int bx, int t_max, int64_t max_pairs) {
  if (Z < 1 || Y < 1 || X < 1 || bz < 1 || by < 1 || bx < 1) return -1;
  ContactWs w;
  if (!contact_layout(stitch_grid(Z, Y, X, bz, by, bx), t_max, max_pairs, nullptr, w)) return -1;
  return w.total;
}

extern "C" int bpx_stitch_contact(const bpx_stitch_block* blocks_d, int Z, int Y, int X, int bz, int by, int bx, const int32_t* nums_d,
                                  const int64_t* offs_d, int t_max, int p, int q, int64_t max_pairs, int32_t* parent_d, int32_t* flag_d, void* ws_d,
                                  int64_t ws_bytes, bpx_stream_t stream) {
  const char* fn = "bpx_stitch_contact";
  BPX_CHECK(blocks_d && nums_d && offs_d && parent_d && flag_d && ws_d, "%s: null pointer", fn);
  StitchGrid g;
  if (check_grid(fn, Z, Y, X, bz, by, bx, g)) return 1;
  BPX_CHECK(t_max >= 1 && t_max < INT32_MAX, "%s: t_max must be in [1, 2^31 - 1) (got %d)", fn, t_max);
  BPX_CHECK(p > 0 && p <= q && q <= 32768, "%s: min_contact (p, q) needs 0 < p <= q <= 32768 (got %d, %d)", fn, p, q);
  BPX_CHECK(max_pairs >= 1, "%s: max_pairs must be at least 1 (got %lld)", fn, (long long)max_pairs);
  ContactWs w;
  BPX_CHECK(contact_layout(g, t_max, max_pairs, ws_d, w), "%s: the block faces hold 2^31 positions or more, or max_pairs %lld is refused by bpx_overlap_workspace",
            fn, (long long)max_pairs);
  BPX_CHECK(ws_bytes >= w.total, "%s: workspace too small (%lld bytes, bpx_stitch_contact_workspace says %lld)", fn, (long long)ws_bytes, (long long)w.total);
  BPX_CHECK((((uintptr_t)nums_d | (uintptr_t)parent_d | (uintptr_t)flag_d) & 3) == 0 && (((uintptr_t)blocks_d | (uintptr_t)offs_d) & 7) == 0 &&
                ((uintptr_t)ws_d & 15) == 0,
            "%s: nums, parent and flag must be 4-byte aligned, the descriptors and offs 8-byte aligned, the workspace 16-byte aligned", fn);
  if (w.faces == 0) return 0;                       // one block: no face to look at
  hipStream_t s = (hipStream_t)stream;
  const StitchView v{reinterpret_cast<const StitchBlock*>(blocks_d), nums_d, offs_d, t_max};
  const int64_t rows = 6 * ((int64_t)t_max + 1);
  stitch_zero_kernel<<<stream_blocks(rows), 256, 0, s>>>(w.s, rows);
  stitch_faces_kernel<<<(unsigned)((w.faces + 255) / 256), 256, 0, s>>>(g, v, stitch_face_count(g, 0), stitch_face_count(g, 1), w.faces, w.pa, w.pb, w.s);
  BPX_LAUNCH_CHECK(fn);
  if (bpx_label_overlap(w.pa, w.pb, w.faces, max_pairs, w.keys, w.counts, w.num, w.ows, w.ows_bytes, stream)) return 1;
  stitch_contact_kernel<<<(unsigned)((max_pairs + 255) / 256), 256, 0, s>>>(g, offs_d, (int)stitch_blocks(g), t_max, p, q, w.keys, w.counts, w.num, max_pairs,
                                                                           w.s, parent_d, flag_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_stitch_resolve(int32_t* parent_d, const int64_t* first_d, int64_t* key_d, const int64_t* total_d, int t_max, int32_t* flag_d,
                                  bpx_stream_t stream) {
  const char* fn = "bpx_stitch_resolve";
  BPX_CHECK(parent_d && first_d && key_d && total_d && flag_d, "%s: null pointer", fn);
  BPX_CHECK(t_max >= 1 && t_max < INT32_MAX, "%s: t_max must be in [1, 2^31 - 1) (got %d)", fn, t_max);
  BPX_CHECK((((uintptr_t)parent_d | (uintptr_t)flag_d) & 3) == 0 && (((uintptr_t)first_d | (uintptr_t)key_d | (uintptr_t)total_d) & 7) == 0,
            "%s: parent and flag must be 4-byte aligned, first, key and total 8-byte aligned", fn);
  stitch_resolve_kernel<<<stream_blocks(t_max), 256, 0, (hipStream_t)stream>>>(parent_d, first_d, key_d, total_d, t_max, flag_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_stitch_apply(int32_t* labels_d, int64_t n, const int32_t* num_d, const int64_t* off_d, int t_max, const int32_t* map_d,
                                const int32_t* flag_d, bpx_stream_t stream) {
  const char* fn = "bpx_stitch_apply";
  BPX_CHECK(labels_d && num_d && off_d && map_d && flag_d, "%s: null pointer", fn);
  BPX_CHECK(n >= 1, "%s: extents must be at least 1 (got %lld voxels)", fn, (long long)n);
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels per block: blocks of 2^31 voxels or more are not supported (int32 indices)", fn, (long long)n);
  BPX_CHECK(t_max >= 1 && t_max < INT32_MAX, "%s: t_max must be in [1, 2^31 - 1) (got %d)", fn, t_max);
  BPX_CHECK((((uintptr_t)labels_d | (uintptr_t)num_d | (uintptr_t)map_d | (uintptr_t)flag_d) & 3) == 0 && ((uintptr_t)off_d & 7) == 0,
            "%s: labels, num, map and flag must be 4-byte aligned, off 8-byte aligned", fn);
  const unsigned blocks = (unsigned)((n + 1023) / 1024);
  hipStream_t s = (hipStream_t)stream;
  if (((uintptr_t)labels_d & 15) == 0) stitch_apply_kernel<true><<<blocks, 256, 0, s>>>(labels_d, n, num_d, off_d, t_max, map_d, flag_d);
  else stitch_apply_kernel<false><<<blocks, 256, 0, s>>>(labels_d, n, num_d, off_d, t_max, map_d, flag_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
