// Seeded (marker-controlled) watershed of a (Z,Y,X) float32 / int32 image on the device - what label() and the distance transform exist for in
// the instance workflow (skimage.segmentation.watershed(image, markers, mask=foreground) on the host there).  Product-defined semantics, checked
// against a host twin (tests/watershed_ref.py), because scikit-image breaks ties by the age of a heap entry, a property of a sequential program:
//
//   nodes        the voxels with mask != 0 (all voxels without a mask)
//   edges        two nodes that are neighbours at `connectivity` (1 / 2 / 3 as bpx_label_u8; 2-D is Z = 1)
//   edge weight  max(k(u), k(v)), k the order-preserving uint32 image of the value (int32: v + 2^31; float32: the sign-flip map, -0.0 < +0.0; NaN
//                unspecified)
//   edge order   strict and total: (weight, linear index of the edge's raster-first endpoint u, rank of the offset among u's forward offsets in
//                (dz, dy, dx) lexicographic order)
//   seeds        a voxel with markers > 0 inside the mask carries that label; markers <= 0 and markers outside the mask are ignored
//   result       the unique minimum spanning forest in which every tree holds at most one seeded group: the minimum spanning tree of the graph
//                with all seeded voxels tied to one virtual root by edges below every other, minus the root (unique because the order is strict)
//   output       int32: every masked voxel takes the label of its tree, 0 if the tree holds no seed; 0 outside the mask
// So every voxel goes to a seed that reaches it over the lowest pass height (the flooding watershed, the "watershed cut"); seeds with the same
// label need not touch; TIES OF THE IMAGE GO TO THE RASTER-FIRST EDGE, so a flat plateau between two seeds is not split in the middle (the recipe
// for saturated maps: an int32 image (q << 15) | min(d, 32767), d a distance to the nearest marker - prepost.watershed's docstring).
//
// ALGORITHM: Boruvka rounds on the union-find of label_uf.h; the steps, the state and the argument for the round bound R = ceil(log2(max(n, 2))) + 1
// are in watershed_core.h, which the host check program compiles too.  Launches: zero the round flags, init, R x (pick, resolve, unite, flatten),
// last - 4 R + 3, fixed by (Z, Y, X, connectivity) whatever the data.  A round after the last one that picked anything returns at its first
// instruction (the flag of the round before is 0), and every kernel walks the volume with a bounded grid, so such a launch costs its dispatch
// alone.  Nothing is read back; integer atomics only, so two runs give the same bits; capturable; no grid barrier, no cooperative launch, no loop
// whose trip count another thread decides (the grid-stride loops run ceil(n / threads) times; find and unite as label_uf.h bounds them).
// Workspace: best (8 bytes per voxel), P (4 bytes per voxel), R + 1 flags.  Volumes of 2^31 voxels or more are refused (int32 indices, 31-bit u).
#include <algorithm>

#include "bpx_common.h"
#include "watershed_core.h"

namespace {

#define WS_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct WsDev {     // relaxed agent-scope accesses (never register-cached), the mins at the memory side
  int* P;
  unsigned long long* best;
  int* out;
  int* act;
  __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(P + i, WS_RLX_AGENT); }
  __device__ __forceinline__ int amin(int i, int v) const { return __hip_atomic_fetch_min(P + i, v, WS_RLX_AGENT); }
  __device__ __forceinline__ void pstore(int i, int v) const { __hip_atomic_store(P + i, v, WS_RLX_AGENT); }
  __device__ __forceinline__ uint64_t bload(int i) const { return __hip_atomic_load(best + i, WS_RLX_AGENT); }
  __device__ __forceinline__ void bmin(int i, uint64_t k) const { __hip_atomic_fetch_min(best + i, (unsigned long long)k, WS_RLX_AGENT); }
  __device__ __forceinline__ void bstore(int i, uint64_t k) const { __hip_atomic_store(best + i, (unsigned long long)k, WS_RLX_AGENT); }
  __device__ __forceinline__ int oload(int i) const { return __hip_atomic_load(out + i, WS_RLX_AGENT); }
  __device__ __forceinline__ void ostore(int i, int v) const { __hip_atomic_store(out + i, v, WS_RLX_AGENT); }
  __device__ __forceinline__ bool flagged(int r) const { return __hip_atomic_load(act + r, WS_RLX_AGENT) != 0; }
  __device__ __forceinline__ void flag(int r) const { __hip_atomic_store(act + r, 1, WS_RLX_AGENT); }
};

// every kernel: thread t of the grid takes voxels t, t + T, t + 2 T ... - ceil(n / T) trips at most, n and T fixed by the launch
#define WS_FOR_VOXELS(v, n) \
  for (int64_t v##64 = (int64_t)blockIdx.x * 256 + threadIdx.x; v##64 < (n); v##64 += (int64_t)gridDim.x * 256) \
    if (const int v = (int)v##64; true)

__global__ void __launch_bounds__(64) ws_flags_kernel(int* act, int count) {
  for (int r = threadIdx.x; r < count; r += 64) act[r] = 0;     // count = R + 1 <= 33: one trip
}

__global__ void __launch_bounds__(256) ws_init_kernel(WsDev m, const int* __restrict__ markers, const uint8_t* __restrict__ mask, int64_t n) {
  WS_FOR_VOXELS(v, n) ws_init(m, v, mask == nullptr || mask[v] != 0, markers[v]);
}

__global__ void __launch_bounds__(256) ws_pick_kernel(WsDev m, WsGeom g, WsImage img, int64_t n, int round) {
  if (!m.flagged(round)) return;
  WS_FOR_VOXELS(v, n) ws_pick(m, g, img, v, round);
}

__global__ void __launch_bounds__(256) ws_resolve_kernel(WsDev m, WsGeom g, WsImage img, int64_t n, int round) {
  if (!m.flagged(round + 1)) return;
  WS_FOR_VOXELS(v, n) ws_resolve(m, g, img, v);
}

__global__ void __launch_bounds__(256) ws_unite_kernel(WsDev m, int64_t n, int round) {
  if (!m.flagged(round + 1)) return;
  WS_FOR_VOXELS(v, n) ws_unite(m, v);
}

__global__ void __launch_bounds__(256) ws_flatten_kernel(WsDev m, int64_t n, int round) {
  if (!m.flagged(round + 1)) return;
  WS_FOR_VOXELS(v, n) ws_flatten(m, v);
}

__global__ void __launch_bounds__(256) ws_last_kernel(WsDev m, int64_t n, int R, int* __restrict__ rounds) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *rounds = ws_rounds_used(m, R);
  WS_FOR_VOXELS(v, n) ws_last(m, v);
}

int64_t voxels_of(int Z, int Y, int X) { return (Z < 1 || Y < 1 || X < 1) ? 0 : (int64_t)Z * Y * X; }
int64_t flag_bytes(int64_t n) { return cdiv64((int64_t)(ws_rounds(n) + 1) * 4, 8) * 8; }
// 16 blocks of 256 threads per CU: enough requests in flight for passes that wait on memory, and an early return is 4096 blocks, not n / 256
unsigned grid_of(int64_t n) { return (unsigned)std::min<int64_t>(cdiv64(n, 256), 4096); }

}  // namespace

extern "C" int64_t bpx_watershed_workspace(int Z, int Y, int X) {
  const int64_t n = voxels_of(Z, Y, X);
  if (n < 1 || n >= ((int64_t)1 << 31)) return -1;
  return n * 12 + flag_bytes(n);
}

extern "C" int bpx_watershed(const void* image_d, int image_dtype, const int32_t* markers_d, const uint8_t* mask_d, int Z, int Y, int X,
                             int connectivity, int32_t* out_d, int32_t* rounds_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  const char* fn = "bpx_watershed";
  BPX_CHECK(image_d && markers_d && out_d && rounds_d && ws_d, "%s: null pointer", fn);
  BPX_CHECK(image_dtype == BPX_F32 || image_dtype == BPX_I32, "%s: the image must be BPX_F32 or BPX_I32 (got dtype %d)", fn, image_dtype);
  BPX_CHECK(Z >= 1 && Y >= 1 && X >= 1, "%s: extents must be at least 1 (got %d x %d x %d)", fn, Z, Y, X);
  BPX_CHECK(connectivity >= 1 && connectivity <= 3, "%s: connectivity must be 1, 2 or 3 (got %d)", fn, connectivity);
  const int64_t n = voxels_of(Z, Y, X);
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels: volumes of 2^31 voxels or more are not supported (int32 indices)", fn, (long long)n);
  BPX_CHECK(ws_bytes >= bpx_watershed_workspace(Z, Y, X), "%s: workspace too small (%lld bytes, bpx_watershed_workspace says %lld)", fn,
            (long long)ws_bytes, (long long)bpx_watershed_workspace(Z, Y, X));
  BPX_CHECK((((uintptr_t)image_d | (uintptr_t)markers_d | (uintptr_t)out_d | (uintptr_t)rounds_d) & 3) == 0 && ((uintptr_t)ws_d & 7) == 0,
            "%s: image, markers, out and rounds must be 4-byte aligned, the workspace 8-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  const int R = ws_rounds(n);
  unsigned long long* best = reinterpret_cast<unsigned long long*>(ws_d);
  int* P = reinterpret_cast<int*>(best + n);
  int* act = P + n;
  const WsDev m{P, best, out_d, act};
  const WsGeom g{Z, Y, X, connectivity};
  const WsImage img{reinterpret_cast<const uint32_t*>(image_d), image_dtype == BPX_F32 ? 1 : 0};
  const unsigned nb = grid_of(n);
  ws_flags_kernel<<<1, 64, 0, s>>>(act, R + 1);
  ws_init_kernel<<<nb, 256, 0, s>>>(m, markers_d, mask_d, n);
  for (int r = 0; r < R; ++r) {
    ws_pick_kernel<<<nb, 256, 0, s>>>(m, g, img, n, r);
    ws_resolve_kernel<<<nb, 256, 0, s>>>(m, g, img, n, r);
    ws_unite_kernel<<<nb, 256, 0, s>>>(m, n, r);
    ws_flatten_kernel<<<nb, 256, 0, s>>>(m, n, r);
  }
  ws_last_kernel<<<nb, 256, 0, s>>>(m, n, R, rounds_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
