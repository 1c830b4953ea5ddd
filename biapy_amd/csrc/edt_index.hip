// The exact Euclidean distance transform with the nearest source (biapy_amd/prepost.py: distance_transform_edt(return_indices=...),
// expand_labels, voronoi_on_mask).  A voxel is a SOURCE when its value is 0 (with `invert`: when it is nonzero).  index(v) = the linear index
// (int32, C order over (Z,Y,X)) of the source u with the least |u - v|^2, among equally near ones the smallest linear index - the raster-first
// source; a source's index is its own; -1 everywhere where the volume holds no source, beside the distance sentinel of edt.hip (INT32_MAX /
// +inf).  The distances are those of bpx_edt on the same mask, bit for bit: the same kernels (edt_kernels.h) over the same one-dimensional
// pieces (edt_core.h, with the rule's separable form and its tie behaviour), instantiated with the index.  Here: the entry points of that form.
//
// THE INDEX TRAVELS IN THE STACK ENTRY (a fourth field), not through a second index volume.  A column pass cannot gather from the index volume
// it writes - the query walks a run from its end to its start while sites anywhere in the run are still to be read - so the alternative is a
// ping-pong volume of 4 bytes per voxel in the workspace and one per-lane gather per voxel.  Carried in the stack, both values and indices
// are updated in place (a position is loaded before anything at or beyond it is stored) and each column pass adds one coalesced 4-byte read
// and one coalesced 4-byte write per voxel to the traffic of edt.hip.  The price is LDS: the 32 (fp64: 16) entries a thread keeps there are
// 12 (fp64: 20) bytes each, 24 KiB (20 KiB) per wave where edt.hip has 16, so 6 waves fit a CU's 160 KiB where edt.hip runs 8.  The persistent
// grid is sized to that residency: 98304 threads in flight (6 waves x 256 CUs), both paths.  Which of the two designs is faster has not been
// measured against each other; what this one costs beside the distance-only call is in profiles/edt_index_timing.json.
// INTEGER PATH (sampling == NULL): int32 values in place in dist_d - or, when dist_d is NULL, in 4 more bytes per voxel of workspace; the Z
// pass overwrites each with its final int32 or float32.  FP64 PATH: fp64 values in the workspace, the Z pass writes float32 to dist_d if given.
// WORKSPACE: E = max(T(Z * X) * Y, T(Y * X) * Z) stack entries with T(columns) = min(98304, a quarter of the columns rounded up to 64):
// 12 * E bytes on the integer path (1.125 GiB at 1024^3), 8 bytes per voxel + 20 * E on the fp64 path.
#include "edt_kernels.h"

extern "C" int64_t bpx_edt_index_workspace(int Z, int Y, int X, int fp64_path) { return edt_workspace<true>(Z, Y, X, fp64_path); }

extern "C" int bpx_edt_index(const void* key_d, int key_dtype, int invert, int Z, int Y, int X, const double* sampling, int squared, void* dist_d,
                             int32_t* index_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  const char* fn = "bpx_edt_index";
  BPX_CHECK(key_d && index_d && ws_d, "%s: null pointer", fn);
  if (edt_check_args(fn, key_dtype, Z, Y, X, sampling)) return 1;
  const int64_t n = edt_voxels(Z, Y, X);
  const int fp64 = sampling ? 1 : 0, dist = dist_d ? 1 : 0;
  const int64_t need = bpx_edt_index_workspace(Z, Y, X, fp64) + ((fp64 || dist) ? 0 : n * 4);
  BPX_CHECK(ws_bytes >= need, "%s: workspace too small (%lld bytes; bpx_edt_index_workspace%s says %lld)", fn, (long long)ws_bytes,
            (fp64 || dist) ? "" : " + 4 bytes per voxel for the values of a call without dist_d", (long long)need);
  BPX_CHECK(((uintptr_t)dist_d & 3) == 0 && ((uintptr_t)index_d & 3) == 0 && ((uintptr_t)ws_d & 7) == 0 && (key_dtype != BPX_I32 || ((uintptr_t)key_d & 3) == 0),
            "%s: dist, index and int32 keys must be 4-byte aligned, the workspace 8-byte aligned", fn);
  const EdtKeys<true> keys{key_d, key_dtype == BPX_I32 ? 1 : 0, invert ? 1 : 0};
  // fp64 path: the values in the workspace, the stacks behind them; integer path: the stacks first, the values in dist_d or, when the caller
  // wants none, behind the stacks
  void* stacks = fp64 ? reinterpret_cast<double*>(ws_d) + n : ws_d;
  void* val = fp64 ? ws_d : dist ? dist_d : reinterpret_cast<char*>(ws_d) + bpx_edt_index_workspace(Z, Y, X, 0);
  edt_launch<true>(keys, sampling, Z, Y, X, val, stacks, index_d, reinterpret_cast<float*>(dist_d), squared, dist, (hipStream_t)stream);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
