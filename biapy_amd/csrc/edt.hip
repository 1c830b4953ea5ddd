// Exact Euclidean distance transform of a (Z,Y,X) mask or label volume on the device (biapy_amd/prepost.py: distance_transform_edt,
// label_distance).  out(v) = 0 where key(v) == 0, else the least |u - v|^2 over the voxels u with key(u) != key(v) - its square root on
// request - and a sentinel (INT32_MAX / +inf) where the volume holds no voxel of another key.  The volume border is no source.  Binary mode:
// key = (value != 0), scipy.ndimage.distance_transform_edt bit for bit on a unit grid.  Label mode: key = value, each voxel's distance to the
// nearest voxel that does not carry its label.  The rule, its separability and the one-dimensional pieces: edt_core.h.  The three launches,
// the two paths and the kernels, shared with edt_index.hip: edt_kernels.h.  Here: the entry points of the form without indices.
// WORKSPACE: per column pass T * (column length) stack entries of 8 (integer) / 16 (fp64) bytes with T = edt_threads(columns) <= 131072 and
// <= a quarter of the columns (rounded up to a wave), the larger of the two passes: at most half the bytes of the output on the integer
// path (plus one wave's stacks), 1 GiB at 1024^3.  The fp64 path adds 8 bytes per voxel, in front of the stacks.
#include "edt_kernels.h"

extern "C" int64_t bpx_edt_workspace(int Z, int Y, int X, int fp64_path) { return edt_workspace<false>(Z, Y, X, fp64_path); }

extern "C" int bpx_edt(const void* key_d, int key_dtype, int label_mode, int Z, int Y, int X, const double* sampling, int squared, void* out_d,
                       void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  const char* fn = "bpx_edt";
  BPX_CHECK(key_d && out_d && ws_d, "%s: null pointer", fn);
  if (edt_check_args(fn, key_dtype, Z, Y, X, sampling)) return 1;
  const int64_t need = bpx_edt_workspace(Z, Y, X, sampling ? 1 : 0);
  BPX_CHECK(ws_bytes >= need, "%s: workspace too small (%lld bytes, bpx_edt_workspace says %lld)", fn, (long long)ws_bytes, (long long)need);
  BPX_CHECK(((uintptr_t)out_d & 3) == 0 && ((uintptr_t)ws_d & 7) == 0 && (key_dtype != BPX_I32 || ((uintptr_t)key_d & 3) == 0),
            "%s: out and int32 keys must be 4-byte aligned, the workspace 8-byte aligned", fn);
  const EdtKeys<false> keys{key_d, key_dtype == BPX_I32 ? 1 : 0, label_mode ? 0 : 1};
  // integer path: the values in out_d, the workspace all stacks; fp64 path: the values in the workspace, the stacks behind them
  void* val = sampling ? ws_d : out_d;
  void* stacks = sampling ? reinterpret_cast<double*>(ws_d) + edt_voxels(Z, Y, X) : ws_d;
  edt_launch<false>(keys, sampling, Z, Y, X, val, stacks, nullptr, reinterpret_cast<float*>(out_d), squared, 1, (hipStream_t)stream);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
