// Morphology of a uint8, int32 or float32 volume (Z, Y, X) on the device in one pass: the minimum (erosion), the maximum (dilation) or "they
// differ" (the boundary map) over the structuring element scipy.ndimage.generate_binary_structure(ndim, connectivity) - what stands between
// label(), the distance transform, watershed() and region_props() in the instance workflow (seed maps are eroded, speckle is opened or closed
// away, instance targets get their contour channel from find_boundaries) and took the volume to the host until now.
//
// ONE LAUNCH, fixed by (Z, Y, X, dtype): thread t owns chunk t % chunks of row t / chunks, a chunk being 16 bytes of the row (16 uint8 or 4
// int32 / float32 voxels), and everything it does is morph_core.h's morph_lane: up to nine rows of the element fetched by 16-byte loads where the
// address allows (4-byte loads or single bytes otherwise and at the row's ragged end - the same bits), the voxels x0 - 1 and x0 + V of a wide row
// by an overlapping load, the binary path on 0 / 1 bytes packed in words (AND / OR, byte funnel shifts for x +- 1), the grey paths on elements.
// One read and one write per voxel from memory's side; the nine-fold row reuse is left to the caches (figures: profiles/morph_timing.json,
// DESIGN.md section 4).  No atomics, no workspace, no loop that a launch parameter or a constant does not bound; nothing read back; capturable.
#include "bpx_common.h"
#include "morph_core.h"

namespace {

// LOOP BOUND: none - one chunk per thread; `total` = Z * Y * chunks < 2^31
template <class T, int OP, bool BINARY>
__global__ void __launch_bounds__(256) morph_kernel(const T* __restrict__ in, void* __restrict__ out, int Z, int Y, int X, int ndim, int connectivity,
                                                    int flags, int background, uint32_t chunks, uint32_t total) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= total) return;
  const uint32_t row = t / chunks;
  morph_lane<T, OP, BINARY>(in, out, Z, Y, X, ndim, connectivity, flags, background, (int)(row / (uint32_t)Y), (int)(row % (uint32_t)Y),
                            (int)(t - row * chunks));
}

template <class T>
void launch(int op, bool binary, const void* in, void* out, int Z, int Y, int X, int ndim, int connectivity, int flags, int background, hipStream_t s) {
  const uint32_t chunks = (uint32_t)cdiv(X, MORPH_BYTES / (int)sizeof(T)), total = (uint32_t)((int64_t)Z * Y * chunks);
  const unsigned blocks = (unsigned)cdiv64(total, 256);
  const T* x = static_cast<const T*>(in);
#define MORPH_GO(OP, BIN) morph_kernel<T, OP, BIN><<<blocks, 256, 0, s>>>(x, out, Z, Y, X, ndim, connectivity, flags, background, chunks, total)
  if constexpr (sizeof(T) == 1) {
    if (binary) {
      if (op == MORPH_ERODE) MORPH_GO(MORPH_ERODE, true);
      else MORPH_GO(MORPH_DILATE, true);
      return;
    }
  }
  if (op == MORPH_ERODE) MORPH_GO(MORPH_ERODE, false);
  else if (op == MORPH_DILATE) MORPH_GO(MORPH_DILATE, false);
  else MORPH_GO(MORPH_BOUNDARY, false);
#undef MORPH_GO
}

}  // namespace

extern "C" int bpx_morph(const void* in_d, int dtype, int Z, int Y, int X, int ndim, int connectivity, int op, int flags, int background, void* out_d,
                         bpx_stream_t stream) {
  const char* fn = "bpx_morph";
  BPX_CHECK(in_d && out_d, "%s: null pointer", fn);
  BPX_CHECK(Z >= 1 && Y >= 1 && X >= 1, "%s: extents must be at least 1 (got %d x %d x %d)", fn, Z, Y, X);
  const int64_t n = (int64_t)Z * Y * X;
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels: volumes of 2^31 voxels or more are not supported", fn, (long long)n);
  BPX_CHECK((ndim == 3) || (ndim == 2 && Z == 1), "%s: ndim must be 3, or 2 with Z = 1 (got ndim %d, Z %d)", fn, ndim, Z);
  BPX_CHECK(connectivity >= 1 && connectivity <= ndim, "%s: connectivity must be in 1..%d (got %d)", fn, ndim, connectivity);
  BPX_CHECK(dtype == BPX_U8 || dtype == BPX_I32 || dtype == BPX_F32, "%s: dtype must be uint8, int32 or float32 (got %d)", fn, dtype);
  BPX_CHECK(op == MORPH_ERODE || op == MORPH_DILATE || op == MORPH_BOUNDARY, "%s: unknown op %d (0 erode, 1 dilate, 2 boundary)", fn, op);
  BPX_CHECK((flags & ~MORPH_FLAGS) == 0, "%s: unknown flags %d", fn, flags);
  const bool binary = (flags & MORPH_BINARY) != 0;
  BPX_CHECK(!binary || (dtype == BPX_U8 && op != MORPH_BOUNDARY), "%s: the binary flag takes a uint8 input and erode or dilate", fn);
  BPX_CHECK(!(flags & MORPH_ABSORB) || binary, "%s: the absorbing border is offered on the binary path only", fn);
  BPX_CHECK(!(flags & MORPH_INNER) || op == MORPH_BOUNDARY, "%s: the inner flag belongs to the boundary op", fn);
  BPX_CHECK(out_d != in_d, "%s: out_d must not be in_d (a voxel's neighbours are read after it is written)", fn);
  BPX_CHECK(dtype == BPX_U8 || (((uintptr_t)in_d | (op == MORPH_BOUNDARY ? 0 : (uintptr_t)out_d)) & 3) == 0,
            "%s: int32 / float32 volumes must be 4-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == BPX_U8) launch<uint8_t>(op, binary, in_d, out_d, Z, Y, X, ndim, connectivity, flags, background, s);
  else if (dtype == BPX_I32) launch<int32_t>(op, binary, in_d, out_d, Z, Y, X, ndim, connectivity, flags, background, s);
  else launch<float>(op, binary, in_d, out_d, Z, Y, X, ndim, connectivity, flags, background, s);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
