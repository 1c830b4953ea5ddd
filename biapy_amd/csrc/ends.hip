// The kernels at the two ENDS of a network, where one side of the layer is not a 16-channel NDHWC tensor but the fp32 image or the fp32 logits:
//   first layer (bpx_conv3d_c1_*)    Conv3d 1 -> Cout, k = 3, on the fp32 image: forward with the statistics partials; its weight gradient on the
//                                    matrix cores (with the InstanceNorm backward of its output folded in: _nb) or as a scalar kernel (fp32, W <= 8)
//   rank-1    (bpx_conv1x1_c1_wgrad) weight gradient of the first block's 1 -> Cout shortcut
//   SR "pre"  (bpx_upsample_c1_*)    ConvTranspose3d(1, 1, kernel = stride) on the image into channel 0 of a 16-channel tensor, and its gradients
//   head      (bpx_head_*)           1x1x1 conv of 16 / 32 channels to <= 8 planar fp32 logits with the activations; dx, dW and db in one pass
// They sit together because they are built alike and unlike the streaming kernels of elementwise.hip: tiles with a halo in LDS, MFMAs, persistent
// workgroups with register-staged prefetch, and - every gradient here - one row of fp32 partials per workgroup that bpxred::reduce_partials (wgrad.hip)
// sums in a fixed order.  No atomics.  What they share is written once: the image halo of the first layer (C1Tile), the head backward's body, the
// block sums (block_sums.h), the first layer's launch plan.
#include "block_sums.h"
#include "bpx_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// output head (1x1x1 conv to <= 8 fp32 channels, planar output) and its backward
// ------------------------------------------------------------------------------------------------
// COUT is a template parameter (one instance per channel count 1..8): every channel loop unrolls and a[] stays in registers.  The arithmetic is
// that of the former run-time-Cout kernel, operation for operation (same fmaf chain per channel, same softmax order), so Cout <= 4 is bit-identical.
template <typename T, int CIN, int COUT>
__global__ void __launch_bounds__(256) head_fwd_kernel(const T* __restrict__ x, int x_ld, const float* __restrict__ w,
                                                       const float* __restrict__ b, int act, float* __restrict__ out,
                                                       int64_t sn, int64_t sc, int64_t vps, int N) {
  constexpr int KPL = ElemTraits<T>::KPL;
  __shared__ float ws[COUT * CIN + COUT];
  for (int i = threadIdx.x; i < COUT * CIN; i += blockDim.x) ws[i] = w[i];
  if (threadIdx.x < COUT) ws[COUT * CIN + threadIdx.x] = b ? b[threadIdx.x] : 0.f;
  __syncthreads();
  // per-channel codes, 4 bits each (channel 0 in the low nibble): 0 linear, 1 sigmoid, 2 tanh, 3 softmax - consecutive
  // softmax channels form ONE group (apply_model_activations, base_workflow.py:1403-1457); a head may hold several groups.
  // gend[co]: last channel of the softmax group that starts at co, or -1 (no group starts there)
  int gend[COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
    gend[co] = -1;
    if (((act >> (4 * co)) & 15) == 3 && (co == 0 || ((act >> (4 * (co - 1))) & 15) != 3)) {
      int e = co;
      while (e + 1 < COUT && ((act >> (4 * (e + 1))) & 15) == 3) ++e;
      gend[co] = e;
    }
  }
  const int64_t total = (int64_t)N * vps;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    // the weights are re-read from LDS in every iteration: hoisted out of the loop (the channel loops are unrolled) they took up to
    // COUT * CIN VGPRs - occupancy 8 -> 4 at Cout 4 and AGPR spills at CIN 32
    asm volatile("" ::: "memory");
    float f[CIN];
#pragma unroll
    for (int q = 0; q < CIN / KPL; ++q) unpack16<T>(*reinterpret_cast<const u32x4_t*>(x + (size_t)i * x_ld + q * KPL), f + q * KPL);
    int n = (int)(i / vps);
    int64_t v = i - (int64_t)n * vps;
    float a[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
      a[co] = ws[COUT * CIN + co];
#pragma unroll
      for (int c = 0; c < CIN; ++c) a[co] = fmaf(f[c], ws[co * CIN + c], a[co]);
    }
    // channel order, as before; a group's members are addressed with compile-time indices under the run-time bound e = gend[co]
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
      const int code = (act >> (4 * co)) & 15;
      if (code == 1) a[co] = 1.f / (1.f + expf(-a[co]));
      else if (code == 2) a[co] = tanhf(a[co]);
      else if (gend[co] >= 0) {
        const int e = gend[co];
        float m = a[co];
#pragma unroll
        for (int k = co + 1; k < COUT; ++k) if (k <= e) m = fmaxf(m, a[k]);
        float ssum = 0.f;
#pragma unroll
        for (int k = co; k < COUT; ++k) if (k <= e) { a[k] = expf(a[k] - m); ssum += a[k]; }
#pragma unroll
        for (int k = co; k < COUT; ++k) if (k <= e) a[k] /= ssum;
      }
    }
#pragma unroll
    for (int co = 0; co < COUT; ++co) out[n * sn + co * sc + v] = a[co];
  }
}

// The backward for CS input channels from c0 on, as workgroup column `col` of `ncol`: reads every dout channel but only x[:, c0 ..] and w[:, c0 ..];
// writes dx[:, c0 ..] (no sum across slices) and the dW[:, c0 ..] columns of its column's partial row ([ncol][COUT][Cin]), the bias row
// ([ncol][COUT]) where db is given.  Per thread: dwl[COUT][CS] + o[CS] + f[CS].  fp32 dout, per-thread fmaf chains in channel order, wave shuffles,
// the four waves in a fixed order, then bpxred::reduce_partials over the rows.
// TX: element type of the head's input x (BPX_MIX16: fp16 beside the bf16 gradient dx), else T.  SLICED (the Cout 5..8 kernel): w[:, c0 ..] is
// re-read from LDS for every voxel (see head_fwd_kernel) - the accumulators need the registers the hoisted weights would take.
template <typename T, int CS, int COUT, typename TX, bool SLICED>
__device__ __forceinline__ void head_bwd_body(const TX* __restrict__ x, int x_ld, const float* __restrict__ w, int Cin, const float* __restrict__ dout,
                                              int64_t sn, int64_t sc, T* __restrict__ dx, int dx_ld, float* __restrict__ dw, float* __restrict__ db,
                                              int64_t vps, int N, int c0, int col, int ncol, int nws /* = COUT CS: the weights to stage */) {
  constexpr int KPL = ElemTraits<T>::KPL;
  static_assert(ElemTraits<TX>::KPL == KPL, "x and dx: the same element size");
  __shared__ float ws[COUT * CS];
  for (int i = threadIdx.x; i < nws; i += blockDim.x) ws[i] = w[(i / CS) * Cin + c0 + i % CS];
  __syncthreads();
  float dwl[COUT][CS];
  float dbl[COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
    dbl[co] = 0.f;
#pragma unroll
    for (int c = 0; c < CS; ++c) dwl[co][c] = 0.f;
  }
  const int64_t total = (int64_t)N * vps;
  for (int64_t i = (int64_t)col * blockDim.x + threadIdx.x; i < total; i += (int64_t)ncol * blockDim.x) {
    if constexpr (SLICED) asm volatile("" ::: "memory");
    float f[CS], o[CS];
#pragma unroll
    for (int q = 0; q < CS / KPL; ++q) unpack16<TX>(*reinterpret_cast<const u32x4_t*>(x + (size_t)i * x_ld + c0 + q * KPL), f + q * KPL);
#pragma unroll
    for (int c = 0; c < CS; ++c) o[c] = 0.f;
    int n = (int)(i / vps);
    int64_t v = i - (int64_t)n * vps;
    float d[COUT];   // (SLICED: every channel requested ahead of the chains; else one by one - either kernel loses a wave per SIMD in the other's form)
#pragma unroll
    for (int co = 0; co < (SLICED ? COUT : 0); ++co) d[co] = dout[n * sn + co * sc + v];
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
      if constexpr (!SLICED) d[co] = dout[n * sn + co * sc + v];
      dbl[co] += d[co];
#pragma unroll
      for (int c = 0; c < CS; ++c) { o[c] = fmaf(d[co], ws[co * CS + c], o[c]); dwl[co][c] = fmaf(d[co], f[c], dwl[co][c]); }
    }
#pragma unroll
    for (int q = 0; q < CS / KPL; ++q) *reinterpret_cast<u32x4_t*>(dx + (size_t)i * dx_ld + c0 + q * KPL) = pack16<T>(o + q * KPL);
  }
  // block reduction (wave shuffles, then LDS across the 4 waves) -> one partial per value per workgroup column
  __shared__ float redh[4][COUT * CS + COUT];
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
#pragma unroll
    for (int c = 0; c < CS; ++c) {
      const float a = wave_sum(dwl[co][c]);
      if (ln == 0) redh[wv][co * CS + c] = a;
    }
    const float a = wave_sum(dbl[co]);
    if (ln == 0) redh[wv][COUT * CS + co] = a;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < COUT * CS + COUT; i += blockDim.x) {
    const float sum = four_wave_sum_seq(redh, i);
    if (i < COUT * CS) dw[(size_t)col * (COUT * Cin) + (i / CS) * Cin + c0 + i % CS] = sum;
    else if (db) db[(size_t)col * COUT + (i - COUT * CS)] = sum;
  }
}

// Cout <= 4: every input channel in one workgroup, one workgroup per column.  (Cout is COUT - the instance is chosen by it; as the run-time bound
// of the staging loop it keeps that loop rolled.)
template <typename T, int CIN, int COUT, typename TX = T>
__global__ void __launch_bounds__(256) head_bwd_kernel(const TX* __restrict__ x, int x_ld, const float* __restrict__ w, int Cout,
                                                       const float* __restrict__ dout, int64_t sn, int64_t sc, T* __restrict__ dx,
                                                       int dx_ld, float* __restrict__ dw, float* __restrict__ db, int64_t vps, int N) {
  head_bwd_body<T, CIN, COUT, TX, false>(x, x_ld, w, CIN, dout, sn, sc, dx, dx_ld, dw, db, vps, N, 0, (int)blockIdx.x, (int)gridDim.x, Cout * CIN);
}

// Cout 5..8: the input channels are split into 16-channel slices, one workgroup each (the accumulators of head_bwd_kernel would not fit: COUT = 4 at
// CIN = 32 already takes 256 VGPRs); the bias row comes from slice 0.
// 1-D grid of ncol * (Cin / 16) workgroups: the slices of one column are 8 workgroups apart - the same XCD (workgroups go round-robin over the
// eight), dispatched together - so the halves of one x row are read, and the halves of one dx row written, at about the same time.  With the slice
// in blockIdx.y every column of slice 0 ran before slice 1 began: each x line came from HBM twice and dx went out in half lines (Cin 32, Cout 8:
// 775 us at 4 x 128^3).
template <typename T, int COUT, typename TX = T>
__global__ void __launch_bounds__(256) head_bwd_slice_kernel(const TX* __restrict__ x, int x_ld, const float* __restrict__ w, int Cin,
                                                             const float* __restrict__ dout, int64_t sn, int64_t sc, T* __restrict__ dx,
                                                             int dx_ld, float* __restrict__ dw, float* __restrict__ db, int64_t vps, int N) {
  constexpr int CS = 16;
  const int nsl = Cin / CS, ncol = (int)gridDim.x / nsl;
  const int sl = (int)(blockIdx.x >> 3) % nsl, col = (int)(blockIdx.x / (8 * nsl)) * 8 + (int)(blockIdx.x & 7);
  head_bwd_body<T, CS, COUT, TX, true>(x, x_ld, w, Cin, dout, sn, sc, dx, dx_ld, dw, sl == 0 ? db : nullptr, vps, N, sl * CS, col, ncol, COUT * CS);
}

// ------------------------------------------------------------------------------------------------
// first layer: Cin = 1, k = 3, fp32 image -> 16 output channels per blockIdx.y
// ------------------------------------------------------------------------------------------------
// Implicit GEMM with K = 27 taps (padded to 32 / 28): the image halo tile sits in LDS as fp32, a lane gathers the taps
// of its voxel straight from it.  bf16 storage: the fp32 image value is split into hi + lo bf16 parts (two MFMAs) so the
// raw input keeps ~16 mantissa bits; the weights are rounded to bf16 like every other layer in that mode.
// BUF (round 5): image and output move through BUFFER instructions - a halo voxel outside the volume / a tile beyond the launch's range / an output
// voxel outside the volume uses an out-of-range offset (loads return the zero padding, stores are dropped) instead of a predicate.  With predicated
// loads the compiler's wait at the loop head for the prefetched halo was `s_waitcnt vmcnt(0)` (its wait-count pass gives up at the joins of the
// bounds tests), i.e. a wait for the previous tile's 8 stores as well - what the prefetch-before-the-stores order was meant to avoid; now the
// wait is a counted one that leaves the stores in flight.  The launcher takes BUF when image and output lie within 32-bit byte offsets.

// A TZ x TY x TX tile of the first layer and its image halo (one voxel on every side), staged by 256 threads in NI pieces per thread: piece u of
// thread tid is halo voxel u 256 + tid.  The forward walks C1FwdTile, the MFMA weight gradient C1MfmaTile, the scalar one C1ScalarTile.
template <int TZ_, int TY_, int TX_>
struct C1Tile {
  static constexpr int TZ = TZ_, TY = TY_, TX = TX_, HZ = TZ + 2, HY = TY + 2, HX = TX + 2, HV = HZ * HY * HX, NI = (HV + 255) / 256;
  static int tiles(int D, int H, int W) { return cdiv(D, TZ) * cdiv(H, TY) * cdiv(W, TX); }   // per sample (host)
  // The buffer-addressed plan: the halo voxel (hz, hy, hx) a thread stages is the same for every tile - its coordinates (one packed word per piece)
  // and its offset relative to the tile's first voxel are set up once; a tile costs three unsigned range tests and one add per piece.  (As written
  // for the pointer-addressed form - the divisions by HX / HY inside the tile loop - the five requests were 200 of the forward loop's 1060
  // instructions, and that kernel is bound by instruction issue: ~1000 instructions per tile and wave = the 105 us it takes.)
  uint32_t hpk[NI];
  int hrel[NI];
  __device__ __forceinline__ void plan(int tid, int H, int W) {
#pragma unroll
    for (int u = 0; u < NI; ++u) {
      const int i = u * 256 + tid;
      const int hx = i % HX, hy = (i / HX) % HY, hz = i / (HX * HY);
      hpk[u] = i < HV ? (uint32_t)(hz | (hy << 8) | (hx << 16)) : 0xFFFFFFFFu;
      hrel[u] = ((hz - 1) * H + (hy - 1)) * W + (hx - 1);
    }
  }
  // the halo of the tile at (n, z0, y0, x0) -> pi[], through buffer loads requested unconditionally: a voxel outside the volume, a piece beyond
  // the halo and every piece of a tile that is not `live` (beyond the launch's range) use an out-of-range offset and read the zero padding
  __device__ __forceinline__ void request_buf(__amdgpu_buffer_rsrc_t rs_img, bool live, int n, int z0, int y0, int x0, int D, int H, int W,
                                              float (&pi)[NI]) const {
    const int base = ((n * D + z0) * H + y0) * W + x0;
#pragma unroll
    for (int u = 0; u < NI; ++u) {
      // z0 + hz - 1 in [0, D) <=> (unsigned)(z0 - 1 + hz) < D; a piece beyond the halo has hz = 255: out of every volume the launcher admits
      const uint32_t z = (uint32_t)(z0 - 1) + (hpk[u] & 255u), y = (uint32_t)(y0 - 1) + ((hpk[u] >> 8) & 255u), x = (uint32_t)(x0 - 1) + (hpk[u] >> 16);
      const bool in = live && hpk[u] != 0xFFFFFFFFu && z < (uint32_t)D && y < (uint32_t)H && x < (uint32_t)W;
      pi[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_img, (int)(in ? (uint32_t)(base + hrel[u]) * 4u : 0xFFFFFFF0u), 0, 0));
    }
  }
  // the same through predicated pointer loads (needs no plan; 64-bit offsets)
  static __device__ __forceinline__ void request_ptr(const float* __restrict__ img, int tid, int n, int z0, int y0, int x0, int D, int H, int W,
                                                     float (&pi)[NI]) {
#pragma unroll
    for (int u = 0; u < NI; ++u) {
      const int i = u * 256 + tid;
      const int hx = i % HX, hy = (i / HX) % HY, hz = i / (HX * HY);
      const int z = z0 + hz - 1, y = y0 + hy - 1, x = x0 + hx - 1;
      pi[u] = (i < HV && z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W) ? img[(((size_t)n * D + z) * H + y) * W + x] : 0.f;
    }
  }
};
using C1FwdTile = C1Tile<4, 8, 16>;
using C1MfmaTile = C1Tile<4, 4, 16>;
using C1ScalarTile = C1Tile<4, 8, 8>;

template <typename T, bool BUF>
__global__ void __launch_bounds__(256) conv_c1_fwd_kernel(const float* __restrict__ img, const float* __restrict__ w /* (Cout,1,27) */,
                                                          const float* __restrict__ bias, T* __restrict__ y, int y_ld, int Cout, int D,
                                                          int H, int W, int tilesY, int tilesX, int tilesPerSample, float* __restrict__ part, int totalTiles,
                                                          uint32_t img_bytes, uint32_t y_bytes) {
  constexpr bool BF = sizeof(T) == 2;   // 16-bit storage (bf16 bits or fp16): hi + lo split of the fp32 image, two MFMAs
  using Tile = C1FwdTile;
  constexpr int TZ = Tile::TZ, TY = Tile::TY, TX = Tile::TX, HY = Tile::HY, HX = Tile::HX, HV = Tile::HV, NI = Tile::NI, MS = 8;
  __shared__ float simg[HV];
  __shared__ float red[4][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int cb = blockIdx.y * 16;
  // Round 4: persistent workgroups.  As one workgroup per tile the kernel was bound by the LIFE of a workgroup - image load latency, 16 MFMAs,
  // then its stores' write acknowledgements before the slot frees - at 2.1 TB/s written (0.144 ms at 4 x 128^3).  The image halo of the NEXT tile
  // is requested into registers (five floats per thread) BEFORE this tile's stores: a wave's VMEM operations retire in order, so the wait for
  // those loads then leaves the stores outstanding; weights / tap offsets / bias are set up once.
  float pi[NI];
  const __amdgpu_buffer_rsrc_t rs_img = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(img), 0, (int)img_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc(y, 0, (int)y_bytes, 0x00020000);
  Tile halo;
  if constexpr (BUF) halo.plan(tid, H, W);
  auto issue = [&](int tt) {
    const int n_ = tt / tilesPerSample, tile_ = tt - n_ * tilesPerSample;
    const int x0_ = (tile_ % tilesX) * TX, y0_ = ((tile_ / tilesX) % tilesY) * TY, z0_ = (tile_ / (tilesX * tilesY)) * TZ;
    if constexpr (BUF) halo.request_buf(rs_img, tt < totalTiles, n_, z0_, y0_, x0_, D, H, W, pi);
    else Tile::request_ptr(img, tid, n_, z0_, y0_, x0_, D, H, W, pi);
  };
  if (BUF || (int)blockIdx.x < totalTiles) issue(blockIdx.x);
  // weight operand of this lane: output channel cb + j, taps 8g..8g+7 (bf16) or 4s+g (f32)
  u32x4_t wa = u32x4_t{0u, 0u, 0u, 0u};
  float wf32[7];
  int toff[BF ? 8 : 7];
  if constexpr (BF) {
    float wv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int t = 8 * g + e;
      wv[e] = t < 27 ? w[(size_t)(cb + j) * 27 + t] : 0.f;
      int tc = t < 27 ? t : 26;
      toff[e] = ((tc / 9) * HY + (tc / 3) % 3) * HX + tc % 3;
    }
    wa = pack16<T>(wv);
  } else {
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      int t = 4 * s + g;
      wf32[s] = t < 27 ? w[(size_t)(cb + j) * 27 + t] : 0.f;
      int tc = t < 27 ? t : 26;
      toff[s] = ((tc / 9) * HY + (tc / 3) % 3) * HX + tc % 3;
    }
  }
  float bsv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bsv[r] = bias ? bias[cb + 4 * g + r] : 0.f;
  for (int tt = blockIdx.x; tt < totalTiles; tt += gridDim.x) {
  const int n = tt / tilesPerSample, tile = tt - n * tilesPerSample;
  const int x0 = (tile % tilesX) * TX, y0 = ((tile / tilesX) % tilesY) * TY, z0 = (tile / (tilesX * tilesY)) * TZ;
  __syncthreads();                                   // the previous tile's reads of simg / red are done
  // 16-bit storage (round 5): the hi + lo split happens HERE, once per halo voxel (5 values per thread), and LDS holds the pair as one word
  // (hi in the low half); the gather below then builds the two MFMA operands with two byte permutes per pair of taps.  Before, every lane split
  // the 8 gathered taps of each of its 8 voxels itself: 24 conversions / subtractions per m-subtile, ~40 % of the kernel's VALU work.  Same
  // conversions of the same values: same bits.
#pragma unroll
  for (int u = 0; u < NI; ++u)
    if (u * 256 + tid < HV) {
      if constexpr (BF) {
        const float f = pi[u];
        const float hf = lo16<T>(pk16<T>(f, 0.f));
        simg[u * 256 + tid] = __uint_as_float(pk16<T>(f, f - hf));
      } else {
        simg[u * 256 + tid] = pi[u];
      }
    }
  __syncthreads();
  if (BUF || tt + (int)gridDim.x < totalTiles) issue(tt + gridDim.x);   // (BUF: a tile beyond the range requests nothing - every lane out of range)
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  const uint32_t ybase = ((uint32_t)(((n * D + z0 + wave) * H + y0) * W + x0 + j) * (uint32_t)y_ld + (uint32_t)(cb + 4 * g)) * (uint32_t)sizeof(T);
  const uint32_t yrowb = (uint32_t)(W * y_ld) * (uint32_t)sizeof(T);
  const bool full = z0 + TZ <= D && y0 + TY <= H && x0 + TX <= W;       // (uniform)
  f32x2_t p1[2] = {f32x2_t{0.f, 0.f}, f32x2_t{0.f, 0.f}}, p2[2] = {f32x2_t{0.f, 0.f}, f32x2_t{0.f, 0.f}};   // BUF: s1 / s2 as pairs
#pragma unroll
  for (int ms = 0; ms < MS; ++ms) {
    int t = (wave * MS + ms) * 16 + j;
    int tz = t / (TY * TX), ty = (t / TX) % TY, tx = t % TX;
    const float* base = simg + (tz * HY + ty) * HX + tx;
    f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if constexpr (BF) {
      uint32_t v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = __float_as_uint(base[toff[e]]);
      u32x4_t hi, lov;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        hi[k] = __builtin_amdgcn_perm(v[2 * k + 1], v[2 * k], 0x05040100u);    // the low halves (hi parts) of taps 2k, 2k + 1
        lov[k] = __builtin_amdgcn_perm(v[2 * k + 1], v[2 * k], 0x07060302u);   // the high halves (lo parts)
      }
      acc = mfma_step<T>(wa, hi, acc);
      acc = mfma_step<T>(wa, lov, acc);
    } else {
#pragma unroll
      for (int s = 0; s < 7; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf32[s], base[toff[s]], acc, 0, 0, 0);
    }
    int z = z0 + tz, yy = y0 + ty, x = x0 + tx;
    const bool inside = z < D && yy < H && x < W;
    if constexpr (BUF) {
      // (packed fp32 pairs: the same additions / multiplications, half the instructions; the outside-the-volume select only on a partial tile)
      const f32x2_t va = f32x2_t{acc[0], acc[1]} + f32x2_t{bsv[0], bsv[1]}, vb = f32x2_t{acc[2], acc[3]} + f32x2_t{bsv[2], bsv[3]};
      const float v4[4] = {va[0], va[1], vb[0], vb[1]};
      f32x2_t sa = va, sb = vb;
      if (!full && !inside) sa = sb = f32x2_t{0.f, 0.f};
      p1[0] = p1[0] + sa; p1[1] = p1[1] + sb;
      p2[0] = p2[0] + sa * sa; p2[1] = p2[1] + sb * sb;
      // (t = (wave MS + ms) 16 + j: tz = wave, ty = ms, tx = j - the voxel's offset is the m-subtile-0 offset of this lane + ms rows)
      const uint32_t off = inside ? ybase + (uint32_t)ms * yrowb : 0xFFFFFFF0u;
      if constexpr (BF) __builtin_amdgcn_raw_buffer_store_b64(u32x2_t{pk16s<T>(v4[0], v4[1]), pk16s<T>(v4[2], v4[3])}, rs_y, (int)off, 0, 0);
      else __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{__float_as_uint(v4[0]), __float_as_uint(v4[1]), __float_as_uint(v4[2]), __float_as_uint(v4[3])}, rs_y, (int)off, 0, 0);
    } else if (inside) {
      float v4[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) { v4[r] = acc[r] + bsv[r]; s1[r] += v4[r]; s2[r] += v4[r] * v4[r]; }
      T* yp = y + ((((size_t)n * D + z) * H + yy) * W + x) * (size_t)y_ld + cb + 4 * g;
      if constexpr (BF) *reinterpret_cast<u32x2_t*>(yp) = u32x2_t{pk16s<T>(v4[0], v4[1]), pk16s<T>(v4[2], v4[3])};
      else *reinterpret_cast<f32x4_t*>(yp) = f32x4_t{v4[0], v4[1], v4[2], v4[3]};
    }
  }
  if (part) {
    if constexpr (BUF) {
      const f32x2_t q0 = p1[0], q1 = p1[1], q2 = p2[0], q3 = p2[1];   // (copies first: elements of an array of vectors, see bpx_common.h)
      s1[0] = q0[0]; s1[1] = q0[1]; s1[2] = q1[0]; s1[3] = q1[1];
      s2[0] = q2[0]; s2[1] = q2[1]; s2[2] = q3[0]; s2[3] = q3[1];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // (row16_sum pairs lanes as the xor butterfly it replaces did - 1, 2, then the other quad of the half, then the other half - the same
      //  additions of the same values: same bits; four DPP adds instead of four cross-lane shuffles each)
      const float a = row16_sum(s1[r]), b = row16_sum(s2[r]);
      if (j == 0) { red[wave][4 * g + r] = a; red[wave][16 + 4 * g + r] = b; }
    }
    __syncthreads();
    if (tid < 32) {
      int k = tid >> 4, c = tid & 15;
      float s = red[0][k * 16 + c] + red[1][k * 16 + c] + red[2][k * 16 + c] + red[3][k * 16 + c];
      part[(((size_t)n * tilesPerSample + tile) * 2 + k) * Cout + cb + c] = s;
    }
  }
  }   // tiles of this workgroup
}

// dW[co][tap] += sum_v img[v+tap]*dy[v][co]; thread = (tap, voxel subset), 16 co in registers.
template <typename T>
__global__ void __launch_bounds__(256) conv_c1_wgrad_kernel(const float* __restrict__ img, const T* __restrict__ dy, int dy_ld,
                                                            int D, int H, int W, int N, int totalTiles, float* __restrict__ dw,
                                                            float* __restrict__ db) {
  using Tile = C1ScalarTile;
  constexpr int TZ = Tile::TZ, TY = Tile::TY, TX = Tile::TX, HY = Tile::HY, HX = Tile::HX, HV = Tile::HV;
  __shared__ float simg[HV];
  __shared__ __attribute__((aligned(16))) float sdy[TZ * TY * TX][16];
  __shared__ float sred[9][27 + 1][16];
  const int cb = blockIdx.y * 16;
  const int tap = threadIdx.x % 27, sub = threadIdx.x / 27;  // sub 0..8 active (243 threads)
  const bool worker = threadIdx.x < 243;
  const int toff = ((tap / 9) * HY + (tap / 3) % 3) * HX + tap % 3;
  float acc[16], bs[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) { acc[c] = 0.f; bs[c] = 0.f; }
  const int tilesX = cdiv(W, TX), tilesY = cdiv(H, TY), tilesZ = cdiv(D, TZ);
  const int tps = tilesX * tilesY * tilesZ;
  for (int tt = blockIdx.x; tt < totalTiles; tt += gridDim.x) {
    const int n = tt / tps, tile = tt % tps;
    const int x0 = (tile % tilesX) * TX, y0 = ((tile / tilesX) % tilesY) * TY, z0 = (tile / (tilesX * tilesY)) * TZ;
    __syncthreads();
    {
      float pi[Tile::NI];
      Tile::request_ptr(img, threadIdx.x, n, z0, y0, x0, D, H, W, pi);
#pragma unroll
      for (int u = 0; u < Tile::NI; ++u)
        if (u * 256 + (int)threadIdx.x < HV) simg[u * 256 + threadIdx.x] = pi[u];
    }
    {  // dy tile -> fp32 in LDS, moved as 16-byte pieces (KPL channels per piece)
      constexpr int KPL = ElemTraits<T>::KPL, PPV = 16 / KPL;
#pragma unroll
      for (int u = 0; u < TZ * TY * TX * PPV / 256; ++u) {
        const int i = u * 256 + threadIdx.x, t = i / PPV, sp = i % PPV;
        const int x = x0 + t % TX, y = y0 + (t / TX) % TY, z = z0 + t / (TX * TY);
        float f[KPL];
#pragma unroll
        for (int e = 0; e < KPL; ++e) f[e] = 0.f;
        if (z < D && y < H && x < W)
          unpack16<T>(*reinterpret_cast<const u32x4_t*>(dy + ((((size_t)n * D + z) * H + y) * W + x) * dy_ld + cb + sp * KPL), f);
#pragma unroll
        for (int q = 0; q < KPL / 4; ++q)
          *reinterpret_cast<f32x4_t*>(&sdy[t][sp * KPL + q * 4]) = f32x4_t{f[q * 4], f[q * 4 + 1], f[q * 4 + 2], f[q * 4 + 3]};
      }
    }
    __syncthreads();
    if (worker) {
      for (int t = sub; t < TZ * TY * TX; t += 9) {
        int tx = t % TX, ty = (t / TX) % TY, tz = t / (TX * TY);
        float iv = simg[(tz * HY + ty) * HX + tx + toff];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4_t d = *reinterpret_cast<const f32x4_t*>(&sdy[t][q * 4]);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[q * 4 + e] = fmaf(iv, d[e], acc[q * 4 + e]);
            if (tap == 0) bs[q * 4 + e] += d[e];
          }
        }
      }
    }
  }
  __syncthreads();
  if (worker) {
#pragma unroll
    for (int c = 0; c < 16; ++c) { sred[sub][tap][c] = acc[c]; if (tap == 0) sred[sub][27][c] = bs[c]; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 28 * 16; i += 256) {
    int t = i / 16, c = i % 16;
    float s = 0.f;
    for (int q = 0; q < 9; ++q) s += sred[q][t][c];
    // partial slab of this workgroup column: dw = [gridDim.x][27][Cout], db = [gridDim.x][Cout] (Cout = 16 * gridDim.y)
    const int Cout = 16 * gridDim.y;
    if (t < 27) dw[((size_t)blockIdx.x * 27 + t) * Cout + cb + c] = s;
    else if (db) db[(size_t)blockIdx.x * Cout + cb + c] = s;
  }
}


// The same on the matrix cores (bf16 dy): D[tap][co] += sum_v A[tap][v] * G[v][co] with K = 32 voxels per MFMA step.
// A = image patches (fp32 in LDS, split hi + lo into two bf16 operands exactly like conv_c1_fwd_kernel, so the image keeps
// ~16 mantissa bits), two 16-row blocks for the 27 taps; row 27 is all ones -> D[27][co] = sum_v dy = the bias gradient.
// G = dy^T fragments through ds_read_b64_tr_b16.  Wave w owns K-chunks {2w, 2w+1} of every 4x4x16 tile.
// NB (round 4): dy is not read but formed on the way into LDS from the InstanceNorm-backward operands of the layer's output,
//   dy = a[n,c] * g + b[n,c] * t + c0[n,c]   (bpx_norm_bwd_finalize's coefficients; t = the conv's raw output, TT = fp16 in the mixed mode)
// in the arithmetic of norm_bwd_apply_kernel and rounded to bf16 as that kernel's store would: the pass that wrote dy (3 tensor units of
// traffic at 128^3, 139 us per cfg-2 step) is gone and this kernel reads two units instead of one.
// BUF (round 5): image, dy and t arrive through buffer loads with out-of-range offsets for voxels outside the volume and for tiles beyond the
// launch, requested unconditionally.  With predicated loads every wait for a staged tile was `s_waitcnt vmcnt(0)` (the wait-count pass gives up at
// the joins of the bounds tests): the wait for tile i also waited for tile i + 1's requests, issued later - the two-tiles-ahead staging ran one
// tile ahead.  The sample's coefficients are re-read behind a SCALAR branch (they were re-loaded for every tile: 8 more 16-byte loads per thread,
// as many VMEM instructions as the tile's own operands).
template <typename TT, bool NB, bool BUF>
__global__ void __launch_bounds__(256) conv_c1_wgrad_mfma_kernel(const float* __restrict__ img, const uint16_t* __restrict__ dy, int dy_ld,
                                                                 int D, int H, int W, int N, int totalTiles, float* __restrict__ dw,
                                                                 float* __restrict__ db, const TT* __restrict__ tsrc, int t_ld,
                                                                 const bpx_nbwd_coef* __restrict__ coef, uint32_t img_bytes, uint32_t dy_bytes,
                                                                 uint32_t t_bytes) {
  using Tile = C1MfmaTile;
  constexpr int TZ = Tile::TZ, TY = Tile::TY, TX = Tile::TX, TV = TZ * TY * TX, HY = Tile::HY, HX = Tile::HX, HV = Tile::HV, NI = Tile::NI;
  constexpr int VBG = 32;
  __shared__ float simg[HV + 8];
  __shared__ __attribute__((aligned(16))) unsigned char sG[TV * VBG];
  __shared__ float sred[4][2][64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int cb = blockIdx.y * 16;
  f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
  // this lane's two taps (rows i and 16 + i) as float offsets into the halo image; row 27 = ones, rows 28..31 unused
  int toff[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int tap = b * 16 + i;
    toff[b] = tap < 27 ? ((tap / 9) * HY + (tap / 3) % 3) * HX + tap % 3 : -1;
  }
  const int tilesX = cdiv(W, TX), tilesY = cdiv(H, TY), tilesZ = cdiv(D, TZ);
  const int tps = tilesX * tilesY * tilesZ;
  // register-prefetched staging, TWO tiles ahead (round 4; one tile ahead until then): the MFMA part is tiny, the kernel is pure load latency - with
  // the operands of one tile in flight per workgroup an iteration was a full memory latency (3.3 TB/s with the folded IN-backward operands)
  struct Stage { float pi[NI]; u32x4_t pg[2]; u32x4_t pt[NB ? 2 : 1]; };
  Stage st0, st1;
  f32x4_t ck[NB ? 8 : 1];   // {a, b, c0, -} of this thread's 8 channels in the current sample
  int cur_n = -1;
  const __amdgpu_buffer_rsrc_t rs_img = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(img), 0, (int)img_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_dy = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(dy), 0, (int)dy_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_t = __builtin_amdgcn_make_buffer_rsrc(const_cast<TT*>(tsrc), 0, (int)t_bytes, 0x00020000);
  // BUF: this thread's halo voxels (the tile's plan) and tile voxels are the same for every tile
  Tile halo;
  if constexpr (BUF) halo.plan(tid, H, W);
  auto issue = [&](int tt, Stage& sg) {
    const int n = tt / tps, tile = tt % tps;
    const int x0 = (tile % tilesX) * TX, y0 = ((tile / tilesX) % tilesY) * TY, z0 = (tile / (tilesX * tilesY)) * TZ;
    if constexpr (BUF) {
      const bool live = tt < totalTiles;
      halo.request_buf(rs_img, live, n, z0, y0, x0, D, H, W, sg.pi);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int q = u * 256 + tid, t = q >> 1;
        const int x = x0 + (t & 15), y = y0 + ((t >> 4) & 3), z = z0 + (t >> 6);
        const bool in = live && z < D && y < H && x < W;
        const uint32_t v = (uint32_t)(((n * D + z) * H + y) * W + x);
        sg.pg[u] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rs_dy, (int)(in ? (v * (uint32_t)dy_ld + (uint32_t)(cb + (q & 1) * 8)) * 2u : 0xFFFFFFF0u), 0, 0));
        if (NB) sg.pt[NB ? u : 0] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rs_t, (int)(in ? (v * (uint32_t)t_ld + (uint32_t)(cb + (q & 1) * 8)) * 2u : 0xFFFFFFF0u), 0, 0));
      }
    } else {
      Tile::request_ptr(img, tid, n, z0, y0, x0, D, H, W, sg.pi);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int q = u * 256 + tid, t = q >> 1;
        const int x = x0 + (t & 15), y = y0 + ((t >> 4) & 3), z = z0 + (t >> 6);
        sg.pg[u] = u32x4_t{0u, 0u, 0u, 0u};
        if (NB) sg.pt[NB ? u : 0] = u32x4_t{0u, 0u, 0u, 0u};
        if (z < D && y < H && x < W) {
          const size_t v = (((size_t)n * D + z) * H + y) * W + x;
          sg.pg[u] = *reinterpret_cast<const u32x4_t*>(dy + v * dy_ld + cb + (q & 1) * 8);
          if (NB) sg.pt[NB ? u : 0] = *reinterpret_cast<const u32x4_t*>(tsrc + v * t_ld + cb + (q & 1) * 8);
        }
      }
    }
  };
  // the staged dy piece: as loaded, or a * g + b * t + c0 (out-of-volume voxels stay zero: their operands were never loaded)
  auto piece = [&](int u, int tt, const Stage& sg) -> u32x4_t {
    if (!NB) return sg.pg[u];
    const int q = u * 256 + tid, t = q >> 1;
    const int tile = tt % tps;
    const int x = (tile % tilesX) * TX + (t & 15), y = ((tile / tilesX) % tilesY) * TY + ((t >> 4) & 3), z = (tile / (tilesX * tilesY)) * TZ + (t >> 6);
    const bool inside = z < D && y < H && x < W;
    if (!BUF && !inside) return u32x4_t{0u, 0u, 0u, 0u};
    float gf[8], tf[8], of[8];
    unpack16<uint16_t>(sg.pg[u], gf);
    unpack16<TT>(sg.pt[NB ? u : 0], tf);
#pragma unroll
    for (int e = 0; e < 8; ++e) { const f32x4_t k = ck[NB ? e : 0]; of[e] = k[0] * gf[e] + k[1] * tf[e] + k[2]; }
    const u32x4_t r = pack16<uint16_t>(of);
    if (BUF) return inside ? r : u32x4_t{0u, 0u, 0u, 0u};          // (a select: no branch between the staged loads and their consumers)
    return r;
  };
  const int step = gridDim.x;
  if (BUF || (int)blockIdx.x < totalTiles) issue(blockIdx.x, st0);
  if (BUF || (int)blockIdx.x + step < totalTiles) issue(blockIdx.x + step, st1);
  auto body = [&](int tt, Stage& sg) {
    if (NB) {
      const int n = BUF ? __builtin_amdgcn_readfirstlane(tt / tps) : tt / tps;
      if (n != (BUF ? __builtin_amdgcn_readfirstlane(cur_n) : cur_n)) {   // (a handful of times per workgroup; BUF: a scalar branch)
        cur_n = n;
        if constexpr (BUF) {
          // through the SCALAR cache (uniform addresses, lgkmcnt): as vector loads they would be the youngest VMEM operations at the staged tile's first
          // use, and the wait for them - on every path, the counts are static - a wait for the prefetched tiles behind them
          const f32x4_t* kp = reinterpret_cast<const f32x4_t*>(coef + (size_t)n * (16 * gridDim.y) + cb);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const f32x4_t lo = kp[e], hi = kp[8 + e];
            ck[NB ? e : 0] = (tid & 1) ? hi : lo;
          }
        } else {
          const f32x4_t* kp = reinterpret_cast<const f32x4_t*>(coef + (size_t)n * (16 * gridDim.y) + cb + (tid & 1) * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) ck[NB ? e : 0] = kp[e];
        }
      }
    }
    __syncthreads();
    // (round 5) the hi + lo bf16 split once per halo voxel, the pair as one LDS word (hi in the low half) - see conv_c1_fwd_kernel
#pragma unroll
    for (int u = 0; u < NI; ++u)
      if (u * 256 + tid < HV) {
        const float f = sg.pi[u];
        simg[u * 256 + tid] = __uint_as_float(cvt_pk_bf16(f, f - bf16lo(cvt_pk_bf16(f, 0.f))));
      }
#pragma unroll
    for (int u = 0; u < 2; ++u) *reinterpret_cast<u32x4_t*>(sG + (size_t)(u * 256 + tid) * 16) = piece(u, tt, sg);
    __syncthreads();
    if (BUF || tt + 2 * step < totalTiles) issue(tt + 2 * step, sg);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int kc = wave * 2 + kk;
      const int t0 = kc * 32 + g * 8;                       // 8 consecutive x voxels of one row
      const int hb = (((t0 >> 6) + 0) * HY + ((t0 >> 4) & 3)) * HX + (t0 & 15);
      u32x4_t gf;
      {
        const unsigned char* q = sG + (t0 + (i >> 2)) * VBG + (i & 3) * 8;
        s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(q));
        s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(q + 4 * VBG));
        u32x2_t l2 = __builtin_bit_cast(u32x2_t, lo), h2 = __builtin_bit_cast(u32x2_t, hi);
        gf = u32x4_t{l2[0], l2[1], h2[0], h2[1]};
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        uint32_t f[8];   // {hi | lo << 16} words; the ones row: bf16(1) = 0x3F80 with lo part 0
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = toff[b] >= 0 ? __float_as_uint(simg[hb + toff[b] + k]) : ((b == 1 && i == 11) ? 0x3F80u : 0u);
        u32x4_t ah, al;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          ah[k] = __builtin_amdgcn_perm(f[2 * k + 1], f[2 * k], 0x05040100u);
          al[k] = __builtin_amdgcn_perm(f[2 * k + 1], f[2 * k], 0x07060302u);
        }
        acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ah), __builtin_bit_cast(bf16x8_t, gf), acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, al), __builtin_bit_cast(bf16x8_t, gf), acc[b], 0, 0, 0);
      }
    }
  };
  if constexpr (BUF) {
    // pairs of tiles in a loop whose every trip runs both bodies, the odd last tile behind it: with the second body under a test inside the loop
    // there is a static path on which stage 1 was not refilled, and the first body's waits are counted for THAT path (vmcnt(6 .. 0): a wait for
    // stage 1's requests as well)
    int tt = blockIdx.x;
    for (; tt + step < totalTiles; tt += 2 * step) {
      body(tt, st0);
      body(tt + step, st1);
    }
    if (tt < totalTiles) body(tt, st0);
  } else {
    for (int tt = blockIdx.x; tt < totalTiles; tt += 2 * step) {
      body(tt, st0);
      if (tt + step < totalTiles) body(tt + step, st1);
    }
  }
  // lane holds D[row = 4g + r][co = i] of each block: sum the four waves, then one partial per (tap, co) and workgroup
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) sred[wave][b][lane][r] = acc[b][r];
  __syncthreads();
  for (int q = tid; q < 2 * 64 * 4; q += 256) {
    const int r = q & 3, ln = (q >> 2) & 63, b = q >> 8;
    const float sum = sred[0][b][ln][r] + sred[1][b][ln][r] + sred[2][b][ln][r] + sred[3][b][ln][r];
    const int row = b * 16 + 4 * (ln >> 4) + r, co = ln & 15;
    const int Cout = 16 * gridDim.y;
    if (row < 27) dw[((size_t)blockIdx.x * 27 + row) * Cout + cb + co] = sum;
    else if (row == 27 && db) db[(size_t)blockIdx.x * Cout + cb + co] = sum;
  }
}

// shortcut of the first block (Conv3d 1 -> Cout, k = 1): dW[co] += sum_v img[v]*dy[v][co]; 16 channels per blockIdx.y
template <typename T>
__global__ void __launch_bounds__(256) rank1_wgrad_kernel(const float* __restrict__ img, const T* __restrict__ dy, int dy_ld, int64_t total,
                                                          float* __restrict__ dw) {
  constexpr int KPL = ElemTraits<T>::KPL;
  const int cb = blockIdx.y * 16;
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.f;
  // four voxels in flight per thread: with one, the 32 iterations of a thread were a chain of memory latencies (138 us for
  // 268 MB); the order of the additions into acc[] is unchanged
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; v + 3 * stride < total; v += 4 * stride) {
    float iv[4];
    u32x4_t raw[4][16 / KPL];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      iv[u] = img[v + u * stride];
#pragma unroll
      for (int q = 0; q < 16 / KPL; ++q) raw[u][q] = *reinterpret_cast<const u32x4_t*>(dy + (size_t)(v + u * stride) * dy_ld + cb + q * KPL);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float f[16];
#pragma unroll
      for (int q = 0; q < 16 / KPL; ++q) unpack16<T>(raw[u][q], f + q * KPL);
#pragma unroll
      for (int c = 0; c < 16; ++c) acc[c] = fmaf(iv[u], f[c], acc[c]);
    }
  }
  for (; v < total; v += stride) {
    float iv = img[v], f[16];
#pragma unroll
    for (int q = 0; q < 16 / KPL; ++q) unpack16<T>(*reinterpret_cast<const u32x4_t*>(dy + (size_t)v * dy_ld + cb + q * KPL), f + q * KPL);
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = fmaf(iv, f[c], acc[c]);
  }
  __shared__ float redr[4][16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = wave_sum(acc[c]);
  four_wave_hand_over(acc, redr);
  if (threadIdx.x < 16)   // partial row of this workgroup column: [gridDim.x][Cout]
    dw[(size_t)blockIdx.x * (16 * gridDim.y) + cb + threadIdx.x] = four_wave_sum_seq(redr, threadIdx.x);
}

}  // namespace

// ---- super-resolution "pre" up-sampling of the 1-channel input image (biapy/models/resunet.py:206-213, :368-369):
// ConvTranspose3d(1, 1, kernel = stride = (fz, fy, fx)), out[n, fz*z+a, fy*y+b, fx*x+c] = img[n,z,y,x] * w[a][b][c] + bias, written as
// channel 0 of a 16-channel NDHWC tensor of the storage dtype (channels 1..15 = 0): the first residual block then runs on the
// generic 16-channel kernels (its 1-input-channel weights zero-padded), which also yield the gradient of the up-sampled image.
template <typename T>
__global__ void __launch_bounds__(256) upsample_c1_fwd_kernel(const float* __restrict__ img, const float* __restrict__ w, const float* __restrict__ b,
                                                              T* __restrict__ out16, int D, int H, int W, int fz, int fy, int fx, int64_t total) {
  constexpr int KPL = ElemTraits<T>::KPL;
  const int Ho = H * fy, Wo = W * fx, Do = D * fz;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    int64_t r = v;
    const int xo = (int)(r % Wo); r /= Wo;
    const int yo = (int)(r % Ho); r /= Ho;
    const int zo = (int)(r % Do);
    const int64_t n = r / Do;
    const int z = zo / fz, a = zo - z * fz, y = yo / fy, bb = yo - y * fy, x = xo / fx, c = xo - x * fx;
    const float val = img[((n * D + z) * H + y) * (int64_t)W + x] * w[(a * fy + bb) * fx + c] + b[0];
    float f[8] = {val, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float zz[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<u32x4_t*>(out16 + v * 16) = pack16<T>(f);
#pragma unroll
    for (int q = 1; q < 16 / KPL; ++q) *reinterpret_cast<u32x4_t*>(out16 + v * 16 + q * KPL) = pack16<T>(zz);
  }
}

// gradients of the layer above: grid (blocks, taps): block (bx, t) sums img * g and g over its share of the INPUT voxels for tap
// t = (a*fy + b)*fx + c, g = channel 0 of dx16 at the tap's output voxel -> part[(t*gridDim.x + bx)*2 + {0,1}] (deterministic).
template <typename T>
__global__ void __launch_bounds__(256) upsample_c1_bwd_kernel(const float* __restrict__ img, const T* __restrict__ dx16, int D, int H, int W, int fz,
                                                              int fy, int fx, int64_t total_in, float* __restrict__ part) {
  const int t = blockIdx.y;
  const int c = t % fx, bb = (t / fx) % fy, a = t / (fx * fy);
  const int Ho = H * fy, Wo = W * fx, Do = D * fz;
  float sw = 0.f, sg = 0.f;   // sum img g (the tap's weight gradient), sum g (its share of the bias gradient)
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total_in; v += (int64_t)gridDim.x * 256) {
    int64_t r = v;
    const int x = (int)(r % W); r /= W;
    const int y = (int)(r % H); r /= H;
    const int z = (int)(r % D);
    const int64_t n = r / D;
    const int64_t vo = ((n * Do + (int64_t)z * fz + a) * Ho + (int64_t)y * fy + bb) * Wo + (int64_t)x * fx + c;
    const float g = ElemTraits<T>::ld(dx16 + vo * 16);
    sw += img[v] * g;
    sg += g;
  }
  __shared__ float red[4][2];
  const float ws[2] = {wave_sum(sw), wave_sum(sg)};
  four_wave_hand_over(ws, red);
  if (threadIdx.x < 2) part[((size_t)t * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = four_wave_sum_seq(red, threadIdx.x);
}

extern "C" int bpx_head_fwd(int dtype, int64_t vps, int N, bpx_tensor x, const float* w_d, const float* b_d, int Cout, int head_act,
                            float* out_d, int64_t sn, int64_t sc, bpx_stream_t stream) {
  BPX_CHECK(x.cs == 0, "bpx_head_fwd: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_head_fwd";
  BPX_CHECK(x.ptr && w_d && out_d, "%s: null pointer", fn);
  BPX_CHECK(Cout >= 1 && Cout <= 8, "%s: Cout must be 1..8 (got %d)", fn, Cout);
  BPX_CHECK(x.C == 16 || x.C == 32, "%s: Cin must be 16 or 32 (got %d)", fn, x.C);
  int64_t total = (int64_t)N * vps;
  hipStream_t s = (hipStream_t)stream;
#define HL2(T, CIN, CO) head_fwd_kernel<T, CIN, CO><<<grid_for(total), 256, 0, s>>>((const T*)x.ptr, x.ld, w_d, b_d, head_act, out_d, sn, sc, vps, N)
#define HL(T, CIN)                                                                                                      \
  do {                                                                                                                  \
    switch (Cout) {                                                                                                     \
      case 1: HL2(T, CIN, 1); break; case 2: HL2(T, CIN, 2); break; case 3: HL2(T, CIN, 3); break; case 4: HL2(T, CIN, 4); break; \
      case 5: HL2(T, CIN, 5); break; case 6: HL2(T, CIN, 6); break; case 7: HL2(T, CIN, 7); break; default: HL2(T, CIN, 8); break; \
    }                                                                                                                   \
  } while (0)
  if (dtype == BPX_BF16) { if (x.C == 16) HL(uint16_t, 16); else HL(uint16_t, 32); }
  else if (dtype == BPX_F16) { if (x.C == 16) HL(f16_t, 16); else HL(f16_t, 32); }
  else if (dtype == BPX_F32) { if (x.C == 16) HL(float, 16); else HL(float, 32); }
  else BPX_FAIL("%s: dtype must be BF16, F16 or F32", fn);
#undef HL2
#undef HL
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

// scratch of the per-workgroup partials (the kernels launch at most 1024 workgroup columns; Cout 5..8: one row per column, its Cin / 16 slices
// write disjoint parts of it)
extern "C" int64_t bpx_head_bwd_workspace(int Cin, int Cout) { return (int64_t)1024 * ((int64_t)Cout * Cin + Cout) * 4; }
extern "C" int64_t bpx_conv3d_c1_wgrad_workspace(int Cout) { return (int64_t)1024 * 28 * Cout * 4; }
extern "C" int64_t bpx_conv1x1_c1_wgrad_workspace(int Cout) { return (int64_t)1024 * Cout * 4; }

extern "C" int bpx_head_bwd(int dtype, int64_t vps, int N, bpx_tensor x, const float* w_d, int Cout, const float* dout_d, int64_t sn,
                            int64_t sc, bpx_tensor dx, float* dw_d, float* db_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  BPX_CHECK(x.cs == 0 && dx.cs == 0, "bpx_head_bwd: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_head_bwd";
  BPX_CHECK(x.ptr && w_d && dout_d && dx.ptr && dw_d, "%s: null pointer", fn);
  BPX_CHECK(Cout >= 1 && Cout <= 8, "%s: Cout must be 1..8 (got %d)", fn, Cout);
  BPX_CHECK(x.C == 16 || x.C == 32, "%s: Cin must be 16 or 32 (got %d)", fn, x.C);
  BPX_CHECK(ws_d && ws_bytes >= bpx_head_bwd_workspace(x.C, Cout), "%s: workspace too small (%lld bytes)", fn, (long long)ws_bytes);
  int64_t total = (int64_t)N * vps;
  int blocks = (int)std::min<int64_t>(cdiv64(total, 256), 1024);
  if (Cout > 4 && x.C > 16) blocks = (blocks + 7) & ~7;   // the sliced kernel pairs columns 8 workgroups apart (<= 1024 still)
  hipStream_t s = (hipStream_t)stream;
  float* pw = reinterpret_cast<float*>(ws_d);
  float* pb = db_d ? pw + (size_t)blocks * Cout * x.C : nullptr;
#define HL2(T, CIN, CO, TX) head_bwd_kernel<T, CIN, CO, TX><<<blocks, 256, 0, s>>>((const TX*)x.ptr, x.ld, w_d, Cout, dout_d, sn, sc, (T*)dx.ptr, dx.ld, pw, pb, vps, N)
#define HS2(T, CO, TX) head_bwd_slice_kernel<T, CO, TX><<<blocks * (x.C / 16), 256, 0, s>>>((const TX*)x.ptr, x.ld, w_d, x.C, dout_d, sn, sc, (T*)dx.ptr, dx.ld, pw, pb, vps, N)
#define HL(T, CIN, TX)                                                                                                        \
  do {                                                                                                                        \
    switch (Cout) {                                                                                                           \
      case 1: HL2(T, CIN, 1, TX); break; case 2: HL2(T, CIN, 2, TX); break; case 3: HL2(T, CIN, 3, TX); break; case 4: HL2(T, CIN, 4, TX); break; \
      case 5: HS2(T, 5, TX); break; case 6: HS2(T, 6, TX); break; case 7: HS2(T, 7, TX); break; default: HS2(T, 8, TX); break;              \
    }                                                                                                                         \
  } while (0)
  if (dtype == BPX_BF16) { if (x.C == 16) HL(uint16_t, 16, uint16_t); else HL(uint16_t, 32, uint16_t); }
  else if (dtype == BPX_MIX16) { if (x.C == 16) HL(uint16_t, 16, f16_t); else HL(uint16_t, 32, f16_t); }   // x fp16, dx bf16
  else if (dtype == BPX_F32) { if (x.C == 16) HL(float, 16, float); else HL(float, 32, float); }
  else BPX_FAIL("%s: dtype must be BF16, F32 or MIX16", fn);
#undef HL2
#undef HS2
#undef HL
  BPX_LAUNCH_CHECK(fn);
  // dw[co][ci] flat = one "tap", one "input channel", Cout*Cin outputs; bias rows of Cout values
  return bpxred::reduce_partials(fn, pw, dw_d, blocks, 1, 1, Cout * x.C, 0, 1, 0, pb, db_d, Cout, false, s);
}

static int g_c1_persist = 2048;   // persistent workgroups of the first-layer forward (bpx_debug_set_c1_persist; 0 = one workgroup per tile, as until round 3)
static int g_c1_nobuf = 0;        // bit 30 of the hook's argument: the pointer-addressed instance (tests / A-B of the buffer-addressed one)
extern "C" int bpx_debug_set_c1_persist(int wgs) { g_c1_nobuf = (wgs >> 30) & 1; g_c1_persist = wgs & 0x3FFFFFFF; return 0; }
// the first layer's launch plan: tiles per sample are C1FwdTile / C1MfmaTile / C1ScalarTile::tiles(D, H, W); the buffer-addressed instance when every
// operand's byte span lies within 32-bit offsets of its base (A/B and tests: bpx_debug_set_c1_persist bit 30 clears it)
static bool c1_buffer_addressed(int64_t span0, int64_t span1, int64_t span2 = 0) {
  return !g_c1_nobuf && span0 < 0xFFFFFF00ll && span1 < 0xFFFFFF00ll && span2 < 0xFFFFFF00ll;
}
extern "C" int bpx_conv3d_c1_stats_tiles(int D, int H, int W) { return C1FwdTile::tiles(D, H, W); }

extern "C" int bpx_conv3d_c1_fwd(int dtype, int N, int D, int H, int W, const float* img_d, const float* w_d, const float* bias_d,
                                 bpx_tensor y, float* stats_part_d, bpx_stream_t stream) {
  BPX_CHECK(y.cs == 0, "bpx_conv3d_c1_fwd: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_conv3d_c1_fwd";
  BPX_CHECK(img_d && w_d && y.ptr, "%s: null pointer", fn);
  BPX_CHECK(y.C % 16 == 0, "%s: Cout must be a multiple of 16", fn);
  int tiles = bpx_conv3d_c1_stats_tiles(D, H, W);
  int tY = cdiv(H, C1FwdTile::TY), tX = cdiv(W, C1FwdTile::TX);
  const int total = tiles * N;
  dim3 grid((unsigned)std::min(total, g_c1_persist > 0 ? g_c1_persist : total), (unsigned)(y.C / 16));   // persistent: 8 workgroups per CU
  hipStream_t s = (hipStream_t)stream;
  BPX_CHECK(dtype == BPX_BF16 || dtype == BPX_F16 || dtype == BPX_F32, "%s: dtype must be BF16, F16 or F32", fn);
  const int64_t vox = (int64_t)N * D * H * W;
  const int64_t ib = vox * 4, yb = vox * y.ld * (int64_t)dtype_size(dtype);
  const bool buf = c1_buffer_addressed(ib, yb);
#define C1F(T_, B_) conv_c1_fwd_kernel<T_, B_><<<grid, 256, 0, s>>>(img_d, w_d, bias_d, (T_*)y.ptr, y.ld, y.C, D, H, W, tY, tX, tiles, stats_part_d, total, (uint32_t)ib, (uint32_t)yb)
  if (dtype == BPX_BF16) { if (buf) C1F(uint16_t, true); else C1F(uint16_t, false); }
  else if (dtype == BPX_F16) { if (buf) C1F(f16_t, true); else C1F(f16_t, false); }
  else { if (buf) C1F(float, true); else C1F(float, false); }
#undef C1F
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

static int c1_wgrad_impl(const char* fn, int dtype, int N, int D, int H, int W, const float* img_d, bpx_tensor dy, bpx_tensor t,
                         const bpx_nbwd_coef* coef_d, float* dw_d, float* db_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  BPX_CHECK(dy.cs == 0, "%s: chunk-planar tensors (cs != 0) are not accepted here", fn);
  BPX_CHECK(img_d && dy.ptr && dw_d, "%s: null pointer", fn);
  BPX_CHECK(dy.C % 16 == 0, "%s: Cout must be a multiple of 16", fn);
  BPX_CHECK(ws_d && ws_bytes >= bpx_conv3d_c1_wgrad_workspace(dy.C), "%s: workspace too small (%lld bytes)", fn, (long long)ws_bytes);
  const bool nb = coef_d != nullptr, mix = dtype == BPX_MIX16;
  if (mix) dtype = BPX_BF16;
  int totalTiles = N * C1ScalarTile::tiles(D, H, W);
  dim3 grid((unsigned)std::min(totalTiles, 1024), (unsigned)(dy.C / 16));
  hipStream_t s = (hipStream_t)stream;
  int groups = (int)grid.x;
  float* pw = reinterpret_cast<float*>(ws_d);
  const bool mfma_ok = dtype == BPX_BF16 && W > 8 && ((uintptr_t)dy.ptr & 15) == 0 && (dy.ld & 7) == 0;
  if (nb)
    BPX_CHECK(mfma_ok && t.ptr && t.cs == 0 && t.C == dy.C && ((uintptr_t)t.ptr & 15) == 0 && (t.ld & 7) == 0 && ((uintptr_t)coef_d & 15) == 0,
              "%s: needs bf16 gradients (BF16 / MIX16), W > 8 and 16-byte aligned dense g / t (bpx_conv3d_c1_wgrad_nb_supported)", fn);
  if (mfma_ok) {
    const int tiles = N * C1MfmaTile::tiles(D, H, W);
    // 768 workgroups (3 per CU), each looping over its share of the tiles
    dim3 gm((unsigned)std::min(std::min(tiles, 768), g_c1_persist > 0 ? g_c1_persist : tiles), (unsigned)(dy.C / 16));   // (tests cap the workgroups through bpx_debug_set_c1_persist)
    groups = (int)gm.x;
    float* pb = db_d ? pw + (size_t)groups * 27 * dy.C : nullptr;
    const int64_t vox = (int64_t)N * D * H * W;
    const int64_t ib = vox * 4, gb = vox * dy.ld * 2, tb = nb ? vox * t.ld * 2 : 16;
    const bool buf = c1_buffer_addressed(ib, gb, tb);
#define C1W(TT_, NB_, B_, tp_, tld_, cf_) conv_c1_wgrad_mfma_kernel<TT_, NB_, B_><<<gm, 256, 0, s>>>(img_d, (const uint16_t*)dy.ptr, dy.ld, D, H, W, N, tiles, pw, pb, tp_, tld_, cf_, (uint32_t)ib, (uint32_t)gb, (uint32_t)tb)
    if (nb && mix) { if (buf) C1W(f16_t, true, true, (const f16_t*)t.ptr, t.ld, coef_d); else C1W(f16_t, true, false, (const f16_t*)t.ptr, t.ld, coef_d); }
    else if (nb) { if (buf) C1W(uint16_t, true, true, (const uint16_t*)t.ptr, t.ld, coef_d); else C1W(uint16_t, true, false, (const uint16_t*)t.ptr, t.ld, coef_d); }
    else { if (buf) C1W(uint16_t, false, true, (const uint16_t*)nullptr, 0, (const bpx_nbwd_coef*)nullptr); else C1W(uint16_t, false, false, (const uint16_t*)nullptr, 0, (const bpx_nbwd_coef*)nullptr); }
#undef C1W
  } else {
    float* pb = db_d ? pw + (size_t)groups * 27 * dy.C : nullptr;
    if (dtype == BPX_BF16) conv_c1_wgrad_kernel<uint16_t><<<grid, 256, 0, s>>>(img_d, (const uint16_t*)dy.ptr, dy.ld, D, H, W, N, totalTiles, pw, pb);
    else if (dtype == BPX_F32) conv_c1_wgrad_kernel<float><<<grid, 256, 0, s>>>(img_d, (const float*)dy.ptr, dy.ld, D, H, W, N, totalTiles, pw, pb);
    else BPX_FAIL("%s: dtype must be BF16 or F32", fn);
  }
  BPX_LAUNCH_CHECK(fn);
  // partials [groups][27][1][Cout] -> dw (Cout,1,3,3,3): index = co*27 + tap
  return bpxred::reduce_partials(fn, pw, dw_d, groups, 27, 1, dy.C, 0, 27, 1, pw + (size_t)groups * 27 * dy.C, db_d, 0, true, s);
}

extern "C" int bpx_conv3d_c1_wgrad(int dtype, int N, int D, int H, int W, const float* img_d, bpx_tensor dy, float* dw_d, float* db_d,
                                   void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  BPX_CHECK(dtype == BPX_BF16 || dtype == BPX_F32, "bpx_conv3d_c1_wgrad: dtype must be BF16 or F32");
  return c1_wgrad_impl("bpx_conv3d_c1_wgrad", dtype, N, D, H, W, img_d, dy, bpx_tensor{nullptr, 0, 0}, nullptr, dw_d, db_d, ws_d, ws_bytes, stream);
}

// The same with dy = a * g + b * t + c0 formed inside the kernel (the InstanceNorm backward of the first layer's output: bpx_norm_bwd_apply folded
// into its only consumer - the first layer has no input gradient).  dtype BF16 (g, t bf16) or MIX16 (t fp16); W > 8.
extern "C" int bpx_conv3d_c1_wgrad_nb_supported(int dtype, int W) { return (dtype == BPX_BF16 || dtype == BPX_MIX16) && W > 8 ? 1 : 0; }
extern "C" int bpx_conv3d_c1_wgrad_nb(int dtype, int N, int D, int H, int W, const float* img_d, bpx_tensor g, bpx_tensor t, const bpx_nbwd_coef* coef_d,
                                      float* dw_d, float* db_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream) {
  const char* fn = "bpx_conv3d_c1_wgrad_nb";
  BPX_CHECK(dtype == BPX_BF16 || dtype == BPX_MIX16, "%s: dtype must be BF16 or MIX16", fn);
  BPX_CHECK(coef_d != nullptr, "%s: coefficients are null", fn);
  return c1_wgrad_impl(fn, dtype, N, D, H, W, img_d, g, t, coef_d, dw_d, db_d, ws_d, ws_bytes, stream);
}

extern "C" int bpx_conv1x1_c1_wgrad(int dtype, int64_t voxels_total, const float* img_d, bpx_tensor dy, float* dw_d, void* ws_d, int64_t ws_bytes,
                                    bpx_stream_t stream) {
  BPX_CHECK(dy.cs == 0, "bpx_conv1x1_c1_wgrad: chunk-planar tensors (cs != 0) are not accepted here");
  const char* fn = "bpx_conv1x1_c1_wgrad";
  BPX_CHECK(img_d && dy.ptr && dw_d, "%s: null pointer", fn);
  BPX_CHECK(dy.C % 16 == 0, "%s: Cout must be a multiple of 16", fn);
  BPX_CHECK(ws_d && ws_bytes >= bpx_conv1x1_c1_wgrad_workspace(dy.C), "%s: workspace too small (%lld bytes)", fn, (long long)ws_bytes);
  dim3 grid((unsigned)std::min<int64_t>(cdiv64(voxels_total, 256), 1024), (unsigned)(dy.C / 16));
  hipStream_t s = (hipStream_t)stream;
  float* pw = reinterpret_cast<float*>(ws_d);
  if (dtype == BPX_BF16) rank1_wgrad_kernel<uint16_t><<<grid, 256, 0, s>>>(img_d, (const uint16_t*)dy.ptr, dy.ld, voxels_total, pw);
  else if (dtype == BPX_F32) rank1_wgrad_kernel<float><<<grid, 256, 0, s>>>(img_d, (const float*)dy.ptr, dy.ld, voxels_total, pw);
  else BPX_FAIL("%s: dtype must be BF16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return bpxred::reduce_partials(fn, pw, dw_d, (int)grid.x, 1, 1, dy.C, 0, 1, 0, nullptr, nullptr, 0, true, s);
}

extern "C" int bpx_upsample_c1_fwd(int dtype, int N, int D, int H, int W, int fz, int fy, int fx, const float* img_d, const float* w_d, const float* bias_d,
                                   void* out16_d, bpx_stream_t stream) {
  const char* fn = "bpx_upsample_c1_fwd";
  BPX_CHECK(img_d && w_d && bias_d && out16_d, "%s: null pointer", fn);
  BPX_CHECK(fz >= 1 && fy >= 1 && fx >= 1 && fz * fy * fx <= 512, "%s: bad factors (%d,%d,%d)", fn, fz, fy, fx);
  const int64_t total = (int64_t)N * D * fz * H * fy * W * fx;
  if (total == 0) return 0;
  if (dtype == BPX_BF16) upsample_c1_fwd_kernel<uint16_t><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(img_d, w_d, bias_d, (uint16_t*)out16_d, D, H, W, fz, fy, fx, total);
  else if (dtype == BPX_F16) upsample_c1_fwd_kernel<f16_t><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(img_d, w_d, bias_d, (f16_t*)out16_d, D, H, W, fz, fy, fx, total);
  else if (dtype == BPX_F32) upsample_c1_fwd_kernel<float><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(img_d, w_d, bias_d, (float*)out16_d, D, H, W, fz, fy, fx, total);
  else BPX_FAIL("%s: dtype must be BF16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_upsample_c1_blocks(int64_t voxels_in) { return (int)std::min<int64_t>(std::max<int64_t>(1, cdiv64(voxels_in, 2048)), 256); }

extern "C" int bpx_upsample_c1_bwd(int dtype, int N, int D, int H, int W, int fz, int fy, int fx, const float* img_d, const void* dx16_d, float* partials_d,
                                   bpx_stream_t stream) {
  const char* fn = "bpx_upsample_c1_bwd";
  BPX_CHECK(img_d && dx16_d && partials_d, "%s: null pointer", fn);
  BPX_CHECK(fz >= 1 && fy >= 1 && fx >= 1 && fz * fy * fx <= 512, "%s: bad factors (%d,%d,%d)", fn, fz, fy, fx);
  const int64_t total_in = (int64_t)N * D * H * W;
  if (total_in == 0) return 0;
  dim3 grid((unsigned)bpx_upsample_c1_blocks(total_in), (unsigned)(fz * fy * fx));
  if (dtype == BPX_BF16) upsample_c1_bwd_kernel<uint16_t><<<grid, 256, 0, (hipStream_t)stream>>>(img_d, (const uint16_t*)dx16_d, D, H, W, fz, fy, fx, total_in, partials_d);
  else if (dtype == BPX_F32) upsample_c1_bwd_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>(img_d, (const float*)dx16_d, D, H, W, fz, fy, fx, total_in, partials_d);
  else BPX_FAIL("%s: dtype must be BF16 or F32", fn);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
