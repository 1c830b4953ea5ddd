/*
 * biapy_amd.h - C-ABI of libbiapy_amd.so: the MI355X (gfx950) kernels behind BiaPy's 3D patch
 * U-Net hot path.  Plain pointers and sizes only; every pointer named *_d is a DEVICE pointer,
 * the caller owns all memory, nothing is retained across calls, all launches go to `stream`
 * (a hipStream_t; NULL = the default stream).  Every entry returns 0 on success, non-zero on
 * error with bpx_last_error() (thread-local) describing it.
 *
 * The reference (BiaPyX/BiaPy v3.7.0) is 100 % Python on PyTorch/NumPy, so there is no native FFI
 * to bind to; each entry cites the reference operator/function it replaces (paths relative to the
 * reference root).  INTEGRATION.md shows the ctypes stubs a BiaPy maintainer would add.
 *
 * Tensor layout: activations are NDHWC ("(Z,Y,X,C) patch layout"), i.e. [N][D][H][W][ld] with the
 * channel stride `ld` >= C so that a tensor can be a channel slice of a wider buffer (this is how
 * torch.cat([up, skip], 1) - biapy/models/blocks.py:1653 - is eliminated).
 */
#ifndef BIAPY_AMD_H
#define BIAPY_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* bpx_stream_t; /* hipStream_t */

enum bpx_dtype { BPX_F32 = 0, BPX_BF16 = 1, BPX_F16 = 2, BPX_U8 = 3,
                 /* BPX_MIX16: the mixed 16-bit TRAINING mode, accepted by the backward entry points only.  Activation tensors (the forward
                  * pass's raw outputs: the `t` / `x` operands below) are fp16 - written by the BPX_F16 forward kernels, whose logits
                  * agree with the fp32 reference to Dice delta < 1e-4 - while every GRADIENT tensor (dy, g, dx, addend) and the MFMA
                  * operands of the backward kernels are bf16 (fp32 exponent range: no loss scaling).  Each backward entry says which of
                  * its operands are activations. */
                 BPX_MIX16 = 4,
                 /* BPX_U16: unsigned 16-bit integers - the image of bpx_patch_gather only (a resident volume as the microscope stored it) */
                 BPX_U16 = 5,
                 /* BPX_I32: signed 32-bit integers - the label volume of bpx_edt (what bpx_label_u8 writes) and the image of bpx_watershed only */
                 BPX_I32 = 6 };
/* Block activations (biapy/models/blocks.py:1973-1998, get_activation): codes 0-3 since round 1; round 4 adds leaky_relu (slope 0.01, nn.LeakyReLU's
 * default), gelu (nn.GELU(): the exact erf form), tanh, sigmoid and softplus (beta 1, threshold 20).  "softmax" as a block activation needs a
 * reduction over channels and is not a per-element prologue: not offered.  ELU (the reference default) has compile-time instances of every
 * kernel; the other codes take the run-time-switch instances. */
enum bpx_act { BPX_ACT_NONE = 0, BPX_ACT_ELU = 1, BPX_ACT_RELU = 2, BPX_ACT_SILU = 3, BPX_ACT_LEAKY_RELU = 4, BPX_ACT_GELU = 5, BPX_ACT_TANH = 6,
               BPX_ACT_SIGMOID = 7, BPX_ACT_SOFTPLUS = 8, BPX_ACT_LAST = 8 };
enum bpx_pad_mode { BPX_PAD_REFLECT = 0, BPX_PAD_ZEROS = 1 };

int bpx_version(void);
const char* bpx_last_error(void);
/* MFMA / LDS-transpose lane-layout self test (prints nothing; writes 64*16 floats). Used by tests. */
int bpx_selftest_layouts(float* out_d /* 1024 floats */, bpx_stream_t stream);
/* Test / A-B hook of the weight-gradient kernels (default 1).  bit 0: ds_read_b64_tr_b16 operands (0 = scalar LDS gathers);
 * bits 1-2 choose the bf16 3x3x3 schedule: 2 = never a shift-dy kernel, 4 = always; bits 3-5: input-channel chunks per
 * workgroup of the windowed shift-dy kernel (1, 2, 3 forced; 4 = the plain shift-dy kernel); bit 6: transposed-conv wgrad
 * with the former 2048-workgroup target; bit 7 + bits 8..: k = 1 launches target (value)% of 1024 workgroups; without bit 7,
 * bits 8..: windowed kernel workgroups in percent of the co-resident capacity. */
int bpx_debug_set_wgrad_tr(int use_tr);
int bpx_debug_set_conv_stamps(void* stamps_d); /* profiling hook: [workgroup][16] int64 cycle stamps of the plain conv kernel, NULL = off */
int bpx_debug_set_conv_ws(int on);     /* test / A-B hook of the bf16 3x3x3 conv schedule: 0 = automatic, 4 = always the double-buffered kernel, 5 = always the lean persistent one */
int bpx_debug_set_conv_occ(int wg_per_cu); /* test / A-B hook: persistent workgroups per CU of the lean bf16 conv kernel (0 = built-in table) */
int bpx_debug_set_conv_zm(int mode);       /* test / A-B hook of the z-marching forward kernel of the 16-output-channel layers (conv3d_zmarch.hip; same bits as the lean kernel): -1 = environment BPX_CONV_ZM (default 1), 0 = off, 1 = where a run has several z-steps, 2 = wherever the shape admits it; + 4 = without the role-split form (conv3_zs_kernel) of the one-chunk layers; bits 8.. (tests) = cap on the number of workgroups */
int bpx_debug_conv_zm_launches(void);      /* tests: how many launches took the z-marching kernel so far */
int bpx_debug_conv_zm_occupancy(int nch);  /* tests: resident workgroups per CU of the z-marching kernel (1 or 3 input chunks; 0 = its role-split form of 512 threads) as the runtime computes it; -1 = query failed */
int bpx_debug_set_c1_persist(int wgs); /* test / A-B hook: persistent workgroups of bpx_conv3d_c1_fwd (default 2048; 0 = one workgroup per tile); + 2^30 = the pointer-addressed instance instead of the buffer-addressed one (same bits) */
int bpx_debug_set_convt_k1(int on);  /* test / A-B hook of the transposed-conv forward with one K step into a chunk-planar buffer: -1 = environment BPX_CONVT_K1 (default 1), 1 = the branch-free buffer-addressed kernel where it applies (W % 16 == 0, operands within 32-bit offsets), 0 = the general kernel; same bits */
int bpx_debug_set_pw_stream(int on); /* test / A-B hook: 1 (default) = the streaming kernel for bpx_conv1x1_fwd_split with the IN-backward affine at the large levels, 0 = the tile kernel */
int bpx_debug_set_wgrad_k1(int on); /* test / A-B hook of the streaming weight-gradient kernels at the large levels: 1 (default) = both on, 0 = the tile kernels, 3 = streaming k = 1 (raw-input shortcut) only, 5 = streaming transposed-conv only, 7 = both and the 32 -> 32 transposed-conv instance too (measured slower than its tile kernel) */
int bpx_debug_set_wgrad_cap(int percent); /* test / A-B hook: size cap of a conv layer's weight-gradient partial slabs in percent of the default (~26 / 64 MB) */
int bpx_debug_set_tile_order(int bits); /* test / A-B hook: bit 0 = XCD-contiguous y-strip tile walk of the windowed shift-dy wgrad kernel (default 1; 0 = tile = group + k * groups as until round 3) */
int bpx_debug_set_tiling_scalar(int on); /* test / A-B hook: 1 = crop / merge through the element-per-thread kernels instead of the 16-byte row kernels */

/* ------------------------------------------------------------------------------------------------
 * Tiling.  Patch placement along one axis, exactly the reference's integer rule
 * (biapy/data/data_3D_manipulation.py:541-547, :596-598 / :789-795, :826-835):
 *   start(i) = i*step - ((i*step + patch < limit) ? 0 : last)
 * ---------------------------------------------------------------------------------------------- */
typedef struct bpx_axis_grid {
  int32_t n, step, last, patch, limit;
} bpx_axis_grid;

/* crop_3D_data_with_overlap's copy loop + np.pad (data_3D_manipulation.py:505-515, :591-623) as an
 * on-device gather: out[c] = padded(vol)[z0:z0+Pz, y0:y0+Py, x0:x0+Px] for the patches
 * c in [c_begin, c_begin+c_count) of the z-major patch order.  elem_size = bytes per element
 * (1, 2 or 4); data is moved bit-exactly.  grid[] is the CROP grid (padded coordinates). */
int bpx_crop3d_gather(const void* vol_d, int elem_size, int Z, int Y, int X, int C,
                      int pad_z, int pad_y, int pad_x, int pad_mode,
                      const bpx_axis_grid* grid_zyx /* host, 3 entries */,
                      int64_t c_begin, int64_t c_count, void* out_d, bpx_stream_t stream);

/* merge_3D_data_with_overlap (data_3D_manipulation.py:754-856) as a deterministic gather: every
 * output voxel sums fl32(patch*w) over the patches covering it in the reference's patch order
 * (z-major), w = fl32(fl32(wz*wy)*wx), then divides by fl32(sum(w)+1e-18f) and casts to out_dtype
 * (truncating for u8, as NumPy's astype).  grid[] is the MERGE grid (original coordinates,
 * padding-stripped patch).  Patches are [n][Pz][Py][Px][C] including the padding that is skipped.
 *
 * Sharding (one Z-slab of the volume per GPU): only output slices z in [z_lo, z_hi) are produced,
 * from the patches whose z-row index is in [zrow_lo, zrow_hi) - `patches_d` holds just those rows.
 * acc_d / wacc_d (float, [z_hi-z_lo][Y][X][C] / [..][1], may be NULL) seed the sums with a
 * neighbour's partial sums; with write_partial != 0 the un-normalised sums are written back to
 * acc_d / wacc_d instead of the normalised volume (used for the slab-boundary exchange). */
int bpx_merge3d_blend(const void* patches_d, int dtype, int Pz, int Py, int Px, int C,
                      int pad_z, int pad_y, int pad_x,
                      const bpx_axis_grid* grid_zyx /* host, 3 entries */,
                      const float* wz_d, const float* wy_d, const float* wx_d,
                      int Z, int Y, int X, int z_lo, int z_hi, int zrow_lo, int zrow_hi,
                      float* acc_d, float* wacc_d, int write_partial,
                      void* out_d, int out_dtype, bpx_stream_t stream);

/* By-chunks tiler (chunked_test_pair_data_generator.py:440-565; base_workflow.py:2603-2610).
 * gather: out[b,z,y,x,c] = vol[tz[z], ty[y], tx[x], c] with the three int32 source-index tables of patch b stored back to
 * back in tables_d[b*(Pz+Py+Px) ...] (they encode the clipped read region + np.pad "reflect"); data moves bit-exactly.
 * scatter: the prediction of patch b without its padding goes to its place in the output volume; regions_d[b*9 ...] =
 * {first kept voxel of the patch z,y,x ; destination z,y,x ; extent z,y,x}.  Regions of different patches are disjoint. */
int bpx_gather3d_tables(const void* vol_d, int elem_size, int Z, int Y, int X, int C, const int* tables_d, int n, int Pz, int Py, int Px,
                        void* out_d, bpx_stream_t stream);
/* Inverse of bpx_gather3d_tables: vol[tz[z], ty[y], tx[x], c] = in[b,z,y,x,c] for the non-negative table entries (negative entries
 * of either call mean "outside the volume": the gather returns 0 there, the scatter skips them).  Together they are the
 * space-to-batch / batch-to-space pair that turns a dilated 3x3x3 convolution (ASPP, heads.py:77-104) into ordinary ones. */
int bpx_scatter3d_tables(const void* in_d, int elem_size, const int* tables_d, int n, int Pz, int Py, int Px, void* vol_d, int Z, int Y,
                         int X, int C, bpx_stream_t stream);
int bpx_scatter3d_regions(const float* pred_d, int n, int Pz, int Py, int Px, int C, const int* regions_d, float* out_d, int Z, int Y,
                          int X, bpx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Network kernels.  T = BPX_BF16 (bf16 storage, fp32 accumulate, v_mfma_f32_16x16x32_bf16) or
 * BPX_F32 (fp32 storage, exact-fp32 v_mfma_f32_16x16x4_f32; the parity/debug mode).
 * ---------------------------------------------------------------------------------------------- */

/* Per-(n,c) normalisation record produced by bpx_norm_finalize and consumed by conv prologues. */
typedef struct bpx_norm_rec {
  float mean, rstd, scale, shift; /* y = act(scale*x + shift), scale = gamma*rstd, shift = beta - mean*scale */
} bpx_norm_rec;

typedef struct bpx_tensor {
  void* ptr;   /* device; element (n,z,y,x,c) at ((((n*D+z)*H+y)*W+x)*ld + c) */
  int32_t ld;  /* channel stride in elements */
  int32_t C;   /* channels used */
  int64_t cs;  /* 0: the C channels of a voxel are contiguous (above).  != 0: CHUNK-PLANAR - the 16-channel chunk c/16 of every voxel
                * lives in its own plane, element (voxel v, channel c) at v*ld + (c/16)*cs + c%16 (cs in elements, a multiple of 8;
                * ptr 16-byte aligned at channel 0 of a chunk).  The engine keeps the torch.cat buffers of the decoder this way (planes
                * written by different producers are whole cache lines).  Accepted only where an entry point says so. */
} bpx_tensor;

/* Weight packing: PyTorch fp32 weights -> MFMA operand order (DESIGN.md "packed weights").
 *   mode 0 BPX_PK_K3     Conv3d (Cout,Cin,3,3,3)       -> [Cin/16][q<QPAD][Cout][KPL]      (bpx_conv3d_fwd)
 *   mode 1 BPX_PK_K3_T   same weight, dgrad operator   -> [Cout/16][q<QPAD][Cin][KPL], taps mirrored (bpx_conv3d_dgrad)
 *   mode 2 BPX_PK_K1     Conv3d (Cout,Cin,1,1,1)       -> [Cin/16][4][Cout][KPL]           (fused shortcut of bpx_conv3d_fwd)
 *   mode 3 BPX_PK_DENSE  Conv3d k=1                    -> [ceil4(Cin/KPL)][Cout][KPL]      (bpx_conv1x1_fwd)
 *   mode 4 BPX_PK_DENSE_T same weight, dgrad operator  -> [ceil4(Cout/KPL)][Cin][KPL]      (bpx_conv1x1_fwd as dgrad)
 *   mode 5 BPX_PK_CT     ConvTranspose3d (Cin,Cout,2,2,2) -> [ceil4(Cin/KPL)][8*Cout][KPL] (bpx_convT3d_k2s2_fwd)
 *   mode 6 BPX_PK_CT_T   same weight, dgrad operator   -> [8*Cout/KPL][Cin][KPL]           (bpx_convT3d_k2s2_dgrad)
 *   mode 7 / 8 BPX_PK_CT4 / _T   the same for the anisotropic kernel (1,2,2) (Z_DOWN = 1): 4 sub-positions instead of 8
 * KPL = 8 (bf16) / 4 (f32) elements per 16-byte lane operand; QPAD = 56 (bf16) / 108 (f32).
 * dtype BPX_MIX16: the forward operators (modes 0, 2, 3, 5, 7) are packed as fp16, the transposed / backward ones (1, 4, 6, 8) as bf16. */
enum bpx_pack_mode { BPX_PK_K3 = 0, BPX_PK_K3_T = 1, BPX_PK_K1 = 2, BPX_PK_DENSE = 3, BPX_PK_DENSE_T = 4, BPX_PK_CT = 5, BPX_PK_CT_T = 6,
                     BPX_PK_CT4 = 7, BPX_PK_CT4_T = 8 };
int64_t bpx_packed_weight_elems(int mode, int Cin, int Cout, int dtype);
int bpx_pack_weight(int mode, const float* w_d, int Cin, int Cout, int dtype, void* packed_d, bpx_stream_t stream);
/* The same for up to 64 weights in ONE launch (a training step re-packs ~60 small tensors after every optimizer step;
 * one launch instead of 60).  `jobs` is a HOST array; it is copied into the kernel arguments, nothing is retained. */
typedef struct bpx_pack_job {
  const float* w_d;   /* fp32 weights, PyTorch layout, device */
  void* packed_d;     /* destination, device, bpx_packed_weight_elems(mode, Cin, Cout, dtype) elements */
  int32_t mode, Cin, Cout, reserved;
} bpx_pack_job;
int bpx_pack_weights_batched(int dtype, int count, const bpx_pack_job* jobs, bpx_stream_t stream);

/* torch.optim.Adam / AdamW step (capturable form: `step` is a device float per tensor, lr may be a device scalar) over `count` fp32 tensors in
 * ceil(count / 64) + 1 launches of 4096-element blocks; the arithmetic, its order and its TYPES (double hyper-parameters, double x float products rounded to float at the assignment) are those of torch's fused kernel (train_engine.py:173-177
 * `optimizer.step()` of the reference loop).  `tensors` is a HOST array copied into the kernel arguments.  lr_d (device) overrides lr when not
 * NULL; decoupled = 1: AdamW (p -= lr * wd * p), 0: Adam (g += wd * p).  amsgrad / maximize are not supported (the caller keeps torch's step). */
typedef struct bpx_adam_tensor {
  float* p; const float* g; float* m; float* v; /* parameter, gradient, exp_avg, exp_avg_sq: `numel` contiguous floats each, device */
  float* step;                                  /* device scalar, incremented by one */
  int64_t numel;
} bpx_adam_tensor;
int bpx_adam_step(int count, const bpx_adam_tensor* tensors, const float* lr_d, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int decoupled, bpx_stream_t stream);

/* Global L2 norm of the gradients (`.g`, `.numel` of every entry; the other fields are not read) of `count` tensors - every param group of an
 * optimizer in ONE list - and the coefficient of torch's clip_grad_norm_ (norm_type 2, error_if_nonfinite False), both left on the device:
 *   out_d[0] = (float)sqrt(sum g^2)      out_d[1] = min(1.0f, (float)(max_norm / ((double)out_d[0] + 1e-6)))
 * The squares are summed in fp64 in a fixed order (one double per 4096-element chunk, then one block over the chunks; no atomics): two calls agree
 * bit for bit.  A NaN gradient gives NaN for both.  workspace_d: bpx_grad_norm_workspace bytes (8-byte aligned, device), -1 for a bad list. */
int64_t bpx_grad_norm_workspace(int count, const bpx_adam_tensor* tensors);
int bpx_grad_norm(int count, const bpx_adam_tensor* tensors, double max_norm, void* workspace_d, int64_t workspace_bytes, float* out_d,
                  bpx_stream_t stream);
/* bpx_adam_step with hyper-parameters that change between the replays of a captured step: beta1_d (device DOUBLE, as torch keeps the betas;
 * NULL = the host argument) and gscale_d (device float, NULL = none): every gradient element is first multiplied by it - one fp32 product - and the
 * product is stored back to `.g`, which is what clip_grad_norm_ leaves in p.grad.  Same arithmetic, order and types otherwise. */
int bpx_adam_step_dev(int count, const bpx_adam_tensor* tensors, const float* lr_d, double lr, const double* beta1_d, double beta1, double beta2,
                      double eps, double weight_decay, int decoupled, const float* gscale_d, bpx_stream_t stream);
/* torch.optim.SGD's step (`_multi_tensor_sgd`) in ONE pass over parameter, gradient and momentum buffer (`.m`; `.v` / `.step` are not read), in its
 * fp32 arithmetic and order, every scalar rounded to float once as a foreach op rounds its alpha:
 *   d = g + wd * p (weight_decay != 0);  b = b * mom, b = b + (1 - dampening) * d;  u = nesterov ? d + mom * b : b;  p = p + (-lr) * u.
 * Without momentum (momentum_d NULL and momentum 0) `.m` may be NULL, no buffer is touched and u = d.  lr_d (float), momentum_d (DOUBLE, rounded
 * to float by the kernel) and gscale_d (float: g = g * gscale first, one fp32 product, stored back to `.g`) are device scalars that override their
 * host arguments when not NULL; a NULL gscale_d leaves `.g` unwritten.  The first step of a fresh torch optimizer (buffer = gradient) is the
 * caller's: with dampening 0 a zeroed buffer gives the same.  No atomics: two runs agree bit for bit. */
int bpx_sgd_step(int count, const bpx_adam_tensor* tensors, const float* lr_d, double lr, const double* momentum_d, double momentum,
                 double dampening, double weight_decay, int nesterov, const float* gscale_d, bpx_stream_t stream);

/* Conv3d k=3 "same" + bias (biapy/models/blocks.py:154-157), implicit GEMM on MFMA with an
 * LDS-staged input halo.  Fusions:
 *   prologue : x <- act(scale*x+shift) with in_norm_d[n*Cin+c]  (the InstanceNorm+ELU that
 *              precedes this conv, blocks.py:1308-1314 / :158-161); NULL = raw input.
 *   shortcut : + Conv3d k=1 of a second raw tensor `sc` (blocks.py:1372, :1458) when sc.ptr != NULL;
 *              sc.C == 1 is handled as a rank-1 update.  w_sc packed with k=1.
 *   epilogue : per-(n,c) sum / sum-of-squares partials of the fp32 result into stats_part_d
 *              ([n][tiles][2][Cout] floats) for the next InstanceNorm (NULL = skip).
 * x.C must be 1 or a multiple of 16; Cout a multiple of 16. */
int bpx_conv3d_fwd(int dtype, int N, int D, int H, int W, bpx_tensor x, const bpx_norm_rec* in_norm_d, int act,
                   const void* w_packed_d, const float* bias_d, bpx_tensor sc, const void* w_sc_packed_d,
                   const float* bias_sc_d, bpx_tensor y, float* stats_part_d, bpx_stream_t stream);
int bpx_conv3d_stats_tiles(int dtype, int N, int D, int H, int W, int Cout); /* partial-sum slots per sample the call above writes */
/* The same convolution with the MaxPool3d (pool_sz,2,2) that follows an encoder block (resunet.py:256-257) fused into the
 * epilogue: `pooled` (extents D/pool_sz, H/2, W/2) and its statistics partials ([n][tiles][2][Cout], same tile count) are
 * written from registers, so the output slice is not read again.  Only where bpx_conv3d_fwd_pool_supported() returns 1
 * (the lean 16-bit kernel of the >= 32^3 levels); elsewhere use bpx_conv3d_fwd + bpx_maxpool3d_fwd. */
int bpx_conv3d_fwd_pool(int dtype, int N, int D, int H, int W, bpx_tensor x, const bpx_norm_rec* in_norm_d, int act,
                        const void* w_packed_d, const float* bias_d, bpx_tensor sc, const void* w_sc_packed_d,
                        const float* bias_sc_d, bpx_tensor y, float* stats_part_d, int pool_sz, bpx_tensor pooled,
                        float* pool_stats_part_d, bpx_stream_t stream);
int bpx_conv3d_fwd_pool_supported(int dtype, int N, int D, int H, int W, int x_ld, int y_ld, int Cout);
/* Conv3d k = 3 from x.C to 16 * s^3 channels followed by a 3-D pixel shuffle by s, in one pass (the up-scaling stage of the RCAN
 * super-resolution network, cfg 5).  biapy/models/rcan.py:317-319 builds `conv(filters, filters * scale**2) + nn.PixelShuffle(scale)`, which is
 * 2-D only (on 5-D tensors it raises); the 3-D form is DEFINED here as its natural extension:
 *   out[n, c, s z + a, s y + b, s x + e] = conv[n, c s^3 + (a s + b) s + e, z, y, x]        (a, b, e in [0, s))
 * The kernel takes the conv's output channels in the order [sub-position (a, b, e)][c] (w_packed_d = BPX_PK_K3 of the re-ordered weight, bias_d
 * re-ordered alike) and stores block (a, b, e) of voxel (z, y, x) to voxel (s z + a, s y + b, s x + e) of y = (N, sD, sH, sW, 16): the
 * 16 s^3-channel tensor never exists in memory.  dtype BF16 / F16; volumes the lean kernel takes (D*H*W >= 32^3, W > 8); s = 2, 3, 4. */
int bpx_conv3d_fwd_shuffle(int dtype, int N, int D, int H, int W, bpx_tensor x, const bpx_norm_rec* in_norm_d, int act, const void* w_packed_d,
                           const float* bias_d, int s, bpx_tensor y, bpx_stream_t stream);

/* dgrad of the conv above w.r.t. its (normalised+activated) input, fused with the backward of that
 * activation:  g = convT(dy, W) * act'(scale*t+shift),  t = the conv's raw input tensor.
 * Writes g and the per-(n,c) partials of sum(g) and sum(g*xhat) (xhat = (t-mean)*rstd) that both
 * InstanceNorm's input gradient and its dgamma/dbeta need.  t_norm_d == NULL: plain dgrad. */
int bpx_conv3d_dgrad(int dtype, int N, int D, int H, int W, bpx_tensor dy, const void* w_packed_T_d,
                     bpx_tensor t, const bpx_norm_rec* t_norm_d, int act, bpx_tensor g,
                     float* red_part_d, bpx_stream_t stream);

/* wgrad: dW[co][ci][tap] = sum_v act(norm(x))[v+tap][ci] * dy[v][co] written (overwritten) in the PyTorch
 * layout (Cout,Cin,k,k,k); db[co] += sum_v dy[v][co] (db_d must be zeroed by the caller, may be NULL).
 * k = 3 or 1.  Deterministic: per-workgroup partial sums of dW AND of the bias column sums go to the caller-provided workspace
 * and are summed in a fixed order (no atomics; db is updated by the reduction, i.e. at the flush in the deferred mode).
 * ws_bytes >= bpx_conv3d_wgrad_workspace(...).  x may be chunk-planar (bpx_tensor.cs). */
int64_t bpx_conv3d_wgrad_workspace(int N, int D, int H, int W, int Cin, int Cout, int k);
int bpx_conv3d_wgrad(int dtype, int N, int D, int H, int W, bpx_tensor x, const bpx_norm_rec* in_norm_d, int act,
                     bpx_tensor dy, int k, float* dw_d, float* db_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream);
/* The same with a second bias-gradient destination: db2_d[co] += the same column sums (needs db_d).  A residual block adds the biases of its
 * second convolution and of its 1x1x1 shortcut to the same tensor (biapy/models/blocks.py:1456-1459), so the two bias gradients are equal:
 * the reduction writes both instead of the caller copying one onto the other after the flush. */
int bpx_conv3d_wgrad_db2(int dtype, int N, int D, int H, int W, bpx_tensor x, const bpx_norm_rec* in_norm_d, int act,
                         bpx_tensor dy, int k, float* dw_d, float* db_d, float* db2_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream);

/* Backward of ONE 3x3x3 convolution in one pass over its operands: bpx_conv3d_dgrad (g, its sum(g) / sum(g*xhat) partials) AND
 * bpx_conv3d_wgrad_db2 (dW, db, db2) of the same (dy, t) pair - the two Conv3d gradients autograd computes for blocks.py:154-157 under
 * train_engine.py:173.  Both kernels stage the same haloed dy tile and the same raw input tile t (t is the conv's raw input; the conv saw
 * act(scale*t+shift)); fused, dy and t are read once (16 -> 16 channels: 3 tensor passes instead of 5; dy 16 -> t 48: 7 instead of 11).
 * Results are those of the two separate calls: g bit for bit that of bpx_conv3d_dgrad; its partials, dW and db fixed-order sums
 * of per-workgroup partials (bit-reproducible; the grouping of the voxels differs from bpx_conv3d_wgrad's, so the fp32 sums differ in the last bits).
 * Supported (bpx_conv3d_bwd_fused_supported): dtype BF16 or MIX16 (t fp16); (dy.C, t.C) = (16, 16 | 48) - the level-0 layers of cfg 2 - or
 * (32, 16 | 32) - level-1 layers (32 -> 96 measured no faster than the two kernels and is not taken); W > 8, >= 32^3 voxels per sample, t_norm_d given.  red_part_d: [N][bpx_conv3d_bwd_fused_stats_tiles(N, D, H, W, t.C, dy.C)][2][t.C] floats - one row per (sample, persistent workgroup column), every row written (zeros where a workgroup had no tile of the sample); (dy 16, t 48): one row per 4x4x16 tile.  ws_bytes >= bpx_conv3d_bwd_fused_workspace(...); inside a
 * bpx_wgrad_defer_begin / _flush window the reduction is queued like bpx_conv3d_wgrad's (own workspace per call).  t may be chunk-planar. */
int bpx_conv3d_bwd_fused_supported(int dtype, int N, int D, int H, int W, int Ct, int Cdy);
int bpx_conv3d_bwd_fused_stats_tiles(int N, int D, int H, int W, int Ct, int Cdy);
int64_t bpx_conv3d_bwd_fused_workspace(int N, int D, int H, int W, int Ct, int Cdy);
int bpx_conv3d_bwd_fused(int dtype, int N, int D, int H, int W, bpx_tensor dy, const void* w_packed_T_d, bpx_tensor t,
                         const bpx_norm_rec* t_norm_d, int act, bpx_tensor g, float* red_part_d, float* dw_d, float* db_d, float* db2_d,
                         void* ws_d, int64_t ws_bytes, bpx_stream_t stream);
int bpx_debug_set_bwd_fused(int bits); /* test / A-B hook: bit 0 clear = bpx_conv3d_bwd_fused_supported answers 0 everywhere (the engine then takes the two separate kernels); bit 1 set = only the dy.C == 16 instances */
int bpx_debug_set_bwd_rs(int mask);     /* test / A-B hook: bit 0 = the (dy 16, t 48) shape of bpx_conv3d_bwd_fused runs the role-split kernel (8 waves per CU: 4 dgrad + 4 wgrad, two tiles in flight), bit 1 = the (dy 16, t 16) shape does; call before _stats_tiles / _workspace */
int bpx_debug_set_conv_kg(int on);      /* test / A-B hook: the two-K-group form of the small-tile conv kernel (<= 16^3 layers with >= 4 input chunks): 1 on, 0 off, -1 = environment BPX_CONV_KG (default on) */
int bpx_debug_set_conv_wn(int wn);      /* test / A-B hook: how many of a K group's four waves lie across the output channels in the small-tile 16-bit conv kernel (<= 16^3 layers): -1 = environment BPX_CONV_WN (default 0), 0 = the launcher's choice, 1 / 2 / 4 = that value where an instance exists (else 1).  Results are the same bits for every value */
int bpx_conv3d_wn_supported(int dtype, int D, int H, int W, int Cout, int wn);   /* 1 when bpx_conv3d_fwd / _dgrad launches of this shape (below 32^3 voxels per sample) have an instance with `wn` waves across the output channels */

/* Deferred reduction of the weight-gradient partials.  Between bpx_wgrad_defer_begin() and bpx_wgrad_defer_flush() (same
 * host thread) bpx_conv3d_wgrad and the bf16 bpx_convT3d_k2s2_wgrad write only their partial slabs and queue the reduction;
 * the flush finishes up to 32 of them per launch (dw_d is written then).  Every deferred call needs its OWN workspace, alive
 * and untouched until the flush has run on the stream; dw_d AND db_d are complete only after the flush (a caller that copies a
 * bias gradient elsewhere does so after it).  bpx_conv3d_c1_wgrad and bpx_conv1x1_c1_wgrad queue their reductions the same way. */
int bpx_wgrad_defer_begin(void);
int bpx_wgrad_defer_flush(bpx_stream_t stream);

/* Per-(n,c) coefficients of InstanceNorm's input gradient, dx = a*g + b*t + c0 (see bpx_norm_bwd_finalize). */
typedef struct bpx_nbwd_coef { float a, b, c0, pad; } bpx_nbwd_coef;

/* Conv3d k=1 as a GEMM over voxels: y = x*W + bias [+ a*g + b*t + c0] [+ addend].  Used for the dgrad of
 * the residual shortcut (blocks.py:1372) fused with the InstanceNorm-backward affine of the main path, and
 * for stand-alone 1x1x1 convolutions.  `voxels` = voxels per sample; g/t/coef_d and addend may be null. */
int bpx_conv1x1_fwd(int dtype, int N, int64_t voxels, bpx_tensor x, const void* w_packed_d, const float* bias_d,
                    bpx_tensor g, bpx_tensor t, const bpx_nbwd_coef* coef_d, bpx_tensor addend, bpx_tensor y,
                    bpx_stream_t stream);
/* Same, with the output columns split over two dense tensors: [0, y_lo.C) -> y_lo, the rest -> y_hi (both counts multiples
 * of 4).  The gradient of torch.cat([up, bridge], 1) (blocks.py:1653) leaves as its two parts, each consumed by a kernel
 * that would otherwise read a channel slice with a 3/2x or 3x line over-fetch. */
int bpx_conv1x1_fwd_split(int dtype, int N, int64_t voxels, bpx_tensor x, const void* w_packed_d, const float* bias_d,
                          bpx_tensor g, bpx_tensor t, const bpx_nbwd_coef* coef_d, bpx_tensor addend, bpx_tensor y_lo,
                          bpx_tensor y_hi, bpx_stream_t stream);
/* The same with the residual block's SHORTCUT WEIGHT GRADIENT riding along (round 6): dw_d[co][ci] (Cout = x.C, Cin = t.C, 1, 1, 1) = sum_v t[v][ci] * x[v][co]
 * - the k = 1 bpx_conv3d_wgrad of the raw block input t against dOut = x (biapy/models/blocks.py ResConvBlock `shortcut(x)`), whose two operands this
 * kernel streams anyway.  Only where the streaming kernel applies: _workspace answers the bytes of ws_d, or 0 = call bpx_conv1x1_fwd_split and
 * bpx_conv3d_wgrad instead (BPX_PWS_WG=0 forces that).  Between bpx_wgrad_defer_begin and _flush dw_d is complete at the flush and ws_d must stay untouched until then. */
int64_t bpx_conv1x1_fwd_split_wgrad_workspace(int dtype, int N, int64_t voxels, int K);
/* The same answer for the operands themselves: 0 also where the 32-bit spans, pitches or alignment keep them off the streaming kernel, so that a
 * non-zero answer is always a call bpx_conv1x1_fwd_split_wgrad accepts.  g and coef_d may be null when they are allocated after the query (dense,
 * 16-byte aligned); their shape is read then. */
int64_t bpx_conv1x1_fwd_split_wgrad_query(int dtype, int N, int64_t voxels, bpx_tensor x, bpx_tensor g, bpx_tensor t, const void* coef_d,
                                          bpx_tensor y_lo, bpx_tensor y_hi);
int bpx_conv1x1_fwd_split_wgrad(int dtype, int N, int64_t voxels, bpx_tensor x, const void* w_packed_d, bpx_tensor g, bpx_tensor t,
                                const bpx_nbwd_coef* coef_d, bpx_tensor y_lo, bpx_tensor y_hi, float* dw_d, void* ws_d, int64_t ws_bytes,
                                bpx_stream_t stream);

/* ConvTranspose3d k = s = (sz,2,2), sz = z_down of the level = 1 or 2 (blocks.py:1607):
 * y[n,sz*z+a,2y+b,2x+c,:] = x[n,z,y,x,:]*W[:,:,a,b,c] + b.
 * (D,H,W) are the INPUT extents; y has extents (sz*D,2H,2W) and may be a channel slice of the
 * concat buffer.  stats_part_d: ([n][tiles][2][Cout]) partials for the following norm.
 * Weights packed with BPX_PK_CT / _T (sz = 2) or BPX_PK_CT4 / _T (sz = 1). */
int bpx_convT3d_k2s2_fwd(int dtype, int N, int D, int H, int W, int sz, bpx_tensor x, const void* w_packed_d,
                         const float* bias_d, bpx_tensor y, float* stats_part_d, bpx_stream_t stream);
int bpx_convT3d_stats_tiles(int D, int H, int W, int sz);
int bpx_convT3d_k2s2_dgrad(int dtype, int N, int D, int H, int W, int sz, bpx_tensor dy, const void* w_packed_T_d,
                           bpx_tensor dx, bpx_stream_t stream);
int64_t bpx_convT3d_k2s2_wgrad_workspace(int N, int D, int H, int W, int sz, int Cin, int Cout);
int bpx_convT3d_k2s2_wgrad(int dtype, int N, int D, int H, int W, int sz, bpx_tensor x, bpx_tensor dy,
                           float* dw_d /* (Cin,Cout,sz,2,2), overwritten */, float* db_d /* accumulated */,
                           void* ws_d, int64_t ws_bytes, bpx_stream_t stream);
/* Both gradients of the layer in one call: dx as bpx_convT3d_k2s2_dgrad (w_packed_T_d: BPX_PK_CT_T / BPX_PK_CT4_T, bf16 for BPX_MIX16), dw_d and
 * db_d as bpx_convT3d_k2s2_wgrad (same workspace, same deferral), bit for bit.  For 32 -> 32 channels, sz = 2, >= 262144 input voxels, bf16 /
 * MIX16, dense dx the weight-gradient kernel forms dx from the dy tiles it has staged and dy is read once; every other shape runs the two
 * kernels one after the other. */
int bpx_convT3d_k2s2_bwd(int dtype, int N, int D, int H, int W, int sz, bpx_tensor x, bpx_tensor dy, const void* w_packed_T_d,
                         bpx_tensor dx, float* dw_d, float* db_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream);
int bpx_debug_set_convt_bwd(int on); /* test / A-B hook: 1 (default) = bpx_convT3d_k2s2_bwd uses its one-pass instance where it applies, 0 = always the two kernels; same bits */
int bpx_debug_convt_bwd_launches(void); /* test hook: how many calls of bpx_convT3d_k2s2_bwd have taken the one-pass instance so far (host-side count, graph replays not included) */

/* InstanceNorm3d(affine, eps) == GroupNorm with G = C (blocks.py:2122-2125).  Reduces the partials
 * written by a producer kernel to bpx_norm_rec[n*out_ld + out_off + c]; groups < C gives GroupNorm(groups).
 * out_ld/out_off let two producers (up-conv and skip) fill one record array for the concatenated tensor.
 * The partial array is CONSUMED: with >= 1024 tiles a first pass compacts it in place (no scratch buffer). */
int bpx_norm_finalize(float* stats_part_d, int N, int tiles, int C, int64_t count_per_channel,
                      const float* gamma_d, const float* beta_d, float eps, int groups,
                      bpx_norm_rec* out_d, int out_ld, int out_off, bpx_stream_t stream);
/* GroupNorm(groups) with ANY channels-per-group, also over the concatenation of two producers' outputs (torch.cat([up, skip], 1) in front of
 * the decoder's first norm, blocks.py:1653: with 8 groups over 48 / 96 / 192 / 384 channels one group straddles the boundary).
 *   bpx_norm_channel_sums     : a producer's partials [N][tiles][2][C] (CONSUMED like in bpx_norm_finalize) -> per-channel totals
 *                               sums_d[(n*out_ld + out_off + c)*2 + {0, 1}] (double): each producer fills its columns of one (N, out_ld, 2) array
 *   bpx_groupnorm_finalize    : the records of all C channels from those totals (group statistics = fixed-order sums of the group's channels)
 *   bpx_groupnorm_bwd_finalize: bpx_norm_bwd_finalize for the same layout: sums_d = per-channel totals of {S1 = sum g, S2 = sum g*xhat};
 *                               like it, it ADDS to what dgamma_d / dbeta_d hold (either may be null)
 * The reference's "gn" (nn.GroupNorm(out_channels, num_groups=8), blocks.py:2122-2125) raises a TypeError; what it means - GroupNorm(8, C) -
 * is what these implement, checked against torch.nn.GroupNorm. */
int bpx_norm_channel_sums(float* stats_part_d, int N, int tiles, int C, double* sums_d, int out_ld, int out_off, bpx_stream_t stream);
int bpx_groupnorm_finalize(const double* sums_d, int N, int C, int64_t count_per_channel, const float* gamma_d, const float* beta_d, float eps,
                           int groups, bpx_norm_rec* out_d, bpx_stream_t stream);
int bpx_groupnorm_bwd_finalize(const double* sums_d, int N, int C, int64_t count_per_channel, const bpx_norm_rec* rec_d, const float* gamma_d,
                               float* dgamma_d, float* dbeta_d, int groups, bpx_nbwd_coef* coef_d, bpx_stream_t stream);
/* Stand-alone statistics of a tensor (used for tensors no conv kernel produced, and in tests). */
int bpx_tensor_stats(int dtype, int N, int64_t voxels, bpx_tensor x, float* stats_part_d, bpx_stream_t stream);
int bpx_tensor_stats_tiles(int64_t voxels);

/* Backward of InstanceNorm (groups == C) / GroupNorm(groups) (blocks.py:2117-2125) given the per-channel partials from
 * bpx_conv3d_dgrad / bpx_norm_act_bwd (S1 = sum g, S2 = sum g*xhat with the group's statistics in rec_d):
 *   coef[n*C+c] = {a, b, c0} with dx = a*g + b*t + c0 ;  dgamma[c] += sum_n S2 ; dbeta[c] += sum_n S1
 * (sums over the samples in a fixed order by one thread per channel: deterministic).  dgamma_d / dbeta_d are ADDED to, never overwritten: the
 * caller zeroes them (or lets several layers that share a parameter accumulate); either may be null.  Channels per group: 1, 2, 4, 8, 16, 32, 64;
 * count_per_channel = voxels per sample. */
int bpx_norm_bwd_finalize(float* red_part_d /* consumed, see bpx_norm_finalize */, int N, int tiles, int C, int64_t count_per_channel,
                          const bpx_norm_rec* rec_d, const float* gamma_d, float* dgamma_d, float* dbeta_d, int groups,
                          bpx_nbwd_coef* coef_d, bpx_stream_t stream);
/* The same inside a bpx_wgrad_defer_begin / _flush window, one block per (channel block, sample): coef_d is complete when the call's kernel is; the
 * sums over the samples that dgamma / dbeta need are queued with the window's weight-gradient reductions and arrive at the flush (sample order,
 * fixed: bit-reproducible).  The first partial row of every sample is overwritten with that sample's totals: red_part_d must stay untouched
 * until the flush.  The flush ADDS the sums to what dgamma_d / dbeta_d hold then, as the plain entry does at once.  dbeta_d == dgamma_d + C (the
 * engines' gradient slab) is one reduction over 2 C columns, any other pair two; either may be null.  Outside a window (or for N = 1) it is
 * bpx_norm_bwd_finalize. */
int bpx_norm_bwd_finalize_deferred(float* red_part_d /* consumed, see bpx_norm_finalize */, int N, int tiles, int C, int64_t count_per_channel,
                          const bpx_norm_rec* rec_d, const float* gamma_d, float* dgamma_d, float* dbeta_d, int groups,
                          bpx_nbwd_coef* coef_d, bpx_stream_t stream);
/* BatchNorm3d(C, eps, momentum, affine, track_running_stats) (blocks.py:2113-2127 'bn'), in the record / coefficient layouts above, so that the
 * conv prologues, epilogues and the InstanceNorm backward kernels consume it unchanged.  Statistics are over all N samples x voxels, summed in
 * fp64 in a fixed order (samples in index order, then the tile lanes): two identical calls give identical bits.  No atomics, no host sync.
 *   bpx_batchnorm_finalize    : training-mode forward.  stats_part_d [N][tiles][2][C] as in bpx_norm_finalize (CONSUMED).  mean = S1/n,
 *                               var = S2/n - mean^2 (biased, clamped at 0), n = N * count_per_sample; the same record goes to all N rows
 *                               out_d[n*out_ld + out_off + c].  Non-null running buffers (pointers at the channel offset of this call) are
 *                               updated in place: rm = (1-m) rm + m mean, rv = (1-m) rv + m var n/(n-1); num_batches_tracked_d (int64, may be
 *                               null: pass it to ONE call per layer) += 1.  n must be > 1.
 *   bpx_batchnorm_bwd_finalize: training-mode backward.  red_part_d [N][tiles][2][C] partials of {S1 = sum g, S2 = sum g*xhat} (CONSUMED) as
 *                               the dgrad / fused-backward / norm-act-dropout kernels write them; rec_d the forward's records (row 0 is read).
 *                               coef[n*C + c] = {a, b, c0} of bpx_norm_bwd_finalize with the batch totals and 1/n over N * count_per_sample, the
 *                               same for every n; dgamma[c] += sum S2, dbeta[c] += sum S1 (dgamma / dbeta may be null).  It needs every sample
 *                               for the coefficients anyway, so dgamma / dbeta are written by the same thread: there is no deferred form.
 *                               running_stats != 0: the backward of an eval-mode forward (records from bpx_batchnorm_eval_records): the
 *                               statistics are constants, so a = gamma*rstd and b = c0 = 0 (dgamma / dbeta as above).
 *   bpx_batchnorm_eval_records: eval mode, every BN layer of a network in ONE launch (count <= 64 jobs, `jobs` is a HOST array copied into the
 *                               kernel arguments): out_d[n*C + c] = {rm, rstd, scale, shift} for n < N with rstd = 1/sqrt(rv + eps),
 *                               scale = gamma * rstd, shift = beta - rm * scale. */
int bpx_batchnorm_finalize(float* stats_part_d, int N, int tiles, int C, int64_t count_per_sample, const float* gamma_d, const float* beta_d,
                           float eps, float momentum, float* running_mean_d, float* running_var_d, int64_t* num_batches_tracked_d,
                           bpx_norm_rec* out_d, int out_ld, int out_off, bpx_stream_t stream);
int bpx_batchnorm_bwd_finalize(float* red_part_d, int N, int tiles, int C, int64_t count_per_sample, const bpx_norm_rec* rec_d,
                               const float* gamma_d, float* dgamma_d, float* dbeta_d, int running_stats, bpx_nbwd_coef* coef_d,
                               bpx_stream_t stream);
typedef struct bpx_bn_eval_job {
  const float* gamma_d;
  const float* beta_d;
  const float* running_mean_d;
  const float* running_var_d;
  bpx_norm_rec* out_d;   /* N x C records */
  int32_t C;
  float eps;
} bpx_bn_eval_job;
int bpx_batchnorm_eval_records(int count, const bpx_bn_eval_job* jobs, int N, bpx_stream_t stream);
/* dx = a*g + b*t + c0 (+ addend): applies the coefficients above elementwise. dx may alias g. */
int bpx_norm_bwd_apply(int dtype, int N, int64_t voxels, bpx_tensor g, bpx_tensor t, const bpx_nbwd_coef* coef_d,
                       bpx_tensor addend, bpx_tensor dx, bpx_stream_t stream);

/* Materialised InstanceNorm + activation and its backward, for consumers without a fused prologue (plain U-Net:
 * biapy/models/blocks.py:154-166 Conv -> Norm -> Act feeding MaxPool / ConvTranspose / the head, unet.py:382-394).
 *   fwd: y = act(scale*x + shift), rec_d = [N][C] records of bpx_norm_finalize.
 *   bwd: g = dy * act'(scale*x + shift) (+ addend); red_part_d = [N][bpx_norm_act_tiles()][2][C] partial sums of
 *        S1 = sum g, S2 = sum g*xhat of the product term only, the layout bpx_norm_bwd_finalize reads.  g may alias dy.
 * dtype fwd: BF16, F16, F32; bwd: BF16, F32, or MIX16 (x = the forward pass's fp16 tensor; dy, addend, g bf16 - the mixed training mode). */
int bpx_norm_act_tiles(int dtype, int64_t voxels, int C);
int bpx_norm_act_fwd(int dtype, int N, int64_t voxels, bpx_tensor x, const bpx_norm_rec* rec_d, int act, bpx_tensor y,
                     bpx_stream_t stream);
int bpx_norm_act_bwd(int dtype, int N, int64_t voxels, bpx_tensor dy, bpx_tensor x, const bpx_norm_rec* rec_d, int act,
                     bpx_tensor addend, bpx_tensor g, float* red_part_d, bpx_stream_t stream);

/* Dropout of a residual block (biapy/models/blocks.py:163: `nn.Dropout(p)` after Conv -> Norm -> Act, element-wise) - only for p > 0; p = 0 (BiaPy's
 * default DROPOUT_VALUES) keeps the fused prologue of the block's second convolution.
 *   fwd: y = act(scale*x + shift) * keep / (1 - p)        (the tensor the second convolution then reads WITHOUT a prologue)
 *   bwd: g = dy * keep / (1 - p) * act'(scale*x + shift), red_part_d = [N][bpx_norm_act_dropout_tiles()][2][C] partial sums for bpx_norm_bwd_finalize
 * keep = Philox4x32-10(key = seed, counter = (element / 4, site, *counter_d)) >= p * 2^32 over the linear index of the dense NDHWC tensor: forward and
 * backward regenerate the same mask, nothing is stored; *counter_d is a DEVICE uint64 the caller bumps once per forward pass (a replayed graph
 * draws a new mask each time).  Not the reference's random stream (torch's CPU / CUDA generators cannot be reproduced): parity is held with the
 * mask made explicit - mask_mode 1 reads the keep flags (uint8 per element) from mask_io_d instead of drawing them, 2 also writes the drawn
 * flags there (forward only), 0 ignores it.  dtype fwd: BF16, F16, F32; bwd: BF16, MIX16 (x fp16), F32.  Dense tensors (ld == C). */
int bpx_norm_act_dropout_tiles(int dtype, int64_t voxels, int C);
int bpx_norm_act_dropout_fwd(int dtype, int N, int64_t voxels, bpx_tensor x, const bpx_norm_rec* rec_d, int act, float p, uint64_t seed,
                             const uint64_t* counter_d, int site, uint8_t* mask_io_d, int mask_mode, bpx_tensor y, bpx_stream_t stream);
int bpx_norm_act_dropout_bwd(int dtype, int N, int64_t voxels, bpx_tensor dy, bpx_tensor x, const bpx_norm_rec* rec_d, int act, float p,
                             uint64_t seed, const uint64_t* counter_d, int site, uint8_t* mask_io_d, int mask_mode, bpx_tensor g,
                             float* red_part_d, bpx_stream_t stream);

/* Channel attention of the RCAN trunk (biapy/models/rcan.py: ChannelAttention.forward `x * module(x)`, RCAB_rcan.forward
 * `x + module(x)`): y = [x +] scale[n,c] * h [+ offset[n,c]] with per-(sample, channel) fp32 factors (x.ptr / offset_d may be
 * null; y may alias h), and the reduction its backward needs: part_d[n][bpx_norm_act_tiles()][C] partial sums of a*b over
 * voxels (d scale[n,c] = sum_v dy*h). */
int bpx_channel_affine(int dtype, int N, int64_t voxels, bpx_tensor x, bpx_tensor h, const float* scale_d, const float* offset_d,
                       bpx_tensor y, bpx_stream_t stream);
int bpx_dot_stats(int dtype, int N, int64_t voxels, bpx_tensor a, bpx_tensor b, float* part_d, bpx_stream_t stream);
/* The gate itself, on the pooled (N, C) vector (rcan.py ChannelAttention.module: Conv 1x1 -> SiLU -> Conv 1x1 -> Sigmoid;
 * blocks.py:1119-1191 SqExBlock.excitation: Linear -> ReLU -> Linear -> Sigmoid, no biases):
 *   m[n,c] = sum_t part_d[n][t][0][c] / voxels   (part_d: [N][tiles][2][C] statistics partials of the producing kernel, NOT consumed)
 *   u1 = W1 m + b1 (R values; w1_d [R][C]),  a1 = act(u1),  s = sigmoid(W2 a1 + b2) (w2_d [C][R]);  b1_d / b2_d may be null
 *   saved_d [N][C + 2R] = m, u1, a1 (read by the backward).  C <= 256, R <= 64.
 * Backward: dpart_d [N][tiles][C] partial sums of dy*h (bpx_dot_stats) -> ds[n,c]; dW1 / db1 / dW2 / db2 are ACCUMULATED (+=; db may be
 * null) with the samples summed in index order (deterministic); off_d[n][c] = d mean[n,c] / voxels, the offset of the affine pass
 * that carries the pooled gradient back to every voxel. */
int bpx_gate_mlp_fwd(const float* part_d, int N, int tiles, int C, int64_t voxels, const float* w1_d, const float* b1_d, const float* w2_d,
                     const float* b2_d, int R, int act, float* s_d, float* saved_d, bpx_stream_t stream);
int bpx_gate_mlp_bwd(const float* dpart_d, int N, int tiles, int C, int64_t voxels, const float* s_d, const float* saved_d, const float* w1_d,
                     const float* w2_d, int R, int act, float* dw1_d, float* db1_d, float* dw2_d, float* db2_d, float* off_d,
                     bpx_stream_t stream);

/* MaxPool3d (sz,2,2), sz = z_down of the level = 1 or 2 (resunet.py:256-257) + statistics of the pooled tensor.
 * (D,H,W) = input extents. */
int bpx_maxpool3d_fwd(int dtype, int N, int D, int H, int W, int sz, bpx_tensor x, bpx_tensor y, float* stats_part_d,
                      bpx_stream_t stream);
int bpx_maxpool3d_stats_tiles(int dtype, int D, int H, int W, int sz, int C);
/* dx = addend + scatter(dy to the first maximal element of each window); addend may be dx itself (in place) or null.  D % sz, H % 2 and W % 2 must be
 * 0, as in bpx_maxpool3d_fwd: the call is refused otherwise (a trailing plane / row / column of dx would stay unwritten). */
int bpx_maxpool3d_bwd(int dtype, int N, int D, int H, int W, int sz, bpx_tensor x, bpx_tensor dy, bpx_tensor addend,
                      bpx_tensor dx, bpx_stream_t stream);
/* The same (addend required) with the rank-1 shortcut weight gradient of the first residual block riding along (round 6): dw_d[co] (16, 1, 1, 1, 1) =
 * sum_v img_d[v] * dx[v][co] over the values this call STORES - what bpx_conv1x1_c1_wgrad computes from dx afterwards (blocks.py ResConvBlock `shortcut(x)`
 * on a one-channel image).  16 channels, 16-bit storage; _workspace answers the bytes of ws_d or 0 = call the two entry points (BPX_POOL_R1=0 forces that).
 * Between bpx_wgrad_defer_begin and _flush dw_d is complete at the flush and ws_d must stay untouched until then. */
int64_t bpx_maxpool3d_bwd_r1_workspace(int dtype, int N, int D, int H, int W, int sz, int C);
int bpx_maxpool3d_bwd_r1(int dtype, int N, int D, int H, int W, int sz, bpx_tensor x, bpx_tensor dy, bpx_tensor addend, bpx_tensor dx,
                         const float* img_d, float* dw_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream);

/* Output head: Conv3d k=1 to `Cout` (<= 8) fp32 channels (resunet.py:346-348) with the head
 * activation (base_workflow.py:1403-1457) fused: head_act holds one 4-bit code per output channel, Cout <= 8 codes (channel 0
 * in the low nibble; eight softmax channels = 0x33333333): 0 = linear (logits), 1 = sigmoid, 2 = tanh, 3 = softmax, consecutive
 * softmax channels forming one group (a head may hold several groups, separated by other codes).  Cin is 16 or 32.
 * out is (N,Cout,D,H,W) fp32 contiguous per channel plane with arbitrary strides given in elements. */
int bpx_head_fwd(int dtype, int64_t voxels_per_sample, int N, bpx_tensor x, const float* w_d /* [Cout][Cin] */,
                 const float* b_d, int Cout, int head_act, float* out_d, int64_t out_stride_n, int64_t out_stride_c,
                 bpx_stream_t stream);
/* bwd (Cout <= 8): dx, dW (overwritten) and db (added to).  The parameter gradients are sums of per-workgroup partials held in ws_d
 * (>= bpx_head_bwd_workspace bytes) and combined in a fixed order right after the kernel - no atomics, bit-reproducible from run to run. */
int64_t bpx_head_bwd_workspace(int Cin, int Cout);
int bpx_head_bwd(int dtype, int64_t voxels_per_sample, int N, bpx_tensor x, const float* w_d, int Cout,
                 const float* dout_d, int64_t stride_n, int64_t stride_c, bpx_tensor dx, float* dw_d, float* db_d,
                 void* ws_d, int64_t ws_bytes, bpx_stream_t stream);

/* First layer, Cin = 1 (fp32 image in, blocks.py:154 with in_size = 1): direct convolution. */
int bpx_conv3d_c1_fwd(int dtype, int N, int D, int H, int W, const float* img_d, const float* w_d /* (Cout,1,3,3,3) */,
                      const float* bias_d, bpx_tensor y, float* stats_part_d, bpx_stream_t stream);
int bpx_conv3d_c1_stats_tiles(int D, int H, int W);
/* dW (Cout,1,3,3,3) is overwritten, db is added to; partial sums in ws_d (deterministic).  With bpx_wgrad_defer_begin active the
 * combination runs at the flush, like that of bpx_conv3d_wgrad: ws_d must stay untouched until then. */
int64_t bpx_conv3d_c1_wgrad_workspace(int Cout);
int bpx_conv3d_c1_wgrad(int dtype, int N, int D, int H, int W, const float* img_d, bpx_tensor dy,
                        float* dw_d, float* db_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream);
/* bpx_norm_bwd_apply folded into bpx_conv3d_c1_wgrad: dy = a * g + b * t + c0 (coef_d of bpx_norm_bwd_finalize, t = the first conv's raw output)
 * is formed while the tile is staged and never stored - the first layer has no input gradient, so the weight gradient is dy's only consumer
 * (blocks.py:154-157 under autograd, first ConvBlock of the encoder).  dtype BF16, or MIX16 (t fp16); needs W > 8 and dense 16-byte aligned g / t. */
int bpx_conv3d_c1_wgrad_nb_supported(int dtype, int W);
int bpx_conv3d_c1_wgrad_nb(int dtype, int N, int D, int H, int W, const float* img_d, bpx_tensor g, bpx_tensor t, const bpx_nbwd_coef* coef_d,
                           float* dw_d, float* db_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream);

/* Shortcut of the first block (Conv3d 1 -> Cout, k = 1, blocks.py:1372 with in_size = 1): dW[co] = sum_v img[v]*dy[v][co]
 * (overwritten; partial sums in ws_d as for bpx_conv3d_c1_wgrad, deterministic, deferrable). */
int64_t bpx_conv1x1_c1_wgrad_workspace(int Cout);
int bpx_conv1x1_c1_wgrad(int dtype, int64_t voxels_total, const float* img_d, bpx_tensor dy, float* dw_d, void* ws_d, int64_t ws_bytes,
                         bpx_stream_t stream);

/* Super-resolution "pre" up-sampling of the 1-channel image: ConvTranspose3d(1, 1, kernel = stride = (fz, fy, fx))
 * (biapy/models/resunet.py:206-213, :368-369).  fwd writes channel 0 of a dense 16-channel NDHWC tensor of the storage dtype
 * (extents fz*D, fy*H, fx*W; channels 1..15 = 0) so that the first residual block can run on the 16-channel kernels with its weights
 * zero-padded.  bwd: partials_d[(t * bpx_upsample_c1_blocks(N*D*H*W) + b) * 2 + {0, 1}] = partial sums of img * g and of g for tap
 * t = (a*fy + b)*fx + c, g = channel 0 of the gradient of that tensor; the caller reduces them (dW[t] = sum of the first, dbias = sum
 * over all taps of the second). */
int bpx_upsample_c1_fwd(int dtype, int N, int D, int H, int W, int fz, int fy, int fx, const float* img_d, const float* w_d, const float* bias_d,
                        void* out16_d, bpx_stream_t stream);
int bpx_upsample_c1_blocks(int64_t voxels_in);
int bpx_upsample_c1_bwd(int dtype, int N, int D, int H, int W, int fz, int fy, int fx, const float* img_d, const void* dx16_d, float* partials_d,
                        bpx_stream_t stream);

/* dtype conversion helpers (NDHWC, strided channel slices) */
int bpx_cast(int src_dtype, const void* src_d, int dst_dtype, void* dst_d, int64_t n, bpx_stream_t stream);
/* An fp32 image of C channels (1 <= C <= 16), element (n, v, c) at img_d[n*stride_n + v*stride_v + c*stride_c] (strides in elements, 64-bit), as
 * the dense (N, voxels, 16) tensor of the storage dtype (BPX_F32 / BPX_BF16 / BPX_F16) the first block of a network with a zero-padded input reads:
 * channels C .. 15 are written as zero, the others round as bpx_cast rounds.  Planar (N, C, voxels): stride_v = 1, stride_c = voxels;
 * channels-last (N, voxels, C): stride_v = C, stride_c = 1.  out16_d is 16-byte aligned; N <= 65535. */
int bpx_image_pack16(int dtype, int N, int64_t voxels, int C, const float* img_d, int64_t stride_n, int64_t stride_v, int64_t stride_c,
                     void* out16_d, bpx_stream_t stream);

/* ---- binary segmentation loss (1-channel head) ---------------------------------------------------------------------------
 * Replaces biapy/engine/metrics.py:493-586 (CrossEntropyLoss_wrapper -> BCEWithLogitsLoss), :726-762 (DiceLoss, batch_dice),
 * :764-973 (DiceCELoss, binary case) and the counts of :138-232 (jaccard_index at threshold 0.5) with one streaming pass each
 * way.  bpx_seg_loss_sums writes bpx_seg_loss_blocks(n) rows of {sum bce, sum p*t, sum p, sum t, |P&T|, |P|T|}
 * (p = sigmoid(logit), P = p > 0.5, T = t > 0.5); the caller reduces the rows (deterministic) and forms the loss.
 * bpx_seg_loss_bwd: dlogits = a (p - t) - p (1 - p) (b t - c) with coef_d = {a, b, c} on the device
 * (a = w_ce*g/n, b = 2 w_dice*g/(U+s), c = w_dice*g*(2I+s)/(U+s)^2; biapy_amd/losses.py). fp32 planar logits and targets. */
int bpx_seg_loss_blocks(int64_t n);
int bpx_seg_loss_sums(const float* logits_d, const float* target_d, int64_t n, float* partials_d, bpx_stream_t stream);
int bpx_seg_loss_bwd(const float* logits_d, const float* target_d, int64_t n, const float* coef_d, float* dlogits_d, bpx_stream_t stream);
/* The scalar tail of the same losses on the device (no host-side element-wise launches inside a captured training step):
 *   bpx_seg_loss_finish   : sums_d[6] (double) = the fixed-order column sums of the `blocks` partial rows; loss_d (float) =
 *                           w_ce * S0 / n + w_dice * (1 - (2 S1 + smooth) / (S2 + S3 + smooth))
 *   bpx_seg_loss_bwd_fused: bpx_seg_loss_bwd with a, b, c formed in the kernel from sums_d and the upstream gradient gup_d[0] (device float). */
int bpx_seg_loss_finish(const float* partials_d, int blocks, int64_t n, float w_ce, float w_dice, float smooth, double* sums_d, float* loss_d,
                        bpx_stream_t stream);
int bpx_seg_loss_bwd_fused(const float* logits_d, const float* target_d, int64_t n, const double* sums_d, const float* gup_d, float w_ce, float w_dice,
                           float smooth, float* dlogits_d, bpx_stream_t stream);

/* ---- per-channel losses of a multi-channel head (row X / cfg 4: instance segmentation with B, C, D channels) ------------------------------
 * Replaces biapy/engine/metrics.py:1418-1810 (instance_segmentation_loss; plain channels: no masks, class re-balancing or border
 * weights) composed with the training-time head activation the workflow applies before it (base_workflow.py:1403-1457: ce_* channels
 * stay logits, other channels - 'D': tanh, instance_seg.py:405-409 - are activated).  codes: one 4-bit code per channel (channel 0
 * in the low nibble) = kind | act << 2; kind 0 = BCE with logits, 1 = MSE, 2 = L1; act (of the logit, for MSE / L1) 0 = linear,
 * 1 = tanh, 2 = sigmoid.  Planar fp32 logits / targets [N][C][voxels], C <= 8.
 *   bpx_chan_loss_sums: partials_d[(n*C + c) * bpx_chan_loss_blocks(voxels) + b] = partial sums of the per-element loss terms;
 *                       the caller reduces them (deterministic) and forms  sum_c w_c * S_c / (N * voxels).
 *   bpx_chan_loss_bwd : dlogits = coef_d[c] * d term / d logit  with coef_d[c] = upstream gradient * w_c / (N * voxels) on the device. */
int bpx_chan_loss_blocks(int64_t voxels);
int bpx_chan_loss_sums(const float* logits_d, const float* target_d, int N, int C, int64_t voxels, unsigned codes, float* partials_d,
                       bpx_stream_t stream);
int bpx_chan_loss_bwd(const float* logits_d, const float* target_d, int N, int C, int64_t voxels, unsigned codes, const float* coef_d,
                      float* dlogits_d, bpx_stream_t stream);
/* Multi-class cross entropy of the semantic-segmentation head and the counts of the multi-class IoU (replaces biapy/engine/metrics.py:493-586
 * CrossEntropyLoss_wrapper with num_classes > 2 = torch.nn.CrossEntropyLoss(ignore_index, weight), mean reduction, and the confusion counts behind
 * :138-232 jaccard_index).  logits (N, C, voxels) fp32 planar, 2 <= C <= 8; target (N, 1, voxels) class ids as floats; class_w_d: C floats or NULL;
 * labels equal to ignore_index (or outside [0, C)) are not counted.
 *   bpx_softmax_ce_sums  : partials_d[N * bpx_softmax_ce_blocks(voxels)][bpx_softmax_ce_row()] = {sum w nll, sum w, tp[8], pred[8], tgt[8]} per block
 *   bpx_softmax_ce_finish: sums_d[bpx_softmax_ce_row()] (double, fixed summation order), loss_d = sums[0] / sums[1]
 *   bpx_softmax_ce_bwd   : dlogits = gup_d[0] * w[y] / sums[1] * (softmax - onehot(y)), 0 for uncounted labels. */
int bpx_softmax_ce_blocks(int64_t voxels);
int bpx_softmax_ce_row(void);
int bpx_softmax_ce_sums(const float* logits_d, const float* target_d, int N, int C, int64_t voxels, int ignore_index, const float* class_w_d,
                        float* partials_d, bpx_stream_t stream);
int bpx_softmax_ce_finish(const float* partials_d, int N, int64_t voxels, double* sums_d, float* loss_d, bpx_stream_t stream);
int bpx_softmax_ce_bwd(const float* logits_d, const float* target_d, int N, int C, int64_t voxels, int ignore_index, const float* class_w_d,
                       const double* sums_d, const float* gup_d, float* dlogits_d, bpx_stream_t stream);
/* Dice and Dice + cross-entropy losses of heads with 2..8 channels (biapy_amd/losses.py states the definitions; csrc/losses.hip).  logits (N, C, voxels)
 * fp32 planar.  class_mode != 0: target (N, 1, voxels) class ids as floats, p = softmax over the channels, a voxel counts if its label is not
 * ignore_index and lies in [0, C), class_w_d (C floats or NULL) weighs the cross-entropy term only.  class_mode == 0: target (N, C, voxels),
 * p = sigmoid per channel, the CE term is BCEWithLogits averaged over all elements, class_w_d must be NULL.  Three launches per loss, no atomics,
 * no host read-back; 16-byte loads where voxels % 4 == 0 and the pointers are 16-byte aligned, dword loads otherwise.
 *   bpx_dice_sums  : partials_d[N * bpx_dice_blocks(voxels)][bpx_dice_row()], one row per (sample, block):
 *                    {I[8] = sum p t, P[8] = sum p, T[8] = sum t, sum w nll (class) | sum bce (channel), sum w, labels outside [0, C) other than
 *                    ignore_index, counted voxels}; with_ce == 0 leaves the CE columns 0
 *   bpx_dice_finish: sums_d[bpx_dice_row()] = the batch totals (double, fixed order); with U = P + T per class of the batch (batch_dice != 0) or of
 *                    every sample, and M = C or N C dice terms:  loss_d = w_ce CE + w_dice (1 - sum (2 I + smooth) / (U + smooth) / M), a term whose
 *                    weight is 0 is not formed;  coef_d[8 + 16 G] floats, G = 1 or N groups: coef[0] = w_ce / (sum w | N C voxels) (0 for w_ce == 0),
 *                    group g at coef + 8 + 16 g: a0[8] = w_dice (2 I + s) / (M (U + s)^2), a1[8] = a0 - 2 w_dice / (M (U + s))
 *   bpx_dice_bwd   : class:   dlogits[c] = gup_d[0] (p_c (A_c - sum_k p_k A_k) + coef[0] w[y] (p_c - [c == y])), A_c = a1[c] where c == y, else a0[c];
 *                             0 on uncounted voxels
 *                    channel: dlogits[c] = gup_d[0] (A_c p_c (1 - p_c) + coef[0] (p_c - t_c)), A_c = a0[c] + t_c (a1[c] - a0[c]) */
int bpx_dice_blocks(int64_t voxels);
int bpx_dice_row(void);
int bpx_dice_sums(const float* logits_d, const float* target_d, int N, int C, int64_t voxels, int class_mode, int ignore_index, const float* class_w_d,
                  int with_ce, float* partials_d, bpx_stream_t stream);
int bpx_dice_finish(const float* partials_d, int N, int C, int64_t voxels, int class_mode, int batch_dice, double w_ce, double w_dice, double smooth,
                    double* sums_d, float* coef_d, float* loss_d, bpx_stream_t stream);
int bpx_dice_bwd(const float* logits_d, const float* target_d, int N, int C, int64_t voxels, int class_mode, int batch_dice, int ignore_index,
                 const float* class_w_d, const float* coef_d, const float* gup_d, float* dlogits_d, bpx_stream_t stream);
/*   bpx_chan_loss_finish  : loss_d = sum_c weights_d[c] * (fixed-order double sum of channel c's partials) / (N * voxels)
 *   bpx_chan_loss_bwd_fused: bpx_chan_loss_bwd with coef[c] = gup_d[0] * weights_d[c] / (N * voxels) formed in the kernel. */
int bpx_chan_loss_finish(const float* partials_d, int N, int C, int64_t voxels, const float* weights_d, float* loss_d, bpx_stream_t stream);
int bpx_chan_loss_bwd_fused(const float* logits_d, const float* target_d, int N, int C, int64_t voxels, unsigned codes, const float* weights_d,
                            const float* gup_d, float* dlogits_d, bpx_stream_t stream);

/* ---- attention gate of ResUNet++ (biapy/models/blocks.py:2168-2298, `return out * x2`: a 1-channel map times a C-channel tensor) ----
 * fwd: y[v][c] = a[v] * x[v][c], a = the FIRST channel of tensor `a` (channel stride a.ld);  bwd: dx = dy * a and
 * da16[v][0] = sum_c dy[v][c] * x[v][c], da16[v][1..15] = 0 (a dense 16-channel tensor: the gradient of the zero-padded 16-output
 * 1x1 convolution that produced the gate).  total_voxels = N * voxels per sample. */
int bpx_gate_mul_fwd(int dtype, int64_t total_voxels, bpx_tensor a, bpx_tensor x, bpx_tensor y, bpx_stream_t stream);
int bpx_gate_mul_bwd(int dtype, int64_t total_voxels, bpx_tensor dy, bpx_tensor a, bpx_tensor x, bpx_tensor dx, void* da16_d, bpx_stream_t stream);

/* ---- scans either side of the network ---------------------------------------------------------------
 * Input normalisation (biapy/data/norm.py: percentile_clip :395-473 -> np.percentile, zero_mean_unit_variance_normalization
 * :586-645) and the Otsu binarisation after the merge (biapy/engine/semantic_seg.py:418-431) on volumes that live on the device.
 *   bpx_select_kth_f32 : exact k-th smallest element (0-based), 4-pass radix select, result written to out_d (device float)
 *   bpx_minmax_f32     : per-block {min, max} partials, bpx_scan_blocks(n) rows; a NaN in a block's share makes both of its partials NaN,
 *                        a block without a share writes {+inf, -inf}
 *   bpx_moment_f32     : per-block partial sums of (x - center)^power in double (power 1 or 2), bpx_scan_blocks(n) rows
 *   bpx_histogram_f32  : np.histogram(a, bins=nbins, range=(first, last)) of a float32 array, bit-identical counts;
 *                        edges_d = the float32 edge table NumPy builds (np.linspace(first, last, nbins + 1, dtype=float32));
 *                        counts_d (uint64[nbins]) is ACCUMULATED into (zero it first)
 *   bpx_threshold_u8   : out = x > thr
 *   bpx_clip_affine_f32: out = (clip(x, lo, hi) - sub) / div in float32 operations
 * x_d needs the 4-byte alignment of a float only: 16-byte loads are used where it allows them, and the results do not depend on it. */
int bpx_scan_blocks(int64_t n);
int64_t bpx_select_workspace(void);
int bpx_select_kth_f32(const float* x_d, int64_t n, int64_t k, float* out_d, void* ws_d, bpx_stream_t stream);
int bpx_minmax_f32(const float* x_d, int64_t n, float* partials_d, bpx_stream_t stream);
int bpx_moment_f32(const float* x_d, int64_t n, double center, int power, double* partials_d, bpx_stream_t stream);
int bpx_histogram_f32(const float* x_d, int64_t n, float first_edge, float last_edge, int nbins, const float* edges_d,
                      unsigned long long* counts_d, bpx_stream_t stream);
int bpx_threshold_u8(const float* x_d, int64_t n, float thr, uint8_t* out_d, bpx_stream_t stream);
int bpx_clip_affine_f32(const float* x_d, int64_t n, float lo, float hi, float sub, float div, float* out_d, bpx_stream_t stream);
/* Class head of the sliding-window harness (biapy/engine/base_workflow.py:2135-2141, `separated_class_channel`): the last k channels of a
 * (voxels, C) float32 volume are replaced by ONE channel holding np.argmax over them (first maximum), out_d is (voxels, C - k + 1). */
int bpx_class_argmax(const float* in_d, int64_t voxels, int C, int k, float* out_d, bpx_stream_t stream);

/* ---- test-time augmentation -------------------------------------------------------------------------
 * Signed axis permutations of a (Z,Y,X,C) float32 volume (biapy/data/post_processing/tta.py:64-196, AxisTransform: output
 * axis a comes from input axis perm[a], reversed when sign[a] == -1; 2D images use Z = 1) and the reduction of
 * post_processing.py:1349-1383.  (Z,Y,X) are always the extents of the UN-oriented volume.
 *   bpx_tta_orient     : out = t.apply(in); out has extents (n[perm[0]], n[perm[1]], n[perm[2]])
 *   bpx_tta_accumulate : acc (op)= t.inverse.apply(pred), op: first != 0 -> assign, else mode 0 add / 1 min / 2 max;
 *                        count_if_last > 0 with mode 0 divides the finished sum by that count (np.mean's sum / n). */
int bpx_tta_orient(const float* in_d, int Z, int Y, int X, int C, const int* perm, const int* sign, float* out_d, bpx_stream_t stream);
int bpx_tta_accumulate(const float* pred_d, int Z, int Y, int X, int C, const int* perm, const int* sign, int mode, int first,
                       int count_if_last, float* acc_d, bpx_stream_t stream);

/* ---- training-time augmentation on the device (biapy_amd/augment.py states the semantics; csrc/augment.hip) -------------------
 * Flips, rot90 over (Y, X), contrast, brightness, Gaussian noise and cutout of a float32 (B,Z,Y,X,C) image batch, 1 <= C <= 16, and its
 * (B,Z,Y,X,Ct) float32 / uint8 target, 1 <= Ct <= 8, in one gather pass.  The draws of a call live in one RECORD of 32 four-byte words
 * per sample:
 *   word 0       flags: bit 0 zflip, 1 vflip (Y), 2 hflip (X); bits 3-4 k of rot90; bit 5 contrast, 6 brightness, 7 noise fired;
 *                bits 8-10 number of cutout boxes (0..4)
 *   word 1       a, the contrast factor (float)          word 2   b, the brightness offset (float)
 *   word 3       s, the noise standard deviation (float)  word 4   m, the sample mean (float; written by bpx_aug_mean)
 *   words 5-6    the counter value the call drew with, low and high          word 7   reserved, 0
 *   words 8-31   four boxes z0, y0, x0, dz, dy, dx (int32) in OUTPUT coordinates */
#define BPX_AUG_REC_WORDS 32
#define BPX_AUG_MAX_BOXES 4
#define BPX_AUG_F_ZFLIP 0x1u
#define BPX_AUG_F_VFLIP 0x2u
#define BPX_AUG_F_HFLIP 0x4u
#define BPX_AUG_K_SHIFT 3
#define BPX_AUG_F_CONTRAST 0x20u
#define BPX_AUG_F_BRIGHTNESS 0x40u
#define BPX_AUG_F_NOISE 0x80u
#define BPX_AUG_NBOX_SHIFT 8
#define BPX_AUG_W_FLAGS 0
#define BPX_AUG_W_A 1
#define BPX_AUG_W_B 2
#define BPX_AUG_W_S 3
#define BPX_AUG_W_M 4
#define BPX_AUG_W_CTR 5
#define BPX_AUG_W_BOX 8
/* which transforms a bpx_aug_draw may fire (bpx_aug_cfg.enable) */
#define BPX_AUG_EN_ROT90 0x1u
#define BPX_AUG_EN_ZFLIP 0x2u
#define BPX_AUG_EN_VFLIP 0x4u
#define BPX_AUG_EN_HFLIP 0x8u
#define BPX_AUG_EN_CONTRAST 0x10u
#define BPX_AUG_EN_BRIGHTNESS 0x20u
#define BPX_AUG_EN_NOISE 0x40u
#define BPX_AUG_EN_CUTOUT 0x80u
typedef struct {
  uint64_t seed;          /* Philox key */
  uint64_t thr;           /* floor(da_prob * 2^32): a transform fires when its 32-bit word is below it (compared in 64 bits) */
  uint32_t enable;        /* BPX_AUG_EN_* */
  int32_t box_lo, box_hi; /* number of cutout boxes, 1 <= box_lo <= box_hi <= 4 */
  float c_lo, c_hi;       /* contrast: a = 1 + uniform */
  float b_lo, b_hi;       /* brightness offset */
  float s_lo, s_hi;       /* noise standard deviation */
  float f_lo, f_hi;       /* cutout extent as a fraction of each axis, in (0, 1] */
} bpx_aug_cfg;
/*   bpx_aug_draw  : fills records_d[B][32] (word 4 = 0) from Philox4x32-10(key = seed, counter = (sample, stream, state_d[0] low, high)) and then
 *                   adds 1 to state_d[0], the augmenter's counter; state_d[1] is a ticket the blocks of the launch count themselves on (0 between
 *                   launches).  One launch, nothing is read back: capturable, a replay draws anew.
 *   bpx_aug_mean  : records_d[b][4] = float(fp64 sum of sample b / n), n = elements per sample; ws_d: B * bpx_aug_mean_blocks(n) doubles; fixed
 *                   summation order (two launches, no atomics)
 *   bpx_aug_apply : out = the augmented pair as augment.py defines it; t_dtype BPX_F32 or BPX_U8; out-of-place only.  Y != X: rot90 records with an
 *                   odd k are applied with that bit cleared.  cval / mask_too: the cutout value of the image / whether boxes also zero the target. */
int bpx_aug_draw(const bpx_aug_cfg* cfg, int B, int Z, int Y, int X, uint64_t* state_d, uint32_t* records_d, bpx_stream_t stream);
int bpx_aug_mean_blocks(int64_t n);
int bpx_aug_mean(const float* x_d, int B, int64_t n, double* ws_d, uint32_t* records_d, bpx_stream_t stream);
int bpx_aug_apply(const float* x_d, const void* t_d, int t_dtype, int B, int Z, int Y, int X, int C, int Ct, const uint32_t* records_d, uint64_t seed,
                  float cval, int mask_too, float* x_out_d, void* t_out_d, bpx_stream_t stream);

/* ---- affine warp in the (Y, X) plane: random rotation, zoom, shear and shift (step 0 of biapy_amd/augment.py; csrc/augment.hip) ----------
 * One 2x3 matrix per sample, identical for every z and channel; the image is interpolated bilinearly, the target takes the nearest voxel.
 * The draws of a call live in one WARP RECORD of 16 four-byte words per sample:
 *   word 0       flags: bit 0 rotation, 1 zoom, 2 shear, 3 shift fired; 0 = the sample is copied bit for bit
 *   words 1-6    m00 m01 m02 m10 m11 m12 (float): the source coordinate of output voxel (y, x) is
 *                fy = (m00 dy + m01 dx) + m02, fx = (m10 dy + m11 dx) + m12 with dy = y - (Y-1)/2, dx = x - (X-1)/2, each clamped to +-2^30
 *   word 7       0
 *   words 8-12   the drawn parameters (float): theta in degrees, zoom z, shear phi in degrees, ty, tx as fractions of Y and X; a transform
 *                that did not fire holds its neutral value 0, 1, 0, 0, 0
 *   words 13-15  0
 * The matrix of the drawn parameters, in fp32:  A = (1/z) [[cos t, sin t], [-sin t, cos t]] [[1, 0], [tan p, 1]],  m00 m01 m10 m11 = A,
 * m02 = (Y-1)/2 - ty Y, m12 = (X-1)/2 - tx X. */
#define BPX_WARP_REC_WORDS 16
#define BPX_WARP_F_ROT 0x1u
#define BPX_WARP_F_ZOOM 0x2u
#define BPX_WARP_F_SHEAR 0x4u
#define BPX_WARP_F_SHIFT 0x8u
#define BPX_WARP_W_FLAGS 0
#define BPX_WARP_W_M 1
#define BPX_WARP_W_P 8
/* border rule of a tap outside the plane (bpx_warp_apply's mode), per integer tap index and axis of n voxels */
#define BPX_WARP_CONSTANT 0 /* cval for the image, 0 for the target */
#define BPX_WARP_REFLECT 1  /* numpy.pad's "reflect": period 2n - 2, true modulo; n == 1: index 0 */
#define BPX_WARP_EDGE 2     /* the index is clamped */
typedef struct {
  uint64_t seed;              /* Philox key: the augmenter's */
  uint64_t thr;               /* floor(da_prob * 2^32), as in bpx_aug_cfg */
  uint32_t enable;            /* BPX_WARP_F_*: which transforms may fire */
  uint32_t reserved;
  float rot_lo, rot_hi;       /* degrees */
  float zoom_lo, zoom_hi;     /* > 0 */
  float shear_lo, shear_hi;   /* degrees */
  float shift_lo, shift_hi;   /* fraction of the axis, ty and tx drawn independently */
} bpx_warp_cfg;
/*   bpx_warp_draw  : fills warp_d[B][16] from Philox4x32-10(key = seed, counter = (sample, stream, c low, c high)), c = the counter value in
 *                    words 5-6 of the sample's augmentation record records_d[b] (what bpx_aug_draw drew with: no second ticket).  Streams: 16
 *                    fires (r0 rotation, r1 zoom, r2 shear, r3 shift), 17 uniforms theta, z, phi, 18 uniforms ty, tx.  One launch, nothing
 *                    is read back: capturable.
 *   bpx_warp_apply : out = the warped pair, ONE out-of-place pass over image (1..16 channels) and target (1..8, BPX_F32 or BPX_U8).  Whatever
 *                    the matrix words hold, the clamp and the border rule keep every load inside the sample's plane. */
int bpx_warp_draw(const bpx_warp_cfg* cfg, int B, int Y, int X, const uint32_t* records_d, uint32_t* warp_d, bpx_stream_t stream);
int bpx_warp_apply(const float* x_d, const void* t_d, int t_dtype, int B, int Z, int Y, int X, int C, int Ct, const uint32_t* warp_d, int mode,
                   float cval, float* x_out_d, void* t_out_d, bpx_stream_t stream);

/* ---- elastic deformation in the (Y, X) plane (step 0b of biapy_amd/augment.py, after the affine warp; csrc/elastic.hip, csrc/augment_core.h) ----
 * One displacement field per sample, identical for every z and channel; the image is interpolated bilinearly, the target takes the nearest
 * voxel.  A sample's draw is an ELASTIC RECORD of 8 four-byte words:
 *   word 0       flags: bit 0 fired; 0 = the sample is copied bit for bit
 *   word 1       alpha (float), the scale of the displacement in voxels; 0 when the sample did not fire
 *   words 2-3    the counter value the call drew with, low and high
 *   words 4-7    0
 * THE FIELD of a call is float32 (B, 2, Y, X), plane 0 dy and plane 1 dx, fewer than 2^31 elements.
 *   noise      field[b] element e (the linear (plane, y, x) index within the sample) = u * 2 - 1, u = (r >> 8) * 2^-24, r = word e % 4 of
 *              Philox4x32-10(key = (seed low ^ 0x454C4153, seed high), counter = (q low, q high ^ (b << 8), c low, c high)), q = e / 4, c the
 *              call's counter value: a function of (seed, c, b, e) only, the tail of a field of 4 q + 1..3 elements included
 *   smoothing  bpx_sepfilter on the field seen as a (2 B, Y, X) volume: wz = NULL, the Gaussian weights along y and x, mode "reflect"
 *   gather     output voxel (y, x) reads the source at fy = y + alpha s[0][y][x], fx = x + alpha s[1][y][x] of the smoothed field s, each one
 *              float32 multiply and one add, clamped to +-2^30 (a NaN becomes the lower bound); from there bpx_warp_apply's rules: the four
 *              bilinear taps and their association for the image, the voxel (floor(fy + 0.5), floor(fx + 0.5)) for the target, the border
 *              mode per integer tap index (BPX_WARP_CONSTANT / _REFLECT / _EDGE), cval for the image and 0 for the target outside. */
#define BPX_ELASTIC_REC_WORDS 8
#define BPX_ELASTIC_F_FIRED 0x1u
#define BPX_ELASTIC_W_FLAGS 0
#define BPX_ELASTIC_W_ALPHA 1
#define BPX_ELASTIC_W_CTR 2
#define BPX_ELASTIC_STREAM 24          /* the draw's Philox stream (counter word 1) */
#define BPX_ELASTIC_KEY_XOR 0x454C4153u /* the noise's key: seed low ^ this */
#define BPX_ELASTIC_ALPHA_MAX 1024.0f
/*   bpx_elastic_draw  : fills elastic_d[B][8] from Philox4x32-10(key = seed, counter = (sample, 24, c low, c high)), c = words 5-6 of the
 *                       sample's augmentation record records_d[b] (what bpx_aug_draw drew with: no second ticket): r0 fires ((uint64) r0 <
 *                       thr), r1 is the uniform of alpha, min(lo + u (hi - lo), hi), 0 <= lo <= hi <= 1024.  One launch, nothing read back.
 *   bpx_elastic_noise : fills field_d[B][2][Y][X] as stated above, c = words 2-3 of elastic_d[b].  One launch: one Philox call per four
 *                       elements, 16-byte stores where an address allows them.
 *   bpx_elastic_apply : out = the deformed pair, ONE out-of-place pass over image (1..16 channels) and target (1..8, BPX_F32 or BPX_U8) through
 *                       the smoothed field_d.  Whatever the field and alpha hold, the clamp and the border rule keep every load inside the
 *                       sample's plane.  No atomics, no workspace, nothing read back; capturable.
 * Argument checks run on the host before anything is launched and set bpx_last_error: null pointers, extents, the 2^31-element field,
 * channel counts, the target dtype, the mode, cval, out overlapping an input. */
int bpx_elastic_draw(uint64_t seed, uint64_t thr, float alpha_lo, float alpha_hi, int B, const uint32_t* records_d, uint32_t* elastic_d,
                     bpx_stream_t stream);
int bpx_elastic_noise(uint64_t seed, int B, int Y, int X, const uint32_t* elastic_d, float* field_d, bpx_stream_t stream);
int bpx_elastic_apply(const float* x_d, const void* t_d, int t_dtype, int B, int Z, int Y, int X, int C, int Ct, const uint32_t* elastic_d,
                      const float* field_d, int mode, float cval, float* x_out_d, void* t_out_d, bpx_stream_t stream);

/* ---- Noise2Void: blind-spot masking and its masked MSE (biapy_amd/n2v.py states the semantics; csrc/n2v.hip, csrc/n2v_core.h) -------------
 * x (B,Z,Y,X,C) float32, 1 <= C <= 8, B < 2^24, fewer than 2^31 voxels per sample; 2-D data is Z = 1.  The sample is cut into boxes of
 * box[0] x box[1] x box[2] voxels (each 1..64; 1 on an axis of extent 1), n_a = ceil(dim_a / s_a) per axis, box index i = (iz n_y + iy) n_x + ix,
 * fewer than 2^31 per sample.  Every (sample b, channel c, box i) draws on its own from Philox4x32-10 with the key (seed low ^ 0x4E32564D, seed
 * high) and the counter words (i, (b << 4) | c | (stream << 28), q low, q high), q = the call's counter value; mulhi(r, n) = (r * n) >> 32.
 *   stream 0: p_a = i_a s_a + mulhi(r_a, s_a) for a = z, y, x from words 0, 1, 2; any p_a >= dim_a: the box masks nothing.
 *   stream 1: the window [max(0, p_a - R_a), min(dim_a, p_a + R_a + 1)) per axis (radius 0..15; 0 on an axis of extent 1), n its voxels, cen the
 *     raster index of p in it.  BPX_N2V_UNIFORM_WITH_CP: k = mulhi(r0, n); _WITHOUT_CP: k = mulhi(r0, n - 1), k += (k >= cen), a one-voxel
 *     window masks nothing; the new value is the INPUT at the window's voxel of raster index k.  _IDENTITY: the value stays.  _NORMAL_ADDITIVE:
 *     x[p] + sigma n (one fp32 multiply, one add), n = sqrtf(-2 logf(u1)) cosf(2 pi u2), u1 = ((r0 >> 8) + 1) 2^-24, u2 = (r1 >> 8) 2^-24.
 *   bpx_n2v_boxes : boxes per sample of a configuration on a (Z, Y, X) sample, -1 (and bpx_last_error) when the configuration is refused.
 *   bpx_n2v_mask  : x_out = x except at the masked voxels; target (B,2C,Z,Y,X) channel-first: plane c the ORIGINAL value at the masked voxels of
 *                   channel c and 0 elsewhere, plane C + c 1 there and 0 elsewhere; coords / sources [B][C][boxes] int32: the linear (z, y, x)
 *                   index within the sample of the masked voxel and of its source (itself for identity / normal_additive), -1 and -1 when the
 *                   box masks nothing.  state_d[0] is the counter (the call draws with it and adds 1), state_d[1] the value the call drew with.
 *                   Two launches, no atomics, no workspace, nothing read back: capturable, a replay draws anew.  Out-of-place only.
 * Argument checks, in this order, before anything is launched: null pointers, B, C, extents, the 2^31-voxel sample, the manipulator, box and radius
 * per axis, sigma, the box count, alignment, overlap. */
#define BPX_N2V_UNIFORM_WITH_CP 0
#define BPX_N2V_UNIFORM_WITHOUT_CP 1
#define BPX_N2V_IDENTITY 2
#define BPX_N2V_NORMAL_ADDITIVE 3
typedef struct {
  uint64_t seed;
  int32_t box[3];          /* z, y, x */
  int32_t radius[3];       /* z, y, x */
  int32_t manipulator;     /* BPX_N2V_* */
  float sigma;             /* normal_additive only */
} bpx_n2v_cfg;
int64_t bpx_n2v_boxes(const bpx_n2v_cfg* cfg, int Z, int Y, int X);
int bpx_n2v_mask(const float* x_d, int B, int Z, int Y, int X, int C, const bpx_n2v_cfg* cfg, uint64_t* state_d, float* x_out_d, float* target_d,
                 int32_t* coords_d, int32_t* sources_d, bpx_stream_t stream);
/* The masked MSE: pred (N,C,voxels), target (N,2C,voxels) fp32 planar, v = target[:, :C], m = target[:, C:], e = v - pred m,
 * loss = sum e^2 / sum m over the whole batch (0 when sum m = 0).  bpx_chan_loss_*'s layout: grid (bpx_n2v_loss_blocks(voxels), N C).
 *   bpx_n2v_loss_sums  : partials_d[2][N C][blocks]: the blocks' partial sums of e^2, then those of m; fixed order.
 *   bpx_n2v_loss_finish: out_d[0] = the loss, out_d[1] = 1 / sum m (0 when sum m = 0), from fixed-order double sums in one block.
 *   bpx_n2v_loss_bwd   : dpred = (gup_d[0] saved_d[1]) * (-2 (m e)), saved_d = the finish's out_d. */
int bpx_n2v_loss_blocks(int64_t voxels);
int bpx_n2v_loss_sums(const float* pred_d, const float* target_d, int N, int C, int64_t voxels, float* partials_d, bpx_stream_t stream);
int bpx_n2v_loss_finish(const float* partials_d, int N, int C, int64_t voxels, float* out_d, bpx_stream_t stream);
int bpx_n2v_loss_bwd(const float* pred_d, const float* target_d, int N, int C, int64_t voxels, const float* saved_d, const float* gup_d,
                     float* dpred_d, bpx_stream_t stream);

/* ---- instance-segmentation training targets from id patches (biapy_amd/targets.py states the semantics; csrc/itarget.hip, csrc/itarget_core.h) ----
 * A batch of B samples (Z,Y,X), fewer than 2^31 voxels each, 1 <= B <= 65535, 0 <= n_max < 2^24, B (n_max + 1) < 2^31; 2-D data is Z = 1, ndim = 2.
 * Everything is per sample: the record of (sample b, id l) is row b (n_max + 1) + l.
 *   bpx_itarget_ids   : ids_d[i] = the id value i counts for: the value itself when it is an integer in 0..n_max, else 0 (background) and
 *                       *faults_d += 1 (NaN, +-inf, a fraction, a negative value, a value above n_max).  dtype BPX_F32, BPX_U8 (any address) or
 *                       BPX_I32.  One launch; the counter is only ever added to, the caller clears it.
 *   bpx_itarget_stats : the records of the batch from the ids of bpx_itarget_ids and their distances dist_d (B,Z,Y,X) float32 - bpx_edt per
 *                       sample in label mode, the float32 result.  Per present id: the area A, the coordinate sums S_a, the INCLUSIVE box lo_a, hi_a,
 *                       dmax = the largest d (+inf where the instance fills its sample), then the centroid c_a = double(S_a) / double(A) in the
 *                       sums' place and, with want_rc, rcmax = the largest rc over the instance,
 *                         rc = float32(sqrt(((dz sz)^2 + (dy sy)^2) + (dx sx)^2)), d_a = double(p_a) - c_a, fp64, in this order, no FMA;
 *                       (sz, sy, sx) = sampling, 1 when NULL.  Both maxima are taken on the uint32 bits of the non-negative float32, whose order
 *                       they keep.  Integer atomics only (add, min, max): the same bits every run.  Launches: init, accumulate, finish, and the
 *                       rcmax accumulate with want_rc.  records_d: bpx_itarget_records_bytes(B, n_max) bytes, 8-byte aligned (-1: refused).
 *   bpx_itarget_pack  : target (B,channels,Z,Y,X) float32 channel-first; channel i is BPX_ITARGET_* code (codes >> 4 i) & 15.  l = the voxel's id,
 *                       `edge` = an in-volume neighbour within generate_binary_structure(ndim, connectivity) carries another id, contour = edge
 *                       (BPX_ITARGET_THICK) or edge and l > 0 (BPX_ITARGET_INNER).  Every channel but C is 0 where l == 0.
 *                         F : 1; with BPX_ITARGET_F_EXCLUDES_C 0 where contour.          C : 1 where contour.
 *                         D : d / dmax[l] (one fp32 division), 1 where d is +inf; with BPX_ITARGET_D_RAW d itself, with BPX_ITARGET_D_CLIP too
 *                             min(d, d_clip).                                             Dc: 1.0f - rc / rcmax[l] (two fp32 operations), 1 when rcmax == 0.
 *                         H, V, Z (axes x, y, z): o = double(p_a) - c_a, e = o >= 0 ? double(hi_a) - c_a : c_a - double(lo_a),
 *                             float32(o / e), 0 when e == 0.  Z needs ndim = 3.
 *                       One launch, 64-bit offsets into the target (its element count may pass 2^31), 16-byte stores where a plane's address allows.
 * Argument checks, in this order, before anything is launched, setting bpx_last_error: null pointers, extents, the voxel count, B, n_max (and the
 * record count), the channel count and codes, connectivity, the contour mode, the flags and d_clip, sampling, alignment, overlap. */
#define BPX_ITARGET_F 1
#define BPX_ITARGET_C 2
#define BPX_ITARGET_D 3
#define BPX_ITARGET_DC 4
#define BPX_ITARGET_H 5
#define BPX_ITARGET_V 6
#define BPX_ITARGET_Z 7
#define BPX_ITARGET_THICK 0
#define BPX_ITARGET_INNER 1
#define BPX_ITARGET_F_EXCLUDES_C 1
#define BPX_ITARGET_D_RAW 2
#define BPX_ITARGET_D_CLIP 4
int64_t bpx_itarget_records_bytes(int B, int n_max);
int bpx_itarget_ids(const void* t_d, int dtype, int64_t n, int n_max, int32_t* ids_d, int32_t* faults_d, bpx_stream_t stream);
int bpx_itarget_stats(const int32_t* ids_d, const float* dist_d, int B, int Z, int Y, int X, int n_max, const double* sampling, int want_rc,
                      void* records_d, bpx_stream_t stream);
int bpx_itarget_pack(const int32_t* ids_d, const float* dist_d, const void* records_d, int B, int Z, int Y, int X, int n_max, uint32_t codes,
                     int channels, int ndim, int connectivity, int mode, int flags, float d_clip, const double* sampling, float* target_d,
                     bpx_stream_t stream);

/* ---- random training patches from device-resident volumes (biapy_amd/sampler.py states the semantics; csrc/sampler.hip) ---------
 * V volumes stay on the device: image (Z,Y,X,C), 1 <= C <= 16, float32 / uint8 / uint16; target (Z,Y,X,Ct), 1 <= Ct <= 8, uint8 / float32;
 * 2-D data is Z = 1.  A call draws B patch origins and copies the B windows of Pz x Py x Px voxels into a (B,Pz,Py,Px,C) float32 batch
 * and its (B,Pz,Py,Px,Ct) target.
 * ORIGIN RECORD, origins_d[B][4] int32 (16-byte rows):  word 0  v, the volume    word 1  z0    word 2  y0    word 3  x0
 * RANDOM NUMBERS: Philox4x32-10, key = seed, counter words = (sample b, stream, state_d[0] low, state_d[0] high).  Stream 0 is the only one
 * in use: r0..r3 its four words, r64 = (uint64) r0 << 32 | r1, mulhi64(a, n) = the high 64 bits of a * n (uniform in [0, n)).
 *   uniform mode (K == 0): every valid origin of every volume is equally likely.  n_v = (Z_v-Pz+1)(Y_v-Py+1)(X_v-Px+1), cum_d[V+1] their
 *     exclusive int64 prefix; k = mulhi64(r64, cum_d[V]); v = the volume with cum_d[v] <= k < cum_d[v+1]; k - cum_d[v] = (z0 * ny + y0) * nx + x0.
 *   class mode (1 <= K <= 8): every volume has a uint8 class map (Z,Y,X) with values < K.  u = (r2 >> 8) * 2^-24; the class c is the first
 *     with u < class_cum[c] (fp32 compare; the entries from the last class of positive probability on are 1.0).  rowcum_d[K][R+1] is the
 *     exclusive int64 prefix of the number of voxels of class c per row, the rows being all (v, z, y) of all volumes in that order
 *     (volume v starts at row row0_v).  k = mulhi64(r64, rowcum_d[c][R]); the row has rowcum_d[c][row] <= k < rowcum_d[c][row+1];
 *     j = k - rowcum_d[c][row]; the centre (z, y, x) is the (j+1)-th voxel of class c of that row;
 *     origin = clamp(centre - P / 2, 0, dim - P) per axis (integer division). */
typedef struct {
  const void* img;         /* (Z,Y,X,C) */
  const void* tgt;         /* (Z,Y,X,Ct) */
  const uint8_t* cls;      /* (Z,Y,X) class map, class mode only */
  int32_t Z, Y, X;
  int32_t reserved;
  int64_t row0;            /* index of the volume's first (z, y) row among the rows of all volumes: sum of Z * Y of the volumes before it */
} bpx_patch_vol;
typedef struct {
  uint64_t seed;           /* Philox key */
  int32_t V;               /* number of volumes */
  int32_t Pz, Py, Px;      /* the patch */
  int32_t K;               /* 0: uniform mode; 1..8: class mode with K classes */
  float class_cum[8];      /* class mode: running fp32 sum of the class probabilities */
} bpx_patch_cfg;
/*   bpx_patch_draw   : fills origins_d and then adds 1 to state_d[0], the sampler's counter; state_d[1] is the ticket of bpx_aug_draw's scheme
 *                      (0 between launches).  vols_h / vols_d: the same V descriptors on the host (argument checks: a patch larger than a volume
 *                      is refused) and on the device.  cum_d: uniform mode; rowcum_d and R (the number of rows): class mode.  One launch,
 *                      nothing is read back: capturable, a replay draws anew.
 *   bpx_patch_gather : x_out[b] = float32(img_v[z0:z0+Pz, y0:y0+Py, x0:x0+Px, :]) (uint8 / uint16 convert exactly; times `scale`, one fp32
 *                      multiply, when use_scale != 0; a float32 image without scale moves bit for bit), t_out[b] = the same window of the target,
 *                      bit for bit.  Origins are read from origins_d and clamped into their volume.  One launch. */
int bpx_patch_draw(const bpx_patch_cfg* cfg, const bpx_patch_vol* vols_h, const bpx_patch_vol* vols_d, const int64_t* cum_d, const int64_t* rowcum_d,
                   int64_t R, int B, uint64_t* state_d, int32_t* origins_d, bpx_stream_t stream);
int bpx_patch_gather(const bpx_patch_vol* vols_h, const bpx_patch_vol* vols_d, int V, int img_dtype, int C, int tgt_dtype, int Ct, int Pz, int Py, int Px,
                     const int32_t* origins_d, int B, int use_scale, float scale, float* x_out_d, void* t_out_d, bpx_stream_t stream);

/* ---- connected-component labelling of a binary volume (biapy_amd/prepost.py: label, component_sizes, remove_small_objects; csrc/label.hip) ----
 * mask (Z,Y,X) uint8, contiguous, every nonzero byte foreground; 2-D is Z = 1.  connectivity 1 / 2 / 3: faces, + edges, + corners (6 / 18 / 26
 * neighbours; 4 / 8 at Z = 1).  labels (Z,Y,X) int32: 0 background, components 1..N IN RASTER ORDER OF EACH COMPONENT'S FIRST VOXEL - bit for bit
 * scipy.ndimage.label(mask, generate_binary_structure(ndim, connectivity)).  Union-find with integer atomics, labels_d itself the parent array:
 * the same bits every run, a launch sequence fixed by (Z, Y, X, connectivity), nothing read back, capturable.  Z * Y * X < 2^31.
 *   bpx_label_workspace : bytes of workspace bpx_label_u8 needs (4 per chunk of 4096 voxels); NEGATIVE when an extent is < 1 or the volume has
 *                         2^31 voxels or more (refused: int32 indices).
 *   bpx_label_u8        : labels_d = the labels, *num_d = N (device int32).  labels_d is the only voxel-sized array written.
 *   bpx_label_sizes     : sizes_d[l] = number of the n voxels with label l for 0 <= l <= n_max (np.bincount(labels, minlength = n_max + 1) cut
 *                         at n_max); labels outside [0, n_max] are not counted.
 *   bpx_label_filter    : zeroes every component with fewer than min_size voxels (skimage.morphology.remove_small_objects on a label image).
 *                         sizes_d: IN the sizes from bpx_label_sizes for the same n_max, OUT the id map applied (scratch).  relabel == 0 keeps the
 *                         survivors' ids; relabel != 0 renumbers them 1..N' in the same order.  *num_out_d = N', the number of survivors (may be
 *                         NULL).  Labels above n_max become 0.
 * All entry points check their arguments on the host and return nonzero, with bpx_last_error naming the cause, before anything is launched. */
int64_t bpx_label_workspace(int Z, int Y, int X);
int bpx_label_u8(const uint8_t* mask_d, int Z, int Y, int X, int connectivity, int32_t* labels_d, int32_t* num_d, void* ws_d, int64_t ws_bytes,
                 bpx_stream_t stream);
int bpx_label_sizes(const int32_t* labels_d, int64_t n, int n_max, int32_t* sizes_d, bpx_stream_t stream);
int bpx_label_filter(int32_t* labels_d, int64_t n, int n_max, int32_t* sizes_d, int min_size, int relabel, int32_t* num_out_d, bpx_stream_t stream);
int bpx_debug_set_label_tiled(int on); /* test / A-B hook of bpx_label_u8's merge: 0 (default) = every union on global memory; 1 = tiles resolved in LDS, then unions across tile borders only; same bits (environment: BPX_LABEL_TILED) */

/* ---- exact Euclidean distance transform of a mask or a label volume (biapy_amd/prepost.py: distance_transform_edt, label_distance; csrc/edt.hip) ----
 * keys (Z,Y,X) contiguous, BPX_U8 or BPX_I32; 2-D is Z = 1.  key(v) = (value != 0) with label_mode == 0, the value itself otherwise.
 *   out(v) = 0 where key(v) == 0, else the least |u - v|^2 over the voxels u with key(u) != key(v), |.| the Euclidean norm of the index
 *   difference scaled per axis by sampling (host pointer to 3 doubles, z y x).  The volume border is no source.  Where the volume holds no
 *   voxel of another key the result is a SENTINEL: INT32_MAX (int32 results), +inf (float32 results) - scipy.ndimage.distance_transform_edt
 *   answers with distances to a fictitious point there.
 * sampling == NULL, the integer path: exact.  squared != 0: out_d int32; else out_d float32 = float32(sqrt(float64(squared distance))), which
 *   is scipy's float64 result rounded to float32 bit for bit.  out_d is the only voxel-sized array written (in place); Z^2 + Y^2 + X^2 must stay
 *   below 2^31 - 1.  sampling given (positive, finite), the fp64 path: fp64 throughout, out_d float32 = the rounded distance, or its square.
 * Three launches fixed by (Z, Y, X) and the path, no atomics, nothing read back, the same bits every run, capturable.  Z * Y * X < 2^31.
 *   bpx_edt_workspace : bytes of workspace; NEGATIVE for a refused shape (an extent < 1, 2^31 voxels or more, the integer path's limit).
 *                       Integer path: 8 * E, E = max(T(Z * X) * Y, T(Y * X) * Z) with T(columns) = min(131072, a quarter of the columns rounded
 *                       up to 64) - the envelope stacks of the threads in flight of the Y and of the Z pass, never more than half the output's
 *                       bytes plus one wave's share.  The fp64 path: 8 bytes per voxel + 16 * E.
 * Argument checks run on the host before anything is launched and set bpx_last_error. */
int64_t bpx_edt_workspace(int Z, int Y, int X, int fp64_path);
int bpx_edt(const void* key_d, int key_dtype, int label_mode, int Z, int Y, int X, const double* sampling, int squared, void* out_d, void* ws_d,
            int64_t ws_bytes, bpx_stream_t stream);

/* ---- the same transform with the nearest source (biapy_amd/prepost.py: distance_transform_edt(return_indices=...), expand_labels,
 *      voronoi_on_mask; csrc/edt_index.hip) ----
 * keys (Z,Y,X) contiguous, BPX_U8 or BPX_I32; 2-D is Z = 1.  A voxel is a SOURCE when its value is 0; with invert != 0, when it is nonzero.
 *   index_d (Z,Y,X) int32: for every voxel the linear index (C order) of the source u with the least |u - v|^2, |.| as in bpx_edt; among equally
 *   near sources the one with the SMALLEST LINEAR INDEX (the raster-first one; not scipy's choice).  A source's index is its own.  A volume
 *   without any source gets -1 everywhere, beside the distance sentinel.  On the fp64 path the source returned is a nearest one up to that path's
 *   rounding; which of several sources whose fp64 costs differ by rounding only is returned is unspecified.
 *   dist_d: the distances of bpx_edt for key = "not a source" (int32 squared / float32, the same bits), or NULL for the indices alone.
 * Three launches fixed by (Z, Y, X) and the path, no atomics, nothing read back, the same bits every run, capturable.  Z * Y * X < 2^31; on the
 *   integer path Z^2 + Y^2 + X^2 < 2^31 - 1.
 *   bpx_edt_index_workspace : bytes of workspace OF A CALL WITH dist_d; an integer-path call with dist_d == NULL needs this PLUS 4 * Z * Y * X bytes
 *                       (bpx_edt_index refuses less).  NEGATIVE for a refused shape, as bpx_edt_workspace.  The index travels in the envelope's stack
 *                       entries: integer path 12 * E, E = max(T(Z * X) * Y, T(Y * X) * Z) with T(columns) = min(98304, a quarter of the columns
 *                       rounded up to 64); the fp64 path 8 bytes per voxel + 20 * E, with or without dist_d.  The 4 more bytes per voxel without dist_d are
 *                       the home of the integer path's values, which otherwise live in dist_d.
 * Argument checks run on the host before anything is launched and set bpx_last_error. */
int64_t bpx_edt_index_workspace(int Z, int Y, int X, int fp64_path);
int bpx_edt_index(const void* key_d, int key_dtype, int invert, int Z, int Y, int X, const double* sampling, int squared, void* dist_d,
                  int32_t* index_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream);

/* ---- seeded watershed of an image from a marker volume (biapy_amd/prepost.py: watershed; csrc/watershed.hip, csrc/watershed_core.h) ----
 * image (Z,Y,X) BPX_F32 or BPX_I32, markers (Z,Y,X) int32, mask (Z,Y,X) uint8 or NULL (every voxel), all contiguous; 2-D is Z = 1.
 *   nodes: the voxels with mask != 0.  edges: two nodes that are neighbours at `connectivity` (1 / 2 / 3 as bpx_label_u8).  weight of an edge:
 *   max(k(u), k(v)), k the order-preserving uint32 image of the value (int32: v + 2^31; float32: the sign-flip map, -0.0 < +0.0; NaN unspecified).
 *   Strict total order of the edges: (weight, linear index of the raster-first endpoint u, rank of the offset among u's forward offsets in
 *   (dz, dy, dx) lexicographic order).  A voxel with markers > 0 inside the mask is seeded with that label; other markers are ignored.
 *   out (Z,Y,X) int32 = the label of the voxel's tree in the unique minimum spanning forest in which no tree holds two seeds (Kruskal in that
 *   order, joining two trees unless they are the same or both seeded); 0 where the tree holds no seed and outside the mask.  Ties of the image go
 *   to the raster-first edge.  Not scikit-image's tie-breaking (the age of a heap entry), no compactness, no watershed line.
 * Boruvka rounds on the union-find of the labelling: 4 R + 3 launches with R = ceil(log2(max(n, 2))) + 1, fixed by (Z, Y, X, connectivity); rounds
 * after the last one that joined anything return at once.  *rounds_d (device int32) = the number of rounds that did.  Integer atomics only: the
 * same bits every run; nothing read back; capturable.  Z * Y * X < 2^31.
 *   bpx_watershed_workspace : bytes of workspace: 12 per voxel (8 the pick of a tree, 4 its parent) + the round flags; NEGATIVE when an extent is
 *                             < 1 or the volume has 2^31 voxels or more.  12.9 GB at 1024^3.
 * Argument checks run on the host before anything is launched and set bpx_last_error. */
int64_t bpx_watershed_workspace(int Z, int Y, int X);
int bpx_watershed(const void* image_d, int image_dtype, const int32_t* markers_d, const uint8_t* mask_d, int Z, int Y, int X, int connectivity,
                  int32_t* out_d, int32_t* rounds_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream);

/* ---- sparse overlap (contingency) table of two label volumes (biapy_amd/prepost.py: label_overlap, matching; csrc/overlap.hip, csrc/overlap_core.h) ----
 * a, b: n contiguous int32 labels each, 1 <= n < 2^31; a label <= 0 counts as background 0 (as the markers of bpx_watershed).  The result is
 * every distinct pair (a[i], b[i]) with the number of voxels that carry it, background pairs included: keys_d[k] = a << 32 | b (int64),
 * counts_d[k] the count, for k in [0, K) in UNSPECIFIED order; the entries [K, max_pairs) are INT64_MAX and 0; *num_d (device int32) = K.
 * With more than max_pairs distinct pairs *num_d = -1, the call returns normally and keys_d / counts_d are unspecified.
 * An open-addressing table of the power of two >= 2 * max_pairs slots (64-bit key claimed by compare-and-swap, 32-bit count by atomic add) in the
 * workspace; a wave run-length-compresses a span of 8192 voxels, carries the open run in registers and counts into its block's 512-slot table in
 * LDS, which is added to the global table once per block: a uniform block costs one global update.
 * Three launches (clear, count, compact) fixed by (n, max_pairs); integer atomics only; nothing read back; capturable.
 *   bpx_overlap_workspace : bytes of workspace: 12 per slot + 16; NEGATIVE when max_pairs < 1 or the table would pass 2^31 slots (max_pairs > 2^30).
 * Argument checks run on the host before anything is launched and set bpx_last_error. */
int64_t bpx_overlap_workspace(int64_t max_pairs);
int bpx_label_overlap(const int32_t* a_d, const int32_t* b_d, int64_t n, int64_t max_pairs, int64_t* keys_d, int32_t* counts_d, int32_t* num_d,
                      void* ws_d, int64_t ws_bytes, bpx_stream_t stream);
int bpx_debug_set_overlap_per_voxel(int on); /* timing hook of bpx_label_overlap's count pass: 0 (default) = spans, run lengths and the carried run; 1 = one table insert per voxel; the same table (environment: BPX_OVERLAP_PER_VOXEL) */

/* ---- stitching per-block labels into the labels of the whole volume (biapy_amd/prepost.py: LabelStitcher, label_blocks; csrc/stitch.hip, csrc/stitch_core.h) ----
 * A volume (Z,Y,X) is cut by a regular grid of blocks (bz,by,bx), the last block of an axis may be ragged; blocks are numbered in raster order of
 * (i,j,k).  Block b is a contiguous int32 array of its own extents with local labels 1..n_b (<= 0 or > n_b: background), n_b = nums_d[b] on the
 * device.  offs_d[b] = exclusive prefix sum of max(n_b, 0), offs_d[nblocks] = T; the global id of (b, l) is offs_d[b] + l; parent_d[0..t_max] is a
 * union-find over these ids (bpx_label_u8's, integer atomic min only); first_d / key_d[0..t_max] are int64.  When T > t_max flag_d becomes 1, ids
 * above t_max take part in nothing and bpx_stitch_apply writes nothing.
 *   bpx_stitch_begin   : offs_d from nums_d, parent = identity, first = key = INT64_MAX, *flag_d = 0.
 *   bpx_stitch_first   : per block: first_d[g] = the smallest global linear index (z Y + y) X + x of g's voxels (64-bit atomic min, issued by run
 *                        heads only).  num_d / off_d point at the block's entries of nums_d / offs_d.
 *   bpx_stitch_shell   : rule "touch": every labelled shell voxel of every block is united with every labelled backward neighbour (3 / 9 / 13
 *                        offsets at connectivity 1 / 2 / 3) that lies inside the volume in another block - face, edge and corner neighbours.
 *   bpx_stitch_contact : rule "contact": for every pair of face-adjacent blocks A (low), B (high): c(a,b) = in-plane positions where A's last
 *                        plane holds a and B's first plane holds b, s_A(a) / s_B(b) = positions of the plane that hold the label; a and b are
 *                        united iff c(a,b) q >= p min(s_A(a), s_B(b)) in int64.  Unions are transitive.  More than max_pairs distinct pairs raise
 *                        the flag.  bpx_stitch_contact_workspace: the bytes it needs, NEGATIVE when refused.
 *   bpx_stitch_resolve : parent_d[g] = root of g, key_d[root] = min of first_d over the root's set (INT64_MAX: no voxel), the flag when
 *                        *total_d > t_max (total_d = offs_d + nblocks).  Numbering the roots 1..M by ascending key - raster order of each object's
 *                        first voxel, scipy.ndimage.label's numbering - is one sort over t_max + 1 keys on the caller's side.
 *   bpx_stitch_apply   : per block, in place: labels[i] = map_d[off + labels[i]] (0 for background); nothing when *flag_d != 0.
 * No float arithmetic: the same bits every run.  Launches fixed by the grid, nothing read back, capturable.  A block stays below 2^31 voxels, the
 * volume need not.  Argument checks run on the host, in the order of the arguments' mention above, and set bpx_last_error. */
typedef struct bpx_stitch_block { void* labels; int32_t z0, y0, x0, ez, ey, ex; } bpx_stitch_block; /* 32 bytes: pointer, origin, extents */
int bpx_stitch_begin(const int32_t* nums_d, int nblocks, int t_max, int64_t* offs_d, int32_t* parent_d, int64_t* first_d, int64_t* key_d,
                     int32_t* flag_d, bpx_stream_t stream);
int bpx_stitch_first(const int32_t* labels_d, int ez, int ey, int ex, int z0, int y0, int x0, int Y, int X, const int32_t* num_d,
                     const int64_t* off_d, int t_max, int64_t* first_d, bpx_stream_t stream);
int bpx_stitch_shell(const bpx_stitch_block* blocks_d, int Z, int Y, int X, int bz, int by, int bx, int connectivity, const int32_t* nums_d,
                     const int64_t* offs_d, int t_max, int32_t* parent_d, bpx_stream_t stream);
int64_t bpx_stitch_contact_workspace(int Z, int Y, int X, int bz, int by, int bx, int t_max, int64_t max_pairs);
int bpx_stitch_contact(const bpx_stitch_block* blocks_d, int Z, int Y, int X, int bz, int by, int bx, const int32_t* nums_d, const int64_t* offs_d,
                       int t_max, int p, int q, int64_t max_pairs, int32_t* parent_d, int32_t* flag_d, void* ws_d, int64_t ws_bytes,
                       bpx_stream_t stream);
int bpx_stitch_resolve(int32_t* parent_d, const int64_t* first_d, int64_t* key_d, const int64_t* total_d, int t_max, int32_t* flag_d,
                       bpx_stream_t stream);
int bpx_stitch_apply(int32_t* labels_d, int64_t n, const int32_t* num_d, const int64_t* off_d, int t_max, const int32_t* map_d,
                     const int32_t* flag_d, bpx_stream_t stream);

/* ---- region properties of a label volume (biapy_amd/prepost.py: region_props, centroids, select_objects; csrc/regionprops.hip, csrc/regionprops_core.h) ----
 * labels (Z,Y,X) int32, contiguous, 4-byte aligned; 2-D is Z = 1; Z * Y * X < 2^31; 0 <= n_max < 2^31 - 1.  For every label l in 1..n_max:
 *   area_d[l]    = the number of voxels that carry l (int32; bpx_label_sizes' count),
 *   sums_d[l][3] = the sums of those voxels' z, y and x (int64, exact: below 2^62),
 *   bbox_d[l][6] = (z0, y0, x0, z1, y1, x1), half-open: scikit-image's bbox, the slices of scipy.ndimage.find_objects.
 * Row 0 (background) is all zeros, and so is the row of a label that no voxel carries.  Voxels with a label <= 0 or > n_max contribute nothing
 * (the convention of bpx_label_sizes and bpx_watershed).
 * A wave run-length-compresses a span of 8192 voxels as bpx_label_overlap does, with every row start a run head as well, so that a run
 * x0 .. x0 + L - 1 of row (z, y) adds in closed form: area L, sums (L z, L y, L x0 + L (L - 1) / 2), box min (z, y, x0), max (z, y, x0 + L - 1).
 * Three launches (init, accumulate, finish) fixed by (Z, Y, X, n_max); the outputs are the accumulators, no workspace; integer atomics only
 * (uint32 / uint64 add, int32 min / max): the same bits every run; nothing read back; capturable.
 * Argument checks run on the host before anything is launched and set bpx_last_error. */
int bpx_region_props(const int32_t* labels_d, int Z, int Y, int X, int n_max, int32_t* area_d, int64_t* sums_d, int32_t* bbox_d, bpx_stream_t stream);
int bpx_debug_set_regionprops_local(int on); /* test / A-B hook of bpx_region_props' accumulate pass: 1 (default) = the runs of a block meet in a 256-slot table in LDS that is merged into the outputs once per block; 0 = every run straight to the outputs, faster on a volume without labels and far slower on any other; negative = back to the default; same bits (environment: BPX_REGIONPROPS_LOCAL) */

/* ---- shape properties of a label volume (biapy_amd/prepost.py: shape_props and the derived measures; csrc/shapeprops.hip, csrc/shapeprops_core.h) ----
 * labels (Z,Y,X) int32, contiguous, 4-byte aligned; 2-D is Z = 1; Z * Y * X < 2^31; 0 <= n_max < 2^31 - 1; a label <= 0 or > n_max is background 0
 * (as for bpx_region_props).  Row 0 and the row of a label that no voxel carries are all zeros in every output.
 *   bpx_region_moments: mom_d[l][6] = the sums of zz, yy, xx, zy, zx, yx over the voxels of l (int64, exact).  Refused when
 *     n * (Emax - 1)^2 >= 2^63 (n = Z * Y * X, Emax the largest extent): below that every sum fits.  The accumulate pass of bpx_region_props with
 *     another closed form per run: sum xx = L x0^2 + x0 L (L - 1) + (L - 1) L (2 L - 1) / 6, sum zx = z sum x, sum yx = y sum x, sum zz = L z^2,
 *     sum yy = L y^2, sum zy = L z y.  With cov_d != NULL a finish pass forms cov_d[l][6] (float64, the same order) from area_d and sums_d, THE
 *     OUTPUTS OF bpx_region_props for the same volume and n_max: the numerator A * S_ab - S_a * S_b exactly in 128 bits, converted to double
 *     (high word * 2^64 + low word), divided by A twice; 0 where the area is 0.  cov_d == NULL: the sums only; area_d and sums_d are not read.
 *     Launches: zero, accumulate, finish (with cov_d).
 *   bpx_region_faces: faces_d[l][3] (int64) = per axis z, y, x the number of pairs (voxel of l, one of the two directions along the axis) whose
 *     neighbour lies outside the volume or carries another label: the surface of l in voxel faces.  Z = 1 gives 2 * area on the z axis.
 *     Launches: zero, count.
 *   bpx_region_perimeter2d: classes_d[l][3] (int32) = the number of pixels of l in the three weight classes (1, sqrt 2, (1 + sqrt 2) / 2) of
 *     scikit-image's perimeter(labels == l, neighborhood=4): a border pixel carries a label > 0 and has a 4-neighbour that differs (outside the
 *     image differs); k4 / kd count its 4- / diagonal neighbours that are border pixels of the same label; code = 1 + 2 k4 + 10 kd is of class 0
 *     for 5, 7, 15, 17, 25, 27, class 1 for 21, 33, class 2 for 13, 23, of none otherwise.  Launches: zero, classify.
 * Integer atomics only (uint32 / uint64 add): the same bits every run; no workspace; nothing read back; capturable.
 * Argument checks run on the host before anything is launched, those of bpx_region_props in its order first, and set bpx_last_error. */
int bpx_region_moments(const int32_t* labels_d, int Z, int Y, int X, int n_max, const int32_t* area_d, const int64_t* sums_d, int64_t* mom_d,
                       double* cov_d, bpx_stream_t stream);
int bpx_region_faces(const int32_t* labels_d, int Z, int Y, int X, int n_max, int64_t* faces_d, bpx_stream_t stream);
int bpx_region_perimeter2d(const int32_t* labels_d, int Y, int X, int n_max, int32_t* classes_d, bpx_stream_t stream);

/* ---- intensity properties of a label volume (biapy_amd/prepost.py: intensity_props; csrc/intensityprops.hip, csrc/intensityprops_core.h) ----
 * labels (Z,Y,X) int32 and image (Z,Y,X) of image_dtype BPX_F32, BPX_U8 or BPX_U16, both contiguous; 2-D is Z = 1; Z * Y * X < 2^31;
 * 0 <= n_max < 2^31 - 1; a label <= 0 or > n_max is background 0 (as for bpx_region_props).  NL = 9 for BPX_F32, 1 for the integer types.  For
 * every label l in 1..n_max, over the voxels that carry it:
 *   area_d[l]         = their number (int32; bpx_region_props' area),
 *   min_d[l], max_d[l] = the smallest and the largest image value: float32 for BPX_F32 (the winning voxel's bits, -0.0 < +0.0, NaN voxels left
 *                       out, NaN when every voxel is NaN), int32 for the integer types,
 *   limbs_d[l][NL]    = the exact sum of the finite voxels as int64 limbs.  BPX_F32: unit 2^-149, limb j weighs 2^(32 j); with E = (bits >> 23)
 *                       & 255, f = bits & 0x7fffff, (m, q) = (f, 0) if E == 0 else (f | 0x800000, E - 1) and w = m << (q & 31) a voxel adds
 *                       w & 0xffffffff to limb q >> 5 and w >> 32 to limb (q >> 5) + 1, both negated for a negative voxel.  Integers: the plain sum,
 *   nonfinite_d[l][3] = the numbers of NaN, +inf and -inf voxels (int32; zeros for the integer types),
 *   sum_d[l]          = sum_j limbs[j] * 2^(32 j - 149) (unit 1 for integers) rounded ONCE to float64, to nearest even; +0.0 for an exact zero; NaN
 *                       with a NaN voxel or infinities of both signs, else the infinity present,
 *   mean_d[l]         = sum_d[l] / area_d[l], one IEEE division (a second rounding).
 * Row 0 and the row of a label that no voxel carries are all zeros, with NaN in mean_d.
 * Three launches (init, accumulate, finish) fixed by the shape, the dtype and n_max; the outputs are the accumulators (min_d / max_d hold
 * order-preserving keys until the finish pass), no workspace; relaxed integer atomics only (uint32 / int64 add, uint32 min / max), no float
 * atomics: the same bits every run; nothing read back; capturable.
 * Argument checks run on the host before anything is launched, in this order, and set bpx_last_error: null pointers, extents, the voxel
 * count, n_max, the dtype, alignment (4 bytes for labels, area, min, max, nonfinite; 8 for limbs, sum, mean; the element size for the image). */
int bpx_intensity_props(const int32_t* labels_d, const void* image_d, int image_dtype, int Z, int Y, int X, int n_max, int32_t* area_d, void* min_d,
                        void* max_d, int64_t* limbs_d, int32_t* nonfinite_d, double* sum_d, double* mean_d, bpx_stream_t stream);
int bpx_debug_set_intensityprops_wave(int on); /* test / A-B hook of bpx_intensity_props' accumulate pass: 0 = form (a), each lane merges its four voxels and sends them to the block's table; 1 = form (b), in addition a trip of 256 voxels of one label and one limb pair is reduced across the wave and sent once; negative = back to the default; same bits (environment: BPX_INTENSITYPROPS_WAVE) */
/* the per-voxel decomposition and the rounding of bpx_intensity_props on HOST memory (nothing is launched; for tests without a device):
 * the limb (q >> 5; -1 for NaN and the infinities, which have no pieces) and the two signed pieces of a float32's bits; the float64 nearest to
 * nl limbs (nl 9: unit 2^-149; nl 1: unit 1), every limb below 2^63 - 2^32 in magnitude. */
int bpx_intensity_pieces_host(uint32_t bits, int* limb, int64_t* lo, int64_t* hi);
int bpx_intensity_round_host(const int64_t* limbs, int nl, double* out);

/* ---- morphology: erosion, dilation and the boundary map (biapy_amd/prepost.py: binary_erosion, binary_dilation, binary_opening, binary_closing,
 * erosion, dilation, find_boundaries; csrc/morph.hip, csrc/morph_core.h) ----
 * in (Z,Y,X) contiguous, dtype BPX_U8, BPX_I32 or BPX_F32 (the 4-byte types 4-byte aligned; uint8 at any address); ndim 3, or 2 with Z = 1;
 * Z * Y * X < 2^31.  The structuring element is scipy.ndimage.generate_binary_structure(ndim, connectivity), 1 <= connectivity <= ndim: the row
 * (dz, dy) of the 3 x 3 (x 3) neighbourhood, k = |dz| + |dy|, belongs to it when k <= connectivity (ndim 2: only dz = 0) and contributes
 * x - 1, x, x + 1 when k + 1 <= connectivity, x alone otherwise.
 *   op 0 (erode): out = the minimum over the element, 1 (dilate): the maximum - out has the input's type;
 *   op 2 (boundary): out is uint8, 1 where the minimum and the maximum differ; with flag 4 (inner) only where in != background as well.
 * Out-of-volume neighbours are ignored (scipy's grey filters in mode="reflect" for these elements; binary erosion with border_value=1, binary
 * dilation with border_value=0); with flag 2 (absorbing border; binary only) they count as 0 for erosion and 1 for dilation (scipy's
 * border_value=0 erosion, border_value=1 dilation).  Flag 1 (binary; uint8, erode / dilate only): every nonzero byte is 1, out holds 0 / 1.
 * float32: equal as values; which of -0.0 / +0.0 is chosen and NaN are unspecified.
 * One launch, 16 bytes of a row per lane; no atomics, no workspace; the same bits every run; nothing read back; capturable.  out_d must not
 * be in_d.  Argument checks run on the host before anything is launched and set bpx_last_error. */
int bpx_morph(const void* in_d, int dtype, int Z, int Y, int X, int ndim, int connectivity, int op, int flags, int background, void* out_d,
              bpx_stream_t stream);

/* ---- local maxima (biapy_amd/prepost.py: peak_mask, peak_local_max; csrc/peaks.hip, csrc/peaks_core.h) ----
 * img (Z,Y,X) contiguous, dtype BPX_F32 or BPX_I32, 4-byte aligned (16-byte accesses where the address allows, the same bits otherwise);
 * Z * Y * X < 2^31; a 2-D image is Z = 1, rz = 0.  The key of voxel v is (k(v) << 32) | (0xFFFFFFFF - linear_index(v)) as uint64, k the
 * order-preserving uint32 image of the value that bpx_watershed uses (int32: v + 2^31; float32: the sign-flip map, -0.0 < +0.0; NaN
 * unspecified).  Voxel v is a PEAK when its key is the maximum of the keys in the box [z-rz, z+rz] x [y-ry, y+ry] x [x-rx, x+rx] clipped to
 * the volume (radii 0..64), its value is > threshold (compared in double; -inf: no threshold) and it lies at least bz / by / bx voxels from both
 * faces of its axis (no voxel on an axis of extent <= 2 b).  Among equal values the raster-first voxel wins, so no two peaks lie in each
 * other's box.
 *   mask_d  : uint8 (Z,Y,X), 1 at the peaks and 0 elsewhere; may be null.
 *   keys_d  : uint64[max_peaks], 8-byte aligned: the peaks' keys in an order that may vary between runs (the set does not), 0 in the unused
 *             slots (no voxel carries key 0); may be null.  Past max_peaks keys are dropped.
 *   *num_d  : the number of peaks, counted beyond max_peaks as well (more than max_peaks: the key array holds some max_peaks of them).
 * One pass per axis with a nonzero radius and more than one voxel (one pass when there is none) after one launch that clears the outputs: launches fixed by (Z, Y, X, radii),
 * at most 2 r + 4 loads per voxel and axis, never the box.  The workspace holds at most two key volumes:
 *   bpx_peaks_workspace : bytes of workspace (16 per voxel); NEGATIVE when an extent is < 1 or the volume has 2^31 voxels or more.
 * Integer atomics only (one per block with a peak); nothing read back; capturable.  Argument checks run on the host before anything is
 * launched and set bpx_last_error. */
int64_t bpx_peaks_workspace(int Z, int Y, int X);
int bpx_peak_local_max(const void* img_d, int dtype, int Z, int Y, int X, int rz, int ry, int rx, double threshold, int bz, int by, int bx,
                       void* mask_d, void* keys_d, int max_peaks, int* num_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream);

/* ---- median filter (biapy_amd/prepost.py: median_filter, median_filter_axes; csrc/median.hip, csrc/median_core.h) ----
 * in / out (Z,Y,X) contiguous, dtype BPX_F32 (4-byte aligned) or BPX_U8; Z * Y * X < 2^31; a 2-D image is Z = 1, sz = 1; out_d must not be
 * in_d.  out[v] is the element of rank W / 2 among the W = sz * sy * sx values of the window centred on v (sizes odd, 1..15 each, W <= 125),
 * ordered by their order-preserving uint32 key (float32: bits | 0x80000000 for a clear sign bit, ~bits otherwise, so -0.0 < +0.0 and NaNs sort
 * by their bits beyond the infinities of their sign; uint8: the value) and returned with its bits: scipy.ndimage.median_filter(in, size=(sz,
 * sy, sx), mode=, cval=) as values.  mode: 0 "reflect" (d c b a | a b c d, over as many periods as the window needs), 1 "nearest", 2
 * "constant" with cval (finite as float32; an integer in 0..255 for uint8; ignored by the other modes but checked).
 * One launch fixed by (Z, Y, X, dtype, sizes): a block stages its tile and halo into LDS as keys and every thread selects in registers with
 * min / max only.  No workspace, no atomics, nothing read back; the same bits every run; capturable.  Argument checks run on the host before
 * anything is launched and set bpx_last_error. */
int bpx_median_filter(const void* in_d, int dtype, int Z, int Y, int X, int sz, int sy, int sx, int mode, double cval, void* out_d,
                      bpx_stream_t stream);

/* ---- separable filter (biapy_amd/prepost.py: separable_filter, gaussian_filter, gaussian_laplace; csrc/sepfilter.hip, csrc/sepfilter_core.h) ----
 * in / out / ws (Z,Y,X) contiguous float32 (4-byte aligned; 16-byte stores are used only where an address allows them); Z * Y * X < 2^31; a
 * 2-D image is Z = 1 with wz = NULL.  Correlation with one 1-D kernel per axis, z then y then x (scipy.ndimage.correlate1d chained): wz / wy /
 * wx are HOST pointers to 2 r + 1 float32 weights, r in 0..32; NULL with a negative radius skips the axis.  Along an axis of n voxels
 *   acc = w[0] * v[f(i - r)];  acc = acc + w[j] * v[f(i + j - r)] for j = 1 .. 2r in that order;  out[i] = acc
 * every * and + one IEEE float32 operation, round to nearest, no FMA, no folded taps, denormals kept; the float32 result of one axis is the
 * input of the next.  mode f: 0 "reflect" (d c b a | a b c d), 1 "mirror" (d c b | a b c d; n = 1 maps to 0), 2 "nearest", 3 "constant" with
 * float32(cval) outside the axis at every pass (cval finite as float32; ignored by the other modes but checked); all fold over as many
 * periods as r needs.
 *   bpx_sepfilter_workspace : 4 * Z * Y * X bytes when two or more radii are not negative, else 0; -1 when an extent is < 1, the volume has
 *                             2^31 voxels or more, or a radius is above 32.
 * One launch per active axis; the passes alternate between out_d and ws_d so that the last writes out_d; in_d is never written and must
 * overlap neither; with no active axis out is a copy of in's bits.  The weights travel by value in the kernel arguments: no atomics, nothing
 * allocated, copied or read back; the same bits every run; capturable.  Argument checks run on the host before anything is launched, in
 * this order, and set bpx_last_error: null pointers (in_d, out_d, weights of a radius that is not negative); extents; 2^31 voxels; a radius
 * outside 0..32; a weight that is not finite; the mode; cval; the workspace; aliasing; alignment. */
int64_t bpx_sepfilter_workspace(int Z, int Y, int X, int rz, int ry, int rx);
int bpx_sepfilter(const void* in_d, int Z, int Y, int X, const float* wz, int rz, const float* wy, int ry, const float* wx, int rx, int mode,
                  double cval, void* out_d, void* ws_d, int64_t ws_bytes, bpx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BIAPY_AMD_H */
