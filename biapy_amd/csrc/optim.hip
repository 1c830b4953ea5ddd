// What sits between `backward` and the end of `optimizer.step()` in the reference loop (biapy/engine/train_engine.py:166-177), for a step that is
// replayed from a HIP graph and therefore may hold no host value that changes from step to step:
//   * the global gradient norm and torch's clip coefficient (`clip_grad_norm_`, norm_type 2) as two device floats;
//   * the Adam / AdamW update (`bpx_adam_step`), which `bpx_adam_step_dev` runs with beta1 read from device memory (OneCycleLR cycles it every
//     step) and the gradient scaled by a device float first (the clip coefficient), the product stored back so that `p.grad` holds what
//     `clip_grad_norm_` leaves;
//   * the SGD update (momentum, dampening, Nesterov, weight decay) in the fp32 arithmetic and order of torch's `_multi_tensor_sgd`, one pass over
//     parameter, gradient and momentum buffer, with `lr`, the momentum (OneCycleLR cycles it on an SGD) and the clip coefficient read from
//     device memory.
// All of them walk a tensor list the same way: a block takes 4096 consecutive elements of one tensor, 64 tensors to a launch (opt_for_batches on
// the host, opt_chunk on the device).
#include <algorithm>
#include <type_traits>

#include "bpx_common.h"

namespace {

constexpr int OPT_CHUNK = 4096, OPT_MAX = 64;
struct OptBatch { bpx_adam_tensor t[OPT_MAX]; int first_chunk[OPT_MAX + 1]; int count; };
struct OptSteps { float* step[256]; int count; };

// The chunk of this block: its tensor (a block-uniform search: tensor k owns chunks [first_chunk[k], first_chunk[k + 1])), the chunk's first element
// `off` and its length `n`.
__device__ __forceinline__ bpx_adam_tensor opt_chunk(const OptBatch& b, int64_t& off, int& n) {
  int lo = 0, hi = b.count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int)blockIdx.x >= b.first_chunk[mid]) lo = mid; else hi = mid;
  }
  const bpx_adam_tensor t = b.t[lo];
  off = (int64_t)((int)blockIdx.x - b.first_chunk[lo]) * OPT_CHUNK;
  n = (int)(t.numel - off < OPT_CHUNK ? t.numel - off : OPT_CHUNK);
  return t;
}

// Sum over the 256 threads of a block in a FIXED order (a tree over thread indices): the result does not depend on scheduling, two runs agree bit
// for bit.  Valid in thread 0.
__device__ __forceinline__ double opt_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  return sh[0];
}

// ------------------------------------------------------------------------------------------------
// Global gradient norm.  Pass 1: one double per 4096-element chunk, sum of g^2 in fp64 (thread t takes elements t, t + 256, ... of the chunk -
// four consecutive ones per turn where the gradient is 16-byte aligned - then the tree above).  Pass 2 (one block): the partials in a fixed order.
// No atomics.  fp64: the order of a sum of n non-negative doubles moves it by at most ~n 2^-53 relative, so only the final rounding to float can
// differ from any other fp64 evaluation.  A NaN gradient gives a NaN norm and a NaN coefficient, as torch does (error_if_nonfinite=False).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) grad_sq_partials_kernel(const OptBatch b, double* __restrict__ partials) {
  __shared__ double sh[256];
  int64_t off;
  int n;
  const float* __restrict__ g = opt_chunk(b, off, n).g + off;
  double acc = 0.0;
  if (((uintptr_t)g & 15) == 0) {
    const int n4 = n >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      const f32x4_t gv = reinterpret_cast<const f32x4_t*>(g)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc += (double)gv[e] * (double)gv[e];
    }
    for (int i = (n4 << 2) + threadIdx.x; i < n; i += 256) acc += (double)g[i] * (double)g[i];
  } else {
    for (int i = threadIdx.x; i < n; i += 256) acc += (double)g[i] * (double)g[i];
  }
  const double s = opt_block_sum(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// out[0] = ||g||_2, out[1] = min(1, max_norm / (out[0] + 1e-6)) - `clip_grad_norm_`'s coefficient.  The comparison (not fminf) keeps a NaN.
__global__ void __launch_bounds__(256) grad_norm_finish_kernel(const double* __restrict__ partials, int64_t n, double max_norm, float* __restrict__ out) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc += partials[i];
  const double s = opt_block_sum(acc, sh);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s);
    const float c = (float)(max_norm / ((double)norm + 1e-6));
    out[0] = norm;
    out[1] = c > 1.0f ? 1.0f : c;
  }
}

int64_t opt_total_chunks(int count, const bpx_adam_tensor* tensors) {
  int64_t chunks = 0;
  for (int k = 0; k < count; ++k) chunks += cdiv64(tensors[k].numel, OPT_CHUNK);
  return chunks;
}

// The launches over a tensor list: `check(k)` for every tensor first (an entry point's own pointer checks; non-zero = refused, nothing launched), then
// `launch(batch, chunks, chunks_done)` for every OPT_MAX tensors that hold at least one chunk.
template <typename Check, typename Launch>
int opt_for_batches(const char* fn, int count, const bpx_adam_tensor* tensors, Check check, Launch launch) {
  BPX_CHECK(count >= 0 && (count == 0 || tensors != nullptr), "%s: bad tensor list", fn);
  for (int k = 0; k < count; ++k)
    if (const int rc = check(k)) return rc;
  int64_t done = 0;
  for (int base = 0; base < count; base += OPT_MAX) {
    OptBatch b{};
    b.count = std::min(OPT_MAX, count - base);
    int64_t chunks = 0;
    for (int k = 0; k < b.count; ++k) {
      b.t[k] = tensors[base + k];
      b.first_chunk[k] = (int)chunks;
      chunks += cdiv64(b.t[k].numel, OPT_CHUNK);
      BPX_CHECK(chunks < (1ll << 30), "%s: too many elements in one launch", fn);
    }
    b.first_chunk[b.count] = (int)chunks;
    if (chunks > 0) launch(b, chunks, done);
    done += chunks;
  }
  return 0;
}

}  // namespace

extern "C" int64_t bpx_grad_norm_workspace(int count, const bpx_adam_tensor* tensors) {
  if (count < 0 || (count > 0 && tensors == nullptr)) return -1;
  for (int k = 0; k < count; ++k)
    if (tensors[k].numel < 0 || tensors[k].numel >= ((int64_t)1 << 40)) return -1;
  return std::max<int64_t>(opt_total_chunks(count, tensors), 1) * (int64_t)sizeof(double);
}

extern "C" int bpx_grad_norm(int count, const bpx_adam_tensor* tensors, double max_norm, void* workspace_d, int64_t workspace_bytes, float* out_d,
                             bpx_stream_t stream) {
  const char* fn = "bpx_grad_norm";
  BPX_CHECK(workspace_d && out_d, "%s: null pointer", fn);
  BPX_CHECK(((uintptr_t)workspace_d & 7) == 0, "%s: the workspace must be 8-byte aligned", fn);
  const int64_t need = bpx_grad_norm_workspace(count, tensors);      // -1: a list that the checks of opt_for_batches refuse below
  BPX_CHECK(need < 0 || workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed", fn, (long long)workspace_bytes, (long long)need);
  hipStream_t s = (hipStream_t)stream;
  double* partials = (double*)workspace_d;
  auto check = [&](int k) {
    BPX_CHECK(tensors[k].numel >= 0 && tensors[k].numel < ((int64_t)1 << 40) && (tensors[k].numel == 0 || tensors[k].g), "%s: tensor %d has a null gradient or a bad size", fn, k);
    return 0;
  };
  if (const int rc = opt_for_batches(fn, count, tensors, check, [&](const OptBatch& b, int64_t chunks, int64_t done) {
        grad_sq_partials_kernel<<<(unsigned)chunks, 256, 0, s>>>(b, partials + done);
      })) return rc;
  grad_norm_finish_kernel<<<1, 256, 0, s>>>(partials, opt_total_chunks(count, tensors), max_norm, out_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Adam / AdamW step over a list of parameter tensors (torch.optim.Adam(W), capturable: `step` is a device float per tensor).
// The math and its order are those of torch's fused kernel (torch/optim/adam.py `_fused_adam` -> fused_adam_utils.cuh):
//   AdamW: p -= lr * wd * p          Adam: g += wd * p
//   m = m + (g - m) * (1 - b1)       v = b2 * v + (1 - b2) * g * g
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps),   t = step + 1
// Why not torch's own launch: its multi-tensor kernel hands one 64 K-element chunk to a 512-thread block - the 6.7 M parameters of cfg 2
// are ~200 blocks on 256 CUs, three launches of 45 us (188 MB of traffic at 1.4 TB/s).  Here a block takes 4096 elements.
// `step` is read by every block of a tensor, so it is incremented by a second (one-block) launch after the update.
// Two hyper-parameters may live on the device (bpx_adam_step_dev):
//   beta1_d  : a DOUBLE (torch holds the betas as host doubles; OneCycleLR's 0.8999999999999999 is not a float), NULL = the host argument;
//   gscale_d : a float the gradient is multiplied by first - a plain fp32 product, what `g.mul_(coef)` of clip_grad_norm_ computes - and the
//              product is stored back to .g (SCALE); without it the gradient is read as it is and .g is not written.
// ------------------------------------------------------------------------------------------------
namespace {

template <bool SCALE>
__global__ void __launch_bounds__(256) adam_multi_kernel(const OptBatch b, const float* __restrict__ lr_d, double lr_h, const double* __restrict__ beta1_d,
                                                         double beta1_h, double beta2, double eps, double wd, int decoupled,
                                                         const float* __restrict__ gscale_d) {
  int64_t off;
  int n;
  const bpx_adam_tensor t = opt_chunk(b, off, n);
  // The types below are those of torch's fused kernel (ATen/native/cuda/fused_adam_utils.cuh): hyper-parameters are DOUBLES (0.999 is not 0.999f:
  // 1 - beta2 differs by 1.3e-5 relative), a double times a float is evaluated in double and rounded to float at the assignment; the bias
  // corrections are computed in double and handed on as floats.
  const double lr = lr_d ? (double)*lr_d : lr_h;
  const double beta1 = beta1_d ? *beta1_d : beta1_h;
  const float gs = SCALE ? *gscale_d : 1.0f;
  const double step = (double)*t.step + 1.0;
  const float bc1 = (float)(1.0 - pow(beta1, step)), bc2s = (float)sqrt(1.0 - pow(beta2, step));
  const float step_size = (float)(lr / (double)bc1);
  const double omb1 = 1.0 - beta1, omb2 = 1.0 - beta2;
  float* __restrict__ p = t.p + off;
  std::conditional_t<SCALE, float, const float>* __restrict__ g = const_cast<float*>(t.g) + off;      // written only when scaled
  float* __restrict__ m = t.m + off;
  float* __restrict__ v = t.v + off;
  auto upd = [&](float& pf, float gf, float& mf, float& vf) {
    if (wd != 0.0) { if (decoupled) pf = (float)((double)pf - lr * wd * (double)pf); else gf = (float)((double)gf + (double)pf * wd); }
    mf = (float)(beta1 * (double)mf + omb1 * (double)gf);
    vf = (float)(beta2 * (double)vf + omb2 * (double)gf * (double)gf);
    const float denom = (float)((double)(sqrtf(vf) / bc2s) + eps);
    pf -= step_size * mf / denom;
  };
  auto one = [&](int i) {
    float gf = g[i];
    if constexpr (SCALE) { gf = gf * gs; g[i] = gf; }
    upd(p[i], gf, m[i], v[i]);
  };
  const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  if (vec) {
    const int n4 = n >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      const f32x4_t pv = reinterpret_cast<f32x4_t*>(p)[i], mv = reinterpret_cast<f32x4_t*>(m)[i], vv = reinterpret_cast<f32x4_t*>(v)[i];
      f32x4_t gv = reinterpret_cast<const f32x4_t*>(g)[i];
      if constexpr (SCALE) {
#pragma unroll
        for (int e = 0; e < 4; ++e) gv[e] = gv[e] * gs;
        reinterpret_cast<f32x4_t*>(g)[i] = gv;
      }
      float pe[4], me[4], ve[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) { pe[e] = pv[e]; me[e] = mv[e]; ve[e] = vv[e]; upd(pe[e], gv[e], me[e], ve[e]); }
      reinterpret_cast<f32x4_t*>(p)[i] = f32x4_t{pe[0], pe[1], pe[2], pe[3]};
      reinterpret_cast<f32x4_t*>(m)[i] = f32x4_t{me[0], me[1], me[2], me[3]};
      reinterpret_cast<f32x4_t*>(v)[i] = f32x4_t{ve[0], ve[1], ve[2], ve[3]};
    }
    for (int i = (n4 << 2) + threadIdx.x; i < n; i += 256) one(i);
  } else {
    for (int i = threadIdx.x; i < n; i += 256) one(i);
  }
}

__global__ void __launch_bounds__(256) adam_step_inc_kernel(const OptSteps s) {
  if ((int)threadIdx.x < s.count) *s.step[threadIdx.x] += 1.f;
}

// step += 1 for every tensor of the list, 256 tensors to a launch
void opt_step_inc(int count, const bpx_adam_tensor* tensors, hipStream_t s) {
  for (int base = 0; base < count; base += 256) {
    OptSteps st{};
    st.count = std::min(256, count - base);
    for (int k = 0; k < st.count; ++k) st.step[k] = tensors[base + k].step;
    adam_step_inc_kernel<<<1, 256, 0, s>>>(st);
  }
}

int opt_adam_step(const char* fn, int count, const bpx_adam_tensor* tensors, const float* lr_d, double lr, const double* beta1_d, double beta1,
                  double beta2, double eps, double weight_decay, int decoupled, const float* gscale_d, hipStream_t s) {
  auto check = [&](int k) {
    BPX_CHECK(tensors[k].p && tensors[k].g && tensors[k].m && tensors[k].v && tensors[k].step && tensors[k].numel >= 0 &&
              tensors[k].numel < ((int64_t)1 << 40), "%s: tensor %d has a null pointer or a bad size", fn, k);
    return 0;
  };
  if (const int rc = opt_for_batches(fn, count, tensors, check, [&](const OptBatch& b, int64_t chunks, int64_t) {
        if (gscale_d) adam_multi_kernel<true><<<(unsigned)chunks, 256, 0, s>>>(b, lr_d, lr, beta1_d, beta1, beta2, eps, weight_decay, decoupled, gscale_d);
        else adam_multi_kernel<false><<<(unsigned)chunks, 256, 0, s>>>(b, lr_d, lr, beta1_d, beta1, beta2, eps, weight_decay, decoupled, nullptr);
      })) return rc;
  opt_step_inc(count, tensors, s);      // after every update launch: the updates read the old step
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

}  // namespace

extern "C" int bpx_adam_step(int count, const bpx_adam_tensor* tensors, const float* lr_d, double lr, double beta1, double beta2, double eps,
                             double weight_decay, int decoupled, bpx_stream_t stream) {
  return opt_adam_step("bpx_adam_step", count, tensors, lr_d, lr, nullptr, beta1, beta2, eps, weight_decay, decoupled, nullptr, (hipStream_t)stream);
}

extern "C" int bpx_adam_step_dev(int count, const bpx_adam_tensor* tensors, const float* lr_d, double lr, const double* beta1_d, double beta1,
                                 double beta2, double eps, double weight_decay, int decoupled, const float* gscale_d, bpx_stream_t stream) {
  const char* fn = "bpx_adam_step_dev";
  BPX_CHECK(((uintptr_t)beta1_d & 7) == 0 && ((uintptr_t)gscale_d & 3) == 0 && ((uintptr_t)lr_d & 3) == 0, "%s: misaligned device scalar", fn);
  return opt_adam_step(fn, count, tensors, lr_d, lr, beta1_d, beta1, beta2, eps, weight_decay, decoupled, gscale_d, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// SGD.  torch's `_multi_tensor_sgd` as ONE pass: every foreach op of it is an fp32 operation with its scalar rounded to float once, and so is
// every line below - products and sums are kept apart (no contraction), so each rounds as the foreach op it stands for:
//   d = g + wd * p                      (WD)
//   b = b * mom;  b = b + (1 - dampening) * d;  u = b        (MODE 1)      u = d + mom * b   (MODE 2, Nesterov)      u = d   (MODE 0: no buffer)
//   p = p + (-lr) * u
// lr_d (float), momentum_d (DOUBLE: the scheduler assigns host doubles; rounded to float here) and gscale_d (float; g = g * gscale first, one fp32
// product, stored back) are read from device memory when not NULL.  No atomics, nothing depends on scheduling.
// ------------------------------------------------------------------------------------------------
namespace {

template <int MODE, bool WD>
__device__ __forceinline__ void sgd_update(float& p, float g, float& b, float nlr, float mom, float omd, float wd) {
#pragma clang fp contract(off)
  float d = g;
  if (WD) { const float t = wd * p; d = g + t; }
  float u = d;
  if (MODE != 0) {
    float bb = b * mom;
    const float t = omd * d;
    bb = bb + t;
    b = bb;
    if (MODE == 2) { const float t2 = mom * bb; u = d + t2; } else u = bb;
  }
  const float t3 = nlr * u;
  p = p + t3;
}

template <int MODE, bool WD>
__global__ void __launch_bounds__(256) sgd_kernel(const OptBatch b, const float* __restrict__ lr_d, float lr_h, const double* __restrict__ mom_d,
                                                  float mom_h, float omd, float wd, const float* __restrict__ gscale_d) {
  int64_t off;
  int n;
  const bpx_adam_tensor t = opt_chunk(b, off, n);
  const float nlr = -(lr_d ? *lr_d : lr_h);
  const float mom = mom_d ? (float)*mom_d : mom_h;
  const bool scale = gscale_d != nullptr;
  const float gs = scale ? *gscale_d : 1.0f;
  float* __restrict__ p = t.p + off;
  float* __restrict__ g = const_cast<float*>(t.g) + off;
  float* __restrict__ m = MODE != 0 ? t.m + off : nullptr;
  auto one = [&](int i) {
    float gf = g[i];
    if (scale) { gf = gf * gs; g[i] = gf; }
    float pf = p[i], bf = 0.f;
    if (MODE != 0) bf = m[i];
    sgd_update<MODE, WD>(pf, gf, bf, nlr, mom, omd, wd);
    p[i] = pf;
    if (MODE != 0) m[i] = bf;
  };
  const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0);
  if (vec) {
    const int n4 = n >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      f32x4_t pv = reinterpret_cast<f32x4_t*>(p)[i], gv = reinterpret_cast<const f32x4_t*>(g)[i], mv = {0.f, 0.f, 0.f, 0.f};
      if (MODE != 0) mv = reinterpret_cast<f32x4_t*>(m)[i];
      if (scale) {
#pragma unroll
        for (int e = 0; e < 4; ++e) gv[e] = gv[e] * gs;
        reinterpret_cast<f32x4_t*>(g)[i] = gv;
      }
      float pe[4], me[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) { pe[e] = pv[e]; me[e] = mv[e]; sgd_update<MODE, WD>(pe[e], gv[e], me[e], nlr, mom, omd, wd); }
      reinterpret_cast<f32x4_t*>(p)[i] = f32x4_t{pe[0], pe[1], pe[2], pe[3]};
      if (MODE != 0) reinterpret_cast<f32x4_t*>(m)[i] = f32x4_t{me[0], me[1], me[2], me[3]};
    }
    for (int i = (n4 << 2) + threadIdx.x; i < n; i += 256) one(i);
  } else {
    for (int i = threadIdx.x; i < n; i += 256) one(i);
  }
}

}  // namespace

extern "C" int bpx_sgd_step(int count, const bpx_adam_tensor* tensors, const float* lr_d, double lr, const double* momentum_d, double momentum,
                            double dampening, double weight_decay, int nesterov, const float* gscale_d, bpx_stream_t stream) {
  const char* fn = "bpx_sgd_step";
  BPX_CHECK(((uintptr_t)momentum_d & 7) == 0 && ((uintptr_t)gscale_d & 3) == 0 && ((uintptr_t)lr_d & 3) == 0, "%s: misaligned device scalar", fn);
  const bool use_mom = momentum_d != nullptr || momentum != 0.0;
  BPX_CHECK(!nesterov || use_mom, "%s: Nesterov momentum needs a momentum", fn);
  auto check = [&](int k) {
    BPX_CHECK(tensors[k].p && tensors[k].g && tensors[k].numel >= 0 && tensors[k].numel < ((int64_t)1 << 40),
              "%s: tensor %d has a null pointer or a bad size", fn, k);
    BPX_CHECK(!use_mom || tensors[k].m, "%s: tensor %d has no momentum buffer, and momentum is in use", fn, k);
    return 0;
  };
  hipStream_t s = (hipStream_t)stream;
  const int mode = !use_mom ? 0 : (nesterov ? 2 : 1);
  const bool has_wd = weight_decay != 0.0;
  const float lr_h = (float)lr, mom_h = (float)momentum, omd = (float)(1.0 - dampening), wd = (float)weight_decay;
  if (const int rc = opt_for_batches(fn, count, tensors, check, [&](const OptBatch& b, int64_t chunks, int64_t) {
#define BPX_SGD_LAUNCH(M, W) sgd_kernel<M, W><<<(unsigned)chunks, 256, 0, s>>>(b, lr_d, lr_h, momentum_d, mom_h, omd, wd, gscale_d)
        switch (mode * 2 + (has_wd ? 1 : 0)) {
          case 0: BPX_SGD_LAUNCH(0, false); break;
          case 1: BPX_SGD_LAUNCH(0, true); break;
          case 2: BPX_SGD_LAUNCH(1, false); break;
          case 3: BPX_SGD_LAUNCH(1, true); break;
          case 4: BPX_SGD_LAUNCH(2, false); break;
          default: BPX_SGD_LAUNCH(2, true); break;
        }
#undef BPX_SGD_LAUNCH
      })) return rc;
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
