// Instance-segmentation training targets on the device (biapy_amd/targets.py states the semantics, include/biapy_amd.h the entry points and their
// arithmetic): from a batch of instance-id patches the channel planes F, C, D, Dc, H, V, Z that InstanceChannelsLoss is trained against.
//
//   bpx_itarget_ids    one launch: float32 / uint8 / int32 values -> sanitised int32 ids (itarget_core.h: it_id_*), the values that are no id
//                      counted into the fault counter (one atomic add per block that met one).
//   (bpx_edt per sample, label mode, float32: the distance d - the caller's launches, edt.hip unchanged)
//   bpx_itarget_stats  init, accumulate, finish and - on request - the rcmax accumulate over the (B, n_max + 1) records.  The accumulate is
//                      label_walk.h's run walk, one wave to a span of 8192 voxels of ONE sample (grid y = the sample): a finished run contributes
//                      regionprops' closed form and the largest d of its voxels, formed by the lane that holds the run's head - serially, L loads
//                      in one lane: itarget_core.h, it_run_max, states the limit at rows of thousands of voxels - and sent once.  The
//                      block's four waves first meet in a table of RP_LOCAL_SLOTS = 256 records keyed by id in LDS (regionprops_core.h's sizing: 60
//                      bytes a slot here, 15 368 bytes, ten blocks per CU by LDS where the 32 waves of a CU allow eight; the rcmax pass keeps keys and one maximum: 2 052 bytes), flushed once per occupied
//                      slot; an id the table does not take (more than 128 ids in a block, 16 probes) goes to its global row directly - the same
//                      bits, since every field is reached by integer add / min / max only.  The finish turns sums into centroids.  The rcmax pass
//                      is the same walk: rc is largest at an end of a run (it_run_rc_max), two evaluations and one maximum per run.
//   bpx_itarget_pack   one launch, a thread to 4 consecutive voxels of a sample: ids, the neighbours' ids for the contour, d and the instance's
//                      record in; per channel one 16-byte store where the plane's address allows it, 4-byte stores otherwise (the planes of a
//                      sample whose voxel count is no multiple of 4, the last voxels of a sample).  Offsets into the target are 64-bit.  No LDS.
// Nothing is read back; every launch is fixed by the arguments: capturable.  Every loop is bounded by a launch parameter or a constant.
#include <type_traits>

#include "bpx_common.h"
#include "itarget_core.h"
#include "label_walk.h"

namespace {

struct ItDev {     // the global records, the atomics at the memory side
  unsigned* area_p;
  unsigned long long* sums_p;
  int* box_p;
  unsigned* max_p[2];
  __device__ __forceinline__ void area(uint32_t r, uint32_t c) const { __hip_atomic_fetch_add(area_p + r, c, LW_RLX_AGENT); }
  __device__ __forceinline__ void sum(uint32_t r, int k, uint64_t v) const {
    __hip_atomic_fetch_add(sums_p + (int64_t)r * 3 + k, (unsigned long long)v, LW_RLX_AGENT);
  }
  __device__ __forceinline__ void lo(uint32_t r, int k, int32_t v) const { __hip_atomic_fetch_min(box_p + (int64_t)r * 6 + k, v, LW_RLX_AGENT); }
  __device__ __forceinline__ void hi(uint32_t r, int k, int32_t v) const { __hip_atomic_fetch_max(box_p + (int64_t)r * 6 + 3 + k, v, LW_RLX_AGENT); }
  __device__ __forceinline__ void umax(uint32_t r, int k, uint32_t v) const { __hip_atomic_fetch_max(max_p[k] + r, v, LW_RLX_AGENT); }
};

struct ItLds : LwKeysLds {     // the block's table in LDS
  unsigned* area_p;
  unsigned long long* sums_p;
  int* box_p;
  unsigned* max_p;             // one maximum per slot: dmax in the accumulate, rcmax in the rcmax pass
  __device__ __forceinline__ void area(uint32_t s, uint32_t c) const { __hip_atomic_fetch_add(area_p + s, c, LW_RLX_WG); }
  __device__ __forceinline__ void sum(uint32_t s, int k, uint64_t v) const { __hip_atomic_fetch_add(sums_p + s * 3 + k, (unsigned long long)v, LW_RLX_WG); }
  __device__ __forceinline__ void lo(uint32_t s, int k, int32_t v) const { __hip_atomic_fetch_min(box_p + s * 6 + k, v, LW_RLX_WG); }
  __device__ __forceinline__ void hi(uint32_t s, int k, int32_t v) const { __hip_atomic_fetch_max(box_p + s * 6 + 3 + k, v, LW_RLX_WG); }
  __device__ __forceinline__ void umax(uint32_t s, int, uint32_t v) const { __hip_atomic_fetch_max(max_p + s, v, LW_RLX_WG); }
  __device__ __forceinline__ uint32_t area_of(uint32_t s) const { return area_p[s]; }
  __device__ __forceinline__ uint64_t sum_of(uint32_t s, int k) const { return sums_p[s * 3 + k]; }
  __device__ __forceinline__ int32_t lo_of(uint32_t s, int k) const { return box_p[s * 6 + k]; }
  __device__ __forceinline__ int32_t hi_of(uint32_t s, int k) const { return box_p[s * 6 + 3 + k]; }
  __device__ __forceinline__ uint32_t umax_of(uint32_t s, int) const { return max_p[s]; }
};

// where the fields of `rows` records lie in one 8-byte aligned allocation of it_record_bytes(rows): sums, area, box, dmax, rcmax
int64_t it_record_bytes(int64_t rows) { return rows * 60 + ((rows * 60) & 4); }
ItDev it_records(void* rec, int64_t rows) {
  char* p = static_cast<char*>(rec);
  return ItDev{reinterpret_cast<unsigned*>(p + rows * 24), reinterpret_cast<unsigned long long*>(p), reinterpret_cast<int*>(p + rows * 28),
               {reinterpret_cast<unsigned*>(p + rows * 52), reinterpret_cast<unsigned*>(p + rows * 56)}};
}

// ---- ids ------------------------------------------------------------------------------------------------------------------------------------------
// thread t takes the values t, t + T ...  LOOP BOUND: ceil(n / T) trips, fixed by the launch.  The block's faults meet in one counter in LDS.
template <typename T>
__global__ void __launch_bounds__(256) it_ids_kernel(const T* __restrict__ t, int64_t n, int n_max, int* __restrict__ ids, int* __restrict__ faults) {
  __shared__ unsigned block_faults;
  if (threadIdx.x == 0) block_faults = 0;
  __syncthreads();
  unsigned mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    uint32_t fault;
    if constexpr (sizeof(T) == 4 && !std::is_integral<T>::value) ids[i] = it_id_f32(t[i], n_max, fault);
    else ids[i] = it_id_i32((int32_t)t[i], n_max, fault);
    mine += fault;
  }
  if (mine) __hip_atomic_fetch_add(&block_faults, mine, LW_RLX_WG);
  __syncthreads();
  if (threadIdx.x == 0 && block_faults) __hip_atomic_fetch_add(faults, (int)block_faults, LW_RLX_AGENT);
}

// ---- the records ----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) it_init_kernel(ItDev m, int64_t rows) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256)
    it_init_row(m.area_p + r, reinterpret_cast<uint64_t*>(m.sums_p) + r * 3, m.box_p + r * 6, m.max_p[0] + r, m.max_p[1] + r);
}
__global__ void __launch_bounds__(256) it_finish_kernel(ItDev m, int64_t rows) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256)
    it_finish_row(m.area_p + r, reinterpret_cast<uint64_t*>(m.sums_p) + r * 3, m.box_p + r * 6);
}

// accumulate (RC == false) and the rcmax pass (RC == true): block (x, b), wave w of the block owns the voxels [span * OVL_SPAN, + OVL_SPAN) below n
// of sample b and walks their runs (label_walk.h: lw_walk_runs, 32 trips).  LOOP BOUND: the clear and the flush of the block's table
// RP_LOCAL_SLOTS / 256 = 1 trip.  Every wave reaches both barriers, with or without voxels.
template <bool RC>
__global__ void __launch_bounds__(64 * OVL_WAVES) it_accumulate_kernel(ItDev m, const int* __restrict__ ids, const uint32_t* __restrict__ dist, int64_t n, int Y,
                                                                       int X, int n_max, RpStride stride, double sz, double sy, double sx) {
  __shared__ int lkeys[RP_LOCAL_SLOTS];
  __shared__ unsigned larea[RC ? 1 : RP_LOCAL_SLOTS];
  __shared__ unsigned long long lsums[RC ? 1 : RP_LOCAL_SLOTS * 3];
  __shared__ int lbox[RC ? 1 : RP_LOCAL_SLOTS * 6];
  __shared__ unsigned lmax[RP_LOCAL_SLOTS];
  __shared__ unsigned lclaimed;
  const ItLds loc{{lkeys, &lclaimed}, larea, lsums, lbox, lmax};
  for (int s = threadIdx.x; s < RP_LOCAL_SLOTS; s += 64 * OVL_WAVES) {
    lkeys[s] = 0;
    lmax[s] = 0;
    if constexpr (!RC) {
      larea[s] = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) { lsums[s * 3 + k] = 0; lbox[s * 6 + k] = RP_LO_INIT; lbox[s * 6 + 3 + k] = RP_HI_INIT; }
    }
  }
  if (threadIdx.x == 0) lclaimed = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const uint32_t base = blockIdx.y * (uint32_t)(n_max + 1);
  const int* labels = ids + (int64_t)blockIdx.y * n;
  const uint32_t* d = dist + (int64_t)blockIdx.y * n;
  const int64_t begin = ((int64_t)blockIdx.x * OVL_WAVES + (threadIdx.x >> 6)) * OVL_SPAN;
  if (begin < n) {                                                      // the whole wave
    const int64_t end = begin + OVL_SPAN < n ? begin + OVL_SPAN : n;
    const double s3[3] = {sz, sy, sx};
    lw_walk_runs(labels, begin, end, lane, Y, X, n_max, stride, [&](int32_t label, int32_t z, int32_t y, int32_t x0, uint32_t L) {
      if constexpr (RC) {
        const uint64_t* cp = reinterpret_cast<const uint64_t*>(m.sums_p) + (int64_t)(base + (uint32_t)label) * 3;
        const double c[3] = {it_double(cp[0]), it_double(cp[1]), it_double(cp[2])};
        it_emit_rc(loc, m, base, label, it_run_rc_max(c, z, y, x0, L, s3));
      } else {
        it_emit(loc, m, base, label, z, y, x0, L, it_run_max(d + ((int64_t)z * Y + y) * X + x0, L));
      }
    });
  }
  __syncthreads();
  for (int s = threadIdx.x; s < RP_LOCAL_SLOTS; s += 64 * OVL_WAVES) {   // the flush: every id of the block once
    if constexpr (RC) it_merge_rc(loc, (uint32_t)s, m, base);
    else it_merge(loc, (uint32_t)s, m, base);
  }
}

// ---- pack -----------------------------------------------------------------------------------------------------------------------------------------
// block (x, b): thread g of the grid's x takes the voxels 4 g .. 4 g + 3 of sample b.  LOOP BOUND: the channels, at most 8; it_differs 27.
__global__ void __launch_bounds__(256) it_pack_kernel(const int* __restrict__ ids, const float* __restrict__ dist, ItRecords rec, int Z, int Y, int X, int n_max,
                                                      ItPack p, float* __restrict__ target) {
  const int64_t V = (int64_t)Z * Y * X;
  const int64_t v0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (v0 >= V) return;
  const int b = blockIdx.y;
  const int* sid = ids + (int64_t)b * V;
  const float* sd = dist + (int64_t)b * V;
  const uint32_t base = (uint32_t)b * (uint32_t)(n_max + 1);
  const bool contour = it_needs_contour(p);
  const bool want_d = it_has(p.codes, p.channels, IT_D);
  int32_t l[4];
  float d[4];
  bool edge[4];
  RpPos pos[4];
  pos[0] = rp_pos_of((uint32_t)v0, Y, X);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool in = v0 + e < V;
    if (e) { pos[e] = pos[e - 1]; rp_step(pos[e], Y, X); }
    l[e] = in ? rp_label(sid[v0 + e], n_max) : 0;                 // ids of bpx_itarget_ids lie in 0..n_max already: the row index stays in range whatever comes
    d[e] = in && want_d ? sd[v0 + e] : 0.f;
    edge[e] = in && contour ? it_differs(sid, Z, Y, X, pos[e].z, pos[e].y, pos[e].x, p.ndim, p.conn, l[e]) : false;
  }
  for (int c = 0; c < p.channels; ++c) {
    const int code = it_code(p.codes, c);
    float* plane = target + ((int64_t)b * p.channels + c) * V + v0;
    float val[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) val[e] = it_value(code, p, rec, base + (uint32_t)l[e], l[e], edge[e], d[e], pos[e].z, pos[e].y, pos[e].x);
    if (v0 + 4 <= V && ((uintptr_t)plane & 15) == 0) {
      *reinterpret_cast<f32x4_t*>(plane) = f32x4_t{val[0], val[1], val[2], val[3]};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (v0 + e < V) plane[e] = val[e];
    }
  }
}

bool spans_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

// the refusals the stats and the pack pass share, in the order of include/biapy_amd.h: extents, the voxel count, B, n_max
int it_check_batch(const char* fn, int B, int Z, int Y, int X, int n_max) {
  BPX_CHECK(Z >= 1 && Y >= 1 && X >= 1, "%s: extents must be at least 1 (got %d x %d x %d)", fn, Z, Y, X);
  const int64_t n = (int64_t)Z * Y * X;
  BPX_CHECK(n < ((int64_t)1 << 31), "%s: %lld voxels in a sample: 2^31 or more are not supported", fn, (long long)n);
  BPX_CHECK(B >= 1 && B <= 65535, "%s: 1 to 65535 samples (got %d)", fn, B);
  BPX_CHECK(n_max >= 0 && n_max < IT_ID_LIMIT, "%s: n_max must be in [0, 2^24) (got %d)", fn, n_max);
  BPX_CHECK((int64_t)B * ((int64_t)n_max + 1) < ((int64_t)1 << 31), "%s: B * (n_max + 1) = %lld records: 2^31 or more are not supported", fn,
            (long long)B * ((long long)n_max + 1));
  return 0;
}
int it_check_sampling(const char* fn, const double* sampling) {
  if (sampling)
    for (int a = 0; a < 3; ++a) BPX_CHECK(isfinite(sampling[a]) && sampling[a] > 0.0, "%s: sampling must be positive and finite (axis %d)", fn, a);
  return 0;
}

}  // namespace

extern "C" int64_t bpx_itarget_records_bytes(int B, int n_max) {
  const char* fn = "bpx_itarget_records_bytes";
  if (it_check_batch(fn, B, 1, 1, 1, n_max)) return -1;
  return it_record_bytes((int64_t)B * ((int64_t)n_max + 1));
}

extern "C" int bpx_itarget_ids(const void* t_d, int dtype, int64_t n, int n_max, int32_t* ids_d, int32_t* faults_d, bpx_stream_t stream) {
  const char* fn = "bpx_itarget_ids";
  BPX_CHECK(t_d && ids_d && faults_d, "%s: null pointer", fn);
  BPX_CHECK(n >= 1, "%s: the value count must be at least 1 (got %lld)", fn, (long long)n);
  BPX_CHECK(n_max >= 0 && n_max < IT_ID_LIMIT, "%s: n_max must be in [0, 2^24) (got %d)", fn, n_max);
  BPX_CHECK(dtype == BPX_F32 || dtype == BPX_U8 || dtype == BPX_I32, "%s: values must be float32, uint8 or int32 (dtype %d)", fn, dtype);
  BPX_CHECK((((uintptr_t)ids_d | (uintptr_t)faults_d) & 3) == 0 && (dtype == BPX_U8 || ((uintptr_t)t_d & 3) == 0),
            "%s: ids, the fault counter and 4-byte values must be 4-byte aligned", fn);
  BPX_CHECK(!spans_overlap(t_d, n * (dtype == BPX_U8 ? 1 : 4), ids_d, n * 4), "%s: the ids overlap the values", fn);
  hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)(cdiv64(n, 1024) < 8192 ? cdiv64(n, 1024) : 8192);
  if (dtype == BPX_F32) it_ids_kernel<float><<<blocks, 256, 0, s>>>(static_cast<const float*>(t_d), n, n_max, ids_d, faults_d);
  else if (dtype == BPX_U8) it_ids_kernel<uint8_t><<<blocks, 256, 0, s>>>(static_cast<const uint8_t*>(t_d), n, n_max, ids_d, faults_d);
  else it_ids_kernel<int32_t><<<blocks, 256, 0, s>>>(static_cast<const int32_t*>(t_d), n, n_max, ids_d, faults_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_itarget_stats(const int32_t* ids_d, const float* dist_d, int B, int Z, int Y, int X, int n_max, const double* sampling, int want_rc,
                                 void* records_d, bpx_stream_t stream) {
  const char* fn = "bpx_itarget_stats";
  BPX_CHECK(ids_d && dist_d && records_d, "%s: null pointer", fn);
  if (it_check_batch(fn, B, Z, Y, X, n_max) || it_check_sampling(fn, sampling)) return 1;
  BPX_CHECK((((uintptr_t)ids_d | (uintptr_t)dist_d) & 3) == 0 && ((uintptr_t)records_d & 7) == 0,
            "%s: ids and distances must be 4-byte aligned, the records 8-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)Z * Y * X, rows = (int64_t)B * ((int64_t)n_max + 1);
  const ItDev m = it_records(records_d, rows);
  const dim3 grid(lw_span_blocks(n), (unsigned)B);
  const double sz = sampling ? sampling[0] : 1.0, sy = sampling ? sampling[1] : 1.0, sx = sampling ? sampling[2] : 1.0;
  const uint32_t* dbits = reinterpret_cast<const uint32_t*>(dist_d);
  it_init_kernel<<<lw_rows_grid(rows), 256, 0, s>>>(m, rows);
  it_accumulate_kernel<false><<<grid, 64 * OVL_WAVES, 0, s>>>(m, ids_d, dbits, n, Y, X, n_max, rp_stride(Y, X), sz, sy, sx);
  it_finish_kernel<<<lw_rows_grid(rows), 256, 0, s>>>(m, rows);
  if (want_rc) it_accumulate_kernel<true><<<grid, 64 * OVL_WAVES, 0, s>>>(m, ids_d, dbits, n, Y, X, n_max, rp_stride(Y, X), sz, sy, sx);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int bpx_itarget_pack(const int32_t* ids_d, const float* dist_d, const void* records_d, int B, int Z, int Y, int X, int n_max, uint32_t codes,
                                int channels, int ndim, int connectivity, int mode, int flags, float d_clip, const double* sampling, float* target_d,
                                bpx_stream_t stream) {
  const char* fn = "bpx_itarget_pack";
  BPX_CHECK(ids_d && dist_d && records_d && target_d, "%s: null pointer", fn);
  if (it_check_batch(fn, B, Z, Y, X, n_max)) return 1;
  BPX_CHECK(channels >= 1 && channels <= IT_MAX_CHANNELS, "%s: 1..%d channels (got %d)", fn, IT_MAX_CHANNELS, channels);
  BPX_CHECK(ndim == 3 || (ndim == 2 && Z == 1), "%s: ndim must be 3, or 2 with Z = 1 (got ndim %d, Z %d)", fn, ndim, Z);
  for (int c = 0; c < channels; ++c) {
    const int code = it_code(codes, c);
    BPX_CHECK(code >= IT_F && code <= IT_Z, "%s: unknown channel code %d at channel %d", fn, code, c);
    BPX_CHECK(code != IT_Z || ndim == 3, "%s: the channel code Z at channel %d needs 3-D samples", fn, c);
  }
  BPX_CHECK(channels == IT_MAX_CHANNELS || (codes >> (4 * channels)) == 0, "%s: channel codes past the %d channels", fn, channels);
  BPX_CHECK(connectivity >= 1 && connectivity <= ndim, "%s: connectivity must be in 1..%d (got %d)", fn, ndim, connectivity);
  BPX_CHECK(mode == IT_MODE_THICK || mode == IT_MODE_INNER, "%s: unknown contour mode %d", fn, mode);
  BPX_CHECK(flags >= 0 && flags < 8 && (!(flags & IT_FLAG_D_CLIP) || (flags & IT_FLAG_D_RAW)), "%s: bad flags %d", fn, flags);
  BPX_CHECK(!(flags & IT_FLAG_D_CLIP) || d_clip >= 0.f, "%s: d_clip must be a number >= 0", fn);
  if (it_check_sampling(fn, sampling)) return 1;
  BPX_CHECK((((uintptr_t)ids_d | (uintptr_t)dist_d | (uintptr_t)target_d) & 3) == 0 && ((uintptr_t)records_d & 7) == 0,
            "%s: ids, distances and target must be 4-byte aligned, the records 8-byte aligned", fn);
  const int64_t n = (int64_t)Z * Y * X, rows = (int64_t)B * ((int64_t)n_max + 1);
  BPX_CHECK(!spans_overlap(target_d, (int64_t)B * channels * n * 4, ids_d, (int64_t)B * n * 4) &&
                !spans_overlap(target_d, (int64_t)B * channels * n * 4, dist_d, (int64_t)B * n * 4) &&
                !spans_overlap(target_d, (int64_t)B * channels * n * 4, records_d, it_record_bytes(rows)),
            "%s: the target overlaps an input", fn);
  const ItDev m = it_records(const_cast<void*>(records_d), rows);
  const ItRecords rec{reinterpret_cast<const uint64_t*>(m.sums_p), m.box_p, m.max_p[0], m.max_p[1]};
  ItPack p{codes, channels, ndim, connectivity, mode, flags, (flags & IT_FLAG_D_CLIP) ? d_clip : 0.f,
           {sampling ? sampling[0] : 1.0, sampling ? sampling[1] : 1.0, sampling ? sampling[2] : 1.0}};
  const dim3 grid((unsigned)cdiv64(n, 1024), (unsigned)B);
  it_pack_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(ids_d, dist_d, rec, Z, Y, X, n_max, p, target_d);
  BPX_LAUNCH_CHECK(fn);
  return 0;
}
