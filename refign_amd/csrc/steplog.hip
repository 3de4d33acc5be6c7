// refign_amd/csrc/steplog.hip -- the device side of the step log (refign_amd/steplog.py): what a training step wants to keep a
// record of -- its losses, the loss scale, the found-inf flag, the gradient norms per optimizer group -- already lives on the
// device when the step ends.  Two entry points put it into one row of fp64 values of a device ring buffer, from where a copy
// engine takes it to pinned host memory; the step never waits for the device.
//
//   steplog_gather_kernel   up to 32 device scalars of mixed dtype (f32, bf16, f16, f64, i32) -> fp64 (exact for each of them),
//                           one lane per value, one launch: a torch.stack of casts would be one ATen launch per value.  The
//                           table of pointers and dtype codes travels in the kernel arguments.
//   grad_sqnorm_chunk_kernel / grad_sqnorm_groups_kernel
//                           sum of squares of a flat fp32 buffer per parameter group in one pass over the buffer.  The host
//                           describes the buffer as chunks (offset, length, group), none crossing a group boundary.  Stage one:
//                           one workgroup per chunk, 16-byte loads, squares and sums in fp64 (the square of an fp32 is exact in
//                           fp64), wave shuffle + LDS reduction, one fp64 partial per chunk, plain store.  Stage two: one
//                           workgroup adds each group's partials in chunk order and writes G sums and the count of non-finite
//                           partials.  No floating-point atomics: the result does not depend on arrival order, two launches give
//                           the same bits, and the entry point is legal in deterministic mode.
//                           Bound by HBM reads (343 MB for the bench model's buffer).
//   amp_unscale_sqnorm_chunk_kernel, grad_clip_coef_kernel, grad_scale_kernel, grad_clamp_kernel
//                           gradient clipping decided and applied on the device (described where they stand, below).
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace rfn {

constexpr int kSlMaxScalars = 32;
constexpr int kSlMaxGroups = 32;

struct SlTable {
  const void* p[kSlMaxScalars];
  int dt[kSlMaxScalars];
};

// dtype codes: 0 f32, 1 bf16, 2 f16 (the ABI's activation codes), 3 f64, 4 i32
__global__ __launch_bounds__(64) void steplog_gather_kernel(SlTable t, int n, double* __restrict__ row) {
  const int i = threadIdx.x;
  if (i >= n) return;
  const void* p = t.p[i];
  double v;
  switch (t.dt[i]) {
    case 0: v = (double)*(const float*)p; break;
    case 1: v = (double)(float)*(const __bf16*)p; break;
    case 2: v = (double)(float)*(const _Float16*)p; break;
    case 3: v = *(const double*)p; break;
    default: v = (double)*(const int*)p; break;
  }
  row[i] = v;
}

struct SlChunk {
  long off, len, group;
};

__device__ __forceinline__ double sl_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ bool sl_chunk_ok(const SlChunk& c, long n, int G) {
  return c.off >= 0 && c.len >= 0 && c.len <= n && c.off <= n - c.len && c.group >= 0 && c.group < G;
}

// The body of stage one, one workgroup per chunk: -> the chunk's fp64 sum of squares in thread 0 (every thread must call it).
// Unscale = false: reads only.  Unscale = true (the fp16 recipe's unscale and the norm in one pass): every element is checked
// for inf / NaN as it stands (`bad`), multiplied by `inv` in fp32 and stored, and the square taken is the stored value's -- the
// same loads, products and order of additions as amp_unscale_kernel (csrc/reduce.hip) followed by the read-only form.
template <bool Unscale, typename T>
__device__ __forceinline__ double sl_chunk_sqsum(T* __restrict__ p, long off, long len, float inv, bool& bad) {
  __shared__ double wsum[4];
  const int tid = threadIdx.x;
  auto take = [&](float v) {
    if constexpr (Unscale) {
      bad |= !isfinite(v);
      v *= inv;
    }
    return v;
  };
  // scalar head up to the next 16-byte boundary (the buffer itself is 16-byte aligned), float4 body, scalar tail
  const long head = min(len, (long)((4 - (off & 3)) & 3));
  const long n4 = (len - head) >> 2, tail0 = head + 4 * n4;
  double a0 = 0.0, a1 = 0.0;
  if (tid < head) {
    const float f = take(p[tid]);
    if constexpr (Unscale) p[tid] = f;
    const double v = (double)f;
    a0 = v * v;
  }
  auto* p4 = reinterpret_cast<std::conditional_t<Unscale, float4, const float4>*>(p + head);
#pragma unroll 4
  for (long i = tid; i < n4; i += 256) {
    float4 v = p4[i];
    v.x = take(v.x); v.y = take(v.y); v.z = take(v.z); v.w = take(v.w);
    if constexpr (Unscale) p4[i] = v;
    const double x = (double)v.x, y = (double)v.y, z = (double)v.z, w = (double)v.w;
    a0 = fma(x, x, a0);
    a1 = fma(y, y, a1);
    a0 = fma(z, z, a0);
    a1 = fma(w, w, a1);
  }
  if (tail0 + tid < len) {
    const float f = take(p[tail0 + tid]);
    if constexpr (Unscale) p[tail0 + tid] = f;
    const double v = (double)f;
    a1 = fma(v, v, a1);
  }
  const double s = sl_wave_sum(a0 + a1);
  if ((tid & 63) == 0) wsum[tid >> 6] = s;
  __syncthreads();
  return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one workgroup per chunk.  A chunk that does not lie inside [0, n) or names no group reads nothing and leaves a NaN partial
// (counted by stage two): a damaged table cannot make the kernel read out of bounds.
__global__ __launch_bounds__(256) void grad_sqnorm_chunk_kernel(const float* __restrict__ g, long n,
                                                                const SlChunk* __restrict__ chunks, int G,
                                                                double* __restrict__ partials) {
  const SlChunk c = chunks[blockIdx.x];
  if (!sl_chunk_ok(c, n, G)) {
    if (threadIdx.x == 0) partials[blockIdx.x] = __builtin_nan("");
    return;
  }
  bool bad = false;
  const double s = sl_chunk_sqsum<false>(g + c.off, c.off, c.len, 1.f, bad);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// The same with the unscale: g *= 1 / scale inside the chunks (what lies between them -- the zero-filled alignment gaps -- is
// not touched; a chunk the table describes wrongly is neither read nor written), found_inf = 1 if an element was inf / NaN.
__global__ __launch_bounds__(256) void amp_unscale_sqnorm_chunk_kernel(float* __restrict__ g, long n,
                                                                       const SlChunk* __restrict__ chunks, int G,
                                                                       const float* __restrict__ scale,
                                                                       float* __restrict__ found_inf,
                                                                       double* __restrict__ partials) {
  const SlChunk c = chunks[blockIdx.x];
  if (!sl_chunk_ok(c, n, G)) {
    if (threadIdx.x == 0) partials[blockIdx.x] = __builtin_nan("");
    return;
  }
  const float inv = (float)(1.0 / (double)*scale);
  bool bad = false;
  const double s = sl_chunk_sqsum<true>(g + c.off, c.off, c.len, inv, bad);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
  if (__any(bad) && (threadIdx.x & 63) == 0) *found_inf = 1.f;   // every writer writes the same value
}

// one workgroup: tiles of 256 partials go through LDS, lane g (< G) adds the partials of group g in chunk order (a partial of
// another group is added as +0.0, which changes nothing: the sums are non-negative).  out[0 .. G-1] <- sums, out[G] <- the
// number of non-finite partials.
__global__ __launch_bounds__(256) void grad_sqnorm_groups_kernel(const double* __restrict__ partials,
                                                                 const SlChunk* __restrict__ chunks, int nchunks, int G,
                                                                 double* __restrict__ out) {
  __shared__ double sp[256];
  __shared__ int sg[256];
  __shared__ int sbad;
  const int tid = threadIdx.x;
  if (tid == 0) sbad = 0;
  double acc = 0.0;
  int bad = 0;
  for (int base = 0; base < nchunks; base += 256) {
    __syncthreads();
    const int c = base + tid;
    double v = 0.0;
    int grp = -1;
    if (c < nchunks) {
      v = partials[c];
      const long gl = chunks[c].group;
      grp = gl >= 0 && gl < G ? (int)gl : -1;
      bad += isfinite(v) ? 0 : 1;
    }
    sp[tid] = v;
    sg[tid] = grp;
    __syncthreads();
    if (tid < G) {
      const int m = min(256, nchunks - base);
#pragma unroll 8
      for (int k = 0; k < m; ++k) acc += sg[k] == tid ? sp[k] : 0.0;
    }
  }
  if (bad) atomicAdd(&sbad, bad);                       // integer: the count does not depend on the order
  __syncthreads();
  if (tid < G) out[tid] = acc;
  if (tid == 0) out[G] = (double)sbad;
}

// Gradient clipping (Trainer(gradient_clip_val=...), refign_amd/steplog.py): the decision and the scaling on the device.
//   grad_clip_coef_kernel  torch.nn.utils.clip_grad_norm_'s coefficient from the G group sums of stage two, in fp64
//   grad_scale_kernel      g *= *coef; every workgroup returns at once when *coef == 1 (the product would change no bit)
//   grad_clamp_kernel      clip_grad_value_: comparisons, not fminf / fmaxf, so that a NaN stays a NaN
// The two streaming kernels are amp_unscale_kernel's shape (csrc/reduce.hip): float4 over the 256-byte aligned flat buffer,
// scalar tail, grid-stride loop.
__global__ __launch_bounds__(64) void grad_clip_coef_kernel(const double* __restrict__ sqnorms, int G, float max_norm,
                                                            float* __restrict__ coef) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += sqnorms[g];
  const double total = sqrt(s);
  const double c = (double)max_norm / (total + 1e-6);     // NaN norm -> NaN (c > 1 is false), infinite norm -> 0
  coef[0] = (float)(c > 1.0 ? 1.0 : c);
  coef[1] = (float)total;
}

__global__ __launch_bounds__(256) void grad_scale_kernel(float* __restrict__ g, long n, const float* __restrict__ coef) {
  const float c = *coef;
  if (c == 1.0f) return;
  const long n4 = n >> 2, stride = (long)gridDim.x * 256;
  float4* g4 = reinterpret_cast<float4*>(g);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 v = g4[i];
    v.x *= c; v.y *= c; v.z *= c; v.w *= c;
    g4[i] = v;
  }
  for (long i = 4 * n4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) g[i] *= c;
}

__device__ __forceinline__ float sl_clamp(float v, float lim) { return v < -lim ? -lim : (v > lim ? lim : v); }

__global__ __launch_bounds__(256) void grad_clamp_kernel(float* __restrict__ g, long n, float lim) {
  const long n4 = n >> 2, stride = (long)gridDim.x * 256;
  float4* g4 = reinterpret_cast<float4*>(g);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 v = g4[i];
    v.x = sl_clamp(v.x, lim); v.y = sl_clamp(v.y, lim); v.z = sl_clamp(v.z, lim); v.w = sl_clamp(v.w, lim);
    g4[i] = v;
  }
  for (long i = 4 * n4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) g[i] = sl_clamp(g[i], lim);
}

static int sl_stream_grid(long n) { return (int)std::min<long>(std::max<long>(1, cdiv(n, 4 * 256)), 256L * 8); }

}  // namespace rfn

extern "C" {
using namespace rfn;

// see include/refign_hip.h
int rfn_steplog_gather(const void* const* ptrs, const int* dtypes, int n, double* row, rfn_stream_t stream) {
  RFN_REQUIRE(ptrs && dtypes && row, "steplog_gather: null pointer");
  RFN_REQUIRE(n > 0 && n <= kSlMaxScalars, "steplog_gather: %d values (1 ... %d)", n, kSlMaxScalars);
  SlTable t{};
  for (int i = 0; i < n; ++i) {
    RFN_REQUIRE(ptrs[i] != nullptr, "steplog_gather: value %d is a null pointer", i);
    RFN_REQUIRE(dtypes[i] >= 0 && dtypes[i] <= 4,
                "steplog_gather: value %d has dtype code %d (0 = f32, 1 = bf16, 2 = f16, 3 = f64, 4 = i32)", i, dtypes[i]);
    static const size_t kAlign[5] = {4, 2, 2, 8, 4};
    RFN_REQUIRE(((size_t)ptrs[i] & (kAlign[dtypes[i]] - 1)) == 0, "steplog_gather: value %d is not aligned to its dtype", i);
    t.p[i] = ptrs[i];
    t.dt[i] = dtypes[i];
  }
  RFN_REQUIRE(((size_t)row & 7) == 0, "steplog_gather: row is not 8-byte aligned");
  hipLaunchKernelGGL(steplog_gather_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, t, n, row);
  return check_launch("steplog_gather_kernel");
}

// the argument checks the two chunked entry points share
static int sl_check_chunked(const char* what, const void* flat, long n, const void* chunks, int nchunks, int ngroups,
                            const void* partials, const void* out) {
  RFN_REQUIRE(flat && chunks && partials && out, "%s: null pointer", what);
  RFN_REQUIRE(n > 0 && nchunks > 0 && nchunks <= (1 << 22), "%s: n=%ld nchunks=%d (1 ... 2^22)", what, n, nchunks);
  RFN_REQUIRE(ngroups > 0 && ngroups <= kSlMaxGroups, "%s: %d groups (1 ... %d)", what, ngroups, kSlMaxGroups);
  RFN_REQUIRE(((size_t)flat & 15) == 0 && ((size_t)chunks & 7) == 0 && ((size_t)partials & 7) == 0 && ((size_t)out & 7) == 0,
              "%s: flat must be 16-byte aligned, chunks / partials / out 8-byte aligned", what);
  return RFN_OK;
}

static int sl_launch_groups(const double* partials, const long* chunks, int nchunks, int ngroups, double* out, hipStream_t s) {
  hipLaunchKernelGGL(grad_sqnorm_groups_kernel, dim3(1), dim3(256), 0, s, partials, (const SlChunk*)chunks, nchunks, ngroups, out);
  return check_launch("grad_sqnorm_groups_kernel");
}

int rfn_grad_sqnorm_groups(const float* flat, long n, const long* chunks, int nchunks, int ngroups, double* partials,
                           double* out, rfn_stream_t stream) {
  int rc = sl_check_chunked("grad_sqnorm_groups", flat, n, chunks, nchunks, ngroups, partials, out);
  if (rc != RFN_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_sqnorm_chunk_kernel, dim3(nchunks), dim3(256), 0, s, flat, n, (const SlChunk*)chunks, ngroups, partials);
  rc = check_launch("grad_sqnorm_chunk_kernel");
  if (rc != RFN_OK) return rc;
  return sl_launch_groups(partials, chunks, nchunks, ngroups, out, s);
}

int rfn_amp_unscale_sqnorm_groups_f32(float* grads, long n, const long* chunks, int nchunks, int ngroups, const float* scale,
                                      float* found_inf, double* partials, double* out, rfn_stream_t stream) {
  int rc = sl_check_chunked("amp_unscale_sqnorm_groups_f32", grads, n, chunks, nchunks, ngroups, partials, out);
  if (rc != RFN_OK) return rc;
  RFN_REQUIRE(scale && found_inf, "amp_unscale_sqnorm_groups_f32: null pointer");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(amp_unscale_sqnorm_chunk_kernel, dim3(nchunks), dim3(256), 0, s, grads, n, (const SlChunk*)chunks, ngroups,
                     scale, found_inf, partials);
  rc = check_launch("amp_unscale_sqnorm_chunk_kernel");
  if (rc != RFN_OK) return rc;
  return sl_launch_groups(partials, chunks, nchunks, ngroups, out, s);
}

int rfn_grad_clip_coef(const double* sqnorms, int ngroups, float max_norm, float* coef, rfn_stream_t stream) {
  RFN_REQUIRE(sqnorms && coef && ((size_t)sqnorms & 7) == 0 && ((size_t)coef & 3) == 0,
              "grad_clip_coef: null or unaligned pointer");
  RFN_REQUIRE(ngroups > 0 && ngroups <= kSlMaxGroups, "grad_clip_coef: %d groups (1 ... %d)", ngroups, kSlMaxGroups);
  RFN_REQUIRE(max_norm >= 0.f, "grad_clip_coef: max_norm %g (a number >= 0)", (double)max_norm);
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sqnorms, ngroups, max_norm, coef);
  return check_launch("grad_clip_coef_kernel");
}

int rfn_grad_scale_f32(float* grads, long n, const float* coef, rfn_stream_t stream) {
  RFN_REQUIRE(grads && coef && n > 0 && ((size_t)grads & 15) == 0 && ((size_t)coef & 3) == 0,
              "grad_scale_f32: null pointer, empty or unaligned buffer");
  hipLaunchKernelGGL(grad_scale_kernel, dim3(sl_stream_grid(n)), dim3(256), 0, (hipStream_t)stream, grads, n, coef);
  return check_launch("grad_scale_kernel");
}

int rfn_grad_clamp_f32(float* grads, long n, float clip_value, rfn_stream_t stream) {
  RFN_REQUIRE(grads && n > 0 && ((size_t)grads & 15) == 0, "grad_clamp_f32: null pointer, empty or unaligned buffer");
  RFN_REQUIRE(clip_value >= 0.f, "grad_clamp_f32: clip_value %g (a number >= 0)", (double)clip_value);
  hipLaunchKernelGGL(grad_clamp_kernel, dim3(sl_stream_grid(n)), dim3(256), 0, (hipStream_t)stream, grads, n, clip_value);
  return check_launch("grad_clamp_kernel");
}

}  // extern "C"
