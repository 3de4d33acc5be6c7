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

// one workgroup per chunk.  A chunk that does not lie inside [0, n) or names no group reads nothing and leaves a NaN partial
// (counted by stage two): a damaged table cannot make the kernel read out of bounds.
__global__ __launch_bounds__(256) void grad_sqnorm_chunk_kernel(const float* __restrict__ g, long n,
                                                                const SlChunk* __restrict__ chunks, int G,
                                                                double* __restrict__ partials) {
  __shared__ double wsum[4];
  const SlChunk c = chunks[blockIdx.x];
  const int tid = threadIdx.x;
  if (!sl_chunk_ok(c, n, G)) {
    if (tid == 0) partials[blockIdx.x] = __builtin_nan("");
    return;
  }
  const float* p = g + c.off;
  // scalar head up to the next 16-byte boundary (the buffer itself is 16-byte aligned), float4 body, scalar tail
  const long head = min(c.len, (long)((4 - (c.off & 3)) & 3));
  const long n4 = (c.len - head) >> 2, tail0 = head + 4 * n4;
  double a0 = 0.0, a1 = 0.0;
  if (tid < head) {
    const double v = (double)p[tid];
    a0 = v * v;
  }
  const float4* p4 = reinterpret_cast<const float4*>(p + head);
#pragma unroll 4
  for (long i = tid; i < n4; i += 256) {
    const float4 v = p4[i];
    const double x = (double)v.x, y = (double)v.y, z = (double)v.z, w = (double)v.w;
    a0 = fma(x, x, a0);
    a1 = fma(y, y, a1);
    a0 = fma(z, z, a0);
    a1 = fma(w, w, a1);
  }
  if (tail0 + tid < c.len) {
    const double v = (double)p[tail0 + tid];
    a1 = fma(v, v, a1);
  }
  const double s = sl_wave_sum(a0 + a1);
  if ((tid & 63) == 0) wsum[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
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

int rfn_grad_sqnorm_groups(const float* flat, long n, const long* chunks, int nchunks, int ngroups, double* partials,
                           double* out, rfn_stream_t stream) {
  RFN_REQUIRE(flat && chunks && partials && out, "grad_sqnorm_groups: null pointer");
  RFN_REQUIRE(n > 0 && nchunks > 0 && nchunks <= (1 << 22), "grad_sqnorm_groups: n=%ld nchunks=%d (1 ... 2^22)", n, nchunks);
  RFN_REQUIRE(ngroups > 0 && ngroups <= kSlMaxGroups, "grad_sqnorm_groups: %d groups (1 ... %d)", ngroups, kSlMaxGroups);
  RFN_REQUIRE(((size_t)flat & 15) == 0 && ((size_t)chunks & 7) == 0 && ((size_t)partials & 7) == 0 && ((size_t)out & 7) == 0,
              "grad_sqnorm_groups: flat must be 16-byte aligned, chunks / partials / out 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_sqnorm_chunk_kernel, dim3(nchunks), dim3(256), 0, s, flat, n, (const SlChunk*)chunks, ngroups, partials);
  int rc = check_launch("grad_sqnorm_chunk_kernel");
  if (rc != RFN_OK) return rc;
  hipLaunchKernelGGL(grad_sqnorm_groups_kernel, dim3(1), dim3(256), 0, s, (const double*)partials, (const SlChunk*)chunks, nchunks,
                     ngroups, out);
  return check_launch("grad_sqnorm_groups_kernel");
}

}  // extern "C"
