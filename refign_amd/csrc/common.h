// refign_amd/csrc/common.h -- shared helpers for the gfx950 kernels (error reporting, launch checks, math).
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <type_traits>

#include "../../include/refign_hip.h"
#include "elem.h"

namespace rfn {

// Thread-local last-error message (rfn_last_error()).
char* err_buf();
int fail(int code, const char* fmt, ...);

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(RFN_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return RFN_OK;
}

constexpr int kWave = 64;  // CDNA wavefront width

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Activation dtype codes of the C ABI: 0 = float32, 1 = bfloat16, 2 = float16 (elem.h: ElemOf).  dt_one / dt_pair call fn with
// an ElemTag<T> per code (dt_pair: the pairs that meet in one call -- equal codes, or one of them fp32; bf16 and fp16 never
// mix) and return RFN_EINVAL with `what` in the message for anything else.
template <typename Fn>
inline int dt_one(int a, const char* what, Fn&& fn) {
  switch (a) {
    case 0: return fn(ElemOf<0>{});
    case 1: return fn(ElemOf<1>{});
    case 2: return fn(ElemOf<2>{});
  }
  return fail(RFN_EINVAL, "%s: dtype code must be 0 (f32), 1 (bf16) or 2 (f16) (got %d)", what, a);
}
template <typename Fn>
inline int dt_pair(int a, int b, const char* what, Fn&& fn) {
  if (a == 0 && b == 0) return fn(ElemOf<0>{}, ElemOf<0>{});
  if (a == 0 && b == 1) return fn(ElemOf<0>{}, ElemOf<1>{});
  if (a == 1 && b == 0) return fn(ElemOf<1>{}, ElemOf<0>{});
  if (a == 1 && b == 1) return fn(ElemOf<1>{}, ElemOf<1>{});
  if (a == 0 && b == 2) return fn(ElemOf<0>{}, ElemOf<2>{});
  if (a == 2 && b == 0) return fn(ElemOf<2>{}, ElemOf<0>{});
  if (a == 2 && b == 2) return fn(ElemOf<2>{}, ElemOf<2>{});
  return fail(RFN_EINVAL, "%s: dtype codes (%d, %d): each 0 (f32), 1 (bf16) or 2 (f16), bf16 and f16 not mixed", what, a, b);
}

// The entry points that take 16-bit activations only.  dt16: the matrix-core kernels are templated on the code itself,
// fn(std::integral_constant<int, 1 or 2>); dt16_type: fn(ElemTag<T>) as dt_one, for kernels templated on the storage type.
inline int dt16_check(int a, const char* what) {      // the check alone, for entry points that keep their own launch code
  return a == 1 || a == 2 ? RFN_OK : fail(RFN_EINVAL, "%s: dtype %d (1 = bf16, 2 = f16)", what, a);
}
template <typename Fn>
inline int dt16(int a, const char* what, Fn&& fn) {
  if (a == 1) return fn(std::integral_constant<int, 1>{});
  if (a == 2) return fn(std::integral_constant<int, 2>{});
  return dt16_check(a, what);
}
template <typename Fn>
inline int dt16_type(int a, const char* what, Fn&& fn) {
  return dt16(a, what, [&](auto code) { return fn(ElemOf<decltype(code)::value>{}); });
}

// compile-time loop: f(std::integral_constant<int, I>) for I = B .. N - 1 (register arrays need literal indices)
template <int I, int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// rfn_set_deterministic() / rfn_get_deterministic(): process-wide (capi.hip)
int deterministic();

// out[c] = sum over r of part[r * cols + c], added in an order that depends on (rows, cols) only (det.hip): the second launch
// of the store-and-sum forms that replace floating-point atomics in deterministic mode
int ordered_colsum_f32(const float* part, float* out, long rows, int cols, hipStream_t st);
int ordered_colsum_f64(const double* part, double* out, long rows, int cols, hipStream_t st);

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// zero-fill as a kernel on `st` (capi.hip: why not hipMemsetAsync)
int zero_async(void* p, size_t bytes, hipStream_t st);

// 64 bytes of zeros in device memory (capi.hip): what an LDS-DMA piece or a tap outside the image / past the last k reads.
// Null if the look-up failed.
const void* zero_page();

}  // namespace rfn

// Entry points whose result depends on the arrival order of floating-point atomics refuse while the deterministic flag is set.
#define RFN_REFUSE_NONDET(cond, entry, why)                                                                              \
  do {                                                                                                                   \
    if (rfn::deterministic() && (cond))                                                                                  \
      return rfn::fail(RFN_ENONDET, "%s refused in deterministic mode: %s", entry, why);                                 \
  } while (0)

#define RFN_REQUIRE(cond, ...) \
  do {                         \
    if (!(cond)) return rfn::fail(RFN_EINVAL, __VA_ARGS__); \
  } while (0)
