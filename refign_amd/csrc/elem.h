// refign_amd/csrc/elem.h -- the activation dtypes of the C ABI and the conversions between their storage forms and fp32:
// one tag per storage type, the map between the ABI's dtype codes and the tags, and scalar / packed-pair / 8-wide loads,
// stores and roundings.  Widening is exact; narrowing is one hardware rounding (round to nearest even, torch's conversion).
// Everything here is __forceinline__: a kernel pays for what it calls and nothing else.  (mfma.h keeps pack4 / unpack4 /
// join8, the MFMA operand forms of the matrix kernels.)
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <type_traits>

#include "mfma.h"   // f8e4m3, quant4

namespace rfn {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// Storage tags: float, __hip_bfloat16, _Float16 (and mfma.h's f8e4m3, store side only).  ElemTag<T> is what the dispatchers of
// common.h hand to their callbacks (`typename decltype(t)::type`); ElemOf<code> / elem_t<code> / code_of<T> are the ABI's
// dtype codes: 0 = float32, 1 = bfloat16, 2 = float16.
template <typename T>
struct ElemTag {
  using type = T;
};
template <int CODE> struct ElemOf;
template <> struct ElemOf<0> : ElemTag<float> {};
template <> struct ElemOf<1> : ElemTag<__hip_bfloat16> {};
template <> struct ElemOf<2> : ElemTag<_Float16> {};
template <int CODE> using elem_t = typename ElemOf<CODE>::type;
template <typename T>
constexpr int code_of = std::is_same<T, float>::value ? 0 : std::is_same<T, __hip_bfloat16>::value ? 1 : 2;
// the compiler's arithmetic type behind a tag (__hip_bfloat16 is a struct: vectors and casts want __bf16)
template <typename T>
using native_t = std::conditional_t<std::is_same<T, __hip_bfloat16>::value, __bf16, T>;

// fp32 -> bf16 bits, round to nearest even (torch's conversion; NaN stays NaN): gfx950 has the conversion in hardware
// (v_cvt_pk_bf16_f32, two values per instruction).  The integer formulation (add 0x7fff + lsb, NaN select) is 5-6
// instructions per element -- it made up a third of the instructions of the 16-bit element-wise kernels.
__device__ __forceinline__ unsigned bf16_bits(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }
__device__ __forceinline__ unsigned bf16x2_bits(float lo, float hi) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  const bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, v);
}

// fp32 -> fp16 bits, round to nearest even (torch's .to(torch.float16): overflow -> inf, NaN stays NaN), and back
__device__ __forceinline__ unsigned f16_bits(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
__device__ __forceinline__ unsigned f16x2_bits(float lo, float hi) {
  typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
  const f16x2 v = {(_Float16)lo, (_Float16)hi};
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float f16_lo(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu)); }
__device__ __forceinline__ float f16_hi(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }

// ---- one element ---------------------------------------------------------------------------------------------------------
// the 16 bits of v rounded to T (for kernels that address 16-bit storage as unsigned short)
template <typename T>
__device__ __forceinline__ unsigned bits16(float v) {
  if constexpr (std::is_same<T, _Float16>::value) return f16_bits(v);
  else return bf16_bits(v);
}
template <typename T>
__device__ __forceinline__ float ldf(const T* p) {
  return (float)*reinterpret_cast<const native_t<T>*>(p);
}
template <typename T>
__device__ __forceinline__ void stf(T* p, float v) {
  if constexpr (std::is_same<T, __hip_bfloat16>::value) *reinterpret_cast<unsigned short*>(p) = (unsigned short)bf16_bits(v);
  else if constexpr (std::is_same<T, f8e4m3>::value) p->v = (unsigned char)(quant4(v, 0.f, 0.f, 0.f) & 0xffu);
  else *p = (T)v;
}
// the value a store of v reads back as.  BITS (bf16 only): through bf16_bits and a shift instead of a pair of casts -- the same
// value, but the rounded bits are then the ones a following narrow2 / store8 of v produces, and the compiler shares the
// conversion: dwconv3x3_fwd_kernel<bf16, stats> has 1682 instructions with it and 1765 (32 more v_cvt_pk_bf16_f32) without,
// while loss.hip's kernels, which store nothing 16-bit, gain a v_max_f32 (canonicalisation) per rounded value with it.
template <typename T, bool BITS = false>
__device__ __forceinline__ float round_to(float v) {
  if constexpr (std::is_same<T, float>::value) return v;
  else if constexpr (BITS && std::is_same<T, __hip_bfloat16>::value) return __uint_as_float(bf16_bits(v) << 16);
  else return (float)(native_t<T>)v;
}

// ---- one packed word = two adjacent 16-bit elements (low half first) --------------------------------------------------------
template <typename T>
__device__ __forceinline__ f32x2 widen2(unsigned w) {
  if constexpr (std::is_same<T, _Float16>::value) return f32x2{f16_lo(w), f16_hi(w)};
  else return f32x2{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
}
template <typename T>
__device__ __forceinline__ unsigned narrow2(float lo, float hi) {
  if constexpr (std::is_same<T, _Float16>::value) return f16x2_bits(lo, hi);
  else return bf16x2_bits(lo, hi);
}

// ---- eight adjacent elements: one 16-byte vector of a 16-bit type (two float4 of fp32, one uint2 of e4m3) <-> float[8] ------
// VCAST: widen / narrow through mfma.h's unpack4 / pack4 (a cast of a 4-vector) instead of shifts and masks per word.  The values
// are the same; the compiler schedules the two differently, and the kernels written against raw 16-bit words (bn.hip,
// kvpath.hip: the code-keyed load8 / store8 below) keep their registers only with the cast: with shifts and masks
// bn_apply_kernel<1, true> goes from 80 to 92 VGPRs and bn_stats_kernel<1, true> from 130 to 169, one occupancy step each,
// while the row kernels of layernorm.hip / reduce.hip gain instructions with the cast (profiles/elem_refactor_build.txt).
// The code-keyed forms also keep bn.hip's 16-byte access through the compiler's own vector type: as a uint4 (a struct to
// the alias analysis) the same loads cost those kernels one to three address instructions each.
template <typename T, bool VCAST = false>
__device__ __forceinline__ void widen8(const uint4& t, float (&v)[8]) {
  if constexpr (VCAST) {
    float a[4], b[4];
    unpack4<code_of<T>>(u32x2{t.x, t.y}, a);
    unpack4<code_of<T>>(u32x2{t.z, t.w}, b);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = a[i];
      v[4 + i] = b[i];
    }
  } else {
    const unsigned w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (std::is_same<T, _Float16>::value) {
        v[2 * i] = f16_lo(w[i]);
        v[2 * i + 1] = f16_hi(w[i]);
      } else {
        v[2 * i] = __uint_as_float(w[i] << 16);
        v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
      }
    }
  }
}
template <typename T, bool VCAST = false>
__device__ __forceinline__ uint4 narrow8(const float (&v)[8]) {
  if constexpr (VCAST) {
    const u32x2 lo = pack4<code_of<T>>(v[0], v[1], v[2], v[3]), hi = pack4<code_of<T>>(v[4], v[5], v[6], v[7]);
    return make_uint4(lo[0], lo[1], hi[0], hi[1]);
  } else {
    return make_uint4(narrow2<T>(v[0], v[1]), narrow2<T>(v[2], v[3]), narrow2<T>(v[4], v[5]), narrow2<T>(v[6], v[7]));
  }
}
template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&v)[8]) {
  if constexpr (std::is_same<T, float>::value) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    widen8<T>(*reinterpret_cast<const uint4*>(p), v);
  }
}
template <typename T>
__device__ __forceinline__ void store8(T* p, const float (&v)[8]) {
  if constexpr (std::is_same<T, float>::value) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  } else if constexpr (std::is_same<T, f8e4m3>::value) {       // K5: e4m3 bytes, saturating RNE
    *reinterpret_cast<uint2*>(p) = make_uint2(quant4(v[0], v[1], v[2], v[3]), quant4(v[4], v[5], v[6], v[7]));
  } else {
    *reinterpret_cast<uint4*>(p) = narrow8<T>(v);
  }
}

// ---- the same, for kernels templated on the ABI's code and written against raw 16-bit words --------------------------------
template <int CODE>
__device__ __forceinline__ float ldf(const void* p, long i) { return ldf(reinterpret_cast<const elem_t<CODE>*>(p) + i); }
template <int CODE>
__device__ __forceinline__ float round_to(float v) { return round_to<elem_t<CODE>>(v); }
template <int CODE>
__device__ __forceinline__ f32x2 widen2(unsigned w) { return widen2<elem_t<CODE>>(w); }
template <int CODE>
__device__ __forceinline__ void load8(const uint16_t* p, float (&v)[8]) {
  const u32x4 t = *(const u32x4*)p;
  widen8<elem_t<CODE>, true>(make_uint4(t[0], t[1], t[2], t[3]), v);
}
template <int CODE>
__device__ __forceinline__ void store8(uint16_t* p, const float (&v)[8]) {
  const uint4 t = narrow8<elem_t<CODE>, true>(v);
  *(u32x4*)p = u32x4{t.x, t.y, t.z, t.w};
}

}  // namespace rfn
