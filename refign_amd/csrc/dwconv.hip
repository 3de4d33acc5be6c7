// refign_amd/csrc/dwconv.hip -- depthwise 3x3 convolution on channels-last maps, forward + both backward passes (gfx950).
//
// Where it sits in the reference: the Mix-FFN of every MiT block runs fc1 -> DWConv 3x3 -> GELU -> fc2
// (models/backbones/mix_transformer.py:96-103,556-568: tokens are transposed to NCHW, nn.Conv2d(dim, dim, 3, 1, 1,
// groups=dim), transposed back), and the DAFormer head's ASPP has three dilated depthwise 3x3 branches on 1024 channels
// (models/heads/daformer.py:46-62).  On this stack the library path for those (MIOpen -> CK grouped conv) is a
// dense-conv kernel with group size 1 and was measured at 59 % of the whole training step; the op itself is a pure
// HBM-bound 9-tap stencil.
//
// Weights and weight gradients cross the ABI TAP-MAJOR, (9, C) fp32 (= weight.view(C, 9).t()), so that the 9 x VEC
// weights of a thread are nine contiguous vectors.
// Layout: x, y, grad tensors are (B, H, W, C) contiguous = the MiT token layout (B, N, C) itself, so no transposes at
// all; lanes run along C (16-byte vectors: 8 bf16 or 4 fp32 channels per lane => a wave reads 1 KiB contiguous), each
// thread produces 4 consecutive pixels along W and keeps its 9 x VEC weights in registers.  Halo re-reads between
// neighbouring threads/blocks are served by L1/L2.  Accumulation is fp32; weights/bias/weight-gradients stay fp32
// (master precision) while activations may be bf16 or fp16.
//   forward       y[b,h,w,c]  = bias[c] + sum_{ky,kx} wgt[c,ky,kx] * x[b, h+(ky-1)d, w+(kx-1)d, c]
//   backward-data dx           = same stencil over gy with the taps flipped, no bias
//   backward-wgt  dw[c,ky,kx]  = sum_{b,h,w} gy[b,h,w,c] * x[b, h+(ky-1)d, w+(kx-1)d, c];   db[c] = sum gy
//                 (per-thread register partials over its pixel quads -> LDS tree over the block's pixel lanes ->
//                  one workspace row per block row -> fixed-order reduction kernel: deterministic, no atomics)
//   backward      both of them from ONE pass over gy (dwconv3x3_bwd_kernel): gy, x and dx cross HBM once each
// Kernels: dwconv3x3_fwd_kernel (forward; taps flipped = backward-data alone; + GELU; + the BatchNorm statistics of what it
// stores), dwconv3x3_roll_kernel (the gradient-free forms: statistics only, convolution + BatchNorm + ReLU),
// dwconv3x3_bwd_kernel (both gradients, or the parameter gradients alone) and dwconv3x3_bwd_weight_reduce_kernel.
#include <hip/hip_bf16.h>

#include <type_traits>

#include "common.h"
#include "elem.h"

namespace rfn {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// Vector I/O of one lane: N channels as a packed Raw; unpack2 -> adjacent-channel fp32 pairs, store <- N fp32 values.
template <typename T>
struct VecIO;

template <>
struct VecIO<float> {
  static constexpr int N = 4;
  typedef float4 Raw;
  __device__ static Raw load_raw(const float* p) { return *reinterpret_cast<const float4*>(p); }
  __device__ static void unpack2(const Raw& t, f32x2 (&v)[2]) { v[0] = f32x2{t.x, t.y}; v[1] = f32x2{t.z, t.w}; }
  __device__ static void store(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
  __device__ static float rnd(float v) { return round_to<float>(v); }   // the value a store of v reads back as
};

// 16-bit activations: bf16, and fp16 (the reference's `precision: 16` recipe) in the same layout with IEEE half conversions
// (elem.h: widen2, one packed word -> two adjacent channels, and narrow2, back).
// NCH = 8 channels per lane (16-byte vectors: dwconv3x3_fwd_kernel) or 4 (8-byte vectors: dwconv3x3_roll_kernel, dwconv3x3_bwd_kernel)
template <typename T, int NCH>
struct Vec16 {
  static constexpr int N = NCH, NW = NCH / 2;
  typedef std::conditional_t<NCH == 8, uint4, uint2> Raw;
  __device__ static Raw load_raw(const T* p) { return *reinterpret_cast<const Raw*>(p); }
  __device__ static void unpack2(const Raw& t, f32x2 (&v)[NW]) {      // adjacent channels land in adjacent registers
    v[0] = widen2<T>(t.x);
    v[1] = widen2<T>(t.y);
    if constexpr (NCH == 8) {
      v[2] = widen2<T>(t.z);
      v[3] = widen2<T>(t.w);
    }
  }
  __device__ static unsigned pack(float lo, float hi) { return narrow2<T>(lo, hi); }
  __device__ static void store(T* p, const float (&v)[NCH]) {
    Raw t;
    t.x = pack(v[0], v[1]);
    t.y = pack(v[2], v[3]);
    if constexpr (NCH == 8) {
      t.z = pack(v[4], v[5]);
      t.w = pack(v[6], v[7]);
    }
    *reinterpret_cast<Raw*>(p) = t;
  }
  __device__ static float rnd(float v) { return round_to<T, true>(v); }   // BITS: elem.h
};
template <>
struct VecIO<__hip_bfloat16> : Vec16<__hip_bfloat16, 8> {};
template <>
struct VecIO<_Float16> : Vec16<_Float16, 8> {};

// K5: e4m3 activations, 8 channels per lane (8-byte vectors); dequantisation / quantisation scales are kernel arguments
template <>
struct VecIO<f8e4m3> {
  static constexpr int N = 8;
  typedef uint2 Raw;
  __device__ static Raw load_raw(const f8e4m3* p) { return *reinterpret_cast<const uint2*>(p); }
  __device__ static void unpack2(const Raw& t, f32x2 (&v)[4]) {
    v[0] = __builtin_amdgcn_cvt_pk_f32_fp8((int)t.x, false);
    v[1] = __builtin_amdgcn_cvt_pk_f32_fp8((int)t.x, true);
    v[2] = __builtin_amdgcn_cvt_pk_f32_fp8((int)t.y, false);
    v[3] = __builtin_amdgcn_cvt_pk_f32_fp8((int)t.y, true);
  }
  __device__ static void store(f8e4m3* p, const float (&v)[8]) { store8(p, v); }
};

constexpr int kPX = 4;   // pixels along W per thread

// A "quad" is 4 pixels of one image row spaced by the dilation: w0, w0+d, w0+2d, w0+3d.  Their 3x3 dilated taps fall on
// the 6 columns w0-d .. w0+4d, so 6 loads per row feed 4 outputs for ANY dilation (for d = 1 it is 4 adjacent pixels).
// Per row there are d phases x ceil(ceil(W/d)/4) quads.
__host__ __device__ __forceinline__ int quads_per_row(int W, int dil) { return dil * (((W + dil - 1) / dil + kPX - 1) / kPX); }

__device__ __forceinline__ void quad_coords(long quad, int WQ, int H, int dil, int& b, int& h, int& w0) {
  const int wq = (int)(quad % WQ);
  const long t = quad / WQ;
  h = (int)(t % H);
  b = (int)(t / H);
  w0 = (wq % dil) + (wq / dil) * kPX * dil;
}

// Thread layout (all three kernels): blockDim = 256 = cvb channel-vectors (fastest, so a wave reads contiguous
// channels) x pl pixel lanes.  A thread keeps ONE channel vector for its whole life -- its 9 x V weights are loaded
// once -- and walks items ("quads": 4 pixels of one image row; the rolling walk: strips of a row segment) with stride
// block rows x pl.
// Two launch geometries.
//  * grid (channel blocks, block rows), rows in image order: the first-generation mapping.
//  * SLICED (gridDim.y == 1, sliced != 0): a 1-D grid of 8 j blocks; block id runs on XCD id % 8 (the dispatcher's
//    round-robin) and owns channel slice id % 8 (cvb = CV / 8 vectors) -- so the three uses of an input row (output
//    rows h - d, h, h + d) are made by ONE XCD and the second and third find the row in that XCD's L2 -- provided they
//    come soon enough: the blocks of an XCD walk the rows in lockstep (the grid is exactly the resident blocks), and
//    for a dilated convolution in residue-class order r, r + d, r + 2 d, ... (h_slots = d ceil(H / d) slots per image),
//    so the uses are 1 and 2 rows apart whatever the dilation.  With the first mapping a row's uses land on different
//    XCDs / megabytes apart: each is a fabric read (measured round 3: tools/kbench.py --only dw).
struct DwMap {
  int pl, cvbase, cv;      // pixel lanes of the block; first channel vector of the block; the thread's channel vector
  int first, stride, row;  // the thread's first item and item stride; block row (= row of a partial-sum workspace)
  bool active;             // false: a lane past the last channel vector (or past cvb x pl), it only joins the block's folds
};
// (nthreads = blockDim.x, read by the kernel: in a kernel body the compiler folds the work-group size lookup to one load,
// in a device function it keeps the partial-group select)
__device__ __forceinline__ DwMap dw_map(int sliced, int cvb, int CV, unsigned nthreads) {
  DwMap m;
  if (sliced) {
    m.pl = nthreads / cvb;
    m.active = (int)threadIdx.x < cvb * m.pl;
    m.cvbase = (blockIdx.x & 7) * cvb;
    m.cv = m.cvbase + threadIdx.x % cvb;
    m.row = blockIdx.x >> 3;
    m.first = m.row * m.pl + threadIdx.x / cvb;
    m.stride = (gridDim.x >> 3) * m.pl;
  } else {
    m.pl = 256 / cvb;
    m.cvbase = blockIdx.x * cvb;
    m.cv = m.cvbase + threadIdx.x % cvb;
    m.active = m.cv < CV;
    m.row = blockIdx.y;
    m.first = m.row * m.pl + threadIdx.x / cvb;
    m.stride = gridDim.y * m.pl;
  }
  return m;
}

// The thread's 9 x V tap-major weights (9, C) as adjacent-channel pairs: one contiguous fp32 vector per tap.  FLIP: wr[k] is
// tap 8 - k (the backward-data stencil); SCALE (e4m3 activations): the input scale xs folded in.
template <int V, bool FLIP, bool SCALE = false>
__device__ __forceinline__ void load_taps(const float* wgt, int C, int c0, f32x2 (&wr)[9][V / 2], float xs = 1.f) {
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float* wp = wgt + (size_t)(FLIP ? 8 - k : k) * C + c0;
#pragma unroll
    for (int i = 0; i < V; i += 4) {
      const float4 t4 = *reinterpret_cast<const float4*>(wp + i);
      wr[k][i / 2] = f32x2{t4.x, t4.y};
      wr[k][i / 2 + 1] = f32x2{t4.z, t4.w};
      if constexpr (SCALE) {
        wr[k][i / 2] *= xs;
        wr[k][i / 2 + 1] *= xs;
      }
    }
  }
}

// The statistics epilogue of dwconv3x3_fwd_kernel<STATS> and dwconv3x3_roll_kernel<STATS = 2>: per-thread fp32 sums (st0: sum,
// st1: sum of squares, V channels as floats or as pairs) -> LDS -> thread (which, channel vector of the block, element) folds
// the pixel lanes in lane order -> one fp64 atomic per channel and block, or (spart: the deterministic form) one row of 2 C
// partial sums per block row, plain stores, added in row order afterwards.  One thread of the launch writes the row count.
template <int N>
__device__ __forceinline__ float stat_elem(const float (&s)[N], int i) { return s[i]; }
template <int N>
__device__ __forceinline__ float stat_elem(const f32x2 (&s)[N], int i) { return (i & 1) ? s[i / 2].y : s[i / 2].x; }

template <int V, typename St>
__device__ __forceinline__ void fold_stats(const DwMap& m, int cvb, int CV, int B, int H, int W, int C, const St& st0,
                                           const St& st1, double* sums, double* spart) {
  __shared__ float sred[2][256][V + 1];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    sred[0][threadIdx.x][i] = m.active ? stat_elem(st0, i) : 0.f;
    sred[1][threadIdx.x][i] = m.active ? stat_elem(st1, i) : 0.f;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 2 * cvb * V; idx += blockDim.x) {
    const int which = idx / (cvb * V), rem = idx % (cvb * V), v = rem / V, e = rem % V;
    if (m.cvbase + v >= CV) continue;
    float sum = 0.f;
    for (int r = 0; r < m.pl; ++r) sum += sred[which][r * cvb + v][e];
    if (spart != nullptr) spart[((size_t)m.row * 2 + which) * C + (m.cvbase + v) * V + e] = (double)sum;
    else atomicAdd(sums + which * C + (m.cvbase + v) * V + e, (double)sum);
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    if (spart != nullptr) sums[2 * C] = (double)B * H * W;
    else atomicAdd(sums + 2 * C, (double)B * H * W);
  }
}

// zero a packed load when its tap is outside the image (true zero padding; 4 selects instead of one multiply per FMA)
__device__ __forceinline__ float4 mask_raw(const float4& t, bool ok) {
  return ok ? t : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ uint4 mask_raw(const uint4& t, bool ok) { return ok ? t : make_uint4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ uint2 mask_raw(const uint2& t, bool ok) { return ok ? t : make_uint2(0u, 0u); }

// ACT: the Mix-FFN applies GELU (exact erf) right after this convolution (mix_transformer.py:99-101): with ACT the
// activation is computed on the fp32 accumulators and written to `ya`; the pre-activation goes to `y` only if that
// pointer is given (the backward needs it, a gradient-free pass does not) -- the separate GELU kernel (one more read
// and write of the 4C-wide hidden tensor) disappears.
// STATS: the BatchNorm that follows a depthwise convolution of the decode heads (daformer.py:10-62: DepthwiseSeparable ASPP
// branch = depthwise 3x3 -> BN -> ReLU -> 1x1 -> BN -> ReLU) needs the per-channel sum and sum of squares of THIS kernel's
// result: a thread owns one channel vector for its whole life, so it adds up what it stores (the ROUNDED values: what the
// statistics pass of csrc/bn.hip would have read back -- 2.65 GB for the teacher's 42 maps, 0.5 ms, per branch), the block
// folds its pixel lanes in LDS and adds to the fp64 buffer of csrc/bn.hip (sum x, sum x^2, rows).
// The gradient-free form (the EMA teacher's decode head) runs as two passes over the INPUT in dwconv3x3_roll_kernel below:
// statistics only (nothing stored), then convolution + BatchNorm(batch statistics from `sums`) + ReLU; 3 tensor passes (read,
// read, write) instead of the 5 of convolution (read, write), statistics (read), BatchNorm (read, write).  BnEpi: gamma / beta
// (may be null), eps, relu, and the running buffers the blocks of the first row of the grid update (momentum), as
// csrc/bn.hip's apply pass does.
struct BnEpi {
  const float* gamma;
  const float* beta;
  float* running_mean;
  float* running_var;
  float eps, momentum;
  int relu;
};

template <typename T, bool FLIP, bool ACT = false, bool STATS = false>
__global__ __launch_bounds__(256) void dwconv3x3_fwd_kernel(const T* __restrict__ x, const float* __restrict__ wgt,
                                                            const float* __restrict__ bias, T* __restrict__ y, int B,
                                                            int H, int W, int C, int dil, int cvb,
                                                            T* __restrict__ ya = nullptr, float xs = 1.f,
                                                            float oq = 1.f, int sliced = 0,
                                                            double* __restrict__ sums = nullptr,
                                                            double* __restrict__ spart = nullptr) {
  // xs / oq (e4m3 activations only): stored input bytes mean xs * value -- folded into the weights; outputs are stored as
  // value * oq
  constexpr bool F8 = std::is_same<T, f8e4m3>::value;
  constexpr int V = VecIO<T>::N, V2 = V / 2;
  const int CV = C / V, WQ = quads_per_row(W, dil);
  const DwMap m = dw_map(sliced, cvb, CV, blockDim.x);
  if (!STATS && !m.active) return;                       // (STATS: idle threads stay for the block reduction)
  const int Hd = (H + dil - 1) / dil, h_slots = sliced ? dil * Hd : H;
  const int c0 = (m.active ? m.cv : 0) * V;
  float st0[STATS ? V : 1], st1[STATS ? V : 1];
  if constexpr (STATS) {
#pragma unroll
    for (int i = 0; i < V; ++i) st0[i] = st1[i] = 0.f;
  }
  // weights, bias and accumulators live as adjacent-channel PAIRS: every multiply-add below is one v_pk_fma_f32
  f32x2 wr[9][V2];
  load_taps<V, FLIP, F8>(wgt, C, c0, wr, xs);
  f32x2 bs[V2];
#pragma unroll
  for (int i = 0; i < V2; ++i)
    bs[i] = (bias != nullptr) ? f32x2{bias[c0 + 2 * i], bias[c0 + 2 * i + 1]} : f32x2{0.0f, 0.0f};
  const long nquads = m.active ? (long)B * h_slots * WQ : 0;
  for (long quad = m.first; quad < nquads; quad += m.stride) {
    int b, h, w0;
    quad_coords(quad, WQ, h_slots, dil, b, h, w0);
    if (sliced && dil > 1) {                            // slot -> row of residue class slot / Hd
      h = h / Hd + (h % Hd) * dil;
      if (h >= H) continue;
    }
    f32x2 acc[kPX][V2];
#pragma unroll
    for (int p = 0; p < kPX; ++p)
#pragma unroll
      for (int i = 0; i < V2; ++i) acc[p][i] = bs[i];
    const T* xb = x + (size_t)b * H * W * C + c0;
    // branch-free window: all 18 loads (3 rows x 6 columns, clamped addresses) are issued back to back and the
    // out-of-image taps are zeroed by a select on the packed data -- per-tap `if`s made hipcc wait for each load in turn
    typename VecIO<T>::Raw raw[3][kPX + 2];            // kept packed (bf16: 4 VGPRs per 8 channels) until used
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int yy = h + (ky - 1) * dil;
      const bool rowok = yy >= 0 && yy < H;
      const T* xr = xb + (size_t)min(max(yy, 0), H - 1) * W * C;
#pragma unroll
      for (int j = 0; j < kPX + 2; ++j) {
        const int xx = w0 + (j - 1) * dil;
        raw[ky][j] = mask_raw(VecIO<T>::load_raw(xr + (size_t)min(max(xx, 0), W - 1) * C),
                              rowok && xx >= 0 && xx < W);
      }
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int j = 0; j < kPX + 2; ++j) {
        f32x2 v[V2];
        VecIO<T>::unpack2(raw[ky][j], v);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int p = j - kx;                        // output pixel fed by column j through tap kx
          if (p < 0 || p >= kPX) continue;
#pragma unroll
          for (int i = 0; i < V2; ++i) acc[p][i] = __builtin_elementwise_fma(wr[ky * 3 + kx][i], v[i], acc[p][i]);
        }
      }
    const size_t obase = ((size_t)b * H + h) * W * C + c0;
#pragma unroll
    for (int p = 0; p < kPX; ++p)
      if (w0 + p * dil < W) {
        float o[V];
#pragma unroll
        for (int i = 0; i < V2; ++i) { o[2 * i] = acc[p][i].x; o[2 * i + 1] = acc[p][i].y; }
        if (!ACT || y != nullptr) VecIO<T>::store(y + obase + (size_t)(w0 + p * dil) * C, o);
        if constexpr (STATS) {
#pragma unroll
          for (int i = 0; i < V; ++i) {
            const float r = VecIO<T>::rnd(o[i]);
            st0[i] += r;
            st1[i] = fmaf(r, r, st1[i]);
          }
        }
        if (ACT) {
#pragma unroll
          for (int i = 0; i < V; ++i) {
            // fp32 activations (parity mode): libm's erff; 16-bit / e4m3 results: mfma.h gelu_erf_fast
            if constexpr (sizeof(T) == 4) o[i] = 0.5f * o[i] * (1.f + erff(o[i] * 0.70710678118654752440f));
            else o[i] = gelu_erf_fast(o[i]) * (F8 ? oq : 1.f);
          }
          VecIO<T>::store(ya + obase + (size_t)(w0 + p * dil) * C, o);
        }
      }
  }
  if constexpr (STATS) fold_stats<V>(m, cvb, CV, B, H, W, C, st0, st1, sums, spart);
}

// ---------------------------------------------------------------------------------------------------------------------
// Rolling row walk: the body of the gradient-free forms (STATS == 2: statistics only; BNE: convolution + BatchNorm +
// activation), 16-bit activations.  dwconv3x3_fwd_kernel fetches and converts 3 rows x 6 columns for every quad, so every
// input row is fetched, converted and edge-masked three times (for the output rows h - d, h, h + d).  Here a thread owns a
// channel vector and a strip of 4 outputs spaced by the dilation, as there, but walks a SEGMENT of consecutive rows of one
// residue class of one image (h, h + d, h + 2 d, ...): every row of 6 columns is loaded and converted ONCE and added into
// the three output rows it belongs to, whose fp32 accumulators stay in registers (the rolling window, kept as three rows of
// partial sums instead of three rows of inputs: 48 registers instead of 72 + 16); the three roles rotate by renaming (the
// walk is unrolled by 3, or by 6 with two load buffers), no register moves.  Loads run DEPTH rows ahead of their use.
//  * 4 channels per thread (8-byte loads; the lanes of a pixel still cover the 128-byte-or-longer run of their slice): with
//    8 channels the accumulators, 72 weights and the rows in flight do not fit in the 256 registers of 2 waves per SIMD.
//  * zero padding by ADDRESS: a column outside the image reads the zeroed line `zero` (its row step is 0), a row outside the
//    image is a row of zeros without loads; the zeros enter the same FMAs the masked loads of the first body entered, and an
//    output row meets its taps in the same order (bias, then ky = 0, 1, 2, within a row kx = 0, 1, 2), so the convolution
//    values are bit-equal.
//  * a segment starts from nothing: its first two rows (k0 - 1, k0) are loaded again, no sum is carried over an image, a
//    residue class or a segment.
// Items (image, residue class, segment, strip), strip fastest, are dealt to the pixel lanes of either launch geometry
// (dw_map: grid of channel blocks x lane blocks, or XCD-sliced); `seg` rows per segment: roll_geom().
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kRV = 4;                       // channels per thread of the rolling body
// rows in flight per thread: 2 for bf16 (measured against 1, profiles/dwconv_roll_kbench.txt); fp16, whose conversions need
// more temporaries, spills with 2
template <typename T>
constexpr int kRollDepth = std::is_same<T, _Float16>::value ? 1 : 2;

template <typename T, int STATS, bool BNE, int DEPTH>
__global__ __launch_bounds__(256, 2) void dwconv3x3_roll_kernel(const T* __restrict__ x, const float* __restrict__ wgt,
                                                             const float* __restrict__ bias, T* __restrict__ y, int B,
                                                             int H, int W, int C, int dil, int cvb, int seg, int sliced,
                                                             double* __restrict__ sums, BnEpi bn,
                                                             double* __restrict__ spart, const void* __restrict__ zero) {
  static_assert(sizeof(T) == 2 && (STATS == 2) != BNE, "statistics-only or BatchNorm form, 16-bit activations");
  static_assert(DEPTH == 1 || DEPTH == 2, "the walk is written for one or two rows in flight");
  constexpr int V = kRV, V2 = V / 2, NC = kPX + 2;
  const int CV = C / V, WQ = quads_per_row(W, dil);
  const DwMap m = dw_map(sliced, cvb, CV, blockDim.x);
  if (STATS == 0 && !m.active) return;                   // (STATS: idle threads stay for the block reduction)
  const int c0 = (m.active ? m.cv : 0) * V;
  f32x2 st0[STATS ? V2 : 1], st1[STATS ? V2 : 1];
  if constexpr (STATS != 0) {
#pragma unroll
    for (int i = 0; i < V2; ++i) st0[i] = st1[i] = f32x2{0.f, 0.f};
  }
  f32x2 bsc[BNE ? V2 : 1], bsh[BNE ? V2 : 1];            // y = relu(conv * bsc + bsh)
  if constexpr (BNE) {
    const double cnt = sums[2 * C], inv = 1.0 / cnt;
    const bool first = m.row == 0 && m.active && threadIdx.x / cvb == 0;   // the first pixel lane of the first block row
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int c = c0 + i;
      const double m = sums[c] * inv;
      const float var = (float)fmax(sums[C + c] * inv - m * m, 0.0), mean = (float)m;
      const float g = bn.gamma != nullptr ? bn.gamma[c] : 1.f, be = bn.beta != nullptr ? bn.beta[c] : 0.f;
      const float sc = rsqrtf(var + bn.eps) * g, sh = be - mean * sc;
      if (i & 1) bsc[i / 2].y = sc, bsh[i / 2].y = sh;
      else bsc[i / 2].x = sc, bsh[i / 2].x = sh;
      if (first && bn.running_mean != nullptr) {
        const float n = (float)cnt;
        bn.running_mean[c] = (1.f - bn.momentum) * bn.running_mean[c] + bn.momentum * mean;
        bn.running_var[c] = (1.f - bn.momentum) * bn.running_var[c] + bn.momentum * var * (n / fmaxf(n - 1.f, 1.f));
      }
    }
  }
  f32x2 wr[9][V2], bs[V2];
  load_taps<V, false>(wgt, C, c0, wr);
#pragma unroll
  for (int i = 0; i < V2; ++i)
    bs[i] = (bias != nullptr) ? f32x2{bias[c0 + 2 * i], bias[c0 + 2 * i + 1]} : f32x2{0.0f, 0.0f};

  const int Hd = (H + dil - 1) / dil, nseg = (Hd + seg - 1) / seg;
  const int nitems = m.active ? B * dil * nseg * WQ : 0; // (fits: checked at launch)
  const unsigned rs = (unsigned)((size_t)dil * W * C * sizeof(T));   // one row of a residue class down, in bytes
  const size_t dc = (size_t)dil * C;                                  // one output of the strip to the right
  for (int it = m.first; it < nitems; it += m.stride) {
    const int wq = it % WQ;
    int t = it / WQ;
    const int sg = t % nseg;
    t /= nseg;
    const int r = t % dil, b = t / dil;
    const int nr = (H - r + dil - 1) / dil;              // rows of residue class r (0 when r >= H)
    const int k0 = sg * seg, k1 = min(k0 + seg, nr);     // this segment: rows r + k dil, k0 <= k < k1
    const int w0 = (wq % dil) + (wq / dil) * kPX * dil;
    if (k0 >= nr || w0 >= W) continue;
    // column addresses at row k0 - 1 (never dereferenced while that is outside the image) and their row steps
    typedef const __attribute__((address_space(1))) char* gptr;   // (global: the loads stay global_load through the asm below)
    gptr ap[NC];
    unsigned astep[NC];
    const long row0 = ((long)b * H + r + (long)(k0 - 1) * dil) * W;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int xx = w0 + (j - 1) * dil;
      const bool ok = xx >= 0 && xx < W;
      ap[j] = ok ? (gptr)x + ((row0 + xx) * C + c0) * (long)sizeof(T) : (gptr)zero;
      astep[j] = ok ? rs : 0u;
    }
    typedef __attribute__((address_space(1))) T* optr;
    optr yo = BNE ? (optr)y + (((size_t)b * H + r + (size_t)k0 * dil) * W + w0) * C + c0 : nullptr;
    // row q of the class into a load buffer (zeros unless it is in the image and this segment needs it); one row step down
    auto fetch = [&](u32x2 (&raw)[NC], int q) __attribute__((always_inline)) {
      if (q >= 0 && q < nr && q <= k1) {
#pragma unroll
        for (int j = 0; j < NC; ++j) raw[j] = *(const __attribute__((address_space(1))) u32x2*)ap[j];
      } else {
#pragma unroll
        for (int j = 0; j < NC; ++j) raw[j] = u32x2{0u, 0u};
      }
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        ap[j] += astep[j];
        // opaque to the optimiser: it would otherwise keep ap[j] + n astep[j] for every step n of the unrolled walk (spills)
        asm("" : "+v"(ap[j]));
      }
    };
    // One arriving row q of the class, converted out of `raw` (which then takes row q + DEPTH), feeds three output rows: it
    // completes row q - 1 (its ky = 2 taps; A), is the middle row of row q (ky = 1; B) and opens row q + 1 (bias + its
    // ky = 0 taps; C) -- each output row meets its input rows in the order ky = 0, 1, 2.  Row q - 1 then goes out.
    auto step = [&](f32x2 (&aa)[kPX][V2], f32x2 (&ab)[kPX][V2], f32x2 (&ac)[kPX][V2], u32x2 (&raw)[NC], int q, auto parts)
                    __attribute__((always_inline)) {
      constexpr int PARTS = decltype(parts)::value;      // bit 0: A and the output, bit 1: B, bit 2: C
      f32x2 row[NC][V2];
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        row[j][0] = widen2<T>(raw[j].x);
        row[j][1] = widen2<T>(raw[j].y);
      }
      fetch(raw, q + DEPTH);
#pragma unroll
      for (int j = 0; j < NC; ++j)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int p = j - kx;                          // output pixel fed by column j through tap kx
          if (p < 0 || p >= kPX) continue;
#pragma unroll
          for (int i = 0; i < V2; ++i) {
            if constexpr ((PARTS & 1) != 0) aa[p][i] = __builtin_elementwise_fma(wr[6 + kx][i], row[j][i], aa[p][i]);
            if constexpr ((PARTS & 2) != 0) ab[p][i] = __builtin_elementwise_fma(wr[3 + kx][i], row[j][i], ab[p][i]);
            if constexpr ((PARTS & 4) != 0) ac[p][i] = __builtin_elementwise_fma(wr[kx][i], row[j][i], kx == 0 ? bs[i] : ac[p][i]);
          }
        }
      if constexpr ((PARTS & 1) != 0) {
#pragma unroll
        for (int p = 0; p < kPX; ++p)
          if (w0 + p * dil < W) {
            // the ROUNDED convolution result (what the unfused path stores and reads back) enters the sums / the BatchNorm
            unsigned o[V2];
#pragma unroll
            for (int i = 0; i < V2; ++i) {
              const f32x2 rv = widen2<T>(VecIO<T>::pack(aa[p][i].x, aa[p][i].y));
              if constexpr (BNE) {
                const f32x2 z = __builtin_elementwise_fma(rv, bsc[i], bsh[i]);
                o[i] = VecIO<T>::pack((bn.relu && z.x <= 0.f) ? 0.f : z.x, (bn.relu && z.y <= 0.f) ? 0.f : z.y);
              } else {
                st0[i] += rv;
                st1[i] = __builtin_elementwise_fma(rv, rv, st1[i]);
              }
            }
            if constexpr (BNE) *(__attribute__((address_space(1))) u32x2*)(yo + p * dc) = u32x2{o[0], o[1]};
          }
        if constexpr (BNE) {
          yo += (size_t)dil * W * C;
          asm("" : "+v"(yo));
        }
      }
    };
    f32x2 a0[kPX][V2], a1[kPX][V2], a2[kPX][V2];
    u32x2 r0[NC], r1[NC];
    constexpr std::integral_constant<int, 4> open_only{};
    constexpr std::integral_constant<int, 6> no_output{};
    constexpr std::integral_constant<int, 7> full{};
    // (pinned per item: left to itself the optimiser keeps a copy of the weights per unrolled step and spills)
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
      for (int i = 0; i < V2; ++i) asm("" : "+v"(wr[k][i]));
    // rows k0 - 1 and k0 complete nothing of this segment; then rows k0 + 1 .. k1, the roles rotating by renaming
    fetch(r0, k0 - 1);
    if constexpr (DEPTH == 2) {
      fetch(r1, k0);
      step(a2, a2, a0, r0, k0 - 1, open_only);
      step(a2, a0, a1, r1, k0, no_output);
      for (int q = k0 + 1;;) {
        step(a0, a1, a2, r0, q, full); if (++q > k1) break;
        step(a1, a2, a0, r1, q, full); if (++q > k1) break;
        step(a2, a0, a1, r0, q, full); if (++q > k1) break;
        step(a0, a1, a2, r1, q, full); if (++q > k1) break;
        step(a1, a2, a0, r0, q, full); if (++q > k1) break;
        step(a2, a0, a1, r1, q, full); if (++q > k1) break;
      }
    } else {
      step(a2, a2, a0, r0, k0 - 1, open_only);
      step(a2, a0, a1, r0, k0, no_output);
      for (int q = k0 + 1;;) {
        step(a0, a1, a2, r0, q, full); if (++q > k1) break;
        step(a1, a2, a0, r0, q, full); if (++q > k1) break;
        step(a2, a0, a1, r0, q, full); if (++q > k1) break;
      }
    }
  }
  if constexpr (STATS != 0) fold_stats<V>(m, cvb, CV, B, H, W, C, st0, st1, sums, spart);
}

// Vector I/O of dwconv3x3_bwd_kernel: 4 channels per lane for every activation type (fp32: VecIO; 16-bit: 8-byte vectors, as
// dwconv3x3_roll_kernel) -- with 8 channels the 72 weights, 72 weight partials, 32 accumulators and 32 values of x do not fit in
// the 256 registers of 2 waves per SIMD (the 8-channel build spilled 356 bytes per lane).
template <typename T>
struct BwdIO : Vec16<T, kRV> {};
template <>
struct BwdIO<float> : VecIO<float> {};

// Backward, both gradients from ONE pass over gy.  With y[p] = sum_d w[d] x[p + d dil]:
//   gx[q] = sum_d w[d] gy[q - d dil]        gw[d] = sum_q x[q] gy[q - d dil]        gb = sum_q gy[q]
// so a thread that holds the 3 x 6 window of gy around its quad q (the window of dwconv3x3_fwd_kernel<FLIP>) needs only the
// 4 vectors of x AT q on top: the window value v at offset ((ky - 1) dil, (kx - 1) dil), k = 3 ky + kx, enters
// gx[q] += w[8 - k] v and gw[8 - k] += x[q] v; the centre row of the window is gb's.  gy, x and gx cross HBM once each (the
// two-kernel form read gy twice and an 18-vector window of x).  Out-of-image window values are zero (select on the packed
// data) and x is zero for the pixels of a quad past the row end, whose gx is not stored.
//  * either launch geometry (dw_map); idle threads stay for the block's fold.
//  * weight / bias partials: registers over the thread's quads -> LDS fold over the block's pixel lanes -> ONE workspace row
//    per block row, ws[row][k][C] (k = 0..8 taps, 9 = bias) -> dwconv3x3_bwd_weight_reduce_kernel in fixed order.  No atomics:
//    bit-reproducible.
//  * GX = false (no input gradient wanted): no weights, no gx accumulators, no store -- the weight-gradient pass alone, the same
//    sums in the same order.
//  * the window is loaded row by row (6 packed vectors in flight), not all 18 at once: the registers go to the 9 x V weights,
//    the 9 x V weight partials and the 4 x V accumulators.
template <typename T, bool GX>
__global__ __launch_bounds__(256, 2) void dwconv3x3_bwd_kernel(const T* __restrict__ x, const T* __restrict__ gy,
                                                               const float* __restrict__ wgt, T* __restrict__ gx,
                                                               float* __restrict__ ws, int B, int H, int W, int C, int dil,
                                                               int cvb, int sliced) {
  typedef BwdIO<T> IO;
  constexpr int V = IO::N, V2 = V / 2;
  const int CV = C / V, WQ = quads_per_row(W, dil);
  const DwMap m = dw_map(sliced, cvb, CV, blockDim.x);                 // (idle threads stay for the block's fold)
  const int c0 = (m.active ? m.cv : 0) * V;
  const int Hd = (H + dil - 1) / dil, h_slots = sliced ? dil * Hd : H;
  f32x2 wr[GX ? 9 : 1][V2];         // wr[k] = w[8 - k]: the weight of window position k in gx
  if constexpr (GX) load_taps<V, true>(wgt, C, c0, wr);
  f32x2 aw[9][V2], ab[V2];          // aw[k]: the partial of gw[8 - k]; adjacent-channel pairs: every multiply-add is one v_pk_fma_f32
#pragma unroll
  for (int i = 0; i < V2; ++i) {
    ab[i] = f32x2{0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 9; ++k) aw[k][i] = f32x2{0.0f, 0.0f};
  }
  const long nquads = m.active ? (long)B * h_slots * WQ : 0;
  for (long quad = m.first; quad < nquads; quad += m.stride) {
    int b, h, w0;
    quad_coords(quad, WQ, h_slots, dil, b, h, w0);
    if (sliced && dil > 1) h = h / Hd + (h % Hd) * dil;  // slot -> row of residue class slot / Hd
    if (h >= H || w0 >= W) continue;
    const size_t img = (size_t)b * H * W * C + c0;
    f32x2 xv[kPX][V2];
    {
      const T* xp = x + img + (size_t)h * W * C;
      typename IO::Raw xraw[kPX];
#pragma unroll
      for (int p = 0; p < kPX; ++p)
        xraw[p] = mask_raw(IO::load_raw(xp + (size_t)min(w0 + p * dil, W - 1) * C), w0 + p * dil < W);
#pragma unroll
      for (int p = 0; p < kPX; ++p) IO::unpack2(xraw[p], xv[p]);
    }
    f32x2 acc[GX ? kPX : 1][V2];
    if constexpr (GX) {
#pragma unroll
      for (int p = 0; p < kPX; ++p)
#pragma unroll
        for (int i = 0; i < V2; ++i) acc[p][i] = f32x2{0.0f, 0.0f};
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int yy = h + (ky - 1) * dil;
      const bool rowok = yy >= 0 && yy < H;
      const T* gr = gy + img + (size_t)min(max(yy, 0), H - 1) * W * C;
      typename IO::Raw raw[kPX + 2];
#pragma unroll
      for (int j = 0; j < kPX + 2; ++j) {
        const int xx = w0 + (j - 1) * dil;
        raw[j] = mask_raw(IO::load_raw(gr + (size_t)min(max(xx, 0), W - 1) * C), rowok && xx >= 0 && xx < W);
      }
#pragma unroll
      for (int j = 0; j < kPX + 2; ++j) {
        f32x2 v[V2];
        IO::unpack2(raw[j], v);
        if (ky == 1 && j >= 1 && j <= kPX) {             // gy at the quad's own pixels (zero past the row end)
#pragma unroll
          for (int i = 0; i < V2; ++i) ab[i] += v[i];
        }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int p = j - kx;                          // pixel of the quad that sees column j at window position kx
          if (p < 0 || p >= kPX) continue;
#pragma unroll
          for (int i = 0; i < V2; ++i) {
            if constexpr (GX) acc[p][i] = __builtin_elementwise_fma(wr[ky * 3 + kx][i], v[i], acc[p][i]);
            aw[ky * 3 + kx][i] = __builtin_elementwise_fma(xv[p][i], v[i], aw[ky * 3 + kx][i]);
          }
        }
      }
    }
    if constexpr (GX) {
      T* gp = gx + img + (size_t)h * W * C;
#pragma unroll
      for (int p = 0; p < kPX; ++p)
        if (w0 + p * dil < W) {
          float o[V];
#pragma unroll
          for (int i = 0; i < V2; ++i) { o[2 * i] = acc[p][i].x; o[2 * i + 1] = acc[p][i].y; }
          IO::store(gp + (size_t)(w0 + p * dil) * C, o);
        }
    }
  }
  // fold the block's pixel lanes: two passes of 5 of the 10 rows (9 taps + bias) through LDS, every thread sums
  // (10 one-row passes with two barriers each and only the first pixel lane summing were a 3-5 us tail)
  __shared__ float red[5][256][V];
  float* wrow = ws + (size_t)m.row * 10 * C;
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 5; ++kk) {
      const int k = pass * 5 + kk;                       // workspace row k: tap k = window position 8 - k
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const f32x2 t = (k < 9) ? aw[k < 9 ? 8 - k : 0][i / 2] : ab[i / 2];
        red[kk][threadIdx.x][i] = (i & 1) ? t.y : t.x;
      }
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 5 * cvb * V; o += 256) {
      const int kk = o / (cvb * V), rem = o - kk * cvb * V, cvj = rem / V, i = rem - cvj * V;
      if (m.cvbase + cvj >= CV) continue;
      float sum = 0.0f;
      for (int p = 0; p < m.pl; ++p) sum += red[kk][p * cvb + cvj][i];
      wrow[(size_t)(pass * 5 + kk) * C + (m.cvbase + cvj) * V + i] = sum;
    }
  }
}

// stage 2: dw[k][c] = sum over stripes (fixed order => deterministic); k = 9 -> bias gradient.
// flags bit0: accumulate into dw/db (they are the parameters' .grad); bit1: dw in parameter layout (C,1,3,3) = [c][k]
// instead of tap-major [k][c]
__global__ __launch_bounds__(256) void dwconv3x3_bwd_weight_reduce_kernel(const float* __restrict__ ws,
                                                                          float* __restrict__ dw,
                                                                          float* __restrict__ db, int C, int stripes,
                                                                          int flags) {
  // 32 columns x 8 stripe segments per workgroup (the stripe dimension has to supply parallelism: 10*C columns are
  // only 50 workgroups of 256 at C = 1280), LDS combine in a fixed order
  __shared__ float part[8][32];
  const int lane = threadIdx.x & 31, seg = threadIdx.x >> 5;
  const int idx = blockIdx.x * 32 + lane;
  float s = 0.0f;
  if (idx < 10 * C) {
#pragma unroll 4
    for (int t = seg; t < stripes; t += 8) s += ws[(size_t)t * 10 * C + idx];
  }
  part[seg][lane] = s;
  __syncthreads();
  if (seg != 0 || idx >= 10 * C) return;
  s = ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) +
      ((part[4][lane] + part[5][lane]) + (part[6][lane] + part[7][lane]));
  float* dst;
  if (idx < 9 * C) {
    const int k = idx / C, c = idx - k * C;
    dst = (flags & 2) ? dw + c * 9 + k : dw + idx;
  } else {
    if (db == nullptr) return;
    dst = db + (idx - 9 * C);
  }
  *dst = (flags & 1) ? *dst + s : s;
}

static inline int pick_cvb(int CV) { return CV >= 64 ? 64 : (CV >= 32 ? 32 : (CV >= 16 ? 16 : 8)); }
// block rows for `nitems` items on `pl` pixel lanes per block, `cap` at the most
static inline int block_rows(long nitems, int pl, long cap) {
  return (int)std::max<long>(1, std::min<long>(cdiv(nitems, pl), cap));
}

// the SLICED geometry (dw_map): one channel slice of CV / 8 vectors per XCD (at least 8 vectors = 128-byte runs per pixel),
// and exactly the blocks that are resident at once -- 2 per CU (216 VGPRs: 2 waves per SIMD), 64 per XCD (or twice that: no
// difference measured) -- so that an XCD's blocks advance through the rows together.
struct SlicedGeom {
  bool on;
  int cvb, grid;
};
// Measured (round 3, tools/kbench.py --only dw, first-generation grid -> sliced): ASPP 40 x 135 x 240 x 1024, dilation 6:
// 1884 -> 1451 us (1422 with 128 blocks per XCD, 1706 with 32); fp32, dilation 12: 361 -> 272 us; 4 x 34 x 60 x 1280: 19.1 ->
// 14.4 us; Mix-FFN + GELU 40 x 34 x 60 x 1280: 160 -> 149 us.  NOT for slices under 16 vectors (512 channels: 128-byte runs
// per pixel, 214 -> 240 us).
static inline SlicedGeom sliced_geom(int CV, long nslots) {
  // workgroups per XCD: 128 was the optimum of the isolated launches; inside the step (three streams share the CUs) 64 is
  // 0.6 ms per step better (152.8 vs 153.4, twice), 32 is 7 ms worse
  constexpr int per_xcd = 64;
  if (CV % 8 != 0 || CV / 8 < 16 || CV / 8 > 64) return SlicedGeom{false, 0, 0};
  const int cvb = CV / 8;
  return SlicedGeom{true, cvb, 8 * block_rows(nslots, 256 / cvb, per_xcd)};
}
constexpr int kMaxStripes = 128;

// items of one pass over a map in quads: the residue-class slots B d ceil(H / d) WQ of the sliced geometry, else B H WQ
static inline long quad_slots(bool sliced, int B, int H, int W, int dil) {
  return (long)B * (sliced ? dil * cdiv(H, dil) : H) * quads_per_row(W, dil);
}

// Launch geometry of dwconv3x3_fwd_kernel for CV channel vectors (16 bytes each): sliced where sliced_geom() has it, else
// channel blocks x block rows, at most 4096 workgroups.
struct FwdGeom {
  dim3 grid;
  int cvb, sliced, rows;           // rows: block rows = rows of the deterministic statistics' partial image
};
static FwdGeom fwd_geom(int CV, int B, int H, int W, int dil) {
  if (SlicedGeom sg = sliced_geom(CV, quad_slots(true, B, H, W, dil)); sg.on) return FwdGeom{dim3(sg.grid), sg.cvb, 1, sg.grid / 8};
  const int cvb = pick_cvb(CV), gx = cdiv(CV, cvb);
  const int gy = block_rows(quad_slots(false, B, H, W, dil), 256 / cvb, (256L * 16) / gx);
  return FwdGeom{dim3(gx, gy), cvb, 0, gy};
}

// a run-time bool as a template argument: fn(std::true_type{}) or fn(std::false_type{})
template <typename Fn>
static inline void with_bool(bool b, Fn&& fn) {
  if (b) fn(std::true_type{});
  else fn(std::false_type{});
}

template <typename T>
static int launch_fwd(const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int C, int dil,
                      int flip, hipStream_t st) {
  const FwdGeom g = fwd_geom(C / VecIO<T>::N, B, H, W, dil);
  with_bool(flip != 0, [&](auto f) {
    hipLaunchKernelGGL((dwconv3x3_fwd_kernel<T, decltype(f)::value>), g.grid, dim3(256), 0, st, (const T*)x, w, bias, (T*)y, B,
                       H, W, C, dil, g.cvb, (T*)nullptr, 1.f, 1.f, g.sliced);
  });
  return check_launch("dwconv3x3_fwd_kernel");
}

template <typename T>
static int launch_fwd_gelu(const void* x, const float* w, const float* bias, void* y, void* ya, int B, int H, int W,
                           int C, hipStream_t st, float xs = 1.f, float oq = 1.f) {
  const FwdGeom g = fwd_geom(C / VecIO<T>::N, B, H, W, 1);
  hipLaunchKernelGGL((dwconv3x3_fwd_kernel<T, false, true>), g.grid, dim3(256), 0, st, (const T*)x, w, bias, (T*)y, B, H, W,
                     C, 1, g.cvb, (T*)ya, xs, oq, g.sliced);
  return check_launch("dwconv3x3_fwd_kernel<gelu>");
}

// convolution stored + its statistics (spart: the deterministic form, one partial row per block row + the ordered column sum)
template <typename T>
static int launch_fwd_stats(const void* x, const float* w, const float* bias, void* y, double* sums, double* spart, int B, int H,
                            int W, int C, int dil, hipStream_t st) {
  const FwdGeom g = fwd_geom(C / VecIO<T>::N, B, H, W, dil);
  hipLaunchKernelGGL((dwconv3x3_fwd_kernel<T, false, false, true>), g.grid, dim3(256), 0, st, (const T*)x, w, bias, (T*)y, B,
                     H, W, C, dil, g.cvb, (T*)nullptr, 1.f, 1.f, g.sliced, sums, spart);
  if (int rc = check_launch("dwconv3x3_fwd_kernel<stats>")) return rc;
  if (spart != nullptr) return ordered_colsum_f64(spart, sums, g.rows, 2 * C, st);
  return RFN_OK;
}

// Launch geometry of dwconv3x3_roll_kernel (16-bit activations, 4 channels per thread): the XCD-sliced grid where
// sliced_geom() has it (slices of C / 8 channels, 64 resident blocks per XCD), else channel blocks x lane blocks.
// `seg`, the rows of a segment: a whole residue class (ceil(H / d) rows: no refill rows at all, the rows above and below a
// class are outside the image) whenever that still leaves every pixel lane of the grid 4 items -- the teacher's ASPP
// (40 x 135 x 240 x 1024: 14 400 / 28 800 / 51 840 items of 23 / 12 / 8 rows on the 512 lanes of a channel slice) is there for every dilation;
// smaller maps are cut down to segments of 8 rows at the least, where the two refill rows are a quarter more loads.
struct RollGeom {
  bool sliced;
  int cvb, gx, gy, seg, rows;      // grid (gx, gy); sliced: gy == 1; rows: block rows = rows of the deterministic partial image
  long nitems;
};
static RollGeom roll_geom(int B, int H, int W, int C, int dil) {
  RollGeom g{};
  const int CV = C / kRV, Hd = cdiv(H, dil);
  const SlicedGeom sg = sliced_geom(C / 8, 1L << 30);
  long cap;                                                                   // block rows at the most
  if (sg.on) g.sliced = true, g.cvb = 2 * sg.cvb, cap = sg.grid / 8;
  else g.cvb = pick_cvb(CV), g.gx = cdiv(CV, g.cvb), cap = (256L * 16) / g.gx;
  const int pl = 256 / g.cvb;
  const long per_seg = (long)B * dil * quads_per_row(W, dil);
  const long want = std::max<long>(1, cdiv(4 * cap * pl, per_seg));           // segments per class for 4 items per lane
  g.seg = (int)std::min<long>(Hd, std::max<long>(8, cdiv(Hd, want)));
  g.nitems = per_seg * cdiv(Hd, g.seg);
  g.rows = block_rows(g.nitems, pl, cap);
  if (sg.on) g.gx = 8 * g.rows, g.gy = 1;
  else g.gy = g.rows;
  return g;
}

// STATS 2: statistics only; BNE: convolution + BatchNorm + activation from complete statistics
template <typename T, int STATS, bool BNE>
static int launch_roll(const void* x, const float* w, const float* bias, void* y, double* sums, int B, int H, int W, int C,
                       int dil, hipStream_t st, BnEpi bn, double* spart) {
  const void* zero_line = zero_page();       // its first 16 bytes: what a tap left or right of the image reads
  if (zero_line == nullptr) return fail(RFN_ELAUNCH, "dwconv3x3_roll_kernel: zero line symbol");
  const RollGeom g = roll_geom(B, H, W, C, dil);
  RFN_REQUIRE(g.nitems < (1L << 30) && (long)dil * W * C * (long)sizeof(T) < (1L << 32),
              "dwconv3x3_roll_kernel: B=%d H=%d W=%d C=%d dilation=%d too large", B, H, W, C, dil);
  hipLaunchKernelGGL((dwconv3x3_roll_kernel<T, STATS, BNE, kRollDepth<T>>), dim3(g.gx, g.gy), dim3(256), 0, st, (const T*)x, w, bias, (T*)y, B, H,
                     W, C, dil, g.cvb, g.seg, g.sliced ? 1 : 0, sums, bn, spart, zero_line);
  if (int rc = check_launch("dwconv3x3_roll_kernel")) return rc;
  if (spart != nullptr) return ordered_colsum_f64(spart, sums, g.rows, 2 * C, st);
  return RFN_OK;
}

// block rows of the statistics launches for 16-bit activations: the larger of the two bodies' (one workspace size serves
// rfn_dwconv3x3_nhwc_fwd_stats_det and rfn_dwconv3x3_nhwc_stats_det)
static int dw_stats_rows(int B, int H, int W, int C, int dil) {
  return std::max(roll_geom(B, H, W, C, dil).rows, fwd_geom(C / 8, B, H, W, dil).rows);
}

// Launch geometry of dwconv3x3_bwd_kernel (gx == nullptr: the weight / bias gradient alone) + the ordered reduction.
//  * the XCD-sliced residue-class grid where sliced_geom() has it for 16-byte vectors, as roll_geom() (a gy row's three uses
//    stay in one XCD's L2): at most 64 block rows = workspace rows.
//  * else channel blocks x block rows.  The workspace holds kMaxStripes rows, so the block rows cannot supply the parallelism
//    on their own: the channel blocks are made as narrow as it takes (down to 8 vectors = 128-byte runs per pixel) for 4 of
//    them -- 512 workgroups, two per CU, at the row cap -- and a narrow block has more pixel lanes to fold in LDS, so the same
//    workgroups write FEWER workspace rows (a row is 10 C floats however the channels are split).  Stage 3 of the student
//    (4 x 34 x 60 x 1280 bf16): 64 rows = 3.3 MB of partials where the two-kernel form wrote 128 rows = 6.5 MB.
template <typename T>
static int launch_bwd(const void* x, const void* gy, const float* w, void* gx, float* dw, float* db, float* ws, int B, int H,
                      int W, int C, int dil, int flags, hipStream_t st) {
  constexpr int V = BwdIO<T>::N, V16 = 16 / (int)sizeof(T);   // channels per lane; per 16-byte vector, sliced_geom()'s unit
  const int CV = C / V;
  const SlicedGeom sg = sliced_geom(C / V16, 1L << 30);
  int cvb, rows;
  dim3 grid;
  if (sg.on) {
    cvb = sg.cvb * (V16 / V);
    rows = block_rows(quad_slots(true, B, H, W, dil), 256 / cvb, sg.grid / 8);
    grid = dim3(8 * rows);
  } else {
    cvb = pick_cvb(CV);
    while (cvb > 8 && cdiv(CV, cvb) < 4) cvb >>= 1;
    const int gxb = cdiv(CV, cvb);
    rows = block_rows(quad_slots(false, B, H, W, dil), 256 / cvb, std::min<long>(kMaxStripes, std::max<long>(1, (256L * 8) / gxb)));
    grid = dim3(gxb, rows);
  }
  with_bool(gx != nullptr, [&](auto want_gx) {
    hipLaunchKernelGGL((dwconv3x3_bwd_kernel<T, decltype(want_gx)::value>), grid, dim3(256), 0, st, (const T*)x, (const T*)gy, w,
                       (T*)gx, ws, B, H, W, C, dil, cvb, sg.on ? 1 : 0);
  });
  if (int rc = check_launch("dwconv3x3_bwd_kernel")) return rc;
  hipLaunchKernelGGL(dwconv3x3_bwd_weight_reduce_kernel, dim3(cdiv(10L * C, 32)), dim3(256), 0, st, ws, dw, db, C, rows, flags);
  return check_launch("dwconv3x3_bwd_weight_reduce_kernel");
}

}  // namespace rfn

using namespace rfn;

extern "C" {
int rfn_dwconv3x3_nhwc_fwd(const void* x, const float* weight, const float* bias, void* y, int B, int H, int W, int C,
                           int dilation, int dtype, int flip, rfn_stream_t stream) {
  RFN_REQUIRE(x && weight && y, "rfn_dwconv3x3_nhwc_fwd: null pointer");
  RFN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && dilation > 0, "rfn_dwconv3x3_nhwc_fwd: bad size");
  if (dtype == 0) {
    RFN_REQUIRE(C % 4 == 0, "rfn_dwconv3x3_nhwc_fwd: C must be a multiple of 4 for f32 (got %d)", C);
    return launch_fwd<float>(x, weight, bias, y, B, H, W, C, dilation, flip, (hipStream_t)stream);
  }
  RFN_REQUIRE(C % 8 == 0, "rfn_dwconv3x3_nhwc_fwd: C must be a multiple of 8 for 16-bit activations (got %d)", C);
  return dt_one(dtype, "rfn_dwconv3x3_nhwc_fwd", [&](auto t) {
    return launch_fwd<typename decltype(t)::type>(x, weight, bias, y, B, H, W, C, dilation, flip, (hipStream_t)stream);
  });
}

// rfn_dwconv3x3_nhwc_fwd (bf16 / f16) that also leaves the BatchNorm statistics of its result in `sums` (2 C + 1 doubles: sum,
// sum of squares, rows -- the buffer of rfn_bn_stats_fwd, zeroed here): the statistics pass over the result is not needed
int rfn_dwconv3x3_nhwc_fwd_stats(const void* x, const float* weight, const float* bias, void* y, double* sums, int B, int H,
                                 int W, int C, int dilation, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && weight && y && sums, "rfn_dwconv3x3_nhwc_fwd_stats: null pointer");
  RFN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && dilation > 0, "rfn_dwconv3x3_nhwc_fwd_stats: bad size");
  RFN_REQUIRE(C % 8 == 0, "rfn_dwconv3x3_nhwc_fwd_stats: C %% 8 == 0");
  return dt16_type(dtype, "rfn_dwconv3x3_nhwc_fwd_stats", [&](auto t) {
    RFN_REFUSE_NONDET(true, "rfn_dwconv3x3_nhwc_fwd_stats", "dwconv3x3_fwd_kernel<stats>, fp64 atomics (use rfn_dwconv3x3_nhwc_fwd_stats_det)");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = zero_async(sums, (2 * (size_t)C + 1) * sizeof(double), st)) return rc;
    return launch_fwd_stats<typename decltype(t)::type>(x, weight, bias, y, sums, nullptr, B, H, W, C, dilation, st);
  });
}

// Deterministic forms of rfn_dwconv3x3_nhwc_fwd_stats / rfn_dwconv3x3_nhwc_stats: every block row stores its 2 C partial sums
// into `workspace` (rfn_dwconv3x3_stats_det_workspace_bytes(B, H, W, C, dilation) bytes, no need to zero it) and a second launch
// adds the rows in row order.  Same convolution, same `sums` layout.
unsigned long rfn_dwconv3x3_stats_det_workspace_bytes(int B, int H, int W, int C, int dilation) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || dilation <= 0) return 0;
  return (unsigned long)dw_stats_rows(B, H, W, C, dilation) * 2 * C * sizeof(double);
}

int rfn_dwconv3x3_nhwc_fwd_stats_det(const void* x, const float* weight, const float* bias, void* y, double* sums, void* workspace,
                                     int B, int H, int W, int C, int dilation, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && weight && y && sums && workspace, "rfn_dwconv3x3_nhwc_fwd_stats_det: null pointer");
  RFN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && dilation > 0, "rfn_dwconv3x3_nhwc_fwd_stats_det: bad size");
  RFN_REQUIRE(C % 8 == 0, "rfn_dwconv3x3_nhwc_fwd_stats_det: C %% 8 == 0");
  return dt16_type(dtype, "rfn_dwconv3x3_nhwc_fwd_stats_det", [&](auto t) {
    return launch_fwd_stats<typename decltype(t)::type>(x, weight, bias, y, sums, (double*)workspace, B, H, W, C, dilation,
                                                        (hipStream_t)stream);
  });
}

int rfn_dwconv3x3_nhwc_stats_det(const void* x, const float* weight, const float* bias, double* sums, void* workspace, int B, int H,
                                 int W, int C, int dilation, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && weight && sums && workspace, "rfn_dwconv3x3_nhwc_stats_det: null pointer");
  RFN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && dilation > 0, "rfn_dwconv3x3_nhwc_stats_det: bad size");
  RFN_REQUIRE(C % 8 == 0, "rfn_dwconv3x3_nhwc_stats_det: C %% 8 == 0");
  return dt16_type(dtype, "rfn_dwconv3x3_nhwc_stats_det", [&](auto t) {
    return launch_roll<typename decltype(t)::type, 2, false>(x, weight, bias, nullptr, sums, B, H, W, C, dilation,
                                                             (hipStream_t)stream, BnEpi{}, (double*)workspace);
  });
}

// Gradient-free depthwise 3x3 -> BatchNorm(batch statistics) -> ReLU in two passes over the INPUT (bf16 / f16):
//   rfn_dwconv3x3_nhwc_stats        sums <- (sum, sum of squares, rows) of the rounded convolution result, nothing stored;
//   rfn_dwconv3x3_bn_act_nhwc_fwd   y = act(bn(conv(x))) with the statistics in `sums` (between the two a SyncBatchNorm
//                                   all-reduces `sums`); running_mean / running_var (may be NULL) updated as rfn_bn_apply_fwd.
int rfn_dwconv3x3_nhwc_stats(const void* x, const float* weight, const float* bias, double* sums, int B, int H, int W, int C,
                             int dilation, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && weight && sums, "rfn_dwconv3x3_nhwc_stats: null pointer");
  RFN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && dilation > 0, "rfn_dwconv3x3_nhwc_stats: bad size");
  RFN_REQUIRE(C % 8 == 0, "rfn_dwconv3x3_nhwc_stats: C %% 8 == 0");
  return dt16_type(dtype, "rfn_dwconv3x3_nhwc_stats", [&](auto t) {
    RFN_REFUSE_NONDET(true, "rfn_dwconv3x3_nhwc_stats", "dwconv3x3_roll_kernel<stats>, fp64 atomics (use rfn_dwconv3x3_nhwc_stats_det)");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = zero_async(sums, (2 * (size_t)C + 1) * sizeof(double), st)) return rc;
    return launch_roll<typename decltype(t)::type, 2, false>(x, weight, bias, nullptr, sums, B, H, W, C, dilation, st, BnEpi{}, nullptr);
  });
}

int rfn_dwconv3x3_bn_act_nhwc_fwd(const void* x, const float* weight, const float* bias, const float* gamma, const float* beta,
                                  const double* sums, float* running_mean, float* running_var, void* y, int B, int H, int W,
                                  int C, int dilation, float eps, float momentum, int relu, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && weight && sums && y, "rfn_dwconv3x3_bn_act_nhwc_fwd: null pointer");
  RFN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && dilation > 0, "rfn_dwconv3x3_bn_act_nhwc_fwd: bad size");
  RFN_REQUIRE(C % 8 == 0 && (relu == 0 || relu == 1), "rfn_dwconv3x3_bn_act_nhwc_fwd: C %% 8 == 0, relu 0 / 1");
  BnEpi bn{gamma, beta, running_mean, running_var, eps, momentum, relu};
  return dt16_type(dtype, "rfn_dwconv3x3_bn_act_nhwc_fwd", [&](auto t) {
    return launch_roll<typename decltype(t)::type, 0, true>(x, weight, bias, y, const_cast<double*>(sums), B, H, W, C, dilation,
                                                            (hipStream_t)stream, bn, nullptr);
  });
}

int rfn_dwconv3x3_gelu_nhwc_fwd(const void* x, const float* weight, const float* bias, void* y_pre, void* y_act, int B,
                                int H, int W, int C, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && weight && y_act, "rfn_dwconv3x3_gelu_nhwc_fwd: null pointer");
  RFN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "rfn_dwconv3x3_gelu_nhwc_fwd: bad size");
  if (dtype == 0) {
    RFN_REQUIRE(C % 4 == 0, "rfn_dwconv3x3_gelu_nhwc_fwd: C must be a multiple of 4 for f32 (got %d)", C);
    return launch_fwd_gelu<float>(x, weight, bias, y_pre, y_act, B, H, W, C, (hipStream_t)stream);
  }
  RFN_REQUIRE(C % 8 == 0, "rfn_dwconv3x3_gelu_nhwc_fwd: C must be a multiple of 8 for 16-bit activations (got %d)", C);
  return dt_one(dtype, "rfn_dwconv3x3_gelu_nhwc_fwd", [&](auto t) {
    return launch_fwd_gelu<typename decltype(t)::type>(x, weight, bias, y_pre, y_act, B, H, W, C, (hipStream_t)stream);
  });
}

int rfn_dwconv3x3_gelu_nhwc_fwd_f8(const void* x8, const float* weight, const float* bias, void* y8, int B, int H, int W, int C,
                                   float x_scale, float out_q, rfn_stream_t stream) {
  RFN_REQUIRE(x8 && weight && y8, "rfn_dwconv3x3_gelu_nhwc_fwd_f8: null pointer");
  RFN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "rfn_dwconv3x3_gelu_nhwc_fwd_f8: bad size (C %% 8)");
  return launch_fwd_gelu<f8e4m3>(x8, weight, bias, nullptr, y8, B, H, W, C, (hipStream_t)stream, x_scale, out_q);
}

unsigned long rfn_dwconv3x3_bwd_weight_workspace_bytes(int C) {
  return (unsigned long)kMaxStripes * 10ul * (unsigned long)(C > 0 ? C : 0) * sizeof(float);
}

// Backward of rfn_dwconv3x3_nhwc_fwd: grad_x and grad_weight / grad_bias from one pass over grad_y (dwconv3x3_bwd_kernel);
// grad_x == NULL (rfn_dwconv3x3_nhwc_bwd_weight): the parameter gradients alone.
static int dw_bwd(const char* who, const void* x, const void* grad_y, const float* weight, void* grad_x, float* grad_weight,
                  float* grad_bias, void* workspace, int B, int H, int W, int C, int dilation, int dtype, int flags,
                  hipStream_t st) {
  RFN_REQUIRE(x && grad_y && grad_weight && workspace, "%s: null pointer", who);
  RFN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && dilation > 0, "%s: bad size", who);
  if (dtype == 0) {
    RFN_REQUIRE(C % 4 == 0, "%s: C must be a multiple of 4 for f32", who);
    return launch_bwd<float>(x, grad_y, weight, grad_x, grad_weight, grad_bias, (float*)workspace, B, H, W, C, dilation, flags, st);
  }
  RFN_REQUIRE(C % 8 == 0, "%s: C must be a multiple of 8 for 16-bit activations", who);
  return dt_one(dtype, who, [&](auto t) {
    return launch_bwd<typename decltype(t)::type>(x, grad_y, weight, grad_x, grad_weight, grad_bias, (float*)workspace, B, H, W, C,
                                                  dilation, flags, st);
  });
}

int rfn_dwconv3x3_nhwc_bwd_weight(const void* x, const void* grad_y, float* grad_weight, float* grad_bias,
                                  void* workspace, int B, int H, int W, int C, int dilation, int dtype, int flags,
                                  rfn_stream_t stream) {
  return dw_bwd("rfn_dwconv3x3_nhwc_bwd_weight", x, grad_y, nullptr, nullptr, grad_weight, grad_bias, workspace, B, H, W, C,
                dilation, dtype, flags, (hipStream_t)stream);
}

int rfn_dwconv3x3_nhwc_bwd(const void* x, const void* grad_y, const float* weight_tap_major, void* grad_x, float* grad_weight,
                           float* grad_bias, void* workspace, int B, int H, int W, int C, int dilation, int dtype, int flags,
                           rfn_stream_t stream) {
  RFN_REQUIRE(weight_tap_major && grad_x, "rfn_dwconv3x3_nhwc_bwd: null pointer");
  return dw_bwd("rfn_dwconv3x3_nhwc_bwd", x, grad_y, weight_tap_major, grad_x, grad_weight, grad_bias, workspace, B, H, W, C,
                dilation, dtype, flags, (hipStream_t)stream);
}

}  // extern "C"
