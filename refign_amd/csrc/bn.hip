// refign_amd/csrc/bn.hip -- training-mode BatchNorm2d (+ ReLU) on channels-last 16-bit tensors, forward and backward:
// the norm + activation of every ConvBNReLU of the decode heads (models/modules.py:16-56; daformer.py:65-126,
// segformer.py:62-70), which run with BATCH statistics in the student AND in the EMA teacher.
//
//   forward   stats pass : sums[0][c] = sum_t x[t,c], sums[1][c] = sum_t x[t,c]^2          (fp64, pre-zeroed)
//             apply pass : y = relu?( (x - mean) * rstd * gamma + beta ), running statistics updated by block 0
//   backward  stats pass : sums[0][c] = sum_t g'[t,c], sums[1][c] = sum_t g'[t,c] * xhat[t,c],  g' = g * (y > 0)
//             apply pass : dx = gamma * rstd * ( g' - (sums[0] + xhat * sums[1]) / T )
// The two-pass split is the data dependence of BatchNorm itself (3 tensor passes forward, 5 backward -- what any
// implementation moves); what is fused away are the separate ReLU / ReLU-backward passes and the per-call
// normalisation-constant kernels.  Lanes run along channels (16-byte vectors), rows are strided over lanes.
//
// The forward sums are DOUBLES from the first addition to the atomics: the variance is E[x^2] - mean^2, which cancels
// catastrophically in fp32 once |mean| >> std over ~1e6 rows (torch's BatchNorm uses Welford / two passes for that
// reason); in fp64 the one-pass formula has 29 more bits than the 16-bit inputs can use, and the order of the atomics no
// longer shows in the fp32 constants derived from the sums.  The kernels stay HBM-bound (16 fp64 operations per 16-byte
// load).  The backward sums have no cancellation and stay fp32.
//
// Data parallelism (SyncBatchNorm, torch/nn/modules/_functions.py: the reference trains with `sync_batchnorm: True`): the
// statistics buffer is 2 C + 1 doubles, the last one the number of rows the sums were taken over -- the stats pass adds
// its own T there -- so that ONE all-reduce (SUM) of the buffer between the stats pass and the apply pass turns local
// statistics into global ones; the apply passes normalise with the count they find in the buffer, never with T.  The
// four phases are separate entry points for that (rfn_bn_stats_fwd / _apply_fwd / _stats_bwd / _apply_bwd); the
// parameter gradients are the LOCAL backward sums (read before the exchange), as in SyncBatchNorm.
#include <hip/hip_bf16.h>

#include <type_traits>

#include "common.h"
#include "elem.h"

namespace rfn {

// per-channel constants from the forward sums
__device__ __forceinline__ float batch_var(const double* sums, int C, int c, double invT, float& mean) {
  // invT = 1 / sums[2 C]: the (global) number of rows behind the sums
  const double m = sums[c] * invT;
  mean = (float)m;
  return (float)fmax(sums[C + c] * invT - m * m, 0.0);
}
__device__ __forceinline__ void norm_consts(const double* sums, int C, int c, double invT, float eps, float& mean, float& rstd) {
  rstd = rsqrtf(batch_var(sums, C, c, invT, mean) + eps);
}

// The operands of the `_ext` kernels (the decode heads' Dropout2d folded in, and grad_y read in place from a channel slice):
//   drop  (B, C) multipliers in the activation dtype, sample = row / rps; nullptr: none.  Forward: y = round16(act(bn(x))) * drop,
//         rounded again by the store -- the bits of the 16-bit y followed by ATen's 16-bit mul.  Backward: g = round16(g * drop)
//         as it is loaded -- what that mul's backward stored.
//   ldg   row pitch of grad_y in elements (C: dense).
struct BnExt {
  const uint16_t* drop;
  long rps, ldg;
};

// sample index of a row, kept by addition (rows advance by the grid's stride, which may exceed a sample in small launches)
struct SampleCursor {
  long b, rem;
  __device__ __forceinline__ SampleCursor(long t, long rps) : b(t / rps), rem(t % rps) {}
  __device__ __forceinline__ void advance(long by, long rps) {
    rem += by;
    while (rem >= rps) {
      rem -= rps;
      ++b;
    }
  }
};

// g <- round16(g * drop[b]): the gradient the dropout multiply's backward hands to BatchNorm
template <int DT>
__device__ __forceinline__ void drop_grad(const uint16_t* __restrict__ drop, long b, int C, int c0, float (&gv)[8]) {
  float dv[8];
  load8<DT>(drop + b * C + c0, dv);
#pragma unroll
  for (int i = 0; i < 8; ++i) gv[i] = round_to<DT>(gv[i] * dv[i]);
}

// BWD = false: sums of x and x^2.  BWD = true: sums of g' and g' * xhat (fwd_sums give mean / rstd, gamma / beta the sign of y)
// EXT (backward only): grad_y at a row pitch and / or multiplied by the dropout noise (BnExt)
template <int DT, bool BWD, bool EXT>
__device__ __forceinline__ void bn_stats_body(const uint16_t* __restrict__ x, const uint16_t* __restrict__ g,
                                              const double* __restrict__ fwd_sums, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, void* __restrict__ sums_, long T,
                                              int C, int cvb, float eps, int relu, float slope,
                                              void* __restrict__ part_, const BnExt ext) {
  static_assert(BWD || !EXT, "the forward statistics have no extended form");
  const long ldg = EXT ? ext.ldg : C;
  using ST = typename std::conditional<BWD, float, double>::type;      // forward sums: doubles (header)
  ST* __restrict__ sums = (ST*)sums_;
  // deterministic form: part[gridDim.y][2 C], one row per workgroup row with plain stores (every element is written);
  // ordered_colsum adds the rows in row order afterwards
  ST* __restrict__ part = (ST*)part_;
  __shared__ ST red[2][256][8];
  const int CV = C / 8, pl = 256 / cvb;
  const int cv = blockIdx.x * cvb + threadIdx.x % cvb, rl = threadIdx.x / cvb;
  ST s0[8] = {0}, s1[8] = {0};
  if (cv < CV) {
    const int c0 = cv * 8;
    float mean[8], a[8], b[8];
    if (BWD) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float r;
        norm_consts(fwd_sums, C, c0 + i, 1.0 / fwd_sums[2 * C], eps, mean[i], r);
        a[i] = r;                                                       // xhat = (x - mean) * rstd
        b[i] = (gamma ? gamma[c0 + i] : 1.f);
      }
    }
    float bt[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) bt[i] = (BWD && beta) ? beta[c0 + i] : 0.f;
    auto accumulate = [&](const float (&xv)[8], const float (&gv)[8]) {
      if (!BWD) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          s0[i] += (ST)xv[i];
          s1[i] += (ST)xv[i] * (ST)xv[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float xh = (xv[i] - mean[i]) * a[i];
          const float z = xh * b[i] + bt[i];
          const float gp = (relu && z <= 0.f) ? slope * gv[i] : gv[i];
          s0[i] += gp;
          s1[i] += gp * xh;
        }
      }
    };
    // four rows per iteration, their loads issued together: one row at a time (two 16-byte loads in flight per thread) ran at
    // 1.5-2.1 TB/s on the decode head's backward statistics (section 4.5 of DESIGN.md: memory-level parallelism per thread)
    const long stride = (long)gridDim.y * pl;
    long t = (long)blockIdx.y * pl + rl;
    const bool dropped = EXT && ext.drop != nullptr;
    SampleCursor cur(dropped ? t : 0, dropped ? ext.rps : 1);
    for (; t + 3 * stride < T; t += 4 * stride) {
      float xv[4][8], gv[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        load8<DT>(x + (t + u * stride) * C + c0, xv[u]);
        if (BWD) load8<DT>(g + (t + u * stride) * ldg + c0, gv[u]);
      }
      if (dropped) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          drop_grad<DT>(ext.drop, cur.b, C, c0, gv[u]);
          cur.advance(stride, ext.rps);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) accumulate(xv[u], gv[u]);
    }
    for (; t < T; t += stride) {
      float xv[8], gv[8];
      load8<DT>(x + t * C + c0, xv);
      if (BWD) load8<DT>(g + t * ldg + c0, gv);
      if (dropped) {
        drop_grad<DT>(ext.drop, cur.b, C, c0, gv);
        cur.advance(stride, ext.rps);
      }
      accumulate(xv, gv);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    red[0][threadIdx.x][i] = s0[i];
    red[1][threadIdx.x][i] = s1[i];
  }
  __syncthreads();
  // thread (which, channel vector, element): sum over the row lanes, one atomic per channel
  for (int idx = threadIdx.x; idx < 2 * cvb * 8; idx += 256) {
    const int which = idx / (cvb * 8), rem = idx % (cvb * 8), v = rem / 8, e = rem % 8;
    const int cvg = blockIdx.x * cvb + v;
    if (cvg >= CV) continue;
    ST sum = 0;
    for (int r = 0; r < pl; ++r) sum += red[which][r * cvb + v][e];
    if (part != nullptr) part[((long)blockIdx.y * 2 + which) * C + cvg * 8 + e] = sum;
    else atomicAdd(sums + which * C + cvg * 8 + e, sum);
  }
  if (!BWD && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    if (part != nullptr) sums[2 * C] = (ST)T;
    else atomicAdd(sums + 2 * C, (ST)T);
  }
}

template <int DT, bool BWD>
__global__ __launch_bounds__(256) void bn_stats_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ g,
                                                       const double* __restrict__ fwd_sums, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, void* __restrict__ sums_, long T,
                                                       int C, int cvb, float eps, int relu, float slope,
                                                       void* __restrict__ part_ = nullptr) {
  bn_stats_body<DT, BWD, false>(x, g, fwd_sums, gamma, beta, sums_, T, C, cvb, eps, relu, slope, part_, BnExt{nullptr, 1, 0});
}

template <int DT>
__global__ __launch_bounds__(256) void bn_stats_bwd_ext_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ g,
                                                               const double* __restrict__ fwd_sums,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               void* __restrict__ sums_, long T, int C, int cvb, float eps,
                                                               int relu, float slope, void* __restrict__ part_, BnExt ext) {
  bn_stats_body<DT, true, true>(x, g, fwd_sums, gamma, beta, sums_, T, C, cvb, eps, relu, slope, part_, ext);
}

// EXT: BnExt's multiplier on the result (forward) or on grad_y (backward), grad_y at a row pitch
template <int DT, bool BWD, bool EXT>
__device__ __forceinline__ void bn_apply_body(const uint16_t* __restrict__ x, const uint16_t* __restrict__ g,
                                              const double* __restrict__ fwd_sums, const float* __restrict__ bwd_sums,
                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                              uint16_t* __restrict__ out, float* __restrict__ running_mean,
                                              float* __restrict__ running_var, long T, int C, int cvb, float eps,
                                              float momentum, int relu, float slope, long ldo, const BnExt ext) {
  const long ldg = EXT ? ext.ldg : C;
  // ldo: row pitch of `out` in elements (C for a dense result; larger when the result is a channel slice of a wider
  // channels-last tensor -- the branches of the ASPP write straight into their concatenation, daformer.py:110-118)
  const int CV = C / 8, pl = 256 / cvb;
  const int cv = blockIdx.x * cvb + threadIdx.x % cvb, rl = threadIdx.x / cvb;
  const double invTd = 1.0 / fwd_sums[2 * C];          // rows behind the statistics (all ranks')
  const float cnt = (float)fwd_sums[2 * C], invT = (float)invTd;
  if (!BWD && running_mean != nullptr && blockIdx.y == 0 && rl == 0 && cv < CV) {
    // running statistics: mean and UNBIASED variance of this batch, as nn.BatchNorm2d
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = cv * 8 + i;
      float mean;
      const float var = batch_var(fwd_sums, C, c, invTd, mean);
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * var * (cnt / fmaxf(cnt - 1.f, 1.f));
    }
  }
  if (cv >= CV) return;
  const int c0 = cv * 8;
  float mean[8], rstd[8], gm[8], bt[8], k0[8], k1[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    norm_consts(fwd_sums, C, c0 + i, invTd, eps, mean[i], rstd[i]);
    gm[i] = gamma ? gamma[c0 + i] : 1.f;
    bt[i] = beta ? beta[c0 + i] : 0.f;
    if (BWD) {
      k0[i] = bwd_sums[c0 + i] * invT;
      k1[i] = bwd_sums[C + c0 + i] * invT;
    }
  }
  const long stride = (long)gridDim.y * pl;
  long t = (long)blockIdx.y * pl + rl;
  const bool dropped = EXT && ext.drop != nullptr;
  SampleCursor cur(dropped ? t : 0, dropped ? ext.rps : 1);
  for (; t < T; t += stride) {
    float xv[8], o[8];
    load8<DT>(x + t * C + c0, xv);
    if (!BWD) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float z = (xv[i] - mean[i]) * rstd[i] * gm[i] + bt[i];
        o[i] = (relu && z <= 0.f) ? slope * z : z;
      }
      if (dropped) {
        float dv[8];
        load8<DT>(ext.drop + cur.b * C + c0, dv);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = round_to<DT>(o[i]) * dv[i];
        cur.advance(stride, ext.rps);
      }
    } else {
      float gv[8];
      load8<DT>(g + t * ldg + c0, gv);
      if (dropped) {
        drop_grad<DT>(ext.drop, cur.b, C, c0, gv);
        cur.advance(stride, ext.rps);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float xh = (xv[i] - mean[i]) * rstd[i];
        const float z = xh * gm[i] + bt[i];
        const float gp = (relu && z <= 0.f) ? slope * gv[i] : gv[i];
        o[i] = gm[i] * rstd[i] * (gp - k0[i] - xh * k1[i]);
      }
    }
    store8<DT>(out + t * ldo + c0, o);
  }
}

template <int DT, bool BWD>
__global__ __launch_bounds__(256) void bn_apply_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ g,
                                                       const double* __restrict__ fwd_sums, const float* __restrict__ bwd_sums,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       uint16_t* __restrict__ out, float* __restrict__ running_mean,
                                                       float* __restrict__ running_var, long T, int C, int cvb, float eps,
                                                       float momentum, int relu, float slope, long ldo) {
  bn_apply_body<DT, BWD, false>(x, g, fwd_sums, bwd_sums, gamma, beta, out, running_mean, running_var, T, C, cvb, eps, momentum,
                                relu, slope, ldo, BnExt{nullptr, 1, 0});
}

template <int DT, bool BWD>
__global__ __launch_bounds__(256) void bn_apply_ext_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ g,
                                                           const double* __restrict__ fwd_sums, const float* __restrict__ bwd_sums,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           uint16_t* __restrict__ out, float* __restrict__ running_mean,
                                                           float* __restrict__ running_var, long T, int C, int cvb, float eps,
                                                           float momentum, int relu, float slope, long ldo, BnExt ext) {
  bn_apply_body<DT, BWD, true>(x, g, fwd_sums, bwd_sums, gamma, beta, out, running_mean, running_var, T, C, cvb, eps, momentum,
                               relu, slope, ldo, ext);
}

static inline int bn_cvb(int CV) { return CV >= 64 ? 64 : (CV >= 32 ? 32 : (CV >= 16 ? 16 : 8)); }

// workgroup rows of a statistics launch (= rows of the deterministic form's partial image)
static inline int bn_stats_rows(long T, int C) {
  const int CV = C / 8, cvb = bn_cvb(CV), gx = cdiv(CV, cvb), pl = 256 / cvb;
  return (int)std::max<long>(1, std::min<long>(cdiv(T, (long)pl * 4), std::max<long>(1, 512 / gx)));
}

template <int DT>
static int bn_launch(bool bwd, bool apply, const void* x, const void* g, const double* fwd_sums, void* sums_or_bwd,
                     const float* gamma, const float* beta, void* out, float* rmean, float* rvar, long T, int C, float eps,
                     float momentum, int relu, float slope, hipStream_t s, long ldo = 0, void* part = nullptr,
                     const BnExt* ext = nullptr) {
  // ext: the `_ext` kernels (same grid, same lane and row mapping; the forward statistics have none)
  if (ldo == 0) ldo = C;
  const int CV = C / 8, cvb = bn_cvb(CV), gx = cdiv(CV, cvb), pl = 256 / cvb;
  // workgroups per launch.  A statistics workgroup ends with 2 x (its channels) atomics on the SAME 2C sums: 512 of them
  // instead of 2048 (129 600 x 256 backward statistics 68 -> 37 us, 1 296 000 x 256 forward 142 -> 116 us); the apply passes
  // 2048 in isolation (191 vs 166 us at 512) -- and 1024 in the step, where three streams share the CUs (end of round 4, together
  // with the GEMM tile threshold and the fused GELU backward: -1.5 ms, profiles/r04_knob_ab.txt).  RFN_BN_STATS_WGS / RFN_BN_WGS.
  static const long wgs_apply = 1024;
  static const long wgs_stats = 512;
  const long wgs = apply ? wgs_apply : wgs_stats;
  const int gy = apply ? (int)std::max<long>(1, std::min<long>(cdiv(T, (long)pl * 4), std::max<long>(1, wgs / gx)))
                       : bn_stats_rows(T, C);
  dim3 grid(gx, gy), block(256);
  if (ext != nullptr) {
    if (!apply)
      hipLaunchKernelGGL((bn_stats_bwd_ext_kernel<DT>), grid, block, 0, s, (const uint16_t*)x, (const uint16_t*)g, fwd_sums, gamma,
                         beta, sums_or_bwd, T, C, cvb, eps, relu, slope, part, *ext);
    else if (bwd)
      hipLaunchKernelGGL((bn_apply_ext_kernel<DT, true>), grid, block, 0, s, (const uint16_t*)x, (const uint16_t*)g, fwd_sums,
                         (const float*)sums_or_bwd, gamma, beta, (uint16_t*)out, nullptr, nullptr, T, C, cvb, eps, momentum, relu,
                         slope, ldo, *ext);
    else
      hipLaunchKernelGGL((bn_apply_ext_kernel<DT, false>), grid, block, 0, s, (const uint16_t*)x, nullptr, fwd_sums, nullptr, gamma,
                         beta, (uint16_t*)out, rmean, rvar, T, C, cvb, eps, momentum, relu, slope, ldo, *ext);
  } else if (!apply) {
    if (bwd)
      hipLaunchKernelGGL((bn_stats_kernel<DT, true>), grid, block, 0, s, (const uint16_t*)x, (const uint16_t*)g, fwd_sums,
                         gamma, beta, sums_or_bwd, T, C, cvb, eps, relu, slope, part);
    else
      hipLaunchKernelGGL((bn_stats_kernel<DT, false>), grid, block, 0, s, (const uint16_t*)x, nullptr, nullptr, nullptr,
                         nullptr, sums_or_bwd, T, C, cvb, eps, relu, slope, part);
  } else {
    if (bwd)
      hipLaunchKernelGGL((bn_apply_kernel<DT, true>), grid, block, 0, s, (const uint16_t*)x, (const uint16_t*)g, fwd_sums,
                         (const float*)sums_or_bwd, gamma, beta, (uint16_t*)out, nullptr, nullptr, T, C, cvb, eps, momentum, relu, slope, ldo);
    else
      hipLaunchKernelGGL((bn_apply_kernel<DT, false>), grid, block, 0, s, (const uint16_t*)x, nullptr, fwd_sums, nullptr,
                         gamma, beta, (uint16_t*)out, rmean, rvar, T, C, cvb, eps, momentum, relu, slope, ldo);
  }
  return check_launch("bn kernel");
}

}  // namespace rfn

extern "C" {
using namespace rfn;

// activation code of the entry points (as rfn_gemm_nt): 0 none, 1 ReLU, 3 LeakyReLU(0.1)
static inline float bn_slope(int act) { return act == 3 ? 0.1f : 0.f; }

static int bn_check(const char* what, long T, int C) {
  RFN_REQUIRE(T >= 1 && C > 0 && C % 8 == 0, "%s: T=%ld C=%d (C %% 8)", what, T, C);
  return RFN_OK;
}

int rfn_bn_stats_fwd(const void* x, double* sums, long T, int C, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && sums, "bn_stats_fwd: null pointer");
  if (int rc = bn_check("bn_stats_fwd", T, C)) return rc;
  return dt16(dtype, "rfn_bn_stats_fwd", [&](auto dt) {
    RFN_REFUSE_NONDET(true, "rfn_bn_stats_fwd", "bn_stats_kernel, fp64 atomics (use rfn_bn_stats_fwd_det)");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = zero_async(sums, (2 * (size_t)C + 1) * sizeof(double), s)) return rc;   // kernel, not a memset node (capi.hip)
    return bn_launch<decltype(dt)::value>(false, false, x, nullptr, nullptr, sums, nullptr, nullptr, nullptr, nullptr, nullptr, T, C,
                                          0.f, 0.f, 0, 0.f, s);
  });
}

// y may be a channel slice of a wider channels-last tensor: ld_y (0 = C) is its row pitch in elements
static int bn_apply_fwd(const char* who, const void* x, const float* gamma, const float* beta, void* y, long ld_y, const double* sums,
                        float* running_mean, float* running_var, long T, int C, float eps, float momentum, int relu, int dtype,
                        rfn_stream_t stream) {
  return dt16(dtype, who, [&](auto dt) {
    return bn_launch<decltype(dt)::value>(false, true, x, nullptr, sums, nullptr, gamma, beta, y, running_mean, running_var, T, C, eps,
                                          momentum, relu != 0, bn_slope(relu), (hipStream_t)stream, ld_y);
  });
}

int rfn_bn_apply_fwd(const void* x, const float* gamma, const float* beta, void* y, const double* sums, float* running_mean,
                     float* running_var, long T, int C, float eps, float momentum, int relu, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && y && sums, "bn_apply_fwd: null pointer");
  if (int rc = bn_check("bn_apply_fwd", T, C)) return rc;
  return bn_apply_fwd("rfn_bn_apply_fwd", x, gamma, beta, y, 0, sums, running_mean, running_var, T, C, eps, momentum, relu, dtype, stream);
}

// rfn_bn_apply_fwd with the result written at a row pitch of ld_y elements (>= C, multiple of 8): y is a channel slice of a
// wider channels-last tensor
int rfn_bn_apply_fwd_ld(const void* x, const float* gamma, const float* beta, void* y, long ld_y, const double* sums,
                        float* running_mean, float* running_var, long T, int C, float eps, float momentum, int relu, int dtype,
                        rfn_stream_t stream) {
  RFN_REQUIRE(x && y && sums, "bn_apply_fwd_ld: null pointer");
  RFN_REQUIRE(ld_y >= C && ld_y % 8 == 0 && ((size_t)y & 15) == 0, "bn_apply_fwd_ld: pitch %ld (>= C = %d, %% 8, 16-byte base)", ld_y, C);
  if (int rc = bn_check("bn_apply_fwd_ld", T, C)) return rc;
  return bn_apply_fwd("rfn_bn_apply_fwd_ld", x, gamma, beta, y, ld_y, sums, running_mean, running_var, T, C, eps, momentum, relu, dtype,
                      stream);
}

// the operands of the extended forms: grad_y's pitch (0 = C) and the dropout multiplier (may be null) -> BnExt
static int bn_ext(const char* who, long ld_g, const void* drop, long rows_per_sample, long T, int C, const void* g, BnExt* ext) {
  RFN_REQUIRE(ld_g == 0 || (ld_g >= C && ld_g % 8 == 0), "%s: pitch %ld (>= C = %d, %% 8)", who, ld_g, C);
  RFN_REQUIRE(g == nullptr || ((size_t)g & 15) == 0, "%s: grad_y needs a 16-byte base", who);
  RFN_REQUIRE(drop == nullptr || (((size_t)drop & 15) == 0 && rows_per_sample >= 1 && T % rows_per_sample == 0),
              "%s: drop needs a 16-byte base and T=%ld a multiple of rows_per_sample=%ld", who, T, rows_per_sample);
  *ext = BnExt{(const uint16_t*)drop, drop ? rows_per_sample : 1, ld_g ? ld_g : (long)C};
  return RFN_OK;
}

// rfn_bn_apply_fwd_ld with Dropout2d folded in: y = round16(relu?(bn(x))) * drop[t / rows_per_sample][c], drop (T / rows_per_sample, C)
// in the activation dtype -- bit for bit the 16-bit result followed by ATen's 16-bit multiply.  ld_y: 0 = C.
int rfn_bn_apply_fwd_drop(const void* x, const float* gamma, const float* beta, void* y, long ld_y, const double* sums,
                          float* running_mean, float* running_var, const void* drop, long rows_per_sample, long T, int C, float eps,
                          float momentum, int relu, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && y && sums && drop, "bn_apply_fwd_drop: null pointer");
  if (int rc = bn_check("bn_apply_fwd_drop", T, C)) return rc;
  RFN_REQUIRE((ld_y == 0 || (ld_y >= C && ld_y % 8 == 0)) && ((size_t)y & 15) == 0, "bn_apply_fwd_drop: pitch %ld (>= C = %d, %% 8, 16-byte base)",
              ld_y, C);
  BnExt ext;
  if (int rc = bn_ext("bn_apply_fwd_drop", 0, drop, rows_per_sample, T, C, nullptr, &ext)) return rc;
  return dt16(dtype, "rfn_bn_apply_fwd_drop", [&](auto dt) {
    return bn_launch<decltype(dt)::value>(false, true, x, nullptr, sums, nullptr, gamma, beta, y, running_mean, running_var, T, C, eps,
                                          momentum, relu != 0, bn_slope(relu), (hipStream_t)stream, ld_y, nullptr, &ext);
  });
}

// the backward statistics launch; workspace != null: the deterministic form's partial rows; ext != null: the extended kernel
static int bn_stats_bwd(const char* who, const void* x, const void* grad_y, const double* fwd_sums, const float* gamma, const float* beta,
                        float* bwd_sums, void* workspace, long T, int C, float eps, int relu, int dtype, hipStream_t s,
                        const BnExt* ext = nullptr) {
  return dt16(dtype, who, [&](auto dt) {
    if (workspace == nullptr) {
      RFN_REFUSE_NONDET(true, "rfn_bn_stats_bwd", "bn_stats_kernel, fp32 atomics (use rfn_bn_stats_bwd_det)");
      if (int rc = zero_async(bwd_sums, 2 * (size_t)C * sizeof(float), s)) return rc;
    }
    return bn_launch<decltype(dt)::value>(true, false, x, grad_y, fwd_sums, bwd_sums, gamma, beta, nullptr, nullptr, nullptr, T, C, eps,
                                          0.f, relu != 0, bn_slope(relu), s, 0, workspace, ext);
  });
}

int rfn_bn_stats_bwd(const void* x, const void* grad_y, const double* fwd_sums, const float* gamma, const float* beta,
                     float* bwd_sums, long T, int C, float eps, int relu, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && grad_y && fwd_sums && bwd_sums, "bn_stats_bwd: null pointer");
  if (int rc = bn_check("bn_stats_bwd", T, C)) return rc;
  return bn_stats_bwd("rfn_bn_stats_bwd", x, grad_y, fwd_sums, gamma, beta, bwd_sums, nullptr, T, C, eps, relu, dtype, (hipStream_t)stream);
}

// Deterministic forms of the two statistics passes: every workgroup row stores its 2 C partial sums into `workspace`
// (rfn_bn_stats_det_workspace_bytes(T, C) bytes, no need to zero it), a second launch adds the rows in row order.
unsigned long rfn_bn_stats_det_workspace_bytes(long T, int C) {
  if (T < 1 || C <= 0 || C % 8 != 0) return 0;
  return (unsigned long)bn_stats_rows(T, C) * 2 * C * sizeof(double);
}

int rfn_bn_stats_fwd_det(const void* x, double* sums, void* workspace, long T, int C, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && sums && workspace, "bn_stats_fwd_det: null pointer");
  if (int rc = bn_check("bn_stats_fwd_det", T, C)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = dt16(dtype, "rfn_bn_stats_fwd_det", [&](auto dt) {
        return bn_launch<decltype(dt)::value>(false, false, x, nullptr, nullptr, sums, nullptr, nullptr, nullptr, nullptr, nullptr, T, C,
                                              0.f, 0.f, 0, 0.f, s, 0, workspace);
      }))
    return rc;
  return ordered_colsum_f64((const double*)workspace, sums, bn_stats_rows(T, C), 2 * C, s);
}

int rfn_bn_stats_bwd_det(const void* x, const void* grad_y, const double* fwd_sums, const float* gamma, const float* beta,
                         float* bwd_sums, void* workspace, long T, int C, float eps, int relu, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && grad_y && fwd_sums && bwd_sums && workspace, "bn_stats_bwd_det: null pointer");
  if (int rc = bn_check("bn_stats_bwd_det", T, C)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = bn_stats_bwd("rfn_bn_stats_bwd_det", x, grad_y, fwd_sums, gamma, beta, bwd_sums, workspace, T, C, eps, relu, dtype, s))
    return rc;
  return ordered_colsum_f32((const float*)workspace, bwd_sums, bn_stats_rows(T, C), 2 * C, s);
}

int rfn_bn_apply_bwd(const void* x, const void* grad_y, const double* fwd_sums, const float* bwd_sums, const float* gamma,
                     const float* beta, void* grad_x, long T, int C, float eps, int relu, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && grad_y && fwd_sums && bwd_sums && grad_x, "bn_apply_bwd: null pointer");
  if (int rc = bn_check("bn_apply_bwd", T, C)) return rc;
  return dt16(dtype, "rfn_bn_apply_bwd", [&](auto dt) {
    return bn_launch<decltype(dt)::value>(true, true, x, grad_y, fwd_sums, (void*)bwd_sums, gamma, beta, grad_x, nullptr, nullptr, T, C,
                                          eps, 0.f, relu != 0, bn_slope(relu), (hipStream_t)stream);
  });
}

// The backward passes with grad_y read at a row pitch of ld_g elements (0 = C; a channel slice of a wider channels-last tensor:
// the ASPP branches read the bottleneck's input gradient in place) and, with drop != NULL, multiplied by the Dropout2d noise as it
// is loaded: g = round16(grad_y * drop[t / rows_per_sample][c]).  Same lane and row mapping as the dense entry points.
int rfn_bn_stats_bwd_ld(const void* x, const void* grad_y, long ld_g, const void* drop, long rows_per_sample, const double* fwd_sums,
                        const float* gamma, const float* beta, float* bwd_sums, long T, int C, float eps, int relu, int dtype,
                        rfn_stream_t stream) {
  RFN_REQUIRE(x && grad_y && fwd_sums && bwd_sums, "bn_stats_bwd_ld: null pointer");
  if (int rc = bn_check("bn_stats_bwd_ld", T, C)) return rc;
  BnExt ext;
  if (int rc = bn_ext("bn_stats_bwd_ld", ld_g, drop, rows_per_sample, T, C, grad_y, &ext)) return rc;
  return bn_stats_bwd("rfn_bn_stats_bwd_ld", x, grad_y, fwd_sums, gamma, beta, bwd_sums, nullptr, T, C, eps, relu, dtype, (hipStream_t)stream,
                      &ext);
}

int rfn_bn_stats_bwd_det_ld(const void* x, const void* grad_y, long ld_g, const void* drop, long rows_per_sample, const double* fwd_sums,
                            const float* gamma, const float* beta, float* bwd_sums, void* workspace, long T, int C, float eps, int relu,
                            int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && grad_y && fwd_sums && bwd_sums && workspace, "bn_stats_bwd_det_ld: null pointer");
  if (int rc = bn_check("bn_stats_bwd_det_ld", T, C)) return rc;
  BnExt ext;
  if (int rc = bn_ext("bn_stats_bwd_det_ld", ld_g, drop, rows_per_sample, T, C, grad_y, &ext)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = bn_stats_bwd("rfn_bn_stats_bwd_det_ld", x, grad_y, fwd_sums, gamma, beta, bwd_sums, workspace, T, C, eps, relu, dtype, s, &ext))
    return rc;
  return ordered_colsum_f32((const float*)workspace, bwd_sums, bn_stats_rows(T, C), 2 * C, s);
}

int rfn_bn_apply_bwd_ld(const void* x, const void* grad_y, long ld_g, const void* drop, long rows_per_sample, const double* fwd_sums,
                        const float* bwd_sums, const float* gamma, const float* beta, void* grad_x, long T, int C, float eps, int relu,
                        int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && grad_y && fwd_sums && bwd_sums && grad_x, "bn_apply_bwd_ld: null pointer");
  if (int rc = bn_check("bn_apply_bwd_ld", T, C)) return rc;
  BnExt ext;
  if (int rc = bn_ext("bn_apply_bwd_ld", ld_g, drop, rows_per_sample, T, C, grad_y, &ext)) return rc;
  return dt16(dtype, "rfn_bn_apply_bwd_ld", [&](auto dt) {
    return bn_launch<decltype(dt)::value>(true, true, x, grad_y, fwd_sums, (void*)bwd_sums, gamma, beta, grad_x, nullptr, nullptr, T, C,
                                          eps, 0.f, relu != 0, bn_slope(relu), (hipStream_t)stream, 0, nullptr, &ext);
  });
}

// one rank: stats + apply back to back (`sums`: 2 C + 1 doubles)
int rfn_bn_train_fwd(const void* x, const float* gamma, const float* beta, void* y, double* sums, float* running_mean,
                     float* running_var, long T, int C, float eps, float momentum, int relu, int dtype,
                     rfn_stream_t stream) {
  RFN_REQUIRE(T > 1, "bn_train_fwd: T=%ld", T);
  if (int rc = rfn_bn_stats_fwd(x, sums, T, C, dtype, stream)) return rc;
  return rfn_bn_apply_fwd(x, gamma, beta, y, sums, running_mean, running_var, T, C, eps, momentum, relu, dtype, stream);
}

int rfn_bn_train_bwd(const void* x, const void* grad_y, const double* fwd_sums, const float* gamma, const float* beta,
                     void* grad_x, float* bwd_sums, long T, int C, float eps, int relu, int dtype, rfn_stream_t stream) {
  if (int rc = rfn_bn_stats_bwd(x, grad_y, fwd_sums, gamma, beta, bwd_sums, T, C, eps, relu, dtype, stream)) return rc;
  return rfn_bn_apply_bwd(x, grad_y, fwd_sums, bwd_sums, gamma, beta, grad_x, T, C, eps, relu, dtype, stream);
}

}  // extern "C"
