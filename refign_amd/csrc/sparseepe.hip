// refign_amd/csrc/sparseepe.hip -- the matcher's evaluation metric in one launch: helpers/metrics.py:68-201 (SparseEPE.update
// and its compute_aucs), which on the host is, per sample, a synchronising count of the valid correspondences, four boolean-index
// selections and 100 torch.quantile calls with a masked mean each -- well over a hundred small launches around a forward whose
// own tail takes microseconds.  Here a workgroup of 1024 lanes owns a sample (at most 8192 correspondences, 8 per lane):
//   1. validity (the four coordinates rounded half to even -- torch.round -- inside [0, w) x [0, h)), the flow and the confidence
//      gathered at the rounded target point, EPE = |(src - trg) - flow| in fp32; the sample's EPE sum (fp64), the four PCK counts
//      and n_valid by a block reduction;
//   2. the oracle curve: keys -EPE (+inf for an invalid point, so the valid ones come first) sorted ascending by a bitonic network
//      in LDS; the 50 thresholds by torch.quantile's fp32 recipe (rank = fp32(q) * fp32(n - 1), lerp between floor and ceil);
//      `key >= threshold` keeps a SUFFIX of the sorted order, found by bisection, and its mean comes from an fp64 scan: every
//      lane sums its 8 consecutive values, the lane sums are scanned over the workgroup, the lane that owns a cut finishes it;
//   3. the sparsification curve: the same with keys -confidence and the EPE travelling with its key;
//   4. both curves over max(oracle) + 1e-6, trapezoid over t / 50, |difference|: fp32 element by element as torch forms it.
// LDS: 8192 keys + 8192 values = 64 KB, no opt-in.  The scan's few hundred bytes of scratch live in the VALUE half, which is free
// by then: the values sit in registers.  No atomics, fixed summation orders: the result is a function of the inputs alone.
#include "common.h"

// Every fp32 value below is formed operation by operation, as the ATen kernels this restates form it: a multiply fused into the
// add or subtract that follows it (the compiler's default; the _rn intrinsics of the headers do not stop it, plain operators under this pragma do) keeps the unrounded
// product -- fma(q, n - 1, -floor(rank)) is not rank - floor(rank) -- which at n - 1 a multiple of 50 moves a point across a
// threshold.
#pragma clang fp contract(off)

namespace rfn {

constexpr int kSeMaxN = 8192, kSeThreads = 1024, kSePer = kSeMaxN / kSeThreads, kSeWaves = kSeThreads / kWave;
constexpr int kSeMaxB = 64, kSeIntervals = 50;

struct SeOffsets {
  int v[kSeMaxB + 1];                          // first row of every sample in the point arrays; travels in the kernel arguments
};

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ascending bitonic sort of key[0, P) (P a power of two), val travelling along when PAIRS
template <bool PAIRS>
__device__ __forceinline__ void se_sort(float* key, float* val, int P, int tid) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int t = tid; t < (P >> 1); t += kSeThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;      // l < P: bit j of i is clear
        const float a = key[i], c = key[l];
        if ((a > c) == ((i & k) == 0)) {
          key[i] = c, key[l] = a;
          if (PAIRS) {
            const float u = val[i];
            val[i] = val[l], val[l] = u;
          }
        }
      }
    }
  }
  __syncthreads();
}

// torch.quantile(key[0, nv), t / 50) for the sorted keys, in fp32 as ATen forms it (quantile_compute + lerp)
__device__ __forceinline__ float se_threshold(const float* key, int nv, int t) {
  const float q = (float)((double)t / (double)kSeIntervals);
  const float rank = q * (float)(nv - 1);
  const float fl = floorf(rank), wgt = rank - fl;
  const int lo = min(max((int)fl, 0), nv - 1), hi = min(max((int)ceilf(rank), 0), nv - 1);
  const float a = key[lo], b = key[hi], d = b - a;
  return wgt < 0.5f ? a + wgt * d : b - d * (1.0f - wgt);
}

// the curve of one sorted order: lane t < 50 returns mean(value | key >= threshold t).  key[0, P) sorted, the nv valid points
// first.  `sd`: the value half of LDS as scratch -- every lane takes its values into registers first.
template <bool PAIRS>
__device__ __forceinline__ float se_curve(const float* key, float* val, int P, int nv, int tid) {
  double* sd = reinterpret_cast<double*>(val);           // [0, 16) wave totals, [16, 66) suffix sums
  int* scut = reinterpret_cast<int*>(sd + 16 + kSeIntervals);
  const int c0 = tid * kSePer, lane = tid & 63, wave = tid >> 6;
  float v[kSePer];
  double ts = 0.0;
#pragma unroll
  for (int e = 0; e < kSePer; ++e) {
    const int i = c0 + e;
    v[e] = i < nv ? (PAIRS ? val[min(i, P - 1)] : -key[min(i, P - 1)]) : 0.0f;      // (nv <= P)
    ts += (double)v[e];
  }
  __syncthreads();                                       // the values are in registers: their half of LDS is scratch now
  double incl = ts;                                      // inclusive scan of the lane sums over the wave, then over the waves
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) sd[wave] = incl;
  if (tid < kSeIntervals) {
    const float thr = se_threshold(key, nv, tid);
    int lo = 0, hi = nv;                                 // first index with key >= thr
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (key[mid] >= thr) hi = mid; else lo = mid + 1;
    }
    scut[tid] = lo;
    sd[16 + tid] = 0.0;                                  // (an empty kept set -- cut == nv -- has no owner below)
  }
  __syncthreads();
  double before = 0.0, total = 0.0;
#pragma unroll
  for (int i = 0; i < kSeWaves; ++i) {
    const double s = sd[i];
    before += i < wave ? s : 0.0;
    total += s;
  }
  const double excl = before + incl - ts;                // sum of the values before this lane's first
  for (int t = 0; t < kSeIntervals; ++t) {
    const int c = scut[t] - c0;
    if (c >= 0 && c < kSePer && scut[t] < nv) {
      double prefix = excl;
#pragma unroll
      for (int e = 0; e < kSePer; ++e) prefix += e < c ? (double)v[e] : 0.0;
      sd[16 + t] = total - prefix;
    }
  }
  __syncthreads();
  float out = 0.0f;
  if (tid < kSeIntervals) out = (float)(sd[16 + tid] / (double)(nv - scut[tid]));     // (empty: 0 / 0 = NaN, torch's mean of nothing)
  __syncthreads();
  return out;
}

__global__ __launch_bounds__(kSeThreads) void sparse_epe_kernel(const float* __restrict__ flow, const float* __restrict__ conf,
                                                                const float2* __restrict__ ps, const float2* __restrict__ pt,
                                                                SeOffsets off, int h, int w, double* __restrict__ rows) {
  __shared__ __attribute__((aligned(16))) float smem[2 * kSeMaxN];
  float *skey = smem, *sval = smem + kSeMaxN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  int p0 = 0, p1 = 0;                                   // off.v[b], off.v[b + 1] at compile-time indices: a run-time index into
#pragma unroll                                          // the kernel arguments would copy them to scratch first
  for (int i = 0; i <= kSeMaxB; ++i) p0 = i == b ? off.v[i] : p0, p1 = i == b + 1 ? off.v[i] : p1;
  const int n = min(p1 - p0, kSeMaxN);
  const size_t plane = (size_t)h * w;
  const float* __restrict__ fl = flow + (size_t)b * 2 * plane;
  const float* __restrict__ cf = conf != nullptr ? conf + (size_t)b * plane : nullptr;
  const float fw = (float)w, fh = (float)h;

  float epe[kSePer], cfv[kSePer];
  unsigned valid = 0u;
  double st[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};        // EPE sum, #EPE <= 1 / 3 / 5 / 10, n_valid
#pragma unroll
  for (int e = 0; e < kSePer; ++e) {
    const int i = tid + e * kSeThreads;
    epe[e] = 0.0f, cfv[e] = 0.0f;
    if (i < n) {
      const float2 s = ps[p0 + i], t = pt[p0 + i];
      const float xs = rintf(s.x), ys = rintf(s.y), xt = rintf(t.x), yt = rintf(t.y);
      if (xs >= 0.0f && xs < fw && ys >= 0.0f && ys < fh && xt >= 0.0f && xt < fw && yt >= 0.0f && yt < fh) {
        const size_t o = (size_t)min(max((int)yt, 0), h - 1) * w + min(max((int)xt, 0), w - 1);
        const float dx = (s.x - t.x) - fl[o], dy = (s.y - t.y) - fl[plane + o];
        const float d = sqrtf(dx * dx + dy * dy);
        valid |= 1u << e;
        epe[e] = d;
        if (cf != nullptr) cfv[e] = cf[o];
        st[0] += (double)d;
        st[1] += d <= 1.0f ? 1.0 : 0.0, st[2] += d <= 3.0f ? 1.0 : 0.0, st[3] += d <= 5.0f ? 1.0 : 0.0;
        st[4] += d <= 10.0f ? 1.0 : 0.0, st[5] += 1.0;
      }
    }
  }
  double* sd = reinterpret_cast<double*>(sval);         // [wave][6] partial sums, then [96, 102) the totals
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    st[q] = wave_sum_d(st[q]);
    if (lane == 0) sd[wave * 6 + q] = st[q];
  }
  __syncthreads();
  if (tid < 6) {                                        // six lanes add the sixteen wave sums, in wave order
    double s = 0.0;
    for (int i = 0; i < kSeWaves; ++i) s += sd[i * 6 + tid];
    sd[kSeWaves * 6 + tid] = s;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 6; ++q) st[q] = sd[kSeWaves * 6 + q];
  __syncthreads();
  const int nv = (int)st[5];                            // (uniform over the workgroup)
  double* __restrict__ row = rows + (size_t)b * 8;
  if (nv == 0) {                                        // `continue` of the reference: the sample is not counted
    if (tid < 8) row[tid] = 0.0;
    return;
  }

  float ause = 0.0f;
  if (cf != nullptr) {
    int P = 8;
    while (P < n) P <<= 1;
    // oracle: the worst EPE is removed first
#pragma unroll
    for (int e = 0; e < kSePer; ++e) {
      const int i = tid + e * kSeThreads;
      if (i < P) skey[i] = (valid >> e) & 1u ? -epe[e] : INFINITY;
    }
    se_sort<false>(skey, sval, P, tid);
    const float co = se_curve<false>(skey, sval, P, nv, tid);
    // sparsification: the least confident point is removed first
#pragma unroll
    for (int e = 0; e < kSePer; ++e) {
      const int i = tid + e * kSeThreads;
      if (i < P) skey[i] = (valid >> e) & 1u ? -cfv[e] : INFINITY, sval[i] = epe[e];
    }
    se_sort<true>(skey, sval, P, tid);
    const float cs = se_curve<true>(skey, sval, P, nv, tid);
    if (tid <= kSeIntervals) skey[tid] = tid < kSeIntervals ? co : 0.0f, sval[tid] = tid < kSeIntervals ? cs : 0.0f;
    __syncthreads();
    if (tid < 8) {                                      // (the eight writing lanes each form the value: no broadcast needed)
      float mmax = skey[0];
      for (int t = 1; t <= kSeIntervals; ++t) mmax = fmaxf(mmax, skey[t]);
      mmax = mmax + 1e-6f;
      double as = 0.0, ao = 0.0;
      for (int t = 0; t < kSeIntervals; ++t) {
        const float dxp = (float)((double)(t + 1) / (double)kSeIntervals) - (float)((double)t / (double)kSeIntervals);
        as += (double)((sval[t] / mmax + sval[t + 1] / mmax) * dxp);
        ao += (double)((skey[t] / mmax + skey[t + 1] / mmax) * dxp);
      }
      ause = fabsf((float)as / 2.0f - (float)ao / 2.0f);
    }
  }
  if (tid < 8) {
    const double out[8] = {st[0] / (double)nv, st[1], st[2], st[3], st[4], (double)ause, (double)nv, 1.0};
    double v = out[0];
#pragma unroll
    for (int q = 1; q < 8; ++q) v = tid == q ? out[q] : v;
    row[tid] = v;
  }
}

}  // namespace rfn

extern "C" {
using namespace rfn;

// see include/refign_hip.h
int rfn_sparse_epe_f32(const float* flow, const float* conf, const float* pts_src, const float* pts_trg, const int* offsets, int B,
                       int h, int w, double* rows, rfn_stream_t stream) {
  RFN_REQUIRE(flow && pts_src && pts_trg && offsets && rows, "rfn_sparse_epe_f32: null pointer");
  RFN_REQUIRE(B > 0 && B <= kSeMaxB && h > 0 && w > 0, "rfn_sparse_epe_f32: B=%d (1 ... %d) h=%d w=%d", B, kSeMaxB, h, w);
  RFN_REQUIRE(offsets[0] == 0, "rfn_sparse_epe_f32: offsets[0] = %d, not 0", offsets[0]);
  SeOffsets off;
  off.v[0] = 0;
  for (int b = 0; b < B; ++b) {
    const int n = offsets[b + 1] - offsets[b];
    RFN_REQUIRE(n >= 0 && n <= kSeMaxN, "rfn_sparse_epe_f32: sample %d has %d points (0 ... %d)", b, n, kSeMaxN);
    off.v[b + 1] = offsets[b + 1];
  }
  hipLaunchKernelGGL(sparse_epe_kernel, dim3((unsigned)B), dim3(kSeThreads), 0, (hipStream_t)stream, flow, conf,
                     (const float2*)pts_src, (const float2*)pts_trg, off, h, w, rows);
  return check_launch("sparse_epe_kernel");
}

}  // extern "C"
