// refign_amd/csrc/flowloss.hip -- the multi-level flow loss of matcher training (models/losses.py:37-188, MultiScaleFlowLoss
// with downsample_gt_flow=True) over ALL pyramid levels of one call: one forward launch + one finalize launch, one backward
// launch.  The torch formulation costs ~15 small launches per level each way and decides "no valid pixel" on the host.
//
// Per level pixel: the full-resolution ground-truth flow resized to the level (the arithmetic of F.interpolate(mode=
// 'bilinear', align_corners=False)), the per-channel L1 / L2 / Huber term summed over the two channels, the Gaussian negative
// log-likelihood when the level carries log-variances (two channels: logsumexp), the level's validity mask.  A workgroup
// covers kPixels consecutive pixels of ONE level and stores its partial {sum, count} (fp64) to a workspace; the finalize
// launch adds each level's partials in index order.  No floating-point atomics anywhere: the same inputs give the same bits,
// so the entry points are legal under rfn_set_deterministic(1).  The backward evaluates the same per-pixel function again
// (nothing per pixel is saved) and scales by grad_out * weight / count, all read on the device.
#include <cmath>

#include "bilinear.h"
#include "common.h"

namespace rfn {

constexpr int kFlThreads = 256, kFlPerThread = 4, kFlPixels = kFlThreads * kFlPerThread;
constexpr int kFlMaxLevels = 8;

struct FlLevel {
  const float* flow;            // (B, 2, h, w)
  const float* logvar;          // (B, lvc, h, w) or null
  const unsigned char* mask;    // (B, h, w) bytes 0 / 1, or null
  float* gflow;                 // backward: (B, 2, h, w) or null
  float* glogvar;               // backward: (B, lvc, h, w) or null
  int h, w, lvc, block0;        // block0: the first workgroup of this level
  float weight;
};
struct FlTable {
  FlLevel l[kFlMaxLevels];
  int n;
};

// the per-channel term and its derivative.  loss_type: 0 L1Loss, 1 L2Loss (MSE), 2 HuberLoss = 2 delta smooth_l1(beta = delta)
__device__ __forceinline__ float fl_term(float d, int loss_type, float delta, float& dd) {
  const float a = fabsf(d), sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  if (loss_type == 0) {
    dd = sgn;
    return a;
  }
  if (loss_type == 1) {
    dd = 2.f * d;
    return d * d;
  }
  if (a < delta) {
    dd = 2.f * delta * (d / delta);
    return 2.f * (0.5f * a * a / delta) * delta;
  }
  dd = 2.f * delta * sgn;
  return 2.f * (a - 0.5f * delta) * delta;
}

struct FlPixel {
  float value;                  // the pixel's contribution to the level's sum
  float df0, df1;               // d value / d flow (channel 0, 1)
  float dl0, dl1;               // d value / d log-variance (channel 0, 1)
};

// pixel (b, y, x) of level L; the caller has checked the mask
__device__ __forceinline__ FlPixel fl_pixel(const FlLevel& L, const float* __restrict__ gt, int H, int W, int b, int y, int x,
                                            int loss_type, float delta) {
  int y0, y1, x0, x1;
  float ly1, lx1;
  up_src(y, (float)H / (float)L.h, H, y0, y1, ly1);
  up_src(x, (float)W / (float)L.w, W, x0, x1, lx1);
  const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
  const long hw = (long)L.h * L.w, pix = (long)y * L.w + x;
  FlPixel r;
  float loss = 0.f, dd[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float* g = gt + ((long)b * 2 + c) * H * W;
    const float want = ly0 * (lx0 * g[(long)y0 * W + x0] + lx1 * g[(long)y0 * W + x1]) +
                       ly1 * (lx0 * g[(long)y1 * W + x0] + lx1 * g[(long)y1 * W + x1]);
    loss += fl_term(L.flow[((long)b * 2 + c) * hw + pix] - want, loss_type, delta, dd[c]);
  }
  if (L.lvc == 0) {
    r.value = loss;
    r.df0 = dd[0];
    r.df1 = dd[1];
    r.dl0 = r.dl1 = 0.f;
    return r;
  }
  float lv, s0 = 1.f, s1 = 0.f;
  if (L.lvc == 1) {
    lv = L.logvar[(long)b * hw + pix];
  } else {                                                     // two independent terms: the variances add
    const float a0 = L.logvar[((long)b * 2) * hw + pix], a1 = L.logvar[((long)b * 2 + 1) * hw + pix];
    const float m = fmaxf(a0, a1);
    lv = m + logf(expf(a0 - m) + expf(a1 - m));
    s0 = expf(a0 - lv);
    s1 = expf(a1 - lv);
  }
  const float half_inv = 0.5f * expf(-lv);
  r.value = half_inv * loss + lv + 1.8378770664093453f;        // log(2 pi)
  r.df0 = half_inv * dd[0];
  r.df1 = half_inv * dd[1];
  const float dlv = 1.f - half_inv * loss;
  r.dl0 = dlv * s0;
  r.dl1 = dlv * s1;
  return r;
}

__device__ __forceinline__ int fl_level_of_block(const FlTable& t, int block) {
  int li = 0;
  while (li + 1 < t.n && block >= t.l[li + 1].block0) ++li;
  return li;
}

__global__ __launch_bounds__(kFlThreads) void flowloss_fwd_kernel(FlTable t, const float* __restrict__ gt, int B, int H, int W,
                                                                  int loss_type, float delta, double* __restrict__ partials) {
  const FlLevel L = t.l[fl_level_of_block(t, blockIdx.x)];
  const int hw = L.h * L.w, n = B * hw;
  const int base = (blockIdx.x - L.block0) * kFlPixels;
  double sum = 0.0;
  int count = 0;
#pragma unroll
  for (int k = 0; k < kFlPerThread; ++k) {
    const int idx = base + k * kFlThreads + threadIdx.x;
    if (idx >= n || (L.mask != nullptr && L.mask[idx] == 0)) continue;
    const int b = idx / hw, rem = idx - b * hw;
    sum += (double)fl_pixel(L, gt, H, W, b, rem / L.w, rem % L.w, loss_type, delta).value;
    ++count;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    count += __shfl_xor(count, o, 64);
  }
  __shared__ double wsum[kFlThreads / kWave];
  __shared__ int wcount[kFlThreads / kWave];
  if ((threadIdx.x & 63) == 0) {
    wsum[threadIdx.x >> 6] = sum;
    wcount[threadIdx.x >> 6] = count;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    int c = 0;
    for (int i = 0; i < kFlThreads / kWave; ++i) {
      s += wsum[i];
      c += wcount[i];
    }
    partials[2 * (long)blockIdx.x] = s;
    partials[2 * (long)blockIdx.x + 1] = (double)c;
  }
}

// thread l adds level l's partials in index order; loss_out = {total, mean of level 0, 1, ...}, counts = valid pixels per level
__global__ void flowloss_finalize_kernel(FlTable t, int nblocks, const double* __restrict__ partials, float* __restrict__ loss_out,
                                         double* __restrict__ counts) {
  __shared__ float mean[kFlMaxLevels];
  const int l = threadIdx.x;
  if (l < t.n) {
    const int end = l + 1 < t.n ? t.l[l + 1].block0 : nblocks;
    double s = 0.0, c = 0.0;
    for (int i = t.l[l].block0; i < end; ++i) {
      s += partials[2 * (long)i];
      c += partials[2 * (long)i + 1];
    }
    mean[l] = c > 0.0 ? (float)(s / c) : 0.f;                  // no valid pixel: the level contributes 0
    loss_out[1 + l] = mean[l];
    counts[l] = c;
  }
  __syncthreads();
  if (l == 0) {
    float total = 0.f;
    for (int i = 0; i < t.n; ++i) total = total + t.l[i].weight * mean[i];
    loss_out[0] = total;
  }
}

__global__ __launch_bounds__(kFlThreads) void flowloss_bwd_kernel(FlTable t, const float* __restrict__ gt, int B, int H, int W,
                                                                  int loss_type, float delta, const double* __restrict__ counts,
                                                                  const float* __restrict__ grad_out) {
  const int li = fl_level_of_block(t, blockIdx.x);
  const FlLevel L = t.l[li];
  const int hw = L.h * L.w, n = B * hw;
  const int base = (blockIdx.x - L.block0) * kFlPixels;
  const double cnt = counts[li];
  const float scale = cnt > 0.0 ? *grad_out * L.weight / (float)cnt : 0.f;
#pragma unroll
  for (int k = 0; k < kFlPerThread; ++k) {
    const int idx = base + k * kFlThreads + threadIdx.x;
    if (idx >= n) continue;
    const int b = idx / hw, rem = idx - b * hw;
    FlPixel p{0.f, 0.f, 0.f, 0.f, 0.f};
    const bool valid = cnt > 0.0 && (L.mask == nullptr || L.mask[idx] != 0);
    if (valid) p = fl_pixel(L, gt, H, W, b, rem / L.w, rem % L.w, loss_type, delta);
    if (L.gflow != nullptr) {
      L.gflow[((long)b * 2) * hw + rem] = valid ? scale * p.df0 : 0.f;
      L.gflow[((long)b * 2 + 1) * hw + rem] = valid ? scale * p.df1 : 0.f;
    }
    if (L.glogvar != nullptr) {
      L.glogvar[((long)b * L.lvc) * hw + rem] = valid ? scale * p.dl0 : 0.f;
      if (L.lvc == 2) L.glogvar[((long)b * 2 + 1) * hw + rem] = valid ? scale * p.dl1 : 0.f;
    }
  }
}

// levels: HOST array of nlevels x 8 longs {flow, logvar, mask, grad_flow, grad_logvar, h, w, logvar channels}; weights: HOST.
// -> the number of workgroups, or -1 after fail()
static int fl_table(const char* what, const float* gt, int B, int H, int W, const long* levels, const double* weights,
                    int nlevels, int loss_type, float delta, FlTable& t) {
  if (!(gt && levels && weights && B > 0 && H > 0 && W > 0 && nlevels > 0 && nlevels <= kFlMaxLevels && loss_type >= 0 &&
        loss_type <= 2 && delta > 0.f)) {
    fail(RFN_EINVAL, "%s: null pointer, empty shape, more than %d levels, loss type outside 0..2 or delta <= 0", what, kFlMaxLevels);
    return -1;
  }
  long blocks = 0;
  for (int i = 0; i < nlevels; ++i) {
    const long* r = levels + 8 * i;
    FlLevel& L = t.l[i];
    L.flow = (const float*)r[0];
    L.logvar = (const float*)r[1];
    L.mask = (const unsigned char*)r[2];
    L.gflow = (float*)r[3];
    L.glogvar = (float*)r[4];
    const long h = r[5], w = r[6], lvc = r[7];
    if (!(L.flow && h > 0 && w > 0 && lvc >= 0 && lvc <= 2 && (lvc == 0) == (L.logvar == nullptr) &&
          (L.glogvar == nullptr || lvc > 0) && (long)B * h * w * 2 < (1L << 31))) {
      fail(RFN_EINVAL, "%s: level %d: null flow, empty or too large shape (%ld x %ld), or log-variance channels %ld not "
                       "0 (no pointer), 1 or 2", what, i, h, w, lvc);
      return -1;
    }
    L.h = (int)h;
    L.w = (int)w;
    L.lvc = (int)lvc;
    L.block0 = (int)blocks;
    L.weight = (float)weights[i];
    blocks += cdiv((long)B * h * w, kFlPixels);
  }
  t.n = nlevels;
  return (int)blocks;
}

}  // namespace rfn

extern "C" {

int rfn_flowloss_block_pixels(void) { return rfn::kFlPixels; }

int rfn_flowloss_fwd_f32(const float* gt_flow, int B, int H, int W, const long* levels, const double* weights, int nlevels,
                         int loss_type, float delta, double* partials, int nblocks, float* loss_out, double* counts,
                         rfn_stream_t stream) {
  rfn::FlTable t{};
  const int blocks = rfn::fl_table("rfn_flowloss_fwd_f32", gt_flow, B, H, W, levels, weights, nlevels, loss_type, delta, t);
  if (blocks < 0) return RFN_EINVAL;
  RFN_REQUIRE(partials && loss_out && counts && nblocks == blocks,
              "rfn_flowloss_fwd_f32: null output, or a workspace of %d workgroups where the levels need %d", nblocks, blocks);
  hipLaunchKernelGGL(rfn::flowloss_fwd_kernel, dim3(blocks), dim3(rfn::kFlThreads), 0, (hipStream_t)stream, t, gt_flow, B, H, W,
                     loss_type, delta, partials);
  hipLaunchKernelGGL(rfn::flowloss_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, t, blocks,
                     (const double*)partials, loss_out, counts);
  return rfn::check_launch("flowloss_fwd_kernel");
}

int rfn_flowloss_bwd_f32(const float* gt_flow, int B, int H, int W, const long* levels, const double* weights, int nlevels,
                         int loss_type, float delta, const double* counts, const float* grad_out, rfn_stream_t stream) {
  rfn::FlTable t{};
  const int blocks = rfn::fl_table("rfn_flowloss_bwd_f32", gt_flow, B, H, W, levels, weights, nlevels, loss_type, delta, t);
  if (blocks < 0) return RFN_EINVAL;
  RFN_REQUIRE(counts && grad_out, "rfn_flowloss_bwd_f32: null counts or grad_out");
  hipLaunchKernelGGL(rfn::flowloss_bwd_kernel, dim3(blocks), dim3(rfn::kFlThreads), 0, (hipStream_t)stream, t, gt_flow, B, H, W,
                     loss_type, delta, counts, grad_out);
  return rfn::check_launch("flowloss_bwd_kernel");
}

}  // extern "C"
