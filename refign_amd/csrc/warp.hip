// refign_amd/csrc/warp.hip -- bilinear warp kernels (gfx950): forward, the two forms of the backward, the tail of align().
//
// Reference behaviour restated from scratch:
//   warp()            helpers/matching_utils.py:11-49  (grid = base + flow, normalise with max(W-1,1),
//                      grid_sample bilinear / align_corners=True / zeros; mask = strictly inside (-1,1)^2)
//   tail of align()   models/segmentation_model.py:514-522 (bilinear align_corners=False upsampling of the
//                      quarter-res flow and log-variance, confidence, warp of the reference logits)
// The tap and the source index of the up-sampling: bilinear.h.
//
// HBM-bound gathers: one thread per output pixel computes the four taps once and streams the channels, so every
// global access of a wave is contiguous along w for the store and near-contiguous (smooth flow) for the loads.
#include "bilinear.h"
#include "common.h"

namespace rfn {

// grid: (ceil(HW/256), channel groups, B)
template <int CG>
__global__ __launch_bounds__(256) void warp_kernel(const float* __restrict__ x, const float* __restrict__ flow,
                                                   float* __restrict__ out, unsigned char* __restrict__ mask,
                                                   int C, int H, int W) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int HW = H * W;
  if (pix >= HW) return;
  const int n = blockIdx.z, c0 = blockIdx.y * CG;
  const int gy = pix / W, gx = pix - gy * W;
  const float* fl = flow + (size_t)n * 2 * HW;
  const WarpTap t = warp_tap((float)gx, (float)gy, fl[pix], fl[HW + pix], H, W);
  if (mask != nullptr && blockIdx.y == 0) mask[(size_t)n * HW + pix] = t.inside ? 1 : 0;
  const float* src = x + ((size_t)n * C + c0) * HW;
  float* dst = out + ((size_t)n * C + c0) * HW + pix;
  const int cend = min(CG, C - c0);
  for (int c = 0; c < cend; ++c) dst[(size_t)c * HW] = tap_sample(src + (size_t)c * HW, t);
}

// E with M < 2^E for the bit pattern of a finite M > 0 (a denormal M: below 2^-126 < 2^-125)
__device__ __forceinline__ int det_exponent(unsigned bits) { return max((int)(bits >> 23), 1) - 126; }
__device__ __forceinline__ double pow2(int e) { return __longlong_as_double((long long)(1023 + e) << 52); }   // |e| < 1023
__device__ __forceinline__ bool det_plane_live(unsigned bits) { return bits != 0u && bits < 0x7f800000u; }

// Backward of warp() = backward of grid_sample(bilinear, align_corners=True, zeros) composed with the flow -> grid map
// (ATen grid_sampler_2d_backward: gix = sum_c g [ (ne - nw) (1 - ty) + (se - sw) ty ], giy likewise; taps outside the
// image contribute zero).  d ix / d flow_x = ((W - 1) / 2) (2 / max(W - 1, 1)): 1 for W > 1, 0 for a one-pixel axis.
// One thread per pixel and channel group, in two forms that share everything but how a sum crosses threads:
//   atomic (rfn_warp_bwd_f32)      grad_x is a scatter of g w with float atomics (gx_out pre-zeroed), grad_flow the sum over the
//                                  channel groups with float atomics on 2 floats per pixel (pre-zeroed);
//   DET (rfn_warp_bwd_det_f32)     no floating-point atomic.  grad_x: every term g w is turned into a 64-bit integer multiple of a
//                                  per-plane unit u = 2^(E - F) and added with an integer atomic -- integer addition is associative, so
//                                  the sum has the same bits in whatever order the adds arrive.  E comes from the plane's largest
//                                  |grad_out| M (M < 2^E), F = 62 - ceil(log2(H W)): an output pixel sends at most one tap to a given
//                                  destination and every weight is <= 1, so |sum| < H W 2^F <= 2^62.  grad_flow across channel
//                                  groups: every group stores its two partial sums per pixel (part[G][B][2][H W]), the finalize pass
//                                  adds them in ascending group order.
// ONE_GROUP (C <= CG, the flow compositions and every map of at most CG channels), either form: the one group's thread owns its
// pixel's two grad_flow values and stores them -- no zero pass, no atomics, and the bits of the atomic form (0 + sum; a pixel the
// atomic form skips keeps its 0).
// DET workspace: int64 acc[B C H W] | uint32 maxbits[B C] | float part[G][B][2][H W]   (the first two with grad_x, the last with
// grad_flow over G > 1 groups)
template <int CG, bool ONE_GROUP, bool DET>
__device__ __forceinline__ void warp_bwd_body(const float* __restrict__ x, const float* __restrict__ flow,
                                              const float* __restrict__ gout, float* __restrict__ gx_out,
                                              unsigned long long* __restrict__ acc, const unsigned* __restrict__ maxbits,
                                              float* __restrict__ gflow, float* __restrict__ part, int C, int H, int W, int F) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int HW = H * W;
  if (pix >= HW) return;
  const int n = blockIdx.z, c0 = blockIdx.y * CG;
  const int gy = pix / W, gx = pix - gy * W;
  const float* fl = flow + (size_t)n * 2 * HW;
  const WarpTap t = warp_tap((float)gx, (float)gy, fl[pix], fl[HW + pix], H, W);
  const float tx = t.tx, ty = t.ty, ax = 1.0f - tx, ay = 1.0f - ty;
  const float* src = x + ((size_t)n * C + c0) * HW;
  const float* go = gout + ((size_t)n * C + c0) * HW + pix;
  const int cend = min(CG, C - c0);
  float gix = 0.f, giy = 0.f;
  for (int c = 0; c < cend; ++c) {
    const float g = go[(size_t)c * HW];
    if (gflow) {
      const float* s = src + (size_t)c * HW;
      const float nw = t.v00 ? s[t.o00] : 0.f, ne = t.v01 ? s[t.o01] : 0.f, sw = t.v10 ? s[t.o10] : 0.f, se = t.v11 ? s[t.o11] : 0.f;
      gix += g * ((ne - nw) * ay + (se - sw) * ty);
      giy += g * ((sw - nw) * ax + (se - ne) * tx);
    }
    const size_t plane = (size_t)n * C + c0 + c;
    if constexpr (DET) {
      const unsigned mb = acc ? maxbits[plane] : 0u;
      if (det_plane_live(mb)) {                            // (an all-zero or a non-finite plane: written whole by the finalize pass)
        const double scale = pow2(F - det_exponent(mb));   // exact: |g w| 2^(F - E) < 2^F
        unsigned long long* d = acc + plane * HW;
        if (t.v00) atomicAdd(d + t.o00, (unsigned long long)llrint((double)(g * t.w00) * scale));
        if (t.v01) atomicAdd(d + t.o01, (unsigned long long)llrint((double)(g * t.w01) * scale));
        if (t.v10) atomicAdd(d + t.o10, (unsigned long long)llrint((double)(g * t.w10) * scale));
        if (t.v11) atomicAdd(d + t.o11, (unsigned long long)llrint((double)(g * t.w11) * scale));
      }
    } else if (gx_out) {
      float* d = gx_out + plane * HW;
      if (t.v00) atomicAdd(d + t.o00, g * t.w00);
      if (t.v01) atomicAdd(d + t.o01, g * t.w01);
      if (t.v10) atomicAdd(d + t.o10, g * t.w10);
      if (t.v11) atomicAdd(d + t.o11, g * t.w11);
    }
  }
  if (gflow) {
    const bool live_x = W > 1 && t.finite, live_y = H > 1 && t.finite;
    if constexpr (ONE_GROUP || DET) {
      float* gf = ONE_GROUP ? gflow + (size_t)n * 2 * HW : part + ((size_t)blockIdx.y * gridDim.z + n) * 2 * HW;
      gf[pix] = live_x ? 0.0f + gix : 0.0f;                // (0 + x: what the add onto the zeroed buffer gives for x = -0)
      gf[HW + pix] = live_y ? 0.0f + giy : 0.0f;
    } else {
      float* gf = gflow + (size_t)n * 2 * HW;
      if (live_x) atomicAdd(gf + pix, gix);
      if (live_y) atomicAdd(gf + HW + pix, giy);
    }
  }
}

// grid: (ceil(HW/256), channel groups, B)
template <int CG, bool ONE_GROUP>
__global__ __launch_bounds__(256) void warp_bwd_kernel(const float* __restrict__ x, const float* __restrict__ flow,
                                                       const float* __restrict__ gout, float* __restrict__ gx_out,
                                                       float* __restrict__ gflow, int C, int H, int W) {
  warp_bwd_body<CG, ONE_GROUP, false>(x, flow, gout, gx_out, nullptr, nullptr, gflow, nullptr, C, H, W, 0);
}

template <int CG, bool ONE_GROUP>
__global__ __launch_bounds__(256) void warp_bwd_det_scatter_kernel(const float* __restrict__ x, const float* __restrict__ flow,
                                                                   const float* __restrict__ gout,
                                                                   unsigned long long* __restrict__ acc,
                                                                   const unsigned* __restrict__ maxbits, float* __restrict__ gflow,
                                                                   float* __restrict__ part, int C, int H, int W, int F) {
  warp_bwd_body<CG, ONE_GROUP, true>(x, flow, gout, nullptr, acc, maxbits, gflow, part, C, H, W, F);
}

// The first pass of the DET form: maxbits[plane] = the largest bit pattern of |grad_out| over the plane (monotone in |g|;
// >= 0x7f800000: an inf or a NaN).
// grid: (ceil(HW/1024), C, B); maxbits zeroed before.
__global__ __launch_bounds__(256) void warp_bwd_det_scale_kernel(const float* __restrict__ gout, unsigned* __restrict__ maxbits,
                                                                 int C, int HW) {
  __shared__ unsigned wave_max[4];
  const size_t plane = (size_t)blockIdx.z * C + blockIdx.y;
  const float* g = gout + plane * HW;
  unsigned m = 0u;
  for (int k = 0; k < 4; ++k) {
    const long i = (long)blockIdx.x * 1024 + k * 256 + threadIdx.x;
    if (i < HW) m = max(m, __float_as_uint(g[i]) & 0x7fffffffu);
  }
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(maxbits + plane, max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3])));
}

// The last: grad_x = acc * u (a non-finite plane: NaN throughout; an all-zero plane: 0) for idx < nx, then grad_flow = the groups'
// partial sums added in ascending order onto 0 for the nf elements behind.  Either part may be empty.
__global__ __launch_bounds__(256) void warp_bwd_det_finalize_kernel(const long long* __restrict__ acc,
                                                                    const unsigned* __restrict__ maxbits, float* __restrict__ gx_out,
                                                                    const float* __restrict__ part, float* __restrict__ gflow,
                                                                    long nx, long nf, int HW, int F, int G) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx < nx) {
    const unsigned mb = maxbits[idx / HW];
    float v = 0.0f;
    if (mb >= 0x7f800000u) v = __uint_as_float(0x7fc00000u);
    else if (mb != 0u) v = (float)((double)acc[idx] * pow2(det_exponent(mb) - F));
    gx_out[idx] = v;
  } else if (idx < nx + nf) {
    const long j = idx - nx;
    float s = 0.0f;
    for (int g = 0; g < G; ++g) s += part[(size_t)g * nf + j];
    gflow[j] = s;
  }
}

__device__ __forceinline__ float up_sample(const float* __restrict__ p, int w, int y0, int y1, int x0, int x1,
                                           float ly0, float ly1, float lx0, float lx1) {
#pragma clang fp contract(off)
  return ly0 * (lx0 * p[y0 * w + x0] + lx1 * p[y0 * w + x1]) + ly1 * (lx0 * p[y1 * w + x0] + lx1 * p[y1 * w + x1]);
}

// grid: (ceil(HW/256), 1, B)
__global__ __launch_bounds__(256) void align_tail_kernel(const float* __restrict__ logits,
                                                         const float* __restrict__ flow_q,
                                                         const float* __restrict__ logvar_q,
                                                         float* __restrict__ warped, unsigned char* __restrict__ mask,
                                                         float* __restrict__ cert, float* __restrict__ flow_up, int C,
                                                         int H, int W, int h, int w, float sy, float sx) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int HW = H * W, hw = h * w;
  if (pix >= HW) return;
  const int n = blockIdx.z;
  const int gy = pix / W, gx = pix - gy * W;
  int y0, y1, x0, x1;
  float ly1, lx1;
  up_src_nofma(gy, sy, h, y0, y1, ly1);
  up_src_nofma(gx, sx, w, x0, x1, lx1);
  const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
  const float* fq = flow_q + (size_t)n * 2 * hw;
  const float fx = up_sample(fq, w, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
  const float fy = up_sample(fq + hw, w, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
  const float lv = up_sample(logvar_q + (size_t)n * hw, w, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
  // matching_utils.py:55-56 with R = 1
  cert[(size_t)n * HW + pix] = 1.0f - expf(-1.0f / (2.0f * expf(lv)));
  if (flow_up != nullptr) {
    flow_up[(size_t)n * 2 * HW + pix] = fx;
    flow_up[(size_t)n * 2 * HW + HW + pix] = fy;
  }
  const WarpTap t = warp_tap((float)gx, (float)gy, fx, fy, H, W);
  mask[(size_t)n * HW + pix] = t.inside ? 1 : 0;
  const float* src = logits + (size_t)n * C * HW;
  float* dst = warped + (size_t)n * C * HW + pix;
  for (int c = 0; c < C; ++c) dst[(size_t)c * HW] = tap_sample(src + (size_t)c * HW, t);
}

}  // namespace rfn

using namespace rfn;

extern "C" {

int rfn_warp_f32(const float* x, const float* flow, float* out, unsigned char* mask, int B, int C, int H, int W,
                 rfn_stream_t stream) {
  RFN_REQUIRE(x && flow && out, "rfn_warp_f32: null pointer");
  RFN_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "rfn_warp_f32: non-positive size");
  RFN_REQUIRE((long)H * W < 0x7fffffffL && B <= 65535, "rfn_warp_f32: tensor too large");
  constexpr int CG = 32;
  dim3 grid(cdiv((long)H * W, 256), cdiv(C, CG), B);
  hipLaunchKernelGGL((warp_kernel<CG>), grid, dim3(256), 0, (hipStream_t)stream, x, flow, out, mask, C, H, W);
  return check_launch("warp_kernel");
}

int rfn_warp_bwd_f32(const float* x, const float* flow, const float* grad_out, float* grad_x, float* grad_flow, int B,
                     int C, int H, int W, rfn_stream_t stream) {
  RFN_REQUIRE(x && flow && grad_out && (grad_x || grad_flow), "rfn_warp_bwd_f32: null pointer");
  RFN_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "rfn_warp_bwd_f32: non-positive size");
  RFN_REQUIRE((long)H * W < 0x7fffffffL && B <= 65535, "rfn_warp_bwd_f32: tensor too large");
  RFN_REFUSE_NONDET(true, "rfn_warp_bwd_f32", "warp_bwd_kernel, fp32 atomics (no deterministic form)");
  hipStream_t s = (hipStream_t)stream;
  const size_t HW = (size_t)H * W;
  constexpr int CG = 32;
  const bool one_group = C <= CG;
  // zero-fill as kernels on the caller's stream, not memset nodes: the matcher's training step is captured into a hipGraph
  // (capi.hip zero_async)
  if (grad_x)
    if (int rc = zero_async(grad_x, (size_t)B * C * HW * sizeof(float), s)) return rc;
  if (grad_flow && !one_group)
    if (int rc = zero_async(grad_flow, (size_t)B * 2 * HW * sizeof(float), s)) return rc;
  dim3 grid(cdiv((long)HW, 256), cdiv(C, CG), B);
  if (one_group)
    hipLaunchKernelGGL((warp_bwd_kernel<CG, true>), grid, dim3(256), 0, s, x, flow, grad_out, grad_x, grad_flow, C, H, W);
  else
    hipLaunchKernelGGL((warp_bwd_kernel<CG, false>), grid, dim3(256), 0, s, x, flow, grad_out, grad_x, grad_flow, C, H, W);
  return check_launch("warp_bwd_kernel");
}

// ceil(log2(HW)) for HW >= 1
static inline int ceil_log2(long v) {
  int l = 0;
  while ((1L << l) < v) ++l;
  return l;
}

unsigned long rfn_warp_bwd_det_workspace_bytes(int B, int C, int H, int W, int want_grad_x, int want_grad_flow) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  const size_t HW = (size_t)H * W, G = (size_t)cdiv(C, 32);
  size_t bytes = 0;
  if (want_grad_x) bytes += 8 * (size_t)B * C * HW + 4 * (size_t)B * C;
  if (want_grad_flow && G > 1) bytes += 8 * G * B * HW;
  return bytes;
}

int rfn_warp_bwd_det_f32(const float* x, const float* flow, const float* grad_out, float* grad_x, float* grad_flow,
                         void* workspace, int B, int C, int H, int W, rfn_stream_t stream) {
  RFN_REQUIRE(x && flow && grad_out && (grad_x || grad_flow), "rfn_warp_bwd_det_f32: null pointer");
  RFN_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "rfn_warp_bwd_det_f32: non-positive size");
  RFN_REQUIRE((long)H * W < 0x7fffffffL && B <= 65535 && C <= 65535, "rfn_warp_bwd_det_f32: tensor too large");
  hipStream_t s = (hipStream_t)stream;
  const size_t HW = (size_t)H * W;
  constexpr int CG = 32;
  const int G = cdiv(C, CG);
  const bool one_group = G == 1;
  const size_t planes = (size_t)B * C, acc_bytes = grad_x ? 8 * planes * HW : 0, max_bytes = grad_x ? 4 * planes : 0;
  const bool partials = grad_flow && !one_group;
  RFN_REQUIRE(workspace || !(grad_x || partials), "rfn_warp_bwd_det_f32: null workspace");
  RFN_REQUIRE(((size_t)workspace & 15) == 0, "rfn_warp_bwd_det_f32: workspace must be 16-byte aligned");
  const long nx = grad_x ? (long)(planes * HW) : 0, nf = partials ? (long)(2 * B * HW) : 0;
  RFN_REQUIRE((nx + nf) / 256 < 0x7fffffffL, "rfn_warp_bwd_det_f32: tensor too large");
  unsigned long long* acc = grad_x ? (unsigned long long*)workspace : nullptr;
  unsigned* maxbits = grad_x ? (unsigned*)((char*)workspace + acc_bytes) : nullptr;
  float* part = partials ? (float*)((char*)workspace + acc_bytes + max_bytes) : nullptr;
  const int F = 62 - ceil_log2((long)HW);
  if (grad_x) {
    // (a kernel on the caller's stream, as in rfn_warp_bwd_f32: the step is captured into a hipGraph)
    if (int rc = zero_async(workspace, acc_bytes + max_bytes, s)) return rc;
    hipLaunchKernelGGL(warp_bwd_det_scale_kernel, dim3(cdiv((long)HW, 1024), C, B), dim3(256), 0, s, grad_out, maxbits, C, (int)HW);
    if (int rc = check_launch("warp_bwd_det_scale_kernel")) return rc;
  }
  dim3 grid(cdiv((long)HW, 256), G, B);
  if (one_group)
    hipLaunchKernelGGL((warp_bwd_det_scatter_kernel<CG, true>), grid, dim3(256), 0, s, x, flow, grad_out, acc, maxbits, grad_flow,
                       part, C, H, W, F);
  else
    hipLaunchKernelGGL((warp_bwd_det_scatter_kernel<CG, false>), grid, dim3(256), 0, s, x, flow, grad_out, acc, maxbits, grad_flow,
                       part, C, H, W, F);
  if (int rc = check_launch("warp_bwd_det_scatter_kernel")) return rc;
  if (nx + nf == 0) return RFN_OK;
  hipLaunchKernelGGL(warp_bwd_det_finalize_kernel, dim3((unsigned)cdiv(nx + nf, 256)), dim3(256), 0, s, (const long long*)acc,
                     maxbits, grad_x, part, grad_flow, nx, nf, (int)HW, F, G);
  return check_launch("warp_bwd_det_finalize_kernel");
}

int rfn_align_tail_f32(const float* logits_ref, const float* flow_q, const float* logvar_q, float* warped,
                       unsigned char* mask, float* cert, float* flow_up, int B, int C, int H, int W, int h, int w,
                       rfn_stream_t stream) {
  RFN_REQUIRE(logits_ref && flow_q && logvar_q && warped && mask && cert, "rfn_align_tail_f32: null pointer");
  RFN_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && h > 0 && w > 0, "rfn_align_tail_f32: non-positive size");
  RFN_REQUIRE((long)H * W < 0x7fffffffL && B <= 65535, "rfn_align_tail_f32: tensor too large");
  dim3 grid(cdiv((long)H * W, 256), 1, B);
  // ATen area_pixel_compute_scale(align_corners=False, no explicit scale): input_size / output_size in float
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  hipLaunchKernelGGL(align_tail_kernel, grid, dim3(256), 0, (hipStream_t)stream, logits_ref, flow_q, logvar_q,
                     warped, mask, cert, flow_up, C, H, W, h, w, sy, sx);
  return check_launch("align_tail_kernel");
}

}  // extern "C"
