// refign_amd/csrc/flowsynth.hip -- the matcher's warp supervision on the device: data_modules/transforms.py:573-1395
// (RandomAffine / RandomHomography / RandomTPS / RandomAffineTPS / RandomElastic under CompositeFlow) followed by CenterCrop,
// for ONE sample per call.  Every flow of the reference is analytic per pixel, so nothing but the flow itself is stored:
//   flowsynth_flow_kernel   per pixel of the full frame: the final mapping from 9 + 24 + 6 floats, a transform code and, with
//                           the elastic step, the blurred perturbation field and at most 13 Gaussian bumps.  The elastic step is
//                           helpers/matching_utils.py:11-49 `warp(mapping, perturbation)`: a zero-padded bilinear sample of the
//                           pixel-unit mapping, which is evaluated at the four integer neighbours.  It also counts
//                           create_border_mask over the full frame: a ballot per wave, one integer atomic per workgroup.
//   flowsynth_warp_kernel   per pixel of the crop window: grid_sample(image, grid + flow, align_corners=True, zeros), the
//                           warp mask and the border mask, and the fallback to the border mask decided from the count.
//   flowsynth_blur_kernel   cv2.GaussianBlur's arithmetic for a float32 image as OpenCV documents it: separable, the
//                           float32 taps given by the caller, BORDER_REFLECT_101 folded by period 2(n - 1), accumulated in
//                           fp64 through BOTH passes (the intermediate is fp64) and rounded once.  Lanes run along W in both.
// The values are fp32, formed operation by operation in the reference's order (no contraction): the sentinel arithmetic
// (mask * g + (mask - 1) * 1e10, blended by bilinear weights) and the comparisons against the frame's borders depend on it.
// No floating-point atomics: legal in deterministic mode, bit-identical from launch to launch.
#include "common.h"

#pragma clang fp contract(off)

namespace rfn {

constexpr int kFsMaxBumps = 13, kFsThreads = 256, kFsBlurUnroll = 8;
constexpr float kFsSentinel = 1e10f;

struct FsBump {
  float x, y, sig2, div, scale;                // mu of axis 0 / axis 1 (the reference's quirk: x runs along the ROWS), 2 s^2, s * 2 pi
};
struct FsParams {
  float hom[9];                                // h0 .. h8
  float wx[9], wy[9], ax[3], ay[3];            // thin-plate spline: W_X, W_Y, A_X, A_Y
  float aff[6];                                // theta of affine_grid
  int kind, n_bumps;                           // 0 hom, 1 affine, 2 tps, 3 afftps
  FsBump bump[kFsMaxBumps];
};

// torch.linspace(-1, 1, n)[i] in fp32 as ATen forms it: from the start in the first half, from the end in the second
__device__ __forceinline__ float fs_lin(int i, int n) {
  const float step = 2.0f / (float)(n - 1);
  return i < n / 2 ? -1.0f + step * (float)i : 1.0f - step * (float)(n - 1 - i);
}

__device__ __forceinline__ void fs_hom(const FsParams& p, float gx, float gy, float& ox, float& oy) {
  const float xp = gx * p.hom[0] + gy * p.hom[1] + p.hom[2];
  const float yp = gx * p.hom[3] + gy * p.hom[4] + p.hom[5];
  const float k = gx * p.hom[6] + gy * p.hom[7] + p.hom[8];
  ox = xp / k, oy = yp / k;
}

__device__ __forceinline__ void fs_tps(const FsParams& p, float gx, float gy, float& ox, float& oy) {
  float sx = 0.0f, sy = 0.0f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {                // control point k: (axis[k / 3], axis[k % 3]), axis = -1, 0, 1
    const float dx = gx - (float)(k / 3 - 1), dy = gy - (float)(k % 3 - 1);
    float d = dx * dx + dy * dy;
    d = d == 0.0f ? 1.0f : d;
    const float u = d * logf(d);
    sx += p.wx[k] * u, sy += p.wy[k] * u;
  }
  ox = p.ax[0] + p.ax[1] * gx + p.ax[2] * gy + sx;
  oy = p.ay[0] + p.ay[1] * gx + p.ay[2] * gy + sy;
}

// F.affine_grid(theta, align_corners=False) at integer (xi, yi): the base grid is linspace * (n - 1) / n
__device__ __forceinline__ void fs_aff(const FsParams& p, int xi, int yi, int h, int w, float& ox, float& oy) {
  const float bx = fs_lin(xi, w) * (float)(w - 1) / (float)w, by = fs_lin(yi, h) * (float)(h - 1) / (float)h;
  ox = bx * p.aff[0] + by * p.aff[1] + p.aff[2];
  oy = bx * p.aff[3] + by * p.aff[4] + p.aff[5];
}

// the affine grid with its out-of-bounds sentinel (mask * g + (mask - 1) * 1e10), 0 outside the frame (zero padding)
__device__ __forceinline__ void fs_aff_sentinel(const FsParams& p, int xi, int yi, int h, int w, float& ox, float& oy) {
  ox = 0.0f, oy = 0.0f;
  if (xi < 0 || xi >= w || yi < 0 || yi >= h) return;
  fs_aff(p, xi, yi, h, w, ox, oy);
  if (!(ox > -1.0f && ox < 1.0f && oy > -1.0f && oy < 1.0f)) ox = -kFsSentinel, oy = -kFsSentinel;
}

// zero-padded bilinear blend as F.grid_sample forms it; get(xi, yi, vx, vy) returns the two channels at an integer point
template <typename Get>
__device__ __forceinline__ void fs_bilinear2(float ix, float iy, Get&& get, float& ox, float& oy) {
  const float fx = floorf(ix), fy = floorf(iy);
  const float wx1 = ix - fx, wy1 = iy - fy, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
  // (a position beyond the int range has no neighbour inside the frame: clamp before the conversion)
  const int x0 = (int)fminf(fmaxf(fx, -2.0f), 2.0e9f), y0 = (int)fminf(fmaxf(fy, -2.0f), 2.0e9f);
  float ax, ay, bx, by, cx, cy, dx, dy;
  get(x0, y0, ax, ay), get(x0 + 1, y0, bx, by), get(x0, y0 + 1, cx, cy), get(x0 + 1, y0 + 1, dx, dy);
  const float nw = wx0 * wy0, ne = wx1 * wy0, sw = wx0 * wy1, se = wx1 * wy1;
  ox = ax * nw + bx * ne + cx * sw + dx * se;
  oy = ay * nw + by * ne + cy * sw + dy * se;
}

// the transform's normalised mapping at integer (xi, yi) of the frame
__device__ __forceinline__ void fs_map_norm(const FsParams& p, int xi, int yi, int h, int w, float& ox, float& oy) {
  const int kind = p.kind;
  if (kind == 1) {
    fs_aff(p, xi, yi, h, w, ox, oy);
    return;
  }
  const float gx = fs_lin(xi, w), gy = fs_lin(yi, h);
  if (kind == 0) {
    fs_hom(p, gx, gy, ox, oy);
    return;
  }
  float tx, ty;
  fs_tps(p, gx, gy, tx, ty);
  if (kind == 2) {
    ox = tx, oy = ty;
    return;
  }
  // afftps: grid_sample(sentinel'd affine grid, tps grid, align_corners=True, zeros), then the tps grid's own sentinel
  if (!(tx > -1.0f && tx < 1.0f && ty > -1.0f && ty < 1.0f)) {
    ox = -kFsSentinel, oy = -kFsSentinel;
    return;
  }
  const float ix = (tx + 1.0f) * ((float)(w - 1) / 2.0f), iy = (ty + 1.0f) * ((float)(h - 1) / 2.0f);
  fs_bilinear2(ix, iy, [&](int x, int y, float& vx, float& vy) { fs_aff_sentinel(p, x, y, h, w, vx, vy); }, ox, oy);
}

// the pixel-unit mapping `flow + grid` of unnormalise_and_convert_mapping_to_flow at integer (xi, yi); 0 outside the frame
__device__ __forceinline__ void fs_map_px(const FsParams& p, int xi, int yi, int h, int w, float& ox, float& oy) {
  ox = 0.0f, oy = 0.0f;
  if (xi < 0 || xi >= w || yi < 0 || yi >= h) return;
  float mx, my;
  fs_map_norm(p, xi, yi, h, w, mx, my);
  const float fx = (mx + 1.0f) * (float)(w - 1) / 2.0f - (float)xi, fy = (my + 1.0f) * (float)(h - 1) / 2.0f - (float)yi;
  ox = fx + (float)xi, oy = fy + (float)yi;
}

__global__ __launch_bounds__(kFsThreads) void flowsynth_flow_kernel(FsParams p, const float* __restrict__ field, int h, int w,
                                                                   float* __restrict__ flow, int* __restrict__ count) {
  const long plane = (long)h * w;
  const long i = (long)blockIdx.x * kFsThreads + threadIdx.x;
  bool inside = false;
  if (i < plane) {
    const int y = (int)(i / w), x = (int)(i - (long)y * w);
    float fx, fy;
    if (field == nullptr) {
      float mx, my;
      fs_map_norm(p, x, y, h, w, mx, my);
      fx = (mx + 1.0f) * (float)(w - 1) / 2.0f - (float)x, fy = (my + 1.0f) * (float)(h - 1) / 2.0f - (float)y;
    } else {
      float m = 0.0f;                          // the bump mask: every bump clamped to [0, 1], then their sum
#pragma unroll                                  // (compile-time indices into the kernel arguments, a wave-uniform skip)
      for (int b = 0; b < kFsMaxBumps; ++b) {
        if (b >= p.n_bumps) break;
        const FsBump g = p.bump[b];
        const float ry = (float)y - g.x, rx = (float)x - g.y;
        const float e1 = expf(-(ry * ry) / g.sig2), e2 = expf(-(rx * rx) / g.sig2);
        m += fminf(fmaxf(g.scale * (e1 * e2 / g.div), 0.0f), 1.0f);
      }
      m = fminf(fmaxf(m, 0.0f), 1.0f);
      const float px = field[i] * m, py = field[plane + i] * m;
      // warp(): grid + flow normalised to [-1, 1], un-normalised again by grid_sample(align_corners=True)
      const float gx = 2.0f * ((float)x + px) / (float)(w - 1) - 1.0f, gy = 2.0f * ((float)y + py) / (float)(h - 1) - 1.0f;
      const float ix = (gx + 1.0f) * ((float)(w - 1) / 2.0f), iy = (gy + 1.0f) * ((float)(h - 1) / 2.0f);
      float mx, my;
      fs_bilinear2(ix, iy, [&](int xi, int yi, float& vx, float& vy) { fs_map_px(p, xi, yi, h, w, vx, vy); }, mx, my);
      fx = mx - (float)x, fy = my - (float)y;
    }
    flow[i] = fx, flow[plane + i] = fy;
    const float bx = fx + (float)x, by = fy + (float)y;      // create_border_mask
    inside = bx >= 0.0f && bx <= (float)(w - 1) && by >= 0.0f && by <= (float)(h - 1);
  }
  __shared__ int s_cnt[kFsThreads / kWave];
  const int n = __popcll(__ballot(inside));
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int k = 0; k < kFsThreads / kWave; ++k) t += s_cnt[k];
    if (t != 0) atomicAdd(count, t);
  }
}

__global__ __launch_bounds__(kFsThreads) void flowsynth_warp_kernel(const float* __restrict__ image, const float* __restrict__ flow,
                                                                   const int* __restrict__ count, int h, int w, int top, int left,
                                                                   int ch, int cw, double min_valid, float* __restrict__ out_image,
                                                                   float* __restrict__ out_flow, unsigned char* __restrict__ out_mask) {
  const long cplane = (long)ch * cw, plane = (long)h * w;
  const long i = (long)blockIdx.x * kFsThreads + threadIdx.x;
  if (i >= cplane) return;
  const int cy = (int)(i / cw), cx = (int)(i - (long)cy * cw);
  const int y = cy + top, x = cx + left;
  const long o = (long)y * w + x;
  const float fx = flow[o], fy = flow[plane + o];
  const float gx = 2.0f * ((float)x + fx) / (float)(w - 1) - 1.0f, gy = 2.0f * ((float)y + fy) / (float)(h - 1) - 1.0f;
  const bool m_warp = gx > -1.0f && gy > -1.0f && gx < 1.0f && gy < 1.0f;
  const float bx = fx + (float)x, by = fy + (float)y;
  const bool m_border = bx >= 0.0f && bx <= (float)(w - 1) && by >= 0.0f && by <= (float)(h - 1);
  // (`mask.sum() < W * H * fraction`: an integer tensor against a Python float compares in fp32)
  const bool fallback = (float)count[0] < (float)((double)((long)w * h) * min_valid);
  const float ix = (gx + 1.0f) * ((float)(w - 1) / 2.0f), iy = (gy + 1.0f) * ((float)(h - 1) / 2.0f);
  const float ffx = floorf(ix), ffy = floorf(iy);
  const float wx1 = ix - ffx, wy1 = iy - ffy, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
  const float nw = wx0 * wy0, ne = wx1 * wy0, sw = wx0 * wy1, se = wx1 * wy1;
  const int x0 = (int)fminf(fmaxf(ffx, -2.0f), 2.0e9f), y0 = (int)fminf(fmaxf(ffy, -2.0f), 2.0e9f);
  const bool okx0 = x0 >= 0 && x0 < w, okx1 = x0 + 1 >= 0 && x0 + 1 < w, oky0 = y0 >= 0 && y0 < h, oky1 = y0 + 1 >= 0 && y0 + 1 < h;
  // (an address is formed for neighbours inside the frame only)
  const long a00 = okx0 && oky0 ? (long)y0 * w + x0 : -1, a01 = okx1 && oky0 ? (long)y0 * w + x0 + 1 : -1;
  const long a10 = okx0 && oky1 ? (long)(y0 + 1) * w + x0 : -1, a11 = okx1 && oky1 ? (long)(y0 + 1) * w + x0 + 1 : -1;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* __restrict__ im = image + c * plane;
    const float v00 = a00 >= 0 ? im[a00] : 0.0f, v01 = a01 >= 0 ? im[a01] : 0.0f;
    const float v10 = a10 >= 0 ? im[a10] : 0.0f, v11 = a11 >= 0 ? im[a11] : 0.0f;
    out_image[c * cplane + i] = v00 * nw + v01 * ne + v10 * sw + v11 * se;
  }
  out_flow[i] = fx, out_flow[cplane + i] = fy;
  out_mask[i] = (fallback ? m_border : m_warp) ? 1 : 0;
}

// BORDER_REFLECT_101 as often as needed: fold i by period 2(n - 1), n >= 2
__device__ __forceinline__ int fs_fold(int i, int n) {
  const int period = 2 * (n - 1);
  int r = i % period;
  r = r < 0 ? r + period : r;
  return r < n ? r : period - r;
}

// one output per lane, lanes along W.  ROWS: src is float, taps run along x; else src is double, taps run along y.  The walk
// over the reflected index starts folded and turns round at the ends, so the fold is computed once per output.
template <bool ROWS, typename Src, typename Dst>
__global__ __launch_bounds__(kFsThreads) void flowsynth_blur_kernel(const Src* __restrict__ src, const float* __restrict__ taps,
                                                                   int ntaps, int h, int w, Dst* __restrict__ dst) {
  const int x = blockIdx.x * kFsThreads + threadIdx.x, y = blockIdx.y;
  if (x >= w) return;
  const long plane = (long)h * w;
  const Src* __restrict__ s = src + (long)blockIdx.z * plane + (ROWS ? (long)y * w : (long)x);
  const int n = ROWS ? w : h, r = ntaps / 2;
  const long stride = ROWS ? 1 : w;
  const int start = (ROWS ? x : y) - r;
  int pos = fs_fold(start, n);
  // the direction of the walk at `start`: rising on the even half-periods of the unfolded index
  const int period = 2 * (n - 1);
  int m = start % period;
  m = m < 0 ? m + period : m;
  int dir = m < n - 1 ? 1 : -1;
  // Eight loads in flight per lane, then eight fused multiply-adds in tap order: a loop of load / wait / multiply / add waits
  // for vmcnt(0) every tap (seen in the ISA).  The sum's order does not depend on the unroll.
  const auto step = [&]() {
    const Src v = s[(long)pos * stride];
    pos += dir;
    if (pos == n - 1) dir = -1;
    if (pos == 0) dir = 1;
    return v;
  };
  double acc = 0.0;
  int k = 0;
  for (; k + kFsBlurUnroll <= ntaps; k += kFsBlurUnroll) {
    Src v[kFsBlurUnroll];
#pragma unroll
    for (int j = 0; j < kFsBlurUnroll; ++j) v[j] = step();
#pragma unroll
    for (int j = 0; j < kFsBlurUnroll; ++j) acc = __builtin_fma((double)taps[k + j], (double)v[j], acc);
  }
  for (; k < ntaps; ++k) acc = __builtin_fma((double)taps[k], (double)step(), acc);
  dst[(long)blockIdx.z * plane + (long)y * w + x] = (Dst)acc;
}

}  // namespace rfn

extern "C" {
using namespace rfn;

// see include/refign_hip.h
int rfn_flowsynth_flow_f32(const float* theta, int kind, const float* bumps, int n_bumps, const float* field, int h, int w,
                           float* flow, int* count, rfn_stream_t stream) {
  RFN_REQUIRE(theta && flow && count, "rfn_flowsynth_flow_f32: null pointer");
  RFN_REQUIRE(h >= 2 && w >= 2, "rfn_flowsynth_flow_f32: h=%d w=%d (each >= 2)", h, w);
  RFN_REQUIRE(kind >= 0 && kind <= 3, "rfn_flowsynth_flow_f32: kind %d (0 hom, 1 affine, 2 tps, 3 afftps)", kind);
  RFN_REQUIRE(n_bumps >= 0 && n_bumps <= kFsMaxBumps, "rfn_flowsynth_flow_f32: %d bumps (0 ... %d)", n_bumps, kFsMaxBumps);
  RFN_REQUIRE(n_bumps == 0 || (bumps && field), "rfn_flowsynth_flow_f32: bumps without a bump list or a field");
  FsParams p;
  for (int i = 0; i < 9; ++i) p.hom[i] = theta[i], p.wx[i] = theta[9 + i], p.wy[i] = theta[18 + i];
  for (int i = 0; i < 3; ++i) p.ax[i] = theta[27 + i], p.ay[i] = theta[30 + i];
  for (int i = 0; i < 6; ++i) p.aff[i] = theta[33 + i];
  p.kind = kind, p.n_bumps = n_bumps;
  for (int b = 0; b < kFsMaxBumps; ++b) {
    const float s = b < n_bumps ? bumps[4 * b + 2] : 1.0f;
    p.bump[b] = {b < n_bumps ? bumps[4 * b] : 0.0f, b < n_bumps ? bumps[4 * b + 1] : 0.0f, 2.0f * s * s,
                 (float)((double)s * (2.5066282746310002 * 2.5066282746310002)), b < n_bumps ? bumps[4 * b + 3] : 0.0f};
  }
  hipLaunchKernelGGL(flowsynth_flow_kernel, dim3((unsigned)cdiv((long)h * w, kFsThreads)), dim3(kFsThreads), 0, (hipStream_t)stream, p,
                     field, h, w, flow, count);
  return check_launch("flowsynth_flow_kernel");
}

int rfn_flowsynth_warp_f32(const float* image, const float* flow, const int* count, int h, int w, int top, int left, int ch, int cw,
                           double min_fraction_valid, float* out_image, float* out_flow, void* out_mask, rfn_stream_t stream) {
  RFN_REQUIRE(image && flow && count && out_image && out_flow && out_mask, "rfn_flowsynth_warp_f32: null pointer");
  RFN_REQUIRE(h >= 2 && w >= 2, "rfn_flowsynth_warp_f32: h=%d w=%d (each >= 2)", h, w);
  RFN_REQUIRE(ch >= 1 && cw >= 1 && top >= 0 && left >= 0 && top + ch <= h && left + cw <= w,
              "rfn_flowsynth_warp_f32: crop %d x %d at (%d, %d) does not lie in the %d x %d frame", ch, cw, top, left, h, w);
  hipLaunchKernelGGL(flowsynth_warp_kernel, dim3((unsigned)cdiv((long)ch * cw, kFsThreads)), dim3(kFsThreads), 0, (hipStream_t)stream,
                     image, flow, count, h, w, top, left, ch, cw, min_fraction_valid, out_image, out_flow, (unsigned char*)out_mask);
  return check_launch("flowsynth_warp_kernel");
}

int rfn_gaussian_blur_f32(const float* src, const float* taps, int ntaps, int planes, int h, int w, double* tmp, float* dst,
                          rfn_stream_t stream) {
  RFN_REQUIRE(src && taps && tmp && dst, "rfn_gaussian_blur_f32: null pointer");
  RFN_REQUIRE(h >= 2 && w >= 2 && planes >= 1 && planes <= 65535 && h <= 65535, "rfn_gaussian_blur_f32: planes=%d h=%d w=%d", planes, h, w);
  RFN_REQUIRE(ntaps >= 1 && (ntaps & 1), "rfn_gaussian_blur_f32: %d taps (odd, >= 1)", ntaps);
  const dim3 grid((unsigned)cdiv(w, kFsThreads), (unsigned)h, (unsigned)planes);
  hipLaunchKernelGGL((flowsynth_blur_kernel<true, float, double>), grid, dim3(kFsThreads), 0, (hipStream_t)stream, src, taps, ntaps, h, w,
                     tmp);
  int rc = check_launch("flowsynth_blur_kernel (rows)");
  if (rc != RFN_OK) return rc;
  hipLaunchKernelGGL((flowsynth_blur_kernel<false, double, float>), grid, dim3(kFsThreads), 0, (hipStream_t)stream,
                     (const double*)tmp, taps, ntaps, h, w, dst);
  return check_launch("flowsynth_blur_kernel (columns)");
}

}  // extern "C"
