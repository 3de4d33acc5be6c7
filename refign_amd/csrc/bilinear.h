// refign_amd/csrc/bilinear.h -- the two pieces of bilinear index arithmetic whose exact sequence of fp32 operations the parity
// tests depend on.  They live here and nowhere else:
//   * warp_tap / tap_sample: the four taps of warp() (helpers/matching_utils.py:11-49 on top of ATen grid_sampler_2d);
//   * up_src / up_src_nofma / up_cell_window: the source index of upsample_bilinear2d(align_corners=False) and its inverse.
// (flowsynth.hip's fs_bilinear2 is a different blend with a sentinel, and upcat.hip's backward window a narrower one: see there.)
#pragma once
#include <hip/hip_runtime.h>

namespace rfn {

// ---- warp(): grid = base + flow, normalised with max(W - 1, 1), grid_sample(bilinear, align_corners=True, zeros) ---------------
struct WarpTap {
  int o00, o01, o10, o11;        // clamped offsets of nw, ne, sw, se: always inside the plane
  float w00, w01, w10, w11;      // their weights, 0 for a tap outside the image (zero padding)
  bool inside;                   // strict-inequality validity of the NORMALISED coordinate (matching_utils.py:46-47)
  // what the backward needs on top (a forward kernel reads none of these and carries no instruction for them):
  float tx, ty;                  // fractional parts of the un-normalised coordinate
  bool v00, v01, v10, v11;       // tap inside the image
  bool finite;                   // both coordinates non-NaN and below 1e9 in magnitude: the pixel has a flow gradient
};

// One derivation of the validity flags serves the forward and the backward.  The conversion to int is guarded by a clamp of
// floor(ix) to [-2, W] (NaN: -2).  The backward's `finite` (|ix|, |iy| < 1e9, no NaN) would serve as the guard just as well --
// `finite ? (int)floor(ix) : -2` gives the same four flags for every fp32 input (W, H < 1e9; fp32 pixel coordinates stop being
// exact at 2^24): for |ix| >= 1e9, an infinity or a NaN the clamp yields W or -2, so x0 and x0 + 1 are both outside, as with -2;
// below 1e9 the conversion is exact, and the clamp moves only values below -2 or above W, for which x0 and x0 + 1 are outside
// before and after.  The same along y.  So the flags are derived once, here, and `finite` only gates the flow gradient.
__device__ __forceinline__ WarpTap warp_tap(float gx, float gy, float fx, float fy, int H, int W) {
#pragma clang fp contract(off)
  const float wm = (float)max(W - 1, 1), hm = (float)max(H - 1, 1);
  const float vx = 2.0f * (gx + fx) / wm - 1.0f;               // matching_utils.py:35
  const float vy = 2.0f * (gy + fy) / hm - 1.0f;               // matching_utils.py:36
  const float ix = ((vx + 1.0f) / 2.0f) * (float)(W - 1);      // ATen grid_sampler_unnormalize(align_corners)
  const float iy = ((vy + 1.0f) / 2.0f) * (float)(H - 1);
  float x0f = floorf(ix), y0f = floorf(iy);
  WarpTap t;
  t.tx = ix - x0f;
  t.ty = iy - y0f;
  x0f = fminf(fmaxf(x0f, -2.0f), (float)W);
  y0f = fminf(fmaxf(y0f, -2.0f), (float)H);
  if (!(ix == ix) || !(iy == iy)) { x0f = -2.0f; y0f = -2.0f; }
  const int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
  const bool vx0 = x0 >= 0 && x0 < W, vx1 = x1 >= 0 && x1 < W;
  const bool vy0 = y0 >= 0 && y0 < H, vy1 = y1 >= 0 && y1 < H;
  const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x1, 0), W - 1);
  const int cy0 = min(max(y0, 0), H - 1), cy1 = min(max(y1, 0), H - 1);
  t.o00 = cy0 * W + cx0; t.o01 = cy0 * W + cx1; t.o10 = cy1 * W + cx0; t.o11 = cy1 * W + cx1;
  t.v00 = vx0 && vy0; t.v01 = vx1 && vy0; t.v10 = vx0 && vy1; t.v11 = vx1 && vy1;
  const float ax = 1.0f - t.tx, ay = 1.0f - t.ty;
  t.w00 = t.v00 ? ax * ay : 0.0f;
  t.w01 = t.v01 ? t.tx * ay : 0.0f;
  t.w10 = t.v10 ? ax * t.ty : 0.0f;
  t.w11 = t.v11 ? t.tx * t.ty : 0.0f;
  t.inside = (vx > -1.0f) && (vy > -1.0f) && (vx < 1.0f) && (vy < 1.0f);
  t.finite = (ix == ix) && (iy == iy) && fabsf(ix) < 1e9f && fabsf(iy) < 1e9f;
  return t;
}

// products rounded one by one, added in ATen grid_sampler_2d's order: nw, ne, sw, se
__device__ __forceinline__ float tap_sample(const float* __restrict__ src, const WarpTap& t) {
#pragma clang fp contract(off)
  return src[t.o00] * t.w00 + src[t.o01] * t.w01 + src[t.o10] * t.w10 + src[t.o11] * t.w11;
}

// ---- upsample_bilinear2d(align_corners=False): ATen area_pixel_compute_source_index + the neighbours and the weight of i1 ------
// s = max(scale (dst + 0.5) - 0.5, 0), i0 = min(int(s), in - 1), i1 = min(i0 + 1, in - 1), l1 = s - i0 (the weight of i0: 1 - l1).
// TWO forms, which differ in the last bit of l1 wherever scale (dst + 0.5) is not exact -- a kernel keeps the one it has:
//   up_src        the product and the subtraction contract into one fma: det.hip, loss.hip, evaltail.hip, flowloss.hip, upcat.hip;
//   up_src_nofma  both rounded, as ATen's host-side arithmetic does: warp.hip align_tail_kernel.
// CLAMP = false leaves out the clamp of i0 for a caller that only up-samples (scale <= 1: s < in - 0.5, the clamp is a no-op):
// upcat.hip, whose gather backward runs up_src in its innermost loop and is measurably slower with it.
template <bool CLAMP>
__device__ __forceinline__ void up_split(float s, int in, int& i0, int& i1, float& l1) {
  if constexpr (CLAMP) {
    i0 = min((int)s, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
  } else {
    i0 = (int)s;
    i1 = min(i0 + 1, in - 1);                    // (the same neighbour, in the spelling upcat.hip compiled before)
  }
  l1 = s - (float)i0;
}
template <bool CLAMP = true>
__device__ __forceinline__ void up_src(int dst, float scale, int in, int& i0, int& i1, float& l1) {
  up_split<CLAMP>(fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f), in, i0, i1, l1);
}
__device__ __forceinline__ void up_src_nofma(int dst, float scale, int in, int& i0, int& i1, float& l1) {
  float s;
  {
#pragma clang fp contract(off)
    s = scale * ((float)dst + 0.5f) - 0.5f;
  }
  up_split<true>(fmaxf(s, 0.f), in, i0, i1, l1);
}

// The inverse: the first output index whose i0 or i1 can be `cell`, and one past the last.  A conservative window (the callers
// test the membership exactly per output pixel or tile); cells 0 and 1 are also read by the outputs whose source index was clamped
// to 0, with weight 1 and 0.
__device__ __forceinline__ void up_cell_window(int cell, float scale, int out_size, int& lo, int& hi) {
  const float inv = 1.f / scale;
  lo = cell <= 1 ? 0 : max(0, (int)floorf(((float)cell - 0.5f) * inv - 0.5f) - 1);
  hi = min(out_size, (int)ceilf(((float)cell + 1.5f) * inv - 0.5f) + 2);
}

}  // namespace rfn
