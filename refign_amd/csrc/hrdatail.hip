// refign_amd/csrc/hrdatail.hip -- the HRDA logit merge (the end of seg.hrda_head) in one kernel per direction.
//
// Reference: models/hrda.py:139-235.  From the scale-attention logits `a` and the low-resolution class logits `lr` (both (n, K, h, w))
// and the class logits `hr` of the high-resolution crop(s), on the (2h, 2w) grid:
//   teacher / eval (hrda.py:196-235)   out = up2(sigmoid(a)) * (sum_i crop_i / count) + up2((1 - sigmoid(a)) * lr)
//   student (hrda.py:152-194)          out = up2(att) * insert(hr) + up2((1 - att) * lr),   att = sigmoid(a) * mask
// up2 = bilinear x2, align_corners=False.  Unfused that is 30 launches (teacher: two new_zeros, 9 + 9 slice additions, ...) or about
// 20 forward and as many backward (student), each a pass over a 19-channel map, on the critical path of the step's front half and
// at the two ends of every student pass.  Here one thread owns one output element and reads its <= 4 low-resolution taps (L2) and
// its crop pixel(s); the backward is a gather (every low-resolution cell adds the <= 4 x 4 outputs that read it): no atomics, no
// zero fill, deterministic.
//
// Operands are bf16, the result fp32: the step's bf16 autocast.  FORWARD arithmetic is the unfused chain's, rounding for rounding,
// so that the result is bit-equal to it: under autocast the element-wise steps store bf16 (sigmoid, mask product, 1 - att, product
// with lr, the crop sum after EVERY addition, the division by the count), the up-samplings and the final product and sum are fp32
// (ATen's operand order and bilinear.h's weights; the product and the sum are two roundings, never an fma).  The blend's products
// of bf16 values with the x2 weights (1/4, 3/4) are exact in fp32, and so are their sums unless neighbouring taps are more than
// 2^12 apart in magnitude: the compiler's choice of fma does not show.  With fp32 operands it does (measured: 1 ulp apart from ATen
// in either direction), so the entry points take bf16 only and everything else stays on the chain.  The BACKWARD differentiates the
// formula itself in fp64 and rounds once to bf16.  Open: every thread pays six 64-bit index divisions (and four for the crop offset)
// and reads 19 of a padded pixel's 64 channels -- 57-109 us per launch against a byte floor near 10 us (profiles/hrda_tail_ab.txt).
// Operands are addressed by their four strides (the decode head hands over channels-last views of 64-channel padded buffers);
// results are dense channels-last, what the unfused chain returns.
#include <hip/hip_bf16.h>

#include "bilinear.h"
#include "common.h"
#include "elem.h"

namespace rfn {

constexpr int kHrdaMaxBoxes = 16;

struct HrdaMap {               // an (n, K, rows, cols) operand: element strides
  const void* p;
  long sn, sc, sh, sw;
};
struct HrdaBoxes {             // sliding-crop boxes on the (2h, 2w) grid, by value
  int nb;
  int y1[kHrdaMaxBoxes], y2[kHrdaMaxBoxes], x1[kHrdaMaxBoxes], x2[kHrdaMaxBoxes];
};

template <typename T>
__device__ __forceinline__ float hrda_ld(const HrdaMap& m, long n, int c, long y, long x) {
  return ldf<T>(reinterpret_cast<const T*>(m.p) + n * m.sn + c * m.sc + y * m.sh + x * m.sw);
}

// ATen's upsample_bilinear2d blend: operand order and grouping of UpSampleBilinear2d.cu (contraction left to the compiler, as there)
__device__ __forceinline__ float hrda_blend(float ly, float lx, float v00, float v01, float v10, float v11) {
  const float hy = 1.0f - ly, hx = 1.0f - lx;
  return hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
}

// a * b + c as the two kernels `mul` and `add`: two roundings
__device__ __forceinline__ float hrda_mul_add(float a, float b, float c) {
#pragma clang fp contract(off)
  const float p = a * b;
  return p + c;
}

// one low-resolution tap: att = sigmoid(a) [* mask] and (1 - att) * lr, each step stored as T
template <typename T>
__device__ __forceinline__ void hrda_tap(float av, float lv, bool masked, bool inmask, float& att, float& tl) {
  const float s = round_to<T>(1.0f / (1.0f + expf(-av)));
  att = !masked || inmask ? s : s * 0.0f;
  const float om = round_to<T>(1.0f - att);
  tl = round_to<T>(om * lv);
}

struct HrdaCrop {              // student: the mask box on the (h, w) grid and the insert box on the (2h, 2w) grid
  long my0, mx0, iy0, ix0;
};
__device__ __forceinline__ HrdaCrop hrda_crop(const long* __restrict__ off, int div_mask, int div_ins) {
  const long oy = off[0], ox = off[1];
  return HrdaCrop{oy / div_mask, ox / div_mask, oy / div_ins, ox / div_ins};
}

// MODE 0: teacher (boxes), MODE 1: student (device offset)
template <typename T, int MODE>
__global__ __launch_bounds__(256) void hrda_merge_fwd_kernel(HrdaMap a, HrdaMap lr, HrdaMap hr, HrdaBoxes bx,
                                                             const long* __restrict__ off, float* __restrict__ out, int nl, int K,
                                                             int h, int w, int hc, int wc, int mh, int mw, int div_mask,
                                                             int div_ins, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;                              // total = nl * 2h * 2w * K, channel fastest
  const int H = 2 * h, W = 2 * w;
  const int c = (int)(idx % K);
  long pix = idx / K;
  const int X = (int)(pix % W);
  pix /= W;
  const int Y = (int)(pix % H);
  const long n = pix / H;
  int y0, y1, x0, x1;
  float ly, lx;
  up_src(Y, 0.5f, h, y0, y1, ly);
  up_src(X, 0.5f, w, x0, x1, lx);
  HrdaCrop cr{0, 0, 0, 0};
  if constexpr (MODE == 1) cr = hrda_crop(off, div_mask, div_ins);
  const int ys[2] = {y0, y1}, xs[2] = {x0, x1};
  float att[4], tl[4];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long ry = ys[i] - cr.my0, rx = xs[j] - cr.mx0;
      const bool inmask = ry >= 0 && ry < mh && rx >= 0 && rx < mw;
      hrda_tap<T>(hrda_ld<T>(a, n, c, ys[i], xs[j]), hrda_ld<T>(lr, n, c, ys[i], xs[j]), MODE == 1, inmask, att[2 * i + j],
                  tl[2 * i + j]);
    }
  }
  const float ua = hrda_blend(ly, lx, att[0], att[1], att[2], att[3]);
  const float ul = hrda_blend(ly, lx, tl[0], tl[1], tl[2], tl[3]);
  float q;
  if constexpr (MODE == 0) {
    float acc = 0.0f, cnt = 0.0f;                        // preds and count of hrda.py:209-219, in box order, stored as T
    for (int i = 0; i < bx.nb; ++i) {
      if (Y >= bx.y1[i] && Y < bx.y2[i] && X >= bx.x1[i] && X < bx.x2[i]) {
        acc = round_to<T>(acc + hrda_ld<T>(hr, (long)i * nl + n, c, Y - bx.y1[i], X - bx.x1[i]));
        cnt = cnt + 1.0f;
      }
    }
    q = round_to<T>(acc / cnt);                          // (the host refuses boxes that leave a pixel uncovered)
  } else {
    const long ry = Y - cr.iy0, rx = X - cr.ix0;
    q = ry >= 0 && ry < hc && rx >= 0 && rx < wc ? hrda_ld<T>(hr, n, c, ry, rx) : 0.0f;
  }
  out[idx] = hrda_mul_add(ua, q, ul);
}

// ---- student backward, fp64 -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ double hrda_sigmoid64(float a) { return 1.0 / (1.0 + exp(-(double)a)); }

// grad_a and grad_lr of low-resolution element idx = (n, y, x, c)
template <typename T>
__device__ __forceinline__ void hrda_crop_bwd_lr(const HrdaMap& g, const HrdaMap& a, const HrdaMap& lr, const HrdaMap& hr,
                                                 const long* __restrict__ off, T* __restrict__ g_a, T* __restrict__ g_lr, int K,
                                                 int h, int w, int hc, int wc, int mh, int mw, int div_mask, int div_ins,
                                                 long idx) {
  const int H = 2 * h, W = 2 * w;
  const int c = (int)(idx % K);
  long pix = idx / K;
  const int x = (int)(pix % w);
  pix /= w;
  const int y = (int)(pix % h);
  const long n = pix / h;
  const HrdaCrop cr = hrda_crop(off, div_mask, div_ins);
  double t = 0.0, u = 0.0;                               // up2^T(g * insert(hr)), up2^T(g)
  const int Ylo = max(0, 2 * y - 1), Yhi = min(H - 1, 2 * y + 2), Xlo = max(0, 2 * x - 1), Xhi = min(W - 1, 2 * x + 2);
  for (int Y = Ylo; Y <= Yhi; ++Y) {
    int i0, i1;
    float l;
    up_src(Y, 0.5f, h, i0, i1, l);
    const float wy = (i0 == y ? 1.0f - l : 0.0f) + (i1 == y ? l : 0.0f);
    if (wy == 0.0f) continue;
    const long ry = Y - cr.iy0;
    for (int X = Xlo; X <= Xhi; ++X) {
      up_src(X, 0.5f, w, i0, i1, l);
      const float wx = (i0 == x ? 1.0f - l : 0.0f) + (i1 == x ? l : 0.0f);
      if (wx == 0.0f) continue;
      const double gw = (double)wy * (double)wx * (double)hrda_ld<float>(g, n, c, Y, X);
      u += gw;
      const long rx = X - cr.ix0;
      if (ry >= 0 && ry < hc && rx >= 0 && rx < wc) t += gw * (double)hrda_ld<T>(hr, n, c, ry, rx);
    }
  }
  const long my = y - cr.my0, mx = x - cr.mx0;
  const bool inmask = my >= 0 && my < mh && mx >= 0 && mx < mw;
  const double s = hrda_sigmoid64(hrda_ld<T>(a, n, c, y, x)), lv = (double)hrda_ld<T>(lr, n, c, y, x);
  const double att = inmask ? s : 0.0;
  stf(g_lr + idx, (float)((1.0 - att) * u));
  stf(g_a + idx, (float)(inmask ? (t - lv * u) * s * (1.0 - s) : 0.0));
}

// grad_hr = crop(up2(att) * g) of crop element idx = (n, yh, xh, c)
template <typename T>
__device__ __forceinline__ void hrda_crop_bwd_hr(const HrdaMap& g, const HrdaMap& a, const long* __restrict__ off,
                                                 T* __restrict__ g_hr, int K, int h, int w, int hc, int wc, int mh, int mw,
                                                 int div_mask, int div_ins, long idx) {
  const int H = 2 * h, W = 2 * w;
  const int c = (int)(idx % K);
  long pix = idx / K;
  const int xh = (int)(pix % wc);
  pix /= wc;
  const int yh = (int)(pix % hc);
  const long n = pix / hc;
  const HrdaCrop cr = hrda_crop(off, div_mask, div_ins);
  const long Yl = cr.iy0 + yh, Xl = cr.ix0 + xh;
  double r = 0.0;
  if (Yl >= 0 && Yl < H && Xl >= 0 && Xl < W) {          // a crop pixel outside the grid was never read
    const int Y = (int)Yl, X = (int)Xl;
    int y0, y1, x0, x1;
    float ly, lx;
    up_src(Y, 0.5f, h, y0, y1, ly);
    up_src(X, 0.5f, w, x0, x1, lx);
    const int ys[2] = {y0, y1}, xs[2] = {x0, x1};
    const double wys[2] = {1.0 - (double)ly, (double)ly}, wxs[2] = {1.0 - (double)lx, (double)lx};
    double ua = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const long my = ys[i] - cr.my0, mx = xs[j] - cr.mx0;
        if (my >= 0 && my < mh && mx >= 0 && mx < mw) ua += wys[i] * wxs[j] * hrda_sigmoid64(hrda_ld<T>(a, n, c, ys[i], xs[j]));
      }
    }
    r = ua * (double)hrda_ld<float>(g, n, c, Y, X);
  }
  stf(g_hr + idx, (float)r);
}

// the whole backward: threads [0, tot_lr) own a low-resolution element each, threads [tot_lr, tot_lr + tot_hr) a crop element
template <typename T>
__global__ __launch_bounds__(256) void hrda_crop_bwd_kernel(HrdaMap g, HrdaMap a, HrdaMap lr, HrdaMap hr,
                                                            const long* __restrict__ off, T* __restrict__ g_a,
                                                            T* __restrict__ g_lr, T* __restrict__ g_hr, int K, int h, int w, int hc,
                                                            int wc, int mh, int mw, int div_mask, int div_ins, long tot_lr,
                                                            long tot_hr) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx < tot_lr) hrda_crop_bwd_lr<T>(g, a, lr, hr, off, g_a, g_lr, K, h, w, hc, wc, mh, mw, div_mask, div_ins, idx);
  else if (idx < tot_lr + tot_hr) hrda_crop_bwd_hr<T>(g, a, off, g_hr, K, h, w, hc, wc, mh, mw, div_mask, div_ins, idx - tot_lr);
}

static HrdaMap hrda_map(const void* p, const long* st) { return HrdaMap{p, st[0], st[1], st[2], st[3]}; }

// every pixel of rows x cols inside at least one box: on the grid cut at the boxes' edges (<= 33 x 33 cells)
static bool hrda_boxes_cover(const int* b, int nb, int rows, int cols) {
  int ye[2 * kHrdaMaxBoxes + 2], xe[2 * kHrdaMaxBoxes + 2], ny = 0, nx = 0;
  ye[ny++] = 0;
  xe[nx++] = 0;
  for (int i = 0; i < nb; ++i) {
    ye[ny++] = b[4 * i];
    ye[ny++] = b[4 * i + 1];
    xe[nx++] = b[4 * i + 2];
    xe[nx++] = b[4 * i + 3];
  }
  for (int iy = 0; iy < ny; ++iy) {
    if (ye[iy] < 0 || ye[iy] >= rows) continue;          // a cell starts at an edge inside the grid
    for (int ix = 0; ix < nx; ++ix) {
      if (xe[ix] < 0 || xe[ix] >= cols) continue;
      bool in = false;
      for (int i = 0; i < nb && !in; ++i)
        in = ye[iy] >= b[4 * i] && ye[iy] < b[4 * i + 1] && xe[ix] >= b[4 * i + 2] && xe[ix] < b[4 * i + 3];
      if (!in) return false;
    }
  }
  return true;
}

}  // namespace rfn

using namespace rfn;

extern "C" {

int rfn_hrda_merge_slide(const void* a, const long* a_strides, const void* lr, const long* lr_strides, const void* hr,
                         const long* hr_strides, const int* boxes, int nb, float* out, int nl, int K, int h, int w, int hc, int wc,
                         int dtype, int* accepted, rfn_stream_t stream) {
  RFN_REQUIRE(a && a_strides && lr && lr_strides && hr && hr_strides && boxes && out && accepted && nb > 0 && nl > 0 && K > 0 &&
                  h > 0 && w > 0 && hc > 0 && wc > 0,
              "rfn_hrda_merge_slide: bad arguments");
  RFN_REQUIRE(dtype == 1, "rfn_hrda_merge_slide: bf16 operands only (dtype 1, got %d)", dtype);
  const long total = (long)nl * 2 * h * 2 * w * K;
  RFN_REQUIRE(total / 256 < 0x7fffffffL && h < (1 << 29) && w < (1 << 29), "rfn_hrda_merge_slide: too large");
  *accepted = 0;
  if (nb > kHrdaMaxBoxes) return RFN_OK;
  HrdaBoxes bx;
  int ymax = 0, xmax = 0;
  for (int i = 0; i < nb; ++i) {
    const int y1 = boxes[4 * i], y2 = boxes[4 * i + 1], x1 = boxes[4 * i + 2], x2 = boxes[4 * i + 3];
    // a box is a whole crop inside the grid (what the slice addition of the unfused path needs as well)
    if (y1 < 0 || x1 < 0 || y2 - y1 != hc || x2 - x1 != wc || y2 > 2 * h || x2 > 2 * w) return RFN_OK;
    bx.y1[i] = y1; bx.y2[i] = y2; bx.x1[i] = x1; bx.x2[i] = x2;
    ymax = y2 > ymax ? y2 : ymax;
    xmax = x2 > xmax ? x2 : xmax;
  }
  bx.nb = nb;
  if (ymax != 2 * h || xmax != 2 * w || !hrda_boxes_cover(boxes, nb, 2 * h, 2 * w)) return RFN_OK;
  *accepted = 1;
  const HrdaMap ma = hrda_map(a, a_strides), ml = hrda_map(lr, lr_strides), mh_ = hrda_map(hr, hr_strides);
  using T = __hip_bfloat16;
  hipLaunchKernelGGL((hrda_merge_fwd_kernel<T, 0>), dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, ma, ml, mh_, bx,
                     (const long*)nullptr, out, nl, K, h, w, hc, wc, 0, 0, 1, 1, total);
  return check_launch("hrda_merge_fwd_kernel<slide>");
}

int rfn_hrda_fuse_crop_fwd(const void* a, const long* a_strides, const void* lr, const long* lr_strides, const void* hr,
                           const long* hr_strides, const long* off, float* out, int n, int K, int h, int w, int hc, int wc, int mh,
                           int mw, int div_mask, int div_ins, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(a && a_strides && lr && lr_strides && hr && hr_strides && off && out && n > 0 && K > 0 && h > 0 && w > 0 && hc > 0 &&
                  wc > 0 && mh >= 0 && mw >= 0 && div_mask > 0 && div_ins > 0,
              "rfn_hrda_fuse_crop_fwd: bad arguments");
  RFN_REQUIRE(dtype == 1, "rfn_hrda_fuse_crop_fwd: bf16 operands only (dtype 1, got %d)", dtype);
  const long total = (long)n * 2 * h * 2 * w * K;
  RFN_REQUIRE(total / 256 < 0x7fffffffL && h < (1 << 29) && w < (1 << 29), "rfn_hrda_fuse_crop_fwd: too large");
  const HrdaMap ma = hrda_map(a, a_strides), ml = hrda_map(lr, lr_strides), mh_ = hrda_map(hr, hr_strides);
  HrdaBoxes bx;
  bx.nb = 0;
  using T = __hip_bfloat16;
  hipLaunchKernelGGL((hrda_merge_fwd_kernel<T, 1>), dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, ma, ml, mh_, bx,
                     off, out, n, K, h, w, hc, wc, mh, mw, div_mask, div_ins, total);
  return check_launch("hrda_merge_fwd_kernel<crop>");
}

int rfn_hrda_fuse_crop_bwd(const float* grad_out, const long* g_strides, const void* a, const long* a_strides, const void* lr,
                           const long* lr_strides, const void* hr, const long* hr_strides, const long* off, void* grad_a,
                           void* grad_lr, void* grad_hr, int n, int K, int h, int w, int hc, int wc, int mh, int mw, int div_mask,
                           int div_ins, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(grad_out && g_strides && a && a_strides && lr && lr_strides && hr && hr_strides && off && grad_a && grad_lr &&
                  grad_hr && n > 0 && K > 0 && h > 0 && w > 0 && hc > 0 && wc > 0 && mh >= 0 && mw >= 0 && div_mask > 0 &&
                  div_ins > 0,
              "rfn_hrda_fuse_crop_bwd: bad arguments");
  RFN_REQUIRE(dtype == 1, "rfn_hrda_fuse_crop_bwd: bf16 operands only (dtype 1, got %d)", dtype);
  const long tot_lr = (long)n * h * w * K, tot_hr = (long)n * hc * wc * K;
  RFN_REQUIRE((tot_lr + tot_hr) / 256 < 0x7fffffffL && h < (1 << 29) && w < (1 << 29),
              "rfn_hrda_fuse_crop_bwd: too large");
  const HrdaMap mg = hrda_map(grad_out, g_strides), ma = hrda_map(a, a_strides), ml = hrda_map(lr, lr_strides),
                mh_ = hrda_map(hr, hr_strides);
  using T = __hip_bfloat16;
  hipLaunchKernelGGL((hrda_crop_bwd_kernel<T>), dim3(cdiv(tot_lr + tot_hr, 256)), dim3(256), 0, (hipStream_t)stream, mg, ma, ml,
                     mh_, off, (T*)grad_a, (T*)grad_lr, (T*)grad_hr, K, h, w, hc, wc, mh, mw, div_mask, div_ins, tot_lr, tot_hr);
  return check_launch("hrda_crop_bwd_kernel");
}

}  // extern "C"
