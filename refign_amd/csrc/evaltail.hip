// refign_amd/csrc/evaltail.hip -- the tail of the evaluation forward in one kernel: from the head's LOW-resolution crop logits
// to arg-max labels and confusion counts.
//
// Reference: models/segmentation_model.py:304-382 (whole_inference / slide_inference: every crop's logits up-sampled to the
// crop size with F.interpolate(bilinear, align_corners=False), summed into an image-sized tensor, divided by a count tensor)
// followed by helpers/metrics.py IoU.update (arg-max, target * C + prediction, bincount).  Unfused, a 1080 x 1920 image with
// three 1080 x 1080 crops moves about 2.2 GB through HBM in some twenty launches, with a host synchronisation in the middle
// (`assert (count == 0).sum() == 0`), to produce C x C integers.  Here the up-sampled logits never exist:
//   * a workgroup owns 16 x 16 tiles of image pixels (one pixel per lane) and walks over tiles, grid <= 1024 workgroups;
//   * per box that overlaps the tile, the low-resolution cells under the overlap (its bilinear footprint, all C classes) go to
//     LDS as fp32, classes innermost, so that a lane reads the classes of one of its four cells with 16-byte LDS loads at
//     compile-time offsets -- or are read from global memory directly when the footprint does not fit (scale factors near 1
//     and above);
//   * every lane keeps its pixel's C running sums in registers (ATen's source-index rule and operand order), divides by its box
//     count and takes the first largest class;
//   * counts go to a C x C histogram in LDS (integer atomics) that is added to the global matrix once per workgroup, non-zero
//     entries only, with 64-bit integer atomics.  Integer adds commute: the result does not depend on scheduling.
// That every pixel lies in some box is checked on the HOST from the box list (no device-side assert, no synchronisation).
//
// Two entry points, two kernels:
//   rfn_slide_argmax_confmat          labels, target and counts on the image grid (B, H, W): the list above;
//   rfn_slide_argmax_confmat_resized  on another grid (B, Ho, Wo) -- forward(x, out_size): the `test:` sections that resize the
//                                     image only (540 x 960 images, 1080 x 1920 labels) and predict_step's orig_dims.  Per output
//                                     pixel the bilinear sample (align_corners = False, scale H / Ho, clamped) of m on the image
//                                     grid, then the arg-max; m under a tile of output pixels lives in a second LDS buffer, so
//                                     neither the image-sized nor the label-sized logits (158 MB of fp32 at 19 x 1080 x 1920)
//                                     exist.  With Ho == H, Wo == W it is bit-equal to the first (slide_argmax_confmat_resized_kernel).
// Under 16-bit autocast forward() rounds its intermediate tensors to 16 bits; both kernels keep fp32 from the crop logits to the
// arg-max.
#include "bilinear.h"
#include "common.h"
#include "elem.h"

namespace rfn {

constexpr int kEtTH = 16, kEtTW = 16;          // image pixels per tile (one per lane of a 256-lane workgroup)
constexpr int kEtMaxC = 32, kEtMaxBox = 64;
constexpr int kEtCap = 4608;                   // fp32 values of staged footprint (18 KB): 230 cells of 19 (padded to 20) classes
constexpr int kEtMaxGrid = 1024;               // ~4 workgroups per CU: the flush is <= 1024 x C x C atomics
constexpr int kEtMidCap = 4096;                // resized kernel: fp32 values of m under an output tile (16 KB): 204 image pixels of 19
                                               // (padded to 20) classes -- a 14 x 14 footprint, any up-scaling from x 4/3

struct EtBoxes {
  int v[kEtMaxBox * 4];                        // (y1, y2, x1, x2) per box; travels in the kernel arguments
};

// ---- the pieces of slide_argmax_confmat_resized_kernel (below) ---------------------------------------------------------------------
// et_mean / et_divide / et_label / et_flush restate, statement by statement, the body of slide_argmax_confmat_kernel with the tile
// turned into a parameter (a rectangle of image pixels).  That kernel does NOT call them: built from these functions it computes
// the same bits but hipcc schedules it differently (2197 -> 2224 instructions, 108 -> 102 VGPRs for <fp32, 19>), and its
// --kernel-only rows came out 3 - 4 % above the parent build's in three alternations (profiles/eval_tail_resize_ab.txt), outside
// that build's own spread -- so it keeps its text, and tests/test_evaltail_resize_gpu.py holds the two to the same bits.
// LDS of the resized kernel, at namespace scope so that the functions address it as LDS (a pointer parameter came out as flat loads)
__shared__ __attribute__((aligned(16))) float et_lo[kEtCap];       // [fy][fx][S]: crop logits under a rectangle of image pixels
__shared__ __attribute__((aligned(16))) float et_mid[kEtMidCap];   // [iy][ix][S], or [output pixel of the pass][tap][S]: m
__shared__ unsigned et_hist[kEtMaxC * kEtMaxC];                    // [target][label]
__shared__ int et_sbox[kEtMaxBox * 4];

// a cell's classes side by side, rows of S floats: 16-byte aligned, and S / 4 odd so that neighbouring cells start in other banks
template <int CMAX>
constexpr int et_row() {
  return ((CMAX + 3) / 4 * 4) + ((CMAX + 3) / 4 % 2 ? 0 : 4);
}

// m(y, x) of image b into acc[0 .. C): over the boxes that contain the pixel, the mean of the bilinear samples of their crop logits.
// Called by the WHOLE workgroup (the staging synchronises): [Y0, Y1) x [X0, X1) is a rectangle of image pixels, the same for every
// lane, that holds the pixel of every live lane; a lane that is not live only helps with the staging.
template <int DT, int CMAX>
__device__ __forceinline__ int et_mean(const void* __restrict__ crops, int nbox, int B, int C, int h, int w, int H,
                                        int W, float sy, float sx, int b, int Y0, int Y1, int X0, int X1, int y, int x, bool live,
                                        float (&acc)[CMAX]) {
  constexpr int S = et_row<CMAX>();
  const int tid = threadIdx.x;
  const long plane = (long)h * w;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) acc[c] = 0.f;
  int cnt = 0;
  for (int k = 0; k < nbox; ++k) {
    const int y1 = et_sbox[4 * k], y2 = et_sbox[4 * k + 1], x1 = et_sbox[4 * k + 2], x2 = et_sbox[4 * k + 3];
    // the rectangle's pixels inside this box (the same for every lane)
    const int ya = max(Y0, y1), yb = min(min(Y1, y2), H) - 1;
    const int xa = max(X0, x1), xb = min(min(X1, x2), W) - 1;
    if (ya > yb || xa > xb) continue;
    int fy0, fy1, fx0, fx1, t0, t1;
    float l;
    up_src(ya - y1, sy, h, fy0, t1, l);
    up_src(yb - y1, sy, h, t0, fy1, l);
    up_src(xa - x1, sx, w, fx0, t1, l);
    up_src(xb - x1, sx, w, t0, fx1, l);
    const int nfy = fy1 - fy0 + 1, nfx = fx1 - fx0 + 1, cells = nfy * nfx;
    const bool staged = cells * S <= kEtCap;
    const long base = ((long)k * B + b) * C * plane;             // crop k of image b: row k * B + b
    if (staged) {
      __syncthreads();                                            // the previous footprint has been read
      // lane <-> cell, wave <-> every fourth class: one integer division per cell, rows of the footprint read side by side
      for (int q = tid & 63; q < cells; q += 64) {
        const int fy = q / nfx, fx = q - fy * nfx;
        const long off = base + (long)(fy0 + fy) * w + fx0 + fx;
        for (int c = tid >> 6; c < C; c += 4) et_lo[q * S + c] = ldf<DT>(crops, off + c * plane);
      }
      __syncthreads();
    }
    if (live && y >= y1 && y < y2 && x >= x1 && x < x2) {
      int a0, a1, b0, b1;
      float ly, lx;
      up_src(y - y1, sy, h, a0, a1, ly);
      up_src(x - x1, sx, w, b0, b1, lx);
      const float hy = 1.f - ly, hx = 1.f - lx;
      ++cnt;
      if (staged) {
        const float* p00 = et_lo + ((a0 - fy0) * nfx + b0 - fx0) * S;
        const float* p01 = et_lo + ((a0 - fy0) * nfx + b1 - fx0) * S;
        const float* p10 = et_lo + ((a1 - fy0) * nfx + b0 - fx0) * S;
        const float* p11 = et_lo + ((a1 - fy0) * nfx + b1 - fx0) * S;
        // (all CMAX classes, no guard: the loads merge into 16-byte ones; the sums of classes >= C hold whatever the rows'
        // padding held and are never looked at)
#pragma unroll
        for (int c = 0; c < CMAX; ++c) acc[c] += hy * (hx * p00[c] + lx * p01[c]) + ly * (hx * p10[c] + lx * p11[c]);
      } else {
        const long o00 = base + (long)a0 * w + b0, o01 = base + (long)a0 * w + b1;
        const long o10 = base + (long)a1 * w + b0, o11 = base + (long)a1 * w + b1;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
          if (c < C) {
            const long pc = c * plane;
            acc[c] += hy * (hx * ldf<DT>(crops, o00 + pc) + lx * ldf<DT>(crops, o01 + pc)) +
                      ly * (hx * ldf<DT>(crops, o10 + pc) + lx * ldf<DT>(crops, o11 + pc));
          }
        }
      }
    }
  }
  return cnt;
}

// the sums of et_mean over its count of boxes
template <int CMAX>
__device__ __forceinline__ void et_divide(float (&acc)[CMAX], int cnt) {
  const float n = (float)max(cnt, 1);                             // (cnt >= 1: the host checked the cover)
  if ((cnt & (cnt - 1)) == 0) {                                   // 1, 2, 4, ... boxes: the reciprocal is exact, x / n == x * (1 / n)
    const float rn = 1.f / n;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) acc[c] *= rn;
  } else {
#pragma unroll
    for (int c = 0; c < CMAX; ++c) acc[c] /= n;
  }
}

// the first largest class of v[0 .. C) -> the label; counted against the target at element gi of the (B, rows, cols) grid
template <int CMAX>
__device__ __forceinline__ void et_label(const float (&v)[CMAX], int C, long gi, const long* __restrict__ target, int ignore_index,
                                         unsigned char* __restrict__ labels) {
  float best = v[0];
  int label = 0;
#pragma unroll
  for (int c = 1; c < CMAX; ++c) {
    if (c < C && v[c] > best) {
      best = v[c];
      label = c;
    }
  }
  if (labels != nullptr) labels[gi] = (unsigned char)label;
  if (target != nullptr) {
    const long t = target[gi];
    if (t != (long)ignore_index && t >= 0 && t < C) atomicAdd(&et_hist[(int)t * C + label], 1u);
  }
}

// the workgroup's histogram added to the global matrix, non-zero entries only
__device__ __forceinline__ void et_flush(int C, unsigned long long* __restrict__ confmat) {
  if (confmat != nullptr) {
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += 256) {
      const unsigned v = et_hist[i];
      if (v != 0u) atomicAdd(confmat + i, (unsigned long long)v);
    }
  }
}

template <int DT, int CMAX>
__global__ __launch_bounds__(256, CMAX <= 19 ? 4 : 3) void slide_argmax_confmat_kernel(const void* __restrict__ crops, EtBoxes boxes, int nbox,
                                                                   int B, int C, int h, int w, int H, int W, float sy,
                                                                   float sx, const long* __restrict__ target,
                                                                   int ignore_index, unsigned char* __restrict__ labels,
                                                                   unsigned long long* __restrict__ confmat) {
  // a cell's classes side by side, rows of S floats: 16-byte aligned, and S / 4 odd so that neighbouring cells start in other banks
  constexpr int S = ((CMAX + 3) / 4 * 4) + ((CMAX + 3) / 4 % 2 ? 0 : 4);
  __shared__ __attribute__((aligned(16))) float lo[kEtCap];      // [fy][fx][S]
  __shared__ unsigned hist[kEtMaxC * kEtMaxC];  // [target][label]
  __shared__ int sbox[kEtMaxBox * 4];
  const int tid = threadIdx.x, ty = tid / kEtTW, tx = tid % kEtTW;
  for (int i = tid; i < C * C; i += 256) hist[i] = 0u;
  for (int i = tid; i < nbox * 4; i += 256) sbox[i] = boxes.v[i];
  __syncthreads();
  const int tiles_x = (W + kEtTW - 1) / kEtTW, tiles_y = (H + kEtTH - 1) / kEtTH;
  const int ntiles = B * tiles_y * tiles_x;
  const long plane = (long)h * w;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / (tiles_y * tiles_x), r = tile - b * tiles_y * tiles_x;
    const int Y0 = (r / tiles_x) * kEtTH, X0 = (r % tiles_x) * kEtTW;
    const int y = Y0 + ty, x = X0 + tx;
    const bool live = y < H && x < W;
    float acc[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) acc[c] = 0.f;
    int cnt = 0;
    for (int k = 0; k < nbox; ++k) {
      const int y1 = sbox[4 * k], y2 = sbox[4 * k + 1], x1 = sbox[4 * k + 2], x2 = sbox[4 * k + 3];
      // the tile's pixels inside this box (the same for every lane)
      const int ya = max(Y0, y1), yb = min(min(Y0 + kEtTH, y2), H) - 1;
      const int xa = max(X0, x1), xb = min(min(X0 + kEtTW, x2), W) - 1;
      if (ya > yb || xa > xb) continue;
      int fy0, fy1, fx0, fx1, t0, t1;
      float l;
      up_src(ya - y1, sy, h, fy0, t1, l);
      up_src(yb - y1, sy, h, t0, fy1, l);
      up_src(xa - x1, sx, w, fx0, t1, l);
      up_src(xb - x1, sx, w, t0, fx1, l);
      const int nfy = fy1 - fy0 + 1, nfx = fx1 - fx0 + 1, cells = nfy * nfx;
      const bool staged = cells * S <= kEtCap;
      const long base = ((long)k * B + b) * C * plane;             // crop k of image b: row k * B + b
      if (staged) {
        __syncthreads();                                            // the previous footprint has been read
        // lane <-> cell, wave <-> every fourth class: one integer division per cell, rows of the footprint read side by side
        for (int q = tid & 63; q < cells; q += 64) {
          const int fy = q / nfx, fx = q - fy * nfx;
          const long off = base + (long)(fy0 + fy) * w + fx0 + fx;
          for (int c = tid >> 6; c < C; c += 4) lo[q * S + c] = ldf<DT>(crops, off + c * plane);
        }
        __syncthreads();
      }
      if (live && y >= y1 && y < y2 && x >= x1 && x < x2) {
        int a0, a1, b0, b1;
        float ly, lx;
        up_src(y - y1, sy, h, a0, a1, ly);
        up_src(x - x1, sx, w, b0, b1, lx);
        const float hy = 1.f - ly, hx = 1.f - lx;
        ++cnt;
        if (staged) {
          const float* p00 = lo + ((a0 - fy0) * nfx + b0 - fx0) * S;
          const float* p01 = lo + ((a0 - fy0) * nfx + b1 - fx0) * S;
          const float* p10 = lo + ((a1 - fy0) * nfx + b0 - fx0) * S;
          const float* p11 = lo + ((a1 - fy0) * nfx + b1 - fx0) * S;
          // (all CMAX classes, no guard: the loads merge into 16-byte ones; the sums of classes >= C hold whatever the rows'
          // padding held and are never looked at)
#pragma unroll
          for (int c = 0; c < CMAX; ++c) acc[c] += hy * (hx * p00[c] + lx * p01[c]) + ly * (hx * p10[c] + lx * p11[c]);
        } else {
          const long o00 = base + (long)a0 * w + b0, o01 = base + (long)a0 * w + b1;
          const long o10 = base + (long)a1 * w + b0, o11 = base + (long)a1 * w + b1;
#pragma unroll
          for (int c = 0; c < CMAX; ++c) {
            if (c < C) {
              const long pc = c * plane;
              acc[c] += hy * (hx * ldf<DT>(crops, o00 + pc) + lx * ldf<DT>(crops, o01 + pc)) +
                        ly * (hx * ldf<DT>(crops, o10 + pc) + lx * ldf<DT>(crops, o11 + pc));
            }
          }
        }
      }
    }
    if (live) {
      const float n = (float)max(cnt, 1);                           // (cnt >= 1: the host checked the cover)
      if ((cnt & (cnt - 1)) == 0) {                                 // 1, 2, 4, ... boxes: the reciprocal is exact, x / n == x * (1 / n)
        const float rn = 1.f / n;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) acc[c] *= rn;
      } else {
#pragma unroll
        for (int c = 0; c < CMAX; ++c) acc[c] /= n;
      }
      float best = acc[0];
      int label = 0;
#pragma unroll
      for (int c = 1; c < CMAX; ++c) {
        if (c < C && acc[c] > best) {
          best = acc[c];
          label = c;
        }
      }
      const long gi = ((long)b * H + y) * W + x;
      if (labels != nullptr) labels[gi] = (unsigned char)label;
      if (target != nullptr) {
        const long t = target[gi];
        if (t != (long)ignore_index && t >= 0 && t < C) atomicAdd(&hist[(int)t * C + label], 1u);
      }
    }
  }
  if (confmat != nullptr) {
    __syncthreads();
    for (int i = tid; i < C * C; i += 256) {
      const unsigned v = hist[i];
      if (v != 0u) atomicAdd(confmat + i, (unsigned long long)v);
    }
  }
}

// The same with a second resize: labels, target and counts on a (B, Ho, Wo) grid, the value at an output pixel the bilinear sample
// (align_corners = False, scale H / Ho, W / Wo, clamped: the second stage may shrink) of m on the H x W image grid -- what
// forward(x, out_size) computes.  A workgroup owns 16 x 16 tiles of OUTPUT pixels and works in two phases through `mid` in LDS
// (m per image pixel, classes innermost, rows padded as in `lo`):
//   * the tile's footprint on the image grid fits `mid` (any up-scaling from x 4/3): ONE pass -- lane p computes m at the p-th
//     pixel of the footprint, then every lane blends the rows of its four taps;
//   * it does not fit (the second stage shrinks the map, or keeps it): kEtTH * kEtTW / G passes over G output pixels each -- lane p
//     computes m at tap p % 4 of output pixel p / 4 of the pass, then the G lanes of the pass blend their four rows.
// Both phases are one piece of code; m is et_mean's, the other kernel's arithmetic restated, rounded to fp32 where that has it.  The blend is spelled with fmaf
// (one rounding order, whatever the compiler would contract); at Ho == H, Wo == W its weights are exactly 1 and 0: it returns m.
template <int DT, int CMAX>
__global__ __launch_bounds__(256, 3) void slide_argmax_confmat_resized_kernel(
    const void* __restrict__ crops, EtBoxes boxes, int nbox, int B, int C, int h, int w, int H, int W, float sy, float sx, int Ho,
    int Wo, float ry, float rx, const long* __restrict__ target, int ignore_index, unsigned char* __restrict__ labels,
    unsigned long long* __restrict__ confmat) {
  constexpr int S = et_row<CMAX>();
  constexpr int G = CMAX <= 19 ? 32 : 16;                        // output pixels per pass where the footprint does not fit
  static_assert(kEtMidCap / S <= 256 && 4 * G * S <= kEtMidCap && G % kEtTW == 0, "one lane per row of `mid`");
  const int tid = threadIdx.x, ty = tid / kEtTW, tx = tid % kEtTW;
  for (int i = tid; i < C * C; i += 256) et_hist[i] = 0u;
  for (int i = tid; i < nbox * 4; i += 256) et_sbox[i] = boxes.v[i];
  __syncthreads();
  const int tiles_x = (Wo + kEtTW - 1) / kEtTW, tiles_y = (Ho + kEtTH - 1) / kEtTH;
  const int ntiles = B * tiles_y * tiles_x;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / (tiles_y * tiles_x), r = tile - b * tiles_y * tiles_x;
    const int Y0 = (r / tiles_x) * kEtTH, X0 = (r % tiles_x) * kEtTW;
    const int y = Y0 + ty, x = X0 + tx;
    const bool live = y < Ho && x < Wo;
    // the tile's footprint on the image grid: up_src does not decrease with the output index, so the first pixel's i0 and the
    // last pixel's i1 bound the taps of every pixel between them (a pixel past the border is given the last one's)
    int iy0, iy1, ix0, ix1, t;
    float l;
    up_src(Y0, ry, H, iy0, t, l);
    up_src(min(Y0 + kEtTH, Ho) - 1, ry, H, t, iy1, l);
    up_src(X0, rx, W, ix0, t, l);
    up_src(min(X0 + kEtTW, Wo) - 1, rx, W, t, ix1, l);
    const int nix = ix1 - ix0 + 1, npx = (iy1 - iy0 + 1) * nix;
    const bool fits = npx * S <= kEtMidCap;
    const int passes = fits ? 1 : kEtTH * kEtTW / G;
    for (int j = 0; j < passes; ++j) {
      // phase one: this lane's image pixel, and the rows of the image that the pass touches
      bool on;
      int py, px, ra = iy0, rb = iy1;
      if (fits) {
        on = tid < npx;
        py = on ? tid / nix : 0;
        px = ix0 + (on ? tid - py * nix : 0);
        py += iy0;
      } else {
        on = tid < 4 * G;
        const int o = j * G + (on ? tid >> 2 : 0);                // the output pixel, as a lane of the tile
        int a0, a1, b0, b1;
        up_src(min(Y0 + o / kEtTW, Ho - 1), ry, H, a0, a1, l);
        up_src(min(X0 + o % kEtTW, Wo - 1), rx, W, b0, b1, l);
        py = tid & 2 ? a1 : a0;
        px = tid & 1 ? b1 : b0;
        up_src(min(Y0 + j * G / kEtTW, Ho - 1), ry, H, ra, t, l);
        up_src(min(Y0 + (j * G + G - 1) / kEtTW, Ho - 1), ry, H, t, rb, l);
      }
      float m[CMAX];
      const int cnt = et_mean<DT, CMAX>(crops, nbox, B, C, h, w, H, W, sy, sx, b, ra, rb + 1, ix0, ix1 + 1, py, px, on, m);
      __syncthreads();                                            // the previous blend has read `mid`
      if (on) {
        et_divide<CMAX>(m, cnt);
#pragma unroll
        for (int c = 0; c < CMAX; ++c) et_mid[tid * S + c] = m[c];
      }
      __syncthreads();
      // phase two: the output pixels of this pass
      if (live && (fits || tid / G == j)) {
        int a0, a1, b0, b1;
        float ly, lx;
        up_src(y, ry, H, a0, a1, ly);
        up_src(x, rx, W, b0, b1, lx);
        const float hy = 1.f - ly, hx = 1.f - lx;
        const float* p00 = et_mid + (fits ? (a0 - iy0) * nix + b0 - ix0 : 4 * (tid - j * G)) * S;
        const float* p01 = fits ? et_mid + ((a0 - iy0) * nix + b1 - ix0) * S : p00 + S;
        const float* p10 = fits ? et_mid + ((a1 - iy0) * nix + b0 - ix0) * S : p00 + 2 * S;
        const float* p11 = fits ? et_mid + ((a1 - iy0) * nix + b1 - ix0) * S : p00 + 3 * S;
        float out[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
          out[c] = fmaf(hy, fmaf(lx, p01[c], hx * p00[c]), ly * fmaf(lx, p11[c], hx * p10[c]));
        et_label<CMAX>(out, C, ((long)b * Ho + y) * Wo + x, target, ignore_index, labels);
      }
    }
  }
  et_flush(C, confmat);
}

// every pixel of the H x W image lies in some box: on the grid of the boxes' own edges a cell is either inside or outside
// each box, so one probe per cell decides
static bool et_covered(const int* boxes, int nbox, int H, int W) {
  int ys[2 * kEtMaxBox + 2], xs[2 * kEtMaxBox + 2], ny = 0, nx = 0;
  ys[ny++] = 0;
  xs[nx++] = 0;
  for (int k = 0; k < nbox; ++k) {
    ys[ny++] = boxes[4 * k], ys[ny++] = boxes[4 * k + 1];
    xs[nx++] = boxes[4 * k + 2], xs[nx++] = boxes[4 * k + 3];
  }
  for (int i = 0; i < ny; ++i) {
    const int y = ys[i];
    if (y >= H) continue;
    for (int j = 0; j < nx; ++j) {
      const int x = xs[j];
      if (x >= W) continue;
      bool in = false;
      for (int k = 0; k < nbox && !in; ++k)
        in = y >= boxes[4 * k] && y < boxes[4 * k + 1] && x >= boxes[4 * k + 2] && x < boxes[4 * k + 3];
      if (!in) return false;
    }
  }
  return true;
}

// Both entry points: the checks, then one launch.  `resized`: labels, target and counts on the (B, Ho, Wo) grid.
static int et_run(const char* who, bool resized, const void* crop_logits, int dtype, int B, int C, int h, int w, const int* boxes,
                  int nbox, int H, int W, int Ho, int Wo, const long* target, int ignore_index, unsigned char* labels,
                  long* confmat, rfn_stream_t stream) {
  RFN_REQUIRE(crop_logits && boxes, "%s: null pointer", who);
  RFN_REQUIRE(labels || confmat, "%s: labels and confmat are both NULL: nothing to compute", who);
  RFN_REQUIRE(!confmat || target, "%s: confmat needs a target", who);
  RFN_REQUIRE(B > 0 && C > 0 && C <= kEtMaxC && h > 0 && w > 0 && H > 0 && W > 0, "%s: B=%d C=%d (<= %d) h=%d w=%d H=%d W=%d", who,
              B, C, kEtMaxC, h, w, H, W);
  RFN_REQUIRE(nbox > 0 && nbox <= kEtMaxBox, "%s: %d boxes (1 ... %d)", who, nbox, kEtMaxBox);
  RFN_REQUIRE((long)B * H * W < (1L << 31), "%s: B * H * W >= 2^31 (32-bit counts per workgroup)", who);
  if (resized) {
    RFN_REQUIRE(Ho > 0 && Wo > 0, "%s: Ho=%d Wo=%d", who, Ho, Wo);
    RFN_REQUIRE((long)B * Ho * Wo < (1L << 31), "%s: B * Ho * Wo >= 2^31 (32-bit counts per workgroup)", who);
  }
  EtBoxes bx;
  const int bh = boxes[1] - boxes[0], bw = boxes[3] - boxes[2];
  for (int k = 0; k < nbox; ++k) {
    const int y1 = boxes[4 * k], y2 = boxes[4 * k + 1], x1 = boxes[4 * k + 2], x2 = boxes[4 * k + 3];
    RFN_REQUIRE(y1 >= 0 && y1 < y2 && y2 <= H && x1 >= 0 && x1 < x2 && x2 <= W,
                "%s: box %d = (%d, %d, %d, %d) is not inside the %d x %d image", who, k, y1, y2, x1, x2, H, W);
    RFN_REQUIRE(y2 - y1 == bh && x2 - x1 == bw,
                "%s: box %d is %d x %d, box 0 is %d x %d (the crops share one %d x %d logit size)", who, k, y2 - y1, x2 - x1, bh,
                bw, h, w);
    bx.v[4 * k] = y1, bx.v[4 * k + 1] = y2, bx.v[4 * k + 2] = x1, bx.v[4 * k + 3] = x2;
  }
  RFN_REQUIRE(et_covered(boxes, nbox, H, W), "%s: the %d boxes leave pixels of the %d x %d image uncovered", who, nbox, H, W);
  const float sy = (float)h / (float)bh, sx = (float)w / (float)bw;      // ATen: area_pixel_compute_scale with size=
  const long ntiles = (long)B * cdiv(resized ? Ho : H, kEtTH) * cdiv(resized ? Wo : W, kEtTW);
  const dim3 grid((unsigned)(ntiles < kEtMaxGrid ? ntiles : kEtMaxGrid));
  hipStream_t s = (hipStream_t)stream;
  return dt_one(dtype, who, [&](auto t) {
    constexpr int D = code_of<typename decltype(t)::type>;
    if (resized) {
      const float ry = (float)H / (float)Ho, rx = (float)W / (float)Wo;
      const auto kernel = C <= 19 ? slide_argmax_confmat_resized_kernel<D, 19> : slide_argmax_confmat_resized_kernel<D, kEtMaxC>;
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, crop_logits, bx, nbox, B, C, h, w, H, W, sy, sx, Ho, Wo, ry, rx, target,
                         ignore_index, labels, (unsigned long long*)confmat);
    } else {
      const auto kernel = C <= 19 ? slide_argmax_confmat_kernel<D, 19> : slide_argmax_confmat_kernel<D, kEtMaxC>;
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, crop_logits, bx, nbox, B, C, h, w, H, W, sy, sx, target, ignore_index,
                         labels, (unsigned long long*)confmat);
    }
    return check_launch(who);
  });
}

}  // namespace rfn

extern "C" {
using namespace rfn;

// see include/refign_hip.h
int rfn_slide_argmax_confmat(const void* crop_logits, int dtype, int B, int C, int h, int w, const int* boxes, int nbox, int H,
                             int W, const long* target, int ignore_index, unsigned char* labels, long* confmat,
                             rfn_stream_t stream) {
  return et_run("rfn_slide_argmax_confmat", false, crop_logits, dtype, B, C, h, w, boxes, nbox, H, W, H, W, target, ignore_index,
                labels, confmat, stream);
}

int rfn_slide_argmax_confmat_resized(const void* crop_logits, int dtype, int B, int C, int h, int w, const int* boxes, int nbox,
                                     int H, int W, int Ho, int Wo, const long* target, int ignore_index, unsigned char* labels,
                                     long* confmat, rfn_stream_t stream) {
  return et_run("rfn_slide_argmax_confmat_resized", true, crop_logits, dtype, B, C, h, w, boxes, nbox, H, W, Ho, Wo, target,
                ignore_index, labels, confmat, stream);
}

}  // extern "C"
