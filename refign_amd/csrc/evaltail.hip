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
#include "bilinear.h"
#include "common.h"
#include "elem.h"

namespace rfn {

constexpr int kEtTH = 16, kEtTW = 16;          // image pixels per tile (one per lane of a 256-lane workgroup)
constexpr int kEtMaxC = 32, kEtMaxBox = 64;
constexpr int kEtCap = 4608;                   // fp32 values of staged footprint (18 KB): 230 cells of 19 (padded to 20) classes
constexpr int kEtMaxGrid = 1024;               // ~4 workgroups per CU: the flush is <= 1024 x C x C atomics

struct EtBoxes {
  int v[kEtMaxBox * 4];                        // (y1, y2, x1, x2) per box; travels in the kernel arguments
};

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

}  // namespace rfn

extern "C" {
using namespace rfn;

// see include/refign_hip.h
int rfn_slide_argmax_confmat(const void* crop_logits, int dtype, int B, int C, int h, int w, const int* boxes, int nbox, int H,
                             int W, const long* target, int ignore_index, unsigned char* labels, long* confmat,
                             rfn_stream_t stream) {
  RFN_REQUIRE(crop_logits && boxes, "slide_argmax_confmat: null pointer");
  RFN_REQUIRE(labels || confmat, "slide_argmax_confmat: labels and confmat are both NULL: nothing to compute");
  RFN_REQUIRE(!confmat || target, "slide_argmax_confmat: confmat needs a target");
  RFN_REQUIRE(B > 0 && C > 0 && C <= kEtMaxC && h > 0 && w > 0 && H > 0 && W > 0,
              "slide_argmax_confmat: B=%d C=%d (<= %d) h=%d w=%d H=%d W=%d", B, C, kEtMaxC, h, w, H, W);
  RFN_REQUIRE(nbox > 0 && nbox <= kEtMaxBox, "slide_argmax_confmat: %d boxes (1 ... %d)", nbox, kEtMaxBox);
  RFN_REQUIRE((long)B * H * W < (1L << 31), "slide_argmax_confmat: B * H * W >= 2^31 (32-bit counts per workgroup)");
  EtBoxes bx;
  const int bh = boxes[1] - boxes[0], bw = boxes[3] - boxes[2];
  for (int k = 0; k < nbox; ++k) {
    const int y1 = boxes[4 * k], y2 = boxes[4 * k + 1], x1 = boxes[4 * k + 2], x2 = boxes[4 * k + 3];
    RFN_REQUIRE(y1 >= 0 && y1 < y2 && y2 <= H && x1 >= 0 && x1 < x2 && x2 <= W,
                "slide_argmax_confmat: box %d = (%d, %d, %d, %d) is not inside the %d x %d image", k, y1, y2, x1, x2, H, W);
    RFN_REQUIRE(y2 - y1 == bh && x2 - x1 == bw,
                "slide_argmax_confmat: box %d is %d x %d, box 0 is %d x %d (the crops share one %d x %d logit size)", k,
                y2 - y1, x2 - x1, bh, bw, h, w);
    bx.v[4 * k] = y1, bx.v[4 * k + 1] = y2, bx.v[4 * k + 2] = x1, bx.v[4 * k + 3] = x2;
  }
  RFN_REQUIRE(et_covered(boxes, nbox, H, W), "slide_argmax_confmat: the %d boxes leave pixels of the %d x %d image uncovered",
              nbox, H, W);
  const float sy = (float)h / (float)bh, sx = (float)w / (float)bw;      // ATen: area_pixel_compute_scale with size=
  const long ntiles = (long)B * cdiv(H, kEtTH) * cdiv(W, kEtTW);
  const dim3 grid((unsigned)(ntiles < kEtMaxGrid ? ntiles : kEtMaxGrid));
  hipStream_t s = (hipStream_t)stream;
  return dt_one(dtype, "rfn_slide_argmax_confmat", [&](auto t) {
    constexpr int D = code_of<typename decltype(t)::type>;
    const auto kernel = C <= 19 ? slide_argmax_confmat_kernel<D, 19> : slide_argmax_confmat_kernel<D, kEtMaxC>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, crop_logits, bx, nbox, B, C, h, w, H, W, sy, sx, target, ignore_index, labels,
                       (unsigned long long*)confmat);
    return check_launch("slide_argmax_confmat");
  });
}

}  // extern "C"
