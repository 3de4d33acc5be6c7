// refign_amd/csrc/loss.hip -- the segmentation loss of the student passes in one kernel: bilinear up-sampling of the class
// logits to the label resolution, pixel-weighted cross-entropy, and the gradient with respect to the LOW-resolution logits.
//
// Reference: models/segmentation_model.py:163-179 / :226-250 (source and mixed pass): `F.interpolate(logits, size,
// mode='bilinear', align_corners=False)` followed by models/losses.py:10-22 PixelWeightedCrossEntropyLoss =
// mean over ALL pixels of weight * CE(ignore_index).  Unfused, the (B, 19, 1080, 1920) tensor (158 MB in fp32) is written
// by the up-sampling, read and written by log_softmax, read by nll_loss, and the same again backwards -- 1.3 ms per
// student pass in six ATen kernels, between the forward and the backward of the pass (round 3, tools/aten_census.py).
// Here a workgroup owns a 16 x 16 tile of label pixels (32 KB of LDS: 4-5 workgroups per CU):
//   1. the low-resolution logits under the tile (its bilinear footprint, <= 10 x 10 cells x C) go to LDS;
//   2. every pixel interpolates its C logits (ATen's formula and operand order, optionally rounded to the 16-bit dtype
//      the unfused path would have stored), takes the log-sum-exp, adds weight * (lse - z[target]) to the loss and leaves
//      weight * (softmax - onehot) -- its gradient with respect to the up-sampled logits -- in LDS;
//   3. the transpose of the interpolation, separably: along x into (C, 16 rows, footprint columns), then along y, and the
//      footprint cells are ADDED to the low-resolution gradient (fp32 atomics: neighbouring tiles share their border
//      cells).
// Results are the SUMS (loss: one double; gradient: unscaled); the host divides by the pixel count and multiplies by the
// upstream gradient.  Scale factors >= 2 in both directions (the footprint bound above); anything else stays on ATen.
#include <hip/hip_bf16.h>

#include "bilinear.h"
#include "common.h"
#include "elem.h"

namespace rfn {

constexpr int kLossTH = 16, kLossTW = 16, kLossPX = kLossTH * kLossTW;     // label pixels per workgroup (one per thread)
constexpr int kLossFY = kLossTH / 2 + 2, kLossFX = kLossTW / 2 + 2;         // footprint bound at scale 2
constexpr int kLossSlots = 64;                                              // partial loss sums
constexpr int kLossMaxC = 19;                                               // classes (Cityscapes); LDS is sized for it

// FULLC: C == kLossMaxC, no per-class guards (with a run-time class count every class of every loop is a branch)
template <int DT, bool FULLC>
__global__ __launch_bounds__(256) void upsample_ce_kernel(const void* __restrict__ logits, const long* __restrict__ target,
                                                          const float* __restrict__ weight, float* __restrict__ grad_lo,
                                                          double* __restrict__ loss_sum, int C, int h, int w, int H, int W,
                                                          float sy, float sx, int ignore_index, int round16,
                                                          float* __restrict__ tile_part = nullptr,
                                                          double* __restrict__ loss_part = nullptr) {
  // the footprint logits (steps 1-2) and the x-reduced gradient (step 3) share their LDS
  __shared__ float tmp[kLossMaxC * kLossTH * kLossFX];         // [c][ty][fx]
  float* const lo = tmp;                                       // [c][fy][fx], dead before step 3a writes tmp
  __shared__ float pr[kLossMaxC * kLossPX];                    // [c][ty * 32 + tx]: gradient w.r.t. the up-sampled logits
  __shared__ int ry0[kLossTH], ry1[kLossTH], cx0[kLossTW], cx1[kLossTW];
  __shared__ float rl[kLossTH], cl[kLossTW];
  __shared__ float red[4];
  __shared__ int txlo[kLossFX], txhi[kLossFX], tylo[kLossFY], tyhi[kLossFY];
  const int tid = threadIdx.x, b = blockIdx.z;
  const int Y0 = blockIdx.y * kLossTH, X0 = blockIdx.x * kLossTW;
  const int YN = min(kLossTH, H - Y0), XN = min(kLossTW, W - X0);       // live rows / columns of the tile
  if (tid < kLossTH) {
    int i0, i1;
    float l;
    up_src(min(Y0 + tid, H - 1), sy, h, i0, i1, l);
    ry0[tid] = i0;
    ry1[tid] = i1;
    rl[tid] = l;
  } else if (tid >= 64 && tid < 64 + kLossTW) {
    const int t = tid - 64;
    int i0, i1;
    float l;
    up_src(min(X0 + t, W - 1), sx, w, i0, i1, l);
    cx0[t] = i0;
    cx1[t] = i1;
    cl[t] = l;
  }
  __syncthreads();
  const int fy0 = ry0[0], fx0 = cx0[0];
  const int nfy = ry1[YN - 1] - fy0 + 1, nfx = cx1[XN - 1] - fx0 + 1;   // <= kLossFY, kLossFX for scales >= 2 (host checks)
  const long plane = (long)h * w;
  const char* lg = (const char*)logits;
  for (int i = tid; i < C * nfy * nfx; i += 256) {
    const int c = i / (nfy * nfx), r = i - c * nfy * nfx, fy = r / nfx, fx = r - fy * nfx;
    lo[(c * kLossFY + fy) * kLossFX + fx] = ldf<DT>(lg, ((long)b * C + c) * plane + (long)(fy0 + fy) * w + fx0 + fx);
  }
  __syncthreads();
  // ---- 2. per pixel
  float lsum = 0.f;
#pragma unroll
  for (int k = 0; k < kLossPX / 256; ++k) {
    const int px = tid + 256 * k, ty = px / kLossTW, tx = px % kLossTW;
    const bool live = ty < YN && tx < XN;
    float z[kLossMaxC];
    float m = -3.0e38f;
    const int a0 = (ry0[ty] - fy0) * kLossFX, a1 = (ry1[ty] - fy0) * kLossFX, b0 = cx0[tx] - fx0, b1 = cx1[tx] - fx0;
    const float ly = rl[ty], hy = 1.f - ly, lx = cl[tx], hx = 1.f - lx;
#pragma unroll
    for (int c = 0; c < kLossMaxC; ++c) {
      if (FULLC || c < C) {
        const float* p = lo + c * kLossFY * kLossFX;
        float v = hy * (hx * p[a0 + b0] + lx * p[a0 + b1]) + ly * (hx * p[a1 + b0] + lx * p[a1 + b1]);
        if (round16) v = round_to<DT>(v);
        z[c] = v;
        m = fmaxf(m, v);
      }
    }
    long t = ignore_index;
    float wt = 0.f;
    if (live) {
      const long gi = ((long)b * H + Y0 + ty) * W + X0 + tx;
      t = target[gi];
      wt = weight != nullptr ? weight[gi] : 1.f;
    }
    const bool valid = live && t != ignore_index && t >= 0 && t < C;
    float S = 0.f, zt = 0.f;
#pragma unroll
    for (int c = 0; c < kLossMaxC; ++c) {
      if (FULLC || c < C) {
        if (valid && c == (int)t) zt = z[c];
        z[c] = __expf(z[c] - m);
        S += z[c];
      }
    }
    const float inv = valid ? wt / S : 0.f;
#pragma unroll
    for (int c = 0; c < kLossMaxC; ++c) {
      if (FULLC || c < C) pr[c * kLossPX + px] = z[c] * inv - ((valid && c == (int)t) ? wt : 0.f);
    }
    if (valid) lsum += wt * (m + __logf(S) - zt);                  // weight * (lse - z[target])
  }
  lsum = wave_sum(lsum);
  if ((tid & 63) == 0) red[tid >> 6] = lsum;
  __syncthreads();
  // kLossSlots partial sums (the host adds them): 8 160 tiles adding to ONE address were serialised in the L2 -- 435 us of
  // same-address atomics around 70 us of work
  // tile_part / loss_part (deterministic form): this tile's loss and footprint gradient go to slots of their own with plain
  // stores; upsample_ce_gather_kernel / ordered_colsum add them in tile order
  const long tile_id = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  if (tid == 0) {
    const double v = (double)((red[0] + red[1]) + (red[2] + red[3]));
    if (loss_part != nullptr) loss_part[tile_id] = v;
    else atomicAdd(loss_sum + (blockIdx.x + 7 * blockIdx.y + 13 * blockIdx.z) % kLossSlots, v);
  }
  // the tile columns / rows whose footprint contains a cell are a contiguous run (the source index is monotone): its ends,
  // so that the sums below walk ~2 x scale pixels instead of the whole tile edge
  if (tid < nfx) {
    const int cell = fx0 + tid;
    int lo_ = XN, hi_ = -1;
    for (int tx = 0; tx < XN; ++tx)
      if (cx0[tx] == cell || cx1[tx] == cell) { lo_ = min(lo_, tx); hi_ = tx; }
    txlo[tid] = lo_;
    txhi[tid] = hi_;
  } else if (tid >= 64 && tid < 64 + nfy) {
    const int f = tid - 64, cell = fy0 + f;
    int lo_ = YN, hi_ = -1;
    for (int ty = 0; ty < YN; ++ty)
      if (ry0[ty] == cell || ry1[ty] == cell) { lo_ = min(lo_, ty); hi_ = ty; }
    tylo[f] = lo_;
    tyhi[f] = hi_;
  }
  __syncthreads();
  // ---- 3a. transpose of the interpolation along x: tmp[c][ty][fx] = sum_tx wx(tx, fx) pr[c][ty][tx]
  for (int i = tid; i < C * kLossTH * nfx; i += 256) {
    const int c = i / (kLossTH * nfx), r = i - c * kLossTH * nfx, ty = r / nfx, fx = r - ty * nfx;
    float acc = 0.f;
    if (ty < YN) {
      const float* p = pr + c * kLossPX + ty * kLossTW;
      const int cell = fx0 + fx;
      for (int tx = txlo[fx]; tx <= txhi[fx]; ++tx) {
        const float l = cl[tx];
        const float wgt = (cx0[tx] == cell ? 1.f - l : 0.f) + (cx1[tx] == cell ? l : 0.f);
        acc = fmaf(wgt, p[tx], acc);
      }
    }
    tmp[(c * kLossTH + ty) * kLossFX + fx] = acc;
  }
  __syncthreads();
  // ---- 3b. along y, and out
  for (int i = tid; i < C * nfy * nfx; i += 256) {
    const int c = i / (nfy * nfx), r = i - c * nfy * nfx, fy = r / nfx, fx = r - fy * nfx;
    const int cell = fy0 + fy;
    float acc = 0.f;
    for (int ty = tylo[fy]; ty <= tyhi[fy]; ++ty) {
      const float l = rl[ty];
      const float wgt = (ry0[ty] == cell ? 1.f - l : 0.f) + (ry1[ty] == cell ? l : 0.f);
      acc = fmaf(wgt, tmp[(c * kLossTH + ty) * kLossFX + fx], acc);
    }
    if (tile_part != nullptr) tile_part[((tile_id * C + c) * kLossFY + fy) * kLossFX + fx] = acc;
    else if (acc != 0.f) atomicAdd(grad_lo + ((long)b * C + c) * plane + (long)cell * w + fx0 + fx, acc);
  }
}

// Deterministic form, second launch: grad_lo[b][c][y][x] = sum, over the tiles whose footprint holds the cell (tile rows outer,
// tile columns inner, ascending), of that tile's partial.  One thread per low-resolution cell.
__global__ __launch_bounds__(256) void upsample_ce_gather_kernel(const float* __restrict__ tile_part, float* __restrict__ grad_lo,
                                                                 long total, int C, int h, int w, int H, int W, float sy, float sx,
                                                                 int tiles_x, int tiles_y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w), y = (int)((i / w) % h), c = (int)((i / ((long)w * h)) % C), b = (int)(i / ((long)w * h * C));
  int Ylo, Yhi, Xlo, Xhi;
  up_cell_window(y, sy, H, Ylo, Yhi);
  up_cell_window(x, sx, W, Xlo, Xhi);
  float acc = 0.f;
  for (int TY = Ylo / kLossTH; TY <= (Yhi - 1) / kLossTH; ++TY) {
    const int Y0 = TY * kLossTH, YN = min(kLossTH, H - Y0);
    int f0, f1, t0, t1;
    float l;
    up_src(Y0, sy, h, f0, t1, l);
    up_src(Y0 + YN - 1, sy, h, t0, f1, l);
    if (y < f0 || y > f1) continue;
    for (int TX = Xlo / kLossTW; TX <= (Xhi - 1) / kLossTW; ++TX) {
      const int X0 = TX * kLossTW, XN = min(kLossTW, W - X0);
      int g0, g1;
      up_src(X0, sx, w, g0, t1, l);
      up_src(X0 + XN - 1, sx, w, t0, g1, l);
      if (x < g0 || x > g1) continue;
      const long tile = ((long)b * tiles_y + TY) * tiles_x + TX;
      acc += tile_part[((tile * C + c) * kLossFY + (y - f0)) * kLossFX + (x - g0)];
    }
  }
  grad_lo[i] = acc;
}

static inline unsigned long ce_loss_part_bytes(long tiles) { return ((unsigned long)tiles * sizeof(double) + 15) & ~15ul; }

}  // namespace rfn

extern "C" {
using namespace rfn;

// loss_sum[0..63] <- 64 partial sums (their sum is the result) over all (b, y, x) of weight * CE(bilinear(logits)[b, :, y, x], target), grad_lo (B, C, h, w) fp32 <- the
// gradient of that sum with respect to the low-resolution logits; both are zeroed here.  logits: (B, C, h, w) contiguous,
// dtype 0 fp32 / 1 bf16 / 2 f16; target: (B, H, W) int64; weight: (B, H, W) fp32 or NULL.  round16: round the interpolated
// logits to `dtype` first (what an unfused 16-bit up-sampling stores).
static int upsample_ce_impl(void* workspace, const void* logits, const long* target, const float* weight, float* grad_lo,
                           double* loss_sum, int B, int C, int h, int w, int H, int W, int ignore_index, int dtype, int round16,
                           rfn_stream_t stream) {
  RFN_REQUIRE(logits && target && grad_lo && loss_sum, "upsample_ce: null pointer");
  RFN_REQUIRE(B > 0 && C > 0 && C <= kLossMaxC && h > 0 && w > 0, "upsample_ce: B=%d C=%d (<= %d) h=%d w=%d", B, C, kLossMaxC, h, w);
  RFN_REQUIRE(H >= 2 * h && W >= 2 * w, "upsample_ce: %dx%d -> %dx%d (scale factors >= 2 only)", h, w, H, W);
  const bool det = workspace != nullptr;
  return dt_one(dtype, det ? "rfn_upsample_ce_det" : "rfn_upsample_ce", [&](auto t) {
    constexpr int D = code_of<typename decltype(t)::type>;
    hipStream_t s = (hipStream_t)stream;
    if (!det)
      if (int rc = zero_async(grad_lo, (size_t)B * C * h * w * sizeof(float), s)) return rc;
    if (int rc = zero_async(loss_sum, kLossSlots * sizeof(double), s)) return rc;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;      // ATen: area_pixel_compute_scale with size=
    dim3 grid(cdiv(W, kLossTW), cdiv(H, kLossTH), B);
    // deterministic form: workspace = [tiles doubles: loss][tiles x C x kLossFY x kLossFX floats: footprint gradients]
    const long tiles = (long)grid.x * grid.y * grid.z;
    double* loss_part = det ? (double*)workspace : nullptr;
    float* tile_part = det ? (float*)((char*)workspace + ce_loss_part_bytes(tiles)) : nullptr;
    const auto kernel = C == kLossMaxC ? upsample_ce_kernel<D, true> : upsample_ce_kernel<D, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, logits, target, weight, grad_lo, loss_sum, C, h, w, H, W, sy, sx, ignore_index,
                       round16 && D != 0, tile_part, loss_part);
    if (int rc = check_launch("upsample_ce")) return rc;
    if (!det) return (int)RFN_OK;
    const long total = (long)B * C * h * w;
    hipLaunchKernelGGL(upsample_ce_gather_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, (const float*)tile_part, grad_lo, total, C,
                       h, w, H, W, sy, sx, (int)grid.x, (int)grid.y);
    if (int rc = check_launch("upsample_ce_gather_kernel")) return rc;
    return ordered_colsum_f64(loss_part, loss_sum, tiles, 1, s);          // slot 0 <- every tile's loss in tile order
  });
}

int rfn_upsample_ce(const void* logits, const long* target, const float* weight, float* grad_lo, double* loss_sum, int B,
                    int C, int h, int w, int H, int W, int ignore_index, int dtype, int round16, rfn_stream_t stream) {
  RFN_REFUSE_NONDET(true, "rfn_upsample_ce", "upsample_ce_kernel, fp32 / fp64 atomics (use rfn_upsample_ce_det)");
  return upsample_ce_impl(nullptr, logits, target, weight, grad_lo, loss_sum, B, C, h, w, H, W, ignore_index, dtype, round16, stream);
}

// Deterministic form of rfn_upsample_ce: every 16 x 16 tile stores its loss and its footprint of the low-resolution gradient
// into `workspace` (rfn_upsample_ce_det_workspace_bytes(B, C, H, W) bytes, no need to zero it); a second launch adds, per
// low-resolution cell, the tiles that touch it in tile order, a third the tiles' losses (loss_sum[0]; slots 1 .. 63 are zero).
unsigned long rfn_upsample_ce_det_workspace_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  const long tiles = (long)cdiv(W, kLossTW) * cdiv(H, kLossTH) * B;
  return ce_loss_part_bytes(tiles) + (unsigned long)tiles * C * kLossFY * kLossFX * sizeof(float);
}

int rfn_upsample_ce_det(const void* logits, const long* target, const float* weight, float* grad_lo, double* loss_sum,
                        void* workspace, int B, int C, int h, int w, int H, int W, int ignore_index, int dtype, int round16,
                        rfn_stream_t stream) {
  RFN_REQUIRE(workspace, "upsample_ce_det: null workspace");
  return upsample_ce_impl(workspace, logits, target, weight, grad_lo, loss_sum, B, C, h, w, H, W, ignore_index, dtype, round16, stream);
}

}  // extern "C"
