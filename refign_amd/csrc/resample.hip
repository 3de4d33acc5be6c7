// refign_amd/csrc/resample.hip -- N4, third part: the LOAD-TIME resize of the reference's data set readers
// (data_modules/datasets/cityscapes.py:119-127: Image.resize(dims[::-1], BILINEAR) for images, NEAREST for labels) and of
// data_modules.transforms.Resize (transforms.py:57-74,120-203) on the device, bit-equal to Pillow, fused into the crop that
// follows it (csrc/datastep.hip).  Pillow's 8-bit bilinear resize is two integer passes over host-built tables
// (refign_amd/resample.py: bilinear_tables): per output pixel a first tap `xmin`, a tap count `n` and n 22-bit fixed-point
// coefficients; a pass is (sum_k in[xmin + k] * coef[k] + 2^21) >> 22 clipped to a byte, horizontal first, and the byte
// rounding BETWEEN the passes is part of the result.
//   resize_kernel<0>  a workgroup owns a 16 x 64 tile of the crop (fewer rows when the vertical scale is large): the horizontal pass of the source rows of the tile's vertical
//                     footprint goes to LDS (one dword per pixel: the three rounded bytes), the vertical pass reads LDS, then
//                     u8 / 255, (x - mean) / std with true divisions as crop_flip_norm_kernel does, coalesced fp32 stores.  Only
//                     the crop's footprint of the source is read.  int32 accumulation: 255 * 2^22 + 2^21 fits.
//   resize_kernel<1>  the same two passes, bytes out: Pillow's pixels as a (3, Hd, Wd) image.
//   resize_nearest_kernel  label map through the two index tables (nearest_table: Pillow ACCUMULATES the source coordinate).
//   resize_nearest_lut_kernel  the same gather with a 256-entry code table on the way (RobotCar's raw ids -> train ids,
//                     datasets/robotcar.py encode_semantic_map): the table is staged in LDS once per workgroup, the output is
//                     written once and no encoded map at the file's size exists.  Hd == H, Wd == W is the encode alone.
// The kernel knows nothing of the filter: Pillow's LANCZOS (sinc(x) sinc(x / 3) on [-3, 3), the matcher's data sets and `test:`
// sections) is the same two passes over longer tables with negative taps (refign_amd/resample.py: filter_tables checks
// 255 * sum |coef| + 2^21 < 2^31 per row, so the int32 accumulation holds), and the clip to a byte between the passes is where its
// overshoot goes.  In the fp32 mode the output may be larger than the crop, (3, Hf, Wf) with Hf >= h, Wf >= w: the pixels outside
// the crop are written 0.0f by the tile that covers them -- transforms.PadBottomRight after Normalize, in the same launch.
// Byte work, no MFMA, no scratch.  Every table entry is clamped to the image before it is used as an index.
#include "common.h"

namespace rfn {

constexpr int kResTH = 16, kResTW = 64;      // output tile of a workgroup (4 waves: a wave per row, a lane per column)
constexpr int kResKmax = 129;                // taps per output pixel the entry points accept: ceil(support * scale) * 2 + 1 with
                                             // support * scale <= 64 (the vertical footprint of a ONE-row tile, 2 * 64 + 3 rows of
                                             // 256 bytes, still fits LDS): scale <= 64 for bilinear, <= 64 / 3 for Lanczos
constexpr size_t kResLds = 64 * 1024;        // LDS a workgroup may ask for without an opt-in
constexpr int kResBits = 22;                 // Pillow's PRECISION_BITS for 8-bit pixels

__device__ __forceinline__ unsigned clip8(int v) { return (unsigned)min(max(v >> kResBits, 0), 255); }

template <int MODE>
__global__ __launch_bounds__(256) void resize_kernel(const unsigned char* __restrict__ img, int H, int W,
                                                     const int2* __restrict__ bx, const int* __restrict__ cx, int kx,
                                                     const int2* __restrict__ by, const int* __restrict__ cy, int ky, int top, int left,
                                                     int h, int w, int Hf, int Wf, int flip, int tile_h, int lds_rows, float m0, float m1,
                                                     float m2, float s0, float s1, float s2, float* __restrict__ out_f,
                                                     unsigned char* __restrict__ out_b) {
  extern __shared__ __attribute__((aligned(16))) unsigned int tile[];   // [lds_rows][kResTW]: byte c of a dword = channel c
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int x0 = blockIdx.x * kResTW, y0 = blockIdx.y * tile_h;
  const int tw = min(kResTW, w - x0), th = min(tile_h, h - y0);       // the tile's part of the crop (<= 0: padding alone)
  const int pw = min(kResTW, Wf - x0), ph = min(tile_h, Hf - y0);     // the tile's part of the output (MODE 1: the same)
  const size_t plane = (size_t)Hf * Wf;
  if (MODE == 0 && (tw <= 0 || th <= 0)) {             // (uniform over the workgroup: nobody waits at the barrier below)
    if (lane < pw)
      for (int y = wave; y < ph; y += 4)
#pragma unroll
        for (int c = 0; c < 3; ++c) out_f[c * plane + (size_t)(y0 + y) * Wf + x0 + lane] = 0.0f;
    return;
  }
  const int rc0 = left + (flip ? w - x0 - tw : x0);   // first RESIZED column of the tile (mirrored or not, the columns are contiguous)
  const int2 bfirst = by[top + y0], blast = by[top + y0 + th - 1];
  const int r0 = bfirst.x;                             // the tables are monotonic: rows [r0, last first tap + its count)
  const int nrows = min(blast.x + blast.y - r0, lds_rows);

  if (lane < tw) {                                     // horizontal pass: lane = resized column rc0 + lane, a wave per source row
    const int2 b = bx[rc0 + lane];
    const int* __restrict__ k = cx + (size_t)(rc0 + lane) * kx;
    const int n = min(b.y, kx);
    for (int r = wave; r < nrows; r += 4) {
      const unsigned char* __restrict__ row = img + (size_t)min(r0 + r, H - 1) * W * 3;
      int a0 = 1 << (kResBits - 1), a1 = a0, a2 = a0;
      for (int t = 0; t < n; ++t) {
        const unsigned char* __restrict__ p = row + (size_t)min(max(b.x + t, 0), W - 1) * 3;
        const int c = k[t];
        a0 += (int)p[0] * c, a1 += (int)p[1] * c, a2 += (int)p[2] * c;
      }
      tile[r * kResTW + lane] = clip8(a0) | (clip8(a1) << 8) | (clip8(a2) << 16);
    }
  }
  __syncthreads();

  if (lane >= pw) return;
  const int x = x0 + lane;
  const int j = flip ? tw - 1 - lane : lane;           // column of the tile that output column x shows
  for (int y = wave; y < ph; y += 4) {                 // vertical pass: (first tap, count, coefficients) are wave-uniform
    const size_t o = (size_t)(y0 + y) * Wf + x;
    if (y >= th || lane >= tw) {                       // right of / below the crop (MODE 0 with Hf > h or Wf > w only)
      if (MODE == 0) out_f[o] = out_f[plane + o] = out_f[2 * plane + o] = 0.0f;
      continue;
    }
    const int ry = top + y0 + y;
    const int2 b = by[ry];
    const int* __restrict__ k = cy + (size_t)ry * ky;
    const int n = min(b.y, ky), rb = b.x - r0;
    int a0 = 1 << (kResBits - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < n; ++t) {
      const unsigned p = tile[min(max(rb + t, 0), lds_rows - 1) * kResTW + j];
      const int c = k[t];
      a0 += (int)(p & 255u) * c, a1 += (int)((p >> 8) & 255u) * c, a2 += (int)((p >> 16) & 255u) * c;
    }
    const unsigned u[3] = {clip8(a0), clip8(a1), clip8(a2)};
    if (MODE == 0) {
      const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
#pragma unroll
      for (int c = 0; c < 3; ++c) out_f[c * plane + o] = ((float)u[c] / 255.0f - mean[c]) / sd[c];
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) out_b[c * plane + o] = (unsigned char)u[c];
    }
  }
}

// grid (ceil(Wd / 256), Hd); one thread per output pixel
__global__ __launch_bounds__(256) void resize_nearest_kernel(const unsigned char* __restrict__ lbl, int H, int W, int Hd, int Wd,
                                                             const int* __restrict__ ytab, const int* __restrict__ xtab,
                                                             unsigned char* __restrict__ out) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= Wd) return;
  const int sy = min(max(ytab[y], 0), H - 1), sx = min(max(xtab[x], 0), W - 1);
  out[(size_t)y * Wd + x] = lbl[(size_t)sy * W + sx];
}

// the same geometry; lut[256] goes to LDS (a byte per thread) before anybody may leave
__global__ __launch_bounds__(256) void resize_nearest_lut_kernel(const unsigned char* __restrict__ lbl, int H, int W, int Hd, int Wd,
                                                                 const int* __restrict__ ytab, const int* __restrict__ xtab,
                                                                 const unsigned char* __restrict__ lut,
                                                                 unsigned char* __restrict__ out) {
  __shared__ unsigned char codes[256];
  codes[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= Wd) return;
  const int sy = min(max(ytab[y], 0), H - 1), sx = min(max(xtab[x], 0), W - 1);
  out[(size_t)y * Wd + x] = codes[lbl[(size_t)sy * W + sx]];
}

// taps per output pixel of Pillow's bilinear filter from `in` to `out` pixels: ceil(max(in / out, 1)) * 2 + 1
static inline int taps(int in, int out) { return (in > out ? cdiv(in, out) : 1) * 2 + 1; }

constexpr int kResBilinear = 0, kResLanczos = 1;     // the `filter` argument of the entry points that take one
static inline double filter_support(int filter) { return filter == kResLanczos ? 3.0 : 1.0; }
// ... of filter `filter`: ceil(support * max(in / out, 1)) * 2 + 1, in double as precompute_coeffs forms it
static inline int taps(int in, int out, int filter) {
  if (filter == kResBilinear) return taps(in, out);
  const double scale = (double)in / out;
  return (int)ceil(filter_support(filter) * (scale > 1.0 ? scale : 1.0)) * 2 + 1;
}

static int launch_resize(int mode, int filter, const char* who, const void* image, int H, int W, int Hd, int Wd, const int* bounds_x,
                         const int* coef_x, int kmax_x, const int* bounds_y, const int* coef_y, int kmax_y, int top, int left, int h,
                         int w, int Hf, int Wf, int flip, const float* m, const float* s, float* out_f, unsigned char* out_b,
                         hipStream_t st) {
  RFN_REQUIRE(image && bounds_x && coef_x && bounds_y && coef_y && (out_f || out_b), "%s: null pointer", who);
  RFN_REQUIRE(H > 0 && W > 0 && Hd > 0 && Wd > 0, "%s: sizes must be positive (%d x %d -> %d x %d)", who, H, W, Hd, Wd);
  RFN_REQUIRE(filter == kResBilinear || filter == kResLanczos, "%s: filter %d (0 = bilinear, 1 = lanczos)", who, filter);
  const int tx = taps(W, Wd, filter), ty = taps(H, Hd, filter);
  const char* fname = filter == kResLanczos ? "lanczos" : "bilinear";
  if (filter == kResBilinear)
    RFN_REQUIRE(tx <= kResKmax && ty <= kResKmax,
                "%s: %d x %d -> %d x %d needs %d x %d taps per pixel, the kernel is built for %d (down-scaling by 64 at the most)", who,
                H, W, Hd, Wd, ty, tx, kResKmax);
  else
    RFN_REQUIRE(tx <= kResKmax && ty <= kResKmax,
                "%s: %d x %d -> %d x %d with the %s filter needs %d x %d taps per pixel, the kernel is built for %d (%s: down-scaling "
                "by 64 / 3 at the most)", who, H, W, Hd, Wd, fname, ty, tx, kResKmax, fname);
  RFN_REQUIRE(kmax_x == tx && kmax_y == ty, "%s: tables of %d x %d taps, %d -> %d and %d -> %d pixels take %d x %d (%s)", who, kmax_y,
              kmax_x, H, Hd, W, Wd, ty, tx, fname);
  RFN_REQUIRE(top >= 0 && left >= 0 && h > 0 && w > 0 && top + h <= Hd && left + w <= Wd && h <= 65535,
              "%s: crop (%d, %d, %d, %d) outside the %d x %d resized image", who, top, left, h, w, Hd, Wd);
  RFN_REQUIRE(Hf >= h && Wf >= w && Hf <= 65535 && (mode == 0 || (Hf == h && Wf == w)),
              "%s: output %d x %d smaller than the %d x %d crop (or larger than 65535 rows)", who, Hf, Wf, h, w);
  // source rows under tile_h output rows: (tile_h - 1) * scale between the first and the last centre, the support on either side;
  // the tile loses rows until they fit (support <= 64: a one-row tile does)
  const double scale = (double)H / Hd, support = filter_support(filter) * (scale > 1.0 ? scale : 1.0);
  int tile_h = kResTH, lds_rows = 0;
  size_t lds = 0;
  for (;; tile_h /= 2) {
    lds_rows = (int)((tile_h - 1) * scale + 2.0 * support) + 3;
    lds = (size_t)lds_rows * kResTW * sizeof(unsigned);
    if (lds <= kResLds || tile_h == 1) break;
  }
  RFN_REQUIRE(lds <= kResLds, "%s: %zu bytes of LDS", who, lds);
  const dim3 grid((unsigned)cdiv(Wf, kResTW), (unsigned)cdiv(Hf, tile_h)), block(256);
  if (mode == 0)
    hipLaunchKernelGGL(resize_kernel<0>, grid, block, lds, st, (const unsigned char*)image, H, W, (const int2*)bounds_x, coef_x, kmax_x,
                       (const int2*)bounds_y, coef_y, kmax_y, top, left, h, w, Hf, Wf, flip, tile_h, lds_rows, m[0], m[1], m[2], s[0], s[1], s[2], out_f,
                       out_b);
  else
    hipLaunchKernelGGL(resize_kernel<1>, grid, block, lds, st, (const unsigned char*)image, H, W, (const int2*)bounds_x, coef_x, kmax_x,
                       (const int2*)bounds_y, coef_y, kmax_y, top, left, h, w, Hf, Wf, flip, tile_h, lds_rows, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f, out_f, out_b);
  return check_launch("resize_kernel");
}

}  // namespace rfn

extern "C" {

int rfn_resize_crop_flip_norm_u8(const void* image_hwc, int H, int W, int Hd, int Wd, const int* bounds_x, const int* coef_x, int kmax_x,
                                 const int* bounds_y, const int* coef_y, int kmax_y, int top, int left, int h, int w, int flip,
                                 const float* mean3, const float* std3, float* out_image, rfn_stream_t stream) {
  using namespace rfn;
  RFN_REQUIRE(mean3 && std3 && out_image, "rfn_resize_crop_flip_norm_u8: null pointer");
  return launch_resize(0, kResBilinear, "rfn_resize_crop_flip_norm_u8", image_hwc, H, W, Hd, Wd, bounds_x, coef_x, kmax_x, bounds_y,
                       coef_y, kmax_y, top, left, h, w, h, w, flip ? 1 : 0, mean3, std3, out_image, nullptr, (hipStream_t)stream);
}

int rfn_resize_filter_crop_flip_norm_pad_u8(const void* image_hwc, int H, int W, int Hd, int Wd, int filter, const int* bounds_x,
                                            const int* coef_x, int kmax_x, const int* bounds_y, const int* coef_y, int kmax_y, int top,
                                            int left, int h, int w, int flip, const float* mean3, const float* std3, float* out_image,
                                            int Hf, int Wf, rfn_stream_t stream) {
  using namespace rfn;
  RFN_REQUIRE(mean3 && std3 && out_image, "rfn_resize_filter_crop_flip_norm_pad_u8: null pointer");
  return launch_resize(0, filter, "rfn_resize_filter_crop_flip_norm_pad_u8", image_hwc, H, W, Hd, Wd, bounds_x, coef_x, kmax_x,
                       bounds_y, coef_y, kmax_y, top, left, h, w, Hf, Wf, flip ? 1 : 0, mean3, std3, out_image, nullptr,
                       (hipStream_t)stream);
}

int rfn_resize_filter_u8(const void* image_hwc, int H, int W, int Hd, int Wd, int filter, const int* bounds_x, const int* coef_x,
                         int kmax_x, const int* bounds_y, const int* coef_y, int kmax_y, void* out_chw, rfn_stream_t stream) {
  using namespace rfn;
  RFN_REQUIRE(out_chw, "rfn_resize_filter_u8: null pointer");
  return launch_resize(1, filter, "rfn_resize_filter_u8", image_hwc, H, W, Hd, Wd, bounds_x, coef_x, kmax_x, bounds_y, coef_y, kmax_y,
                       0, 0, Hd, Wd, Hd, Wd, 0, nullptr, nullptr, nullptr, (unsigned char*)out_chw, (hipStream_t)stream);
}

int rfn_resize_u8(const void* image_hwc, int H, int W, int Hd, int Wd, const int* bounds_x, const int* coef_x, int kmax_x,
                  const int* bounds_y, const int* coef_y, int kmax_y, void* out_chw, rfn_stream_t stream) {
  using namespace rfn;
  RFN_REQUIRE(out_chw, "rfn_resize_u8: null pointer");
  return launch_resize(1, kResBilinear, "rfn_resize_u8", image_hwc, H, W, Hd, Wd, bounds_x, coef_x, kmax_x, bounds_y, coef_y, kmax_y, 0,
                       0, Hd, Wd, Hd, Wd, 0, nullptr, nullptr, nullptr, (unsigned char*)out_chw, (hipStream_t)stream);
}

int rfn_resize_nearest_u8(const void* label, int H, int W, int Hd, int Wd, const int* ytab, const int* xtab, void* out,
                          rfn_stream_t stream) {
  using namespace rfn;
  RFN_REQUIRE(label && ytab && xtab && out, "rfn_resize_nearest_u8: null pointer");
  RFN_REQUIRE(H > 0 && W > 0 && Hd > 0 && Wd > 0 && Hd <= 65535, "rfn_resize_nearest_u8: sizes must be positive, Hd <= 65535 (%d x %d -> %d x %d)",
              H, W, Hd, Wd);
  hipLaunchKernelGGL(resize_nearest_kernel, dim3((unsigned)cdiv(Wd, 256), (unsigned)Hd), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)label, H, W, Hd, Wd, ytab, xtab, (unsigned char*)out);
  return check_launch("resize_nearest_kernel");
}

int rfn_resize_nearest_lut_u8(const void* label, int H, int W, int Hd, int Wd, const int* ytab, const int* xtab, const void* lut,
                              void* out, rfn_stream_t stream) {
  using namespace rfn;
  RFN_REQUIRE(label && ytab && xtab && lut && out, "rfn_resize_nearest_lut_u8: null pointer");
  RFN_REQUIRE(H > 0 && W > 0 && Hd > 0 && Wd > 0 && Hd <= 65535, "rfn_resize_nearest_lut_u8: sizes must be positive, Hd <= 65535 (%d x %d -> %d x %d)",
              H, W, Hd, Wd);
  hipLaunchKernelGGL(resize_nearest_lut_kernel, dim3((unsigned)cdiv(Wd, 256), (unsigned)Hd), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)label, H, W, Hd, Wd, ytab, xtab, (const unsigned char*)lut, (unsigned char*)out);
  return check_launch("resize_nearest_lut_kernel");
}

}  // extern "C"
