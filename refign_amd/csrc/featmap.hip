// refign_amd/csrc/featmap.hip -- whole-map passes over the matcher's feature maps (gfx950): L2 normalisation over the channels
// (NCHW fp32, and channels-last 16-bit -> NCHW fp32), area resize, the 2 x 2 max-pool of the VGG pyramid and the re-tiling copy of
// the uncertainty head.  All HBM-bound, one pass each.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "common.h"
#include "elem.h"

namespace rfn {

// F.normalize(p=2, dim=1) for NCHW.  Generic form: one thread per pixel, channels strided by HW (coalesced across the
// wave), two passes over the channels.
__global__ __launch_bounds__(256) void l2norm_channels_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                              int C, int HW) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const float* p = x + (size_t)blockIdx.y * C * HW + pix;
  float* o = out + (size_t)blockIdx.y * C * HW + pix;
  float ss = 0.0f;
  for (int c = 0; c < C; ++c) {
    const float v = p[(size_t)c * HW];
    ss = fmaf(v, v, ss);
  }
  const float d = fmaxf(sqrtf(ss), 1e-12f);
  for (int c = 0; c < C; ++c) o[(size_t)c * HW] = p[(size_t)c * HW] / d;
}

// The VGG pyramid widths (C = SL * CPT = 128, 256, 512): a workgroup is (256/SL pixels) x (SL channel slices), a thread
// keeps its CPT channels of one pixel in registers -- ONE pass over HBM, CPT independent loads in flight per thread
// (the generic kernel is a serial chain of C dependent-latency loads on 250 workgroups at level 2: 0.95 TB/s).
template <int SL, int CPT>
__global__ __launch_bounds__(256) void l2norm_channels_reg_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                  int HW) {
  constexpr int PX = 256 / SL;
  __shared__ float part[SL][PX];
  const int lane = threadIdx.x % PX, sl = threadIdx.x / PX;
  const int pix = blockIdx.x * PX + lane;
  const bool ok = pix < HW;
  const size_t base = ((size_t)blockIdx.y * SL * CPT + (size_t)sl * CPT) * HW + (ok ? pix : 0);
  float v[CPT];
  float ss = 0.0f;
#pragma unroll
  for (int k = 0; k < CPT; ++k) v[k] = ok ? x[base + (size_t)k * HW] : 0.0f;
#pragma unroll
  for (int k = 0; k < CPT; ++k) ss = fmaf(v[k], v[k], ss);
  part[sl][lane] = ss;
  __syncthreads();
  float tot = 0.0f;
#pragma unroll
  for (int t = 0; t < SL; ++t) tot += part[t][lane];
  const float d = fmaxf(sqrtf(tot), 1e-12f);
  if (ok) {
#pragma unroll
    for (int k = 0; k < CPT; ++k) out[base + (size_t)k * HW] = v[k] / d;
  }
}

// The same from the layout and precision the matcher's convolutions deliver under the reference's AMP recipe:
// channels-last 16-bit features (B, HW, C) -> NCHW fp32, L2-normalised over the channels.  Replaces a cast kernel, a
// strided NHWC -> NCHW copy (1.1 ms for 2 x 128 x 270 x 480: 0.25 TB/s) and the NCHW normalisation with one pass: a
// workgroup stages 32 pixels x C channels as fp32 in LDS (16-byte loads along the channels), eight lanes per pixel
// sum the squares, and the write-out runs along the pixels (32 consecutive floats per channel; LDS pitch C + 1 keeps
// both directions conflict-free).
template <typename T16>
__global__ __launch_bounds__(256) void l2norm_nhwc16_to_nchw_kernel(const uint16_t* __restrict__ x,
                                                                    float* __restrict__ out, int C, int HW) {
  extern __shared__ float tile[];                 // [32][C + 1] + inv[32]
  constexpr int PX = 32;
  const int P = C + 1, tid = threadIdx.x, pix0 = blockIdx.x * PX;
  const int npx = min(PX, HW - pix0);
  float* inv = tile + PX * P;
  const uint16_t* src = x + ((size_t)blockIdx.y * HW + pix0) * C;
  const int nvec = npx * C / 8;                    // C % 8 == 0: the tile is a contiguous run of 16-byte vectors
  for (int v = tid; v < nvec; v += 256) {
    const uint4 raw = *reinterpret_cast<const uint4*>(src + (size_t)v * 8);
    const int px = (v * 8) / C, c = (v * 8) % C;
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f32x2 f = widen2<T16>(w[k]);
      tile[px * P + c + 2 * k] = f.x;
      tile[px * P + c + 2 * k + 1] = f.y;
    }
  }
  __syncthreads();
  {
    const int px = tid >> 3, part = tid & 7;
    float ss = 0.0f;
    if (px < npx)
      for (int c = part; c < C; c += 8) {
        const float v = tile[px * P + c];
        ss = fmaf(v, v, ss);
      }
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);
    ss += __shfl_xor(ss, 4, 64);
    if (part == 0) inv[px] = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
  }
  __syncthreads();
  const int px = tid & 31;
  if (px < npx) {
    const float d = 1.0f / inv[px];                // divide, as F.normalize does (x / max(norm, eps))
    float* o = out + (size_t)blockIdx.y * C * HW + pix0 + px;
    for (int c = tid >> 5; c < C; c += 8) o[(size_t)c * HW] = tile[px * P + c] / d;
  }
}

// F.interpolate(mode='area') == adaptive average pooling: out[oy,ox] = mean of in[floor(oy*H/OH) .. ceil((oy+1)*H/OH))
// x the same along W (ATen start_index/end_index).  One thread per output element; windows are <= ~5x8 at 1080->256.
__global__ __launch_bounds__(256) void area_resize_kernel(const float* __restrict__ x, float* __restrict__ out, int H,
                                                          int W, int OH, int OW, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ox = idx % OW;
  const int oy = (idx / OW) % OH;
  const long plane = idx / ((long)OW * OH);
  const int y0 = (int)(((long)oy * H) / OH), y1 = (int)((((long)oy + 1) * H + OH - 1) / OH);
  const int x0 = (int)(((long)ox * W) / OW), x1 = (int)((((long)ox + 1) * W + OW - 1) / OW);
  const float* p = x + plane * H * W;
  float s = 0.0f;
  for (int yy = y0; yy < y1; ++yy)
    for (int xx = x0; xx < x1; ++xx) s += p[(size_t)yy * W + xx];
  out[idx] = s / (float)((y1 - y0) * (x1 - x0));
}

// Re-tiling of the uncertainty head's micro-image chain under autograd (align.py UncertaintyModule._patch_statistics_tiled;
// models/modules.py:528-545 runs one 3x3 valid convolution per s x s micro-image): the micro-images are the (k + 2) x (k + 2) tiles of
// one channels-last image, a valid 3x3 convolution of it holds every tile's k x k result at rows / columns t (k + 2) + i, i < k, and the
// next layer wants those as the k x k tiles of a (k h, k w) image.  Forward: dst (B, k h, k w, .) gathers from src (B, (k + 2) h - 2,
// (k + 2) w - 2, .); backward: the gradient of src gathers from the gradient of dst, zero at the dropped positions (windows that
// straddle two tiles) -- no atomics either way.  A pixel is U 16-byte units of any element type (ATen's strided copy of the 6-d view
// ran at 0.4 TB/s and came with two layout conversions per layer: 26 ms of a 125 ms matcher step, profiles/r04_matcher_census.txt).
// `Us`: 16-byte units from one source pixel to the next (>= U: the implicit-GEMM convolution pads its output channels to 64).
__global__ __launch_bounds__(256) void retile_copy_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int h, int w, int k,
                                                          int U, int Us, int backward, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int k2 = k + 2, Hs = k2 * h - 2, Ws = k2 * w - 2, Hd = k * h, Wd = k * w;
  const int u = (int)(idx % U);
  long t = idx / U;
  if (!backward) {                                         // idx over dst (B, Hd, Wd, U)
    const int x = (int)(t % Wd);
    t /= Wd;
    const int y = (int)(t % Hd), b = (int)(t / Hd);
    const int sy = (y / k) * k2 + y % k, sx = (x / k) * k2 + x % k;
    dst[idx] = src[(((long)b * Hs + sy) * Ws + sx) * Us + u];
  } else {                                                 // idx over the gradient of src (B, Hs, Ws, U)
    const int x = (int)(t % Ws);
    t /= Ws;
    const int y = (int)(t % Hs), b = (int)(t / Hs);
    const int i = y % k2, j = x % k2;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (i < k && j < k) v = src[(((long)b * Hd + (y / k2) * k + i) * Wd + (x / k2) * k + j) * Us + u];
    dst[idx] = v;
  }
}

// 2 x 2 / stride 2 max-pool of a channels-last 16-bit map (the pools of the VGG-16 pyramid, models/backbones/vgg.py:33-60:
// nn.MaxPool2d(2, 2), floor mode): a thread owns 8 channels of 2 adjacent output pixels -- 8 independent 16-byte loads in
// flight (ATen's channels-last pool: 0.54 ms for 4 x 1080 x 1920 x 64 = 2.4 TB/s).  Max of representable values: exact.
template <typename T>
__global__ __launch_bounds__(256) void maxpool2x2_nhwc16_kernel(const T* __restrict__ x_, T* __restrict__ y_, int H, int W,
                                                                int OH, int OW, int CV, long total) {
  using S = native_t<T>;
  typedef S V8 __attribute__((ext_vector_type(8)));
  const S* __restrict__ x = reinterpret_cast<const S*>(x_);
  S* __restrict__ y = reinterpret_cast<S*>(y_);
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;                                // total = B * OH * ceil(OW / 2) * CV
  const int OWP = (OW + 1) / 2;
  const int cv = (int)(idx % CV);
  long t = idx / CV;
  const int xp = (int)(t % OWP);
  t /= OWP;
  const int oy = (int)(t % OH), b = (int)(t / OH);
  const long rs = (long)W * CV * 8;
  const S* p = x + ((long)b * H + 2 * oy) * rs + (long)cv * 8;
  V8 v[2][4];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int ix = min(4 * xp + c, W - 1);
      v[r][c] = *(const V8*)(p + r * rs + (long)ix * CV * 8);
    }
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    const int ox = 2 * xp + o;
    if (ox >= OW) break;
    V8 m;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float a = fmaxf((float)v[0][2 * o][e], (float)v[0][2 * o + 1][e]);
      const float c = fmaxf((float)v[1][2 * o][e], (float)v[1][2 * o + 1][e]);
      m[e] = (S)fmaxf(a, c);
    }
    *(V8*)(y + (((long)b * OH + oy) * OW + ox) * CV * 8 + (long)cv * 8) = m;
  }
}

}  // namespace rfn

using namespace rfn;

extern "C" {

int rfn_area_resize_f32(const float* x, float* out, int planes, int H, int W, int OH, int OW, rfn_stream_t stream) {
  RFN_REQUIRE(x && out, "rfn_area_resize_f32: null pointer");
  RFN_REQUIRE(planes > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "rfn_area_resize_f32: non-positive size");
  const long total = (long)planes * OH * OW;
  hipLaunchKernelGGL(area_resize_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, out, H, W, OH,
                     OW, total);
  return check_launch("area_resize_kernel");
}

int rfn_l2norm_channels_f32(const float* x, float* out, int B, int C, int HW, rfn_stream_t stream) {
  RFN_REQUIRE(x && out, "rfn_l2norm_channels_f32: null pointer");
  RFN_REQUIRE(B > 0 && C > 0 && HW > 0 && B <= 65535, "rfn_l2norm_channels_f32: bad size");
  hipStream_t st = (hipStream_t)stream;
  if (C == 128)
    hipLaunchKernelGGL((l2norm_channels_reg_kernel<4, 32>), dim3(cdiv(HW, 64), B), dim3(256), 0, st, x, out, HW);
  else if (C == 256)
    hipLaunchKernelGGL((l2norm_channels_reg_kernel<8, 32>), dim3(cdiv(HW, 32), B), dim3(256), 0, st, x, out, HW);
  else if (C == 512)
    hipLaunchKernelGGL((l2norm_channels_reg_kernel<8, 64>), dim3(cdiv(HW, 32), B), dim3(256), 0, st, x, out, HW);
  else
    hipLaunchKernelGGL(l2norm_channels_kernel, dim3(cdiv(HW, 256), B), dim3(256), 0, st, x, out, C, HW);
  return check_launch("l2norm_channels_kernel");
}

int rfn_l2norm_channels_nhwc16_f32(const void* x, float* out, int B, int C, int HW, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && out, "rfn_l2norm_channels_nhwc16_f32: null pointer");
  RFN_REQUIRE(B > 0 && B <= 65535 && C > 0 && C % 8 == 0 && C <= 2048 && HW > 0,
              "rfn_l2norm_channels_nhwc16_f32: B=%d C=%d (multiple of 8, <= 2048) HW=%d", B, C, HW);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = ((size_t)32 * (C + 1) + 32) * sizeof(float);
  dim3 grid(cdiv(HW, 32), B);
  return dt16_type(dtype, "rfn_l2norm_channels_nhwc16_f32", [&](auto t) {
    const auto kernel = l2norm_nhwc16_to_nchw_kernel<typename decltype(t)::type>;
    if (lds > 48 * 1024 &&
        hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return fail(RFN_ELAUNCH, "l2norm_nhwc16_to_nchw_kernel: %zu bytes of LDS", lds);
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, (const uint16_t*)x, out, C, HW);
    return check_launch("l2norm_nhwc16_to_nchw_kernel");
  });
}

// y (B, H / 2, W / 2, C) = 2 x 2 / stride 2 max-pool (floor mode) of the channels-last 16-bit x (B, H, W, C), C % 8 == 0; dtype 1
// bf16, 2 f16
int rfn_maxpool2x2_nhwc16(const void* x, void* y, int B, int H, int W, int C, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(x && y, "maxpool2x2_nhwc16: null pointer");
  RFN_REQUIRE(B > 0 && H >= 2 && W >= 2 && C > 0 && C % 8 == 0, "maxpool2x2_nhwc16: B=%d H=%d W=%d C=%d (C %% 8)", B, H, W, C);
  const int OH = H / 2, OW = W / 2, CV = C / 8;
  const long total = (long)B * OH * ((OW + 1) / 2) * CV;
  RFN_REQUIRE(total / 256 < 0x7fffffffL, "maxpool2x2_nhwc16: too large");
  const int grid = cdiv(total, 256);
  return dt16_type(dtype, "rfn_maxpool2x2_nhwc16", [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(maxpool2x2_nhwc16_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, H, W, OH, OW,
                       CV, total);
    return check_launch("maxpool2x2_nhwc16");
  });
}

int rfn_retile_copy(const void* src, void* dst, int B, int h, int w, int k, int units16, int src_stride16, int backward,
                    rfn_stream_t stream) {
  RFN_REQUIRE(src && dst, "rfn_retile_copy: null pointer");
  RFN_REQUIRE(B > 0 && h > 0 && w > 0 && k > 0 && units16 > 0 && src_stride16 >= units16, "rfn_retile_copy: bad size");
  RFN_REQUIRE((((size_t)src | (size_t)dst) & 15) == 0, "rfn_retile_copy: pointers must be 16-byte aligned");
  const long Hs = (long)(k + 2) * h - 2, Ws = (long)(k + 2) * w - 2;
  const long total = backward ? (long)B * Hs * Ws * units16 : (long)B * k * h * k * w * units16;
  RFN_REQUIRE(total / 256 < 0x7fffffffL && Hs < 0x7fffffffL && Ws < 0x7fffffffL, "rfn_retile_copy: too large");
  hipLaunchKernelGGL(retile_copy_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)src,
                     (uint4*)dst, h, w, k, units16, src_stride16, backward, total);
  return check_launch("retile_copy");
}

}  // extern "C"
