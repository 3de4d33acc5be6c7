// refign_amd/csrc/photometric.hip -- the photometric chain on the matcher's image_prime (data_modules/transforms.py:393-519:
// ColorJitter, ChannelShuffle, RandomGaussianBlur, then ConvertImageDtype and Normalize) over a uint8 batch (B, 3, h, w), one
// parameter record per sample (include/refign_hip.h: the record's words), the sample index on the grid.
//   photometric_gray_sum_kernel  the one whole-image quantity of the chain: the contrast step blends with the mean of gray() of
//                                the image AS IT STANDS when the step is reached.  Per pixel the steps in front of contrast, gray(),
//                                summed as integers: a shuffle per wave, LDS per workgroup, one 64-bit integer atomic per workgroup.
//                                The sum is exact, so the mean (float)sum / (float)n is one correctly rounded division and does
//                                not depend on the order of anything.  Samples without a contrast step leave their counter at 0.
//   photometric_apply_kernel     per output pixel the whole chain in the sample's order, the channel permutation, the optional
//                                7 x 7 blur, u8 / 255 and (x - mean) / std, stored as fp32.  A sample with blur stages its 64 x 16
//                                tile plus a 3-pixel halo of the jittered, shuffled uint8 image in LDS (the three channels of a
//                                pixel packed into one word; the jitter is applied while staging, BORDER_REFLECT_101 at the
//                                image's border) and takes the 49 taps from there in row-major order in fp32, then rintf.
//                                Samples with and without blur share the launch: the branch is uniform per workgroup.
// The hue step (step 3; word 7 of the record its flag, word 73 its factor) is adjust_hue of a uint8 image: u8 / 255, _rgb2hsv,
// h = (h + factor) % 1.0, _hsv2rgb, (x * 255) truncated -- pm_hue below.
// With a PmGeom per sample (the *_geom entry points) both kernels GATHER their input pixel through a rotation, a crop and a
// mirror in front of the chain: output pixel (oy, ox) of the (h, w) crop reads pixel (top + oy, left + ox') of the image
// rotated with Pillow's NEAREST fixed-point affine transform (csrc/rotate.hip: the same six integers), ox' = w - 1 - ox when
// mirrored.  Where that falls outside the (H, W) source the pixel is the fill 0, runs through the chain like any other, counts
// in the contrast mean, and the output is 0.0 in all three channels (Normalize's normalize_mask write).  The rotated image is
// never stored.  No blur there (its tile assumes unrotated neighbours): the record's blur flag is not read.
// The arithmetic is torchvision's tensor path for uint8 images restated: every fp32 operation on its own (no contraction),
// products summed left to right, truncation to uint8 after every step.  No floating-point atomics; the jittered uint8 image is
// never written to memory.  Byte loads, lanes along W (64 contiguous bytes per wave and plane); 256-byte fp32 stores per wave.
#include "common.h"

#pragma clang fp contract(off)

namespace rfn {

constexpr int kPmWords = 80, kPmThreads = 256, kPmTileW = 64, kPmTileH = 16, kPmK = 7, kPmR = 3;
constexpr int kPmHaloW = kPmTileW + 2 * kPmR, kPmHaloH = kPmTileH + 2 * kPmR;
constexpr int kPmRowsPerThread = kPmTileH / (kPmThreads / kPmTileW);
constexpr int kPmMaxSumBlocks = 1024;

struct PmRecord {
  int order[4];                                // 0 brightness, 1 contrast, 2 saturation, 3 hue
  int present[4];
  float f[3], g[3];                            // fp32(f), fp32(1.0 - f)
  int perm[3];
  int blur;
  float mean[3], sd[3];
  float k[kPmK * kPmK];
  float hue;                                   // the hue step's factor (present[3])
  int unused[6];
};
static_assert(sizeof(PmRecord) == kPmWords * 4, "the record of include/refign_hip.h");

// the gather in front of the chain (include/refign_hip.h: 12 words per sample)
struct PmGeom {
  int a[6];                                    // Pillow's fixed-point affine coefficients: csrc/rotate.hip
  int top, left, flip;
  int unused[3];
};
static_assert(sizeof(PmGeom) == 12 * 4, "the geometry record of include/refign_hip.h");

// _blend(a, b, f) of a uint8 image: (f * a + (1 - f) * b).clamp(0, 255).to(uint8)
__device__ __forceinline__ int pm_blend(int a, float b, float f, float g) {
  const float v = f * (float)a + g * b;
  return (int)fminf(fmaxf(v, 0.0f), 255.0f);
}

// rgb_to_grayscale of a uint8 image: (0.2989 r + 0.587 g + 0.114 b).to(uint8)
__device__ __forceinline__ int pm_gray(int r, int g, int b) {
  return (int)(0.2989f * (float)r + 0.587f * (float)g + 0.114f * (float)b);
}

// adjust_hue of a uint8 pixel (functional_tensor.py: _rgb2hsv, (h + factor) % 1.0, _hsv2rgb), one fp32 operation at a time.
// The three masked terms of h exclude one another, so their sum is the one selected; the einsum of _hsv2rgb adds five zeros.
// A function of its own (the pixel packed into one word each way: no scratch): inlined into the four unrolled steps of both
// staging loops it took the apply kernel from 78 to 105 SGPRs, below the eight waves per SIMD it had; only samples with the
// step call it.
__device__ __noinline__ int pm_hue_packed(float factor, int rgb) {
  const int ri = rgb & 255, gi = (rgb >> 8) & 255, bi = rgb >> 16;
  const float r = (float)ri / 255.0f, g = (float)gi / 255.0f, b = (float)bi / 255.0f;
  const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.0f : maxc);
  const float div = eqc ? 1.0f : cr;
  const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
  float h = maxc == r ? bc - gc : (maxc == g ? (2.0f + rc) - bc : (4.0f + gc) - rc);
  h = fmodf(h / 6.0f + 1.0f, 1.0f);
  h = fmodf(h + factor, 1.0f);                 // torch.remainder: the sign of the divisor
  if (h < 0.0f) h = h + 1.0f;
  const float h6 = h * 6.0f, fl = floorf(h6), f = h6 - fl;
  const float v = maxc;
  const float p = fminf(fmaxf(v * (1.0f - s), 0.0f), 1.0f);
  const float q = fminf(fmaxf(v * (1.0f - s * f), 0.0f), 1.0f);
  const float t = fminf(fmaxf(v * (1.0f - s * (1.0f - f)), 0.0f), 1.0f);
  const int i = (int)fl % 6;                   // fl in 0 ... 6
  const float ro = i == 0 ? v : (i == 1 ? q : (i == 2 ? p : (i == 3 ? p : (i == 4 ? t : v))));
  const float go = i == 0 ? t : (i == 1 ? v : (i == 2 ? v : (i == 3 ? q : (i == 4 ? p : p))));
  const float bo = i == 0 ? p : (i == 1 ? p : (i == 2 ? t : (i == 3 ? v : (i == 4 ? v : q))));
  return (int)(ro * 255.0f) | ((int)(go * 255.0f) << 8) | ((int)(bo * 255.0f) << 16);
}
__device__ __forceinline__ void pm_hue(float factor, int& r, int& g, int& b) {
  const int o = pm_hue_packed(factor, r | (g << 8) | (b << 16));
  r = o & 255, g = (o >> 8) & 255, b = o >> 16;
}

// the jitter steps in the sample's order; UNTIL_CONTRAST: stop in front of the contrast step (what its mean is taken of)
template <bool UNTIL_CONTRAST>
__device__ __forceinline__ void pm_steps(const PmRecord& p, float gray_mean, int& r, int& g, int& b) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s = p.order[i] & 3;
    if (!p.present[s]) continue;
    if (s == 3) {
      pm_hue(p.hue, r, g, b);
      continue;
    }
    const float f = p.f[s], q = p.g[s];
    if (s == 0) {
      r = pm_blend(r, 0.0f, f, q), g = pm_blend(g, 0.0f, f, q), b = pm_blend(b, 0.0f, f, q);
    } else if (s == 1) {
      if (UNTIL_CONTRAST) return;
      r = pm_blend(r, gray_mean, f, q), g = pm_blend(g, gray_mean, f, q), b = pm_blend(b, gray_mean, f, q);
    } else {
      const float y = (float)pm_gray(r, g, b);
      r = pm_blend(r, y, f, q), g = pm_blend(g, y, f, q), b = pm_blend(b, y, f, q);
    }
  }
}

__device__ __forceinline__ int pm_channel(int c) { return c < 0 ? 0 : (c > 2 ? 2 : c); }
__device__ __forceinline__ int pm_pick(int c, int r, int g, int b) { return c == 0 ? r : (c == 1 ? g : b); }

// BORDER_REFLECT_101 for an index at most kPmR outside [0, n); kept inside for every n >= 1 (n < 4 is refused by the caller)
__device__ __forceinline__ int pm_reflect(int i, int n) {
  i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
  return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// ConvertImageDtype and Normalize of one uint8 value
__device__ __forceinline__ float pm_norm(int u, float mean, float sd) { return ((float)u / 255.0f - mean) / sd; }

// pixel (oy, ox) of the (h, w) crop of the rotated, mirrored (H, W) image `img`: false (and the fill 0) where the source falls
// outside.  The products wrap as unsigned numbers (the host refuses sizes at which they could pass 2^31) and the load is
// bounds-checked: no geometry record can address outside the image.
__device__ __forceinline__ bool pm_gather(const PmGeom& q, const unsigned char* __restrict__ img, long plane, int H, int W, int w,
                                          int oy, int ox, int& r, int& g, int& b) {
  const unsigned y = (unsigned)(q.top + oy), x = (unsigned)(q.left + (q.flip ? w - 1 - ox : ox));
  const int xin = (int)((unsigned)q.a[2] + (unsigned)q.a[1] * y + (unsigned)q.a[0] * x) >> 16;
  const int yin = (int)((unsigned)q.a[5] + (unsigned)q.a[4] * y + (unsigned)q.a[3] * x) >> 16;
  if (xin < 0 || xin >= W || yin < 0 || yin >= H) {
    r = g = b = 0;
    return false;
  }
  const long i = (long)yin * W + xin;
  r = img[i], g = img[plane + i], b = img[2 * plane + i];
  return true;
}

// GEOM: the image is (B, 3, H, W) and the pass runs over the (h, w) crop gathered through geom[bi]; else H = h, W = w
template <bool GEOM>
__global__ __launch_bounds__(kPmThreads) void photometric_gray_sum_kernel(const unsigned char* __restrict__ image,
                                                                         const PmRecord* __restrict__ records,
                                                                         const PmGeom* __restrict__ geom, int H, int W, int h, int w,
                                                                         unsigned long long* __restrict__ sums) {
  const int bi = blockIdx.y;
  const PmRecord& p = records[bi];
  if (!p.present[1]) return;                   // (uniform per workgroup)
  const long plane = (long)h * w, splane = GEOM ? (long)H * W : plane;
  const unsigned char* __restrict__ img = image + (long)bi * 3 * splane;
  unsigned acc = 0;                            // at most plane / (256 * gridDim.x) + 1 pixels of 255 per thread: see the launch
  for (long i = (long)blockIdx.x * kPmThreads + threadIdx.x; i < plane; i += (long)gridDim.x * kPmThreads) {
    int r, g, b;
    if (GEOM) {
      const int oy = (int)(i / w);
      pm_gather(geom[bi], img, splane, H, W, w, oy, (int)(i - (long)oy * w), r, g, b);
    } else {
      r = img[i], g = img[plane + i], b = img[2 * plane + i];
    }
    pm_steps<true>(p, 0.0f, r, g, b);
    acc += (unsigned)pm_gray(r, g, b);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += (unsigned)__shfl_xor((int)acc, o, 64);
  __shared__ unsigned s_sum[kPmThreads / kWave];
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
#pragma unroll
    for (int k = 0; k < kPmThreads / kWave; ++k) t += s_sum[k];
    if (t != 0) atomicAdd(sums + bi, t);
  }
}

template <bool GEOM>
__global__ __launch_bounds__(kPmThreads) void photometric_apply_kernel(const unsigned char* __restrict__ image,
                                                                      const PmRecord* __restrict__ records,
                                                                      const PmGeom* __restrict__ geom,
                                                                      const unsigned long long* __restrict__ sums, int H, int W, int h,
                                                                      int w, float* __restrict__ out) {
  const int bi = blockIdx.z;
  const PmRecord& p = records[bi];
  const long plane = (long)h * w, splane = GEOM ? (long)H * W : plane;
  const unsigned char* __restrict__ img = image + (long)bi * 3 * splane;
  float* __restrict__ o = out + (long)bi * 3 * plane;
  const float gray_mean = sums != nullptr ? (float)sums[bi] / (float)plane : 0.0f;
  const int c0 = pm_channel(p.perm[0]), c1 = pm_channel(p.perm[1]), c2 = pm_channel(p.perm[2]);
  const float m0 = p.mean[0], m1 = p.mean[1], m2 = p.mean[2], s0 = p.sd[0], s1 = p.sd[1], s2 = p.sd[2];
  const int x0 = blockIdx.x * kPmTileW, y0 = blockIdx.y * kPmTileH;
  const int lx = threadIdx.x & (kPmTileW - 1), ly0 = threadIdx.x / kPmTileW;
  const int x = x0 + lx;

  if (GEOM) {
    if (x >= w) return;
    const PmGeom& q = geom[bi];
#pragma unroll
    for (int k = 0; k < kPmRowsPerThread; ++k) {
      const int y = y0 + ly0 + k * (kPmThreads / kPmTileW);
      if (y >= h) break;
      const long i = (long)y * w + x;
      int r, g, b;
      const bool inside = pm_gather(q, img, splane, H, W, w, y, x, r, g, b);
      pm_steps<false>(p, gray_mean, r, g, b);
      o[i] = inside ? pm_norm(pm_pick(c0, r, g, b), m0, s0) : 0.0f;
      o[plane + i] = inside ? pm_norm(pm_pick(c1, r, g, b), m1, s1) : 0.0f;
      o[2 * plane + i] = inside ? pm_norm(pm_pick(c2, r, g, b), m2, s2) : 0.0f;
    }
    return;
  }

  if (!p.blur) {                               // (uniform per workgroup)
    if (x >= w) return;
#pragma unroll
    for (int k = 0; k < kPmRowsPerThread; ++k) {
      const int y = y0 + ly0 + k * (kPmThreads / kPmTileW);
      if (y >= h) break;
      const long i = (long)y * w + x;
      int r = img[i], g = img[plane + i], b = img[2 * plane + i];
      pm_steps<false>(p, gray_mean, r, g, b);
      o[i] = pm_norm(pm_pick(c0, r, g, b), m0, s0);
      o[plane + i] = pm_norm(pm_pick(c1, r, g, b), m1, s1);
      o[2 * plane + i] = pm_norm(pm_pick(c2, r, g, b), m2, s2);
    }
    return;
  }

  // the tile and its halo after jitter and shuffle: channel c of the OUTPUT in byte c of the pixel's word
  __shared__ unsigned s_tile[kPmHaloH * kPmHaloW];
  for (int t = threadIdx.x; t < kPmHaloH * kPmHaloW; t += kPmThreads) {
    const int ty = t / kPmHaloW, tx = t - ty * kPmHaloW;
    const int gy = pm_reflect(y0 - kPmR + ty, h), gx = pm_reflect(x0 - kPmR + tx, w);
    const long i = (long)gy * w + gx;
    int r = img[i], g = img[plane + i], b = img[2 * plane + i];
    pm_steps<false>(p, gray_mean, r, g, b);
    s_tile[t] = (unsigned)pm_pick(c0, r, g, b) | ((unsigned)pm_pick(c1, r, g, b) << 8) | ((unsigned)pm_pick(c2, r, g, b) << 16);
  }
  __syncthreads();
  if (x >= w) return;
#pragma unroll
  for (int k = 0; k < kPmRowsPerThread; ++k) {
    const int ly = ly0 + k * (kPmThreads / kPmTileW), y = y0 + ly;
    if (y >= h) break;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
    for (int dy = 0; dy < kPmK; ++dy) {
#pragma unroll
      for (int dx = 0; dx < kPmK; ++dx) {
        const unsigned u = s_tile[(ly + dy) * kPmHaloW + lx + dx];
        const float wt = p.k[dy * kPmK + dx];
        a0 = a0 + wt * (float)(u & 255u), a1 = a1 + wt * (float)((u >> 8) & 255u), a2 = a2 + wt * (float)((u >> 16) & 255u);
      }
    }
    // torch.round (half to even) and the conversion to uint8
    const int u0 = (int)fminf(fmaxf(rintf(a0), 0.0f), 255.0f), u1 = (int)fminf(fmaxf(rintf(a1), 0.0f), 255.0f);
    const int u2 = (int)fminf(fmaxf(rintf(a2), 0.0f), 255.0f);
    const long i = (long)y * w + x;
    o[i] = pm_norm(u0, m0, s0), o[plane + i] = pm_norm(u1, m1, s1), o[2 * plane + i] = pm_norm(u2, m2, s2);
  }
}

static int pm_check(const char* entry, const void* image, const void* records, int B, int h, int w) {
  RFN_REQUIRE(image && records, "%s: null pointer", entry);
  RFN_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d (1 ... 65535)", entry, B);
  RFN_REQUIRE(h >= 1 && w >= 1 && (long)h * w < (1L << 31) / 3, "%s: h=%d w=%d (each >= 1, 3 h w < 2^31)", entry, h, w);
  return RFN_OK;
}

static int pm_check_geom(const char* entry, const void* geom, int H, int W, int h, int w) {
  RFN_REQUIRE(geom, "%s: null pointer", entry);
  RFN_REQUIRE(H >= 1 && W >= 1 && H < 32768 && W < 32768, "%s: H=%d W=%d (each 1 ... 32767: the fixed-point transform)", entry, H, W);
  RFN_REQUIRE(h <= H && w <= W, "%s: a %d x %d crop of a %d x %d image", entry, h, w, H, W);
  return RFN_OK;
}

static int pm_launch_sums(const char* entry, const void* image, const void* records, const void* geom, int B, int H, int W, int h,
                          int w, unsigned long* sums, hipStream_t st) {
  RFN_REQUIRE(sums, "%s: null pointer", entry);
  int rc = zero_async(sums, (size_t)B * 8, st);
  if (rc != RFN_OK) return rc;
  // (a thread's 32-bit partial: with 1024 workgroups at most 2^31 / 3 / 2^18 + 1 pixels of at most 255)
  const long plane = (long)h * w;
  const int blocks = cdiv(plane, kPmThreads * 8) < kPmMaxSumBlocks ? cdiv(plane, kPmThreads * 8) : kPmMaxSumBlocks;
  const dim3 grid((unsigned)blocks, (unsigned)B);
  if (geom)
    hipLaunchKernelGGL(photometric_gray_sum_kernel<true>, grid, dim3(kPmThreads), 0, st, (const unsigned char*)image,
                       (const PmRecord*)records, (const PmGeom*)geom, H, W, h, w, (unsigned long long*)sums);
  else
    hipLaunchKernelGGL(photometric_gray_sum_kernel<false>, grid, dim3(kPmThreads), 0, st, (const unsigned char*)image,
                       (const PmRecord*)records, (const PmGeom*)nullptr, H, W, h, w, (unsigned long long*)sums);
  return check_launch("photometric_gray_sum_kernel");
}

static int pm_launch_apply(const char* entry, const void* image, const void* records, const void* geom, const unsigned long* sums,
                           int B, int H, int W, int h, int w, float* out, hipStream_t st) {
  RFN_REQUIRE(out, "%s: null pointer", entry);
  const dim3 grid((unsigned)cdiv(w, kPmTileW), (unsigned)cdiv(h, kPmTileH), (unsigned)B);
  RFN_REQUIRE(grid.y <= 65535, "%s: h=%d (at most %d)", entry, h, 65535 * kPmTileH);
  if (geom)
    hipLaunchKernelGGL(photometric_apply_kernel<true>, grid, dim3(kPmThreads), 0, st, (const unsigned char*)image,
                       (const PmRecord*)records, (const PmGeom*)geom, (const unsigned long long*)sums, H, W, h, w, out);
  else
    hipLaunchKernelGGL(photometric_apply_kernel<false>, grid, dim3(kPmThreads), 0, st, (const unsigned char*)image,
                       (const PmRecord*)records, (const PmGeom*)nullptr, (const unsigned long long*)sums, H, W, h, w, out);
  return check_launch("photometric_apply_kernel");
}

}  // namespace rfn

extern "C" {
using namespace rfn;

// see include/refign_hip.h
int rfn_photometric_record_words(void) { return kPmWords; }

int rfn_photometric_gray_sums_u8(const void* image, const void* records, int B, int h, int w, unsigned long* sums,
                                 rfn_stream_t stream) {
  const int rc = pm_check("rfn_photometric_gray_sums_u8", image, records, B, h, w);
  if (rc != RFN_OK) return rc;
  return pm_launch_sums("rfn_photometric_gray_sums_u8", image, records, nullptr, B, h, w, h, w, sums, (hipStream_t)stream);
}

int rfn_photometric_apply_u8(const void* image, const void* records, const unsigned long* sums, int B, int h, int w, float* out,
                             rfn_stream_t stream) {
  const int rc = pm_check("rfn_photometric_apply_u8", image, records, B, h, w);
  if (rc != RFN_OK) return rc;
  return pm_launch_apply("rfn_photometric_apply_u8", image, records, nullptr, sums, B, h, w, h, w, out, (hipStream_t)stream);
}

int rfn_photometric_gray_sums_geom_u8(const void* image, const void* records, const void* geom, int B, int H, int W, int h, int w,
                                      unsigned long* sums, rfn_stream_t stream) {
  int rc = pm_check("rfn_photometric_gray_sums_geom_u8", image, records, B, h, w);
  if (rc != RFN_OK) return rc;
  rc = pm_check_geom("rfn_photometric_gray_sums_geom_u8", geom, H, W, h, w);
  if (rc != RFN_OK) return rc;
  return pm_launch_sums("rfn_photometric_gray_sums_geom_u8", image, records, geom, B, H, W, h, w, sums, (hipStream_t)stream);
}

int rfn_photometric_apply_geom_u8(const void* image, const void* records, const void* geom, const unsigned long* sums, int B, int H,
                                  int W, int h, int w, float* out, rfn_stream_t stream) {
  int rc = pm_check("rfn_photometric_apply_geom_u8", image, records, B, h, w);
  if (rc != RFN_OK) return rc;
  rc = pm_check_geom("rfn_photometric_apply_geom_u8", geom, H, W, h, w);
  if (rc != RFN_OK) return rc;
  return pm_launch_apply("rfn_photometric_apply_geom_u8", image, records, geom, sums, B, H, W, h, w, out, (hipStream_t)stream);
}

}  // extern "C"
