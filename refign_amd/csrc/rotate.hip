// refign_amd/csrc/rotate.hip -- Pillow's NEAREST affine transform in fixed point (libImaging/Geometry.c: affine_fixed), what
// PIL.Image.rotate(angle, NEAREST, expand=False) runs for data_modules/transforms.py:206-247 (RandomRotation of the image, the
// label map and the all-zero normalize_mask).  The six 16.16 coefficients are made on the host in double as Pillow makes them
// (refign_amd/resample.py: rotation_coefficients); per output pixel (y, x)
//     xx = a2 + a1 y + a0 x,  yy = a5 + a4 y + a3 x,  xin = xx >> 16,  yin = yy >> 16   (arithmetic shifts)
// and the pixel is src[yin][xin] inside the image, `fill` (with outside = 1) elsewhere.  Pillow adds a0 / a3 per pixel and
// a1 / a4 per row to running sums; without overflow the products are the same integers, and the entry point refuses sizes at
// which they could pass 2^31.  Lanes along W: byte stores of 64 contiguous pixels per wave and plane; the loads follow the
// rotated row.  photometric.hip gathers through the same coefficients without storing the rotated image.
#include "common.h"

namespace rfn {

constexpr int kRotThreads = 256, kRotTileW = 64, kRotTileH = kRotThreads / kRotTileW;

__global__ __launch_bounds__(kRotThreads) void rotate_nearest_u8_kernel(const unsigned char* __restrict__ src, int C, int H, int W,
                                                                       int a0, int a1, int a2, int a3, int a4, int a5, int fill,
                                                                       unsigned char* __restrict__ out,
                                                                       unsigned char* __restrict__ outside) {
  const int x = blockIdx.x * kRotTileW + (threadIdx.x & (kRotTileW - 1));
  const int y = blockIdx.y * kRotTileH + threadIdx.x / kRotTileW;
  if (x >= W || y >= H) return;
  const int xin = (a2 + a1 * y + a0 * x) >> 16, yin = (a5 + a4 * y + a3 * x) >> 16;
  const bool inside = xin >= 0 && xin < W && yin >= 0 && yin < H;
  const long plane = (long)H * W, o = (long)y * W + x, i = inside ? (long)yin * W + xin : 0;
  for (int c = 0; c < C; ++c) out[c * plane + o] = inside ? src[c * plane + i] : (unsigned char)fill;
  if (outside != nullptr) outside[o] = inside ? 0 : 1;
}

}  // namespace rfn

extern "C" {
using namespace rfn;

// see include/refign_hip.h
int rfn_rotate_nearest_u8(const void* src, int C, int H, int W, int a0, int a1, int a2, int a3, int a4, int a5, int fill,
                          void* out, void* outside, rfn_stream_t stream) {
  RFN_REQUIRE(src && out, "rfn_rotate_nearest_u8: null pointer");
  RFN_REQUIRE(src != out, "rfn_rotate_nearest_u8: not in place");
  RFN_REQUIRE(C >= 1 && C <= 4, "rfn_rotate_nearest_u8: C=%d (1 ... 4)", C);
  RFN_REQUIRE(H >= 1 && W >= 1 && H < 32768 && W < 32768, "rfn_rotate_nearest_u8: H=%d W=%d (each 1 ... 32767)", H, W);
  RFN_REQUIRE(fill >= 0 && fill <= 255, "rfn_rotate_nearest_u8: fill=%d (0 ... 255)", fill);
  const long bx = labs((long)a2) + labs((long)a1) * (H - 1) + labs((long)a0) * (W - 1);
  const long by = labs((long)a5) + labs((long)a4) * (H - 1) + labs((long)a3) * (W - 1);
  RFN_REQUIRE(bx < (1L << 31) && by < (1L << 31),
              "rfn_rotate_nearest_u8: at H=%d W=%d the fixed-point coordinates could pass 2^31 (|xx| <= %ld, |yy| <= %ld)", H, W, bx, by);
  const dim3 grid((unsigned)cdiv(W, kRotTileW), (unsigned)cdiv(H, kRotTileH));
  hipLaunchKernelGGL(rotate_nearest_u8_kernel, grid, dim3(kRotThreads), 0, (hipStream_t)stream, (const unsigned char*)src, C, H, W,
                     a0, a1, a2, a3, a4, a5, fill, (unsigned char*)out, (unsigned char*)outside);
  return check_launch("rotate_nearest_u8_kernel");
}

}  // extern "C"
