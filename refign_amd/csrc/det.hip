// refign_amd/csrc/det.hip -- kernels that exist for the deterministic mode (rfn_set_deterministic, include/refign_hip.h):
//   * ordered_colsum: the second launch of every store-and-sum form.  The kernels that used to add per-workgroup partial sums
//     into one destination with floating-point atomics (BatchNorm / depthwise statistics, the DACS image mean, the loss) store
//     one row of partials per workgroup instead; this kernel adds the rows of a column in an order fixed by (rows, cols).
//   * upsample_bilinear2d_bwd: gather form of the backward of F.interpolate(mode='bilinear', align_corners=False).  ATen's
//     backward scatters every output gradient into its four source cells with atomics; here one thread owns one INPUT cell
//     and adds the output pixels that read it in raster order.
#include "bilinear.h"
#include "common.h"

namespace rfn {

// block = cw columns x (256 / cw) row lanes; lane r adds rows r, r + rl, r + 2 rl, ... in that order, lane 0 of a column then
// adds the lanes' sums in lane order
template <typename T>
__global__ __launch_bounds__(256) void ordered_colsum_kernel(const T* __restrict__ part, T* __restrict__ out, long rows, int cols,
                                                             int cw) {
  __shared__ T red[256];
  const int cl = threadIdx.x % cw, r0 = threadIdx.x / cw, rl = 256 / cw;
  const int c = blockIdx.x * cw + cl;
  T s = 0;
  if (c < cols)
    for (long r = r0; r < rows; r += rl) s += part[r * cols + c];
  red[threadIdx.x] = s;
  __syncthreads();
  if (r0 == 0 && c < cols) {
    T t = red[cl];
    for (int k = 1; k < rl; ++k) t += red[k * cw + cl];
    out[c] = t;
  }
}

template <typename T>
static int ordered_colsum(const T* part, T* out, long rows, int cols, hipStream_t st) {
  if (rows < 1 || cols < 1) return fail(RFN_EINVAL, "ordered_colsum: rows=%ld cols=%d", rows, cols);
  int cw = 64;                                   // a function of cols only: the order of the sum must not depend on anything else
  while (cw > 1 && cw > cols) cw >>= 1;
  hipLaunchKernelGGL((ordered_colsum_kernel<T>), dim3(cdiv(cols, cw)), dim3(256), 0, st, part, out, rows, cols, cw);
  return check_launch("ordered_colsum_kernel");
}

int ordered_colsum_f32(const float* part, float* out, long rows, int cols, hipStream_t st) {
  return ordered_colsum<float>(part, out, rows, cols, st);
}
int ordered_colsum_f64(const double* part, double* out, long rows, int cols, hipStream_t st) {
  return ordered_colsum<double>(part, out, rows, cols, st);
}

template <typename T>
__device__ __forceinline__ float bil_ld(const T* p, long i) { return (float)p[i]; }

// grad_in[plane][y][x] = sum over the output pixels (Y, X) that read cell (y, x), Y outer / X inner ascending, of
// wy(Y, y) * wx(X, x) * grad_out[plane][Y][X].  One thread per input cell; consecutive threads = consecutive x (their output
// windows are neighbours, so a wave reads whole rows of grad_out).
template <typename T>
__global__ __launch_bounds__(256) void upsample_bilinear2d_bwd_kernel(const T* __restrict__ gout, T* __restrict__ gin, long planes,
                                                                      int h, int w, int H, int W, float sy, float sx) {
  const long total = planes * h * w;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int x = (int)(i % w), y = (int)((i / w) % h);
    const long pl = i / ((long)w * h);
    int Ylo, Yhi, Xlo, Xhi;
    up_cell_window(y, sy, H, Ylo, Yhi);
    up_cell_window(x, sx, W, Xlo, Xhi);
    const T* g = gout + pl * (long)H * W;
    float acc = 0.f;
    for (int Y = Ylo; Y < Yhi; ++Y) {
      int a0, a1;
      float ly;
      up_src(Y, sy, h, a0, a1, ly);
      if (a0 != y && a1 != y) continue;
      const float wy = (a0 == y ? 1.f - ly : 0.f) + (a1 == y ? ly : 0.f);
      float row = 0.f;
      for (int X = Xlo; X < Xhi; ++X) {
        int b0, b1;
        float lx;
        up_src(X, sx, w, b0, b1, lx);
        if (b0 != x && b1 != x) continue;
        const float wx = (b0 == x ? 1.f - lx : 0.f) + (b1 == x ? lx : 0.f);
        row = fmaf(wx, bil_ld<T>(g, (long)Y * W + X), row);
      }
      acc = fmaf(wy, row, acc);
    }
    gin[i] = (T)acc;
  }
}

}  // namespace rfn

extern "C" {
using namespace rfn;

// grad_in (planes, h, w) <- backward of F.interpolate(x (planes, h, w), size=(H, W), mode='bilinear', align_corners=False)
// for grad_out (planes, H, W); both contiguous, dtype 0 fp32 / 1 bf16 / 2 f16 (sums in fp32).  No atomics: bit-identical from
// launch to launch.  Up-sampling only (H >= h, W >= w).  scale_y / scale_x: ATen's source-index scales (h / H when the caller
// gave size=, 1 / scale_factor when it gave scale_factor=); <= 0 means h / H, w / W.
int rfn_upsample_bilinear2d_bwd(const void* grad_out, void* grad_in, long planes, int h, int w, int H, int W, float scale_y,
                                float scale_x, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(grad_out && grad_in, "upsample_bilinear2d_bwd: null pointer");
  RFN_REQUIRE(planes > 0 && h > 0 && w > 0 && H >= h && W >= w, "upsample_bilinear2d_bwd: planes=%ld %dx%d -> %dx%d (up-sampling only)",
              planes, h, w, H, W);
  RFN_REQUIRE(planes * h * w < (1L << 40) && (long)H * W < (1L << 31), "upsample_bilinear2d_bwd: extent");
  const float sy = scale_y > 0.f ? scale_y : (float)h / (float)H, sx = scale_x > 0.f ? scale_x : (float)w / (float)W;
  RFN_REQUIRE(sy <= 1.f && sx <= 1.f && sy >= 1.f / 64 && sx >= 1.f / 64, "upsample_bilinear2d_bwd: scales %g, %g (1/64 .. 1)", sy, sx);
  const long total = planes * h * w;
  const int blocks = (int)std::min<long>(cdiv(total, 256), 256L * 32);
  hipStream_t s = (hipStream_t)stream;
  return dt_one(dtype, "rfn_upsample_bilinear2d_bwd", [&](auto t) {
    using E = typename decltype(t)::type;
    hipLaunchKernelGGL((upsample_bilinear2d_bwd_kernel<E>), dim3(blocks), dim3(256), 0, s, (const E*)grad_out, (E*)grad_in, planes, h,
                       w, H, W, sy, sx);
    return check_launch("upsample_bilinear2d_bwd_kernel");
  });
}

}  // extern "C"
