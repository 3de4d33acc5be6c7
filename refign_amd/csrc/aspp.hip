// refign_amd/csrc/aspp.hip -- the DeepLabV2 classifier (models/heads/deeplabv2.py: the SUM of R dilated 3x3 convolutions
// C -> K classes, dilation = padding = d_r, bias each) as a tap-GEMM plus a shifted sum.
//
// A dilated 3x3 tap (ky, kx) of branch r is a 1x1 convolution read at the offset (dy, dx) = ((ky - 1) d_r, (kx - 1) d_r).
// So with the T taps whose offset can land inside the map (|dy| < H and |dx| < W: "live") stacked into one (T x Np, C)
// matrix Wt, Np = K rounded up to 8,
//     Z = X_tokens (M x C) @ Wt^T                                   one dense GEMM (rfn_gemm_nt), the input is read once
//     Y[b, y, x, :] = sum_r bias_r + sum_t Z[b, y + dy_t, x + dx_t, t, :]   zero outside the map     (rfn_aspp_tapsum)
// and in the backward
//     dZ[b, y, x, t, :] = gY[b, y - dy_t, x - dx_t, :]                      zero outside the map     (rfn_aspp_tapsum_bwd)
//     dX = dZ @ Wt, dWt = dZ^T X                                    rfn_gemm_nt / rfn_gemm_tn;  dbias_r = column sum of gY.
// Both kernels here are gathers: one thread owns one 16-byte vector (8 channels) of the result and reads the vectors it is
// made of; nothing is accumulated across threads, there is no atomic, the result does not depend on the launch.  They move
// Z once: M x T x Np 16-bit values (2 x 64 x 64 tokens, 36 taps, Np = 24: 14 MB, against 33 MB for the input map itself),
// so they are bound by the cache / memory system; the tap loop keeps kTapIlp independent 16-byte loads in flight per lane.
// Z is 16-bit because it is the GEMM kernel's result type; the T products are summed in fp32 and rounded once.
#include "common.h"
#include "elem.h"

namespace rfn {

constexpr int kAsppMaxTaps = 64;    // 7 branches with every tap live
constexpr int kAsppMaxBias = 8;
constexpr int kTapIlp = 4;

struct AsppTaps {
  short dy[kAsppMaxTaps], dx[kAsppMaxTaps];
  int T;
};

// one thread = 8 channels of one output pixel.  Z: (B H W, ldz) rows, tap t at columns [t Np, (t + 1) Np); Y: (B H W, Np).
template <typename E>
__global__ __launch_bounds__(256) void aspp_tapsum_kernel(const E* __restrict__ Z, long ldz, const float* __restrict__ bias,
                                                          int nbias, AsppTaps taps, E* __restrict__ Y, int H, int W, int NV,
                                                          long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;                                  // total = B H W NV, NV = Np / 8
  const int v = (int)(idx % NV);
  const long pix = idx / NV;                                 // (b H + y) W + x
  const int x = (int)(pix % W), y = (int)((pix / W) % H);
  const int Np = NV * 8;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  for (int r = 0; r < nbias; ++r) {                          // branch order: the order of the unfused sum
    float b[8];
    load8<float>(bias + (long)r * Np + v * 8, b);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += b[i];
  }
  const E* zp = Z + pix * ldz + v * 8;
  for (int t0 = 0; t0 < taps.T; t0 += kTapIlp) {
    uint4 q[kTapIlp];
    bool in[kTapIlp];
#pragma unroll
    for (int j = 0; j < kTapIlp; ++j) {
      const int t = t0 + j;
      in[j] = false;
      if (t < taps.T) {
        const int dy = taps.dy[t], dx = taps.dx[t];
        in[j] = (unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W;
        if (in[j]) q[j] = *reinterpret_cast<const uint4*>(zp + ((long)dy * W + dx) * ldz + (long)t * Np);
      }
    }
#pragma unroll
    for (int j = 0; j < kTapIlp; ++j) {
      if (in[j]) {
        float f[8];
        widen8<E>(q[j], f);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += f[i];
      }
    }
  }
  *reinterpret_cast<uint4*>(Y + pix * Np + v * 8) = narrow8<E>(acc);
}

// one thread = 8 columns of one row of dZ (B H W, ldz): columns [t Np, (t + 1) Np) = gY (B H W, Np) at the pixel shifted by
// MINUS the tap's offset, zeros where that pixel lies outside the map and in the padding columns [T Np, ldz).
template <typename E>
__global__ __launch_bounds__(256) void aspp_tapsum_bwd_kernel(const E* __restrict__ gY, AsppTaps taps, E* __restrict__ dZ, long ldz,
                                                              int H, int W, int NV, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;                                  // total = B H W (ldz / 8)
  const int ZV = (int)(ldz / 8);
  const int cv = (int)(idx % ZV);
  const long pix = idx / ZV;
  const int x = (int)(pix % W), y = (int)((pix / W) % H);
  const int t = cv / NV, v = cv - t * NV;
  uint4 q = make_uint4(0u, 0u, 0u, 0u);
  if (t < taps.T) {
    const int dy = taps.dy[t], dx = taps.dx[t];
    if ((unsigned)(y - dy) < (unsigned)H && (unsigned)(x - dx) < (unsigned)W)
      q = *reinterpret_cast<const uint4*>(gY + (pix - ((long)dy * W + dx)) * (NV * 8) + v * 8);
  }
  *reinterpret_cast<uint4*>(dZ + pix * ldz + (long)cv * 8) = q;
}

static int aspp_taps(const char* who, const int* taps, int T, AsppTaps& out) {
  RFN_REQUIRE(taps != nullptr && T >= 1 && T <= kAsppMaxTaps, "%s: 1 .. %d taps (got %d)", who, kAsppMaxTaps, T);
  out.T = T;
  for (int t = 0; t < kAsppMaxTaps; ++t) {
    const int dy = t < T ? taps[2 * t] : 0, dx = t < T ? taps[2 * t + 1] : 0;
    RFN_REQUIRE(dy > -32768 && dy < 32768 && dx > -32768 && dx < 32768, "%s: tap %d: offset (%d, %d) outside 16 bits", who, t, dy, dx);
    out.dy[t] = (short)dy;
    out.dx[t] = (short)dx;
  }
  return RFN_OK;
}

}  // namespace rfn

using namespace rfn;

extern "C" {

int rfn_aspp_tapsum(const void* Z, long ldz, const float* bias, int nbias, const int* taps, int T, void* Y, int B, int H, int W,
                    int Np, int dtype, rfn_stream_t stream) {
  RFN_REQUIRE(Z && Y && B > 0 && H > 0 && W > 0 && H < 32768 && W < 32768, "rfn_aspp_tapsum: null pointer or empty / oversized map");
  RFN_REQUIRE(Np >= 8 && Np % 8 == 0 && ldz % 8 == 0 && T >= 1 && ldz >= (long)T * Np,
              "rfn_aspp_tapsum: Np and ldz multiples of 8, ldz >= T Np (Np %d, ldz %ld, T %d)", Np, ldz, T);
  RFN_REQUIRE(nbias >= 0 && nbias <= kAsppMaxBias && (nbias == 0 || bias != nullptr), "rfn_aspp_tapsum: 0 .. %d bias rows", kAsppMaxBias);
  RFN_REQUIRE(((size_t)Z & 15) == 0 && ((size_t)Y & 15) == 0 && ((size_t)bias & 15) == 0, "rfn_aspp_tapsum: 16-byte aligned operands");
  AsppTaps tp;
  if (int rc = aspp_taps("rfn_aspp_tapsum", taps, T, tp)) return rc;
  const int NV = Np / 8;
  const long total = (long)B * H * W * NV;
  RFN_REQUIRE(total / 256 < 0x7fffffffL, "rfn_aspp_tapsum: too large");
  return dt16_type(dtype, "rfn_aspp_tapsum", [&](auto tag) {
    using E = typename decltype(tag)::type;
    hipLaunchKernelGGL((aspp_tapsum_kernel<E>), dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const E*)Z, ldz, bias,
                       nbias, tp, (E*)Y, H, W, NV, total);
    return check_launch("aspp_tapsum_kernel");
  });
}

int rfn_aspp_tapsum_bwd(const void* gY, const int* taps, int T, void* dZ, long ldz, int B, int H, int W, int Np, int dtype,
                        rfn_stream_t stream) {
  RFN_REQUIRE(gY && dZ && gY != dZ && B > 0 && H > 0 && W > 0 && H < 32768 && W < 32768,
              "rfn_aspp_tapsum_bwd: null or in-place pointer, or empty / oversized map");
  RFN_REQUIRE(Np >= 8 && Np % 8 == 0 && ldz % 8 == 0 && T >= 1 && ldz >= (long)T * Np,
              "rfn_aspp_tapsum_bwd: Np and ldz multiples of 8, ldz >= T Np (Np %d, ldz %ld, T %d)", Np, ldz, T);
  RFN_REQUIRE(((size_t)gY & 15) == 0 && ((size_t)dZ & 15) == 0, "rfn_aspp_tapsum_bwd: 16-byte aligned operands");
  AsppTaps tp;
  if (int rc = aspp_taps("rfn_aspp_tapsum_bwd", taps, T, tp)) return rc;
  const long total = (long)B * H * W * (ldz / 8);
  RFN_REQUIRE(total / 256 < 0x7fffffffL, "rfn_aspp_tapsum_bwd: too large");
  return dt16_type(dtype, "rfn_aspp_tapsum_bwd", [&](auto tag) {
    using E = typename decltype(tag)::type;
    hipLaunchKernelGGL((aspp_tapsum_bwd_kernel<E>), dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const E*)gY, tp,
                       (E*)dZ, ldz, H, W, Np / 8, total);
    return check_launch("aspp_tapsum_bwd_kernel");
  });
}

}  // extern "C"
