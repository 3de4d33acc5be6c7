// refign_amd/csrc/corr.hip -- spatial correlation sampler for gfx950 (MI355X), written from scratch.
//
// What it computes (reference: models/correlation_ops/correlation.cpp:13-42,80-129; the CUDA twin
// correlation_cuda_kernel.cu:26-88 computes the same numbers on NHWC copies):
//   out[n,ph,pw,h,w] = sum_c sum_{i<kH} sum_{j<kW} in1[n,c,u+i*dil,v+j*dil] * in2[n,c,u+i*dil+sU,v+j*dil+sV]
//   u = -pad + h*stride, v = -pad + w*stride, sU = (ph - (patchH-1)/2)*dil_patch, zero outside the image.
//
// Forward.  The hot path uses ONE parameterisation (kernel 1, patch 9, stride 1, pad 0; models/modules.py:268-270), fp32.  It
// is HBM-bound by design -- 4*(2C+81) bytes per pixel against 162*C flops per pixel (15 flop/B at C=128) -- so both of its
// kernels tile in registers: a thread owns a strip of 4 consecutive pixels x 9 horizontal x 3 vertical shifts = 108 fp32
// accumulators, the three vertical-shift groups of a tile are three sets of waves, and per channel a thread reads 1 + 9
// 16-byte vectors from LDS for 108 FMAs.  Optional ReLU + L2 norm over the 81 shifts in the epilogue (FUSE:
// LocalFeatureCorrelationLayer, modules.py:272-273 -- saves three passes over the 81 x H x W volume).
//   * corr9_pipe2_kernel -- every map with W % 4 == 0, C % 8 == 0, C >= 16 and samples below 4 GB (launch_corr9): tiles of
//     16 x 32 or 8 x 32 pixels, brought in by global -> LDS DMA through a four-stage ring; the tiny maps' cross-workgroup
//     channel split (launch_corr9_split, with corr9_split_reduce_kernel for the two-launch form) runs the same kernel.
//   * corr9_tile_kernel -- everything else of the hot parameterisation: odd widths, few channels, samples of 4 GB and more,
//     and the fused-warp form (WARP: the source tile is bilinear-warped with the flow while it is staged,
//     helpers/matching_utils.py:11-49 -- the warped feature map never exists in HBM).  8 x 64 tiles staged through registers.
//   * corr_generic_fwd_kernel -- any parameterisation, one thread per output element; float, double or half.
//
// Backward (reference: correlation.cpp:44-78,131-183; CUDA gather form correlation_cuda_kernel.cu:91-238):
//   * corr9_bwd_strip_kernel  -- the hot parameterisation, f32, W % 4 == 0, C % 8 == 0: both gradients in one launch;
//   * corr9_bwd_tile_kernel   -- the hot parameterisation otherwise: one pixel per thread, one launch per gradient;
//   * corr_k1_bwd_kernel      -- gather form for kernel 1 / stride 1 / pad 0 (deterministic, no atomics);
//   * corr_generic_bwd_gather_kernel -- half, and fp32 through rfn_corr_bwd_gather_f32; any parameterisation (deterministic);
//   * corr_generic_bwd_kernel -- scatter with hardware float / double atomics for everything else.
// History of the forward (three earlier kernel generations, what was tried and dropped): docs/history/DESIGN_r01-r04.md
// section 10; their measurements are profiles/r01-r06_*corr*.
#include <cstdlib>
#include <type_traits>

#include <hip/hip_fp16.h>

#include "bilinear.h"
#include "common.h"

namespace rfn {

constexpr int kHalo = 4;           // (9-1)/2

// XCD-local block order.  Workgroup b of a launch runs on XCD b % 8 (round-robin dispatch); this returns b's place in an order
// that gives every XCD a contiguous band of tiles, so that the halo rows two neighbouring tiles both fetch meet in ONE L2
// (the launches that use it are a single round: neighbours run side by side; the forward's DMA alone 65 -> 46 us).
__device__ __forceinline__ int xcd_local_order(int wg, int nwg) {
  const int qq = nwg / 8, rr = nwg % 8, xcd = wg % 8, loc = wg / 8;
  return (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + loc;
}

// tile id -> (tile column, tile row, image): columns run fastest
struct TileId {
  int tx, ty, n;
};
__device__ __forceinline__ TileId decode_tile(int bid, int tilesX, int tilesY) {
  TileId t;
  t.tx = bid % tilesX; bid /= tilesX;
  t.ty = bid % tilesY;
  t.n = bid / tilesY;
  return t;
}

// --------------------------------------------------------------------------------------------------------
// Tiled patch-9 forward, register-staged: a workgroup owns an 8 x 64 pixel tile and walks the channels in chunks of 8; per
// chunk the target tile (8 x 64) and the source tile with its 4-pixel halo (16 x 72) are staged in LDS with 16-byte coalesced
// global loads (NCHW rows are contiguous along w).  Lanes 16-31 / 48-63 of a wave take their strips rotated by 14: with the
// 72-dword row pitch every 16-lane group of a 16-byte LDS read then covers 64 distinct banks.  Any width, any channel count.
// --------------------------------------------------------------------------------------------------------
constexpr int kTW = 64;            // tile width in pixels
constexpr int kTH = 8;             // tile height
constexpr int kCC = 8;             // channels per chunk
constexpr int kStrips = 16;        // 4-pixel strips per tile row
constexpr int kPitch = kTW + 2 * kHalo;  // 72 dwords: LDS row pitch of BOTH tiles (same bank geometry)

template <bool FUSE, bool WARP>
__global__ __launch_bounds__(kTH * kStrips * 3) void corr9_tile_kernel(
    const float* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ flow,
    float* __restrict__ out, int C, int H, int W, int tilesX, int tilesY) {
  constexpr int TH = kTH, CC = kCC;
  constexpr int NT = TH * kStrips * 3;
  constexpr int R2 = TH + 2 * kHalo;
  __shared__ __attribute__((aligned(16))) float smem[CC * (R2 + TH) * kPitch];
  float* s2 = smem;                      // [CC][R2][kPitch]  source tile + halo
  float* s1 = smem + CC * R2 * kPitch;   // [CC][TH][kPitch]  target tile

  const int tid = threadIdx.x;
  const TileId id = decode_tile(blockIdx.x, tilesX, tilesY);
  const int n = id.n, h0 = id.ty * TH, w0 = id.tx * kTW;

  const int lane = tid & 63, wave = tid >> 6;
  constexpr int WPG = TH / 4;            // waves per vertical-shift group
  const int dyg = wave / WPG;            // 0..2 : vertical shifts dyg*3 .. dyg*3+2   (wave-uniform)
  const int q = lane >> 4, j = lane & 15;
  const int row = (wave % WPG) * 4 + q;
  const int strip = (q & 1) ? ((j + 14) & 15) : j;   // bank-conflict-free 16-byte reads, see the banner

  const size_t plane = (size_t)H * W;
  const float* p1 = in1 + (size_t)n * C * plane;
  const float* p2 = in2 + (size_t)n * C * plane;
  const bool vec_ok = (W & 3) == 0;

  float acc[3][9][4];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 9; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[a][b][i] = 0.0f;

  for (int c0 = 0; c0 < C; c0 += CC) {
    __syncthreads();  // previous chunk fully consumed
    // ---- stage the target tile: CC x TH rows x 16 float4 ----
    for (int idx = tid; idx < CC * TH * kStrips; idx += NT) {
      const int v = idx % kStrips, r = (idx / kStrips) % TH, c = idx / (kStrips * TH);
      const int gy = h0 + r, gx = w0 + 4 * v, gc = c0 + c;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gc < C && gy < H) {
        const float* src = p1 + (size_t)gc * plane + (size_t)gy * W + gx;
        if (vec_ok && gx + 3 < W) {
          val = *reinterpret_cast<const float4*>(src);
        } else {
          if (gx + 0 < W) val.x = src[0];
          if (gx + 1 < W) val.y = src[1];
          if (gx + 2 < W) val.z = src[2];
          if (gx + 3 < W) val.w = src[3];
        }
      }
      *reinterpret_cast<float4*>(&s1[(c * TH + r) * kPitch + 4 * v]) = val;
    }
    // ---- stage the source tile with halo ----
    if constexpr (!WARP) {
      constexpr int V2 = kPitch / 4;  // 18 float4 per row
      for (int idx = tid; idx < CC * R2 * V2; idx += NT) {
        const int v = idx % V2, r = (idx / V2) % R2, c = idx / (V2 * R2);
        const int gy = h0 - kHalo + r, gx = w0 - kHalo + 4 * v, gc = c0 + c;
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gc < C && gy >= 0 && gy < H) {
          const float* src = p2 + (size_t)gc * plane + (size_t)gy * W + gx;
          if (vec_ok && gx >= 0 && gx + 3 < W) {
            val = *reinterpret_cast<const float4*>(src);
          } else {
            if (gx + 0 >= 0 && gx + 0 < W) val.x = src[0];
            if (gx + 1 >= 0 && gx + 1 < W) val.y = src[1];
            if (gx + 2 >= 0 && gx + 2 < W) val.z = src[2];
            if (gx + 3 >= 0 && gx + 3 < W) val.w = src[3];
          }
        }
        *reinterpret_cast<float4*>(&s2[(c * R2 + r) * kPitch + 4 * v]) = val;
      }
    } else {
      // one (row, col) position per iteration, all CC channels: the bilinear taps are channel-independent
      const float* fl = flow + (size_t)n * 2 * plane;
      for (int pos = tid; pos < R2 * kPitch; pos += NT) {
        const int x = pos % kPitch, r = pos / kPitch;
        const int gy = h0 - kHalo + r, gx = w0 - kHalo + x;
        const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
        WarpTap t;
        if (inside) {
          const float fx = fl[(size_t)gy * W + gx], fy = fl[plane + (size_t)gy * W + gx];
          t = warp_tap((float)gx, (float)gy, fx, fy, H, W);
        }
#pragma unroll
        for (int c = 0; c < CC; ++c) {
          float val = 0.0f;
          if (inside && c0 + c < C) {
            const float* src = p2 + (size_t)(c0 + c) * plane;
            // ATen's grid_sampler_2d order (nw, ne, sw, se), but NOT bilinear.h tap_sample: this sum contracts into one product
            // and three fmas, tap_sample rounds every product -- the two differ in the last bits, so the loop stays written out
            val = src[t.o00] * t.w00 + src[t.o01] * t.w01 + src[t.o10] * t.w10 + src[t.o11] * t.w11;
          }
          s2[(c * R2 + r) * kPitch + x] = val;
        }
      }
    }
    __syncthreads();

    // ---- 108 FMAs per channel per thread ----
#pragma unroll 2
    for (int c = 0; c < CC; ++c) {
      const float4 a = *reinterpret_cast<const float4*>(&s1[(c * TH + row) * kPitch + 4 * strip]);
      const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int dyi = 0; dyi < 3; ++dyi) {
        const float* rp = &s2[(c * R2 + row + dyg * 3 + dyi) * kPitch + 4 * strip];
        const float4 b0 = *reinterpret_cast<const float4*>(rp);
        const float4 b1 = *reinterpret_cast<const float4*>(rp + 4);
        const float4 b2 = *reinterpret_cast<const float4*>(rp + 8);
        const float bv[12] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w};
#pragma unroll
        for (int dx = 0; dx < 9; ++dx)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[dyi][dx][i] = fmaf(av[i], bv[i + dx], acc[dyi][dx][i]);
      }
    }
  }

  // ---- epilogue ----
  const int h = h0 + row, wx = w0 + 4 * strip;
  float scale[4] = {1.f, 1.f, 1.f, 1.f};
  if constexpr (FUSE) {
    float ss[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 9; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v = fmaxf(acc[a][b][i], 0.0f);
          acc[a][b][i] = v;
          ss[i] = fmaf(v, v, ss[i]);
        }
    __syncthreads();  // tiles no longer needed: reuse LDS for the 3-way reduction
    float* red = smem;  // [3][TH][64]
    *reinterpret_cast<float4*>(&red[(dyg * TH + row) * kTW + 4 * strip]) = make_float4(ss[0], ss[1], ss[2], ss[3]);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float tot = red[(0 * TH + row) * kTW + 4 * strip + i] + red[(1 * TH + row) * kTW + 4 * strip + i] +
                        red[(2 * TH + row) * kTW + 4 * strip + i];
      scale[i] = 1.0f / fmaxf(sqrtf(tot), 1e-12f);   // F.normalize: v / max(||v||, eps)
    }
  }
  if (h < H && wx < W) {
    float* obase = out + ((size_t)n * 81 + (size_t)(dyg * 3) * 9) * plane + (size_t)h * W + wx;
    const bool full = vec_ok && wx + 3 < W;
#pragma unroll
    for (int dyi = 0; dyi < 3; ++dyi)
#pragma unroll
      for (int dx = 0; dx < 9; ++dx) {
        float* o = obase + (size_t)(dyi * 9 + dx) * plane;
        float r0 = acc[dyi][dx][0], r1 = acc[dyi][dx][1], r2 = acc[dyi][dx][2], r3 = acc[dyi][dx][3];
        if constexpr (FUSE) { r0 *= scale[0]; r1 *= scale[1]; r2 *= scale[2]; r3 *= scale[3]; }
        if (full) {
          *reinterpret_cast<float4*>(o) = make_float4(r0, r1, r2, r3);
        } else {
          o[0] = r0;
          if (wx + 1 < W) o[1] = r1;
          if (wx + 2 < W) o[2] = r2;
          if (wx + 3 < W) o[3] = r3;
        }
      }
  }
}


// --------------------------------------------------------------------------------------------------------
// Tiled patch-9 forward, pipelined: corr9_pipe2_kernel (W % 4 == 0, C % 8 == 0; launch_corr9 has the selection rule)
//
// Tile and threads.  A WAVE GROUP of TH / 8 x 3 waves owns a TH x 32 pixel tile (TH = 16 or 8): a wave's lanes are 8 rows x 8
// strips of 4 pixels, and the group's three thirds take vertical shifts 0-2, 3-5, 6-8.  The channels go by in CHUNKS of two.
//
// LDS image of a chunk.  `global_load_lds_dwordx4` (global -> LDS DMA: no VGPR round trip, no ds_write) writes 64 lanes x 16
// bytes at a wave-uniform LDS address, so the image is a linear sequence of 16-byte SLOTS, 64 per instruction, in rows of 12
// (48 floats): [target c0 | target c1 | source c0 | source c1], TH rows per target channel (slots 0-7 of a row in use),
// TH + 8 rows per source channel (the tile with its 4-pixel halo: slots 0-9).  The target rows come first so that the border
// between the two tensors falls on an instruction border (2 x TH x 12 slots = a multiple of 64): every instruction then has
// ONE tensor as its source, a scalar 64-bit base + a 32-bit byte offset per lane -- half the address registers, and the loop
// has none to spare (a spilled pointer is reloaded through `s_waitcnt vmcnt(0)`, which waits for every DMA in flight).  A slot
// without a source (outside the image, or the unused end of a row) is masked out of its instruction and is the same slot in
// every chunk: each lane zeroes its own such slots once, and that is the reference's zero padding.
//
// Why the row pitch is 48 floats, and the strip permutation.  A wave's `ds_read_b128` is served in four groups of 16 lanes --
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 -- one LDS cycle each when the group's lanes touch 16 DISTINCT
// slots of the 256-byte bank row (64 banks x 4 bytes; bank = (address / 4) % 64).  With 8 strips per row a group holds one HALF
// row (4 strips) of each of four consecutive rows.  A row needs 10 slots (32 + 2 x 4 pixels); at a pitch of 12 slots four
// consecutive rows start at slots 0, 12, 8, 4 of the bank row, so four half rows tile it exactly -- if they are the SAME half of
// every row.  The hardware's groups take lanes 0-3 of rows 0 and 3 but lanes 4-7 of rows 1 and 2 (and the other way round), so
// rows 1 and 2 of every four swap their halves: strip = j ^ 4 there.  Group one then reads strips 0-3 of the four rows at slots
// 0-3, 12-15, 8-11, 4-7, group two strips 4-7 at 4-7, 0-3, 12-15, 8-11: conflict-free, and so is every other read of the loop
// (the next 16 bytes of a source row, another channel or vertical shift: a constant added to the whole group).  An unpadded
// pitch of 10 slots starts the rows at 0, 10, 4, 14 and no permutation of half rows avoids the overlap.  The pitch also makes
// the target rows fill whole instructions (above) and gives the paired edge tiles (PAIR) their 2 x 24 floats per row.
//
// The ring and its counted waits.  Each wave group has a ring of kStages = 4 chunk images: three chunks are in flight while one
// is consumed.  A wave issues K instructions per chunk (K or K - 1 of them with a source) and the DMAs of a wave complete in
// order, so "my part of chunk c has landed" is `s_waitcnt vmcnt(n)` with n = the instructions of the NEWER chunks in flight;
// the barrier behind it extends that to every wave's part and says that everybody is done with chunk c - 1, whose stage takes
// chunk c + 3 -- issued one instruction at a time between the row steps of chunk c.  ONE barrier per chunk, and no compiler-
// visible dependence between DMA and `ds_read` (see lds_dma16_masked).  The tile's last four chunks have fewer chunks behind
// them and get their own, smaller counts: a constant count lets a wave read the last chunks before they have landed (the race
// that tools/micro/corr_race.py and tests/test_race_gpu.py look for).
//
// A chunk's arithmetic: six (channel, vertical shift) row steps, unrolled, each one target vector x three source vectors = 36
// products as 16 `v_pk_fma_f32` + 4 `v_fmac_f32`; the three `ds_read_b128` of step s + 1 are issued into a second register set
// in front of the products of step s (`sched_barrier` pins the order).  The loop is VALU-bound, not LDS-bound: ten reads against
// 60 product instructions per channel (profiles/r04_pmc_corr9.txt, r05_pmc_corr9.txt).
//
// Template parameters.
//   TH, TW  tile size; TW is 32 (every constant of the bank argument above depends on it).
//   FUSE    ReLU + L2 norm over the 81 shifts in the epilogue.
//   NTILE   wave groups per workgroup.  Without KSPLIT each owns a tile of its own (ids NTILE b, NTILE b + 1, ..), its own rings
//           and its own DMA stream; only the barrier is shared.  Level 1 (2 x 270 x 480) runs two 16 x 32 tiles per workgroup:
//           twelve waves per CU at 168 registers (a 6-wave workgroup's 2, 2, 1, 1 placement over the SIMDs leaves no room for a
//           second one), and 510 tiles = 255 workgroups = one even round over the 256 CUs.
//   KSPLIT  the NTILE = 2 or 4 wave groups walk the halves / quarters of the channels of ONE tile, each through its own ring;
//           groups 1.. hand their 108 sums per lane to group 0 through the LDS in front of the epilogue (added in group order:
//           deterministic).  For maps of at most one tile per CU: a CU, not a wave, is what a chunk waits for.
//   PAIR    a map whose width leaves at most HALF a tile column over (240 = 7 x 32 + 16) would spend a whole tile per row band
//           on it.  The left-over column band of TWO images shares one tile instead: strips 0-3 are image n's last columns,
//           strips 4-7 image n + 1's (same rows), each half with its own halo in the 48-float row (2 x 24).  Only per-lane
//           constants change (DMA source offsets, the source-row base, the store address).  `tilesX` then counts the FULL tile
//           columns; tiles [0, nreg) are regular, tiles [nreg, ntiles) the (image pair, row band) edge tiles.
//   JOIN    the cross-workgroup channel split of tiny maps in ONE launch (launch_corr9_split): gridDim.y workgroups share a tile,
//           each walks the slice [blockIdx.y C, (blockIdx.y + 1) C) of the Ctot channels and stores its raw partial volume at
//           out + blockIdx.y part_stride, then takes a ticket; the LAST arriver adds the slices in slice order (deterministic),
//           applies ReLU + L2 norm and writes `joined`.  Publication across XCDs (their L2s are not coherent with each other):
//           slab stores, vmcnt(0), barrier, agent-scope release fence, relaxed agent-scope ticket; the joining workgroup takes
//           an agent-scope acquire fence before it reads.  The tickets are zero on entry and the joining workgroup puts its
//           ticket back to zero: the caller zeroes them ONCE per workspace, never per launch (a memset node per launch came out
//           stale under hipGraph replay: profiles/r05_corr_level3_one_launch.txt).
// --------------------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));


// The DMA instruction goes through inline asm, NOT `__builtin_amdgcn_global_load_lds`: with the builtin hipcc tracks the pending
// LDS write and puts `s_waitcnt vmcnt(0)` in front of every `ds_read` it cannot prove disjoint -- inside the channel loop, so
// that no DMA overlapped any arithmetic (profiles/r01_kbench_corr_ablation.txt).  With asm the hand-off is ours: counted waits.
// The lane mask is applied WITHOUT control flow the compiler can see (exec is narrowed and restored inside the statement): a
// branch around the instruction splits the unrolled chunk into basic blocks, the products sink out of their steps, and the
// registers spill.  Scalar 64-bit base + 32-bit byte offset per lane; lane i lands at lds_wave_base + 16 i.
__device__ __forceinline__ void lds_dma16_masked(const void* sbase, unsigned voff, unsigned lds_wave_base,
                                                 unsigned long long mask) {
  unsigned long long saved;
  asm volatile("s_mov_b32 m0, %3\n\ts_and_saveexec_b64 %0, %4\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b64 exec, %0"
               : "=&s"(saved) : "v"(voff), "s"(sbase), "s"(lds_wave_base), "s"(mask) : "memory", "m0", "scc");
}

constexpr int kStages = 4;                              // ring stages per wave group
constexpr int pipe2_threads(int TH, int TW, int NTILE) { return TH * (TW / 4) * 3 * NTILE; }

template <int TH, int TW, bool FUSE, int NTILE, bool KSPLIT = false, bool PAIR = false, bool JOIN = false>
__global__ __launch_bounds__(pipe2_threads(TH, TW, NTILE), 3) void corr9_pipe2_kernel(
    const float* __restrict__ in1, const float* __restrict__ in2, float* __restrict__ out, int C, int H, int W,
    int tilesX, int tilesY, int ntiles, int xcd_remap, int nreg, int Ctot, long part_stride, float* __restrict__ joined,
    unsigned* __restrict__ tickets) {
  // (C = the channels THIS workgroup walks, Ctot = the tensors' channel count: equal except under launch_corr9_split)
  static_assert(TW == 32, "the LDS row pitch and the strip permutation are worked out for 32-pixel tile rows");
  constexpr int NS = kStages;
  constexpr int CC = 2;                                // channels per chunk
  constexpr int STRIPS = TW / 4;                       // 8 strips per tile row
  constexpr int RPW = 64 / STRIPS;                     // 8 rows per wave
  constexpr int NT = TH * STRIPS * 3;                  // threads of a wave group
  constexpr int NW = NT / 64;
  constexpr int R2 = TH + 2 * kHalo;                   // source rows per channel
  constexpr int ROWS = R2 + TH;
  constexpr int PITCH = 48;                            // floats per LDS row (see the banner)
  constexpr int V = PITCH / 4;                         // slots per row
  constexpr int VU2 = (TW + 2 * kHalo) / 4;            // slots of a source row in use
  constexpr int SLOTS = CC * ROWS * V;
  constexpr int NINSTR = (SLOTS + 63) / 64;            // DMA instructions per chunk
  constexpr int K = (NINSTR + NW - 1) / NW;            // ... per wave
  constexpr int BUF = NINSTR * 64 * 4;                 // floats per chunk image
  // the rings: [stage][wave group][BUF]
  static_assert(NS >= 3 && NS * NTILE * BUF * 4 <= 160 * 1024, "ring fits the LDS");
  static_assert(!KSPLIT || ((NTILE == 2 || NTILE == 4) && NS * NTILE * BUF >= (NTILE - 1) * 36 * NT),
                "channel split: two or four wave groups, sums exchanged in the rings");
  __shared__ __attribute__((aligned(16))) float rings_all[NS * NTILE * BUF];
  constexpr unsigned RB = NTILE * BUF * 4;             // bytes from one stage to the next

  const int gw = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // scalar: DMA destinations live in SGPRs
  const int half = gw / NW, wave = gw % NW;            // my wave group, my wave in it
  const int lane = threadIdx.x & 63;
  int wg = blockIdx.x;
  if (xcd_remap) wg = xcd_local_order(wg, gridDim.x);
  const int tile = KSPLIT ? wg : wg * NTILE + half;
  const bool live = tile < ntiles;                     // (an odd tile count leaves the last workgroup's second group without one)
  int bid = live ? tile : 0;
  const bool edge = PAIR && bid >= nreg;               // (scalar) a left-over column band shared by images n and n + 1
  TileId id;
  if (edge) {
    bid -= nreg;
    id.tx = tilesX;
    id.ty = bid % tilesY;
    id.n = 2 * (bid / tilesY);
  } else {
    id = decode_tile(bid, tilesX, tilesY);
  }
  const int n = id.n, h0 = id.ty * TH, w0 = id.tx * TW;
  constexpr int WPG = TH / RPW;                        // waves per vertical-shift group
  const int dyg = wave / WPG;
  const int q = lane / STRIPS, j = lane % STRIPS;
  const int row = (wave % WPG) * RPW + q;
  const int strip = j ^ ((((q & 3) == 1) || ((q & 3) == 2)) ? 4 : 0);   // rows 1, 2 of every four swap their halves (banner)

  const size_t plane = (size_t)H * W;
  const int Cw = KSPLIT ? C / NTILE : C;              // the channels this wave group walks (KSPLIT: group g takes [g Cw, (g+1) Cw))
  const size_t c0 = (size_t)blockIdx.y * C + (KSPLIT ? (size_t)half * Cw : 0);
  const float* p1 = in1 + ((size_t)n * Ctot + c0) * plane;
  const float* p2 = in2 + ((size_t)n * Ctot + c0) * plane;
  const float* const slab0 = out;                      // (JOIN) slice 0 of the partial volumes
  out += (size_t)blockIdx.y * part_stride;

  // per-lane DMA constants: where slot (k-th instruction of mine, lane) of a chunk comes from
  constexpr int F1SLOTS = CC * TH * V;
  static_assert(F1SLOTS % 64 == 0, "the target rows of a chunk must fill whole DMA instructions");
  constexpr int F2BASE = CC * TH * PITCH;              // float offset of the source rows in a ring buffer
  unsigned goff[K];
  unsigned long long gmask[K];                         // lanes of my k-th DMA instruction that have a source (scalar)
  const float* gbase[K];                               // scalar: p1 or p2
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int wi = wave + k * NW;
    const int slot = wi * 64 + lane;
    bool ok = live && (wi < NINSTR) && (slot < SLOTS);
    long off;
    if (wi * 64 < F1SLOTS) {                           // scalar
      const int v = slot % V, rr = (slot / V) % TH, c = slot / (V * TH);
      const int sel = (edge && v >= STRIPS / 2) ? 1 : 0;                   // second image of an edge tile
      const int gy = h0 + rr, gx = w0 + 4 * (v - sel * (STRIPS / 2));
      ok = ok && v < STRIPS && gy < H && gx + 3 < W;
      off = ((long)c + (long)sel * Ctot) * (long)plane + (long)gy * W + gx;
      gbase[k] = p1;
    } else {
      const int s2 = slot - F1SLOTS;
      const int v = s2 % V, rr = (s2 / V) % R2, c = s2 / (V * R2);
      // edge tile: vectors 0 .. V/2 - 1 = image n's columns w0 - 4 .. w0 + 19, vectors V/2 .. V - 1 the same of image n + 1
      const int sel = (edge && v >= V / 2) ? 1 : 0;
      const int gy = h0 - kHalo + rr, gx = w0 - kHalo + 4 * (v - sel * (V / 2));
      ok = ok && (edge || v < VU2) && gy >= 0 && gy < H && gx >= 0 && gx + 3 < W;
      off = ((long)c + (long)sel * Ctot) * (long)plane + (long)gy * W + gx;
      gbase[k] = p2;
    }
    goff[k] = ok ? (unsigned)(off * (long)sizeof(float)) : 0u;
    gmask[k] = __builtin_amdgcn_ballot_w64(ok);
  }

  // one DMA instruction of mine (k-th of the chunk; `on` = all ones, or zero for the chunks past the tile's last) -- issued
  // ONE AT A TIME between the row steps of a chunk: right behind the barrier every wave of the SIMD is in the same phase,
  // and three vector-memory issues in a row there idle the VALU
  const unsigned chunk_bytes = (unsigned)(CC * plane * sizeof(float));
  auto lds_addr = [](float* p) { return (unsigned)(size_t)(__attribute__((address_space(3))) float*)p; };
  auto issue1 = [&](unsigned ring, int k, unsigned long long on) {
    const int wi = wave + k * NW;                      // scalar
    lds_dma16_masked(gbase[k], goff[k], ring + (unsigned)wi * 1024u, gmask[k] & on);
    goff[k] += chunk_bytes;
  };
  const unsigned lds0 = lds_addr(rings_all + half * BUF);              // my tile's stage 0 (scalar); stage r at lds0 + r * RB
  auto issue = [&](unsigned ring) {
#pragma unroll
    for (int k = 0; k < K; ++k) issue1(ring, k, ~0ull);
  };

  f32x2 accp[3][4][4];
  float accs[3][4];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      accs[a][i] = 0.0f;
#pragma unroll
      for (int p = 0; p < 4; ++p) accp[a][i][p] = f32x2{0.0f, 0.0f};
    }

  const int a_off = row * PITCH + 4 * strip;                           // my 4 target pixels (channel 0 of the chunk)
  // my first source row (vertical shift dyg * 3); the second half of an edge tile reads the second image's columns, which
  // start V / 2 vectors into the row (a uniform shift per LDS lane group: strips 0..3 and 4..7 are never in one group)
  const int b_off = F2BASE + (row + dyg * 3) * PITCH + 4 * strip + ((edge && strip >= STRIPS / 2) ? 4 * (V / 2 - STRIPS / 2) : 0);

  // one (channel, vertical shift) row step: 36 products of 4 target pixels with 12 source pixels = 16 packed + 4 single FMAs.
  // VOLATILE asm on purpose: products are pure arithmetic, and nothing else keeps the compiler from emitting them behind the
  // block's last side effect (= behind the next chunks' barriers, every loaded row spilled); volatile statements keep their
  // order among themselves and with the DMA statements and barriers.  The broadcast of a target pixel is an op_sel of the pair
  // it was loaded in (no move).
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  auto step = [&](const f32x4& a, const f32x4* b, int dyi) {
    const f32x2 ap[2] = {a.xy, a.zw};
    const f32x2 bp[6] = {b[0].xy, b[0].zw, b[1].xy, b[1].zw, b[2].xy, b[2].zw};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const f32x2 bb = bp[(i + 2 * p + (i & 1)) / 2];
        if (i & 1) asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0]" : "+v"(accp[dyi][i][p]) : "v"(ap[i >> 1]), "v"(bb));
        else asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(accp[dyi][i][p]) : "v"(ap[i >> 1]), "v"(bb));
      }
      const int kb = (i & 1) ? i : i + 8;
      asm volatile("v_fmac_f32 %0, %1, %2" : "+v"(accs[dyi][i]) : "v"(a[i]), "v"(b[kb >> 2][kb & 3]));
    }
  };
  // LDS reads by byte address: per-lane base (of the ring in use) + immediate offset
  typedef const __attribute__((address_space(3))) f32x4* lds_f32x4_ptr;
  auto lds_ld = [](unsigned addr) { return *(lds_f32x4_ptr)(size_t)addr; };
  auto ldrow = [&](f32x4* b, unsigned pb, int st) {          // st = c * 3 + dyi, compile-time after unrolling
    const unsigned rp = pb + (unsigned)(((st / 3) * R2 + (st % 3)) * PITCH * 4);
    b[0] = lds_ld(rp);
    b[1] = lds_ld(rp + 16);
    b[2] = lds_ld(rp + 32);
  };
  // A chunk in two parts of three row steps.  `nxt`: the stage that takes the chunk three ahead (`on` = 0 for the tile's last
  // three chunks: nothing to fetch); its K DMA instructions go between the row steps of the part that has ISSUE set.  Each part
  // is ONE basic block: no run-time test in here.  The source-row reads run one row step ahead of the products, into the other
  // of two register sets; the sets live across the parts (the first row of part two is requested under the last step of part one).
  static_assert(K <= 3 && CC == 2, "one DMA instruction per row step of a part");
  f32x4 ra[CC], rb[2][3];
  unsigned pa = 0, pb = 0;                             // my target-row / first-source-row byte addresses in the ring in use
  auto part = [&](int cur, int nxt, unsigned long long on, auto second, auto with_issue) {     // stage indices
    constexpr int S0 = decltype(second)::value ? 3 : 0;
    constexpr bool ISSUE = decltype(with_issue)::value;
    const unsigned nx = lds0 + (unsigned)nxt * RB;
    if constexpr (S0 == 0) {
      // (the stage's address passes through a volatile asm: otherwise the compiler keeps eight per-lane addresses, two per
      // stage, alive across the loop, and at 168 registers that is eight spills reloaded through `s_waitcnt vmcnt(0)`)
      unsigned sb = lds0 + (unsigned)cur * RB;
      asm volatile("" : "+s"(sb));
      pa = sb + (unsigned)a_off * 4u;
      pb = sb + (unsigned)b_off * 4u;
      ra[0] = lds_ld(pa);
      ldrow(rb[0], pb, 0);
      ra[1] = lds_ld(pa + (unsigned)(TH * PITCH * 4));
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int st = S0; st < S0 + 3; ++st) {
      if (st + 1 < CC * 3) ldrow(rb[(st + 1) % 2], pb, st + 1);
      __builtin_amdgcn_sched_barrier(0);
      step(ra[st / 3], rb[st % 2], st % 3);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (ISSUE) {
        if (st - S0 < K) {
          issue1(nx, st - S0, on);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  };

  const int nchunks = Cw / CC;                         // multiple of NS (checked by the launcher)
  // chunk hand-off: my own DMA of the chunk has landed once at most `nwait` newer instructions of mine are in flight (in-order
  // completion); the barrier extends that to every wave's and says that everybody is done with the stage about to be refilled
  auto handoff = [&](auto nwait) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(decltype(nwait)::value) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  static_assert((NS - 2) * (K - 1) <= 63, "vmcnt is a 6-bit count");
  const std::false_type first{}, no_issue{};
  const std::true_type second{}, do_issue{};
#pragma unroll
  for (int r = 0; r < NS - 1; ++r) issue(lds0 + r * RB);               // chunks 0 .. NS - 2
  // Zero padding: each lane zeroes ITS slots without a source in every stage, once, AFTER the first chunks are on their way
  // (disjoint addresses; zeroing the whole ring in front of the first DMA costs ~1 us of synchronisation).
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int wi = wave + k * NW;
    if (wi < NINSTR && !((gmask[k] >> lane) & 1)) {
#pragma unroll
      for (int r = 0; r < NS; ++r)
        *reinterpret_cast<float4*>(rings_all + (r * NTILE + half) * BUF + wi * 256 + lane * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // visible to the others behind the first hand-off's barrier
  // barrier in FRONT of chunk c (chunk c landed; chunks c+1 .. c+NS-2 in flight), DMA of chunk c+NS-1 under its first part.
  // NS - 2 newer chunks of K or K - 1 instructions each: counting K - 1 is exact for the waves with an empty last instruction
  // and waits a little longer than needed in the others.  (Both wave groups keep the SAME phase: profiles/r04_corr_pipe2.txt.)
  const std::integral_constant<int, (NS - 2) * (K - 1)> full_behind{};
  for (int ck = 0; ck < nchunks - NS; ck += NS) {        // nchunks is a multiple of NS (checked by the launcher)
    static_for<0, NS>([&](auto rc) {
      constexpr int r = decltype(rc)::value;
      handoff(full_behind);
      part(r, (r + NS - 1) % NS, ~0ull, first, do_issue);
      part(r, (r + NS - 1) % NS, ~0ull, second, no_issue);
    });
  }
  // The tile's last NS chunks, with the waits THEIR queue needs: behind chunk n - NS + r only NS - 1 - r chunks are in flight.
  // Do NOT fold this into the loop's constant count: a wave would read the last chunks before they have landed (seen:
  // tools/micro/corr_race.py, 11 of 300 launches off by the last channels' products under memory load).
  static_for<0, NS>([&](auto rc) {
    constexpr int r = decltype(rc)::value;
    constexpr int behind = (r == 0 ? NS - 2 : NS - 1 - r) * (K - 1);
    handoff(std::integral_constant<int, behind>{});
    if constexpr (r == 0) part(0, NS - 1, ~0ull, first, do_issue);      // chunk n - 1 goes out under chunk n - NS
    else part(r, 0, 0ull, first, no_issue);
    part(r, 0, 0ull, second, no_issue);
  });
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  if constexpr (KSPLIT) {
    // the other wave groups' sums join the first's: [36][NT] floats per group and round (16 pairs + 4 singles of one vertical
    // shift), lane-contiguous (no bank conflict), in the rings' memory -- behind a barrier, because a slower wave may still be
    // reading its last chunk.  Group 0 adds groups 1, 2, 3 in that order (deterministic).
    const int t = (int)threadIdx.x - half * NT;
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (half != 0) {
        f32x2* red2 = reinterpret_cast<f32x2*>(rings_all + (half - 1) * 36 * NT);
        float* red1 = rings_all + (half - 1) * 36 * NT + 32 * NT;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int p = 0; p < 4; ++p) red2[(i * 4 + p) * NT + t] = accp[a][i][p];
          red1[i * NT + t] = accs[a][i];
        }
      }
      __syncthreads();
      if (half == 0) {
#pragma unroll
        for (int hh = 1; hh < NTILE; ++hh) {
          const f32x2* red2 = reinterpret_cast<const f32x2*>(rings_all + (hh - 1) * 36 * NT);
          const float* red1 = rings_all + (hh - 1) * 36 * NT + 32 * NT;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int p = 0; p < 4; ++p) accp[a][i][p] += red2[(i * 4 + p) * NT + t];
            accs[a][i] += red1[i * NT + t];
          }
        }
      }
      __syncthreads();
    }
  }

  // ---- epilogue: ReLU + L2 norm over the 81 shifts on the register PAIRS (packed squares, the ReLU kept in the accumulators;
  // the sum of squares is taken pair-wise, then across the three vertical-shift groups through stage 0 of the ring) ----
  auto get = [&](int dyi, int dx, int i) -> float {
    if (i & 1) return dx == 0 ? accs[dyi][i] : accp[dyi][i][(dx - 1) >> 1][(dx - 1) & 1];
    return dx == 8 ? accs[dyi][i] : accp[dyi][i][dx >> 1][dx & 1];
  };
  const bool img2 = edge && strip >= STRIPS / 2;
  const int h = h0 + row, wx = w0 + 4 * (img2 ? strip - STRIPS / 2 : strip);
  float scale[4] = {1.f, 1.f, 1.f, 1.f};
  if constexpr (FUSE) {
    f32x2 ssp[4];
    float ss[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ssp[i] = f32x2{0.f, 0.f};
      ss[i] = 0.f;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const f32x2 v = __builtin_elementwise_max(accp[a][i][p], f32x2{0.f, 0.f});
          accp[a][i][p] = v;
          ssp[i] = __builtin_elementwise_fma(v, v, ssp[i]);
        }
        const float v = fmaxf(accs[a][i], 0.0f);
        accs[a][i] = v;
        ss[i] = fmaf(v, v, ss[i]);
      }
#pragma unroll
    for (int i = 0; i < 4; ++i) ss[i] += ssp[i][0] + ssp[i][1];
    __syncthreads();
    float* red = rings_all + half * BUF;  // [3][TH][TW]: stage 0 of my tile
    *reinterpret_cast<float4*>(&red[(dyg * TH + row) * TW + 4 * strip]) = make_float4(ss[0], ss[1], ss[2], ss[3]);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float tot = red[(0 * TH + row) * TW + 4 * strip + i] + red[(1 * TH + row) * TW + 4 * strip + i] +
                        red[(2 * TH + row) * TW + 4 * strip + i];
      scale[i] = 1.0f / fmaxf(sqrtf(tot), 1e-12f);
    }
  }
  if (live && (!KSPLIT || half == 0) && h < H && wx + 3 < W) {
    float* o = out + ((size_t)(n + (img2 ? 1 : 0)) * 81 + (size_t)(dyg * 3) * 9) * plane + (size_t)h * W + wx;
#pragma unroll
    for (int dyi = 0; dyi < 3; ++dyi)
#pragma unroll
      for (int dx = 0; dx < 9; ++dx) {
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v val = {get(dyi, dx, 0) * scale[0], get(dyi, dx, 1) * scale[1], get(dyi, dx, 2) * scale[2], get(dyi, dx, 3) * scale[3]};
        *reinterpret_cast<f4v*>(o) = val;               // (non-temporal stores: measured, no change -- profiles/r06_corr_nt_store_ab.txt)
        o += plane;                                    // (a running pointer: one 64-bit add per store instead of a 64-bit multiply-add)
      }
  }
  if constexpr (JOIN) {
    static_assert(!FUSE && !PAIR && KSPLIT, "JOIN: raw partial sums of one tile per workgroup");
    constexpr int PX = TH * TW, NTH = NT * NTILE;
    static_assert((81 * PX + PX) <= NS * NTILE * BUF, "JOIN: the tile's volume fits the rings");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                   // every wave's slab stores have left; the rings are free
    int* flag = reinterpret_cast<int*>(rings_all);
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned prev = __hip_atomic_fetch_add(&tickets[tile], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = prev == gridDim.y - 1;
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        // nobody else touches this ticket in this launch: back to zero for the next one (the caller zeroes the tickets ONCE)
        __hip_atomic_store(&tickets[tile], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      flag[0] = last;
    }
    __syncthreads();
    const int last = flag[0];
    __syncthreads();
    if (!last) return;
    float* acc = rings_all;                            // [81][PX]
    float* scl = rings_all + 81 * PX;                  // [PX]
    const int S = (int)gridDim.y;
    const float* pbase = slab0 + (size_t)n * 81 * plane;
    for (int idx = threadIdx.x; idx < 81 * (PX / 4); idx += NTH) {
      const int d = idx / (PX / 4), sp = idx % (PX / 4), rr = sp / STRIPS, st = sp % STRIPS;
      const int hh = h0 + rr, ww = w0 + 4 * st;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (hh < H && ww < W) {
        const float* q = pbase + (size_t)d * plane + (size_t)hh * W + ww;
        v = *reinterpret_cast<const float4*>(q);
#pragma unroll 4
        for (int sl = 1; sl < S; ++sl) {               // slice order: the same sum for every launch geometry
          const float4 t = *reinterpret_cast<const float4*>(q + (size_t)sl * part_stride);
          v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        }
      }
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
      *reinterpret_cast<float4*>(&acc[d * PX + 4 * sp]) = v;
    }
    __syncthreads();
    for (int px = threadIdx.x; px < PX; px += NTH) {
      float tot = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) {                    // the three vertical-shift groups of the one-kernel epilogue, in its order
        float ss = 0.f;
#pragma unroll
        for (int d = 0; d < 27; ++d) {
          const float r = acc[(k * 27 + d) * PX + px];
          ss = fmaf(r, r, ss);
        }
        tot = k == 0 ? ss : tot + ss;
      }
      scl[px] = 1.0f / fmaxf(sqrtf(tot), 1e-12f);
    }
    __syncthreads();
    float* obase = joined + (size_t)n * 81 * plane;
    for (int idx = threadIdx.x; idx < 81 * (PX / 4); idx += NTH) {
      const int d = idx / (PX / 4), sp = idx % (PX / 4), rr = sp / STRIPS, st = sp % STRIPS;
      const int hh = h0 + rr, ww = w0 + 4 * st;
      if (hh < H && ww < W) {
        float4 v = *reinterpret_cast<const float4*>(&acc[d * PX + 4 * sp]);
        const float4 sc = *reinterpret_cast<const float4*>(&scl[4 * sp]);
        v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w;
        *reinterpret_cast<float4*>(obase + (size_t)d * plane + (size_t)hh * W + ww) = v;
      }
    }
  }
}

// (The fp32-matrix-pipe formulation of this forward -- exact, measured slower: 166-171 vs 139 us, profiles/r02_corr_mfma_*.txt,
// r03_corr_f16_ablation.txt -- lives in tools/experiments/matrix_pipe_corr/, outside the product library.)

constexpr int kPipeTW = 32;        // tile width of the pipelined kernel
constexpr int kSmallTH = 8;        // its tile height for all but the largest maps (and of the tiny maps' tickets)

// One launch of the pipelined kernel over `ntiles` tiles of TH x 32 pixels.  A plain launch leaves the last four fields alone:
// every workgroup walks all C channels, in the XCD-local tile order.  launch_corr9_split sets `slices` > 1: workgroup (b, y)
// walks the y-th of `slices` channel slices and stores at out + y part_stride (tile order as dispatched: a handful of tiles).
struct Pipe2Launch {
  const float *in1, *in2;
  float* out;
  int C, H, W;
  int tilesX;                      // tile columns (PAIR: the full ones)
  long ntiles, nreg;               // tiles in all; PAIR: the regular ones among them
  int slices = 1;
  long part_stride = 0;
  float* joined = nullptr;
  unsigned* tickets = nullptr;
};

template <int TH, bool FUSE, int NTILE, bool KSPLIT = false, bool PAIR = false, bool JOIN = false>
static int launch_pipe2(const Pipe2Launch& a, hipStream_t st) {
  if (a.ntiles <= 0 || a.ntiles > 0x7fffffffL) return fail(RFN_EINVAL, "corr9: grid too large");
  const long blocks = KSPLIT ? a.ntiles : cdiv(a.ntiles, (long)NTILE);
  hipLaunchKernelGGL((corr9_pipe2_kernel<TH, kPipeTW, FUSE, NTILE, KSPLIT, PAIR, JOIN>), dim3((unsigned)blocks, (unsigned)a.slices),
                     dim3(pipe2_threads(TH, kPipeTW, NTILE)), 0, st, a.in1, a.in2, a.out, a.C / a.slices, a.H, a.W, a.tilesX,
                     cdiv(a.H, TH), (int)a.ntiles, a.slices == 1 ? 1 : 0, (int)a.nreg, a.C, a.part_stride, a.joined, a.tickets);
  return check_launch("corr9_pipe2_kernel");
}

template <bool FUSE, bool WARP>
static int launch_corr9(const float* in1, const float* in2, const float* flow, float* out, int B, int C, int H,
                        int W, hipStream_t st) {
  // 1. The pipelined kernel takes W % 4 == 0 (16-byte DMA pieces), C a multiple of the ring's 4 stages x 2 channels, and --
  //    its DMA offsets are 32-bit within a sample (a sample PAIR for edge tiles) -- samples below 4 GB.
  const size_t sample = (size_t)C * H * W * sizeof(float);
  if (!WARP && (W & 3) == 0 && (C % 8) == 0 && C >= 16 && sample < (1ull << 32)) {
    // 2. The geometry: 16 x 32 tile pairs / paired edge tiles / at most one tile per CU / otherwise (chosen under 4).
    const int cols = cdiv(W, kPipeTW), rows8 = cdiv(H, kSmallTH), rem = W % kPipeTW;
    const long nt16 = (long)B * cols * cdiv(H, 16), pairs16 = (nt16 + 1) / 2, nt8 = (long)B * cols * rows8;
    const long nreg = (long)B * (W / kPipeTW) * rows8, npair = nreg + (long)(B / 2) * rows8;
    const bool ksplit_ok = C >= 32 && C % 16 == 0;       // whole ring rounds for each of two wave groups
    // 3. Two or four wave groups on a tile's channels: four when each gets whole ring rounds (twelve waves per CU walk 9.2
    //    wave-chunks / us against 7.1 with six: level 2 64 -> ~50 us).
    const bool four = C >= 64 && C % 32 == 0;
    // 4. One call.
    Pipe2Launch a{in1, in2, out, C, H, W, cols, nt8, 0};
    if (pairs16 >= 192) {
      // level 1 (2 x 270 x 480) and larger: two 16 x 32 tiles per 12-wave workgroup, three waves per SIMD
      a.ntiles = nt16;
      return launch_pipe2<16, FUSE, 2>(a, st);
    }
    if (ksplit_ok && nt8 > 256 && rem > 0 && rem <= 16 && B % 2 == 0 && npair <= 256 && 2 * sample < (1ull << 32)) {
      // more than 256 8 x 32 tiles only because the width leaves at most half a tile column over: image pairs share that band
      // when that brings the map to one workgroup per CU (level 2, 2 x 135 x 240: 272 -> 255 tiles, 83 -> 64 us)
      a.tilesX = W / kPipeTW, a.ntiles = npair, a.nreg = nreg;
      if (four) return launch_pipe2<kSmallTH, FUSE, 4, true, true>(a, st);
      return launch_pipe2<kSmallTH, FUSE, 2, true, true>(a, st);
    }
    if (ksplit_ok && nt8 <= 256) {
      // at most one 8 x 32 tile per CU: the workgroup's wave groups split the channels (256 tiles 64.5 -> 54.7 us with two,
      // profiles/r04_corr_ksplit.txt)
      if (four) return launch_pipe2<kSmallTH, FUSE, 4, true>(a, st);
      return launch_pipe2<kSmallTH, FUSE, 2, true>(a, st);
    }
    return launch_pipe2<kSmallTH, FUSE, 1>(a, st);      // 8 x 32 tiles, one 3-wave workgroup each
  }
  // Anything else: the register-staged kernel.
  const int tilesX = cdiv(W, kTW), tilesY = cdiv(H, kTH);
  const long blocks = (long)B * tilesX * tilesY;
  if (blocks <= 0 || blocks > 0x7fffffffL) return fail(RFN_EINVAL, "corr9: grid too large");
  hipLaunchKernelGGL((corr9_tile_kernel<FUSE, WARP>), dim3((unsigned)blocks), dim3(kTH * kStrips * 3), 0, st, in1, in2, flow,
                     out, C, H, W, tilesX, tilesY);
  return check_launch("corr9_tile_kernel");
}

// --------------------------------------------------------------------------------------------------------
// Channel split for small maps.  The tiled kernels walk the C channels of a tile serially: a 2 x 256 x 32 x 32 level
// is 8 tiles = 8 workgroups on 256 CUs and takes the same ~100 us as the 2 x 128 x 270 x 480 level (pure latency:
// 64 chunk hand-offs of ~1.5 us).  Here S workgroups share a tile, each over C / S channels, writing raw partial sums
// to a workspace (S, B, 81, H, W); the reduce kernel adds them in chunk order (deterministic) and applies the fused
// ReLU + L2-norm epilogue of the one-kernel path.
// --------------------------------------------------------------------------------------------------------
// 32 pixels x 8 shift lanes per workgroup: lane (px, k) adds the S partials of shifts k, k+8, ... (coalesced over the
// pixels) into an LDS tile [81][32]; three lanes per pixel then take the squares of the three vertical-shift groups in
// the one-kernel epilogue's order, and everybody scales and stores.
__global__ __launch_bounds__(256) void corr9_split_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                                 int S, long part_stride, long plane, long total) {
  __shared__ float tile[81][33];
  __shared__ float ssq[3][32];
  const int px = threadIdx.x & 31, k = threadIdx.x >> 5;
  const long idx = (long)blockIdx.x * 32 + px;                   // (n, pixel)
  const bool ok = idx < total;
  const long n = ok ? idx / plane : 0, pix = ok ? idx % plane : 0;
  const float* p = part + n * 81 * plane + pix;
  for (int d = k; d < 81; d += 8) {
    float v = 0.0f;
    if (ok) {
      // chunk order, four loads in flight at a time (the adds stay sequential: same sum for every launch geometry)
      const float* q = p + (long)d * plane;
      v = q[0];
      int s = 1;
      for (; s + 3 < S; s += 4) {
        const float t0 = q[(long)s * part_stride], t1 = q[(long)(s + 1) * part_stride];
        const float t2 = q[(long)(s + 2) * part_stride], t3 = q[(long)(s + 3) * part_stride];
        v = (((v + t0) + t1) + t2) + t3;
      }
      for (; s < S; ++s) v += q[(long)s * part_stride];
    }
    tile[d][px] = fmaxf(v, 0.0f);
  }
  __syncthreads();
  if (k < 3) {
    float ss = 0.0f;
#pragma unroll
    for (int d = 0; d < 27; ++d) {
      const float r = tile[k * 27 + d][px];
      ss = fmaf(r, r, ss);
    }
    ssq[k][px] = ss;
  }
  __syncthreads();
  const float scale = 1.0f / fmaxf(sqrtf(ssq[0][px] + ssq[1][px] + ssq[2][px]), 1e-12f);
  if (ok) {
    float* o = out + n * 81 * plane + pix;
    for (int d = k; d < 81; d += 8) o[(long)d * plane] = tile[d][px] * scale;
  }
}

static int launch_corr9_split(const float* in1, const float* in2, float* out, float* workspace, int B, int C, int H, int W,
                              int S, hipStream_t st) {
  const int Cc = C / S;                                  // channels per slice (the caller checks: a multiple of 8)
  if ((size_t)C * H * W * sizeof(float) >= (1ull << 32))
    return fail(RFN_EINVAL, "corr9 split: samples of 4 GB and more are not tiny maps");
  const long plane = (long)H * W, part_stride = (long)B * 81 * plane;
  Pipe2Launch a{in1, in2, workspace, C, H, W, cdiv(W, kPipeTW), (long)B * cdiv(W, kPipeTW) * cdiv(H, kSmallTH), 0, S, part_stride};
  if (Cc >= 64 && Cc % 32 == 0 && (W & 3) == 0) {
    // ONE launch: four wave groups per workgroup on the quarters of its slice, the tile's last workgroup joins the slices.
    // Tickets: the ntiles unsigned ints behind the partial volumes (rfn_local_corr_layer_split_workspace_bytes).
    a.joined = out;
    a.tickets = reinterpret_cast<unsigned*>(workspace + (size_t)S * part_stride);
    return launch_pipe2<kSmallTH, false, 4, true, false, true>(a, st);
  }
  // two launches: raw partial volumes from one wave group per slice (whole rounds of the ring: Cc % 8 == 0), then the reduce
  if (int rc = launch_pipe2<kSmallTH, false, 1>(a, st)) return rc;
  const long total = (long)B * plane;
  hipLaunchKernelGGL(corr9_split_reduce_kernel, dim3(cdiv(total, 32)), dim3(256), 0, st, workspace, out, S, part_stride, plane,
                     total);
  return check_launch("corr9_split_reduce_kernel");
}

// --------------------------------------------------------------------------------------------------------
// Generic forward: any kernel/patch/stride/pad/dilation, one thread per output element (coalesced along w).
// --------------------------------------------------------------------------------------------------------
struct CorrParams {
  int B, C, iH, iW, oH, oW, kH, kW, patchH, patchW, padH, padW, dilH, dilW, dpH, dpW, dH, dW;
};

// accumulation type: the element type itself for float / double (the CPU reference's `scalar_t` sums, bit for bit), fp32
// for half (the CUDA reference dispatches half too, correlation_cuda_kernel.cu:267; its sums are warp-shuffled partials in
// half -- here every product is formed and summed in fp32 and the result is rounded once)
template <typename T> struct CorrAcc { using type = T; };
template <> struct CorrAcc<__half> { using type = float; };

template <typename T>
__global__ __launch_bounds__(256) void corr_generic_fwd_kernel(const T* __restrict__ in1,
                                                               const T* __restrict__ in2, T* __restrict__ out,
                                                               CorrParams p, long total) {
  using A = typename CorrAcc<T>::type;
  const int radH = (p.patchH - 1) / 2, radW = (p.patchW - 1) / 2;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    long t = idx;
    const int w = t % p.oW; t /= p.oW;
    const int h = t % p.oH; t /= p.oH;
    const int pw = t % p.patchW; t /= p.patchW;
    const int ph = t % p.patchH;
    const int n = t / p.patchH;
    const int u = -p.padH + h * p.dH, v = -p.padW + w * p.dW;
    const int sU = (ph - radH) * p.dpH, sV = (pw - radW) * p.dpW;
    const size_t plane = (size_t)p.iH * p.iW;
    const T* a = in1 + (size_t)n * p.C * plane;
    const T* b = in2 + (size_t)n * p.C * plane;
    A acc = 0;
    for (int c = 0; c < p.C; ++c) {
      for (int i = 0; i < p.kH; ++i) {
        const int i1 = u + i * p.dilH, i2 = i1 + sU;
        if (i1 < 0 || i1 >= p.iH || i2 < 0 || i2 >= p.iH) continue;
        for (int jj = 0; jj < p.kW; ++jj) {
          const int j1 = v + jj * p.dilW, j2 = j1 + sV;
          if (j1 < 0 || j1 >= p.iW || j2 < 0 || j2 >= p.iW) continue;
          acc += (A)a[c * plane + (size_t)i1 * p.iW + j1] * (A)b[c * plane + (size_t)i2 * p.iW + j2];
        }
      }
    }
    out[idx] = (T)acc;
  }
}

// --------------------------------------------------------------------------------------------------------
// Backward, gather form for kernel 1 / stride 1 / pad 0 (deterministic): one thread per (n,c,h,w).
//   g1[n,c,h,w] = sum_{ph,pw} gout[n,ph,pw,h,w]       * in2[n,c,h+sU,w+sV]
//   g2[n,c,y,x] = sum_{ph,pw} gout[n,ph,pw,y-sU,x-sV] * in1[n,c,y-sU,x-sV]
// --------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void corr_k1_bwd_kernel(const T* __restrict__ in1, const T* __restrict__ in2,
                                                          const T* __restrict__ gout, T* __restrict__ g1,
                                                          T* __restrict__ g2, CorrParams p, long total) {
  const int radH = (p.patchH - 1) / 2, radW = (p.patchW - 1) / 2;
  const size_t plane = (size_t)p.iH * p.iW;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    long t = idx;
    const int w = t % p.iW; t /= p.iW;
    const int h = t % p.iH; t /= p.iH;
    const int c = t % p.C;
    const int n = t / p.C;
    const T* a = in1 + ((size_t)n * p.C + c) * plane;
    const T* b = in2 + ((size_t)n * p.C + c) * plane;
    const T* go = gout + (size_t)n * p.patchH * p.patchW * plane;
    T s1 = 0, s2 = 0;
    for (int ph = 0; ph < p.patchH; ++ph) {
      const int sU = (ph - radH) * p.dpH;
      for (int pw = 0; pw < p.patchW; ++pw) {
        const int sV = (pw - radW) * p.dpW;
        const T* gp = go + (size_t)(ph * p.patchW + pw) * plane;
        const int y2 = h + sU, x2 = w + sV;
        if (y2 >= 0 && y2 < p.iH && x2 >= 0 && x2 < p.iW) s1 += gp[(size_t)h * p.iW + w] * b[(size_t)y2 * p.iW + x2];
        const int y1 = h - sU, x1 = w - sV;
        if (y1 >= 0 && y1 < p.iH && x1 >= 0 && x1 < p.iW)
          s2 += gp[(size_t)y1 * p.iW + x1] * a[(size_t)y1 * p.iW + x1];
      }
    }
    g1[idx] = s1;
    g2[idx] = s2;
  }
}

// --------------------------------------------------------------------------------------------------------
// Backward for the hot parameterisation (patch 9, kernel 1, stride 1, pad 0), f32: LDS-tiled gather.
//   MODE 1: g1[n,c,q] = sum_d gout[n,d,q]     * in2[n,c,q+d]      (weights at q, taps forward)
//   MODE 2: g2[n,c,q] = sum_d gout[n,d,q-d]   * in1[n,c,q-d]      (weights and taps mirrored)
// The 81 weights of an output pixel do not depend on the channel: a thread owns ONE pixel, gathers its 81 weights into
// registers once and then walks the channels; per channel chunk the (8+8) x (32+8) halo tile of the other input is
// staged in LDS and every FMA costs one conflict-free ds_read_b32 (lanes = consecutive pixels).  Deterministic.
// --------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void corr9_bwd_tile_kernel(const float* __restrict__ other,
                                                             const float* __restrict__ gout,
                                                             float* __restrict__ grad, int C, int H, int W,
                                                             int tilesX, int tilesY) {
  constexpr int TH = 8, TW = 32, CC = 8, RH = TH + 8, RW = TW + 8;
  __shared__ float tile[CC][RH][RW + 1];
  const TileId id = decode_tile(blockIdx.x, tilesX, tilesY);
  const int n = id.n, h0 = id.ty * TH, w0 = id.tx * TW;
  const int lx = threadIdx.x % TW, ly = threadIdx.x / TW;
  const int qy = h0 + ly, qx = w0 + lx;
  const bool inq = qy < H && qx < W;
  const size_t plane = (size_t)H * W;
  // my 81 weights
  float wgt[81];
  const float* go = gout + (size_t)n * 81 * plane;
#pragma unroll
  for (int dy = 0; dy < 9; ++dy)
#pragma unroll
    for (int dx = 0; dx < 9; ++dx) {
      const int d = dy * 9 + dx;
      float v = 0.0f;
      if (MODE == 1) {
        if (inq) v = go[(size_t)d * plane + (size_t)qy * W + qx];
      } else {
        const int py = qy - (dy - 4), px = qx - (dx - 4);
        if (inq && py >= 0 && py < H && px >= 0 && px < W) v = go[(size_t)d * plane + (size_t)py * W + px];
      }
      wgt[d] = v;
    }
  const float* src = other + (size_t)n * C * plane;
  float* dst = grad + (size_t)n * C * plane;
  for (int c0 = 0; c0 < C; c0 += CC) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < CC * RH * RW; idx += 256) {
      const int x = idx % RW, r = (idx / RW) % RH, c = idx / (RW * RH);
      const int gy = h0 - 4 + r, gx = w0 - 4 + x;
      float v = 0.0f;
      if (c0 + c < C && gy >= 0 && gy < H && gx >= 0 && gx < W) v = src[(size_t)(c0 + c) * plane + (size_t)gy * W + gx];
      tile[c][r][x] = v;
    }
    __syncthreads();
#pragma unroll 2
    for (int c = 0; c < CC; ++c) {
      float acc = 0.0f;
#pragma unroll
      for (int dy = 0; dy < 9; ++dy)
#pragma unroll
        for (int dx = 0; dx < 9; ++dx) {
          // tile origin is (h0-4, w0-4): pixel q sits at [ly+4][lx+4]; MODE 1 taps q+d, MODE 2 taps q-d
          const int r = (MODE == 1) ? ly + dy : ly + 8 - dy;
          const int x = (MODE == 1) ? lx + dx : lx + 8 - dx;
          acc = fmaf(wgt[dy * 9 + dx], tile[c][r][x], acc);
        }
      if (inq && c0 + c < C) dst[(size_t)(c0 + c) * plane + (size_t)qy * W + qx] = acc;
    }
  }
}

// The same gather on register STRIPS, laid out like the forward.  A thread owns 4 adjacent pixels of a row and the
// weights of THREE vertical shifts (27 shifts x 4 pixels = 108 registers); the three wave groups of a 192-thread workgroup split
// the nine vertical shifts of an 8 x 32 tile.  Per channel and vertical shift a thread reads its 12 row values as three
// ds_read_b128 and does 36 FMAs (the one-pixel kernel above: one ds_read_b32 per FMA -- LDS-bound); the groups' partial sums of
// a chunk of 8 channels meet in LDS (group 0 adds groups 1, 2 in that order: deterministic) and leave as 16-byte stores.  The
// next chunk's halo tile is in flight to registers while a chunk is computed (double-buffered LDS, ONE barrier per chunk).
// Both gradients in ONE launch (blockIdx.y).  W % 4 == 0, C % 8 == 0; anything else takes the one-pixel kernel.
// Level 1 (2 x 128 x 270 x 480, both gradients): 997 us in two launches of the one-pixel kernel, 308 us here = 0.25 of 8 TB/s
// on 615 MB (profiles/r05_corr_backward.txt; the steps in between: DESIGN.md section 4).
template <int MODE>
__device__ __forceinline__ void corr9_bwd_strip_body(const float* __restrict__ other, const float* __restrict__ gout,
                                                     float* __restrict__ grad, int C, int H, int W, int tilesX, int tilesY,
                                                     float* lds) {
  constexpr int TH = 8, TW = 32, CC = 8, RH = TH + 8, P4 = (TW + 8) / 4, NT = 192;
  constexpr int CHUNK4 = CC * RH * P4;                   // float4 pieces of a chunk's halo tile
  constexpr int NPF = (CHUNK4 + NT - 1) / NT;            // pieces a thread carries
  float4* tile = reinterpret_cast<float4*>(lds);                                  // [2][CC][RH][P4]
  constexpr int RP = 10;                                  // slots per row of the exchange buffer (same banking argument)
  float4* red = reinterpret_cast<float4*>(lds) + 2 * CHUNK4;                      // [2][2][CC][TH][RP]
  const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
  // lane -> (row, strip): ds_read_b128 is serviced in four groups of 16 lanes (quads {0,3,5,6}, {1,2,4,7} of each half wave),
  // and a group must touch 16 distinct 16-byte slots of the 256-byte bank row.  With rows of 10 slots the half rows start at
  // slot (10 r + 4 h) mod 16; the quads of a group get {(0,0),(0,1),(2,1),(4,1)}, {(2,0),(4,0),(6,0),(6,1)} and the same on the
  // odd rows -- start slots {0,4,8,12} + const for every vertical shift, channel and read of a row: conflict-free.
  const int quad = lane >> 2, q7 = quad & 7;
  const int ly = 2 * ((0x32130210u >> (4 * q7)) & 3) + (quad >> 3);
  const int strip = 4 * ((0xE8u >> q7) & 1) + (lane & 3);
  const TileId id = decode_tile(xcd_local_order(blockIdx.x, gridDim.x), tilesX, tilesY);
  const int n = id.n, h0 = id.ty * TH, w0 = id.tx * TW;
  const int qy = h0 + ly, qx0 = w0 + 4 * strip;
  const bool inq = qy < H && qx0 < W;                    // W % 4 == 0: a strip is all in or all out
  const size_t plane = (size_t)H * W;
  const float* go = gout + (size_t)n * 81 * plane;
  // Weights as REGISTER PAIRS for v_pk_fma_f32 (64-bit operands are even-aligned register pairs): a tap at an EVEN offset into the
  // 12 row values pairs pixels (0, 1) and (2, 3) with the natural halves of the three 16-byte reads; at an ODD offset pixels
  // (1, 2) pair up and pixels 0 and 3 go as single FMAs -- 22 VALU instructions per 36 FMAs, no register shuffling, no
  // unaligned LDS reads (the compiler's own pairing of a plain float loop: ~19 moves + 8 small LDS reads per row).
  f32x2 we[3][5][2];                                     // even horizontal shifts 0, 2, ..., 8: pixels (0, 1), (2, 3)
  f32x2 wo[3][4];                                        // odd shifts 1, 3, 5, 7: pixels (1, 2)
  float wo0[3][4], wo3[3][4];                            //                        pixels 0 and 3
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int dy = 3 * grp + a;
#pragma unroll
    for (int dx = 0; dx < 9; ++dx) {
      const int d = dy * 9 + dx;
      float wv[4];
      if (MODE == 1) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (inq) v = *reinterpret_cast<const float4*>(go + (size_t)d * plane + (size_t)qy * W + qx0);
        wv[0] = v.x; wv[1] = v.y; wv[2] = v.z; wv[3] = v.w;
      } else {
        const int py = qy - (dy - 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int px = qx0 + i - (dx - 4);
          wv[i] = (inq && py >= 0 && py < H && px >= 0 && px < W) ? go[(size_t)d * plane + (size_t)py * W + px] : 0.0f;
        }
      }
      if (dx % 2 == 0) {
        we[a][dx / 2][0] = f32x2{wv[0], wv[1]};
        we[a][dx / 2][1] = f32x2{wv[2], wv[3]};
      } else {
        wo[a][dx / 2] = f32x2{wv[1], wv[2]};
        wo0[a][dx / 2] = wv[0];
        wo3[a][dx / 2] = wv[3];
      }
    }
  }
  const float* src = other + (size_t)n * C * plane;
  float* dst = grad + (size_t)n * C * plane;
  // this thread's pieces of a chunk's halo tile: (channel, row, 16-byte column) -- the same for every chunk
  int poff[NPF];                                         // offset of the piece within a channel chunk, or -1 (outside the image)
#pragma unroll
  for (int k = 0; k < NPF; ++k) {
    const int idx = tid + NT * k;
    const int x4 = idx % P4, r = (idx / P4) % RH, c = idx / (P4 * RH);
    const int gy = h0 - 4 + r, gx = w0 - 4 + 4 * x4;
    poff[k] = (idx < CHUNK4 && gy >= 0 && gy < H && gx >= 0 && gx < W) ? (int)((size_t)c * plane + (size_t)gy * W + gx) : -1;
  }
  float4 pf[NPF];
  auto fetch = [&](int c0) {
    const float* s0 = src + (size_t)c0 * plane;
#pragma unroll
    for (int k = 0; k < NPF; ++k)
      pf[k] = poff[k] >= 0 ? *reinterpret_cast<const float4*>(s0 + poff[k]) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int k = 0; k < NPF; ++k)
      if (tid + NT * k < CHUNK4) tile[buf * CHUNK4 + tid + NT * k] = pf[k];
  };
  fetch(0);
  stage(0);
  __syncthreads();
  const int nchunks = C / CC;
  for (int kc = 0; kc < nchunks; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nchunks) fetch((kc + 1) * CC);
    float4 part[CC];
    const float4* tb = tile + buf * CHUNK4;
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      f32x2 e01 = {0.f, 0.f}, e23 = {0.f, 0.f}, o12 = {0.f, 0.f};
      float o0 = 0.f, o3 = 0.f;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int dy = 3 * grp + a;
        const int r = (MODE == 1) ? ly + dy : ly + 8 - dy;
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f* rowp = reinterpret_cast<const v4f*>(tb + (c * RH + r) * P4 + strip);
        const v4f q0 = rowp[0], q1 = rowp[1], q2 = rowp[2];
        const f32x2 v2[6] = {f32x2{q0[0], q0[1]}, f32x2{q0[2], q0[3]}, f32x2{q1[0], q1[1]},
                             f32x2{q1[2], q1[3]}, f32x2{q2[0], q2[1]}, f32x2{q2[2], q2[3]}};
        const float v1[12] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3], q2[0], q2[1], q2[2], q2[3]};
#pragma unroll
        for (int dx = 0; dx < 9; ++dx) {
          const int o = (MODE == 1) ? dx : 8 - dx;       // pixel i reads row value i + o (same parity as dx)
          if (dx % 2 == 0) {
            e01 = __builtin_elementwise_fma(we[a][dx / 2][0], v2[o / 2], e01);
            e23 = __builtin_elementwise_fma(we[a][dx / 2][1], v2[o / 2 + 1], e23);
          } else {
            o12 = __builtin_elementwise_fma(wo[a][dx / 2], v2[(o + 1) / 2], o12);
            o0 = fmaf(wo0[a][dx / 2], v1[o], o0);
            o3 = fmaf(wo3[a][dx / 2], v1[o + 3], o3);
          }
        }
      }
      part[c] = make_float4(e01[0] + o0, e01[1] + o12[0], e23[0] + o12[1], e23[1] + o3);
    }
    float4* rb = red + buf * (2 * CC * TH * RP);
    if (grp != 0) {
#pragma unroll
      for (int c = 0; c < CC; ++c) rb[((grp - 1) * CC + c) * (TH * RP) + ly * RP + strip] = part[c];
    }
    if (kc + 1 < nchunks) stage(buf ^ 1);
    __syncthreads();
    if (grp == 0 && inq) {
      float* d0 = dst + (size_t)(kc * CC) * plane + (size_t)qy * W + qx0;
#pragma unroll
      for (int c = 0; c < CC; ++c) {
        const float4 p1 = rb[(0 * CC + c) * (TH * RP) + ly * RP + strip];
        const float4 p2 = rb[(1 * CC + c) * (TH * RP) + ly * RP + strip];
        float4 o;
        o.x = (part[c].x + p1.x) + p2.x;
        o.y = (part[c].y + p1.y) + p2.y;
        o.z = (part[c].z + p1.z) + p2.z;
        o.w = (part[c].w + p1.w) + p2.w;
        *reinterpret_cast<float4*>(d0 + (size_t)c * plane) = o;
      }
    }
  }
}

__global__ __launch_bounds__(192) void corr9_bwd_strip_kernel(const float* __restrict__ in1, const float* __restrict__ in2,
                                                              const float* __restrict__ gout, float* __restrict__ g1,
                                                              float* __restrict__ g2, int C, int H, int W, int tilesX,
                                                              int tilesY) {
  __shared__ __attribute__((aligned(16))) float lds[2 * 8 * 16 * 40 + 2 * 2 * 8 * 8 * 40];
  if (blockIdx.y == 0) corr9_bwd_strip_body<1>(in2, gout, g1, C, H, W, tilesX, tilesY, lds);
  else corr9_bwd_strip_body<2>(in1, gout, g2, C, H, W, tilesX, tilesY, lds);
}

// Generic backward: scatter with hardware atomics, one thread per gout element (grads pre-zeroed by the caller).
template <typename T>
__global__ __launch_bounds__(256) void corr_generic_bwd_kernel(const T* __restrict__ in1,
                                                               const T* __restrict__ in2,
                                                               const T* __restrict__ gout, T* __restrict__ g1,
                                                               T* __restrict__ g2, CorrParams p, long total) {
  const int radH = (p.patchH - 1) / 2, radW = (p.patchW - 1) / 2;
  const size_t plane = (size_t)p.iH * p.iW;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    long t = idx;
    const int w = t % p.oW; t /= p.oW;
    const int h = t % p.oH; t /= p.oH;
    const int pw = t % p.patchW; t /= p.patchW;
    const int ph = t % p.patchH;
    const int n = t / p.patchH;
    const T g = gout[idx];
    const int u = -p.padH + h * p.dH, v = -p.padW + w * p.dW;
    const int sU = (ph - radH) * p.dpH, sV = (pw - radW) * p.dpW;
    const T* a = in1 + (size_t)n * p.C * plane;
    const T* b = in2 + (size_t)n * p.C * plane;
    T* ga = g1 + (size_t)n * p.C * plane;
    T* gb = g2 + (size_t)n * p.C * plane;
    for (int i = 0; i < p.kH; ++i) {
      const int i1 = u + i * p.dilH, i2 = i1 + sU;
      if (i1 < 0 || i1 >= p.iH || i2 < 0 || i2 >= p.iH) continue;
      for (int jj = 0; jj < p.kW; ++jj) {
        const int j1 = v + jj * p.dilW, j2 = j1 + sV;
        if (j1 < 0 || j1 >= p.iW || j2 < 0 || j2 >= p.iW) continue;
        const size_t o1 = (size_t)i1 * p.iW + j1, o2 = (size_t)i2 * p.iW + j2;
        for (int c = 0; c < p.C; ++c) {
          atomicAdd(&gb[c * plane + o2], g * a[c * plane + o1]);
          atomicAdd(&ga[c * plane + o1], g * b[c * plane + o2]);
        }
      }
    }
  }
}

// Generic backward, GATHER form (deterministic, any parameterisation): one thread per (n, c, y, x) collects, for every
// patch offset and kernel tap, the output position that touched this pixel -- h = (y + pad - i dil) / stride when that
// division is exact and in range (correlation.cpp:131-183 read from the gradient's side).  Sums in CorrAcc<T>, one rounding.
// Used for half, where the scatter kernel above would need 16-bit atomics and round after every add.
template <typename T>
__global__ __launch_bounds__(256) void corr_generic_bwd_gather_kernel(const T* __restrict__ in1, const T* __restrict__ in2,
                                                                      const T* __restrict__ gout, T* __restrict__ g1,
                                                                      T* __restrict__ g2, CorrParams p, long total) {
  using A = typename CorrAcc<T>::type;
  const int radH = (p.patchH - 1) / 2, radW = (p.patchW - 1) / 2;
  const size_t plane = (size_t)p.iH * p.iW, oplane = (size_t)p.oH * p.oW;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    long t = idx;
    const int x = t % p.iW; t /= p.iW;
    const int y = t % p.iH; t /= p.iH;
    const int c = t % p.C;
    const int n = t / p.C;
    const T* a = in1 + ((size_t)n * p.C + c) * plane;
    const T* b = in2 + ((size_t)n * p.C + c) * plane;
    const T* go = gout + (size_t)n * p.patchH * p.patchW * oplane;
    A s1 = 0, s2 = 0;
    for (int ph = 0; ph < p.patchH; ++ph) {
      const int sU = (ph - radH) * p.dpH;
      for (int pw = 0; pw < p.patchW; ++pw) {
        const int sV = (pw - radW) * p.dpW;
        const T* gp = go + (size_t)(ph * p.patchW + pw) * oplane;
        for (int i = 0; i < p.kH; ++i) {
          // g1: this pixel is input1's tap (i1 = y); its partner in input2 is (y + sU)
          const int hn = y + p.padH - i * p.dilH;
          const bool hok = hn >= 0 && hn % p.dH == 0 && hn / p.dH < p.oH;
          // g2: this pixel is input2's tap (i2 = y), so i1 = y - sU
          const int y1 = y - sU, hn2 = y1 + p.padH - i * p.dilH;
          const bool hok2 = y1 >= 0 && y1 < p.iH && hn2 >= 0 && hn2 % p.dH == 0 && hn2 / p.dH < p.oH;
          if (!hok && !hok2) continue;
          for (int jj = 0; jj < p.kW; ++jj) {
            if (hok) {
              const int wn = x + p.padW - jj * p.dilW;
              const int y2 = y + sU, x2 = x + sV;
              if (wn >= 0 && wn % p.dW == 0 && wn / p.dW < p.oW && y2 >= 0 && y2 < p.iH && x2 >= 0 && x2 < p.iW)
                s1 += (A)gp[(size_t)(hn / p.dH) * p.oW + wn / p.dW] * (A)b[(size_t)y2 * p.iW + x2];
            }
            if (hok2) {
              const int x1 = x - sV, wn2 = x1 + p.padW - jj * p.dilW;
              if (x1 >= 0 && x1 < p.iW && wn2 >= 0 && wn2 % p.dW == 0 && wn2 / p.dW < p.oW)
                s2 += (A)gp[(size_t)(hn2 / p.dH) * p.oW + wn2 / p.dW] * (A)a[(size_t)y1 * p.iW + x1];
            }
          }
        }
      }
    }
    g1[idx] = (T)s1;
    g2[idx] = (T)s2;
  }
}

static int fill_params(CorrParams& p, int B, int C, int iH, int iW, int kH, int kW, int patchH, int patchW,
                       int padH, int padW, int dilH, int dilW, int dpH, int dpW, int dH, int dW) {
  if (B <= 0 || C <= 0 || iH <= 0 || iW <= 0) return fail(RFN_EINVAL, "corr: non-positive tensor size");
  if (kH <= 0 || kW <= 0 || patchH <= 0 || patchW <= 0 || dH <= 0 || dW <= 0 || dilH <= 0 || dilW <= 0 ||
      dpH <= 0 || dpW <= 0 || padH < 0 || padW < 0)
    return fail(RFN_EINVAL, "corr: invalid kernel/patch/stride/dilation/padding");
  p = {B, C, iH, iW, 0, 0, kH, kW, patchH, patchW, padH, padW, dilH, dilW, dpH, dpW, dH, dW};
  p.oH = (iH + 2 * padH - ((kH - 1) * dilH + 1)) / dH + 1;
  p.oW = (iW + 2 * padW - ((kW - 1) * dilW + 1)) / dW + 1;
  if (p.oH <= 0 || p.oW <= 0) return fail(RFN_EINVAL, "corr: empty output (%d x %d)", p.oH, p.oW);
  return RFN_OK;
}

static inline bool is_hot_param(const CorrParams& p) {
  return p.kH == 1 && p.kW == 1 && p.patchH == 9 && p.patchW == 9 && p.padH == 0 && p.padW == 0 && p.dH == 1 &&
         p.dW == 1 && p.dpH == 1 && p.dpW == 1;
}
static inline bool is_k1(const CorrParams& p) {
  return p.kH == 1 && p.kW == 1 && p.padH == 0 && p.padW == 0 && p.dH == 1 && p.dW == 1;
}

// grid of the one-thread-per-element kernels (grid-stride loops)
static inline int flat_grid(long total) { return (int)std::min<long>(cdiv(total, 256), 256L * 32); }

// Backward of the hot parameterisation, f32: the strip kernel, or the one-pixel kernel once per gradient.
static int corr9_bwd_f32(const float* in1, const float* in2, const float* gout, float* g1, float* g2, const CorrParams& p,
                         hipStream_t st) {
  const int tilesX = cdiv(p.iW, 32), tilesY = cdiv(p.iH, 8);
  const long blocks = (long)p.B * tilesX * tilesY;
  if (blocks > 0x7fffffffL) return fail(RFN_EINVAL, "corr bwd: grid too large");
  if (p.iW % 4 == 0 && p.C % 8 == 0 && (size_t)p.C * p.iH * p.iW < (1ull << 31) &&
      (((size_t)in1 | (size_t)in2 | (size_t)gout | (size_t)g1 | (size_t)g2) & 15) == 0) {
    hipLaunchKernelGGL(corr9_bwd_strip_kernel, dim3((unsigned)blocks, 2), dim3(192), 0, st, in1, in2, gout, g1, g2, p.C, p.iH,
                       p.iW, tilesX, tilesY);
    return check_launch("corr9_bwd_strip_kernel");
  }
  hipLaunchKernelGGL((corr9_bwd_tile_kernel<1>), dim3((unsigned)blocks), dim3(256), 0, st, in2, gout, g1, p.C, p.iH, p.iW,
                     tilesX, tilesY);
  if (int rc = check_launch("corr9_bwd_tile_kernel<1>")) return rc;
  hipLaunchKernelGGL((corr9_bwd_tile_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, st, in1, gout, g2, p.C, p.iH, p.iW,
                     tilesX, tilesY);
  return check_launch("corr9_bwd_tile_kernel<2>");
}

// Dispatch, by type at compile time and by parameterisation at run time.
// Forward: the hot parameterisation in f32 -> launch_corr9 (NOT the generic kernel: a caller that wants that one launches it
// itself); anything else -> corr_generic_fwd_kernel.
template <typename T>
static int corr_fwd_any(const T* in1, const T* in2, T* out, const CorrParams& p, hipStream_t st) {
  if constexpr (std::is_same<T, float>::value) {
    if (is_hot_param(p)) return launch_corr9<false, false>(in1, in2, nullptr, out, p.B, p.C, p.iH, p.iW, st);
  }
  const long total = (long)p.B * p.patchH * p.patchW * p.oH * p.oW;
  hipLaunchKernelGGL((corr_generic_fwd_kernel<T>), dim3(flat_grid(total)), dim3(256), 0, st, in1, in2, out, p, total);
  return check_launch("corr_generic_fwd_kernel");
}

// Backward: the hot parameterisation in f32 -> corr9_bwd_f32; half -> gather; kernel 1 / stride 1 / pad 0 ->
// corr_k1_bwd_kernel; anything else -> the scatter kernel (atomics: refused in deterministic mode).
template <typename T>
static int corr_bwd_any(const T* in1, const T* in2, const T* gout, T* g1, T* g2, const CorrParams& p,
                        hipStream_t st) {
  const long npix = (long)p.B * p.C * p.iH * p.iW;
  if constexpr (std::is_same<T, float>::value) {
    if (is_hot_param(p)) return corr9_bwd_f32(in1, in2, gout, g1, g2, p, st);
  }
  if constexpr (std::is_same<T, __half>::value) {
    hipLaunchKernelGGL((corr_generic_bwd_gather_kernel<T>), dim3(flat_grid(npix)), dim3(256), 0, st, in1, in2, gout, g1, g2, p,
                       npix);
    return check_launch("corr_generic_bwd_gather_kernel");
  } else {
    if (is_k1(p)) {
      hipLaunchKernelGGL((corr_k1_bwd_kernel<T>), dim3(flat_grid(npix)), dim3(256), 0, st, in1, in2, gout, g1, g2, p, npix);
      return check_launch("corr_k1_bwd_kernel");
    }
    RFN_REFUSE_NONDET(true, "rfn_corr_bwd", "corr_generic_bwd_kernel, floating-point atomics (no deterministic form)");
    const size_t bytes = sizeof(T) * (size_t)npix;
    // (kernels, not memset nodes: this backward may run inside a captured pass -- capi.hip zero_async)
    if (int rc = zero_async(g1, bytes, st)) return rc;
    if (int rc = zero_async(g2, bytes, st)) return rc;
    const long total = (long)p.B * p.patchH * p.patchW * p.oH * p.oW;
    hipLaunchKernelGGL((corr_generic_bwd_kernel<T>), dim3(flat_grid(total)), dim3(256), 0, st, in1, in2, gout, g1, g2, p, total);
    return check_launch("corr_generic_bwd_kernel");
  }
}

}  // namespace rfn

using namespace rfn;

extern "C" {

// The six sampler entry points: one body per direction.  P is the ABI's pointer type (void for half), T the kernels'.
#define RFN_CORR_ARGS                                                                                                      \
  int B, int C, int iH, int iW, int kH, int kW, int patchH, int patchW, int padH, int padW, int dilH, int dilW, int dpH, \
      int dpW, int dH, int dW, rfn_stream_t stream
#define RFN_CORR_ENTRY(SUFFIX, P, T)                                                                                      \
  int rfn_corr_fwd_##SUFFIX(const P* in1, const P* in2, P* out, RFN_CORR_ARGS) {                                           \
    RFN_REQUIRE(in1 && in2 && out, "rfn_corr_fwd_" #SUFFIX ": null pointer");                                              \
    CorrParams p;                                                                                                         \
    if (int rc = fill_params(p, B, C, iH, iW, kH, kW, patchH, patchW, padH, padW, dilH, dilW, dpH, dpW, dH, dW)) return rc; \
    return corr_fwd_any<T>((const T*)in1, (const T*)in2, (T*)out, p, (hipStream_t)stream);                                \
  }                                                                                                                       \
  int rfn_corr_bwd_##SUFFIX(const P* in1, const P* in2, const P* grad_out, P* grad_in1, P* grad_in2, RFN_CORR_ARGS) {      \
    RFN_REQUIRE(in1 && in2 && grad_out && grad_in1 && grad_in2, "rfn_corr_bwd_" #SUFFIX ": null pointer");                 \
    CorrParams p;                                                                                                         \
    if (int rc = fill_params(p, B, C, iH, iW, kH, kW, patchH, patchW, padH, padW, dilH, dilW, dpH, dpW, dH, dW)) return rc; \
    return corr_bwd_any<T>((const T*)in1, (const T*)in2, (const T*)grad_out, (T*)grad_in1, (T*)grad_in2, p,               \
                           (hipStream_t)stream);                                                                          \
  }
RFN_CORR_ENTRY(f32, float, float)
RFN_CORR_ENTRY(f64, double, double)
RFN_CORR_ENTRY(f16, void, __half)
#undef RFN_CORR_ENTRY

// The gather kernel for fp32, any parameterisation: no atomics, legal in deterministic mode (rfn_corr_bwd_f32 refuses its generic
// parameterisation there).
int rfn_corr_bwd_gather_f32(const float* in1, const float* in2, const float* grad_out, float* grad_in1, float* grad_in2,
                            RFN_CORR_ARGS) {
  RFN_REQUIRE(in1 && in2 && grad_out && grad_in1 && grad_in2, "rfn_corr_bwd_gather_f32: null pointer");
  CorrParams p;
  if (int rc = fill_params(p, B, C, iH, iW, kH, kW, patchH, patchW, padH, padW, dilH, dilW, dpH, dpW, dH, dW)) return rc;
  const long npix = (long)p.B * p.C * p.iH * p.iW;
  hipLaunchKernelGGL((corr_generic_bwd_gather_kernel<float>), dim3(flat_grid(npix)), dim3(256), 0, (hipStream_t)stream, in1, in2,
                     grad_out, grad_in1, grad_in2, p, npix);
  return check_launch("corr_generic_bwd_gather_kernel");
}
#undef RFN_CORR_ARGS

int rfn_local_corr_layer_f32(const float* feature_target, const float* feature_source, const float* flow,
                             float* out, int B, int C, int H, int W, rfn_stream_t stream) {
  RFN_REQUIRE(feature_target && feature_source && out, "rfn_local_corr_layer_f32: null pointer");
  RFN_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "rfn_local_corr_layer_f32: non-positive size");
  hipStream_t st = (hipStream_t)stream;
  if (flow) return launch_corr9<true, true>(feature_target, feature_source, flow, out, B, C, H, W, st);
  return launch_corr9<true, false>(feature_target, feature_source, nullptr, out, B, C, H, W, st);
}

long rfn_local_corr_layer_split_workspace_bytes(int B, int H, int W, int splits) {
  if (B <= 0 || H <= 0 || W <= 0 || splits <= 0) return 0;
  const long tickets = (long)B * rfn::cdiv(W, rfn::kPipeTW) * rfn::cdiv(H, rfn::kSmallTH);   // one per tile of launch_corr9_split
  return ((long)splits * B * 81 * H * W + tickets) * 4;
}

int rfn_local_corr_layer_split_f32(const float* feature_target, const float* feature_source, float* out,
                                   float* workspace, int B, int C, int H, int W, int splits, rfn_stream_t stream) {
  RFN_REQUIRE(feature_target && feature_source && out && workspace, "rfn_local_corr_layer_split_f32: null pointer");
  RFN_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && (W & 3) == 0, "rfn_local_corr_layer_split_f32: B=%d C=%d H=%d W=%d (W %% 4 == 0)",
              B, C, H, W);
  RFN_REQUIRE(splits >= 2 && splits <= 64 && C % splits == 0 && (C / splits) % 8 == 0,
              "rfn_local_corr_layer_split_f32: %d channels in %d chunks (chunks of a multiple of 8 channels)", C, splits);
  return launch_corr9_split(feature_target, feature_source, out, workspace, B, C, H, W, splits, (hipStream_t)stream);
}

}  // extern "C"
