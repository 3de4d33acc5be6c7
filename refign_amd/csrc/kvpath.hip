// refign_amd/csrc/kvpath.hip -- the key / value path of a MiT attention block (mix_transformer.py:142-150) on gradient-free passes, in
// ONE kernel:   norm1(x) tokens -> spatial-reduction Linear over r x r patches (+ bias) -> LayerNorm -> kv Linear (+ bias) -> K's R-pack
// and V's T-pack in the layout rfn_attn_fwd reads (attn.hip).  bf16 or f16, fp32 accumulation.
// The five launches it stands for (patchify_kernel, gemm_nt, layernorm_fwd_vec_kernel, gemm_nt, attn_pack_kernel) move the token map
// twice more than needed (the patch copy is written and re-read), write two pack images nobody reads on a gradient-free pass and send
// three tiny intermediates through HBM; here the map is read once, in place, and everything between it and the packs stays on the CU.
//
// Tile.  A workgroup owns kKvBlocks = 3 whole 32-row pack blocks (96 reduced tokens; blocks are numbered b * nkblk + blk, a tile may
// span two images) and ALL channels of them -- the LayerNorm needs whole rows.  Why 96 rows: every workgroup streams the whole
// spatial-reduction and kv weight (0.5-1.2 MB, L2-resident) once per tile, so rows per tile is what bounds the L2 traffic; the teacher
// has 640 pack blocks per launch on 256 CUs, and 3 blocks per tile make that 214 workgroups -- one round with every workgroup alone on
// its CU -- where 2 blocks are 320 (one round and a quarter) and 4 blocks 160 (a third of the chip idle).
// Waves.  Four waves; in both products a wave owns 32-row blocks of the WEIGHT (output channels) and all three token blocks, so a
// weight row is read by exactly one wave: it goes global -> register in whole 128-byte lines, requested two steps ahead of the MFMAs
// that use it, and is re-shaped into fragments through a 4.5-8.5 KB LDS scratch of the wave's own -- no barrier.  Only the token
// operand is shared: the gathered K-step of the 96 patch rows is staged global -> register (two steps ahead) -> LDS (two stages, one
// barrier per K-step).
// Launches with few blocks (the ImageNet encoder's two images: 32 blocks) take ONE block per workgroup instead of three.
//   C = 64 has two channel blocks only: there a wave owns (channel block wave & 1) x (token blocks wave >> 1 and (wave >> 1) + 2).
// Products are the NT kernel's (gemm2.h): transposed 32x32x16 blocks D[i = n][j = token] = mma(W fragment, token fragment), k slots
// 8 g + e, K ascending in steps of 16 into one accumulator; bias added in fp32, one rounding.  The LayerNorm is
// layernorm_fwd_vec_kernel's arithmetic lane for lane (same lanes per row, same order of the sums).  So the plain kv output is bit-equal
// to the five-launch chain.
// Gather.  Reduced token (b, oy, ox), K index (ry, rx, c): r runs of r * C contiguous elements of the (B, H*W, C) map, W * C apart;
// r * C is a multiple of the K-step, so a step lies inside one run: per-lane token bases computed once + one uniform offset per step.
// Stage 4 (r = 1): the norm1(x) rows are the kv Linear's operand; products and stores only.
// Where it stands (profiles/kvpath_kbench.txt; 40 views, stages 1-4, kernel trace): 52 / 34 / 74 / 51 us against 142 / 73 / 92 / 52 us
// for the five launches.  Stages 1-2 are within 2 x of one pass over the map; stages 3-4 are bound by the weight stream from L2 (214
// workgroups x 1.0-1.2 MB), not by the map.  In the step: profiles/kvpath_ab.txt.
#include "common.h"
#include "elem.h"
#include "mfma.h"

namespace rfn {

constexpr int kKvBlocks = 3;                 // 32-row pack blocks per workgroup (1 for launches of fewer than kKvSmall tiles)
constexpr int kKvSmall = 128;
constexpr int kKvPack = 4096;                // bytes of a pack block (attn.hip)
constexpr int kKvSPitch = 64 + 8;            // transposition scratch: [32 rows][64 d] 16-bit, padded by one 16-byte access

template <int C, int R, int NB> struct KvGeom {
  static constexpr int ROWS = 32 * NB;
  static constexpr int KSTEP = C <= 128 ? 128 : 64;       // elements of K per stage of the gathered operand
  static constexpr int XP = KSTEP + 8, YP = C + 8;                          // LDS row pitches (16-bit elements), + one 16-byte access
  static constexpr int YBYTES = ROWS * YP * 2;
  static constexpr int XBYTES = R > 1 ? ROWS * XP * 2 : 0;
  static constexpr int WSCR = 32 * ((R > 1 && KSTEP > 64 ? KSTEP : 64) + 8) * 2;   // a wave's own scratch: 32 rows of a K-step
  static constexpr int SBYTES = 4 * WSCR;
  static constexpr int LDS = YBYTES + 2 * XBYTES + SBYTES;
  static_assert(C % 64 == 0 && (R == 1 || (R * C) % KSTEP == 0), "a K-step never straddles a run of the gather");
  static_assert(LDS <= 160 * 1024, "LDS");
};

template <int DT, int C, int R, int NB>
__global__ __launch_bounds__(256) void kvpath_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Wsr,
                                                     const uint16_t* __restrict__ bsr, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float eps, const uint16_t* __restrict__ Wkv,
                                                     const uint16_t* __restrict__ bkv, unsigned char* __restrict__ kr,
                                                     unsigned char* __restrict__ vt, uint16_t* __restrict__ kvout, int B, int H,
                                                     int W, int Wr, int Nkv, int nkblk) {
  using E = Elem<DT>;
  using vec8 = typename E::vec8;
  using G = KvGeom<C, R, NB>;
  constexpr int kKvBlocks = NB, kKvRows = G::ROWS;
  constexpr int CB = C / 32, HEADS = C / 64, NCH = 2 * HEADS;   // channel blocks; 64-wide chunks of the kv row: K heads, then V heads
  constexpr int YP = G::YP;
  __shared__ __attribute__((aligned(16))) unsigned char smem[G::LDS];
  uint16_t* yt = (uint16_t*)smem;                                // [96 tokens][C] 16-bit: sr output -> LayerNorm output (in place)
  unsigned char* scr = smem + G::YBYTES + 2 * G::XBYTES;

  const int t = threadIdx.x, lane = t & 63, col = lane & 31, g = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nblocks = B * nkblk, gb0 = blockIdx.x * kKvBlocks;
  // tile row -> (image, block, row of the image); rows past Nkv (a block's tail, the block that makes nkblk even) are stored as zeros
  auto row_of = [&](int tr, int& b, int& blk, int& row) {
    const int gb = gb0 + (tr >> 5);
    b = gb / nkblk;
    blk = gb - b * nkblk;
    row = blk * 32 + (tr & 31);
    return gb < nblocks && row < Nkv;
  };

  if constexpr (R > 1) {
    constexpr int KSTEP = G::KSTEP, XP = G::XP, NKS = KSTEP / 16, K1 = R * R * C;
    constexpr int PPR = KSTEP / 8, RPP = 256 / PPR, NI = kKvRows / RPP;      // 16-byte pieces per row; rows per pass of the 256 threads
    constexpr int NCW = CB >= 4 ? (CB + 3) / 4 : 1, NTW = CB >= 4 ? kKvBlocks : (kKvBlocks + 1) / 2;
    static_assert(CB >= 4 || CB == 2, "wave map");
    // ---- the gather: thread = (piece t % PPR of rows t / PPR + RPP i) --------------------------------------------------------
    const int sub = t % PPR, rb = t / PPR;
    unsigned xo[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      int b, blk, row;
      const bool ok = row_of(rb + RPP * i, b, blk, row);
      const int oy = row / Wr, ox = row - oy * Wr;
      xo[i] = (ok ? (unsigned)(((b * H + oy * R) * W + ox * R) * C) : 0u) + sub * 8;
    }
    auto fetch_x = [&](int k0, u32x4(&rx)[NI]) {
      const int ry = k0 / (R * C);
      const unsigned off = (unsigned)(ry * W * C + (k0 - ry * R * C));      // uniform: the run's row of the map + the place in the run
#pragma unroll
      for (int i = 0; i < NI; ++i) rx[i] = *(const u32x4*)(X + (xo[i] + off));
    };
    auto stash_x = [&](int buf, const u32x4(&rx)[NI]) {
      unsigned char* xs = smem + G::YBYTES + buf * G::XBYTES + (rb * XP + sub * 8) * 2;
#pragma unroll
      for (int i = 0; i < NI; ++i) *(u32x4*)(xs + RPP * i * XP * 2) = rx[i];
    };
    // ---- wave map: channel blocks cbv[], token blocks tbv[]; past the end: clamped (computed twice, stored once) ---------------
    int cbc[NCW], tbc[NTW];
    bool cb_ok[NCW], tb_ok[NTW];
#pragma unroll
    for (int i = 0; i < NCW; ++i) {
      const int cb = CB >= 4 ? wave + 4 * i : (wave & 1);
      cb_ok[i] = cb < CB;
      cbc[i] = min(cb, CB - 1);
    }
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      const int tb = CB >= 4 ? j : (wave >> 1) + 2 * j;
      tb_ok[j] = tb < kKvBlocks;
      tbc[j] = min(tb, kKvBlocks - 1);
    }
    // weight rows are fetched in whole 128-byte lines (instruction q of a 32-row block: rows q RPI .. + RPI - 1, lane = (row, 16-byte
    // piece)) and turned into MFMA fragments (lane = (row, k half)) through the wave's own LDS scratch right before use: fetched as
    // fragments, the NKS instructions of a block each ask for 32 bytes of the same 32 lines and every one of them goes to L2
    constexpr int WP = KSTEP + 8, PPW = KSTEP / 8, RPI = 64 / PPW;
    static_assert(32 / RPI == NKS, "instructions per block");
    const int wr = lane / PPW, wp = lane % PPW;
    const uint16_t* wrow[NCW];
#pragma unroll
    for (int i = 0; i < NCW; ++i) wrow[i] = Wsr + (long)(cbc[i] * 32 + wr) * K1 + wp * 8;
    auto fetch_w = [&](int k0, vec8(&wf)[NCW][NKS]) {
#pragma unroll
      for (int i = 0; i < NCW; ++i)
#pragma unroll
        for (int q = 0; q < NKS; ++q) wf[i][q] = *(const vec8*)(wrow[i] + (long)q * RPI * K1 + k0);
    };
    unsigned char* wscr = scr + wave * G::WSCR;
    // (LDS serves a wave's instructions in order; the empty asm statements keep the compiler from moving them across each other)
    auto to_frags = [&](const vec8(&raw)[NKS], vec8(&fr)[NKS]) {
      asm volatile("" ::: "memory");
#pragma unroll
      for (int q = 0; q < NKS; ++q) *(vec8*)(wscr + ((q * RPI + wr) * WP + wp * 8) * 2) = raw[q];
      asm volatile("" ::: "memory");
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) fr[ks] = *(const vec8*)(wscr + (col * WP + ks * 16 + 8 * g) * 2);
      asm volatile("" ::: "memory");
    };
    f32x16 acc[NCW][NTW];
#pragma unroll
    for (int i = 0; i < NCW; ++i)
#pragma unroll
      for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    constexpr int nk = K1 / KSTEP;
    // one K-step.  Operands are requested TWO steps ahead (a step's products are ~0.5 us, a request takes 1-2 us to come back): step
    // s + 2's loads are issued, step s is multiplied (weight fragments `cur`), then step s + 1's token pieces -- requested during
    // step s - 1 -- go from registers to the other LDS stage; one barrier: that stage was last read in step s - 1.  Three weight
    // register sets and two token register sets rotate, so the loop is written out over 6 steps.
    auto kstep = [&](int s, vec8(&cur)[NCW][NKS], vec8(&far)[NCW][NKS], const u32x4(&rnext)[NI], u32x4(&rfar)[NI]) {
      const bool more = s + 1 < nk;
      if (s + 2 < nk) {
        fetch_x((s + 2) * KSTEP, rfar);
        fetch_w((s + 2) * KSTEP, far);
      }
      const unsigned char* xs = smem + G::YBYTES + (s & 1) * G::XBYTES;
      auto xfrag = [&](int j, int ks) { return *(const vec8*)(xs + ((tbc[j] * 32 + col) * XP + ks * 16 + 8 * g) * 2); };
      vec8 xall[NCW > 1 ? NKS : 1][NTW];                   // several channel blocks per wave: the token fragments are read once
      if constexpr (NCW > 1) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
          for (int j = 0; j < NTW; ++j) xall[ks][j] = xfrag(j, ks);
      }
#pragma unroll
      for (int i = 0; i < NCW; ++i) {
        vec8 wfr[NKS];
        to_frags(cur[i], wfr);
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
          for (int j = 0; j < NTW; ++j) acc[i][j] = E::mma(wfr[ks], NCW > 1 ? xall[NCW > 1 ? ks : 0][j] : xfrag(j, ks), acc[i][j]);
      }
      if (more) stash_x((s + 1) & 1, rnext);
      __syncthreads();
    };
    vec8 wf0[NCW][NKS], wf1[NCW][NKS], wf2[NCW][NKS];
    u32x4 rxa[NI], rxb[NI];
    static_assert(nk >= 2, "two steps in flight");
    fetch_x(0, rxa);
    fetch_w(0, wf0);
    fetch_x(KSTEP, rxb);
    fetch_w(KSTEP, wf1);
    stash_x(0, rxa);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < nk; s += 6) {
      kstep(s, wf0, wf2, rxb, rxa);
      if (s + 1 < nk) kstep(s + 1, wf1, wf0, rxa, rxb);
      if (s + 2 < nk) kstep(s + 2, wf2, wf1, rxb, rxa);
      if (s + 3 < nk) kstep(s + 3, wf0, wf2, rxa, rxb);
      if (s + 4 < nk) kstep(s + 4, wf1, wf0, rxb, rxa);
      if (s + 5 < nk) kstep(s + 5, wf2, wf1, rxa, rxb);
    }
    // ---- + bias, one rounding (what the spatial-reduction GEMM stores) -> yt[token][channel] -----------------------------------
#pragma unroll
    for (int i = 0; i < NCW; ++i)
#pragma unroll
      for (int j = 0; j < NTW; ++j) {
        if (!(cb_ok[i] && tb_ok[j])) continue;                   // wave-uniform
        const int tok = tbc[j] * 32 + col;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n0 = cbc[i] * 32 + 8 * q + 4 * g;            // four consecutive channels
          float bf[4];
          unpack4<DT>(*(const u32x2*)(bsr + n0), bf);
          *(u32x2*)(yt + tok * YP + n0) = pack4<DT>(acc[i][j][4 * q] + bf[0], acc[i][j][4 * q + 1] + bf[1],
                                                   acc[i][j][4 * q + 2] + bf[2], acc[i][j][4 * q + 3] + bf[3]);
        }
      }
    __syncthreads();
    // ---- LayerNorm over C, in place: layernorm_fwd_vec_kernel's lanes and arithmetic (layernorm.hip) ---------------------------
    {
      constexpr int LPR = C <= 64 ? 8 : (C <= 128 ? 16 : (C <= 256 ? 32 : 64)), RPW = 64 / LPR;
      const int ls = lane % LPR, grp = lane / LPR, c = ls * 8;
      const bool act = c < C;
      float gm[8], bt[8];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4 a = *(const f32x4*)(gamma + (act ? c : 0) + 4 * h), b = *(const f32x4*)(beta + (act ? c : 0) + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          gm[4 * h + e] = a[e];
          bt[4 * h + e] = b[e];
        }
      }
      const float invC = 1.0f / (float)C;
#pragma unroll 1
      for (int it = 0; it < kKvRows / (4 * RPW); ++it) {
        uint16_t* p = yt + ((it * 4 + wave) * RPW + grp) * YP + (act ? c : 0);
        float v[8];
        if (act) load8<DT>(p, v);
        else {
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] = 0.0f;
        }
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += v[i];
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float mu = s * invC;
        float q = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float d = act ? v[i] - mu : 0.0f;
          q = fmaf(d, d, q);
        }
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
        const float rs = rsqrtf(q * invC + eps);
        if (act) {
          float o[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) o[i] = fmaf((v[i] - mu) * rs, gm[i], bt[i]);
          const u32x2 lo = pack4<DT>(o[0], o[1], o[2], o[3]), hi = pack4<DT>(o[4], o[5], o[6], o[7]);
          *(u32x4*)p = u32x4{lo[0], lo[1], hi[0], hi[1]};
        }
      }
    }
    __syncthreads();
  } else {
    // ---- stage 4: the rows themselves; rows past Nkv as zeros ------------------------------------------------------------------
    constexpr int PPR = C / 8;
    for (int p = t; p < kKvRows * PPR; p += 256) {
      const int tr = p / PPR, sub = p - tr * PPR;
      int b, blk, row;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (row_of(tr, b, blk, row)) v = *(const u32x4*)(X + ((long)b * Nkv + row) * C + sub * 8);
      *(u32x4*)(yt + tr * YP + sub * 8) = v;
    }
    __syncthreads();
  }

  // ---- kv Linear: per pass a wave owns one 64-wide chunk of the kv row (one head's K or V) and the three token blocks -----------
  constexpr int NPASS = (NCH + 3) / 4;
#pragma unroll 1
  for (int pass = 0; pass < NPASS; ++pass) {
    const int hc = pass * 4 + wave;
    const bool hc_ok = hc < NCH;
    const int hcc = min(hc, NCH - 1);
    // (weight rows in whole lines, fragments through the wave's scratch: as in the first product; 8 rows x 128 bytes per instruction)
    unsigned char* ws = scr + wave * G::WSCR;
    const int wr = lane >> 3, wp = lane & 7;
    const uint16_t* w2row = Wkv + (long)(hcc * 64 + wr) * C + wp * 8;
    auto fetch_w2 = [&](int k0, vec8(&wf)[2][4]) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int q = 0; q < 4; ++q) wf[a][q] = *(const vec8*)(w2row + (long)(a * 32 + q * 8) * C + k0);
    };
    auto to_frags2 = [&](const vec8(&raw)[4], vec8(&fr)[4]) {
      asm volatile("" ::: "memory");
#pragma unroll
      for (int q = 0; q < 4; ++q) *(vec8*)(ws + ((q * 8 + wr) * kKvSPitch + wp * 8) * 2) = raw[q];
      asm volatile("" ::: "memory");
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) fr[ks] = *(const vec8*)(ws + (col * kKvSPitch + ks * 16 + 8 * g) * 2);
      asm volatile("" ::: "memory");
    };
    f32x16 acc2[2][kKvBlocks];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int j = 0; j < kKvBlocks; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[a][j][r] = 0.f;
    auto kstep2 = [&](int s, vec8(&cur)[2][4], vec8(&far)[2][4]) {      // no barrier here: the token operand is the finished tile
      if (s + 2 < HEADS) fetch_w2((s + 2) * 64, far);
      vec8 yf[4][kKvBlocks];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int j = 0; j < kKvBlocks; ++j) yf[ks][j] = *(const vec8*)(yt + (j * 32 + col) * YP + s * 64 + ks * 16 + 8 * g);
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        vec8 wfr[4];
        to_frags2(cur[a], wfr);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
          for (int j = 0; j < kKvBlocks; ++j) acc2[a][j] = E::mma(wfr[ks], yf[ks][j], acc2[a][j]);
      }
    };
    vec8 v0[2][4], v1[2][4], v2[2][4];
    fetch_w2(0, v0);
    if (HEADS > 1) fetch_w2(64, v1);
#pragma unroll 1
    for (int s = 0; s < HEADS; s += 3) {
      kstep2(s, v0, v2);
      if (s + 1 < HEADS) kstep2(s + 1, v1, v0);
      if (s + 2 < HEADS) kstep2(s + 2, v2, v1);
    }
    // ---- + bias, one rounding, 16-byte runs of 8 d (the NT kernel's lane exchange) -> K: R-pack; V: T-pack through a transposition
    // in LDS; both: the plain row if asked for.  Every wave walks the same barriers; what it stores depends on its chunk.
    const bool is_k = hc < HEADS;
#pragma unroll
    for (int j = 0; j < kKvBlocks; ++j) {
      int b, blk, row;
      const bool valid = row_of(j * 32 + col, b, blk, row);
      const bool live = hc_ok && gb0 + j < nblocks;                // wave-uniform
      const long pblk = ((long)(b * NCH + hcc) * nkblk + blk) * kKvPack;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          float ba[4], bb[4];
          const uint16_t* bp = bkv + hcc * 64 + a * 32 + 16 * pr + 4 * g;
          unpack4<DT>(*(const u32x2*)bp, ba);
          unpack4<DT>(*(const u32x2*)(bp + 8), bb);
          const u32x2 pa = pack4<DT>(acc2[a][j][8 * pr] + ba[0], acc2[a][j][8 * pr + 1] + ba[1], acc2[a][j][8 * pr + 2] + ba[2],
                                     acc2[a][j][8 * pr + 3] + ba[3]);
          const u32x2 pb = pack4<DT>(acc2[a][j][8 * pr + 4] + bb[0], acc2[a][j][8 * pr + 5] + bb[1], acc2[a][j][8 * pr + 6] + bb[2],
                                     acc2[a][j][8 * pr + 7] + bb[3]);
          auto r0 = __builtin_amdgcn_permlane32_swap(pa[0], pb[0], false, false);
          auto r1 = __builtin_amdgcn_permlane32_swap(pa[1], pb[1], false, false);
          const u32x4 o = valid ? u32x4{r0[0], r1[0], r0[1], r1[1]} : u32x4{0u, 0u, 0u, 0u};
          const int dc = a * 4 + 2 * pr + g;                        // d = 8 dc .. 8 dc + 7 of row `row`
          if (live && is_k) *(u32x4*)(kr + pblk + (dc * 32 + col) * 16) = o;
          if (live && valid && kvout != nullptr) *(u32x4*)(kvout + ((long)b * Nkv + row) * (2 * C) + hcc * 64 + dc * 8) = o;
          *(u32x4*)(ws + (col * kKvSPitch + dc * 8) * 2) = o;
        }
      __syncthreads();
      if (live && !is_k) {
        // T-pack [8 row quads][64 d][4 rows]: lane = d; b and blk are the block's, the same in every lane
        const uint16_t* sc = (const uint16_t*)ws + lane;
#pragma unroll
        for (int rq = 0; rq < 8; ++rq) {
          const unsigned h0 = sc[(4 * rq) * kKvSPitch], h1 = sc[(4 * rq + 1) * kKvSPitch], h2 = sc[(4 * rq + 2) * kKvSPitch],
                         h3 = sc[(4 * rq + 3) * kKvSPitch];
          *(u32x2*)(vt + pblk + (rq * 64 + lane) * 8) = u32x2{h0 | (h1 << 16), h2 | (h3 << 16)};
        }
      }
      __syncthreads();
    }
  }
}

template <int DT, int C, int R, int NB>
static int kvpath_launch(const void* x, const void* w_sr, const void* b_sr, const float* gamma, const float* beta, float eps,
                         const void* w_kv, const void* b_kv, void* k_rpack, void* v_tpack, void* kv_out, int B, int H, int W, int Nkv,
                         int nkblk, hipStream_t st) {
  const int tiles = cdiv((long)B * nkblk, NB);
  hipLaunchKernelGGL((kvpath_kernel<DT, C, R, NB>), dim3(tiles), dim3(256), 0, st, (const uint16_t*)x, (const uint16_t*)w_sr,
                     (const uint16_t*)b_sr, gamma, beta, eps, (const uint16_t*)w_kv, (const uint16_t*)b_kv, (unsigned char*)k_rpack,
                     (unsigned char*)v_tpack, (uint16_t*)kv_out, B, H, W, R > 1 ? W / R : 1, Nkv, nkblk);
  return check_launch("kvpath_kernel");
}

}  // namespace rfn

extern "C" int rfn_kv_path(const void* x, const void* w_sr, const void* b_sr, const float* gamma, const float* beta, float eps,
                           const void* w_kv, const void* b_kv, void* k_rpack, void* v_tpack, void* kv_out, int B, int H, int W, int C,
                           int r, int nkblk, int blocks_per_wg, int dtype, rfn_stream_t stream) {
  using namespace rfn;
  RFN_REQUIRE(x && w_kv && b_kv && k_rpack && v_tpack, "rfn_kv_path: null pointer");
  RFN_REQUIRE(r == 1 || (w_sr && b_sr && gamma && beta), "rfn_kv_path: r = %d needs the spatial-reduction and LayerNorm parameters", r);
  RFN_REQUIRE(B > 0 && H >= r && W >= r && r >= 1, "rfn_kv_path: B=%d H=%d W=%d r=%d", B, H, W, r);
  RFN_REQUIRE((long)B * H * W * C < (1L << 31), "rfn_kv_path: B*H*W*C = %ld (32-bit element offsets)", (long)B * H * W * C);
  const int Nkv = (H / r) * (W / r);
  RFN_REQUIRE(nkblk % 2 == 0 && (long)nkblk * 32 >= Nkv && (long)B * nkblk < (1L << 24),
              "rfn_kv_path: nkblk=%d (even, >= ceil(%d / 32))", nkblk, Nkv);
  hipStream_t st = (hipStream_t)stream;
  // few blocks (the ImageNet encoder's two images): one block per workgroup, so that the launch still spreads over the chip
  RFN_REQUIRE(blocks_per_wg == 0 || blocks_per_wg == 1 || blocks_per_wg == kKvBlocks, "rfn_kv_path: blocks_per_wg=%d (0, 1 or %d)",
              blocks_per_wg, kKvBlocks);
  const bool small = blocks_per_wg ? blocks_per_wg == 1 : cdiv((long)B * nkblk, kKvBlocks) < kKvSmall;
  return dt16(dtype, "rfn_kv_path", [&](auto dtc) {
    constexpr int DT = decltype(dtc)::value;
#define RFN_KV(CC, RR)                                                                                                   \
  if (C == CC && r == RR)                                                                                                \
    return small ? kvpath_launch<DT, CC, RR, 1>(x, w_sr, b_sr, gamma, beta, eps, w_kv, b_kv, k_rpack, v_tpack, kv_out, B, H, W, Nkv, \
                                                nkblk, st)                                                               \
                 : kvpath_launch<DT, CC, RR, kKvBlocks>(x, w_sr, b_sr, gamma, beta, eps, w_kv, b_kv, k_rpack, v_tpack, kv_out, B, H, \
                                                        W, Nkv, nkblk, st)
    RFN_KV(64, 8);
    RFN_KV(128, 4);
    RFN_KV(320, 2);
    RFN_KV(512, 1);
#undef RFN_KV
    return fail(RFN_EINVAL, "rfn_kv_path: (C, r) = (%d, %d): built for (64, 8), (128, 4), (320, 2), (512, 1)", C, r);
  });
}
