// Forward / dgrad kernels of conv_igemm.hip that keep their activation region
// in LDS: the tap-reuse region kernel and the first-layer (Cin = 8) kernel.
#pragma once
#include "conv_common_dev.h"

namespace dl {

// --------------------------------------------------------------------------
// forward / dgrad implicit GEMM with the activation REGION resident in LDS
// (tap reuse).  The generic kernel above streams the A operand tap by tap:
// each of the KS*KS k-steps of a 64-channel chunk re-reads an almost
// identical shifted window of the input through the L2 -> LDS path, which is
// what bounds it (~25 B/clk/CU of LDS-DMA fill).  Here a workgroup's M tile
// (BM = 128 output pixels = whole output rows of one image, or whole images)
// loads the padded input pixels it touches ONCE per 64-channel chunk, and
// every tap reads its A fragments from that region at a wave-uniform offset;
// only the weight tile (B) is streamed per k-step (3-stage LDS-DMA ring).
// Fill bytes per FLOP drop ~1.8-2.6x.
//
// Region image: pixel-major, S = 10 16-byte slots per pixel (8 data + 2 pad),
// row stride RS = RW*S + RP slots, image stride IS = RH*RS (host-chosen, see
// region_geom): with these paddings the ds_read_b128 fragment reads of 16
// output pixels are bank-conflict free for W = 4, 8, 16, 32 at every tap,
// and a tap is a plain address offset (no per-tap swizzle arithmetic).
// Pad slots are loaded from an out-of-range offset (zeros, no traffic).
// --------------------------------------------------------------------------
struct RegionGeom {
  int S, RS, IS;    // slots per pixel / region row / region image
  int RW, RH;       // region row width (= Wp) and rows per region image
  int nimg;         // images per region (rows mode: 1)
  int rows_mode;    // 1: M tile = BM/W output rows of one image; 0: BM/HW whole images
  int nslot;        // slots per region (multiple of 64)
  int cpw;          // 64-channel chunks per workgroup (1 or 2)
  float inv_S, inv_RS, inv_IS;  // exact slot -> (img,row,col,chunk) decomposition (slots < 2^16)
};


template <int BN, bool STATS, bool SLAB, int STAGES, int WM, int WN, bool BNRED = false>
__global__ void __launch_bounds__(64 * WM * WN) conv_fwd_region_kernel(const bf16_t* __restrict__ x,
                                                              const bf16_t* __restrict__ w, bf16_t* __restrict__ y,
                                                              float* __restrict__ stats, float* __restrict__ slab,
                                                              const ConvGeom g, const RegionGeom rg, int splits,
                                                              unsigned long long* dbg, int ablate,
                                                              const BnRedArgs br) {
  const unsigned long long t_start = dbg ? stamp() : 0ull;
  constexpr int BM = 128, BK = 64, CPR = 8, NW = WM * WN, PD = STAGES - 1;
  constexpr int B_BYTES = BN * BK * 2, B_INS = B_BYTES / 1024 / NW, LPS = B_INS;
  constexpr int TM = BM / WM, TN = BN / WN, FM = TM / 16, FN = TN / 16;
  static_assert(B_INS >= 1 && B_INS * NW * 1024 == B_BYTES, "B DMA split");
  static_assert(FN % 2 == 0, "the 16-byte epilogue pairs N fragments");
  static_assert(STAGES >= 3, "fragment prefetch needs >= 3 ring slots");
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int region_bytes = rg.nslot * 16;
  char* sR = smem;                          // cpw region images
  char* sB = smem + rg.cpw * region_bytes;  // B ring

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int ntm = (g.M + BM - 1) / BM;
  const int npanel = (g.Cout / BN) * splits;
  const int id = xcd_swizzle(blockIdx.x, ntm * npanel);
  const int tm = id % ntm;
  const int panel = id / ntm;
  const int split = panel % splits, tn = panel / splits;
  const int m0 = tm * BM, n0 = tn * BN;
  const int HW = 1 << g.logHW, Wd = g.W;
  const int HpWp = g.Hp * g.Wp;
  const int taps = g.KS * g.KS;
  const int nk = rg.cpw * taps;
  const int img0 = m0 >> g.logHW, oh0 = (m0 & (HW - 1)) >> g.logW;  // oh0 = 0 in images mode
  const int start_pix = img0 * HpWp + oh0 * g.Wp;
  const rsrc_t xr = make_rsrc(x, (unsigned)((int64_t)g.B * HpWp * g.Cin * 2));
  const rsrc_t wr = make_rsrc(w, (unsigned)((int64_t)g.Cout * g.K * 2));
  const int cbase = split * rg.cpw;  // first 64-channel chunk of this workgroup

  // ---- region loads (once per chunk): lane-linear slots -> source pixel/chunk
  {
    const int nq = rg.nslot >> 6;
    // slot -> (region row R, pixel in row, chunk): the region's image rows
    // are consecutive padded rows (rows mode: RH rows of one image; images
    // mode: RH = Hp, whole images), so the source pixel is start + R*Wp + col
    const int nrows = rg.nimg * rg.RH;
    for (int q = wid; q < nq; q += NW) {
      const int sl = q * 64 + lane;
      const int R = (int)(((float)sl + 0.5f) * rg.inv_RS);
      const int r2 = sl - R * rg.RS;
      const int col = (r2 * 6554) >> 16;  // r2 / 10 (exact for r2 < 16384; S == 10)
      const int ch = r2 - col * 10;
      const bool ok = R < nrows && col < rg.RW && ch < 8;
      const int pix = start_pix + R * g.Wp + col;
      const unsigned voff = ok ? 2u * (unsigned)(pix * g.Cin + ch * 8) : kOOB;
      for (int c = 0; c < rg.cpw; ++c)
        blds16(xr, voff, 2u * (unsigned)((cbase + c) * 64), sR + c * region_bytes + q * 1024);
    }
  }
  // ---- B (weight) stream: k-step ks = (chunk c, tap t): k offset t*Cin + (cbase+c)*64
  int b_v[B_INS];
#pragma unroll
  for (int j = 0; j < B_INS; ++j) {
    const int row = 8 * (wid * B_INS + j) + (lane >> 3);
    const int ch = (lane & 7) ^ swz_b(row);
    b_v[j] = 2 * ((n0 + row) * g.K + ch * 8);
  }
  int ld_c = 0, ld_t = 0, ld_slot = 0;  // next k-step to load (wave-uniform)
  // Every step issues its DMA unconditionally (k-steps past the end load
  // zeros from an out-of-range offset into a slot nobody reads again), so the
  // number of loads in flight is the same at every wait and the loop body is
  // one basic block the scheduler can interleave.
  auto issue_b = [&](int q, bool live) {
    const unsigned soff = 2u * (unsigned)(ld_t * g.Cin + (cbase + ld_c) * 64);
    blds16(wr, live ? (unsigned)b_v[q] : kOOB, soff, sB + ld_slot * B_BYTES + (wid * B_INS + q) * 1024);
  };
  int ld_k = 0;
  auto advance_ld = [&]() {  // branch-free (keeps the step one basic block)
    ++ld_k;
    ++ld_t;
    const int wrap = ld_t == taps;
    ld_t -= wrap * taps;
    ld_c = min(ld_c + wrap, rg.cpw - 1);
    ++ld_slot;
    ld_slot -= (ld_slot == STAGES) * STAGES;
  };

  // ---- per-lane A fragment bases (slot of the tap-(0,0) pixel + lane's chunk)
  int a_base[FM];
#pragma unroll
  for (int a = 0; a < FM; ++a) {
    const int m = min(m0 + wm * TM + a * 16 + (lane & 15), g.M - 1);
    const int im = (m >> g.logHW) - img0;
    const int oh = ((m & (HW - 1)) >> g.logW) - oh0;
    const int ow = m & (Wd - 1);
    a_base[a] = (im * rg.IS + oh * rg.RS + ow * rg.S + (lane >> 4)) * 16;
  }
  // B fragment rows: N fragment b, MFMA row i -> channel
  // 32*(b>>1) + 8*(i>>2) + 4*(b&1) + (i&3) of the wave's TN channels (so a
  // lane's fragments 2p, 2p+1 cover 8 consecutive channels of the
  // transposed accumulator)
  int b_row[FN];
#pragma unroll
  for (int b = 0; b < FN; ++b) {
    const int i = lane & 15;
    b_row[b] = wn * TN + 32 * (b >> 1) + 8 * (i >> 2) + 4 * (b & 1) + (i & 3);
  }

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: region + PD B stages in flight
#pragma unroll
  for (int p = 0; p < PD; ++p) {
#pragma unroll
    for (int q = 0; q < LPS; ++q) issue_b(q, ld_k < nk);
    advance_ld();
  }
  const unsigned long long t_issued = dbg ? stamp() : 0ull;

  // fragment reads of k-step (rc, rkh, rkw) from ring slot rslot
  int rc = 0, rkh = 0, rkw = 0, rslot = 0;
  auto read_frags = [&](bf16x8 (&fa)[BK / 32][FM], bf16x8 (&fb)[BK / 32][FN]) {
    const char* As = sR + rc * region_bytes + (rkh * rg.RS + rkw * rg.S) * 16;  // wave-uniform tap offset
    const uint4* Bs = reinterpret_cast<const uint4*>(sB + rslot * B_BYTES);
    {  // advance the read state, branch-free
      ++rkw;
      const int ww = rkw == g.KS;
      rkw -= ww * g.KS;
      rkh += ww;
      const int wh = rkh == g.KS;
      rkh -= wh * g.KS;
      rc = min(rc + wh, rg.cpw - 1);
      ++rslot;
      rslot -= (rslot == STAGES) * STAGES;
    }
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      const int ch = kk * 4 + (lane >> 4);
#pragma unroll
      for (int b = 0; b < FN; ++b) fb[kk][b] = __builtin_bit_cast(bf16x8, Bs[b_row[b] * CPR + (ch ^ swz_b(b_row[b]))]);
#pragma unroll
      for (int a = 0; a < FM; ++a) fa[kk][a] = *reinterpret_cast<const bf16x8*>(As + a_base[a] + kk * 64);
    }
  };
  // Step i: [wait stage i+1, barrier] -> prefetch fragments of step i+1 ->
  // MFMAs of step i (C^T += W * X^T) with the DMA of stage i+PD (into the
  // slot read two steps ago), reads and MFMAs interleaved 1:1 so that a
  // read stalled on a full LDS queue never holds back more than one MFMA.
  constexpr int NRD = (BK / 32) * (FM + FN);  // fragment reads per step
  constexpr int NMF = (BK / 32) * FM * FN;    // MFMAs per step
  bf16x8 fa0[BK / 32][FM], fb0[BK / 32][FN], fa1[BK / 32][FM], fb1[BK / 32][FN];
  wait_vmcnt<(PD - 1) * LPS>();  // region + stage 0 landed
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t_first = dbg ? stamp() : 0ull;
  read_frags(fa0, fb0);
  auto step = [&](bf16x8 (&fca)[BK / 32][FM], bf16x8 (&fcb)[BK / 32][FN], bf16x8 (&fna)[BK / 32][FM],
                  bf16x8 (&fnb)[BK / 32][FN]) {
    wait_vmcnt<(PD - 2) * LPS>();  // stage i+1 landed (stages i+2 .. i+PD-1 may fly)
    // The fragments of step i must be in registers: the builtin wait is seen
    // by the compiler's waitcnt pass (an inline-asm one is not, and it would
    // then wait lgkmcnt(0) at the first MFMA, i.e. also for the prefetch).
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();        // stage i+1 visible to all waves; slot of step i-1 fully read
    __builtin_amdgcn_sched_barrier(0);
    const bool live = ld_k < nk;
    read_frags(fna, fnb);
#pragma unroll
    for (int q = 0; q < LPS; ++q) issue_b(q, live);
    advance_ld();
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk)
#pragma unroll
      for (int a = 0; a < FM; ++a)
#pragma unroll
        for (int b = 0; b < FN; ++b) acc[a][b] = mfma16(fcb[kk][b], fca[kk][a], acc[a][b]);
    // issue order: (MFMA, read) pairs, leftover reads, (MFMA, DMA) pairs, the rest
    constexpr int P1 = NRD < NMF ? NRD : NMF;
    constexpr int P2 = LPS < NMF - P1 ? LPS : NMF - P1;
#pragma unroll
    for (int q = 0; q < P1; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    if constexpr (NRD > P1) __builtin_amdgcn_sched_group_barrier(0x100, NRD - P1, 0);
#pragma unroll
    for (int q = 0; q < LPS; ++q) {
      if (q < P2) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    }
    if constexpr (NMF - P1 - P2 > 0) __builtin_amdgcn_sched_group_barrier(0x008, NMF - P1 - P2, 0);
  };
  int i = 0;
  for (; i + 1 < nk; i += 2) {
    step(fa0, fb0, fa1, fb1);
    step(fa1, fb1, fa0, fb0);
  }
  if (i < nk) step(fa0, fb0, fa1, fb1);
  const unsigned long long t_loop = dbg ? stamp() : 0ull;
  conv_fwd_epilogue_t<128, BN, STATS, SLAB, WM, WN, FM, FN, false, BNRED ? 1 : 0>(acc, g, y, stats, slab, split, tm,
                                                                                 m0, n0, smem, 0, 0, br);
  if (dbg && threadIdx.x == 0) {
    unsigned long long* d = dbg + (size_t)blockIdx.x * 5;
    d[0] = t_start; d[1] = t_issued; d[2] = t_first; d[3] = t_loop; d[4] = stamp();
  }
}

// s_waitcnt immediate (gfx9 encoding) for vmcnt(n), expcnt / lgkmcnt unconstrained
constexpr int vmcnt_imm(int n) { return (n & 15) | ((n >> 4) << 14) | 0x70 | 0xF00; }

// --------------------------------------------------------------------------
// First layer (Cin = 8 after the 3 -> 8 channel pad; K = KS*KS*8 = 200): the
// whole problem of a workgroup fits in LDS at once -- its 128 output pixels'
// padded input rows (16 B per pixel) and the 64 x K weight panel -- so it is
// one DMA burst, one barrier and ceil(K/32) MFMA steps; a 32-deep k-step
// covers 4 taps (lane group q = l>>4 reads tap 4s+q at its own pixel offset).
// The streaming kernel spent most of its time on per-lane tap arithmetic and
// on re-reading each input pixel through the L2 for 25 taps.
// Output: transposed accumulator -> conv_fwd_epilogue_t (16-byte stores, BN
// statistics per M tile).
// --------------------------------------------------------------------------
template <bool STATS, bool PAIR = false>
__global__ void __launch_bounds__(512) conv_fwd_c8_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                          bf16_t* __restrict__ y, float* __restrict__ stats,
                                                          const ConvGeom g, int region_rows, int mt,
                                                          unsigned long long* dbg) {
  // mt consecutive 128-pixel M tiles per workgroup (whole output rows of one
  // image): the weight panel (BN x taps x 16 B = 25.6 KiB for the reference's
  // layer 1) is DMA'd once per workgroup instead of once per tile, the region
  // covers the mt tiles' rows + the kernel halo, and the tiles are computed
  // one after the other from LDS (epilogue scratch after the region).
  constexpr int BM = 128, BN = 64, WM = 4, WN = 2, NW = 8, TM = 32, TN = 32, FM = 2, FN = 2;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const unsigned long long t_start = dbg ? stamp() : 0;  // (set_conv_debug: phase stamps)
  // PAIR: the input has <= 4 real channels and the weights are pair-packed
  // (pack1_index, cp = -KS): one 16-byte K chunk = channels 0-3 of two
  // horizontally adjacent taps, read as the first 8 bytes of two adjacent
  // region pixels -- K = KS * ceil(KS/2) * 8 (120 for 5x5) instead of
  // KS * KS * 8 (200), 4 k-steps instead of 7 and a 15.4 instead of a 25.6 KiB
  // weight panel.  (The odd last tap's partner is a zero weight; the pixel it
  // reads is the next padded row's zero border, or a zero slot.)
  const int cpr = (g.KS + 1) >> 1;
  const int taps = PAIR ? g.KS * cpr : g.KS * g.KS;  // K chunks (16 B) per output channel
  const int nsteps = (taps + 3) / 4;                 // 32-deep k-steps (4 chunks each)
  const int rpix = region_rows * g.Wp;               // region pixels (PAIR: 8 B each, else 16 B)
  const int rslots = PAIR ? (rpix + 1) / 2 : rpix;   // 16-byte region slots
  const int rslots_p = (rslots + 2 + 63) / 64 * 64;  // + >= 2 zero slots, whole DMA pieces
  // weight panel: BN rows x taps 16-B chunks.  (Its B-fragment reads put rows
  // r and r+16 on the same banks; spreading them with 4 empty chunks per 16
  // rows measured no change -- the k loop is not LDS-bound, 12.96 vs 13.24 us,
  // profiles/r6_c8_stamps.txt.)
  const int wslots = BN * taps;
  const int wslots_p = (wslots + 63) / 64 * 64;
  char* sR = smem;
  char* sW = smem + rslots_p * 16;
  char* sX = sW + wslots_p * 16;  // epilogue scratch ([WM][2][BN] floats)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int ntm = (g.M + BM - 1) / BM, ngr = ntm / mt;  // host: mt | ntm, mt * BM | H * W
  const int id = xcd_swizzle(blockIdx.x, ngr * (g.Cout / BN));
  const int tg = id % ngr, tn = id / ngr;
  const int mg0 = tg * mt * BM, n0 = tn * BN;
  const int HW = 1 << g.logHW;
  const int img0 = mg0 >> g.logHW, oh0 = (mg0 & (HW - 1)) >> g.logW;
  const int start_pix = (img0 * g.Hp + oh0) * g.Wp;
  const rsrc_t xr = make_rsrc(x, (unsigned)((int64_t)g.B * g.Hp * g.Wp * (PAIR ? 8 : 16)));
  const rsrc_t wr = make_rsrc(w, (unsigned)((int64_t)g.Cout * taps * 16));
  // one DMA burst: region pixels (contiguous padded rows) then the weight panel
  for (int q = wid; q < rslots_p / 64; q += NW) {
    const int sl = q * 64 + lane;
    blds16(xr, sl < rslots ? (PAIR ? 8u * (unsigned)start_pix + 16u * (unsigned)sl : 16u * (unsigned)(start_pix + sl))
                           : kOOB, 0u, sR + q * 1024);
  }
  for (int q = wid; q < wslots_p / 64; q += NW) {
    const int sl = q * 64 + lane;
    blds16(wr, sl < wslots ? 16u * (unsigned)(n0 * taps + sl) : kOOB, 0u, sW + q * 1024);
  }
  const int i = lane & 15, qg = lane >> 4;
  int b_row[FN];
#pragma unroll
  for (int b = 0; b < FN; ++b) b_row[b] = wn * TN + 8 * (i >> 2) + 4 * b + (i & 3);
  wait_vmcnt<0>();
  block_sync_lds();
  const unsigned long long t_dma = dbg ? stamp() : 0;
  unsigned long long t_mfma = 0;
  const int zero_slot = rslots;  // loaded from an out-of-range offset: zeros
  for (int t_ = 0; t_ < mt; ++t_) {
  const int tm = tg * mt + t_, m0 = tm * BM;
  int a_pix[FM];
#pragma unroll
  for (int a = 0; a < FM; ++a) {
    const int m = min(m0 + wm * TM + a * 16 + i, g.M - 1) - mg0;  // group-local output pixel
    a_pix[a] = (m >> g.logW) * g.Wp + (m & (g.W - 1));
  }
  f32x4 acc[FM][FN];
#pragma unroll
  for (int a = 0; a < FM; ++a)
#pragma unroll
    for (int b = 0; b < FN; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int st = 0; st < nsteps; ++st) {
    const int t = 4 * st + qg;  // this lane group's tap (PAIR: tap pair)
    const int kh = PAIR ? t / cpr : t / g.KS, kw = PAIR ? 2 * (t - kh * cpr) : t - kh * g.KS;
    const int toff = kh * g.Wp + kw;
    bf16x8 fa[FM], fb[FN];
#pragma unroll
    for (int a = 0; a < FM; ++a) {
      if constexpr (PAIR) {  // 8-byte pixels: the chunk is pixels q, q+1 (two 8-byte-aligned reads)
        const int q = a_pix[a] + (t < taps ? toff : 0);
        const uint2 lo = *reinterpret_cast<const uint2*>(sR + q * 8);
        const uint2 hi = *reinterpret_cast<const uint2*>(sR + q * 8 + 8);
        const bool ok = t < taps;  // past the last chunk: zeros (the weights there are clamped, not zero)
        fa[a] = __builtin_bit_cast(bf16x8, make_uint4(ok ? lo.x : 0u, ok ? lo.y : 0u, ok ? hi.x : 0u, ok ? hi.y : 0u));
      } else {
        fa[a] = *reinterpret_cast<const bf16x8*>(sR + (t < taps ? a_pix[a] + toff : zero_slot) * 16);
      }
    }
#pragma unroll
    for (int b = 0; b < FN; ++b)
      fb[b] = *reinterpret_cast<const bf16x8*>(sW + (b_row[b] * taps + min(t, taps - 1)) * 16);
#pragma unroll
    for (int a = 0; a < FM; ++a)
#pragma unroll
      for (int b = 0; b < FN; ++b) acc[a][b] = mfma16(fb[b], fa[a], acc[a][b]);
  }
  if (dbg) t_mfma = stamp();
  conv_fwd_epilogue_t<128, BN, STATS, false, WM, WN, FM, FN>(acc, g, y, stats, nullptr, 0, tm, m0, n0, sX);
  }
  if (dbg && threadIdx.x == 0) {
    unsigned long long* d = dbg + (size_t)blockIdx.x * 4;
    d[0] = t_start; d[1] = t_dma; d[2] = t_mfma; d[3] = stamp();
  }
}

}  // namespace dl
