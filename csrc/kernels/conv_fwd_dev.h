// Streaming forward / dgrad implicit-GEMM kernel of conv_igemm.hip, and the
// stand-alone combine of its split-K slabs.
#pragma once
#include "conv_common_dev.h"
#include "sgd_dev.h"

namespace dl {

// --------------------------------------------------------------------------
// forward / dgrad implicit GEMM, split-K capable
//   C[m][n] = sum_{k in split} im2col(x)[m][k] * w[n][k]
//   splits == 1: bf16 y (+ BN partial sums per M tile)   splits > 1: fp32 slab[split][M][N]
// 256 threads = 4 waves (2 x 2), wave tile (BM/2) x (BN/2), BK = 64,
// 3-stage LDS ring filled by LDS-DMA, one barrier per K step.
// --------------------------------------------------------------------------
// FIX: split-K with the in-launch combine (splitk_fixup): `slab` holds the
// slices, the reducer of each tile runs the plain (STATS / BNR) epilogue;
// fixcnt = the launch's per-tile arrival counters.
template <int BM, int BN, bool STATS, bool SLAB, bool TAPU, int STAGES, int WM = 2, int WN = 2, bool ADD = false,
          bool TRP = true, int BNR = 0, bool FIX = false>
__global__ void __launch_bounds__(64 * WM * WN) conv_fwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                       bf16_t* __restrict__ y, float* __restrict__ stats,
                                                       float* __restrict__ slab, const ConvGeom g, int splits,
                                                       int kt_per_split, unsigned long long* dbg,
                                                       const BnRedArgs br = BnRedArgs{},
                                                       const SgdJob side = SgdJob{},
                                                       int* __restrict__ fixcnt = nullptr) {
  // side job (dl_ops.h SideJob): the last side.nblk workgroups run part of
  // the step's SGD update on the CUs the convolution's one-workgroup-per-CU
  // grid leaves free (its gradients are final by the time this conv runs)
  const int conv_grid = (int)gridDim.x - side.nblk;
  if ((int)blockIdx.x >= conv_grid) {
    sgd_side_block(side, (int)blockIdx.x - conv_grid);
    return;
  }
  // x is the SPATIALLY ZERO-PADDED input [B][Hp][Wp][Cin]: every tap of every
  // output pixel is in bounds, so an activation load is (per-lane pixel base)
  // + (wave-uniform tap offset) with no bounds test.  Cout % BN == 0
  // (host-checked); rows of an M tail load a valid pixel and are masked out
  // of the stores and BN statistics.
  const unsigned long long t_start = dbg ? stamp() : 0ull;
  constexpr int BK = 64, CPR = 8, NW = WM * WN, PD = STAGES - 1;
  static_assert(STAGES >= 2 && STAGES <= 4, "2..4 stages");
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE_BYTES = A_BYTES + B_BYTES;
  constexpr int A_INS = A_BYTES / 1024 / NW, B_INS = B_BYTES / 1024 / NW;  // glds per wave per stage
  constexpr int LPS = A_INS + B_INS;
  constexpr int TM = BM / WM, TN = BN / WN, FM = TM / 16, FN = TN / 16;
  // transposed accumulators (16-byte epilogue stores) unless FN is odd (TRP = false: the old layout)
  constexpr bool TR = TRP && FN % 2 == 0;
  static_assert(A_INS >= 1 && B_INS >= 1, "tile too small");
  static_assert(A_INS * NW * 1024 == A_BYTES && B_INS * NW * 1024 == B_BYTES, "DMA split");
  __shared__ __attribute__((aligned(1024))) char smem[STAGES * STAGE_BYTES];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int ntm = (g.M + BM - 1) / BM;
  // Panel-major order: the workgroups of one XCD (consecutive ids after the
  // swizzle) share one (n-tile, K-split) weight panel and sweep the M tiles,
  // so the panel is fetched into that XCD's L2 once instead of every XCD
  // streaming the whole weight tensor from the Infinity Cache.
  // (M-tile-major measured 0.8 % slower, r2_fwd_order_ab.txt; per-pixel
  // balanced position-major split-K no faster, r2_posm_balance_ab.txt: both
  // removed in round 6)
  const int npanel = (g.Cout / BN) * splits;
  const int id = xcd_swizzle(blockIdx.x, ntm * npanel);
  const int tm = id % ntm;
  const int panel = id / ntm;
  const int split = panel % splits;
  const int tn = panel / splits;
  const int m0 = tm * BM, n0 = tn * BN;
  const int C8 = 1 << g.logC8;
  // Position-major tiles (g.posm, host-enabled for TAPU layers whose output is
  // smaller than twice the kernel, B % BM == 0): M tile tm holds images b0..b0+BM-1
  // at ONE output pixel, so every row of the tile has the same valid taps and
  // the taps that only read the zero border are skipped (4x4 output, 5x5
  // kernel: 9-16 of 25 taps per pixel).  K steps are split evenly per tile.
  int pm_b0 = 0, pm_pos = 0, kh0 = 0, kh1 = g.KS, kw0 = 0, kw1 = g.KS;
  int nkt_total = (g.Kch + CPR - 1) / CPR, ktps = kt_per_split;
  if (TAPU && g.posm) {
    const int nbt = g.B / BM;
    pm_pos = tm / nbt;
    pm_b0 = (tm - pm_pos * nbt) * BM;
    const int oh = pm_pos / g.W, ow = pm_pos - oh * g.W;
    kh0 = max(0, g.pad - oh);
    kh1 = min(g.KS, g.H + g.pad - oh);
    kw0 = max(0, g.pad - ow);
    kw1 = min(g.KS, g.W + g.pad - ow);
    nkt_total = (kh1 - kh0) * (kw1 - kw0) * (g.Cin / BK);
    ktps = (nkt_total + splits - 1) / splits;
  }
  const int kt_beg = split * ktps;
  const int kt_end = min(nkt_total, kt_beg + ktps);
  const int nk = max(0, kt_end - kt_beg);

  // per-lane source roles (fixed over the K loop); 32-bit element offsets.
  // A: instruction j of this wave covers rows 8*(wid*A_INS + j) .. +7;
  //    a_base = padded pixel of tap (0,0) of output pixel m (+ chunk for TAPU)
  int a_base[A_INS], a_ch[A_INS];
#pragma unroll
  for (int j = 0; j < A_INS; ++j) {
    const int row = 8 * (wid * A_INS + j) + (lane >> 3);
    a_ch[j] = (lane & 7) ^ ((row >> 1) & 7);
    const int m = (TAPU && g.posm) ? (pm_b0 + row) * (g.H * g.W) + pm_pos
                                   : min(m0 + row, g.M - 1);  // M tail: any valid pixel (masked in the epilogue)
    a_base[j] = out_pix(g, m) * g.Cin + (TAPU ? a_ch[j] * 8 : 0);
  }
  int b_off[B_INS], b_k[B_INS];
#pragma unroll
  for (int j = 0; j < B_INS; ++j) {
    const int row = 8 * (wid * B_INS + j) + (lane >> 3);
    const int ch = (lane & 7) ^ swz_b(row);
    b_k[j] = ch * 8;
    b_off[j] = (n0 + row) * g.K + ch * 8;
  }
  const rsrc_t xr = make_rsrc(x, (unsigned)((int64_t)g.B * g.Hp * g.Wp * g.Cin * 2));
  const rsrc_t wr = make_rsrc(w, (unsigned)((int64_t)g.Cout * g.K * 2));

  // Wave-uniform tap state of the next K step to load (TAPU: one step = 64
  // channels of one tap): off = (kh*Wp + kw)*Cin + c0 (activation), wk =
  // (kh*KS + kw)*Cin + c0 (weight column), advanced incrementally (no
  // divisions in the loop).
  struct Tap { int off, c0, kw, kh, wk; };
  Tap tnext{0, 0, 0, 0, 0};
  if constexpr (TAPU) {
    int kh, kw;
    if (g.posm) {
      const int chunks = g.Cin / BK, t = kt_beg / chunks, nkw = kw1 - kw0;
      tnext.c0 = (kt_beg - t * chunks) * BK;
      kh = kh0 + t / nkw;
      kw = kw0 + (t - (t / nkw) * nkw);
    } else {
      const int k0 = kt_beg * BK;
      const int kpos = k0 >> (g.logC8 + 3);
      kh = kpos / g.KW;
      kw = kpos - kh * g.KW;
      tnext.c0 = k0 & (g.Cin - 1);
    }
    tnext.kw = kw;
    tnext.kh = kh;
    tnext.off = (kh * g.Wp + kw) * g.Cin + tnext.c0;
    tnext.wk = (kh * g.KW + kw) * g.Cin + tnext.c0;
  }
  auto tap_advance = [&](Tap& t) {
    if constexpr (TAPU) {
      t.off += BK;
      t.wk += BK;
      t.c0 += BK;
      if (t.c0 == g.Cin) {
        t.c0 = 0;
        if (g.posm) {  // next valid tap of the tile's window
          if (++t.kw == kw1) { t.kw = kw0; ++t.kh; }
          t.off = (t.kh * g.Wp + t.kw) * g.Cin;
          t.wk = (t.kh * g.KS + t.kw) * g.Cin;
        } else if (++t.kw == g.KW) {
          t.kw = 0;
          t.off += (g.Wp - g.KW) * g.Cin;
        }
      }
    }
  };
  // One LDS-DMA load (q < A_INS: activation row block, else weight row block)
  // of K step kt into ring slot `slot`.
  auto issue_one = [&](int q, int kt, int slot, const Tap& t) {
    char* sA = smem + slot * STAGE_BYTES;
    char* sB = sA + A_BYTES;
    if (q < A_INS) {
      const int j = q;
      if constexpr (TAPU) {
        blds16(xr, 2u * (unsigned)a_base[j], 2u * (unsigned)t.off, sA + (wid * A_INS + j) * 1024);
      } else {
        // first layer (Cin < 64): a 64-wide K step spans several taps, per lane
        const int kc = kt * CPR + a_ch[j];
        const int kpos = kc >> g.logC8;
        const int c0 = (kc & (C8 - 1)) << 3;
        const int kh = kpos / g.KW, kw = kpos - kh * g.KW;
        const unsigned off = kc < g.Kch ? 2u * (unsigned)(a_base[j] + (kh * g.Wp + kw) * g.Cin + c0) : kOOB;
        blds16(xr, off, 0u, sA + (wid * A_INS + j) * 1024);
      }
    } else {
      const int j = q - A_INS;
      const int kadd = TAPU ? t.wk : kt * BK;
      unsigned voff = 2u * (unsigned)b_off[j];
      if constexpr (!TAPU) voff = (kadd + b_k[j]) < g.K ? voff : kOOB;  // K tail (first layer only)
      blds16(wr, voff, 2u * (unsigned)kadd, sB + (wid * B_INS + j) * 1024);
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const unsigned long long t_setup = dbg ? stamp() : 0ull;
  // Fragment-prefetch pipeline (g_fwd_pf, STAGES >= 3): every step issues one
  // stage unconditionally (zero-fill past nk keeps the vmcnt count constant),
  // right after the barrier and before the fragment reads (asm DMA: the reads
  // cannot be hoisted above it, and hipcc's LDS-DMA alias waits stay out);
  // the fragments of step i+1 are read while the MFMAs of step i run.  The
  // plain loop below read each step's fragments and waited for them before
  // its first MFMA: the LDS latency was exposed at every step.
  // (4 stages: two in flight beyond the one being read; at 3 the step waited
  // for the stage issued one step earlier: 0.352 vs 0.341 ms/step, at 4 0.336)
  bool done = false;
  if constexpr (STAGES >= 4) {
    if (g_fwd_pf) {
      done = true;
      const i32x4 xr4 = make_rsrc4(x, (unsigned)((int64_t)g.B * g.Hp * g.Wp * g.Cin * 2));
      const i32x4 wr4 = make_rsrc4(w, (unsigned)((int64_t)g.Cout * g.K * 2));
      auto issue_stage = [&](int kt, int slot, bool valid) {
        char* sA = smem + slot * STAGE_BYTES;
        char* sB = sA + A_BYTES;
#pragma unroll
        for (int j = 0; j < A_INS; ++j) {
          if constexpr (TAPU) {
            blds16_asm(xr4, valid ? 2u * (unsigned)a_base[j] : kOOB, valid ? 2u * (unsigned)tnext.off : 0u,
                       sA + (wid * A_INS + j) * 1024);
          } else {
            const int kc = kt * CPR + a_ch[j];
            const int kpos = kc >> g.logC8;
            const int c0 = (kc & (C8 - 1)) << 3;
            const int kh = kpos / g.KW, kw = kpos - kh * g.KW;
            const unsigned off =
                (valid && kc < g.Kch) ? 2u * (unsigned)(a_base[j] + (kh * g.Wp + kw) * g.Cin + c0) : kOOB;
            blds16_asm(xr4, off, 0u, sA + (wid * A_INS + j) * 1024);
          }
        }
#pragma unroll
        for (int j = 0; j < B_INS; ++j) {
          const int kadd = TAPU ? tnext.wk : kt * BK;
          unsigned voff = 2u * (unsigned)b_off[j];
          if constexpr (!TAPU) voff = (kadd + b_k[j]) < g.K ? voff : kOOB;
          blds16_asm(wr4, valid ? voff : kOOB, valid ? 2u * (unsigned)kadd : 0u, sB + (wid * B_INS + j) * 1024);
        }
        if (valid) tap_advance(tnext);
      };
      auto read_frags = [&](int slot, bf16x8 (&af)[BK / 32][FM], bf16x8 (&bfr)[BK / 32][FN]) {
        const uint4* As = reinterpret_cast<const uint4*>(smem + slot * STAGE_BYTES);
        const uint4* Bs = reinterpret_cast<const uint4*>(smem + slot * STAGE_BYTES + A_BYTES);
#pragma unroll
        for (int kk = 0; kk < BK / 32; ++kk) {
          const int ch = kk * 4 + (lane >> 4);
#pragma unroll
          for (int a = 0; a < FM; ++a)
            af[kk][a] = __builtin_bit_cast(bf16x8, As[swz_row<CPR>(wm * TM + a * 16 + (lane & 15), ch)]);
#pragma unroll
          for (int b = 0; b < FN; ++b) {
            const int row = wn * TN + (TR ? b_frag_row(b, lane & 15) : b * 16 + (lane & 15));
            bfr[kk][b] = __builtin_bit_cast(bf16x8, Bs[row * CPR + (ch ^ swz_b(row))]);
          }
        }
      };
#pragma unroll
      for (int p = 0; p < PD; ++p) issue_stage(kt_beg + p, p, p < nk);
      constexpr int NRD = (BK / 32) * (FM + FN);  // ds_read_b128 per step
      constexpr int NMF = (BK / 32) * FM * FN;
      bf16x8 fa0[BK / 32][FM], fb0[BK / 32][FN], fa1[BK / 32][FM], fb1[BK / 32][FN];
      wait_vmcnt<(PD - 1) * LPS>();  // stage 0 landed
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      read_frags(0, fa0, fb0);
      int kt_next = kt_beg + PD, slot_n = PD % STAGES, slot_r = 1 % STAGES;
      auto step = [&](int i, bf16x8 (&fca)[BK / 32][FM], bf16x8 (&fcb)[BK / 32][FN], bf16x8 (&fna)[BK / 32][FM],
                      bf16x8 (&fnb)[BK / 32][FN]) {
        wait_vmcnt<(PD - 2) * LPS>();        // stage i+1 landed
        __builtin_amdgcn_s_waitcnt(0xC07F);  // step i's fragments in registers
        __builtin_amdgcn_s_barrier();        // every wave done reading slot i-1
        __builtin_amdgcn_sched_barrier(0);
        issue_stage(kt_next, slot_n, i + PD < nk);
        ++kt_next;
        slot_n = slot_n + 1 == STAGES ? 0 : slot_n + 1;
        __builtin_amdgcn_sched_barrier(0);
        read_frags(slot_r, fna, fnb);  // (past nk: zeros, never used)
        slot_r = slot_r + 1 == STAGES ? 0 : slot_r + 1;
#pragma unroll
        for (int kk = 0; kk < BK / 32; ++kk)
#pragma unroll
          for (int a = 0; a < FM; ++a)
#pragma unroll
            for (int b = 0; b < FN; ++b)
              acc[a][b] = TR ? mfma16(fcb[kk][b], fca[kk][a], acc[a][b]) : mfma16(fca[kk][a], fcb[kk][b], acc[a][b]);
        constexpr int P1 = NRD < NMF ? NRD : NMF;  // (MFMA, read) pairs
#pragma unroll
        for (int q = 0; q < P1; ++q) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        if constexpr (NRD > P1) __builtin_amdgcn_sched_group_barrier(0x100, NRD - P1, 0);
        if constexpr (NMF > P1) __builtin_amdgcn_sched_group_barrier(0x008, NMF - P1, 0);
        __builtin_amdgcn_sched_barrier(0);
      };
      int i = 0;
      for (; i + 1 < nk; i += 2) {
        step(i, fa0, fb0, fa1, fb1);
        step(i + 1, fa1, fb1, fa0, fb0);
      }
      if (i < nk) step(i, fa0, fb0, fa1, fb1);
      wait_vmcnt<0>();  // the trailing zero-fill DMAs still target the ring (the epilogue reuses it)
    }
  }
  if (!done) {
#pragma unroll
    for (int p = 0; p < PD; ++p)
      if (p < nk) {
#pragma unroll
        for (int q = 0; q < LPS; ++q) issue_one(q, kt_beg + p, p, tnext);
        tap_advance(tnext);
      }
    // MFMAs per K step and the spacing of the next stage's DMA issues between them
    constexpr int NMF = (BK / 32) * FM * FN;
    constexpr int IL = NMF / LPS > 0 ? NMF / LPS : 1;
    int slot_c = 0, slot_n = PD % STAGES;
    auto kstep = [&](int i) {
      block_sync_lds();  // stage i landed for every wave; slot (i+PD)%STAGES no longer read
      const bool pf = i + PD < nk;
      const int kt_n = kt_beg + i + PD;
      const uint4* As = reinterpret_cast<const uint4*>(smem + slot_c * STAGE_BYTES);
      const uint4* Bs = reinterpret_cast<const uint4*>(smem + slot_c * STAGE_BYTES + A_BYTES);
      bf16x8 af[BK / 32][FM], bfr[BK / 32][FN];
#pragma unroll
      for (int kk = 0; kk < BK / 32; ++kk) {
        const int ch = kk * 4 + (lane >> 4);
#pragma unroll
        for (int a = 0; a < FM; ++a)
          af[kk][a] = __builtin_bit_cast(bf16x8, As[swz_row<CPR>(wm * TM + a * 16 + (lane & 15), ch)]);
#pragma unroll
        for (int b = 0; b < FN; ++b) {
          const int row = wn * TN + (TR ? b_frag_row(b, lane & 15) : b * 16 + (lane & 15));
          bfr[kk][b] = __builtin_bit_cast(bf16x8, Bs[row * CPR + (ch ^ swz_b(row))]);
        }
      }
      // the next stage's LDS-DMA issues ride between the MFMAs (their issue cost
      // overlaps matrix-core execution instead of serialising in front of it)
#pragma unroll
      for (int kk = 0; kk < BK / 32; ++kk)
#pragma unroll
        for (int a = 0; a < FM; ++a)
#pragma unroll
          for (int b = 0; b < FN; ++b) {
            acc[a][b] = TR ? mfma16(bfr[kk][b], af[kk][a], acc[a][b]) : mfma16(af[kk][a], bfr[kk][b], acc[a][b]);
            const int idx = (kk * FM + a) * FN + b;
            if (idx % IL == IL - 1 && idx / IL < LPS) {
              if (pf) issue_one(idx / IL, kt_n, slot_n, tnext);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
      if (pf) tap_advance(tnext);
      slot_c = slot_c + 1 == STAGES ? 0 : slot_c + 1;
      slot_n = slot_n + 1 == STAGES ? 0 : slot_n + 1;
    };
    // steady state (constant wait: stage i landed, PD-1 younger stages in flight), then the drain
    int i = 0;
    for (; i < nk - (PD - 1); ++i) {
      wait_vmcnt<(PD - 1) * LPS>();
      kstep(i);
    }
    for (; i < nk; ++i) {
      wait_stages<LPS>(nk - 1 - i);
      kstep(i);
    }

  }

  const unsigned long long t_loop = dbg ? stamp() : 0ull;
  auto dbg_out = [&]() {
    if (dbg && threadIdx.x == 0) {
      unsigned long long* d = dbg + (size_t)blockIdx.x * 4;
      d[0] = t_start; d[1] = t_setup; d[2] = t_loop; d[3] = stamp();
    }
  };
  static_assert(BNR == 0 || TR, "the fused BN reduce needs the transposed epilogue");
  if constexpr (FIX) {
    static_assert(TR && !SLAB && !ADD, "FIX: transposed plain epilogue after the in-launch combine");
    if (!splitk_fixup<BM, BN, WM, WN, FM, FN>(acc, g, slab, split, splits, m0, n0, pm_b0, pm_pos, fixcnt + tn * ntm + tm,
                                              smem)) {
      dbg_out();
      return;
    }
  }
  if constexpr (TR)
    conv_fwd_epilogue_t<BM, BN, STATS, SLAB, WM, WN, FM, FN, ADD, BNR>(acc, g, y, stats, slab, split, tm, m0, n0, smem,
                                                                       pm_b0, pm_pos, br);
  else
    conv_fwd_epilogue<BM, BN, STATS, SLAB, WM, WN, ADD>(acc, g, y, stats, slab, split, tm, m0, n0, smem, pm_b0,
                                                        pm_pos);
  dbg_out();
}

// split-K combine: y = bf16(sum_s slab[s]) (+ BN partial sums, one row per block)
template <bool STATS>
__global__ void __launch_bounds__(256) splitk_combine_kernel(const float* __restrict__ slab, bf16_t* __restrict__ y,
                                                             float* __restrict__ stats, int splits, int M, int N,
                                                             int rows_per_block, const ConvGeom g) {
  const int N8 = N >> 3;
  const int tpr = N8;                 // threads per row (one 8-column chunk each)
  const int rpi = 256 / tpr;          // rows per iteration
  const int c8 = threadIdx.x % tpr, rsub = threadIdx.x / tpr;
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = min(M, r0 + rows_per_block);
  float s1[8], s2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { s1[k] = 0.f; s2[k] = 0.f; }
  if (rsub < rpi) {
    for (int m = r0 + rsub; m < r1; m += rpi) {
      const int splits_m = splits;
      float v[8];
      const float* p = slab + (int64_t)m * N + c8 * 8;
      {
        const float4 a = *reinterpret_cast<const float4*>(p);
        const float4 b = *reinterpret_cast<const float4*>(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
      }
      // splits in batches of 4 with every load of a batch issued before the
      // first add (a load->add chain per split was latency-bound); the adds
      // keep the split order
      auto add8 = [&](const float4& a, const float4& b) {
        v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
      };
      int s = 1;
      for (; s + 3 < splits_m; s += 4) {
        float4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float* q = p + (int64_t)(s + u) * M * N;
          a[u] = *reinterpret_cast<const float4*>(q);
          b[u] = *reinterpret_cast<const float4*>(q + 4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) add8(a[u], b[u]);
      }
      for (; s < splits_m; ++s) {
        const float* q = p + (int64_t)s * M * N;
        add8(*reinterpret_cast<const float4*>(q), *reinterpret_cast<const float4*>(q + 4));
      }
      uint4 o;
      o.x = pack_bf16x2(v[0], v[1]); o.y = pack_bf16x2(v[2], v[3]);
      o.z = pack_bf16x2(v[4], v[5]); o.w = pack_bf16x2(v[6], v[7]);
      *reinterpret_cast<uint4*>(y + (int64_t)m * N + c8 * 8) = o;
      if constexpr (STATS) {
        const float h[8] = {lo_bf16(o.x), hi_bf16(o.x), lo_bf16(o.y), hi_bf16(o.y),
                            lo_bf16(o.z), hi_bf16(o.z), lo_bf16(o.w), hi_bf16(o.w)};
#pragma unroll
        for (int k = 0; k < 8; ++k) { s1[k] += h[k]; s2[k] += h[k] * h[k]; }
      }
    }
  }
  if constexpr (STATS) {
    __shared__ float red[256][17];
#pragma unroll
    for (int k = 0; k < 8; ++k) { red[threadIdx.x][k] = s1[k]; red[threadIdx.x][8 + k] = s2[k]; }
    __syncthreads();
    for (int c = threadIdx.x; c < N; c += 256) {
      const int ch = c >> 3, k = c & 7;
      float a = 0.f, b = 0.f;
      for (int t = ch; t < rpi * tpr; t += tpr) { a += red[t][k]; b += red[t][8 + k]; }
      put_stats(stats, blockIdx.x, N, c, a, b);
    }
  }
}

}  // namespace dl
