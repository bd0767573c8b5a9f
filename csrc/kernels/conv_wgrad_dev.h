// Weight-gradient implicit-GEMM kernel of conv_igemm.hip.
#pragma once
#include "conv_common_dev.h"
#include "sgd_dev.h"

namespace dl {

// --------------------------------------------------------------------------
// wgrad implicit GEMM: out[split][co][k] = sum_{m in split} dy[m][co] * im2col(x)[m][k]
// Tiles are staged [m][col] (rows = the reduction index) by LDS-DMA and read
// as MFMA operands with ds_read_b64_tr_b16.  BK = 64 rows of m per stage.
// --------------------------------------------------------------------------
// DL_WGRAD_STAMPS builds only (diagnostics): per-workgroup s_memtime phase
// sums of waves 0 and NW-1 -> [wg][2][6] = start, loop begin, sum of the
// steps' wait+barrier, sum of the steps' issue work, loop end, end
__device__ unsigned long long* g_wgrad_stamps = nullptr;

// (Removed in round 6 after losing their A/B: atomic split-K accumulation,
// r2_mode1_timeline.txt; 256x128 tiles, r3_wgrad_tile256_ab.txt; position-major
// steps, r5_wgrad_posm_ab.txt; the read-before-DMA loop order and the
// read-then-compute loop, r3_wgrad_order_ab.txt.)
template <int BM, int BN, int STAGES, int WM = 2, int WN = 2, int BK_ = 64>
__global__ void __launch_bounds__(64 * WM * WN) conv_wgrad_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                         float* __restrict__ out, const ConvGeom g, int m_per_split,
                                                         int ldo, const SgdJob side = SgdJob{}) {
  // side job (dl_ops.h SideJob, as conv_fwd_kernel): the last side.nblk
  // workgroups run part of the step's SGD update beside the weight gradient
  const int wg_grid = (int)gridDim.x - side.nblk;
  if ((int)blockIdx.x >= wg_grid) {
    sgd_side_block(side, (int)blockIdx.x - wg_grid);
    return;
  }
  // dy and x are both spatially zero-padded [B][Hp][Wp][C] (dy: interior at
  // (pad, pad)).  A 64-row M step starts at a multiple of 64 output pixels;
  // with W | 64 and (H*W | 64 or 64 | H*W) the padded position of row r of the
  // step is U(step) + L(r): a wave-uniform part plus a per-lane constant, so
  // a load is one add, no bounds test (m_per_split % 64 == 0, Cout % BM == 0);
  // only a partial last step (M % 64 != 0) tests rows (wave-uniform branch).
  // BK_ = 32 (the 256x128 tile): 32-row steps, which start at multiples of 32
  // -- the host then needs W | 32 for the pow2 decomposition (H*W and 32 are
  // powers of two, so one divides the other)
  constexpr int BK = BK_, NW = WM * WN, PD = STAGES - 1;
  static_assert(BK == 32 || BK == 64, "32- or 64-row steps");
  static_assert(STAGES >= 2 && STAGES <= 8, "2..8 stages");
  constexpr int ACPR = BM / 8, BCPR = BN / 8;  // chunks per LDS row (row = one m)
  constexpr int A_BYTES = BK * BM * 2, B_BYTES = BK * BN * 2, STAGE_BYTES = A_BYTES + B_BYTES;
  constexpr int A_INS = A_BYTES / 1024 / NW, B_INS = B_BYTES / 1024 / NW;
  constexpr int LPS = A_INS + B_INS;
  constexpr int A_RPI = 64 / ACPR, B_RPI = 64 / BCPR;  // rows per glds instruction
  static_assert(A_INS * NW * 1024 == A_BYTES && B_INS * NW * 1024 == B_BYTES, "DMA split");
  constexpr int TM = BM / WM, TN = BN / WN, FM = TM / 16, FN = TN / 16;
  static_assert(A_INS >= 1 && B_INS >= 1, "tile too small");
  __shared__ __attribute__((aligned(1024))) char smem[STAGES * STAGE_BYTES];

#ifdef DL_WGRAD_STAMPS
  unsigned long long st_start = stamp(), st_loop = 0, st_wait = 0, st_work = 0, st_prev = 0, st_lend = 0;
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int ntm = g.Cout / BM, ntn = (g.Kch * 8 + BN - 1) / BN;
  // split-major XCD-aware order: the workgroups of one K split (same dy rows,
  // same x pixels, different taps / channel tiles) get consecutive ids after
  // the swizzle, i.e. one XCD, so the split's rows are fetched into that XCD's
  // L2 once instead of once per XCD (wgrad1 15.3 -> 11.0 us, r2_wgrad_xcd_ab.txt)
  const int id = xcd_swizzle(blockIdx.x, wg_grid);
  const int split = id / (ntm * ntn);
  const int tile = id - split * (ntm * ntn);
  const int tm = tile % ntm, tn = tile / ntm;
  const int co0 = tm * BM, k0 = tn * BN;
  const int mbeg = split * m_per_split;
  const int mend = min(g.M, mbeg + m_per_split);
  const int HW = 1 << g.logHW, Wd = g.W, C8 = 1 << g.logC8;
  const int HpWp = g.Hp * g.Wp;
  // padded pixel offset of row r inside a 64-aligned step (pow2 H, W: the step's
  // pixel decomposes as wave-uniform step base + per-lane row part; otherwise
  // every lane decomposes its own pixel each step, out_pix)
  auto lane_pix = [&](int r) {
    return g.pow2 ? (r >> g.logHW) * HpWp + ((r & (HW - 1)) >> g.logW) * g.Wp + (r & (Wd - 1)) : 0;
  };

  // A (dy) lanes: row = A_RPI*(wid*A_INS + j) + lane/ACPR, chunk fixed
  int a_off[A_INS], a_row[A_INS];
#pragma unroll
  for (int j = 0; j < A_INS; ++j) {
    const int row = A_RPI * (wid * A_INS + j) + lane / ACPR;
    a_row[j] = row;
    const int ch = swz_tr<ACPR>(row, lane % ACPR) - row * ACPR;  // logical chunk (involution)
    a_off[j] = (lane_pix(row) + (g.dsep ? 0 : g.pad * g.Wp + g.pad)) * g.Cout + co0 + ch * 8;
  }
  // B (im2col of x) lanes: chunk -> fixed tap (kh, kw, c0)
  int b_off[B_INS], b_row[B_INS];
  bool b_kok[B_INS];
#pragma unroll
  for (int j = 0; j < B_INS; ++j) {
    const int row = B_RPI * (wid * B_INS + j) + lane / BCPR;
    b_row[j] = row;
    const int ch = swz_tr<BCPR>(row, lane % BCPR) - row * BCPR;
    const int kc = k0 / 8 + ch;
    b_kok[j] = kc < g.Kch;
    const int kpos = kc >> g.logC8;
    const int kh = kpos / g.KW, kw = (kpos - kh * g.KW) * g.kwstep;
    b_off[j] = (lane_pix(row) + kh * g.Wp + kw) * g.Cin + ((kc & (C8 - 1)) << 3);
  }
  const i32x4 dyr = make_rsrc4(dy, (unsigned)((int64_t)g.B * g.dHp * g.dWp * g.Cout * 2));
  const i32x4 xr = make_rsrc4(x, (unsigned)((int64_t)g.B * g.Hp * g.Wp * g.Cin * 2));
  unsigned a_v[A_INS], b_v[B_INS];  // per-lane byte offsets (K-tail lanes: out of range -> zeros)
#pragma unroll
  for (int j = 0; j < A_INS; ++j) a_v[j] = 2u * (unsigned)a_off[j];
#pragma unroll
  for (int j = 0; j < B_INS; ++j) b_v[j] = b_kok[j] ? 2u * (unsigned)b_off[j] : kOOB;

  // One stage's LDS-DMA (branch-free: rows past the end -- a partial last
  // step, or a k-step past nk issued by the unconditional pipeline -- read
  // zeros from an out-of-range offset).
  auto issue = [&](int kt, int slot) {
    char* sA = smem + slot * STAGE_BYTES;
    char* sB = sA + A_BYTES;
    const int ms = mbeg + kt * BK;  // 64-aligned first row of the step
    const int left = mend - ms;     // rows left (uniform)
    if (g.pow2) {
      const int u = (ms >> g.logHW) * HpWp + ((ms & (HW - 1)) >> g.logW) * g.Wp;  // wave-uniform
      const unsigned ua = 2u * (unsigned)(u * g.Cout), ub = 2u * (unsigned)(u * g.Cin);
#pragma unroll
      for (int j = 0; j < A_INS; ++j)
        blds16_asm(dyr, a_row[j] < left ? a_v[j] : kOOB, ua, sA + (wid * A_INS + j) * 1024);
#pragma unroll
      for (int j = 0; j < B_INS; ++j)
        blds16_asm(xr, b_row[j] < left ? b_v[j] : kOOB, ub, sB + (wid * B_INS + j) * 1024);
    } else {
#pragma unroll
      for (int j = 0; j < A_INS; ++j) {
        const bool ok = a_row[j] < left;
        const int mr = ok ? ms + a_row[j] : 0;
        const int px = g.dsep ? dy_pix(g, mr) : out_pix(g, mr);
        blds16_asm(dyr, ok ? a_v[j] + 2u * (unsigned)(px * g.Cout) : kOOB, 0u, sA + (wid * A_INS + j) * 1024);
      }
#pragma unroll
      for (int j = 0; j < B_INS; ++j) {
        const bool ok = b_row[j] < left;
        const int px = out_pix(g, ok ? ms + b_row[j] : 0);
        blds16_asm(xr, ok && b_v[j] != kOOB ? b_v[j] + 2u * (unsigned)(px * g.Cin) : kOOB, 0u,
                   sB + (wid * B_INS + j) * 1024);
      }
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int gq = lane >> 4, q4 = (lane & 15) >> 2, p4 = lane & 3;
  const int nk = max(0, (mend - mbeg + BK - 1) / BK);
  // (as conv_fwd_region_kernel) every step issues one stage unconditionally,
  // fragments of step i+1 are read (transposed LDS reads) while the MFMAs of
  // step i run, interleaved 1:1 -- needs >= 4 stages to keep DMA lookahead
  static_assert(STAGES >= 3, "fragment prefetch needs >= 3 ring slots");
#pragma unroll
  for (int p = 0; p < PD; ++p) issue(p, p);
  int rslot = 0, dslot = PD % STAGES;
  auto read_frags = [&](bf16x8 (&af)[BK / 32][FM], bf16x8 (&bf)[BK / 32][FN]) {
    const char* As = smem + rslot * STAGE_BYTES;
    const char* Bs = As + A_BYTES;
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      const int r0 = kk * 32 + gq * 8 + q4;
#pragma unroll
      for (int a = 0; a < FM; ++a) {
        const int col = wm * TM + a * 16 + 4 * p4;
        const int ch = col >> 3, sub = (col & 7) * 2;
        s16x4 lo = ds_read_tr16(As + swz_tr<ACPR>(r0, ch) * 16 + sub);
        s16x4 hi = ds_read_tr16(As + swz_tr<ACPR>(r0 + 4, ch) * 16 + sub);
        af[kk][a] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int b = 0; b < FN; ++b) {
        const int col = wn * TN + b * 16 + 4 * p4;
        const int ch = col >> 3, sub = (col & 7) * 2;
        s16x4 lo = ds_read_tr16(Bs + swz_tr<BCPR>(r0, ch) * 16 + sub);
        s16x4 hi = ds_read_tr16(Bs + swz_tr<BCPR>(r0 + 4, ch) * 16 + sub);
        bf[kk][b] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
    }
    ++rslot;
    rslot -= (rslot == STAGES) * STAGES;
  };
  constexpr int NRD = (BK / 32) * (FM + FN) * 2;  // ds_read_b64_tr_b16 per step
  constexpr int NMF = (BK / 32) * FM * FN;
  bf16x8 fa0[BK / 32][FM], fb0[BK / 32][FN], fa1[BK / 32][FM], fb1[BK / 32][FN];
  {
  wait_vmcnt<(PD - 1) * LPS>();  // stage 0 landed
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  read_frags(fa0, fb0);
  int kt_next = PD;
  // The step's LDS-DMA is issued right after the barrier, BEFORE the
  // fragment reads.  The asm DMA carries a memory
  // clobber, so reads issued before it cannot move past it: in the old order
  // (reads, DMA, MFMAs) the 24 reads were bunched ahead of all MFMAs and the
  // compiler hoisted the next step's lgkmcnt(0) + barrier to after the 4th
  // MFMA -- the reads' latency was covered by 4 MFMAs and the other 12 ran
  // with no reads beside them.  DMA first, the reads and MFMAs share one
  // scheduling region and interleave (MFMA, 2 reads) as the group barriers
  // ask, and a closing sched_barrier keeps the next barrier after them.
  auto step = [&](bf16x8 (&fca)[BK / 32][FM], bf16x8 (&fcb)[BK / 32][FN], bf16x8 (&fna)[BK / 32][FM],
                  bf16x8 (&fnb)[BK / 32][FN]) {
#ifdef DL_WGRAD_STAMPS
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long sa = stamp();
    __builtin_amdgcn_sched_barrier(0);
#endif
    wait_vmcnt<(PD - 2) * LPS>();        // stage i+1 landed
    __builtin_amdgcn_s_waitcnt(0xC07F);  // step i's fragments in registers (compiler-visible wait)
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
#ifdef DL_WGRAD_STAMPS
    {
      const unsigned long long sb = stamp();
      __builtin_amdgcn_sched_barrier(0);
      st_wait += sb - sa;
      if (st_prev) st_work += sa - st_prev;
      st_prev = sb;
    }
#endif
    issue(kt_next, dslot);  // into the slot read two steps ago
    ++kt_next;
    ++dslot;
    dslot -= (dslot == STAGES) * STAGES;
    __builtin_amdgcn_sched_barrier(0);
    read_frags(fna, fnb);
    // C^T (k x co): lane holds 4 consecutive k of one co -> 16-byte stores
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk)
#pragma unroll
      for (int a = 0; a < FM; ++a)
#pragma unroll
        for (int b = 0; b < FN; ++b) acc[a][b] = mfma16(fcb[kk][b], fca[kk][a], acc[a][b]);
    constexpr int P1 = NRD / 2 < NMF ? NRD / 2 : NMF;  // (MFMA, 2 reads) pairs
#pragma unroll
    for (int q = 0; q < P1; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    }
    if constexpr (NRD > 2 * P1) __builtin_amdgcn_sched_group_barrier(0x100, NRD - 2 * P1, 0);
    if constexpr (NMF > P1) __builtin_amdgcn_sched_group_barrier(0x008, NMF - P1, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  int i = 0;
#ifdef DL_WGRAD_STAMPS
  st_loop = stamp();
#endif
  for (; i + 1 < nk; i += 2) {
    step(fa0, fb0, fa1, fb1);
    step(fa1, fb1, fa0, fb0);
  }
  if (i < nk) step(fa0, fb0, fa1, fb1);
  }

#ifdef DL_WGRAD_STAMPS
  st_lend = stamp();
  struct StampOut {
    unsigned long long* p;
    unsigned long long v[5];
    int w;
    __device__ ~StampOut() {
      if (p && (threadIdx.x & 63) == 0 && (w == 0 || w == (int)(blockDim.x >> 6) - 1)) {
        unsigned long long* d = p + ((size_t)(blockIdx.x + blockIdx.y * gridDim.x) * 2 + (w ? 1 : 0)) * 6;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3]; d[4] = v[4]; d[5] = stamp();
      }
    }
  } stamp_out{g_wgrad_stamps, {st_start, st_loop, st_wait, st_work, st_lend}, wid};
#endif
  const int col_l = lane & 15, rq = lane >> 4;
  float* o = out + (int64_t)split * g.Cout * ldo;
  if constexpr (BN >= 128) {  // (64-wide tiles: measured no gain)
    // Slab rows through LDS: straight from the accumulators a store
    // instruction writes 16 rows x 64 B; staged, every instruction writes whole
    // BN*4-byte rows (64 lanes x 16 B).  The C^T tile goes into the (drained)
    // DMA ring as [co][k] fp32 with a 16-byte row pad (row stride 2^n + 16 B:
    // the 16 co rows of a store group fall on distinct banks).
    constexpr int LROW = BN + 4;
    static_assert(BM * LROW * 4 <= STAGES * STAGE_BYTES, "staged slab tile fits the ring");
    wait_vmcnt<0>();  // the unconditional pipeline's trailing (zero-fill) DMAs still target the ring
    block_sync_lds();
    float* st = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int a = 0; a < FM; ++a)
#pragma unroll
      for (int b = 0; b < FN; ++b)
        *reinterpret_cast<float4*>(st + (wm * TM + a * 16 + col_l) * LROW + wn * TN + b * 16 + rq * 4) =
            make_float4(acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]);
    block_sync_lds();
    constexpr int C4 = BN / 4, NTH = 64 * NW;  // 16-byte chunks per row, threads
    static_assert(BM * C4 % NTH == 0, "whole store passes");
#pragma unroll
    for (int i = 0; i < BM * C4 / NTH; ++i) {
      const int idx = tid + i * NTH, r = idx / C4, c4 = idx - r * C4;
      const int co = co0 + r, k = k0 + 4 * c4;
      if (co < g.Cout && k < ldo)
        *reinterpret_cast<float4*>(o + (int64_t)co * ldo + k) =
            *reinterpret_cast<const float4*>(st + r * LROW + 4 * c4);
    }
    return;
  }
#pragma unroll
  for (int a = 0; a < FM; ++a)
#pragma unroll
    for (int b = 0; b < FN; ++b) {
      const int k = k0 + wn * TN + b * 16 + rq * 4;
      const int co = co0 + wm * TM + a * 16 + col_l;
      if (co < g.Cout && k < ldo)  // ldo % 4 == 0 and k % 4 == 0: the 4-run is in bounds
        *reinterpret_cast<float4*>(o + (int64_t)co * ldo + k) =
            make_float4(acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]);
    }
}

}  // namespace dl
