// Implicit-GEMM convolution on CDNA4 matrix cores (gfx950, bf16 in, fp32 acc).
//
// Replaces the reference's cunn SpatialConvolutionMM (im2col + cuBLAS GEMM;
// examples/cifar10.lua:108-126, examples/mnist.lua:57-62).
// Layouts are chosen for MFMA, not copied from Torch:
//   activations NHWC (channels-last), weights KRSC = [Cout][KS][KS][Cin].
// Then, for a stride-1 "same" convolution with M = B*H*W, N = Cout,
// K = KS*KS*Cin and k = (kh*KS + kw)*Cin + c:
//   forward  y[m][n]  = sum_k im2col(x)[m][k] * W[n][k]          (A gathered, B K-major)
//   dgrad    dx       = forward(dy, W') with W'[ci][kh][kw][co] = W[co][KS-1-kh][KS-1-kw][ci]
//   wgrad    dW[n][k] = sum_m dy[m][n] * im2col(x)[m][k]          (reduction over m)
// Cin is a power of two >= 8 (the 3-channel input layer is zero-padded to 8),
// so every 16-byte chunk of K (8 channels) lies inside one (kh, kw) tap and is
// one aligned vector load; padding taps and K tails load zeros.
//
// Kernels use v_mfma_f32_16x16x32_bf16 (lane l: A[l&15][8(l>>4)+j],
// B[8(l>>4)+j][l&15], C/D col = l&15, row = 4(l>>4)+j), 256-thread workgroups
// (2x2 waves of 64 lanes), register-staged double-buffered LDS tiles with XOR
// swizzles so that the fragment reads are bank-conflict free:
//   * forward / dgrad: both operands K-contiguous -> ds_read_b128 row reads;
//   * wgrad: both operands have the reduction index (m) as the *row* index of
//     an NHWC tensor -> tiles are staged [m][col] and read with the gfx950
//     hardware transpose ds_read_b64_tr_b16 (no shuffles).
// The forward epilogue also produces the per-channel sum / sum-of-squares
// partials of the bf16 output for train-mode BatchNorm (fused, deterministic:
// one partial row per M tile, reduced by bn_finalize).
//
// This file is the host dispatch; the kernels are in the conv_*_dev.h headers
// below, which only this translation unit includes.
#include "dl_common.h"
#include "dl_ops.h"
#include "conv_common_dev.h"
#include "conv_fwd_dev.h"
#include "conv_region_dev.h"
#include "conv_wgrad_dev.h"
#include "conv_layout_dev.h"

#include <algorithm>
#include <vector>

namespace dl {

static unsigned long long* g_conv_dbg = nullptr;  // debug: per-workgroup s_memtime stamps

static void launch_prep(PrepArgs& a, int64_t P, uintptr_t w1, uintptr_t w1p, int w1_cout, int taps, int w1_c,
                        int w1_cp, const std::vector<uintptr_t>& tw, const std::vector<uintptr_t>& twt,
                        const std::vector<int>& tcout, const std::vector<int>& tcin,
                        const std::vector<uintptr_t>& zp, const std::vector<int64_t>& zn, uintptr_t stream) {
  prep_set_zero(a, zp, zn);
  prep_set_pad(a, P);
  a.w1 = (const float*)w1; a.w1p = (bf16_t*)w1p; a.w1_cout = w1_cout; a.taps = taps; a.w1_c = w1_c; a.w1_cp = w1_cp;
  a.nt = (int)tw.size();
  if (a.nt > 4 || twt.size() != tw.size() || tcout.size() != tw.size() || tcin.size() != tw.size())
    throw std::runtime_error("prep_step: up to 4 consistent transposes");
  if (w1_cp < 0 && (w1_c > 4 || taps != w1_cp * w1_cp)) throw std::runtime_error("prep_step: pair pack needs C <= 4, a square kernel");
  a.nb_pack = (int)std::min<int64_t>(((int64_t)w1_cout * taps * (w1_cp > 0 ? w1_cp : w1_c) + 255) / 256, 256);
  int total = a.nb_pad + a.nb_pack + a.nb_zero;
  for (int j = 0; j < a.nt; ++j) {
    a.tw[j] = (const bf16_t*)tw[j]; a.twt[j] = (bf16_t*)twt[j];
    a.tcout[j] = tcout[j]; a.tcin[j] = tcin[j];
    a.nb_t[j] = (tcin[j] % 64 == 0 && tcout[j] % 64 == 0) ? (tcin[j] / 64) * (tcout[j] / 64) * taps
                                                          : ((tcin[j] + 31) / 32) * ((tcout[j] + 31) / 32) * taps;
    total += a.nb_t[j];
  }
  if (total == 0) return;
  prep_step_kernel<<<total, 256, 0, as_stream(stream)>>>(a);
  DL_HIP_CHECK(hipGetLastError());
}

void prep_step(uintptr_t x, uintptr_t xp, int64_t P, int C, int Cp, int H, int W, int sp, uintptr_t w1, uintptr_t w1p,
               int w1_cout, int taps, int w1_c, int w1_cp, std::vector<uintptr_t> tw, std::vector<uintptr_t> twt,
               std::vector<int> tcout, std::vector<int> tcin, std::vector<uintptr_t> zp, std::vector<int64_t> zn,
               uintptr_t stream) {
  PrepArgs a{};
  a.x = (const bf16_t*)x; a.xp = (bf16_t*)xp; a.C = C; a.Cp = Cp;
  a.H = H; a.W = W; a.sp = sp;
  launch_prep(a, P, w1, w1p, w1_cout, taps, w1_c, w1_cp, tw, twt, tcout, tcin, zp, zn, stream);
}

// The augmentation value of a gather; every check that needs no image runs here.
Augment augment(uintptr_t params, int pad, int flip, int64_t n_samples) {
  if (!params) throw std::runtime_error("augment: null parameter pointer");
  if (params % 8) throw std::runtime_error("augment: the parameters are two aligned int64");
  if (pad < 0 || pad > 8) throw std::runtime_error("augment: pad must be 0..8");
  if (flip != 0 && flip != 1) throw std::runtime_error("augment: flip must be 0 or 1");
  if (n_samples <= 0) throw std::runtime_error("augment: the dataset's sample count must be positive");
  return Augment{params, pad, flip, n_samples};
}

// Same launch with the step's input gathered on the device: batch b of step
// s (= ctr[0]) is sample order[(s*B + b) mod n_order] of the uint8 NHWC
// dataset `img`, normalised ((v/255 - mean)/std), channel- and spatially
// padded into xp; its label goes to lab_out[b].  head_wgrad advances ctr[0]
// later in the step, so a captured graph replays consecutive batches.  aug:
// random crop / flip of each gathered image (dl_ops.h Augment; null: none).
void prep_step_gather(uintptr_t img, uintptr_t order, uintptr_t lab_all, uintptr_t lab_out, uintptr_t ctr,
                      int n_order, int B, int C, std::vector<float> mean, std::vector<float> stdv, uintptr_t xp,
                      int Cp, int H, int W, int sp, uintptr_t w1, uintptr_t w1p, int w1_cout, int taps, int w1_c,
                      int w1_cp, std::vector<uintptr_t> tw, std::vector<uintptr_t> twt, std::vector<int> tcout,
                      std::vector<int> tcin, std::vector<uintptr_t> zp, std::vector<int64_t> zn, uintptr_t stream,
                      const Augment* aug) {
  PrepArgs a{};
  a.xp = (bf16_t*)xp; a.C = C; a.Cp = Cp; a.H = H; a.W = W; a.sp = sp;
  prep_set_gather(a, img, order, lab_all, lab_out, ctr, n_order, B, C, mean, stdv);
  if (aug) prep_set_augment(a, aug->params, aug->pad, aug->flip, aug->n_samples);
  launch_prep(a, (int64_t)B * H * W, w1, w1p, w1_cout, taps, w1_c, w1_cp, tw, twt, tcout, tcin, zp, zn, stream);
}

// --------------------------------------------------------------------------
// host launchers
// --------------------------------------------------------------------------
static int fwd_bm(int tile) { return tile == 1 ? 64 : 128; }
static int fwd_bn(int tile) { return tile == 0 ? 128 : 64; }

static int combine_rows_per_block(int M, int N) {
  const int rpi = 256 / (N / 8);
  int rpb = (M + 383) / 384;            // ~384 blocks
  rpb = ((rpb + rpi - 1) / rpi) * rpi;  // whole iterations
  return rpb < rpi ? rpi : rpb;
}

// number of BN partial-sum rows conv_fwd writes for this configuration (no
// bit of the tile word changes the M tile, so whole-image region tiles count the same)
int conv_fwd_stat_rows(int B, int H, int W, int Cin, int Cout, int KS, int tile, int splits) {
  tile &= 15;
  ConvGeom g = make_geom(B, H, W, Cin, Cout, KS);
  if (splits <= 1) return (g.M + fwd_bm(tile) - 1) / fwd_bm(tile);
  const int rpb = combine_rows_per_block(g.M, Cout);
  return (g.M + rpb - 1) / rpb;
}

// The only cross-call state: the round-robin cursor over the arrival counters g_fix_cnt.
static int g_fix_next = 0;

// The kernel argument of a call's side job (none: nblk 0).  Runs every check of
// make_sgd_job / make_reduce_job, which is how the builders below validate.
static SgdJob side_job(const SideJob* s) {
  if (!s) return SgdJob{};
  SgdJob j = s->reduce ? make_reduce_job(s->g, s->lo, s->hi, s->offs, s->lens, s->slabs, s->splits, {}, 0)
                       : make_sgd_job(s->p, s->g, s->mom, s->p16, s->slot, s->lr, s->momentum, s->wd, s->lo, s->hi,
                                      s->offs, s->lens, s->slabs, s->splits, {}, 0, s->lr_dev);
  j.nblk = s->nblk > 0 ? s->nblk : -1;  // -1: sized by the launch (one float4 per thread)
  return j;
}

// The fused SGD update of the elements [lo, hi) of the flat buffer p: gradient g,
// or the split-K slabs of the given ranges; bf16 shadow p16 required (dl_ops.h SideJob).
SideJob side_sgd_job(uintptr_t p, uintptr_t g, uintptr_t mom, uintptr_t p16, uintptr_t slot, float lr, float momentum,
                     float wd, int64_t lo, int64_t hi, std::vector<int64_t> offs, std::vector<int64_t> lens,
                     std::vector<uintptr_t> slabs, std::vector<int> splits, int nblk, uintptr_t lr_dev) {
  if (!p16) throw std::runtime_error("side_sgd_job: needs the bf16 shadow");
  const SideJob j{false, p, g, mom, p16, slot, lr, momentum, wd, lo, hi, offs, lens, slabs, splits, nblk, lr_dev};
  side_job(&j);
  return j;
}

// The sums of the split-K weight-gradient slabs of the given in-place ranges into
// the gradient buffer g (sgd_dev.h: bitwise slab_reduce's sums), not in a launch of their own.
SideJob side_reduce_job(uintptr_t g, int64_t lo, int64_t hi, std::vector<int64_t> offs, std::vector<int64_t> lens,
                        std::vector<uintptr_t> slabs, std::vector<int> splits, int nblk) {
  if (offs.empty()) throw std::runtime_error("side_reduce_job: no slab range");
  const SideJob j{true, 0, g, 0, 0, 0, 0.f, 0.f, 0.f, lo, hi, offs, lens, slabs, splits, nblk, 0};
  side_job(&j);
  return j;
}

// Process-wide A/B settings of the streaming kernel; a per-call value of the
// tile word (FwdOpts) overrides them for that call without writing them.
static int g_fwd_waves = 8;
static int g_fwd_stages = 3;

// Bits of the packed tile word above the tile id, stages and waves (dl_ops.h conv_fwd)
constexpr int kTileRegionImages = 1 << 16, kTileKeepSlabs = 1 << 20, kTilePair = 1 << 24;

// Everything that is per call in a forward / dgrad launch: the decoded tile
// word (decode_tile) plus what the entry point's own arguments add.
struct FwdOpts {
  int tile = 0;                // 0 = 128x128, 1 = 64x64, 2 = 128x64
  int stages = 0, waves = 0;   // streaming kernel; 0 = the process setting
  bool keep_slabs = false;     // split-K: leave the slabs, the caller combines them
  bool pair = false;           // pair-packed first-layer weights (conv_fwd_c8_kernel PAIR)
  bool region_images = false;  // whole-image region tiles allowed (as set_conv_region(2), unless it is 0)
  uintptr_t addend = 0;        // bf16 [M][Cout] added in the epilogue ...
  uintptr_t addend_mask = 0;   // ... under these optional uint8 [M][Cout/8] mask bits
  bool fix = false;            // split-K combined in-launch (FIX) by each tile's last-arriving slice
  BnRedArgs bnred{};           // rows != nullptr: the BN backward reduce of the block below (BNR 1) in
                               // the epilogue of the region dgrad, or of the fix reducers
  SgdJob side{};               // side job of this launch (streaming kernel only)
};

// The tile word decoded: the first statement of every conv_fwd* entry point,
// and what the read-only queries use.
static FwdOpts decode_tile(int tile) {
  FwdOpts o;
  o.tile = tile & 15;
  o.stages = (tile >> 4) & 15;
  o.waves = (tile >> 8) & 15;
  o.region_images = (tile & kTileRegionImages) != 0;
  o.keep_slabs = (tile & kTileKeepSlabs) != 0;
  o.pair = (tile & kTilePair) != 0;
  if (o.stages && (o.stages < 2 || o.stages > 4)) throw std::runtime_error("conv_fwd: packed stages must be 2..4");
  if (o.waves && o.waves != 4 && o.waves != 8) throw std::runtime_error("conv_fwd: packed waves must be 4 or 8");
  return o;
}

// Position-major tiles with padding taps skipped (conv_fwd_kernel, g.posm):
// for TAPU layers whose output is smaller than twice the kernel (most output
// pixels then have padding-only taps), the batch a multiple of BM and no
// addend.  (8x8 outputs added in round 6: CIFAR layer-3 dgrad 27.2 -> 25.7 us,
// 28 % of its taps read only the border; the per-tile work is then uneven, and
// 4 splits to even it out lost, profiles/r6_posm8_ab.txt.)
// set_conv_posm(0) = the pixel-major tiles (A/B).
static int g_posm = 1;
void set_conv_posm(int on) { g_posm = on ? 1 : 0; }

// Uniform taps (TAPU): every 64-channel K step of the streaming kernel lies in one tap.
static bool fwd_tapu(const ConvGeom& g) { return g.Cin >= 64; }

// Whether the streaming kernel with M tile bm runs this launch position-major
// (tapu: fwd_tapu, the kernel's TAPU instance).
static bool fwd_posm(const ConvGeom& g, int bm, bool tapu, bool addend) {
  return g_posm && tapu && !addend && g.B % bm == 0 && (g.H < 2 * g.KS || g.W < 2 * g.KS) && g.S == 1 && !g.om &&
         g.KH == g.KS && g.KW == g.KS && g.Hp == g.H + 2 * g.pad && g.Wp == g.W + 2 * g.pad;
}

template <int BM, int BN, bool TAPU, int ST, int WM, int WN>
static void launch_fwd_w(ConvGeom& g, const FwdOpts& o, uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t stats,
                         uintptr_t slab, int splits, hipStream_t s) {
  g.posm = fwd_posm(g, BM, TAPU, o.addend != 0) ? 1 : 0;
  const int ntm = (g.M + BM - 1) / BM, ntn = (g.Cout + BN - 1) / BN;
  const int nkt = (g.Kch + 7) / 8;
  const int ktps = (nkt + splits - 1) / splits;
  constexpr int NT = 64 * WM * WN;
  SgdJob side = o.side;
  if (side.nblk < 0)  // auto: one float4 per thread (2048 x 512 measured best of 256..2048 workgroups)
    side.nblk = (int)std::max<int64_t>(1, (side.hi4 - side.lo4 + NT - 1) / NT);
  const int grid = ntm * ntn * splits + side.nblk;
  constexpr bool kTR = (BN / WN / 16) % 2 == 0;
  if (o.fix) {
    if constexpr (kTR && TAPU && BM == 128 && BN == 64 && WM == 4 && WN == 2) {
      if (splits < 2 || g.om || o.addend)
        throw std::runtime_error("conv_fwd_fix: split-K without output maps / addends");
      const int ntiles = ntm * ntn;
      if (ntiles > kFixCnt) throw std::runtime_error("conv_fwd_fix: too many tiles");
      static int* cnt0 = nullptr;
      if (!cnt0) DL_HIP_CHECK(hipGetSymbolAddress((void**)&cnt0, HIP_SYMBOL(g_fix_cnt)));
      if (g_fix_next + ntiles > kFixCnt) g_fix_next = 0;
      int* cnt = cnt0 + g_fix_next;  // distinct counters per call site (graph replays reuse them in order)
      g_fix_next += ntiles;
      if (o.bnred.rows != nullptr) {
        if (stats) throw std::runtime_error("conv_fwd_fix: BN reduce epilogue has no statistics");
        conv_fwd_kernel<BM, BN, false, false, TAPU, ST, WM, WN, false, true, 1, true><<<grid, NT, 0, s>>>(
            (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, nullptr, (float*)slab, g, splits, ktps, g_conv_dbg,
            o.bnred, side, cnt);
      } else if (stats) {
        conv_fwd_kernel<BM, BN, true, false, TAPU, ST, WM, WN, false, true, 0, true><<<grid, NT, 0, s>>>(
            (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, (float*)stats, (float*)slab, g, splits, ktps, g_conv_dbg,
            BnRedArgs{}, side, cnt);
      } else {
        conv_fwd_kernel<BM, BN, false, false, TAPU, ST, WM, WN, false, true, 0, true><<<grid, NT, 0, s>>>(
            (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, nullptr, (float*)slab, g, splits, ktps, g_conv_dbg,
            BnRedArgs{}, side, cnt);
      }
      return;
    } else {
      throw std::runtime_error("conv_fwd_fix: only the 128x64 streaming tile (8 waves) combines in-launch");
    }
  }
  if (o.addend && (splits > 1 || stats)) throw std::runtime_error("conv_fwd_add: no split-K / statistics");
  if (o.addend)  // (ADD: the addend and its mask bits travel in the slab and stats pointers)
    conv_fwd_kernel<BM, BN, false, false, TAPU, ST, WM, WN, true><<<grid, NT, 0, s>>>(
        (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, (float*)o.addend_mask, (float*)o.addend, g, 1, ktps,
        g_conv_dbg, BnRedArgs{}, side);
  else if (splits > 1)
    conv_fwd_kernel<BM, BN, false, true, TAPU, ST, WM, WN><<<grid, NT, 0, s>>>(
        (const bf16_t*)x, (const bf16_t*)w, nullptr, nullptr, (float*)slab, g, splits, ktps, g_conv_dbg, BnRedArgs{}, side);
  else if (stats)
    conv_fwd_kernel<BM, BN, true, false, TAPU, ST, WM, WN><<<grid, NT, 0, s>>>(
        (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, (float*)stats, nullptr, g, 1, ktps, g_conv_dbg, BnRedArgs{}, side);
  else
    conv_fwd_kernel<BM, BN, false, false, TAPU, ST, WM, WN><<<grid, NT, 0, s>>>(
        (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, nullptr, nullptr, g, 1, ktps, g_conv_dbg, BnRedArgs{}, side);
}

template <int BM, int BN, bool TAPU, int ST>
static void launch_fwd_t(ConvGeom& g, const FwdOpts& o, uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t stats,
                         uintptr_t slab, int splits, hipStream_t s) {
  if ((o.waves ? o.waves : g_fwd_waves) == 8) {
    if constexpr (BN >= 128) launch_fwd_w<BM, BN, TAPU, ST, 2, 4>(g, o, x, w, y, stats, slab, splits, s);
    else if constexpr (BM >= 128) launch_fwd_w<BM, BN, TAPU, ST, 4, 2>(g, o, x, w, y, stats, slab, splits, s);
    else launch_fwd_w<BM, BN, TAPU, ST, 2, 4>(g, o, x, w, y, stats, slab, splits, s);
  } else {
    launch_fwd_w<BM, BN, TAPU, ST, 2, 2>(g, o, x, w, y, stats, slab, splits, s);
  }
}

void set_conv_waves(int waves) {
  if (waves != 4 && waves != 8) throw std::runtime_error("waves must be 4 or 8");
  g_fwd_waves = waves;
}

void set_conv_fwd_pf(int on) {
  const int v = on ? 1 : 0;
  DL_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_fwd_pf), &v, sizeof(int)));
}
void set_conv_debug(uintptr_t buf) { g_conv_dbg = (unsigned long long*)buf; }
void set_conv_wgrad_stamps(uintptr_t buf) {
  unsigned long long* p = (unsigned long long*)buf;
  DL_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_wgrad_stamps), &p, sizeof(p)));
}

void set_conv_stages(int fwd, int wgrad) {
  if (fwd < 2 || fwd > 4 || wgrad != 0)
    throw std::runtime_error("stages: fwd 2..4, wgrad 0 (the per-tile default; other rings removed in round 6)");
  g_fwd_stages = fwd;
}

template <int BM, int BN>
static void launch_fwd(ConvGeom& g, const FwdOpts& o, uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t stats,
                       uintptr_t slab, int splits, hipStream_t s) {
  int st = o.stages ? o.stages : g_fwd_stages;
  if ((BM * 64 * 2 + BN * 64 * 2) * 4 > 160 * 1024) st = std::min(st, 3);
  if (fwd_tapu(g)) {
    if (st == 2) launch_fwd_t<BM, BN, true, 2>(g, o, x, w, y, stats, slab, splits, s);
    else if (st == 3) launch_fwd_t<BM, BN, true, 3>(g, o, x, w, y, stats, slab, splits, s);
    else launch_fwd_t<BM, BN, true, 4>(g, o, x, w, y, stats, slab, splits, s);
  } else {
    launch_fwd_t<BM, BN, false, 3>(g, o, x, w, y, stats, slab, splits, s);
  }
}

// ---- tap-reuse (LDS-resident region) forward path --------------------------
// set_conv_region(0) forces the streaming kernel (A/B); 1 = region kernel
// for row tiles (H*W % 128 == 0), 2 = also for whole-image tiles.  Measured
// (MI355X, batch 128, rocprofv3): rows mode wins (conv2 fwd 19.3 -> 17.7 us,
// dgrad 22.8 -> 20.5 us); images mode loses (conv3/conv4 21-25 vs 19.7 us:
// the 4x4/8x8 outputs need 8x8/12x12 padded inputs, the region fill does not
// amortise over 25 k-steps), so it is off by default.
static int g_region = 1, g_region_images = 0;
void set_conv_region(int on) {
  g_region = on ? 1 : 0;
  g_region_images = on >= 2 ? 1 : 0;
}

// LDS budget of one region-kernel workgroup: the CU's 160 KiB minus room for
// one co-resident RCCL collective workgroup (rcclGenericKernel: 19,744 B of
// LDS, 256 threads, <= 280 VGPRs -- read from librccl's gfx950 code object),
// so the bucket all-reduce that overlaps the backward at N > 1 never evicts
// a conv workgroup from a CU (a 1-workgroup-per-CU grid would otherwise need
// a second round for the CUs RCCL holds).  The dgrad instance (BN = 64, the
// one that runs beside the all-reduce) also stays at <= 112 VGPRs, so two
// of its waves fit a SIMD next to a 288-VGPR RCCL wave; the BN = 128
// instance (127 VGPRs) only runs in the forward, before any collective.
// Measured with one CU held by a workgroup of RCCL's footprint
// (bench_conv.py --occupy 1): the dgrad instance (~126 KiB) +1 us, while the
// streaming kernel's 3-stage ring (96 KiB, 90 VGPRs) loses 14 us -- the executor
// switches the overlapped dgrads to its 2-stage ring (models/cifar_hip.py).
constexpr int kRegionLdsCap = 160 * 1024 - 20 * 1024;

// Region geometry for a BM = 128 tile, or false if the shape does not fit the
// region kernel (then the streaming kernel runs).  images: whole-image tiles
// allowed (set_conv_region(2), or the call's own bit of the tile word).
static bool region_geom(const ConvGeom& g, int BN, int splits, bool images, RegionGeom& rg) {
  constexpr int BM = 128, STAGES = 3;
  if (!g.pow2 || !g_region || g.Cin % 64 != 0 || g.W > BM || BM % g.W != 0) return false;
  const int HW = g.H * g.W;
  const int chunks = g.Cin / 64;
  if (chunks % splits != 0) return false;
  rg.cpw = chunks / splits;
  if (rg.cpw > 2) return false;
  rg.S = 10;  // the kernel's region loader divides by 10 with a multiply
  rg.RW = g.Wp;
  if (HW % BM == 0) {  // M tile = BM / W whole output rows of one image
    rg.rows_mode = 1;
    rg.nimg = 1;
    rg.RH = BM / g.W + g.KS - 1;
    rg.RS = rg.RW * rg.S;
  } else if (BM % HW == 0 && images) {  // M tile = BM / HW whole images
    rg.rows_mode = 0;
    rg.nimg = BM / HW;
    rg.RH = g.Hp;
    rg.RS = rg.RW * rg.S + 8;  // + 8 slots per region row: conflict-free fragment reads across rows
  } else {
    return false;
  }
  rg.IS = rg.RH * rg.RS;
  rg.nslot = (rg.nimg * rg.IS + 63) / 64 * 64;
  if (rg.RS >= 16384) return false;
  if (rg.nslot >= (1 << 16)) return false;
  rg.inv_S = 1.0f / rg.S;
  rg.inv_RS = 1.0f / rg.RS;
  rg.inv_IS = 1.0f / rg.IS;
  const int lds = rg.cpw * rg.nslot * 16 + STAGES * BN * 64 * 2;  // at least a 3-stage B ring
  return lds <= kRegionLdsCap;
}

static int g_region_waves = 8;  // 8: 2 waves per SIMD; 4: one wave per SIMD with 2x wider wave tiles
void set_conv_region_waves(int w) {
  if (w != 4 && w != 8) throw std::runtime_error("region waves must be 4 or 8");
  g_region_waves = w;
}
static int g_region_ablate = 0;  // debug: bit 0 = no in-loop weight DMA, bit 1 = no MFMAs
void set_conv_region_ablate(int a) { g_region_ablate = a; }
static int g_region_stages = 0;  // 0 = as many B stages as the LDS holds (max 8)
void set_conv_region_stages(int st) { g_region_stages = st; }

template <int BN, int WM, int WN, int ST>
static void launch_fwd_region_st(const ConvGeom& g, const RegionGeom& rg, const FwdOpts& o, uintptr_t x, uintptr_t w,
                                 uintptr_t y, uintptr_t stats, uintptr_t slab, int splits, hipStream_t s) {
  const int ntm = (g.M + 127) / 128;
  const int grid = ntm * (g.Cout / BN) * splits;
  const size_t lds = (size_t)rg.cpw * rg.nslot * 16 + ST * BN * 64 * 2;
  auto go = [&](auto kern, bf16_t* yy, float* st, float* sl) {
    static bool attr = false;  // per instantiation: allow > 64 KiB of dynamic LDS
    if (!attr) {
      DL_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      attr = true;
    }
    kern<<<grid, 64 * WM * WN, lds, s>>>((const bf16_t*)x, (const bf16_t*)w, yy, st, sl, g, rg, splits, g_conv_dbg,
                                         g_region_ablate, o.bnred);
  };
  if (o.bnred.rows != nullptr) {
    if (splits > 1 || stats) throw std::runtime_error("conv_fwd_bnred: plain unsplit dgrad only");
    go(conv_fwd_region_kernel<BN, false, false, ST, WM, WN, true>, (bf16_t*)y, nullptr, nullptr);
  } else if (splits > 1)
    go(conv_fwd_region_kernel<BN, false, true, ST, WM, WN>, nullptr, nullptr, (float*)slab);
  else if (stats)
    go(conv_fwd_region_kernel<BN, true, false, ST, WM, WN>, (bf16_t*)y, (float*)stats, nullptr);
  else
    go(conv_fwd_region_kernel<BN, false, false, ST, WM, WN>, (bf16_t*)y, nullptr, nullptr);
}

// The LDS-DMA issue -> landed latency is ~1.1 us while a k-step computes in
// ~0.2 us: the B ring must keep ~5 k-steps in flight, so it takes every
// stage the LDS has left after the region.
template <int BN, int WM, int WN>
static void launch_fwd_region(const ConvGeom& g, const RegionGeom& rg, const FwdOpts& o, uintptr_t x, uintptr_t w,
                              uintptr_t y, uintptr_t stats, uintptr_t slab, int splits, hipStream_t s) {
  const int free_b = kRegionLdsCap - rg.cpw * rg.nslot * 16;
  int st = std::min(8, free_b / (BN * 64 * 2));
  if (g_region_stages > 0) st = std::min(st, g_region_stages);
  if (st >= 8) launch_fwd_region_st<BN, WM, WN, 8>(g, rg, o, x, w, y, stats, slab, splits, s);
  else if (st >= 6) launch_fwd_region_st<BN, WM, WN, 6>(g, rg, o, x, w, y, stats, slab, splits, s);
  else if (st >= 5) launch_fwd_region_st<BN, WM, WN, 5>(g, rg, o, x, w, y, stats, slab, splits, s);
  else if (st >= 4) launch_fwd_region_st<BN, WM, WN, 4>(g, rg, o, x, w, y, stats, slab, splits, s);
  else launch_fwd_region_st<BN, WM, WN, 3>(g, rg, o, x, w, y, stats, slab, splits, s);
}

// a region kernel takes the shape (the streaming kernel otherwise).  (The
// direct-B region kernel -- weights streamed into registers, no LDS ring --
// measured slower, layer-2 k-loop 24.3 k vs 23.6 k cycles, layer-3 49.9 k vs
// 34.0 k, README round 5 / scripts/stamp_region.py; removed in round 6.)
static bool any_region_geom(const ConvGeom& g, int tile_word, int splits, RegionGeom& rg) {
  const int tile = tile_word & 15;
  const bool images = g_region_images || (tile_word & kTileRegionImages);
  return (tile == 2 && region_geom(g, 64, splits, images, rg)) || (tile == 0 && region_geom(g, 128, splits, images, rg));
}

// M tiles per workgroup of the first-layer (Cin = 8) kernel (upper bound; set_conv_c8_mt).
// Measured at batch 128 (profiles/r2_c8_mt_ab.txt): 1 tile (1024 workgroups, 4 per CU)
// 12.0 us, 4 tiles (256 workgroups, one weight-panel DMA each) 14.8 us: the kernel is
// bound by its epilogue stores overlapping across workgroups, not by the weight DMA.
static int g_c8_mt = 1;
void set_conv_c8_mt(int mt) {
  if (mt != 1 && mt != 2 && mt != 4 && mt != 8) throw std::runtime_error("c8 tiles per workgroup: 1, 2, 4 or 8");
  g_c8_mt = mt;
}

// Launch plan of the first-layer kernel: M tiles per workgroup, region rows, LDS bytes.
struct C8Plan {
  int mt, rows;
  size_t lds;
};

// Whether the first-layer kernel (tile 2, unsplit, Cin 8 or the pair-packed 4)
// takes the shape, and its plan if so.
static bool c8_plan(const ConvGeom& g, const FwdOpts& o, int splits, C8Plan& p) {
  const int H = g.H, W = g.W, KS = g.KS, Cout = g.Cout;
  // mt M tiles per workgroup (largest of g_c8_mt, ..., 2, 1 that keeps
  // >= 256 workgroups and divides the tiles of one image)
  int c8_mt = 1;
  const int c8_ntm = (H * W) % 128 == 0 ? g.M / 128 : 0;
  for (int mt = g_c8_mt; mt > 1; mt /= 2) {
    if (c8_ntm > 0 && (H * W) % (mt * 128) == 0 && c8_ntm % mt == 0 && (c8_ntm / mt) * std::max(1, Cout / 64) >= 256) {
      c8_mt = mt;
      break;
    }
  }
  const int c8_rows = c8_mt * 128 / std::max(1, W) + KS - 1;
  const int c8_chunks = o.pair ? KS * ((KS + 1) / 2) : KS * KS;  // weight chunks per output channel
  const int c8_rslots = o.pair ? (c8_rows * g.Wp + 1) / 2 : c8_rows * g.Wp;  // 16-B region slots (pair: 2 pixels)
  const size_t c8_lds =
      (size_t)((c8_rslots + 2 + 63) / 64 * 64 + (64 * c8_chunks + 63) / 64 * 64) * 16 + 4 * 2 * 64 * 4;
  p = C8Plan{c8_mt, c8_rows, c8_lds};
  return o.tile == 2 && splits == 1 && g_region && g.pow2 && (g.Cin == 8 || o.pair) && W <= 128 && 128 % W == 0 &&
         (H * W) % 128 == 0 && Cout % 64 == 0 && c8_lds <= 160 * 1024;
}

static void launch_fwd_c8(const ConvGeom& g, const FwdOpts& o, const C8Plan& p, uintptr_t x, uintptr_t w, uintptr_t y,
                          uintptr_t stats, hipStream_t s) {
  const int Cout = g.Cout, c8_mt = p.mt, c8_rows = p.rows;
  const size_t c8_lds = p.lds;
  const int grid = (g.M / 128 / c8_mt) * (Cout / 64);
  auto go = [&](auto kern) {
    static bool attr = false;
    if (!attr) {
      DL_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      attr = true;
    }
    kern<<<grid, 512, c8_lds, s>>>((const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, (float*)stats, g, c8_rows,
                                   c8_mt, g_conv_dbg);
  };
  if (o.pair) {
    if (stats) go(conv_fwd_c8_kernel<true, true>);
    else go(conv_fwd_c8_kernel<false, true>);
  } else if (stats) {
    go(conv_fwd_c8_kernel<true>);
  } else {
    go(conv_fwd_c8_kernel<false>);
  }
}

// The kernel a forward / dgrad launch runs on (the values conv_fwd_path reports).
enum class FwdKernel { Streaming = 0, RegionRows = 1, RegionImages = 2, C8 = 3 };

// Host validation of a forward launch, shared by run_fwd and conv_fwd_path.
static void check_fwd(const ConvGeom& g, const FwdOpts& o) {
  if (g.Cout % 8 != 0) throw std::runtime_error("conv_fwd: Cout % 8 != 0");
  if (o.tile > 2) throw std::runtime_error("conv_fwd: bad tile id");
  if (g.Cout % fwd_bn(o.tile) != 0) throw std::runtime_error("conv_fwd: Cout must be a multiple of the N tile");
}

// Which kernel takes the launch, with its plan (rg: region tiles, c8: first layer).
static FwdKernel pick_fwd(const ConvGeom& g, const FwdOpts& o, int splits, RegionGeom& rg, C8Plan& c8) {
  // addends, the in-launch split-K combine and its BN reduce epilogue are on the streaming kernel
  const bool streaming_only = o.fix || o.addend;
  const bool images = g_region_images || o.region_images;
  if (!streaming_only && c8_plan(g, o, splits, c8)) return FwdKernel::C8;
  if (o.pair)
    throw std::runtime_error("conv_fwd: pair-packed weights need the first-layer kernel (Cin 8, tile 2, no split)");
  if (!streaming_only && ((o.tile == 0 && region_geom(g, 128, splits, images, rg)) ||
                          (o.tile == 2 && region_geom(g, 64, splits, images, rg))))
    return rg.rows_mode ? FwdKernel::RegionRows : FwdKernel::RegionImages;
  return FwdKernel::Streaming;
}

// What every conv_fwd* entry point runs once it has its geometry and options:
// the launch on the kernel that takes the shape, then the split-K combine.
// Returns the number of BN partial rows written to `stats` (if non-null).
static int run_fwd(ConvGeom& g, const FwdOpts& o, uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t stats,
                   uintptr_t slab, int splits, uintptr_t stream) {
  const int tile = o.tile, Cout = g.Cout;
  hipStream_t s = as_stream(stream);
  if (splits < 1) splits = 1;
  if (splits > 1 && !slab) throw std::runtime_error("conv_fwd: split-K needs a slab");
  check_fwd(g, o);
  RegionGeom rg{};
  C8Plan c8{};
  const FwdKernel k = pick_fwd(g, o, splits, rg, c8);
  if (o.side.nblk != 0 && k != FwdKernel::Streaming)  // nothing is enqueued yet
    throw std::runtime_error("conv_fwd: a side job needs the streaming kernel (this call: region / first layer)");
  if (k == FwdKernel::C8) {
    launch_fwd_c8(g, o, c8, x, w, y, stats, s);
  } else if (k != FwdKernel::Streaming && tile == 0) {
    if (g_region_waves == 4) launch_fwd_region<128, 2, 2>(g, rg, o, x, w, y, stats, slab, splits, s);
    else launch_fwd_region<128, 2, 4>(g, rg, o, x, w, y, stats, slab, splits, s);
  } else if (k != FwdKernel::Streaming) {
    if (g_region_waves == 4) launch_fwd_region<64, 2, 2>(g, rg, o, x, w, y, stats, slab, splits, s);
    else launch_fwd_region<64, 4, 2>(g, rg, o, x, w, y, stats, slab, splits, s);
  } else {
    if (tile == 0) launch_fwd<128, 128>(g, o, x, w, y, stats, slab, splits, s);
    else if (tile == 1) launch_fwd<64, 64>(g, o, x, w, y, stats, slab, splits, s);
    else launch_fwd<128, 64>(g, o, x, w, y, stats, slab, splits, s);
  }
  DL_HIP_CHECK(hipGetLastError());
  if (splits == 1 || o.fix) return (g.M + fwd_bm(tile) - 1) / fwd_bm(tile);
  if (o.keep_slabs) {
    if (stats) throw std::runtime_error("conv_fwd keep-slabs: no statistics");
    return 0;
  }
  if (256 % (Cout / 8) != 0) throw std::runtime_error("conv_fwd split-K combine: Cout/8 must divide 256");
  const int rpb = combine_rows_per_block(g.M, Cout);
  const int nb = (g.M + rpb - 1) / rpb;
  if (stats)
    splitk_combine_kernel<true><<<nb, 256, 0, s>>>((const float*)slab, (bf16_t*)y, (float*)stats, splits, g.M, Cout,
                                                   rpb, g);
  else
    splitk_combine_kernel<false><<<nb, 256, 0, s>>>((const float*)slab, (bf16_t*)y, nullptr, splits, g.M, Cout, rpb,
                                                    g);
  DL_HIP_CHECK(hipGetLastError());
  return nb;
}

// tile: 0 = 128x128, 1 = 64x64, 2 = 128x64 (BM x BN, BK = 64) plus the
// per-call bits of dl_ops.h.  splits > 1: split-K into `slab` (fp32
// [splits][M][Cout]) + combine (bf16 y, BN partials).
int conv_fwd(uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t stats, uintptr_t slab, int B, int H, int W, int Cin,
             int Cout, int KS, int tile, int splits, uintptr_t stream, const SideJob* side) {
  FwdOpts o = decode_tile(tile);
  o.side = side_job(side);
  if (o.pair && Cin != 4) throw std::runtime_error("conv_fwd: pair-packed weights need the 4-channel input");
  ConvGeom g = o.pair ? make_geom_pair(B, H, W, Cout, KS) : make_geom(B, H, W, Cin, Cout, KS);
  return run_fwd(g, o, x, w, y, stats, slab, splits, stream);
}

// Read-only: the kernel conv_fwd would run this call on, by the predicates of
// run_fwd itself.  0 = streaming, 1 = region row tiles, 2 = region image tiles,
// 3 = first-layer (c8) kernel; + 4: position-major tiles (streaming only).
// Nothing is launched.
int conv_fwd_path(int B, int H, int W, int Cin, int Cout, int KS, int tile, int splits) {
  const FwdOpts o = decode_tile(tile);
  if (o.pair && Cin != 4) throw std::runtime_error("conv_fwd: pair-packed weights need the 4-channel input");
  const ConvGeom g = o.pair ? make_geom_pair(B, H, W, Cout, KS) : make_geom(B, H, W, Cin, Cout, KS);
  if (splits < 1) splits = 1;
  check_fwd(g, o);
  RegionGeom rg{};
  C8Plan c8{};
  const FwdKernel k = pick_fwd(g, o, splits, rg, c8);
  int path = (int)k;
  if (k == FwdKernel::Streaming && fwd_posm(g, fwd_bm(o.tile), fwd_tapu(g), false)) path |= 4;
  return path;
}

// Whether conv_fwd runs this unsplit shape on the region (tap-reuse) kernel --
// the kernel that carries the fused BN backward reduce epilogue.
int conv_region_ok(int B, int H, int W, int Cin, int Cout, int KS, int tile, int splits) {
  ConvGeom g = make_geom(B, H, W, Cin, Cout, KS);
  RegionGeom rg{};
  if (splits < 1) splits = 1;
  return any_region_geom(g, tile, splits, rg) ? 1 : 0;
}

// conv_fwd (a dgrad) with the previous block's BatchNorm backward reduce in its
// epilogue (BnRedArgs): only the region kernel path; returns the number of
// rows written (M tiles, mode 0) or throws if the shape takes another kernel.
int conv_fwd_bnred(uintptr_t x, uintptr_t w, uintptr_t y, int B, int H, int W, int Cin, int Cout, int KS, int tile,
                   uintptr_t y_prev, uintptr_t coef, uintptr_t rows, uintptr_t stream) {
  FwdOpts o = decode_tile(tile);
  ConvGeom g = make_geom(B, H, W, Cin, Cout, KS);
  RegionGeom rg{};
  if (o.pair || !any_region_geom(g, tile, 1, rg))
    throw std::runtime_error("conv_fwd_bnred: the shape does not take the region kernel");
  if (!rows || !coef || !y_prev) throw std::runtime_error("conv_fwd_bnred: null operand");
  o.bnred = BnRedArgs{(const bf16_t*)y_prev, (const float*)coef, (float*)rows};
  return run_fwd(g, o, x, w, y, 0, 0, 1, stream);
}

// conv_fwd of a split-K plan whose slices are combined inside the launch
// (FIX, splitk_fixup) instead of by splitk_combine / combine_bwd_reduce: the
// reducer of each tile writes bf16 y and either the BN statistics (stats) or,
// y_prev != 0 (a dgrad), the BatchNorm backward reduce of the block below
// into rows (conv_fwd_bnred's epilogue, BNR 1).  128x64 streaming tiles only
// (conv_fix_ok).  Returns the rows written (M tiles).
int conv_fwd_fix(uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t stats, uintptr_t slab, int B, int H, int W, int Cin,
                 int Cout, int KS, int tile, int splits, uintptr_t y_prev, uintptr_t coef, uintptr_t rows,
                 uintptr_t stream, const SideJob* side) {
  FwdOpts o = decode_tile(tile);
  o.side = side_job(side);
  if (splits < 2 || !slab) throw std::runtime_error("conv_fwd_fix: a split-K plan with a slab");
  if ((y_prev != 0) != (rows != 0) || (y_prev && !coef)) throw std::runtime_error("conv_fwd_fix: BN reduce operands");
  o.fix = true;
  if (y_prev) o.bnred = BnRedArgs{(const bf16_t*)y_prev, (const float*)coef, (float*)rows};
  ConvGeom g = make_geom(B, H, W, Cin, Cout, KS);
  return run_fwd(g, o, x, w, y, stats, slab, splits, stream);
}

// Whether conv_fwd_fix serves this plan (the 128x64 streaming tile, 8 waves,
// the transposed epilogue; no balanced position-major split).
int conv_fix_ok(int B, int H, int W, int Cin, int Cout, int KS, int tile, int splits) {
  (void)B; (void)H; (void)W;
  const int t = tile & 15, wv = (tile >> 8) & 15;
  return (t == 2 && splits >= 2 && Cin >= 64 && Cout % 64 == 0 && KS >= 1 && (wv == 0 ? g_fwd_waves : wv) == 8) ? 1 : 0;
}

// y = conv(x, w) + addend (bf16, same layout as y), streaming kernel only
// (KS = 1 or the region kernels disabled for the shape), no split-K / stats.
void conv_fwd_add(uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t addend, int B, int H, int W, int Cin, int Cout,
                  int KS, int tile, uintptr_t stream, uintptr_t addend_mask) {
  FwdOpts o = decode_tile(tile);
  ConvGeom g = make_geom(B, H, W, Cin, Cout, KS);
  if (!addend) throw std::runtime_error("conv_fwd_add: null addend");
  if (KS != 1 && g_region) throw std::runtime_error("conv_fwd_add: only the streaming kernel (KS = 1)");
  o.addend = addend;
  o.addend_mask = addend_mask;
  run_fwd(g, o, x, w, y, 0, 0, 1, stream);
}

// y[om(m)] = conv(x, w)[m] (+ addend[om(m)] when addend != 0: an in-place
// accumulate when addend == y) with the generalised geometry; om_S == 0: no
// output map.  Returns the number of BN statistics rows (stats != 0, no split).
int conv_fwd_ex(uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t stats, uintptr_t slab, int B, int Ho, int Wo, int Hp,
                int Wp, int Cin, int Cout, int KH, int KW, int S, int om_S, int om_H0, int om_W0, int om_W, int om_HW,
                uintptr_t addend, int tile, int splits, uintptr_t stream) {
  FwdOpts o = decode_tile(tile);
  ConvGeom g = make_geom_ex(B, Ho, Wo, Hp, Wp, Cin, Cout, KH, KW, S);
  if (om_S > 0) {
    g.om = 1; g.omS = om_S; g.omH0 = om_H0; g.omW0 = om_W0; g.omW = om_W; g.omHW = om_HW;
    if ((int64_t)B * om_HW * std::max(Cin, Cout) >= (1ll << 31)) throw std::runtime_error("conv_fwd_ex: output too large");
  }
  if (splits > 1 && (addend || g.om)) throw std::runtime_error("conv_fwd_ex: split-K takes no addend / map");
  if (stats && (addend || splits > 1)) throw std::runtime_error("conv_fwd_ex: statistics need a plain, unsplit output");
  if (Cin % 8 != 0) throw std::runtime_error("conv_fwd_ex: Cin % 8 != 0");
  if (Cin >= 64 && Cin % 64 != 0) throw std::runtime_error("conv_fwd_ex: Cin >= 64 must be a multiple of 64");
  o.addend = addend;
  return run_fwd(g, o, x, w, y, stats, slab, splits, stream);
}

// out: fp32 [splits][Cout][ldo], ldo >= K (K = KS*KS*Cin); tile 1 = 64x64, 2 = 128x128 (co x k)
static void conv_wgrad_g(const ConvGeom& g, uintptr_t dy, uintptr_t x, uintptr_t out, int splits, int ldo, int tile,
                         uintptr_t stream, const SideJob* side_in = nullptr) {
  SgdJob side = side_job(side_in);
  const int Cout = g.Cout, W = g.W;
  if (tile != 1 && tile != 2) throw std::runtime_error("conv_wgrad: tile 1 (64x64) or 2 (128x128)");
  if (ldo < g.K) throw std::runtime_error("conv_wgrad: ldo < K");
  if (ldo % 4 != 0) throw std::runtime_error("conv_wgrad: ldo % 4 != 0 (16-byte slab stores)");
  if (Cout % 8 != 0) throw std::runtime_error("conv_wgrad: Cout % 8 != 0");
  const int bm = tile == 1 ? 64 : 128;
  if (Cout % bm != 0) throw std::runtime_error("conv_wgrad: Cout must be a multiple of the Cout tile");
  if (g.pow2 && W > 64) throw std::runtime_error("conv_wgrad: needs W <= 64");
  if (splits < 1) splits = 1;
  int mps = (g.M + splits - 1) / splits;
  mps = (mps + 63) / 64 * 64;  // 64-row aligned M steps (padded-layout addressing)
  hipStream_t s = as_stream(stream);
  // 4-stage LDS-DMA rings with fragment prefetch: 64x64 tiles (2 WGs per CU:
  // wgrad1 22.1 -> 16.8 us vs 3 stages), 128x128 tiles (1 WG per CU, 128 KiB
  // LDS, 141 VGPRs: wgrad2/3/4 31.7/29.7/28.4 us as 128x64 -> 24.7/23.0/21.8 us;
  // the waves wait on the LDS-DMA ring, so the deeper ring wins over occupancy)
  auto go = [&](auto kern, int BM_, int BN_, int NT_) {
    const int nt = ((g.Cout + BM_ - 1) / BM_) * ((g.K + BN_ - 1) / BN_);
    if (side.nblk < 0) side.nblk = (int)std::max<int64_t>(1, (side.hi4 - side.lo4 + NT_ - 1) / NT_);
    kern<<<nt * splits + side.nblk, NT_, 0, s>>>((const bf16_t*)dy, (const bf16_t*)x, (float*)out, g, mps, ldo, side);
  };
  if (tile == 2) go(conv_wgrad_kernel<128, 128, 4, 2, 4>, 128, 128, 512);
  else go(conv_wgrad_kernel<64, 64, 4, 2, 4>, 64, 64, 512);
  DL_HIP_CHECK(hipGetLastError());
}

void conv_wgrad(uintptr_t dy, uintptr_t x, uintptr_t out, int B, int H, int W, int Cin, int Cout, int KS, int splits,
                int ldo, int tile, int atomic_creal, uintptr_t stream, const SideJob* side) {
  if (atomic_creal != 0) throw std::runtime_error("conv_wgrad: atomic split-K was removed in round 6 (pass 0)");
  if (tile & kTilePair) {  // pair-packed first layer (make_geom_pair): x is [B][Hp][Wp][4]
    if (Cin != 4) throw std::runtime_error("conv_wgrad: the pair-packed layout needs a 4-channel input");
    conv_wgrad_g(make_geom_pair(B, H, W, Cout, KS), dy, x, out, splits, ldo, tile & 15, stream, side);
    return;
  }
  conv_wgrad_g(make_geom(B, H, W, Cin, Cout, KS), dy, x, out, splits, ldo, tile, stream, side);
}

// out: fp32 [splits][Cout][ldo] weight-gradient slabs of a generalised-geometry
// conv: x as in conv_fwd_ex, dy [B][dHp][dWp][Cout] with the output interior at dpad.
void conv_wgrad_ex(uintptr_t dy, uintptr_t x, uintptr_t out, int B, int Ho, int Wo, int Hp, int Wp, int dHp, int dWp,
                   int dpad, int Cin, int Cout, int KH, int KW, int S, int splits, int ldo, int tile,
                   uintptr_t stream) {
  ConvGeom g = make_geom_ex(B, Ho, Wo, Hp, Wp, Cin, Cout, KH, KW, S);
  g.dsep = 1; g.dHp = dHp; g.dWp = dWp; g.dpad = dpad;
  if (dHp < Ho + dpad || dWp < Wo + dpad) throw std::runtime_error("conv_wgrad_ex: dy buffer too small");
  if ((int64_t)B * dHp * dWp * Cout >= (1ll << 31)) throw std::runtime_error("conv_wgrad_ex: dy too large");
  conv_wgrad_g(g, dy, x, out, splits, ldo, tile, stream);
}

void set_reduce_atomic_conv(int rows) {
  if (rows < 0 || rows > 64 || (rows & (rows - 1)) != 0)
    throw std::runtime_error("set_reduce_atomic: rows must be 0 or a power of two <= 64");
  const int v = rows;
  DL_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_red_atomic), &v, sizeof(int)));
}

template <bool ACC, bool OIHW = false>
static void slab_reduce_t(uintptr_t slabs, uintptr_t dst, int splits, int Cout, int taps, int Cp, int C,
                          uintptr_t stream) {
  auto s = as_stream(stream);
  const int g = slab_reduce_grid(splits, Cout, taps, C);
  const int tpo = slab_reduce_tpo(splits);
  if (tpo == 32)
    slab_reduce_kernel<32, ACC, OIHW><<<g, 256, 0, s>>>((const float*)slabs, (float*)dst, splits, Cout, taps, Cp, C);
  else if (tpo == 8)
    slab_reduce_kernel<8, ACC, OIHW><<<g, 256, 0, s>>>((const float*)slabs, (float*)dst, splits, Cout, taps, Cp, C);
  else
    slab_reduce_kernel<1, ACC, OIHW><<<g, 256, 0, s>>>((const float*)slabs, (float*)dst, splits, Cout, taps, Cp, C);
  DL_HIP_CHECK(hipGetLastError());
}

void slab_reduce(uintptr_t slabs, uintptr_t dst, int splits, int Cout, int taps, int Cp, int C, uintptr_t stream) {
  slab_reduce_t<false>(slabs, dst, splits, Cout, taps, Cp, C, stream);
}

// dst += sum of the slabs (the ResNet-50 1x1 weight gradients: plain slab
// stores + this reduce beat the atomic split-K 1.3-2.3x, profiles/r2_gemm1x1_wgrad_slab.jsonl)
void slab_reduce_add(uintptr_t slabs, uintptr_t dst, int splits, int Cout, int taps, int Cp, int C, uintptr_t stream) {
  slab_reduce_t<true>(slabs, dst, splits, Cout, taps, Cp, C, stream);
}

// dst [Cout][C][taps] (OIHW, the flat gradient of a KxK conv weight) += sum of the slabs
void slab_reduce_add_oihw(uintptr_t slabs, uintptr_t dst, int splits, int Cout, int taps, int Cp, int C,
                          uintptr_t stream) {
  slab_reduce_t<true, true>(slabs, dst, splits, Cout, taps, Cp, C, stream);
}

void weight_flip_transpose(uintptr_t w, uintptr_t wt, int Cout, int Cin, int KS, uintptr_t stream) {
  dim3 grid((Cin + 31) / 32, (Cout + 31) / 32, KS * KS);
  weight_flip_transpose_kernel<<<grid, 256, 0, as_stream(stream)>>>((const bf16_t*)w, (bf16_t*)wt, Cout, Cin, KS);
  DL_HIP_CHECK(hipGetLastError());
}

// table_dev: n TrEntry on the device (32 bytes each; built once by the caller,
// ops/conv.py WeightTransposes, and reused by every step / graph replay).
void transpose_many(uintptr_t table_dev, int n, int total_tiles, uintptr_t stream) {
  if (n <= 0) return;
  if (total_tiles <= 0) throw std::runtime_error("transpose_many: no tiles");
  transpose_many_kernel<<<total_tiles, 256, 0, as_stream(stream)>>>((const TrEntry*)table_dev, n);
  DL_HIP_CHECK(hipGetLastError());
}

int transpose_entry_bytes() { return (int)sizeof(TrEntry); }

void weights_to_cl(uintptr_t table_dev, int n, uintptr_t stream) {
  if (n <= 0) return;
  weights_to_cl_kernel<<<dim3(256, n), 256, 0, as_stream(stream)>>>((const ClEntry*)table_dev);
  DL_HIP_CHECK(hipGetLastError());
}

int cl_entry_bytes() { return (int)sizeof(ClEntry); }

void pack_weight(uintptr_t w, uintptr_t wp, int Cout, int taps, int C, int Cp, uintptr_t stream) {
  const int64_t total = (int64_t)Cout * taps * Cp;
  pack_weight_kernel<<<stream_grid(total), 256, 0, as_stream(stream)>>>((const float*)w, (bf16_t*)wp, Cout, taps, C,
                                                                        Cp);
  DL_HIP_CHECK(hipGetLastError());
}

void pad_channels(uintptr_t x, uintptr_t xp, int64_t P, int C, int Cp, uintptr_t stream) {
  pad_channels_kernel<<<stream_grid(P), 256, 0, as_stream(stream)>>>((const bf16_t*)x, (bf16_t*)xp, P, C, Cp);
  DL_HIP_CHECK(hipGetLastError());
}

}  // namespace dl
