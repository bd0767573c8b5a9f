// Shared by the implicit-GEMM convolution kernels of conv_igemm.hip (the one
// translation unit that includes this, so the __device__ globals below have
// one definition): the statistics reduction mode, ConvGeom and its host
// constructors, LDS swizzles, LDS-DMA wrappers, the forward / dgrad epilogues
// and the in-launch split-K combine.
#pragma once
#include "dl_common.h"

#include <algorithm>
#include <string>

namespace dl {

// Reduction mode of the train-mode BatchNorm statistics (set_reduce_atomic):
// 0 = one deterministic partial row per M tile (reduced by bn_finalize),
// R >= 1 (a power of two) = every workgroup atomically adds its per-channel
// totals into row (tile & (R-1)) of R zero-initialised [2][C] rows (the
// consumer -- bn_relu_pool_fwd_fin / the head -- sums the R rows and derives
// the BN coefficients itself: no finalize launch).  R = 1 is the single-row
// mode; R > 1 stripes the same-address atomics (measured: 1024 workgroups
// adding into one row serialise in the memory-side atomic unit, layer-1
// forward 31 vs 11 us).  Read once per workgroup epilogue (wave-uniform).
__device__ int g_red_atomic = 0;

__device__ __forceinline__ void put_stats(float* __restrict__ stats, int64_t row, int C, int n, float sa, float sb) {
  if (const int R = g_red_atomic) {
    float* s = stats + (int64_t)(row & (R - 1)) * 2 * C;
    unsafeAtomicAdd(s + n, sa);
    unsafeAtomicAdd(s + C + n, sb);
  } else {
    stats[row * 2 * C + n] = sa;
    stats[row * 2 * C + C + n] = sb;
  }
}

// BatchNorm backward reduce fused into a dgrad epilogue (BNRED): the dgrad's
// output is dP, the gradient of the pooled output of the previous block; for
// every stored element the epilogue also loads that block's pre-BN values y
// under the 2x2 pool window, routes dP to the window's argmax of relu(BN(y))
// and accumulates sum(dz) and sum(dz * xhat) per channel (bn_pool.hip
// bwd_reduce_body's arithmetic) -- the stand-alone reduce launch, and its
// re-read of dP, are gone.  rows: mode 0 = one partial row per M tile
// [T][sum dz (C); sum dz*xhat (C)], atomic modes = R striped rows
// [R][dgamma = sum dz*xhat (C); dbeta = sum dz (C)] (the layouts of the reduce).
// (BNR 2 / 3, the same reduce for the ResNet-50 channels-last BatchNorms in
// the 1x1 dgrad epilogues, measured slower than the reduce pass -- the
// epilogue's re-read of the BN input costs more than it saves,
// profiles/r5_resnet_bn_dgrad_ab.txt -- and was removed in round 6.)
struct BnRedArgs {
  const bf16_t* y;     // [B][2Ho][2Wo][C] pre-BN output of the previous block
  const float* coef;   // [4][C] mean, invstd, scale, shift
  float* rows;
};

// (A BatchNorm -> ReLU applied to the A operand on load of the ResNet-50
// b2 -> c3 1x1 GEMM measured slower than the apply pass it removed, 25.43 vs
// 24.64 ms/step, profiles/r4_resnet_bn_on_load_ab.txt; removed in round 6.)

struct ConvGeom {
  int B, H, W;
  int Hp, Wp;  // spatially zero-padded input dims (H + 2 pad, W + 2 pad)
  int Cin, Cout;
  int KS, pad;
  int logW, logHW, logC8;  // log2(W), log2(H*W) (valid when pow2), log2(Cin/8)
  int M, K, Kch;           // M = B*H*W, K = KS*KS*Cin, Kch = K/8
  int pow2;                // H and W powers of two (the region / c8 kernels and the shift addressing)
  int posm;                // streaming kernel: position-major M tiles with padding taps skipped (fwd_posm)
  float inv_HW, inv_W;     // reciprocals for the non-pow2 pixel decomposition (fdivmod)
  // Generalised geometry (make_geom_ex; the streaming forward and the wgrad
  // kernels only, non-pow2 addressing): tap (kh, kw) of output pixel (oh, ow)
  // reads padded input pixel (S*oh + kh, S*ow + kw) of the [B][Hp][Wp][Cin]
  // buffer; kernels may be KH x KW (K = KH*KW*Cin, taps row-major).
  int S, KH, KW;
  int kwstep;  // wgrad B chunks: tap column kw * kwstep (2: the pair-packed first layer, make_geom_pair)
  int dsep, dHp, dWp, dpad;  // wgrad: dy has its own buffer geometry [B][dHp][dWp][Cout], interior at dpad
  // epilogue output-row map (om != 0): output pixel (b, oh, ow) is stored at
  // row b*omHW + (omS*oh + omH0)*omW + omS*ow + omW0 (the phases of a strided
  // convolution's input gradient, written interleaved into the full tensor)
  int om, omS, omH0, omW0, omW, omHW;
};

// q = n / d, r = n - q*d for 0 <= n < 2^24 via a float reciprocal and one
// correction step (the ResNet-50 spatial sizes 56/28/14/7 are not powers of two)
__device__ __forceinline__ int fdivmod(int n, int d, float inv_d, int& r) {
  int q = (int)((float)n * inv_d);
  r = n - q * d;
  if (r < 0) { --q; r += d; }
  else if (r >= d) { ++q; r -= d; }
  return q;
}

// padded pixel index (b*Hp + S*oh)*Wp + S*ow of tap (0, 0) of output pixel m
// (any H, W; pow2 addressing only ever runs with S == 1)
__device__ __forceinline__ int out_pix(const ConvGeom& g, int m) {
  if (g.pow2) {
    const int b = m >> g.logHW, rem = m & ((1 << g.logHW) - 1);
    return (b * g.Hp + (rem >> g.logW)) * g.Wp + (rem & (g.W - 1));
  }
  int rem, ow;
  const int b = fdivmod(m, g.H * g.W, g.inv_HW, rem);
  const int oh = fdivmod(rem, g.W, g.inv_W, ow);
  return (b * g.Hp + g.S * oh) * g.Wp + g.S * ow;
}

// wgrad with a separate dy geometry (g.dsep): interior pixel of output m in dy
__device__ __forceinline__ int dy_pix(const ConvGeom& g, int m) {
  int rem, ow;
  const int b = fdivmod(m, g.H * g.W, g.inv_HW, rem);
  const int oh = fdivmod(rem, g.W, g.inv_W, ow);
  return (b * g.dHp + oh + g.dpad) * g.dWp + ow + g.dpad;
}

// epilogue row of output pixel m under the output map (g.om)
__device__ __forceinline__ int om_row(const ConvGeom& g, int m) {
  int rem, ow;
  const int b = fdivmod(m, g.H * g.W, g.inv_HW, rem);
  const int oh = fdivmod(rem, g.W, g.inv_W, ow);
  return b * g.omHW + (g.omS * oh + g.omH0) * g.omW + g.omS * ow + g.omW0;
}

// K steps (64 channels of one tap) of a position-major tile at output pixel
// pos: the taps whose input pixel is inside the image, times Cin / 64
__host__ __device__ __forceinline__ int posm_nk(const ConvGeom& g, int pos) {
  const int oh = pos / g.W, ow = pos - oh * g.W;
  const int th = min(g.KS, g.H + g.pad - oh) - max(0, g.pad - oh);
  const int tw = min(g.KS, g.W + g.pad - ow) - max(0, g.pad - ow);
  return th * tw * (g.Cin / 64);
}

static int ilog2_exact(int v, const char* what) {
  int l = 0;
  while ((1 << l) < v) ++l;
  if ((1 << l) != v) throw std::runtime_error(std::string(what) + " must be a power of two");
  return l;
}

static bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

static ConvGeom make_geom(int B, int H, int W, int Cin, int Cout, int KS) {
  ConvGeom g{};  // value-initialised: a field added later must not read stack garbage
  g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.KS = KS; g.pad = KS / 2;
  g.Hp = H + 2 * g.pad; g.Wp = W + 2 * g.pad;
  if (KS % 2 != 1) throw std::runtime_error("conv: odd kernel size required");
  if (Cin < 8) throw std::runtime_error("conv: Cin must be >= 8 (pad the input channels)");
  g.pow2 = is_pow2(W) && is_pow2(H) ? 1 : 0;
  g.posm = 0;
  g.S = 1; g.KH = KS; g.KW = KS; g.kwstep = 1;
  g.dsep = 0; g.dHp = g.Hp; g.dWp = g.Wp; g.dpad = g.pad;
  g.om = 0; g.omS = 1; g.omH0 = 0; g.omW0 = 0; g.omW = W; g.omHW = H * W;
  g.logW = g.pow2 ? ilog2_exact(W, "W") : 0;
  g.logHW = g.pow2 ? ilog2_exact(H * W, "H*W") : 0;
  g.inv_HW = 1.0f / (float)(H * W);
  g.inv_W = 1.0f / (float)W;
  g.logC8 = ilog2_exact(Cin / 8, "Cin/8");
  if (!g.pow2 && (int64_t)B * H * W >= (1 << 24))
    throw std::runtime_error("conv: non-power-of-two H/W needs B*H*W < 2^24 (float pixel decomposition)");
  g.M = B * H * W;
  g.K = KS * KS * Cin;
  g.Kch = g.K / 8;
  if ((int64_t)B * g.Hp * g.Wp * std::max(Cin, Cout) >= (1ll << 31) || (int64_t)Cout * g.K >= (1ll << 31))
    throw std::runtime_error("conv: operand too large for 32-bit offsets");
  return g;
}

// The pair-packed first layer (4-channel padded input, <= 4 real channels):
// one 16-byte K chunk = channels 0-3 of two horizontally adjacent taps
// (dl_common.h pack1_index, cp = -KS), K = KS * ceil(KS/2) * 8.  For the
// wgrad kernel's B operand the chunk is 2 adjacent pixels of the [.][Wp][4]
// buffer: KW = ceil(KS/2) chunk columns at tap column 2 * kw.
static ConvGeom make_geom_pair(int B, int H, int W, int Cout, int KS) {
  ConvGeom g = make_geom(B, H, W, 8, Cout, KS);
  const int cpr = (KS + 1) / 2;
  g.Cin = 4; g.logC8 = 0;
  g.KW = cpr; g.kwstep = 2;
  g.Kch = KS * cpr; g.K = g.Kch * 8;
  return g;
}

// ---- generalised geometry (strided / KH x KW / phase-mapped convolutions) ----
// The ResNet-50 convolutions that are not stride-1 odd-square: the stride-2
// 1x1 downsample and 3x3 convs, the stem (a stride-2 7x7 over 3 channels,
// rewritten as a 4x4 stride-1 conv over its 2x2 space-to-depth image: 12 -> 16
// channels), and the stride-2 convs' input gradients (one phase conv per
// output parity, stored interleaved through the epilogue's output map).
// Streaming forward kernel and wgrad kernel only, float-reciprocal pixel
// addressing (never the pow2 / region / c8 paths).
static ConvGeom make_geom_ex(int B, int Ho, int Wo, int Hp, int Wp, int Cin, int Cout, int KH, int KW, int S) {
  if (KH < 1 || KW < 1 || S < 1) throw std::runtime_error("conv_ex: bad kernel / stride");
  if (Hp < S * (Ho - 1) + KH || Wp < S * (Wo - 1) + KW) throw std::runtime_error("conv_ex: input buffer too small");
  ConvGeom g = make_geom(B, Ho, Wo, Cin, Cout, 1);
  g.KS = std::max(KH, KW);
  g.pad = 0;
  g.Hp = Hp; g.Wp = Wp;
  g.S = S; g.KH = KH; g.KW = KW;
  g.dHp = Ho; g.dWp = Wo; g.dpad = 0;
  g.pow2 = 0;
  g.K = KH * KW * Cin;
  g.Kch = g.K / 8;
  if ((int64_t)B * Ho * Wo >= (1 << 24)) throw std::runtime_error("conv_ex: B*Ho*Wo must be < 2^24");
  if ((int64_t)B * Hp * Wp * std::max(Cin, Cout) >= (1ll << 31) || (int64_t)Cout * g.K >= (1ll << 31))
    throw std::runtime_error("conv_ex: operand too large for 32-bit offsets");
  return g;
}

// --------------------------------------------------------------------------
// LDS swizzles (16-byte chunk granularity)
// --------------------------------------------------------------------------
// Row reads (ds_read_b128, 16 lanes = 16 consecutive rows at one chunk): rows
// of CPR chunks; rows r and r + 16/CPR share a 256-B bank row, so XOR the
// chunk with (r / (16/CPR)) mod CPR.
template <int CPR>
__device__ __forceinline__ int swz_row(int row, int ch) {
  constexpr int RPB = 16 / CPR;  // rows per 256-B bank row
  return row * CPR + (ch ^ ((row / RPB) & (CPR - 1)));
}

// Transposed reads (ds_read_b64_tr_b16): a 32-lane half reads rows
// {r0..r0+3, r0+8..r0+11} (or +4) x two adjacent chunks; the XOR spreads those
// 8 rows over distinct 32-byte slot pairs of the 256-byte bank row.
// CPR = 32 (512-B rows, the 256-wide wgrad tile): chunks ch and ch + 16 share
// banks, so the CPR = 16 XOR on the low four chunk bits spreads the rows the same.
template <int CPR>
__device__ __forceinline__ int swz_tr(int row, int ch) {
  if constexpr (CPR == 16 || CPR == 32) {
    const int f = 2 * ((row & 3) | (((row >> 3) & 1) << 2));
    return row * CPR + (ch ^ f);
  } else {
    static_assert(CPR == 8, "swz_tr: rows of 8 or 16 chunks");
    const int f = 2 * (((row >> 1) & 1) | (((row >> 3) & 1) << 1));
    return row * 8 + (ch ^ f);
  }
}

__device__ __forceinline__ f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

typedef short s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ s16x4 ds_read_tr16(const void* lds_byte_ptr) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lds_byte_ptr));
}

// XCD-aware tile order: consecutive tiles (sharing weight panels) on one XCD.
__device__ __forceinline__ int xcd_swizzle(int bid, int nwg) {
  const int q = nwg / 8, r = nwg % 8, xcd = bid % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
}

// --------------------------------------------------------------------------
// LDS-DMA staging (global_load_lds_dwordx4): one wave instruction writes
// 64 lanes x 16 B = 1 KiB contiguously at a wave-uniform LDS base.  The LDS
// image stays lane-linear; the swizzle is applied to the per-lane SOURCE chunk
// (the XORs above are involutions), and zero padding (halo taps, K tails,
// M/N tails) is read from a 16-byte zero line in global memory.
// --------------------------------------------------------------------------
__device__ uint4 g_zero16[4];

__device__ __forceinline__ unsigned long long stamp() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}

__device__ __forceinline__ void glds16(const void* src, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// Buffer-descriptor LDS-DMA (buffer_load_dwordx4 ... offen lds): per-lane 32-bit
// byte offset in a VGPR + wave-uniform byte offset in an SGPR (soffset), so a
// load whose per-lane part is loop-invariant costs no VALU at all; offsets at
// or past `bytes` read zeros (hardware range check), which replaces the zero
// line for K/M tails.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
constexpr unsigned kOOB = 0x40000000u;  // a voffset past every operand: loads zeros
// streaming fwd/dgrad kernel main loop (set_conv_fwd_pf; A/B): 1 = register
// prefetch of the next step's fragments + unconditional DMA pipeline (4 stages)
__constant__ int g_fwd_pf = 1;

__device__ __forceinline__ rsrc_t make_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}

__device__ __forceinline__ void blds16(rsrc_t r, unsigned voff, unsigned soff, void* lds_wave_base) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds_wave_base, 16, (int)voff,
                                           (int)soff, 0, 0);
}

// The same LDS-DMA as inline asm, for loops that read the staged tiles with
// ds_read_b64_tr_b16: hipcc (ROCm 7.2) puts an `s_waitcnt vmcnt(0)` in front of
// every __builtin_amdgcn_ds_read_tr16_b64 while a builtin LDS-DMA may be in
// flight (it cannot tell which LDS bytes the transposed read touches), which
// drains the whole DMA ring at every K step -- the wgrad kernel waited for the
// stages it had just issued.  Issued from asm, the DMA is invisible to that
// analysis; the kernel's own counted `s_waitcnt vmcnt(N)` before each barrier
// orders it (and the compiler still tracks lgkmcnt for the tr16 results).
// M0 carries the LDS base (nothing else in those kernels uses M0).
typedef int i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4 make_rsrc4(const void* p, unsigned bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(p);
  return i32x4{(int)(unsigned)a, (int)(unsigned)(a >> 32), (int)bytes, 0x00020000};
}

__device__ __forceinline__ void blds16_asm(const i32x4& r, unsigned voff, unsigned soff, void* lds_wave_base) {
  // wave-uniform operands in SGPRs (readfirstlane: the compiler may not prove them uniform)
  const unsigned m0 = __builtin_amdgcn_readfirstlane(
      (unsigned)reinterpret_cast<unsigned long long>((__attribute__((address_space(3))) char*)lds_wave_base));
  const unsigned so = __builtin_amdgcn_readfirstlane(soff);
  const i32x4 rs{__builtin_amdgcn_readfirstlane(r[0]), __builtin_amdgcn_readfirstlane(r[1]),
                 __builtin_amdgcn_readfirstlane(r[2]), __builtin_amdgcn_readfirstlane(r[3])};
  asm volatile("s_mov_b32 m0, %3\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(voff), "s"(rs), "s"(so),
               "s"(m0)
               : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// wait until at most `n` stages (of LPS LDS-DMA loads each) are still in flight
template <int LPS>
__device__ __forceinline__ void wait_stages(int n) {
  switch (n) {
    case 0: wait_vmcnt<0>(); break;
    case 1: wait_vmcnt<LPS>(); break;
    case 2: wait_vmcnt<2 * LPS>(); break;
    case 3: wait_vmcnt<3 * LPS>(); break;
    case 4: wait_vmcnt<(4 * LPS < 63 ? 4 * LPS : 63)>(); break;
    case 5: wait_vmcnt<(5 * LPS < 63 ? 5 * LPS : 63)>(); break;
    default: wait_vmcnt<(6 * LPS < 63 ? 6 * LPS : 63)>(); break;
  }
}

__device__ __forceinline__ void block_sync_lds() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// Forward / dgrad epilogue shared by the implicit-GEMM kernels: SLAB = fp32
// split-K partials; else bf16 y (+ STATS: per-M-tile channel sum / sum of
// squares of exactly the stored bf16 values, one deterministic partial row
// per M tile, reduced through `smem`, which the caller no longer uses).
// ADD (!SLAB): y = bf16(acc + addend) with addend a bf16 [M][Cout] tensor passed
// through the (otherwise unused) slab pointer -- the dgrad of a 1x1 conv whose
// input also feeds a residual branch adds that branch's gradient in place of a
// separate elementwise pass (ops/conv.py).
template <int BM, int BN, bool STATS, bool SLAB, int WM, int WN, bool ADD = false>
__device__ __forceinline__ void conv_fwd_epilogue(const f32x4 (&acc)[BM / WM / 16][BN / WN / 16], const ConvGeom& g,
                                                  bf16_t* __restrict__ y, float* __restrict__ stats,
                                                  float* __restrict__ slab, int split, int tm, int m0, int n0,
                                                  char* smem, int pm_b0 = 0, int pm_pos = 0) {
  // position-major tiles (g.posm): logical row ml -> stored row (pm_b0 + ml - m0) * HW + pm_pos
  auto phys = [&](int ml) {
    return g.posm ? (pm_b0 + ml - m0) * (g.H * g.W) + pm_pos : (g.om ? om_row(g, ml) : ml);
  };
  constexpr int NT = 64 * WM * WN, TM = BM / WM, TN = BN / WN, FM = TM / 16, FN = TN / 16;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = tid >> 6, wm = wid / WN, wn = wid % WN;
  const int col_l = lane & 15, rq = lane >> 4;
  if constexpr (SLAB) {
    float* o = slab + (int64_t)split * g.M * g.Cout;
#pragma unroll
    for (int a = 0; a < FM; ++a)
#pragma unroll
      for (int b = 0; b < FN; ++b) {
        const int n = n0 + wn * TN + b * 16 + col_l;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + wm * TM + a * 16 + rq * 4 + r;
          if (m < g.M && n < g.Cout) o[(int64_t)phys(m) * g.Cout + n] = acc[a][b][r];
        }
      }
  } else {
    float s1[FN], s2[FN];
#pragma unroll
    for (int b = 0; b < FN; ++b) { s1[b] = 0.f; s2[b] = 0.f; }
#pragma unroll
    for (int a = 0; a < FM; ++a) {
#pragma unroll
      for (int b = 0; b < FN; ++b) {
        const int n = n0 + wn * TN + b * 16 + col_l;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + wm * TM + a * 16 + rq * 4 + r;
          float v0 = acc[a][b][r];
          const int64_t mo = (int64_t)phys(m) * g.Cout + n;
          if constexpr (ADD) {  // (ADD: stats carries the addend's optional mask bits, see conv_fwd_add)
            const uint8_t* mb = reinterpret_cast<const uint8_t*>(stats);
            if (m < g.M && n < g.Cout &&
                (mb == nullptr || ((mb[(int64_t)phys(m) * (g.Cout >> 3) + (n >> 3)] >> (n & 7)) & 1u)))
              v0 += bf16_to_f32(reinterpret_cast<const bf16_t*>(slab)[mo]);
          }
          const bf16_t hv = f32_to_bf16(v0);
          if (m < g.M && n < g.Cout) y[mo] = hv;
          if constexpr (STATS) {
            const float v = m < g.M ? bf16_to_f32(hv) : 0.f;  // statistics of exactly what is stored
            s1[b] += v;
            s2[b] += v * v;
          }
        }
      }
    }
    if constexpr (STATS) {
      __syncthreads();  // every wave done with the LDS ring (no DMA in flight: the K loop drained it)
      float* red = reinterpret_cast<float*>(smem);  // [WM][2][BN]
#pragma unroll
      for (int b = 0; b < FN; ++b) {
        s1[b] += __shfl_xor(s1[b], 16, 64);
        s1[b] += __shfl_xor(s1[b], 32, 64);
        s2[b] += __shfl_xor(s2[b], 16, 64);
        s2[b] += __shfl_xor(s2[b], 32, 64);
        if (rq == 0) {
          red[(wm * 2 + 0) * BN + wn * TN + b * 16 + col_l] = s1[b];
          red[(wm * 2 + 1) * BN + wn * TN + b * 16 + col_l] = s2[b];
        }
      }
      __syncthreads();
      for (int c = tid; c < BN; c += NT) {
        const int n = n0 + c;
        if (n < g.Cout) {
          float sa = 0.f, sb = 0.f;
#pragma unroll
          for (int q = 0; q < WM; ++q) { sa += red[(q * 2) * BN + c]; sb += red[(q * 2 + 1) * BN + c]; }
          put_stats(stats, tm, g.Cout, n, sa, sb);
        }
      }
    }
  }
}

// Inclusive sum over the 16 lanes of each DPP row: lane 15 of the row ends
// with the row total (row_shr 1, 2, 4, 8 with zero fill; fixed order).
__device__ __forceinline__ float row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, true));
  return v;
}

// Transposed epilogue (region kernel, and the streaming kernel whenever its
// wave tile has an even number of N fragments).  The MFMAs compute C^T
// (weights as the A operand), so lane l holds, per 16-pixel M fragment a and
// N-fragment pair p, the 8 CONSECUTIVE channels n0 + wn*TN + 32p + 8*(l>>4) +
// 0..7 of pixel m0 + wm*TM + 16a + (l&15) (fragments 2p / 2p+1 hold channel
// quads 0..3 / 4..7, see the B row map b_frag_row): one 16-byte bf16 store (or
// two 16-byte fp32 slab stores) per (a, p) instead of 8 scattered 2-byte
// stores.  Measured on the ResNet-50 1x1 shapes (scripts/bench_gemm1x1.py):
// the write-heavy GEMMs (Cout = 4 Cin) ran at ~2.6 TB/s with the scattered
// stores vs ~5 TB/s for the read-heavy ones.  BN statistics: DPP row sums
// over the 16 pixels of a lane group, then a fixed-order sum over the WM wave
// rows through LDS (deterministic).  ADD: + a bf16 [M][Cout] addend (16-byte
// loads), passed through the slab pointer.
template <int BM, int BN, bool STATS, bool SLAB, int WM, int WN, int FM, int FN, bool ADD = false, int BNR = 0>
__device__ __forceinline__ void conv_fwd_epilogue_t(const f32x4 (&acc)[FM][FN], const ConvGeom& g,
                                                    bf16_t* __restrict__ y, float* __restrict__ stats,
                                                    float* __restrict__ slab, int split, int tm, int m0, int n0,
                                                    char* smem, int pm_b0 = 0, int pm_pos = 0,
                                                    const BnRedArgs br = BnRedArgs{}) {
  constexpr int NT = 64 * WM * WN, TM = BM / WM, TN = BN / WN, NP = FN / 2;
  static_assert(!(ADD && (SLAB || STATS)), "ADD: plain bf16 output only");
  constexpr bool BNRED = BNR != 0;
  static_assert(BNR == 0 || BNR == 1, "BNR 1: the pooled BN backward reduce");
  static_assert(!(BNRED && (SLAB || STATS || ADD)), "BNRED: plain bf16 output");
  static_assert(FN % 2 == 0, "N fragments pair up");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = tid >> 6, wm = wid / WN, wn = wid % WN;
  const int nl = wn * TN + 8 * (lane >> 4);  // + 32p: local channel of the lane's 8-run
  float s1[NP][8], s2[NP][8];
#pragma unroll
  for (int q = 0; q < NP; ++q)
#pragma unroll
    for (int k = 0; k < 8; ++k) { s1[q][k] = 0.f; s2[q][k] = 0.f; }
  // vmcnt(0) before any output store: the k loop's trailing LDS-DMA (zero-fill
  // past nk, inline asm the compiler does not track) has landed, so the LDS-only
  // barriers of the statistics below need not wait for this tile's stores
  if constexpr ((STATS || BNRED) && !SLAB) __builtin_amdgcn_s_waitcnt(0x0F70);
  // BNRED: the lane's channels are fixed per q -- their BN coefficients once
  float rmu[BNRED ? NP : 1][8], ris[BNRED ? NP : 1][8], rsc[BNRED ? NP : 1][8], rsh[BNRED ? NP : 1][8];
  if constexpr (BNR == 1) {
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const int n = n0 + nl + 32 * q;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        rmu[q][k] = br.coef[n + k];
        ris[q][k] = br.coef[g.Cout + n + k];
        rsc[q][k] = br.coef[2 * g.Cout + n + k];
        rsh[q][k] = br.coef[3 * g.Cout + n + k];
      }
    }
  }
  // the stored row of fragment a (position-major tiles hold image pm_b0 + r at
  // output pixel pm_pos)
  auto row_of = [&](int a, bool& ok) {
    const int ml = m0 + wm * TM + a * 16 + (lane & 15);
    ok = ml < g.M;
    return g.posm ? (pm_b0 + ml - m0) * (g.H * g.W) + pm_pos : (g.om && ok ? om_row(g, ml) : ml);
  };
  // ADD (plain): every fragment's addend (and mask byte) loaded before the
  // first store -- y may alias it as far as the compiler knows, so a load left
  // in the loop below waits behind each store, one memory latency per
  // fragment: ResNet-50 c1 dgrads with the residual addend 827 vs 956 / 538 vs
  // 575 us per step (profiles/r5_resnet_bn_dgrad_ab.txt).  Not for BNR 1
  // (the CIFAR region dgrad's pool windows: 24.3 vs 23.7-24.0 us)
  constexpr bool PA = ADD && BNR == 0;
  uint4 pad_[PA ? FM : 1][PA ? NP : 1];
  unsigned padm_[PA ? FM : 1][PA ? NP : 1];
  if constexpr (PA) {
#pragma unroll
    for (int a = 0; a < FM; ++a) {
      bool ok;
      const int m = row_of(a, ok);
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        const int n = n0 + nl + 32 * q;
        const int64_t o = (int64_t)(ok ? m : 0) * g.Cout + n, ob = (int64_t)(ok ? m : 0) * (g.Cout >> 3) + (n >> 3);
        {
          // (ADD: stats carries the addend's optional mask bits, conv_fwd_add: the
          // residual gradient = dy of the BN + residual + ReLU, masked here)
          const uint8_t* mb = reinterpret_cast<const uint8_t*>(stats);
          pad_[a][q] = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(slab) + o);
          padm_[a][q] = mb != nullptr ? mb[ob] : 0xffu;
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < FM; ++a) {
    bool ok;
    const int m = row_of(a, ok);
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const int n = n0 + nl + 32 * q;
      float v[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[j] = acc[a][2 * q][j]; v[4 + j] = acc[a][2 * q + 1][j]; }
      if constexpr (ADD) {
        if (ok) {
          const uint8_t* mb = reinterpret_cast<const uint8_t*>(stats);
          const uint4 ad = PA ? pad_[a][q]
                                    : *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(slab) +
                                                                      (int64_t)m * g.Cout + n);
          const unsigned bits = PA ? padm_[a][q] : (mb != nullptr ? mb[(int64_t)m * (g.Cout >> 3) + (n >> 3)] : 0xffu);
          const float a8[8] = {lo_bf16(ad.x), hi_bf16(ad.x), lo_bf16(ad.y), hi_bf16(ad.y),
                               lo_bf16(ad.z), hi_bf16(ad.z), lo_bf16(ad.w), hi_bf16(ad.w)};
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] += (bits >> k) & 1u ? a8[k] : 0.f;
        }
      }
      if constexpr (SLAB) {
        float* o = slab + ((int64_t)split * g.M + m) * g.Cout + n;
        if (ok) {
          *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
          *reinterpret_cast<float4*>(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
      } else {
        const uint4 pk = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                                    pack_bf16x2(v[6], v[7]));
        if (ok) *reinterpret_cast<uint4*>(y + (int64_t)m * g.Cout + n) = pk;
        if constexpr (BNR == 1) {
          if (ok) {
            // pooled pixel m = (b, oh, ow) of the [B][H][W] dgrad output; its window in y
            int rem, ow;
            const int b = fdivmod(m, g.H * g.W, g.inv_HW, rem);
            const int oh = fdivmod(rem, g.W, g.inv_W, ow);
            const int W2 = 2 * g.W;
            const bf16_t* base = br.y + ((int64_t)(b * 2 * g.H + 2 * oh) * W2 + 2 * ow) * g.Cout + n;
            const uint4 w0 = *reinterpret_cast<const uint4*>(base);
            const uint4 w1 = *reinterpret_cast<const uint4*>(base + g.Cout);
            const uint4 w2 = *reinterpret_cast<const uint4*>(base + (int64_t)W2 * g.Cout);
            const uint4 w3 = *reinterpret_cast<const uint4*>(base + (int64_t)W2 * g.Cout + g.Cout);
            const uint4 wv[4] = {w0, w1, w2, w3};
            const float gd[8] = {lo_bf16(pk.x), hi_bf16(pk.x), lo_bf16(pk.y), hi_bf16(pk.y),
                                 lo_bf16(pk.z), hi_bf16(pk.z), lo_bf16(pk.w), hi_bf16(pk.w)};
            float yv[4][8];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              yv[w][0] = lo_bf16(wv[w].x); yv[w][1] = hi_bf16(wv[w].x); yv[w][2] = lo_bf16(wv[w].y);
              yv[w][3] = hi_bf16(wv[w].y); yv[w][4] = lo_bf16(wv[w].z); yv[w][5] = hi_bf16(wv[w].z);
              yv[w][6] = lo_bf16(wv[w].w); yv[w][7] = hi_bf16(wv[w].w);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              float best = -INFINITY;
              int arg = 0;
#pragma unroll
              for (int w = 0; w < 4; ++w) {
                const float r = fmaxf(fmaf(rsc[q][k], yv[w][k], rsh[q][k]), 0.f);
                if (r > best) { best = r; arg = w; }
              }
#pragma unroll
              for (int w = 0; w < 4; ++w) {
                const float dz = (w == arg && best > 0.f) ? gd[k] : 0.f;
                s1[q][k] += dz;
                s2[q][k] += dz * (yv[w][k] - rmu[q][k]) * ris[q][k];
              }
            }
          }
        }
        if constexpr (STATS) {
          const float h[8] = {lo_bf16(pk.x), hi_bf16(pk.x), lo_bf16(pk.y), hi_bf16(pk.y),
                              lo_bf16(pk.z), hi_bf16(pk.z), lo_bf16(pk.w), hi_bf16(pk.w)};
#pragma unroll
          for (int k = 0; k < 8; ++k) {  // statistics of exactly what is stored
            const float hv = ok ? h[k] : 0.f;
            s1[q][k] += hv;
            s2[q][k] += hv * hv;
          }
        }
      }
    }
  }
  if constexpr ((STATS || BNRED) && !SLAB) {
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
      for (int k = 0; k < 8; ++k) { s1[q][k] = row16_sum(s1[q][k]); s2[q][k] = row16_sum(s2[q][k]); }
    // LDS-only barriers: __syncthreads() would also wait for this wave's output
    // stores (vmcnt(0)) before the tile's statistics, exposing their latency per
    // tile.  No LDS-DMA is in flight (waited above); the ring's reads are lgkm.
    block_sync_lds();  // lgkmcnt(0) (a compiler memory fence) + barrier: every wave done with the ring
    float* red = reinterpret_cast<float*>(smem);  // [WM][2][BN]
    if ((lane & 15) == 15) {
#pragma unroll
      for (int q = 0; q < NP; ++q)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          red[(wm * 2 + 0) * BN + nl + 32 * q + k] = s1[q][k];
          red[(wm * 2 + 1) * BN + nl + 32 * q + k] = s2[q][k];
        }
    }
    block_sync_lds();
    for (int c = tid; c < BN; c += NT) {
      float sa = 0.f, sb = 0.f;
#pragma unroll
      for (int q = 0; q < WM; ++q) { sa += red[(q * 2) * BN + c]; sb += red[(q * 2 + 1) * BN + c]; }
      if constexpr (BNR == 1) {
        // sa = sum dz, sb = sum dz*xhat; atomic rows hold [dgamma; dbeta] (the reduce's layouts)
        if (g_red_atomic) put_stats(br.rows, tm, g.Cout, n0 + c, sb, sa);
        else put_stats(br.rows, tm, g.Cout, n0 + c, sa, sb);
      } else {
        put_stats(stats, tm, g.Cout, n0 + c, sa, sb);
      }
    }
  }
}

// B-tile chunk swizzle of the region kernel: conflict-free ds_read_b128 for
// its permuted fragment rows 8(i>>2) + 4b + (i&3) (and for identity rows)
__device__ __forceinline__ int swz_b(int row) { return ((row >> 1) ^ (row >> 3)) & 7; }

// B fragment row of lane group i (0..15) for N fragment b of a transposed
// (C^T) wave tile: fragment pair p = b/2 covers 32 channels, and lane group
// i>>2 reads channels 8(i>>2) + 4(b&1) + (i&3), so the accumulator lane of
// output row 4(l>>4)+r holds channel 32p + 8(l>>4) + 4(b&1) + r.
__device__ __forceinline__ int b_frag_row(int b, int i) { return 32 * (b >> 1) + 8 * (i >> 2) + 4 * (b & 1) + (i & 3); }

// In-launch split-K combine (FIX, conv_fwd_fix).  Every K slice of a tile
// publishes its fp32 partial tile write-through (sc1 16-byte buffer stores),
// drains its stores (every wave: s_waitcnt vmcnt(0)), and after a workgroup
// barrier one lane adds to the tile's arrival counter (relaxed, agent scope).
// The slice whose add returns splits - 1 is the reducer: it reads EVERY slice
// (its own included) with sc1 loads -- which bypass the CU's L1, so no acquire
// fence is needed -- and sums them in slice order, bitwise the sums of
// splitk_combine / combine_bwd_reduce; it then runs the plain bf16 epilogue
// (BN statistics, or the BN backward reduce of the block below).  The other
// slices exit.  Correct for any placement of a tile's slices over CUs and
// XCDs (cdna_hip_programming.md §5 "in-launch split-K reduction", §6
// Guideline 16: sc1 payload + drained stores + counter, sc1 loads): the
// separate combine launch and its ~1.5-2 us kernel boundary are gone.  The
// reducer resets the counter for the next launch (the counters start zeroed:
// a __device__ array).
__device__ int g_fix_cnt[1 << 16];
constexpr int kFixCnt = 1 << 16;

template <int BM, int BN, int WM, int WN, int FM, int FN>
__device__ __forceinline__ bool splitk_fixup(f32x4 (&acc)[FM][FN], const ConvGeom& g, float* __restrict__ slab,
                                             int split, int splits, int m0, int n0, int pm_b0, int pm_pos, int* cnt,
                                             char* smem) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  constexpr int TM = BM / WM, TN = BN / WN, NP = FN / 2;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = tid >> 6, wm = wid / WN, wn = wid % WN;
  const int nl = wn * TN + 8 * (lane >> 4);
  const rsrc_t sr = make_rsrc(slab, (unsigned)((int64_t)splits * g.M * g.Cout * 4));
  unsigned off[FM][NP];  // byte offset of the lane's 8 channels in slice 0 (or kOOB: M tail)
#pragma unroll
  for (int a = 0; a < FM; ++a) {
    const int ml = m0 + wm * TM + a * 16 + (lane & 15);
    const int row = g.posm ? (pm_b0 + ml - m0) * (g.H * g.W) + pm_pos : ml;
#pragma unroll
    for (int q = 0; q < NP; ++q)
      off[a][q] = ml < g.M ? (unsigned)(((int64_t)row * g.Cout + n0 + nl + 32 * q) * 4) : kOOB;
  }
  const unsigned sstride = (unsigned)((int64_t)g.M * g.Cout * 4);
#pragma unroll
  for (int a = 0; a < FM; ++a)
#pragma unroll
    for (int q = 0; q < NP; ++q)
      if (off[a][q] != kOOB) {
        const unsigned o = off[a][q] + (unsigned)split * sstride;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[a][2 * q]), sr, (int)o, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[a][2 * q + 1]), sr, (int)(o + 16), 0, 16);
      }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave: its slice is out of the CU
  __syncthreads();
  int* flag = reinterpret_cast<int*>(smem);  // the k loop is done with the ring (barrier above)
  if (tid == 0) {
    const int t = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = t == splits - 1 ? 1 : 0;
    if (last) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    flag[0] = last;
  }
  __syncthreads();
  const int last = flag[0];
  __syncthreads();  // flag read by every wave before the epilogue reuses the LDS
  if (!last) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (no instruction) keep the loads below the counter
  if (splits <= 4) {
    // the other slices only (the reducer's own is in registers): up to 3 loads
    // per fragment half, all in flight; unconditional (a slice index past the
    // others re-reads the last one and is not used)
    u32x4 ld[3][FM][NP][2];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int o_s = min(u < split ? u : u + 1, splits - 1);  // u-th slice other than `split`
      const unsigned so = (unsigned)o_s * sstride;
#pragma unroll
      for (int a = 0; a < FM; ++a)
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          const unsigned o = off[a][q] == kOOB ? kOOB : off[a][q] + so;
          ld[u][a][q][0] = __builtin_amdgcn_raw_buffer_load_b128(sr, (int)o, 0, 16);
          ld[u][a][q][1] = __builtin_amdgcn_raw_buffer_load_b128(sr, (int)(o + 16), 0, 16);
        }
    }
#pragma unroll
    for (int a = 0; a < FM; ++a)
#pragma unroll
      for (int q = 0; q < NP; ++q)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4 own = acc[a][2 * q + h];
          f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < 4; ++s) {  // slice order; selects on values, never on loads
            const f32x4 lo = __builtin_bit_cast(f32x4, ld[s < 3 ? s : 2][a][q][h]);
            const f32x4 hi = __builtin_bit_cast(f32x4, ld[s > 0 ? s - 1 : 0][a][q][h]);
            const f32x4 x = s < split ? lo : (s == split ? own : hi);
            if (s == 0) d = x;  // (0 + x would turn -0 into +0)
            else if (s < splits) d = f32x4{d[0] + x[0], d[1] + x[1], d[2] + x[2], d[3] + x[3]};
          }
          acc[a][2 * q + h] = d;
        }
    return true;
  }
  // more slices: every slice (its own re-read), 4 at a time with all their loads in flight
#pragma unroll
  for (int a = 0; a < FM; ++a)
#pragma unroll
    for (int b = 0; b < FN; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s0 = 0; s0 < splits; s0 += 4) {
    u32x4 ld[4][FM][NP][2];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned so = (unsigned)min(s0 + u, splits - 1) * sstride;
#pragma unroll
      for (int a = 0; a < FM; ++a)
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          const unsigned o = off[a][q] == kOOB ? kOOB : off[a][q] + so;
          ld[u][a][q][0] = __builtin_amdgcn_raw_buffer_load_b128(sr, (int)o, 0, 16);
          ld[u][a][q][1] = __builtin_amdgcn_raw_buffer_load_b128(sr, (int)(o + 16), 0, 16);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool use = s0 + u < splits;
#pragma unroll
      for (int a = 0; a < FM; ++a)
#pragma unroll
        for (int q = 0; q < NP; ++q)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const f32x4 v = __builtin_bit_cast(f32x4, ld[u][a][q][h]);
            f32x4& d = acc[a][2 * q + h];
            if (s0 + u == 0) d = v;
            else if (use) d = f32x4{d[0] + v[0], d[1] + v[1], d[2] + v[2], d[3] + v[3]};
          }
    }
  }
  return true;
}

}  // namespace dl
