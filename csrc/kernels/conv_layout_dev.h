// Small layout kernels of conv_igemm.hip: the split-K slab reduce, weight
// transposes, channel pack / pad, and the per-step operand preparation.
#pragma once
#include "dl_common.h"
#include "prep_dev.h"
#include "slab_reduce_dev.h"
#include "wtrans_dev.h"

namespace dl {

// Sum `splits` fp32 slabs [splits][Cout][Kp] (Kp = taps*Cp) into dst
// [Cout][taps][C] (body and options: slab_reduce_dev.h).
template <int TPO, bool ACC = false, bool OIHW = false>
__global__ void __launch_bounds__(256) slab_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ dst,
                                                          int splits, int Cout, int taps, int Cp, int C) {
  slab_reduce_body<TPO, ACC, OIHW>(slabs, dst, splits, Cout, taps, Cp, C, (int)blockIdx.x, (int)gridDim.x);
}

// --------------------------------------------------------------------------
// weight / input re-layouts (bf16)
// --------------------------------------------------------------------------
// W [Cout][KS][KS][Cin] -> Wt [Cin][KS][KS][Cout] with the taps flipped (dgrad B operand)
__global__ void __launch_bounds__(256) weight_flip_transpose_kernel(const bf16_t* __restrict__ w,
                                                                    bf16_t* __restrict__ wt, int Cout, int Cin,
                                                                    int KS) {
  __shared__ bf16_t t[32][33];
  const int taps = KS * KS;
  const int tap = blockIdx.z;
  const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int co = co0 + r, ci = ci0 + tx;
    t[r][tx] = (co < Cout && ci < Cin) ? w[((int64_t)co * taps + tap) * Cin + ci] : (bf16_t)0;
  }
  __syncthreads();
  const int ftap = taps - 1 - tap;  // (KS-1-kh, KS-1-kw)
  for (int r = ty; r < 32; r += 8) {
    const int ci = ci0 + r, co = co0 + tx;
    if (ci < Cin && co < Cout) wt[((int64_t)ci * taps + ftap) * Cout + co] = t[tx][r];
  }
}

// fp32 [Cout][taps][C] -> bf16 [Cout][taps][Cp] (zero channels C..Cp-1)
// Many [rows][cols] bf16 matrices transposed in ONE launch (the ResNet-50 1x1
// weights for their dgrads, once per step: 33 weight_flip_transpose launches
// of ~5 us each before).  Entries sorted by tile0; 64x64 tiles.
struct TrEntry {
  int64_t src, dst;
  int rows, cols, tile0, tiles_c;
};

__global__ void __launch_bounds__(256) transpose_many_kernel(const TrEntry* __restrict__ tab, int n) {
  __shared__ bf16_t t[64][65];
  const int b = blockIdx.x;
  int e = 0;
  for (int i = 1; i < n; ++i)
    if (tab[i].tile0 <= b) e = i;
  const TrEntry en = tab[e];
  const bf16_t* __restrict__ src = reinterpret_cast<const bf16_t*>(en.src);
  bf16_t* __restrict__ dst = reinterpret_cast<bf16_t*>(en.dst);
  const int local = b - en.tile0;
  const int r0 = (local / en.tiles_c) * 64, c0 = (local % en.tiles_c) * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4)
    t[r][tx] = (r0 + r < en.rows && c0 + tx < en.cols) ? src[(int64_t)(r0 + r) * en.cols + c0 + tx] : (bf16_t)0;
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int c = c0 + r, rr = r0 + tx;
    if (c < en.cols && rr < en.rows) dst[(int64_t)c * en.rows + rr] = t[tx][r];
  }
}

// Many conv weights [Cout][Cin][KK] -> channels-last [Cout][KK][Cin] in ONE
// launch (the ResNet-50 MIOpen convolutions read channels-last weights: torch
// converted each one on every call, 34 copy kernels per step).
// blockIdx.y = entry, grid-stride over that entry's elements in dst order.
struct ClEntry {
  int64_t src, dst;
  int cout, cin, kk, pad;
};

__global__ void __launch_bounds__(256) weights_to_cl_kernel(const ClEntry* __restrict__ tab) {
  const ClEntry en = tab[blockIdx.y];
  const bf16_t* __restrict__ src = reinterpret_cast<const bf16_t*>(en.src);
  bf16_t* __restrict__ dst = reinterpret_cast<bf16_t*>(en.dst);
  const int64_t total = (int64_t)en.cout * en.kk * en.cin;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
    const int ci = (int)(j % en.cin);
    const int64_t r = j / en.cin;  // co * kk + t
    const int t = (int)(r % en.kk);
    const int64_t co = r / en.kk;
    dst[j] = src[(co * en.cin + ci) * en.kk + t];
  }
}

__global__ void __launch_bounds__(256) pack_weight_kernel(const float* __restrict__ w, bf16_t* __restrict__ wp,
                                                          int Cout, int taps, int C, int Cp) {
  const int64_t total = (int64_t)Cout * taps * Cp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cp);
    const int64_t rest = i / Cp;
    wp[i] = c < C ? f32_to_bf16(w[rest * C + c]) : (bf16_t)0;
  }
}

// bf16 [P][C] -> bf16 [P][Cp] (zero channels C..Cp-1); one thread per pixel
__global__ void __launch_bounds__(256) pad_channels_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ xp,
                                                           int64_t P, int C, int Cp) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (int64_t)gridDim.x * blockDim.x) {
    for (int c = 0; c < Cp; ++c) xp[p * Cp + c] = c < C ? x[p * C + c] : (bf16_t)0;
  }
}

// --------------------------------------------------------------------------
// Per-step operand preparation in ONE launch (was 5): zero-pad the input
// image channels, pack the first layer's fp32 weights to padded bf16, and
// flip+transpose the bf16 weights of every later layer for its dgrad.
// Job = blockIdx range; each transpose block moves one 32x32 (co, ci) tile of
// one tap through LDS.
// --------------------------------------------------------------------------
// (PrepArgs and the pad / zero jobs: prep_dev.h, shared with the SGD launch
// that prepares the next step of an unrolled graph.)
__global__ void __launch_bounds__(256) prep_step_kernel(const PrepArgs a) {
  __shared__ bf16_t t[32][33];
  int blk = blockIdx.x;
  if (blk < a.nb_pad) {
    prep_pad_block(a, blk);
    return;
  }
  blk -= a.nb_pad;
  if (blk < a.nb_pack) {
    if (a.w1_cp < 0) {  // pair-packed (pack1_index): scatter the real elements, pads stay zero
      const int total = a.w1_cout * a.taps * a.w1_c;
      for (int e = blk * 256 + threadIdx.x; e < total; e += a.nb_pack * 256)
        a.w1p[pack1_index(e, a.w1_c, a.w1_cp)] = f32_to_bf16(a.w1[e]);
      return;
    }
    const int total = a.w1_cout * a.taps * a.w1_cp;
    for (int i = blk * 256 + threadIdx.x; i < total; i += a.nb_pack * 256) {
      const int c = i % a.w1_cp;
      a.w1p[i] = c < a.w1_c ? f32_to_bf16(a.w1[(i / a.w1_cp) * a.w1_c + c]) : (bf16_t)0;
    }
    return;
  }
  blk -= a.nb_pack;
  if (blk < a.nb_zero) {
    prep_zero_block(a, blk);
    return;
  }
  blk -= a.nb_zero;
  for (int j = 0; j < a.nt; ++j) {
    if (blk >= a.nb_t[j]) { blk -= a.nb_t[j]; continue; }
    const int Cin = a.tcin[j], Cout = a.tcout[j], taps = a.taps;
    if (Cin % 64 == 0 && Cout % 64 == 0) {
      // (wtrans_dev.h.  Tiles of 4 consecutive taps per block with every load
      // issued first measured slower: 0.3314-0.3332 vs 0.3296-0.3307 ms/step,
      // 4x fewer blocks and 4x the static LDS of the whole prep launch,
      // profiles/r3_prep_taps_ab.txt.)
      __shared__ __attribute__((aligned(16))) bf16_t tt[64][72];
      wtrans_tile(a.tw[j], a.twt[j], Cin, Cout, taps, blk, tt);
      return;
    }
    const int nci = (Cin + 31) / 32, nco = (Cout + 31) / 32;
    const int tap = blk / (nci * nco);
    const int r = blk % (nci * nco);
    const int ci0 = (r % nci) * 32, co0 = (r / nci) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int q = ty; q < 32; q += 8) {
      const int co = co0 + q, ci = ci0 + tx;
      t[q][tx] = (co < Cout && ci < Cin) ? a.tw[j][((int64_t)co * taps + tap) * Cin + ci] : (bf16_t)0;
    }
    __syncthreads();
    const int ftap = taps - 1 - tap;
    for (int q = ty; q < 32; q += 8) {
      const int ci = ci0 + q, co = co0 + tx;
      if (ci < Cin && co < Cout) a.twt[j][((int64_t)ci * taps + ftap) * Cout + co] = t[tx][q];
    }
    return;
  }
}

}  // namespace dl
