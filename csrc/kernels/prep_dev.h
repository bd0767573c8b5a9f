// Device side of the per-step operand preparation (the input batch into the
// zero-bordered, channel-padded layer-1 buffer + zeroing the step's atomic
// accumulators), shared by the stand-alone prep launch (conv_igemm.hip
// prep_step_kernel) and the SGD launch that prepares the NEXT step of an
// unrolled graph in extra workgroups (flat_ops.hip sgd_slabs_kernel).
#pragma once
#include <algorithm>
#include <stdexcept>
#include <vector>

#include "dl_common.h"

namespace dl {

struct PrepArgs {
  const bf16_t* x; bf16_t* xp; int P; int C, Cp;                // input pad (channels + spatial)
  int H, W, sp;                                                 // image dims, spatial zero pad
  // device-side data path (img != nullptr): gather + normalise the step's
  // batch straight from the HBM-resident uint8 dataset
  const uint8_t* img; const int* order; const int64_t* lab_all; int64_t* lab_out;
  const unsigned long long* ctr;  // [0] = step counter (advanced by head_wgrad)
  int n_order, B;
  float mean[3], inv_std[3];
  const float* w1; bf16_t* w1p; int w1_cout, taps, w1_c, w1_cp;  // layer-1 pack
  int nt;                                                        // transposes
  const bf16_t* tw[4]; bf16_t* twt[4]; int tcout[4], tcin[4];
  int nb_pad, nb_pack, nb_t[4];
  int quad;  // fast gather/pad path: one block per image, 4 pixels per thread
  // zero job: the step's atomic accumulators (BN statistics, BN parameter
  // gradients, split-K weight gradients) -- float4 granularity
  int nz, nb_zero;
  float* zp[8];
  int zn4[8];
  // augmentation of the gathered batch (aug != nullptr; prep_pad_block_aug):
  // aug = device {seed, base}, pad = crop shift range, n_samples = images in img
  const unsigned long long* aug;
  int pad, flip;
  int64_t n_samples;
};

// Crop / flip parameters of draw idx: z = splitmix64's output for the state
// seed + (idx + 1) * golden; flip = bit 0, dx / dy = bits 8..23 / 32..47 mod
// (2 pad + 1).  Python's augment_params (torch_distlearn_amd/data) is the
// same formula; all arithmetic wraps at 64 bits.
__device__ __forceinline__ void augment_draw(unsigned long long seed, unsigned long long idx, int pad, int flip_on,
                                             int& flip, int& dx, int& dy) {
  unsigned long long z = seed + (idx + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const unsigned span = 2u * (unsigned)pad + 1u;
  flip = flip_on ? (int)(z & 1ull) : 0;
  dx = (int)(((unsigned)(z >> 8) & 0xffffu) % span);
  dy = (int)(((unsigned)(z >> 32) & 0xffffu) % span);
}

// The augmented gather (a.img and a.aug set): output pixel (h, w) of batch row
// b is source pixel (h + dy - pad, (flip ? W-1-w : w) + dx - pad) of its stored
// image, normalised by the expression of prep_pad_block, or exactly zero in
// every channel when that position lies outside the image.  Reads stay inside
// [img, img + n_samples*H*W*C); writes stay inside the interior of xp.
__device__ __forceinline__ void prep_pad_block_aug(const PrepArgs& a, int blk) {
  const int HW = a.H * a.W, Hp = a.H + 2 * a.sp, Wp = a.W + 2 * a.sp;
  const unsigned long long step = *a.ctr;  // advanced by head_wgrad later in the step
  const unsigned long long seed = a.aug[0], draw0 = (a.aug[1] + step) * (unsigned long long)a.B;
  if (a.quad) {
    // block = one image (one draw, so flip / dx / dy are uniform), thread = 4
    // consecutive output pixels of one row = 4 consecutive source pixels
    // (reversed under flip): 12 bytes at any byte alignment
    const int b = blk;
    const int pos = (int)((step * (unsigned long long)a.B + (unsigned long long)b) % (unsigned)a.n_order);
    const int smp = a.order[pos];
    if (threadIdx.x == 0) a.lab_out[b] = a.lab_all[smp];
    int flip, dx, dy;
    augment_draw(seed, draw0 + (unsigned long long)b, a.pad, a.flip, flip, dx, dy);
    const int64_t last = a.n_samples * HW * 3 - 4;  // byte offset of the dataset's last dword (H*W*3 % 4 == 0)
    for (int q4 = threadIdx.x; q4 < HW / 4; q4 += 256) {
      const int r = q4 * 4, h = r / a.W, w = r - h * a.W;
      const int hs = h + dy - a.pad;
      const int c0 = (flip ? a.W - 4 - w : w) + dx - a.pad;  // source column of the thread's first source pixel
      uint32_t o[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};      // 4 output pixels x 2 words (3 bf16 + a zero)
      if (hs >= 0 && hs < a.H && c0 > -4 && c0 < a.W) {
        // the aligned dwords covering the 12 bytes, each clamped into the
        // dataset: a clamped dword only ever feeds pixels that are out of range
        const int64_t byte0 = ((int64_t)smp * HW + (int64_t)hs * a.W + c0) * 3;
        const int64_t al = byte0 & ~(int64_t)3;
        const int sh = 8 * (int)(byte0 & 3);
        uint32_t d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int64_t off = al + 4 * k;
          d[k] = *reinterpret_cast<const uint32_t*>(a.img + (off < 0 ? 0 : (off > last ? last : off)));
        }
        uint32_t e[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
          e[k] = (uint32_t)(((((unsigned long long)d[k + 1]) << 32) | (unsigned long long)d[k]) >> sh);
        float f[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
          const float u = (float)((e[k >> 2] >> (8 * (k & 3))) & 0xffu);
          f[k] = (u * (1.0f / 255.0f) - a.mean[k % 3]) * a.inv_std[k % 3];
        }
#pragma unroll
        for (int px = 0; px < 4; ++px) {  // output pixel px = source pixel j (static indices: no scratch)
          const int j = 3 - px;
          const float f0 = flip ? f[3 * j] : f[3 * px], f1 = flip ? f[3 * j + 1] : f[3 * px + 1];
          const float f2 = flip ? f[3 * j + 2] : f[3 * px + 2];
          const int col = c0 + (flip ? j : px);
          const bool in = col >= 0 && col < a.W;
          o[2 * px] = in ? pack_bf16x2(f0, f1) : 0u;
          o[2 * px + 1] = in ? pack_bf16x2(f2, 0.f) : 0u;
        }
      }
      if (a.Cp == 4) {
        uint2* dst = reinterpret_cast<uint2*>(a.xp + (((int64_t)b * Hp + h + a.sp) * Wp + w + a.sp) * 4);
#pragma unroll
        for (int px = 0; px < 4; ++px) dst[px] = make_uint2(o[2 * px], o[2 * px + 1]);
      } else {
        uint4* dst = reinterpret_cast<uint4*>(a.xp + (((int64_t)b * Hp + h + a.sp) * Wp + w + a.sp) * 8);
#pragma unroll
        for (int px = 0; px < 4; ++px) dst[px] = make_uint4(o[2 * px], o[2 * px + 1], 0u, 0u);
      }
    }
    return;
  }
  for (int p = blk * 256 + threadIdx.x; p < a.P; p += a.nb_pad * 256) {
    const int b = p / HW;
    const int r = p - b * HW, h = r / a.W, w = r - h * a.W;
    const int pos = (int)((step * (unsigned long long)a.B + (unsigned long long)b) % (unsigned)a.n_order);
    const int smp = a.order[pos];
    int flip, dx, dy;
    augment_draw(seed, draw0 + (unsigned long long)b, a.pad, a.flip, flip, dx, dy);
    const int hs = h + dy - a.pad, ws = (flip ? a.W - 1 - w : w) + dx - a.pad;
    float f0 = 0.f, f1 = 0.f, f2 = 0.f;  // named, not an indexed array: registers, no scratch
    if (hs >= 0 && hs < a.H && ws >= 0 && ws < a.W && smp >= 0 && smp < a.n_samples) {
      const uint8_t* src = a.img + ((int64_t)smp * HW + hs * a.W + ws) * a.C;
      f0 = (src[0] * (1.0f / 255.0f) - a.mean[0]) * a.inv_std[0];
      if (a.C > 1) f1 = (src[1] * (1.0f / 255.0f) - a.mean[1]) * a.inv_std[1];
      if (a.C > 2) f2 = (src[2] * (1.0f / 255.0f) - a.mean[2]) * a.inv_std[2];
    }
    if (r == 0) a.lab_out[b] = a.lab_all[smp];
    const uint32_t w0 = pack_bf16x2(f0, f1), w1 = pack_bf16x2(f2, 0.f);  // +0.0f packs to the bits 0
    const int64_t q = ((int64_t)b * Hp + h + a.sp) * Wp + w + a.sp;  // interior of the zero-bordered buffer
    if (a.Cp == 4) {
      *reinterpret_cast<uint2*>(a.xp + q * 4) = make_uint2(w0, w1);
    } else {  // Cp 8 or 16 (prep_set_pad)
      *reinterpret_cast<uint4*>(a.xp + q * a.Cp) = make_uint4(w0, w1, 0u, 0u);
      if (a.Cp > 8) *reinterpret_cast<uint4*>(a.xp + q * a.Cp + 8) = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

// Workgroup blk (< nb_pad) of the pad/gather job.
__device__ __forceinline__ void prep_pad_block(const PrepArgs& a, int blk) {
  if (a.aug) {  // kernel argument: uniform over the launch
    prep_pad_block_aug(a, blk);
    return;
  }
  if (a.quad) {
    // fast path (3 -> 8 channels, W % 4 == 0): block = one image, thread =
    // 4 consecutive pixels of one row; every load of a thread is issued
    // before the first use (one dependent round trip for the sample index,
    // one for the pixels) and the 4 padded pixels go out as 64 contiguous B
    const int HW = a.H * a.W, Hp = a.H + 2 * a.sp, Wp = a.W + 2 * a.sp;
    const int b = blk;
    int smp = 0;
    if (a.img) {
      const unsigned long long step = *a.ctr;  // advanced by head_wgrad later in the step
      const int pos = (int)((step * (unsigned long long)a.B + (unsigned long long)b) % (unsigned)a.n_order);
      smp = a.order[pos];
      if (threadIdx.x == 0) a.lab_out[b] = a.lab_all[smp];
    }
    for (int q4 = threadIdx.x; q4 < HW / 4; q4 += 256) {
      const int r = q4 * 4, h = r / a.W, w = r - h * a.W;
      float f[12];
      if (a.img) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.img + ((int64_t)smp * HW + r) * 3);
        const uint32_t d0 = src[0], d1 = src[1], d2 = src[2];
        const uint32_t d[3] = {d0, d1, d2};
#pragma unroll
        for (int k = 0; k < 12; ++k) {
          const float u = (float)((d[k >> 2] >> (8 * (k & 3))) & 0xffu);
          f[k] = (u * (1.0f / 255.0f) - a.mean[k % 3]) * a.inv_std[k % 3];
        }
      } else {
        const uint2* src = reinterpret_cast<const uint2*>(a.x + ((int64_t)b * HW + r) * 3);
        const uint2 e0 = src[0], e1 = src[1], e2 = src[2];
        const uint32_t d[6] = {e0.x, e0.y, e1.x, e1.y, e2.x, e2.y};
#pragma unroll
        for (int k = 0; k < 12; ++k) f[k] = (k & 1) ? hi_bf16(d[k >> 1]) : lo_bf16(d[k >> 1]);
      }
      if (a.Cp == 4) {  // 8-byte pixels (the pair-packed first layer: csrc conv_fwd_c8_kernel PAIR)
        uint2* dst = reinterpret_cast<uint2*>(a.xp + (((int64_t)b * Hp + h + a.sp) * Wp + w + a.sp) * 4);
#pragma unroll
        for (int px = 0; px < 4; ++px)
          dst[px] = make_uint2(pack_bf16x2(f[3 * px], f[3 * px + 1]), pack_bf16x2(f[3 * px + 2], 0.f));
      } else {
        uint4* dst = reinterpret_cast<uint4*>(a.xp + (((int64_t)b * Hp + h + a.sp) * Wp + w + a.sp) * 8);
#pragma unroll
        for (int px = 0; px < 4; ++px)
          dst[px] = make_uint4(pack_bf16x2(f[3 * px], f[3 * px + 1]), pack_bf16x2(f[3 * px + 2], 0.f), 0u, 0u);
      }
    }
    return;
  }
  const int HW = a.H * a.W, Hp = a.H + 2 * a.sp, Wp = a.W + 2 * a.sp;
  // step counter: advanced by head_wgrad later in the same step (stream order)
  const unsigned long long step = a.img ? *a.ctr : 0ull;
  for (int p = blk * 256 + threadIdx.x; p < a.P; p += a.nb_pad * 256) {
    const int b = p / HW;
    const int r = p - b * HW, h = r / a.W, w = r - h * a.W;
    bf16_t v[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) v[c] = 0;
    if (a.img) {
      // sample of this step = order[(step * B + b) mod n_order]
      const int pos = (int)((step * (unsigned long long)a.B + (unsigned long long)b) % (unsigned)a.n_order);
      const int smp = a.order[pos];
      const uint8_t* src = a.img + ((int64_t)smp * HW + r) * a.C;
      for (int c = 0; c < a.C && c < 3; ++c) v[c] = f32_to_bf16((src[c] * (1.0f / 255.0f) - a.mean[c]) * a.inv_std[c]);
      if (r == 0) a.lab_out[b] = a.lab_all[smp];
    } else {
      for (int c = 0; c < a.C; ++c) v[c] = a.x[(int64_t)p * a.C + c];
    }
    const int64_t q = ((int64_t)b * Hp + h + a.sp) * Wp + w + a.sp;  // interior of the zero-bordered buffer
    if (a.Cp == 4) {
      *reinterpret_cast<uint2*>(a.xp + q * 4) = *reinterpret_cast<const uint2*>(v);
    } else {
      for (int c = 0; c < a.Cp; c += 8)
        *reinterpret_cast<uint4*>(a.xp + q * a.Cp + c) = *reinterpret_cast<const uint4*>(v + c);
    }
  }
}

// Workgroup blk (< nb_zero) of the zero job.
__device__ __forceinline__ void prep_zero_block(const PrepArgs& a, int blk) {
  int64_t total = 0;
  for (int j = 0; j < a.nz; ++j) total += a.zn4[j];
  for (int64_t i = (int64_t)blk * 256 + threadIdx.x; i < total; i += (int64_t)a.nb_zero * 256) {
    int64_t r = i;
    int j = 0;
    while (r >= a.zn4[j]) { r -= a.zn4[j]; ++j; }
    reinterpret_cast<float4*>(a.zp[j])[r] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// Host: the zero job's ranges (16-byte aligned, multiples of 4 floats).
inline void prep_set_zero(PrepArgs& a, const std::vector<uintptr_t>& zp, const std::vector<int64_t>& zn) {
  if (zp.size() != zn.size() || zp.size() > 8) throw std::runtime_error("prep_step: up to 8 zero ranges");
  a.nz = (int)zp.size();
  int64_t z4 = 0;
  for (int j = 0; j < a.nz; ++j) {
    if (zn[j] % 4 != 0 || zp[j] % 16 != 0 || zn[j] <= 0 || zn[j] / 4 >= (1ll << 31))
      throw std::runtime_error("prep_step: zero ranges must be 16-byte aligned multiples of 4 floats");
    a.zp[j] = (float*)zp[j];
    a.zn4[j] = (int)(zn[j] / 4);
    z4 += zn[j] / 4;
  }
  a.nb_zero = (int)std::min<int64_t>((z4 + 1023) / 1024, 256);
}

// Host: the pad/gather job over P = B*H*W pixels (sets P, quad, nb_pad).
inline void prep_set_pad(PrepArgs& a, int64_t P) {
  if (a.C > 16 || a.Cp > 16 || (a.Cp % 8 != 0 && a.Cp != 4) || a.C > a.Cp)
    throw std::runtime_error("prep_step: input channels must pad to 4, 8 or 16");
  if (P >= (1ll << 31)) throw std::runtime_error("prep_step: too many pixels");
  if (P > 0 && (a.H <= 0 || a.W <= 0 || P % ((int64_t)a.H * a.W) != 0)) throw std::runtime_error("prep_step: P != B*H*W");
  a.P = (int)P;
  a.quad = (a.C == 3 && (a.Cp == 8 || a.Cp == 4) && P > 0 && a.W % 4 == 0) ? 1 : 0;
  a.nb_pad = a.quad ? (int)(P / ((int64_t)a.H * a.W)) : (int)std::min<int64_t>((P + 255) / 256, 1024);
}

// Host: the device-gather fields (batch b of step ctr[0] = sample
// order[(ctr[0]*B + b) mod n_order], normalised (v/255 - mean)/std).
inline void prep_set_gather(PrepArgs& a, uintptr_t img, uintptr_t order, uintptr_t lab_all, uintptr_t lab_out,
                            uintptr_t ctr, int n_order, int B, int C, const std::vector<float>& mean,
                            const std::vector<float>& stdv) {
  if (C > 3 || mean.size() < (size_t)C || stdv.size() < (size_t)C) throw std::runtime_error("prep_step_gather: C <= 3");
  if (n_order <= 0 || B <= 0) throw std::runtime_error("prep_step_gather: empty order / batch");
  if (!img || !order || !lab_all || !lab_out || !ctr) throw std::runtime_error("prep_step_gather: null pointer");
  a.img = (const uint8_t*)img; a.order = (const int*)order; a.lab_all = (const int64_t*)lab_all;
  a.lab_out = (int64_t*)lab_out; a.ctr = (const unsigned long long*)ctr; a.n_order = n_order; a.B = B;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = c < C ? mean[c] : 0.f;
    a.inv_std[c] = c < C ? 1.0f / stdv[c] : 1.f;
  }
}

// Host: the augmentation of a gather (after prep_set_gather, with a.H / a.W
// set).  params = device int64 {seed, base}; the value's own checks ran in
// augment() (conv_igemm.hip), those against the image run here.
inline void prep_set_augment(PrepArgs& a, uintptr_t params, int pad, int flip, int64_t n_samples) {
  if (!a.img) throw std::runtime_error("augment: only the device-side gather can be augmented");
  if (!params || params % 8 || pad < 0 || pad > 8 || (flip != 0 && flip != 1) || n_samples <= 0)
    throw std::runtime_error("augment: bad value");
  if (pad >= std::min(a.H, a.W)) throw std::runtime_error("augment: pad must be smaller than the image");
  if ((uintptr_t)a.img % 4) throw std::runtime_error("augment: the dataset must be 4-byte aligned");
  a.aug = (const unsigned long long*)params; a.pad = pad; a.flip = flip; a.n_samples = n_samples;
}

}  // namespace dl
