// Evaluation head: the last conv block's eval-mode BN/ReLU/pool + Linear +
// LogSoftMax, ending in per-sample metrics instead of a backward (gfx950).
//
// Reference: the test loop of examples/cifar10.lua:213-234 (predict, then
// confusionMatrix:add per sample).  One workgroup of 256 threads per sample of
// a DeviceEvalLoader batch; built for the reference net (a 2048-feature pooled
// map, 10 classes).
//
// Forward: the POOL path of head_fwd_bwd_kernel (head.hip) -- the 2x2 window
// of the pre-BN output y under the eval coefficients (coef rows 2 = scale,
// 3 = shift), ReLU, max, rounded to bf16 where bn_relu_pool_fwd stores, the
// Linear with the same per-thread sum (its rounding steps spelled out, see
// below) and the same 16x16 LDS reduction, bias, log-softmax -- so the
// log-probabilities are bitwise those of CifarHIPExecutor.predict for the
// same sample.
//
// Metrics: row b of step s = ctr[0] is position pos = (s*B + b) mod n_order of
// the loader's order (the gather's formula, prep_dev.h); it counts iff
// pos < n_valid (the order's padding repeats the last sample).  A valid row
// writes pred[pos] (argmax of the fp32 log-probabilities, ties to the smaller
// class as in confusion_kernel), nll[pos] = lse - logit[label] and adds one to
// mat[label][pred]; an invalid row writes nothing.
//
// Counter: the launch advances ctr[0] by one through an arrival ticket on
// ctr[1] (the loader's reserved slot, zero between launches).  ONE thread of a
// block (the last, in the wave the logit reduction leaves idle) reads ctr[0];
// once that read is consumed (its pos is in LDS) it draws a ticket with an
// agent-scope acquire-release fetch_add.  The release orders its read of
// ctr[0] before its ticket, the acquire of the block that draws B-1 orders
// every block's read before that block's two plain stores: ctr[1] = 0,
// ctr[0] = s + 1.  No block of the launch can observe the advanced value, and
// nothing ever waits on the ticket.
#include "dl_common.h"
#include <stdexcept>
#include "dl_ops.h"

namespace dl {

template <int NC>
__global__ void __launch_bounds__(256) eval_head_kernel(const bf16_t* __restrict__ y, const float* __restrict__ coef,
                                                        int yH, int yW, int yC, const float* __restrict__ w,
                                                        const float* __restrict__ bias,
                                                        const int64_t* __restrict__ labels, int B,
                                                        unsigned long long* ctr, int n_order, int n_valid,
                                                        int* __restrict__ pred, float* __restrict__ nll,
                                                        unsigned long long* __restrict__ mat,
                                                        float* __restrict__ logits_out) {
  constexpr int F = 256 * 8;
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ float lgp[NC][257];  // per-thread logit partials, transposed (+1: conflict-free rows)
  __shared__ float redc[NC];
  __shared__ int spos;
  // every load of the block is issued before the first dependent use: the step
  // counter (its one reader), the label and the bias (thread 0's serial tail),
  // the classifier weights, the window and the coefficient rows
  unsigned long long step = 0ull;
  if (tid == 255) step = __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int ylab = (int)labels[b];
  float bv[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) bv[c] = bias[c];
  float acc[NC];
  const int j0 = tid * 8;
  float4 wc[NC][2];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    wc[c][0] = *reinterpret_cast<const float4*>(w + (int64_t)c * F + j0);
    wc[c][1] = *reinterpret_cast<const float4*>(w + (int64_t)c * F + j0 + 4);
  }
  uint4 v[4];
  uint4 hv;
  {
    // feature j0 = (oh * Wo + ow) * yC + c0 of the pooled NHWC map
    const int Wo = yW >> 1;
    const int pix = j0 / yC, c0 = j0 - pix * yC;
    const int oh = pix / Wo, ow = pix - oh * Wo;
    const bf16_t* base = y + (((int64_t)b * yH + 2 * oh) * yW + 2 * ow) * yC + c0;
    v[0] = *reinterpret_cast<const uint4*>(base);
    v[1] = *reinterpret_cast<const uint4*>(base + yC);
    v[2] = *reinterpret_cast<const uint4*>(base + (int64_t)yW * yC);
    v[3] = *reinterpret_cast<const uint4*>(base + (int64_t)yW * yC + yC);
    float sc[8], sh[8];
    const float4 sc0 = *reinterpret_cast<const float4*>(coef + 2 * yC + c0);
    const float4 sc1 = *reinterpret_cast<const float4*>(coef + 2 * yC + c0 + 4);
    const float4 sh0 = *reinterpret_cast<const float4*>(coef + 3 * yC + c0);
    const float4 sh1 = *reinterpret_cast<const float4*>(coef + 3 * yC + c0 + 4);
    sc[0] = sc0.x; sc[1] = sc0.y; sc[2] = sc0.z; sc[3] = sc0.w; sc[4] = sc1.x; sc[5] = sc1.y; sc[6] = sc1.z;
    sc[7] = sc1.w;
    sh[0] = sh0.x; sh[1] = sh0.y; sh[2] = sh0.z; sh[3] = sh0.w; sh[4] = sh1.x; sh[5] = sh1.y; sh[6] = sh1.z;
    sh[7] = sh1.w;
    float mx[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float f[8] = {lo_bf16(v[q].x), hi_bf16(v[q].x), lo_bf16(v[q].y), hi_bf16(v[q].y),
                          lo_bf16(v[q].z), hi_bf16(v[q].z), lo_bf16(v[q].w), hi_bf16(v[q].w)};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float z = fmaf(sc[k], f[k], sh[k]);
        mx[k] = q == 0 ? z : fmaxf(mx[k], z);
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) mx[k] = fmaxf(mx[k], 0.f);
    hv = make_uint4(pack_bf16x2(mx[0], mx[1]), pack_bf16x2(mx[2], mx[3]), pack_bf16x2(mx[4], mx[5]),
                    pack_bf16x2(mx[6], mx[7]));
  }
  const float hf[8] = {lo_bf16(hv.x), hi_bf16(hv.x), lo_bf16(hv.y), hi_bf16(hv.y),
                       lo_bf16(hv.z), hi_bf16(hv.z), lo_bf16(hv.w), hi_bf16(hv.w)};
  // predict's Linear (head_fwd_bwd_kernel<10>, labels == nullptr) is the plain sum
  //   hf[0]*w0 + hf[1]*w1 + ... + hf[7]*w7
  // under the compiler's floating-point contraction, and what contraction made
  // of it there differs per class (that kernel's classes are vectorised in
  // pairs with swapped lanes, the last pair differently).  Of the first two
  // products one is rounded on its own and the other fused onto it: term 0 is
  // the rounded one for classes 0, 2, 4, 6 and 9, term 1 for classes 1, 3, 5,
  // 7 and 8.  Terms 2..7 are each fused onto the running sum for classes 0..7,
  // and each rounded and then added for classes 8 and 9.  The same operations
  // are spelled out here with contraction off, so that this kernel's bits do
  // not depend on what contraction would make of the expression in this
  // context (tests/kernels/test_eval_graph_gpu.py compares the two kernels'
  // log-probabilities bitwise).
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float wk[8] = {wc[c][0].x, wc[c][0].y, wc[c][0].z, wc[c][0].w,
                           wc[c][1].x, wc[c][1].y, wc[c][1].z, wc[c][1].w};
      const bool term1_rounded = c < 8 ? (c & 1) != 0 : c == 8;
      float a = term1_rounded ? __builtin_fmaf(hf[0], wk[0], hf[1] * wk[1])
                              : __builtin_fmaf(hf[1], wk[1], hf[0] * wk[0]);
#pragma unroll
      for (int k = 2; k < 8; ++k) {
        if (c < 8) {
          a = __builtin_fmaf(hf[k], wk[k], a);
        } else {
          const float p = hf[k] * wk[k];
          a = a + p;
        }
      }
      acc[c] = a;
    }
  }
  // logits: sum of the 256 threads' partials per class through LDS (16 threads
  // per class, 16 values each, then a 16-lane butterfly)
#pragma unroll
  for (int c = 0; c < NC; ++c) lgp[c][tid] = acc[c];
  if (tid == 255)  // consumes the read of ctr[0]
    spos = (int)((step * (unsigned long long)B + (unsigned long long)b) % (unsigned)n_order);
  __syncthreads();
  if (tid < NC * 16) {
    const int c = tid >> 4, j = tid & 15;
    float sp = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) sp += lgp[c][q * 16 + j];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) sp += __shfl_xor(sp, o, 16);
    if (j == 0) redc[c] = sp;
  }
  if (tid == 255) {
    // the arrival ticket, beside the reduction: the last block to arrive
    // re-arms the ticket word and advances the counter (plain vector stores)
    const unsigned long long t = __hip_atomic_fetch_add(ctr + 1, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (t == (unsigned long long)(B - 1)) {
      ctr[1] = 0ull;
      ctr[0] = step + 1ull;
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int pos = spos;
    if (pos >= n_valid) return;  // a padded row: writes nothing, counts nothing
    float lg[NC], mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      lg[c] = redc[c] + bv[c];
      mx = fmaxf(mx, lg[c]);
    }
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) se += __expf(lg[c] - mx);
    const float lse = mx + __logf(se);
    // argmax of the log-probabilities predict stores: larger wins, ties -> smaller class
    float best = -INFINITY, lb = 0.f;
    int arg = 0x7fffffff;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float lp = lg[c] - lse;
      if (logits_out) logits_out[(int64_t)b * NC + c] = lp;
      if (lp > best) { best = lp; arg = c; }
      if (c == ylab) lb = lse - lg[c];
    }
    pred[pos] = arg;
    nll[pos] = lb;
    if (ylab >= 0 && ylab < NC && arg < NC) atomicAdd(&mat[ylab * NC + arg], 1ull);
  }
}

// labels: the loader's labels_out (written by the step's gather); ctr: its int64 [2]
// (step, ticket); pred / nll: [n_order]; mat: int64 [NC][NC]; logits_out: 0 or [B][NC] (tests)
void eval_head(uintptr_t y, uintptr_t coef, int yH, int yW, int yC, uintptr_t w, uintptr_t bias, uintptr_t labels,
               int B, int NC, uintptr_t ctr, int n_order, int n_valid, uintptr_t pred, uintptr_t nll, uintptr_t mat,
               uintptr_t logits_out, uintptr_t stream) {
  if (NC != 10) throw std::runtime_error("eval_head: built for 10 classes");
  if (yH <= 0 || yW <= 0 || yC <= 0 || yH % 2 != 0 || yW % 2 != 0 || yC % 8 != 0 || (yH / 2) * (yW / 2) * yC != 2048)
    throw std::runtime_error("eval_head: needs a 2048-feature pooled map, C % 8 == 0");
  if (B <= 0 || n_order < B || n_valid < 0 || n_valid > n_order)
    throw std::runtime_error("eval_head: needs 0 < B <= n_order and 0 <= n_valid <= n_order");
  if (!y || !coef || !w || !bias || !labels || !ctr || !pred || !nll || !mat)
    throw std::runtime_error("eval_head: null pointer");
  eval_head_kernel<10><<<B, 256, 0, as_stream(stream)>>>(
      (const bf16_t*)y, (const float*)coef, yH, yW, yC, (const float*)w, (const float*)bias, (const int64_t*)labels, B,
      (unsigned long long*)ctr, n_order, n_valid, (int*)pred, (float*)nll, (unsigned long long*)mat,
      (float*)logits_out);
  DL_HIP_CHECK(hipGetLastError());
}

}  // namespace dl
