"""CPU references for the ResNet-50 path's non-conv kernels: the channels-last
BatchNorm (csrc/kernels/bn_nhwc.hip, bn_coef_dev.h), the channels-last max pool
(pool_nhwc.hip) and the glue kernels (resnet_glue.hip), in the style of
tests/kernels/exact_bn_head.py and exact_update.py.

Two regimes:

* exact: small-integer bf16 activations / gradients and dyadic per-channel
  parameters.  Every intermediate is an fp32 number and every sum is exact in
  any order, so atomics, block counts and fma contraction cannot matter; the
  references prove the regime per shape (``check_f32`` / ``check_sum_exact``).
* real: random bf16 values.  Wherever the kernel's rounding sequence is fixed
  by explicit ``fmaf`` or single operations the reference emulates it in fp32
  (``fma32`` / ``mul32`` / ``add32``, one rounding each) and the comparison is
  bitwise; elsewhere a per-element bound is derived from the operation count.

numpy / torch on the CPU only; fp32 arrays hold the bf16 values.  The
references model arithmetic and the documented layouts, never the kernels'
loops.  No constant comes from a run of the code under test.
"""
from __future__ import annotations

import numpy as np
import torch

from tests.kernels import exact
from tests.kernels import exact_bn_head as xb
from tests.kernels.exact_bn_head import U32, check_f32, check_sum_exact, cpu64
from tests.kernels.exact_update import add32, bf16_bits, bf16_round64, bf16_widen, fma32, mul32

F32, F64 = np.float32, np.float64


def np32(t):
    """torch tensor (any float dtype / device) or array -> fp32 numpy array."""
    if isinstance(t, torch.Tensor):
        return t.detach().to("cpu", torch.float32).numpy()
    return np.asarray(t, dtype=F32)


def to_bf16(a32):
    """fp32 values -> their bf16 round-to-nearest-even, held in fp32."""
    a32 = np.ascontiguousarray(np.asarray(a32, dtype=F32))
    return bf16_widen(bf16_bits(a32)).reshape(a32.shape)


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=F64))


def same_values(got, want, what: str):
    """Bitwise comparison of two sets of fp32 / bf16 VALUES (-0 == +0; NaN fails)."""
    g, w = np32(got).reshape(-1), np32(want).reshape(-1)
    assert g.shape == w.shape, f"{what}: {g.shape} vs {w.shape}"
    bad = ~(g == w)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ; first at flat index {i}: "
                             f"got {float(g[i])!r} want {float(w[i])!r}")


# ---------------------------------------------------------------------------
# bn_nhwc.hip: geometry (make_geom's formulas) and which loops a shape reaches
# ---------------------------------------------------------------------------
def bn_geom(M: int, C: int, max_rb: int = 2048, nt: int = 256):
    """make_geom: CVB channel vectors per block, RPI rows per iteration, rows
    per block, row blocks, channel groups."""
    cvb = min(C // 8, 32)
    rpi = nt // cvb
    groups = (C // 8) // cvb
    cap = min(max(262144 // C, 64), max_rb)
    rb = max(1, min((M + rpi * 16 - 1) // (rpi * 16), cap))
    rpb = (M + rb - 1) // rb
    rpb = (rpb + rpi - 1) // rpi * rpi
    rb = (M + rpb - 1) // rpb
    return {"CVB": cvb, "RPI": rpi, "rpb": rpb, "rb": rb, "groups": groups}


def bn_loops(M: int, C: int, max_rb: int = 2048, nt: int = 256, U: int = 4):
    """The loop features a kernel with U rows per iteration meets at (M, C):
    row lane r of a block with n rows owns k = ceil((n - r) / RPI) rows, runs
    k // U unrolled iterations and k % U single-row ones.
      rem_only   a block none of whose lanes reaches the unrolled loop
      u+1..u+3   a lane with unrolled iterations and that many remainder rows
      idle       a block whose last iteration leaves some row lanes without a row
      small      M < RPI
      blocks     two or more row blocks;  groups: two or more channel groups"""
    g = bn_geom(M, C, max_rb, nt)
    f = set()
    for blk in range(g["rb"]):
        n = min(M, (blk + 1) * g["rpb"]) - blk * g["rpb"]
        ks = {-(-(n - r) // g["RPI"]) for r in (0, min(n, g["RPI"]) - 1, (n - 1) % g["RPI"], (n % g["RPI"]))
              if 0 <= r < n}
        if max(ks) < U:
            f.add("rem_only")
        for k in ks:
            if k >= U and k % U:
                f.add(f"u+{k % U}")
        if n % g["RPI"]:
            f.add("idle")
    if M < g["RPI"]:
        f.add("small")
    if g["rb"] >= 2:
        f.add("blocks")
    if g["groups"] >= 2:
        f.add("groups")
    return f


def out_row_corrections(H: int, W: int, M: int):
    """Whether out_row's float-reciprocal divisions need their correction step
    for some row m < M of H x W images: n = int(fp32(m) * fl(1 / HW)) comes out
    one too small (rem >= HW) -> first flag; the same for h = int(fp32(rem) *
    fl(1 / W)) -> second flag.  Plain fp32 arithmetic, no kernel involved:
    5 x 11 images need the first from m = 55 on (55 * fl(1/55) < 1), 3 x 41
    images both; none of 1x1, 3x5, 7x7, 13x9, 56x56 or 57x59 needs either."""
    HW = H * W
    m = np.arange(M, dtype=np.int64)
    n = (m.astype(F32) * (F32(1) / F32(HW))).astype(np.int64)
    rem = m - n * HW
    fixed = np.where(rem >= HW, rem - HW, rem)
    h = (fixed.astype(F32) * (F32(1) / F32(W))).astype(np.int64)
    return bool((rem >= HW).any()), bool((fixed - h * W >= W).any())


# ---------------------------------------------------------------------------
# bn_nhwc.hip: forward
# ---------------------------------------------------------------------------
def bn_stats64(x):
    """fp64 (sum, sum of squares) [2][C] of x [M][C]."""
    x = cpu64(x)
    return torch.stack([x.sum(0), (x * x).sum(0)])


def bn_stats_exact(x):
    """``bn_stats64`` with the exact regime proved: both sums are exact in fp32 in any order."""
    x = cpu64(x)
    check_sum_exact("sum x", x, (0,))
    check_sum_exact("sum x^2", x * x, (0,))
    return bn_stats64(x)


def published_bounds(acc, M: int, w, b, eps: float, momentum: float, running):
    """``bn_coefficient_bounds`` of the fp32 totals acc [2C] for bn_coef8.

    bn_coef8 computes mean = acc * fl(1/M) and sumsq * fl(1/M): two roundings
    each (the reciprocal, the product) where the bounds charge one for a
    division.  The totals are therefore passed as R = 2 rows (the second all
    zero): R u S/M charges exactly one more ulp on the mean and on sumsq/M,
    and that extra propagates into var, invstd and the running statistics by
    the bounds' own formulas.  The remaining roundings are within the bounds'
    budget: fma(-m, m, q) rounds once (two charged), the running mean takes 3
    of its 4 (1 - m, its product, the fma), the running variance its 5
    (unbias, var * unbias, 1 - m, its product, the fma)."""
    a = cpu64(acc).reshape(2, -1)
    sums = torch.stack([a, torch.zeros_like(a)])
    return xb.bn_coefficient_bounds(sums, M, w, b, None, eps, momentum, running, 0)


def assert_published(save, run_after, acc, M: int, w, b, eps, momentum, run_before, what: str):
    """save [2C] (mean, invstd) and the running statistics after the call
    against ``published_bounds``; run_before None: the kernel got null pointers."""
    ref, bnd = published_bounds(acc, M, w, b, eps, momentum, run_before)
    C = ref["mean"].numel()
    s = cpu64(save)
    xb.assert_within(s[:C], ref["mean"], bnd["mean"], f"{what}: mean")
    xb.assert_within(s[C:], ref["invstd"], bnd["invstd"], f"{what}: invstd")
    if run_before is not None:
        xb.assert_within(run_after[0], ref["rmean"], bnd["rmean"], f"{what}: running mean")
        xb.assert_within(run_after[1], ref["rvar"], bnd["rvar"], f"{what}: running var")
    return ref, bnd


def coef_from_save(save, w, b):
    """(sc, sh) as every kernel derives them from the published save [2C]:
    sc = fp32(w * invstd), sh = fma(-mean, sc, b)."""
    s = np32(save)
    C = s.size // 2
    sc = mul32(np32(w), s[C:])
    return sc, fma32(-s[:C], sc, np32(b))


def bn_fwd_ref(x, sc, sh, relu: bool, res=None, rsc=None, rsh=None, round_res: bool = True):
    """y = bf16(relu?(fma(x, sc, sh) [+ res])), bitwise; with (rsc, rsh) the
    residual is bf16(fma(res, rsc, rsh)) (ResBn).  ``round_res`` False is the
    wrong rule (an unrounded residual BN) the oracle must tell apart."""
    f = fma32(np32(x), sc, sh)
    if res is not None:
        q = np32(res)
        if rsc is not None:
            q = fma32(q, rsc, rsh)
            if round_res:
                q = to_bf16(q)
        f = add32(f, q)
    if relu:
        f = np.maximum(f, F32(0))
    return to_bf16(f)


def mask_bits_ref(y):
    """relu mode 3's bits of y [M][C]: byte (m, j) bit k = (y[m][8j + k] != 0)."""
    nz = (np32(y) != 0).reshape(y.shape[0], -1, 8)
    return (nz * (1 << np.arange(8))).sum(2).astype(np.uint8)


def unpack_bits(bits, C: int):
    b = np.asarray(bits, dtype=np.uint8).reshape(-1, C // 8, 1)
    return ((b >> np.arange(8, dtype=np.uint8)) & 1).reshape(-1, C).astype(bool)


# ---------------------------------------------------------------------------
# bn_nhwc.hip: backward
# ---------------------------------------------------------------------------
def relu_mask(mode: int, x, sc, sh, y=None, bits=None, positive: str = "gt"):
    """The elements whose gradient passes: mode 0 all, 1 y > 0, 2 the
    recomputed pre-activation fma(x, sc, sh) > 0 (``positive`` "ge" is the
    wrong rule), 3 the mask bits."""
    x = np32(x)
    if mode == 0:
        return np.ones(x.shape, dtype=bool)
    if mode == 1:
        return np32(y) > 0
    if mode == 2:
        z = fma32(x, sc, sh)
        return z > 0 if positive == "gt" else z >= 0
    return unpack_bits(bits, x.shape[1])


def bn_bwd_sums(g, x, save, exact_regime: bool = False):
    """-> (sums [2][C] = (sum g, sum g xhat), abs sums [2][C]) in fp64, xhat =
    (x - mean) invstd from save [2C].  Exact regime: every term and its sum in
    any order are checked to be exact in fp32."""
    g, x, s = cpu64(g), cpu64(x), cpu64(save)
    C = x.shape[1]
    d = x - s[:C]
    xh = d * s[C:]
    t = g * xh
    if exact_regime:
        check_f32("x - mean", d)
        check_f32("xhat", xh)
        check_sum_exact("sum g", g, (0,))
        check_sum_exact("sum g xhat", t, (0,))
    return torch.stack([g.sum(0), t.sum(0)]), torch.stack([g.abs().sum(0), t.abs().sum(0)])


def bwd_sums_bound(M: int, s_abs):
    """|fp32 sum - fp64 sum| <= (M + 3) 2^-23 sum|term|: three roundings per
    term (the subtraction and the two products of g (x - mean) invstd, the last
    possibly fused) and at most M - 1 roundings of partial sums bounded by
    sum|term|, in any order and partition (``exact_bn_head.sums_bound``)."""
    return (M + 3) * U32 * cpu64(s_abs)


def bn_dx64(g, x, save, w, acc, M: int, exact_regime: bool = False):
    """dx = a (g - mg - xhat mgx), a = w invstd, mg = acc[0]/M, mgx = acc[1]/M
    in fp64 from the fp32 save / totals the kernel read -> (dx, E).

    E bounds the kernel's fp32 evaluation, one ulp (2^-23) per rounding:
      a:            w * invstd (1);
      mg, mgx:      fl(1/M) (1) and the product (1);
      xhat:         x - mean (1), times invstd (1);
      g - mg (1), xhat * mgx (1, or none when fused), the subtraction (1), the
      product with a (1).
    The g term passes through 4 roundings, mg through 6, xhat mgx through 8,
    and every rounding of a partial sum is relative to at most |g| + |mg| +
    |xhat mgx|: E = 9 2^-23 |a| (|g| + |mg| + |xhat| |mgx|) (8 and one for the
    second-order terms).  Exact regime: every intermediate of both the
    contracted and the plain form is checked to be an fp32 number."""
    g, x, s, w, acc = cpu64(g), cpu64(x), cpu64(save), cpu64(w), cpu64(acc).reshape(2, -1)
    C = x.shape[1]
    a = w * s[C:]
    mg, mgx = acc[0] / M, acc[1] / M
    xh = (x - s[:C]) * s[C:]
    inner = g - mg - xh * mgx
    dx = a * inner
    if exact_regime:
        for name, v in (("a", a), ("1/M", torch.tensor(1.0 / M)), ("mg", mg), ("mgx", mgx), ("xhat", xh),
                        ("g - mg", g - mg), ("xhat mgx", xh * mgx), ("inner", inner), ("dx", dx)):
            check_f32(name, v)
    E = 9 * U32 * a.abs() * (g.abs() + mg.abs() + xh.abs() * mgx.abs())
    return dx, E


def bf16_bound(ref, E):
    """half_ulp_bf16(|ref| + E) + E: one bf16 rounding of a value within E of ref."""
    return exact.half_ulp_bf16(ref.abs() + E) + E


def bn_train64(x, w, b, eps: float, dy, relu: bool, res=None):
    """The whole training BN (+ residual, + ReLU) and its backward as formulas
    in fp64 -> dict(y, dx, dw, db, dres): what tests/unit checks against
    autograd, built from ``bn_bwd_sums`` / ``bn_dx64``."""
    x, w, b, dy = cpu64(x), cpu64(w), cpu64(b), cpu64(dy)
    M = x.shape[0]
    mean = x.mean(0)
    var = (x * x).mean(0) - mean * mean
    invstd = (var + eps).rsqrt()
    z = (x - mean) * invstd * w + b
    if res is not None:
        z = z + cpu64(res)
    y = z.clamp_min(0) if relu else z
    g = dy * (y > 0) if relu else dy
    save = torch.cat([mean, invstd])
    sums, _ = bn_bwd_sums(g, x, save)
    dx, _ = bn_dx64(g, x, save, w, sums, M)
    return {"y": y, "dx": dx, "dw": sums[1], "db": sums[0], "dres": g if res is not None else None}


def int_bn_bwd_inputs(M: int, C: int, generator):
    """Integer backward operands: x in [-4, 4], dy in [-4, 4], res-BN input xr
    in [-3, 3] (bf16); save (mean an integer in [-2, 2], invstd = +-2^-j, j in
    0..2), w = +-2^j (j in -1..1) or 0 (channel 3), b dyadic: channels with
    c % 4 == 0 have b = 0 and w != 0, so x == mean gives a pre-activation of
    exactly 0, which relu mode 2 must mask (> 0); the rest multiples of 1/4."""
    x = exact.int_bf16((M, C), -4, 4, generator=generator)
    dy = exact.int_bf16((M, C), -4, 4, generator=generator)
    xr = exact.int_bf16((M, C), -3, 3, generator=generator)
    sgn = lambda: torch.where(torch.rand(C, generator=generator) < 0.3, -1.0, 1.0).double()  # noqa: E731
    mean = torch.randint(-2, 3, (C,), generator=generator).double()
    invstd = torch.pow(2.0, -torch.randint(0, 3, (C,), generator=generator).double()) * sgn()
    w = torch.pow(2.0, torch.randint(-1, 2, (C,), generator=generator).double()) * sgn()
    b = torch.randint(-8, 9, (C,), generator=generator).double() / 4.0
    b[::4] = 0.0
    if C > 3:
        w[3] = 0.0
    save = torch.cat([mean, invstd]).float()
    rmean = torch.randint(-2, 3, (C,), generator=generator).double()
    rinv = torch.pow(2.0, -torch.randint(0, 3, (C,), generator=generator).double()) * sgn()
    rw = torch.pow(2.0, torch.randint(-1, 2, (C,), generator=generator).double()) * sgn()
    return {"x": x, "dy": dy, "xr": xr, "save": save, "w": w.float(), "b": b.float(),
            "rsave": torch.cat([rmean, rinv]).float(), "rw": rw.float()}


# ---------------------------------------------------------------------------
# pool_nhwc.hip
# ---------------------------------------------------------------------------
def pool_out(H: int, K: int, S: int, P: int) -> int:
    return (H + 2 * P - K) // S + 1


def pool_fwd_ref(x, K: int, S: int, P: int, tie: str = "first"):
    """Max pool of x [N][H][W][C] (fp32 array of bf16 values) -> (y, arg):
    the first maximum in row-major window order (tie "last": the wrong rule),
    taps outside the image skipped; arg = u * K + v (uint8)."""
    x = np32(x)
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H, K, S, P), pool_out(W, K, S, P)
    xp = np.full((N, H + 2 * P, W + 2 * P, C), -np.inf, dtype=F32)
    xp[:, P:P + H, P:P + W] = x
    best = np.full((N, Ho, Wo, C), -np.inf, dtype=F32)
    arg = np.zeros((N, Ho, Wo, C), dtype=np.uint8)
    for u in range(K):
        for v in range(K):
            t = xp[:, u:u + S * (Ho - 1) + 1:S, v:v + S * (Wo - 1) + 1:S]
            m = (t > best) if tie == "first" else ((t >= best) & (t > -np.inf))
            best = np.where(m, t, best)
            arg = np.where(m, np.uint8(u * K + v), arg)
    return best, arg


def pool_arg_to_flat(arg, H: int, W: int, K: int, S: int, P: int):
    """arg bytes -> the flat input index h * W + w (F.max_pool2d's indices)."""
    N, Ho, Wo, C = arg.shape
    u, v = arg.astype(np.int64) // K, arg.astype(np.int64) % K
    oh = np.arange(Ho).reshape(1, Ho, 1, 1)
    ow = np.arange(Wo).reshape(1, 1, Wo, 1)
    return (oh * S - P + u) * W + (ow * S - P + v)


def pool_bwd_ref(dy, arg, H: int, W: int, K: int, S: int, P: int, drop_last_col: bool = False):
    """dx [N][H][W][C] in fp32 (before the bf16 rounding): every input pixel
    adds, sequentially in fp32 from 0, dy of the windows whose argmax it is, in
    the kernels' order: oh ascending, then ow ascending (for a fixed pixel that
    is u descending, then v descending)."""
    dy, arg = np32(dy), np.asarray(arg, dtype=np.uint8)
    N, Ho, Wo, C = dy.shape
    dxp = np.zeros((N, H + 2 * P, W + 2 * P, C), dtype=F32)
    for u in range(K - 1, -1, -1):
        for v in range(K - 1, -1, -1):
            sl = (slice(None), slice(u, u + S * (Ho - 1) + 1, S), slice(v, v + S * (Wo - 1) + 1, S))
            dxp[sl] = add32(dxp[sl], np.where(arg == u * K + v, dy, F32(0)))
    return dxp[:, P:P + H, P:P + W]


# ---------------------------------------------------------------------------
# resnet_glue.hip: layouts
# ---------------------------------------------------------------------------
def s2d_ref(x, Hs: int, Ws: int, pad: int = 3):
    """S[n][i][j][(a*2+b)*3 + c] = x[n][2i+a-pad][2j+b-pad][c], 0 outside the
    image; channels 12..15 zero.  x [N][H][W][3]."""
    x = np32(x)
    N, H, W, _ = x.shape
    xp = np.zeros((N, 2 * Hs + 2, 2 * Ws + 2, 3), dtype=F32)
    hh, ww = min(H, 2 * Hs + 2 - pad), min(W, 2 * Ws + 2 - pad)
    xp[:, pad:pad + hh, pad:pad + ww] = x[:, :hh, :ww]
    out = np.zeros((N, Hs, Ws, 16), dtype=F32)
    for a in range(2):
        for b in range(2):
            out[..., (a * 2 + b) * 3:(a * 2 + b) * 3 + 3] = xp[:, a:a + 2 * Hs:2, b:b + 2 * Ws:2]
    return out


def stem_pack_ref(w7):
    """W4[o][th][tw][(a*2+b)*3+c] = W7[o][c][2th+a][2tw+b], 0 where kh or kw = 7
    and in channels 12..15.  w7 [Cout][3][7][7]."""
    w7 = np32(w7)
    w8 = np.zeros((w7.shape[0], 3, 8, 8), dtype=F32)
    w8[:, :, :7, :7] = w7
    out = np.zeros((w7.shape[0], 4, 4, 16), dtype=F32)
    for a in range(2):
        for b in range(2):
            out[..., (a * 2 + b) * 3:(a * 2 + b) * 3 + 3] = w8[:, :, a::2, b::2].transpose(0, 2, 3, 1)
    return out


def stem_unpack_index(swap_parity: bool = False):
    """k[c][kh][kw]: the slot of the 256-wide slab row that holds tap (c, kh,
    kw): ((kh/2)*4 + kw/2)*16 + ((kh%2)*2 + kw%2)*3 + c.  ``swap_parity``: the
    wrong rule with the two parity bits exchanged."""
    c, kh, kw = np.meshgrid(np.arange(3), np.arange(7), np.arange(7), indexing="ij")
    a, b = (kw % 2, kh % 2) if swap_parity else (kh % 2, kw % 2)
    return ((kh // 2) * 4 + kw // 2) * 16 + (a * 2 + b) * 3 + c


def stem_unpack_ref(slab, dw7, swap_parity: bool = False):
    """dw7[o][c][kh][kw] + (sequential fp32 sum from 0 over the splits, in
    split order, of slab[s][o][k]), one more fp32 addition."""
    slab = np32(slab)
    k = stem_unpack_index(swap_parity)
    s = np.zeros(slab.shape[1:2] + k.shape, dtype=F32)
    for q in range(slab.shape[0]):
        s = add32(s, slab[q][:, k])
    return add32(np32(dw7), s)


PHASE_TAPS = ((1, 1), (1, 2), (2, 1), (2, 2))  # (KHp, KWp) of phase p = rh * 2 + rw


def phase_ref(wt):
    """The four phase blocks of wt [Cin][3][3][Cout], concatenated at their
    arena offsets (Cin * Cout * 0, 1, 3, 5): phase (rh, rw) holds
    [Cin][KHp][KWp][Cout] with row taps {1} for parity 0 and {0, 2} for parity 1."""
    wt = np32(wt)
    taps = ([1], [0, 2])
    return np.concatenate([wt[:, taps[p >> 1]][:, :, taps[p & 1]].reshape(-1) for p in range(4)])


def head_pool_ref(h):
    """f = bf16(fp32(s * fl(1/HW))), s the sequential fp32 sum over HW.  h [B][HW][C]."""
    h = np32(h)
    s = np.zeros((h.shape[0], h.shape[2]), dtype=F32)
    for q in range(h.shape[1]):
        s = add32(s, h[:, q])
    return to_bf16(mul32(s, F32(F64(1.0) / F64(h.shape[1]))))


def head_logits_ref(slab, bias, NC: int):
    """logits [B][NC] = the sequential fp32 sum bias + slab_0 + slab_1 + ...; slab [splits][B][NCp]."""
    slab = np32(slab)
    s = np.broadcast_to(np32(bias)[:NC], slab.shape[1:2] + (NC,)).astype(F32)
    for q in range(slab.shape[0]):
        s = add32(s, slab[q][:, :NC])
    return s


def softmax_nll64(logits, labels):
    """fp64 log-softmax, softmax - onehot, per-sample loss and the spread of each row."""
    lg = cpu64(torch.as_tensor(np.asarray(logits, dtype=F64)))
    mx = lg.max(1, keepdim=True).values
    logp = lg - mx - (lg - mx).exp().sum(1, keepdim=True).log()
    out = {"logp": logp, "spread": (lg - mx).abs().max(1).values}
    if labels is not None:
        onehot = torch.nn.functional.one_hot(labels.cpu().long(), lg.shape[1]).double()
        out["g"] = logp.exp() - onehot
        out["loss_b"] = -(logp * onehot).sum(1)
    return out


def saturated_slabs(B: int, NC: int, NCp: int, splits: int, generator):
    """Integer logits slabs on which the fast exp / log are exact: slab
    entries integers in [-3, 3], bias integers in [-3, 3]; slab 0 of the
    intended class k_b gets +512, so logit k_b leads by more than 104 (asserted
    by the caller): every other exponential is 0 in fp32, the sum is exactly 1
    and its log exactly 0.  Padded columns hold NaN (never read).  Labels: odd
    samples get another class (NC > 1).  -> slab, bias, labels, lead."""
    slab = torch.randint(-3, 4, (splits, B, NCp), generator=generator).float()
    bias = torch.randint(-3, 4, (NC,), generator=generator).float()
    k = torch.randint(0, NC, (B,), generator=generator)
    k[0] = NC - 1
    slab[0, torch.arange(B), k] += 512.0
    slab[:, :, NC:] = float("nan")
    lab = k.clone()
    if NC > 1:
        odd = torch.arange(B) % 2 == 1
        lab[odd] = (k[odd] + 1 + torch.randint(0, NC - 1, (int(odd.sum()),), generator=generator)) % NC
    return slab, bias, lab, k
