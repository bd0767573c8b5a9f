"""Exact-integer and per-element oracles for the convolution kernels.

bf16 x bf16 products are exact in fp32.  With small-integer operands and
sum |x||w| < 2**24 every partial sum of a convolution is an exact integer, in
any order and across any split-K partition, whatever adder the matrix unit
uses.  An fp32 output must then equal the fp64 reference bit for bit, and a
bf16 output the reference's single round-to-nearest-even: an indexing,
masking, tail, split or rounding mistake changes at least one bit
(``assert_exact``).  Real-valued operands get a per-element bound derived from
the number formats alone (``assert_elementwise``), and the BatchNorm partial
rows an fp32-summation bound (``assert_stats``).

Everything here runs on the CPU in fp64; tensors from the GPU are copied over.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
EXACT_LIMIT = 2 ** 24  # integers below it are exact in fp32


def magnitude(K: int, density: float = 1.0, want_std: float = 512.0) -> int:
    """Largest operand magnitude ``a`` for a K-term integer dot product: the
    smallest a >= 2 whose typical sum (std a(a+1)/3 * sqrt(K * density) for
    operands uniform in [-a, a]) reaches ``want_std`` -- well past 256, where
    bf16 and fp16 stop holding every integer -- while K * a * a stays below
    2**24 (asserted)."""
    a = 2
    while a * (a + 1) / 3.0 * math.sqrt(max(K * density, 1.0)) < want_std and K * (2 * a) ** 2 < EXACT_LIMIT:
        a *= 2
    assert K * a * a < EXACT_LIMIT, (K, a)
    return a


def int_bf16(shape, lo: int = -2, hi: int = 2, density: float = 1.0, generator=None, device="cpu"):
    """bf16 tensor of integers uniform in [lo, hi]; a share ``1 - density`` of
    the elements is then zeroed.  The caller checks K * max|x| * max|w| < 2**24
    for its case (``check_exact_range``)."""
    assert -256 <= lo <= hi <= 256  # every integer up to 256 is a bf16
    t = torch.randint(lo, hi + 1, tuple(shape), generator=generator, device=device).to(torch.float32)
    if density < 1.0:
        keep = torch.rand(tuple(shape), generator=generator, device=device) < density
        t = t * keep
    return t.to(BF16)


def check_exact_range(K: int, max_x: float, max_w: float):
    assert K * max_x * max_w < EXACT_LIMIT, f"K {K} * {max_x} * {max_w} >= 2**24: sums are not exact in fp32"


def _nchw64(t):
    return t.detach().to("cpu", torch.float64).permute(0, 3, 1, 2).contiguous()


def conv_ref64(x_nhwc, w_krsc, stride: int = 1, pad: int = 2, with_abs: bool = True):
    """fp64 convolution of NHWC x with [Cout][KH][KW][Cin] weights -> (y NHWC,
    S_abs): S_abs is the same convolution of |x| and |w| (None unless
    ``with_abs``)."""
    x, w = _nchw64(x_nhwc), _nchw64(w_krsc)
    y = F.conv2d(x, w, stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()
    s = F.conv2d(x.abs(), w.abs(), stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous() if with_abs else None
    return y, s


def wgrad_ref64(x_nhwc, dy_nhwc, KH: int, KW: int, stride: int = 1, pad: int = 2, with_abs: bool = True):
    """fp64 weight gradient of conv(x, w) under output gradient dy ->
    ([Cout][KH][KW][Cin], S_abs)."""
    def one(x, dy):
        w = torch.zeros(dy.shape[1], x.shape[1], KH, KW, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, w, stride=stride, padding=pad).backward(dy)
        return w.grad.permute(0, 2, 3, 1).contiguous()

    x, dy = _nchw64(x_nhwc), _nchw64(dy_nhwc)
    return one(x, dy), (one(x.abs(), dy.abs()) if with_abs else None)


def dgrad_ref64(dy_nhwc, w_krsc, in_hw, stride: int = 1, pad: int = 2, with_abs: bool = True):
    """fp64 input gradient (autograd) of conv(x, w) under dy -> (dx NHWC, S_abs)."""
    def one(dy, w):
        x = torch.zeros(dy.shape[0], w.shape[1], in_hw[0], in_hw[1], dtype=torch.float64, requires_grad=True)
        F.conv2d(x, w, stride=stride, padding=pad).backward(dy)
        return x.grad.permute(0, 2, 3, 1).contiguous()

    dy, w = _nchw64(dy_nhwc), _nchw64(w_krsc)
    return one(dy, w), (one(dy.abs(), w.abs()) if with_abs else None)


def expected(ref64, dtype):
    """The one correctly rounded result: fp32 of the fp64 reference, then (bf16
    outputs) a single round-to-nearest-even."""
    e = ref64.detach().to("cpu", torch.float64).float()
    return e.to(BF16) if dtype == BF16 else e


def _report(bad, shape, what, tile, row_dims):
    """Where the wrong elements are: count, first / last index, the tile of
    the first, and whether they all lie on the image border / the last M tile."""
    idx = bad.reshape(-1).nonzero().flatten()
    n_cols = 1
    for d in shape[row_dims:]:
        n_cols *= d
    M = bad.numel() // n_cols
    first, last = int(idx[0]), int(idx[-1])
    unr = lambda i: tuple(int(v) for v in torch.unravel_index(torch.tensor(i), shape))  # noqa: E731
    msg = [f"{what}: {idx.numel()} of {bad.numel()} elements wrong; first {unr(first)}, last {unr(last)}"]
    m_all, n_all = idx // n_cols, idx % n_cols
    if tile is not None:
        BM, BN = tile
        m, n = int(m_all[0]), int(n_all[0])
        msg.append(f"first: M tile {m // BM} of {(M + BM - 1) // BM}, N tile {n // BN}, "
                   f"row {m % BM} of the {BM}x{BN} tile")
        msg.append(f"all in the last M tile: {bool((m_all // BM == (M - 1) // BM).all())}")
    if len(shape) == 4 and row_dims == 3:
        H, W = shape[1], shape[2]
        h, w = (m_all // W) % H, m_all % W
        msg.append(f"all on the image border: {bool(((h == 0) | (h == H - 1) | (w == 0) | (w == W - 1)).all())}")
    return "; ".join(msg)


def assert_exact(got, ref64, what: str = "output", tile=None, row_dims=None):
    """``got`` (fp32 or bf16) equals the correctly rounded fp64 reference bit
    for bit.  ``tile`` = (BM, BN) of the kernel, for the failure report;
    ``row_dims``: how many leading dims form the GEMM's M (default all but the last)."""
    assert got.dtype in (torch.float32, BF16), got.dtype
    g = got.detach().cpu()
    want = expected(ref64, g.dtype).reshape(g.shape)
    if torch.equal(g, want):
        return
    bad = (g != want) | (g != g)  # NaN never equals
    rd = g.dim() - 1 if row_dims is None else row_dims
    i = int(bad.reshape(-1).nonzero()[0])
    raise AssertionError(_report(bad, tuple(g.shape), what, tile, rd) +
                         f"; first got {float(g.reshape(-1)[i])} want {float(want.reshape(-1)[i])}")


def half_ulp_bf16(v):
    """Half the spacing of bf16 (8 significant bits) at magnitude v (fp64): 2^(floor(log2 v) - 8)."""
    _, ex = torch.frexp(v.double().abs().clamp_min(2.0 ** -126))  # v = m 2^ex, 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), ex - 9)


def elementwise_bound(ref64, S_abs, K: int, adds: int = 0, dtype=BF16):
    """|got - ref| <= half_ulp_bf16(|ref| + E) + E with E = 2 (K + adds) 2^-24 S_abs
    for bf16 outputs, E alone for fp32: fp32 accumulation of K exact products
    in any order with one ulp per addition (not half: this does not rest on the
    matrix unit rounding to nearest; ``adds``: further fp32 additions, the
    split count), then one round-to-nearest of the accumulator, which lies
    within E of the reference.  Half a bf16 ulp is between 2^-9 |ref| and
    2^-8 |ref|: a flat 2^-9 |ref| would reject correctly rounded results in
    the lower part of every binade."""
    acc = 2.0 * (K + adds) * 2.0 ** -24 * S_abs.double()
    if dtype == BF16:
        return half_ulp_bf16(ref64.double().abs() + acc) + acc
    return acc


def assert_elementwise(got, ref64, S_abs, K: int, adds: int = 0, what: str = "output"):
    """Per-element bound for real-valued operands (``elementwise_bound``)."""
    assert got.dtype in (torch.float32, BF16), got.dtype
    g = got.detach().cpu().double()
    ref = ref64.detach().cpu().double().reshape(g.shape)
    bound = elementwise_bound(ref, S_abs.detach().cpu().reshape(g.shape), K, adds, got.dtype)
    err = (g - ref).abs()
    bad = ~(err <= bound)  # NaN fails
    if bad.any():
        ratio = torch.nan_to_num(err / bound.clamp_min(1e-300), nan=float("inf"))
        i = int(ratio.argmax())
        unr = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), g.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements over the per-element bound; largest "
                             f"error/bound {float(ratio.reshape(-1)[i]):.3f} at {unr}: got {float(g.reshape(-1)[i])} "
                             f"ref {float(ref.reshape(-1)[i])}")


def assert_stats(rows, y_expected_bf16, T=None, what: str = "statistics"):
    """BatchNorm partial rows [T][2][C] (sum, sum of squares per M tile) of the
    expected bf16 output: the T written rows are finite, rows past T still hold
    the caller's NaN pre-fill, and the column sums match fp64 sums of y and y^2
    within M 2^-23 sum|y| and M 2^-23 sum y^2 (fp32 summation in any order)."""
    r = rows.detach().cpu().double()
    T = r.shape[0] if T is None else T
    assert 0 < T <= r.shape[0], f"{what}: {T} rows returned, buffer has {r.shape[0]}"
    assert torch.isfinite(r[:T]).all(), f"{what}: a partial row among the first {T} is not finite"
    assert torch.isnan(r[T:]).all(), f"{what}: rows past the returned count {T} were written"
    y = y_expected_bf16.detach().cpu().double().reshape(-1, r.shape[-1])
    M = y.shape[0]
    for j, (name, v) in enumerate((("sum", y), ("sum of squares", y * y))):
        want, tol = v.sum(0), M * 2.0 ** -23 * v.abs().sum(0)
        err = (r[:T, j].sum(0) - want).abs()
        if not bool((err <= tol).all()):
            c = int((err - tol).argmax())
            raise AssertionError(f"{what}: channel {c} {name} {float(r[:T, j].sum(0)[c])} vs {float(want[c])} "
                                 f"(tolerance {float(tol[c])})")
