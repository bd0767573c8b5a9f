"""Exact and per-element oracles for the fused BatchNorm + ReLU + 2x2 max-pool
kernels (bn_pool.hip, bn_fin_dev.h) and the classifier head (head.hip,
head_wgrad_dev.h), in the style of tests/kernels/exact.py.

Two regimes:

* exact: small-integer activations and gradients with dyadic per-channel
  coefficients make every intermediate of every kernel a multiple of a power
  of two that fp32 holds exactly, so atomic order, split order and fma
  contraction cannot matter.  An fp32 output equals the fp64 reference bit for
  bit, a bf16 output its single round-to-nearest-even (``exact.assert_exact``).
  The references assert the representability of every intermediate
  (``check_f32`` / ``check_sum_exact``): the regime proves itself per shape.
* real-valued: the pool argmax / ReLU decision is reproduced bit for bit from
  the fp32 coefficient table (``pool_select`` emulates the kernels' single
  fp32 fma), so forward outputs are still compared exactly and the backward
  routing is decided identically on both sides; sums and ``dy`` get bounds
  derived from the operation count and the number formats.

Everything here runs on the CPU in fp64; tensors from the GPU are copied over.
No constant comes from a run of the code under test.
"""
from __future__ import annotations

import math

import torch

from tests.kernels import exact

BF16 = torch.bfloat16
U32 = 2.0 ** -23  # one fp32 ulp at 1: every bound below charges a full ulp per rounding (twice round-to-nearest)


def cpu64(t):
    return t.detach().to("cpu", torch.float64)


def representable(t) -> bool:
    return bool((t.float().double() == t).all())


def check_f32(what: str, t):
    """Every element of the fp64 tensor ``t`` is an fp32 number."""
    assert representable(t), f"{what}: not exactly representable in fp32, the exact regime does not hold"


def check_sum_exact(what: str, terms, dims):
    """The fp64 ``terms`` sum exactly in fp32 in ANY order over ``dims``: all
    are multiples of one 2^-g (g <= 24) and sum |terms| 2^g < 2^24, so every
    partial sum is an integer below 2^24 on that grid."""
    check_f32(what, terms)
    for g in range(25):
        s = terms * 2.0 ** g
        if bool((s == s.round()).all()):
            top = float(s.abs().sum(dims).max()) if terms.numel() else 0.0
            assert top < exact.EXACT_LIMIT, f"{what}: sum |terms| 2^{g} = {top} >= 2^24"
            return
    raise AssertionError(f"{what}: terms are not on a 2^-24 grid")


# ---------------------------------------------------------------------------
# BatchNorm + ReLU + 2x2 max-pool
# ---------------------------------------------------------------------------
def windows(t):
    """[B][H][W][C] -> [B][Ho][Wo][4][C], window positions in row-major order
    (0: top-left, 1: top-right, 2: bottom-left, 3: bottom-right)."""
    B, H, W, C = t.shape
    return t.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4, C)


def unwindows(w):
    """Inverse of ``windows``."""
    B, Ho, Wo, _, C = w.shape
    return w.reshape(B, Ho, Wo, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * Ho, 2 * Wo, C)


def pool_select(y, sc, sh, tie: str = "first", positive: str = "gt"):
    """The window choice exactly as the kernels make it -> (best, sel).

    z = fmaf(sc, y, sh) is emulated as (sc.double() * y.double() + sh.double())
    .float(): the fp32 x bf16 product is exact in fp64 (24 + 8 significant
    bits), so this is the fp32 fma's single rounding.  Then relu, then the
    first (row-major) window position holding the maximum; ``sel`` [B][Ho][Wo]
    [4][C] marks it, and is all false where the maximum is not > 0 (no
    gradient).  ``best`` [B][Ho][Wo][C] is the pooled forward value (an fp32
    number held in fp64).  tie = "last" and positive = "ge" are the two wrong
    rules the oracle must tell apart (tests/unit/test_exact_oracle.py)."""
    yw = windows(cpu64(y))
    z = (cpu64(sc) * yw + cpu64(sh)).float().double()
    r = z.clamp_min(0.0)
    best = torch.full_like(r[:, :, :, 0], -math.inf)
    arg = torch.zeros_like(best, dtype=torch.int64)
    for w in range(4):
        m = (r[:, :, :, w] > best) if tie == "first" else (r[:, :, :, w] >= best)
        best = torch.where(m, r[:, :, :, w], best)
        arg = torch.where(m, torch.full_like(arg, w), arg)
    live = (best > 0) if positive == "gt" else (best >= 0)
    sel = torch.nn.functional.one_hot(arg, 4).permute(0, 1, 2, 4, 3).bool() & live.unsqueeze(3)
    return best, sel


def pool_fwd_ref(y, coef):
    """Forward contract given the coefficient table coef [4][C] (mean, invstd,
    scale, shift): pooled = max over the window of relu(fmaf(scale, y, shift)),
    an fp32 number; the kernels store its bf16 rounding."""
    best, _ = pool_select(y, coef[2], coef[3])
    return best


def bwd_terms(y, dP, coef, exact_regime: bool = False, tie: str = "first", positive: str = "gt"):
    """-> (dz, xhat) [B][Ho][Wo][4][C] in fp64: dz = dP at the selected window
    position (``pool_select``) and 0 elsewhere, xhat = (y - mean) * invstd."""
    coef = cpu64(coef)
    _, sel = pool_select(y, coef[2], coef[3], tie, positive)
    dz = torch.where(sel, cpu64(dP).unsqueeze(3), torch.zeros((), dtype=torch.float64))
    d = windows(cpu64(y)) - coef[0]
    xhat = d * coef[1]
    if exact_regime:
        check_f32("scale*y + shift", coef[2] * windows(cpu64(y)) + coef[3])
        check_f32("y - mean", d)
        check_f32("dz*(y - mean)", dz * d)
    return dz, xhat


def bwd_sums_ref(y, dP, coef, exact_regime: bool = False):
    """Backward-reduce contract given coef: per channel (sum dz, sum dz*xhat,
    sum |dz|, sum |dz*xhat|), fp64.  In the exact regime the terms are checked
    to sum exactly in any order (atomics, any block / row partition)."""
    dz, xhat = bwd_terms(y, dP, coef, exact_regime)
    t = dz * xhat
    if exact_regime:
        check_sum_exact("sum dz", dz, (0, 1, 2, 3))
        check_sum_exact("sum dz*xhat", t, (0, 1, 2, 3))
    dims = (0, 1, 2, 3)
    return dz.sum(dims), t.sum(dims), dz.abs().sum(dims), t.abs().sum(dims)


def sums_bound(n_pix: int, s_abs):
    """|fp32 sum - fp64 sum| <= (n_pix + 3) 2^-23 sum|term|.

    Per channel at most n_pix = B*Ho*Wo terms are nonzero (one per window; the
    zeros add exactly).  Each term dz * (y - mean) * invstd carries three
    roundings (the subtraction, two products): 3 ulp of |term|.  Adding n_pix
    terms in any order and over any partition (threads, LDS tree, partial rows
    or atomics) rounds each term's running sum at most n_pix - 1 times with
    |partial| <= sum|term|: (n_pix - 1) ulp of sum|term|.  The read-back rows
    are added in fp64 by the test.  sum dz has no per-term rounding and is
    inside the same bound."""
    return (n_pix + 3) * U32 * s_abs.double()


def apply_coefficients(gamma, invstd, s_dz, s_dzx, M: int):
    """a = gamma*invstd, b = -a*sum(dz*xhat)/M, c = -a*sum(dz)/M in fp64."""
    a = cpu64(gamma) * cpu64(invstd)
    return a, -a * cpu64(s_dzx) / M, -a * cpu64(s_dz) / M


def apply_ref(y, dP, coef, gamma, rows_dz, rows_dzx, M: int, exact_regime: bool = False):
    """Backward-apply contract given coef and the rows [R][C] of per-channel
    sums the kernel read (added here in fp64): dy = a*dz + b*xhat + c ->
    (dy [B][H][W][C] fp64, m_a, m_b, m_c): the term magnitudes |a dz|,
    |a| sum_r|row_r|/M |xhat| (>= |b xhat|) and |a| sum_r|row_r|/M (>= |c|) for
    ``apply_bound``.  In the exact regime every intermediate of both kernel
    formulations is checked: a, b, c (bn_bwd_finalize), b*invstd and
    -a*dgamma*(1/M)*invstd step by step (the SUMS prologue), the three terms
    and their partial sum; the rows must sum exactly in any order."""
    coef = cpu64(coef)
    rz, rzx = cpu64(rows_dz).reshape(-1, coef.shape[1]), cpu64(rows_dzx).reshape(-1, coef.shape[1])
    s_dz, s_dzx = rz.sum(0), rzx.sum(0)
    a, b, c = apply_coefficients(gamma, coef[1], s_dz, s_dzx, M)
    dz, xhat = bwd_terms(y, dP, coef, exact_regime)
    d = windows(cpu64(y)) - coef[0]
    t1, t2 = a * dz, b * xhat
    if exact_regime:
        check_sum_exact("rows of sum dz", rz, (0,))
        check_sum_exact("rows of sum dz*xhat", rzx, (0,))
        for name, v in (("a", a), ("a*dgamma", a * s_dzx), ("a*dbeta", a * s_dz), ("1/M", torch.tensor(1.0 / M)),
                        ("b", b), ("c", c), ("b*invstd", b * coef[1]), ("a*dz", t1), ("b*invstd*(y-mean)", b * coef[1] * d),
                        ("a*dz + b*xhat", t1 + t2), ("dy", t1 + t2 + c)):
            check_f32(name, v)
    dy = unwindows(t1 + t2 + c)
    m_b = unwindows((a.abs() * rzx.abs().sum(0) / M) * xhat.abs())
    m_c = (a.abs() * rz.abs().sum(0) / M).expand_as(dy)
    return dy, unwindows(t1.abs()), m_b, m_c


def apply_bound(dy_ref, m_a, m_b, m_c, rows: int):
    """|dy - ref| <= half_ulp_bf16(|ref| + E) + E,
    E = 2^-23 (3 m_a + (rows + 7) m_b + (rows + 5) m_c).

    The reference coefficients are fp64 functions of the fp32 rows read back
    from the device, so only the kernel's own arithmetic is charged, one ulp
    per rounding (m_a, m_b, m_c: ``apply_ref``):
      a dz term:   a = gamma*invstd (1), the product (1), the addition (1);
      b xhat term: the sum of ``rows`` rows (rows - 1 roundings, each within
                   sum_r |row_r|, which is what m_b is built from), a (1),
                   -a*dgamma (1), 1/M (1) and its product (1) -- or the division
                   by M (1) --, times invstd (1), y - mean (1), the product (1),
                   the addition (1): rows + 7;
      c term:      the row sum (rows - 1), a (1), -a*dbeta (1), 1/M and its
                   product (2), the final addition (1): rows + 5.
    Then one bf16 round-to-nearest of a value within E of the reference."""
    E = U32 * (3.0 * m_a + (rows + 7) * m_b + (rows + 5) * m_c)
    return exact.half_ulp_bf16(dy_ref.abs() + E) + E


def assert_within(got, ref, bound, what: str):
    """Per element |got - ref| <= bound (NaN fails); reports the worst ratio."""
    g, r, b = cpu64(got), cpu64(ref), cpu64(bound)
    r, b = r.reshape(g.shape), b.expand(g.shape) if b.dim() <= g.dim() else b.reshape(g.shape)
    err = (g - r).abs()
    bad = ~(err <= b)
    if bool(bad.any()):
        ratio = torch.nan_to_num(err / b.clamp_min(1e-300), nan=math.inf)
        i = int(ratio.argmax())
        unr = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), g.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements over the bound; largest error/bound "
                             f"{float(ratio.reshape(-1)[i]):.3f} at {unr}: got {float(g.reshape(-1)[i])!r} "
                             f"ref {float(r.reshape(-1)[i])!r} bound {float(b.reshape(-1)[i])!r}")


def bn_coefficients(sums, M: int, gamma, beta, bias, eps: float, momentum: float, running, mode: int = 0):
    """fp64 contract of bn_finalize_kernel / bn_fin_block given the fp32 totals.

    sums: [R][2][C] (or [2][C]) rows of (sum, sum of squares), added here in
    fp64; running = (rmean, rvar) before the call or None; bias may be None.
    mode 0 (train): mean = sum/M, var = max(sumsq/M - mean^2, 0), running
    statistics updated with mean + bias and the UNBIASED variance var M/(M-1).
    mode 1 (eval): mean = rmean - bias, var = rvar, running unchanged.
    eps and momentum are taken at their fp32 values (kernel arguments).
    -> dict of mean, var, invstd, scale, shift, rmean, rvar [C]."""
    eps, momentum = float(torch.tensor(eps, dtype=torch.float32)), float(torch.tensor(momentum, dtype=torch.float32))
    g, b = cpu64(gamma), cpu64(beta)
    bi = cpu64(bias) if bias is not None else torch.zeros_like(g)
    rm, rv = (cpu64(running[0]), cpu64(running[1])) if running is not None else (None, None)
    if mode == 0:
        s = cpu64(sums).reshape(-1, 2, g.numel()).sum(0)
        mean = s[0] / M
        var = (s[1] / M - mean * mean).clamp_min(0.0)
        if rm is not None:
            unb = var * M / (M - 1) if M > 1 else var
            rm, rv = (1.0 - momentum) * rm + momentum * (mean + bi), (1.0 - momentum) * rv + momentum * unb
    else:
        mean, var = rm - bi, rv
    invstd = (var + eps).rsqrt()
    sc = g * invstd
    return {"mean": mean, "var": var, "invstd": invstd, "scale": sc, "shift": b - mean * sc, "rmean": rm, "rvar": rv}


def bn_coefficient_bounds(sums, M: int, gamma, beta, bias, eps: float, momentum: float, running, mode: int = 0):
    """Bounds on the fp32 coefficients against ``bn_coefficients`` of the same
    fp32 totals, one ulp (2^-23 relative) charged per rounding, u = 2^-23.

    R = rows summed, S1 = sum_r |sum_r|, S2 = sum_r |sumsq_r| (>= the totals).
    mean   = t1/M:       R - 1 additions within S1 and the division:
                         e_mean = R u S1/M.
    var    = max(t2/M - mean^2, 0): t2/M as above (R u S2/M); mean^2 carries
                         2 |mean| e_mean + e_mean^2 and its own rounding
                         (u mean^2); the subtraction one more ulp of the larger
                         operand; the clamp is 1-Lipschitz:
                         e_var = R u S2/M + 2 |mean| e_mean + e_mean^2
                                 + u mean^2 + u max(S2/M, mean^2).
                         This is a few ulp of sumsq/M + mean^2, NOT of var: for
                         a channel with mean 64 and variance 1/16 it is about
                         (3R + 2) 2^-23 4096 = 2.4e-3 (R = 1), 4 % of the
                         variance.  That cancellation is the formula's limit.
    invstd = rsqrt(var + eps): the argument is within e_var + u (var + eps) of
                         the reference's; rsqrt is monotone, so the result lies
                         between rsqrt at the two ends of that interval, widened
                         by 2 ulp for the hardware rsqrt (v_rsq_f32 is
                         documented to 1 ulp):
                         e_invstd = max |rsqrt(v +- e) - invstd| + 2 u invstd.
                         With var = 0 (constant channel, eps = 1e-3) e is about
                         5 u c^2, relative 2.5e-3 c^2 u / eps of invstd = 31.6.
    scale  = gamma invstd:     |gamma| e_invstd + u |scale|.
    shift  = beta - mean scale: |scale| e_mean + |mean| e_scale + e_mean e_scale
                         + u |mean scale| + u max(|beta|, |mean scale|).
    rmean  = (1-m) rmean + m (mean + bias): m e_mean + 4 u (|rmean| + m (|mean|
                         + |bias|)) (1 - m, two products, the inner and the
                         outer addition).
    rvar   = (1-m) rvar + m var M/(M-1): m e_var M/(M-1) + 5 u (|rvar| + m unb).
    eval mode: mean = rmean - bias (1 ulp of |rmean| + |bias|), var = rvar (exact).
    -> dict like bn_coefficients' (entries None where there is no output)."""
    ref = bn_coefficients(sums, M, gamma, beta, bias, eps, momentum, running, mode)
    eps = float(torch.tensor(eps, dtype=torch.float32))
    m = float(torch.tensor(momentum, dtype=torch.float32))
    g, b = cpu64(gamma), cpu64(beta)
    bi = cpu64(bias) if bias is not None else torch.zeros_like(g)
    u = U32
    mean, var = ref["mean"], ref["var"]
    if mode == 0:
        s = cpu64(sums).reshape(-1, 2, g.numel())
        R = s.shape[0]
        S1, S2 = s[:, 0].abs().sum(0) / M, s[:, 1].abs().sum(0) / M
        e_mean = R * u * S1
        e_var = R * u * S2 + 2 * mean.abs() * e_mean + e_mean ** 2 + u * mean ** 2 + u * torch.maximum(S2, mean ** 2)
    else:
        e_mean = u * (cpu64(running[0]).abs() + bi.abs())
        e_var = torch.zeros_like(var)
    e_arg = e_var + u * (var + eps)
    lo, hi = ((var - e_arg).clamp_min(0.0) + eps).rsqrt(), (var + e_arg + eps).rsqrt()
    e_is = torch.maximum(lo - ref["invstd"], ref["invstd"] - hi) + 2 * u * ref["invstd"]
    e_sc = g.abs() * e_is + u * ref["scale"].abs()
    ms = (mean * ref["scale"]).abs()
    e_sh = ref["scale"].abs() * e_mean + mean.abs() * e_sc + e_mean * e_sc + u * ms + u * torch.maximum(b.abs(), ms)
    out = {"mean": e_mean, "var": e_var, "invstd": e_is, "scale": e_sc, "shift": e_sh, "rmean": None, "rvar": None}
    if mode == 0 and running is not None:
        unb = var * M / (M - 1) if M > 1 else var
        out["rmean"] = m * e_mean + 4 * u * (cpu64(running[0]).abs() + m * (mean.abs() + bi.abs()))
        out["rvar"] = m * e_var * (M / (M - 1) if M > 1 else 1.0) + 5 * u * (cpu64(running[1]).abs() + m * unb)
    return ref, out


def assert_coefficients(coef, running_after, sums, M, gamma, beta, bias, eps, momentum, running_before, mode=0,
                        what="bn coefficients"):
    """The published table coef [4][C] (mean, invstd, scale, shift) and the
    running statistics after the call, against ``bn_coefficient_bounds``."""
    ref, bnd = bn_coefficient_bounds(sums, M, gamma, beta, bias, eps, momentum, running_before, mode)
    for i, k in enumerate(("mean", "invstd", "scale", "shift")):
        assert_within(coef[i], ref[k], bnd[k], f"{what}: {k}")
    if running_after is not None:
        for i, k in enumerate(("rmean", "rvar")):
            if bnd[k] is not None:
                assert_within(running_after[i], ref[k], bnd[k], f"{what}: {k}")
            else:  # eval mode leaves the running statistics alone
                assert torch.equal(running_after[i].cpu(), running_before[i].cpu()), f"{what}: {k} changed in eval mode"
    return ref


# ---------------------------------------------------------------------------
# classifier head
# ---------------------------------------------------------------------------
def head_ref(h, w, bias, labels):
    """fp64 Linear -> LogSoftMax -> NLL (mean) and its gradients.  labels None:
    predict mode (logits / logp only).  -> dict."""
    h, w, bias = cpu64(h), cpu64(w), cpu64(bias)
    B, NC = h.shape[0], w.shape[0]
    lg = h @ w.t() + bias
    mx = lg.max(1, keepdim=True).values
    lse = mx + (lg - mx).exp().sum(1, keepdim=True).log()
    out = {"logits": lg, "logp": lg - lse, "softmax": (lg - lse).exp(), "spread": (lg - mx).abs().max(1).values,
           "S_logit": h.abs() @ w.abs().t() + bias.abs()}
    if labels is not None:
        onehot = torch.nn.functional.one_hot(labels.cpu().long(), NC).double()
        d = (out["softmax"] - onehot) / B
        lb = -(out["logp"] * onehot).sum(1)
        out.update(dlogits=d, loss_b=lb, loss=lb.mean())
        out.update(head_grads_ref(h, w, d))
    return out


def head_grads_ref(h, w, dlogits):
    """The linear gradients given dlogits (the head kernels' contract for the
    dlogits they were handed): dh = dlogits W, dW = dlogits^T h, db = column
    sums, with the sums of magnitudes for the bounds."""
    h, w, d = cpu64(h), cpu64(w), cpu64(dlogits)
    return {"dh": d @ w, "S_dh": d.abs() @ w.abs(), "dW": d.t() @ h, "S_dW": d.abs().t() @ h.abs(), "db": d.sum(0),
            "S_db": d.abs().sum(0)}


def logit_depth(F: int) -> int:
    """Roundings on the longest path of one logit in head_fwd_bwd_kernel: the
    product and the 7 additions of its 8-feature expression, one addition into
    the accumulator per 2048-feature trip, 15 additions of the 16 LDS
    partials, a 4-level butterfly and the bias: 28 + ceil(F / 2048)."""
    return 28 + (F + 2047) // 2048


def logit_bound(ref, F: int):
    """|fp32 logit - fp64 logit| <= logit_depth(F) 2^-24 (sum_j |h_j w_j| + |b|):
    every product passes through at most logit_depth roundings, each at most
    half an ulp (plain vector-ALU multiplies, adds and fmas round to nearest;
    no matrix unit is involved) of a partial sum no larger than the sum of
    magnitudes."""
    return logit_depth(F) * 0.5 * U32 * ref["S_logit"]


def head_exact_inputs(B: int, F: int, generator, NC: int = 10):
    """Integer head inputs on which the fast exp / log are exact.

    h: integers in [-2, 2] (bf16); features 0..NC-1 one-hot encode an intended
    class k_b (value 2 at k_b), whose weights are 512 on the diagonal, so logit
    k_b leads by 1024 minus the rest; the other weights are multiples of 2^-6
    in [-2/64, 2/64] and the bias small integers.  The caller asserts the lead
    (>= 160: exp of every other term is 0 in fp32, the sum of exponentials is
    exactly 1 and its log exactly 0).  Labels are half the intended class and
    half another one; classes 0 and 9 both occur (B >= 2) as intended classes.
    -> h (bf16), w, bias (fp32), labels (int64), intended (int64)."""
    assert F >= NC or F == 8
    h = exact.int_bf16((B, F), -2, 2, generator=generator)
    w = torch.randint(-2, 3, (NC, F), generator=generator).float() / 64.0
    nb = min(NC, F)  # F = 8: classes 0..7 can win
    k = torch.randint(0, nb, (B,), generator=generator)
    k[0] = 0
    if B > 1:
        k[1] = nb - 1
    h[:, :nb] = 0
    h[torch.arange(B), k] = 2
    w[:, :nb] = 0
    w[torch.arange(nb), torch.arange(nb)] = 512.0
    bias = torch.randint(-3, 4, (NC,), generator=generator).float()
    lab = k.clone()
    wrong = torch.arange(B) % 2 == 1
    lab[wrong] = (k[wrong] + 1 + torch.randint(0, NC - 1, (int(wrong.sum()),), generator=generator)) % NC
    if B > 2:
        lab[2], lab[3 % B] = 9, 0  # both end classes occur as labels too
    return h, w, bias, lab, k


def head_exact_ref(h, w, bias, labels):
    """``head_ref`` on ``head_exact_inputs``, with the regime checked: the lead
    of the largest logit, and fp32 representability / exact summability of
    every intermediate of head_fwd_bwd_kernel and head_wgrad_body."""
    r = head_ref(h, w, bias, labels)
    hh, ww = cpu64(h), cpu64(w)
    B = hh.shape[0]
    top2 = r["logits"].topk(2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) >= 160.0, "the largest logit must lead by 160"
    check_sum_exact("logit products", hh.unsqueeze(1) * ww.unsqueeze(0), (2,))
    for k in ("logits", "logp"):
        check_f32(k, r[k])
    assert bool(((r["softmax"] == 0) | (r["softmax"] == 1)).all())
    if labels is not None:
        check_f32("1/B", torch.tensor(1.0 / B))
        check_sum_exact("dh terms", r["dlogits"].unsqueeze(2) * ww.unsqueeze(0), (1,))
        check_sum_exact("dW terms", r["dlogits"].unsqueeze(2) * hh.unsqueeze(1), (0,))
        check_sum_exact("db terms", r["dlogits"], (0,))
        check_sum_exact("loss terms", r["loss_b"], (0,))
        check_f32("mean loss", r["loss"])
    return r


# ---------------------------------------------------------------------------
# inputs of the exact regime
# ---------------------------------------------------------------------------
def int_bn_inputs(B: int, H: int, C: int, generator, W: int | None = None):
    """Integer BN / ReLU / pool operands with hand-set dyadic coefficients.

    y integers in [-6, 6] (bf16), dP integers in [-8, 8] (bf16); per channel
    mean an integer in [-3, 3], invstd in {1, 1/2, 1/4}, gamma = +-2^j with j in
    {-1, 0, 1} (about 30 % negative; a negative scale puts the pooled max at
    the smallest y), beta an integer in [-2, 2]; channel 0 has gamma = 0 and
    beta = 2: all four window positions tie at shift > 0 and the gradient
    belongs to position 0.  scale = gamma*invstd, shift = beta - mean*scale.
    -> y, dP (bf16), coef [4][C] (mean, invstd, scale, shift), gamma (fp32)."""
    W = H if W is None else W
    y = exact.int_bf16((B, H, W, C), -6, 6, generator=generator)
    dP = exact.int_bf16((B, H // 2, W // 2, C), -8, 8, generator=generator)
    mean = torch.randint(-3, 4, (C,), generator=generator).double()
    invstd = torch.pow(2.0, -torch.randint(0, 3, (C,), generator=generator).double())
    gamma = torch.pow(2.0, torch.randint(-1, 2, (C,), generator=generator).double())
    gamma = gamma * torch.where(torch.rand(C, generator=generator) < 0.3, -1.0, 1.0).double()
    beta = torch.randint(-2, 3, (C,), generator=generator).double()
    gamma[0], beta[0] = 0.0, 2.0
    scale = gamma * invstd
    coef = torch.stack([mean, invstd, scale, beta - mean * scale])
    check_f32("hand-set coefficients", coef)
    return y, dP, coef.float(), gamma.float()
