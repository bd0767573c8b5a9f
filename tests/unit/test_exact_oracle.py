"""The exact-integer / per-element oracles of tests/kernels/exact.py catch what
the whole-tensor Frobenius ratio of the older conv tests lets through.

A correct result is computed on the CPU (fp32 accumulation of exact bf16
products, two K slabs, one bf16 rounding), then mutated the way a kernel goes
wrong: a border tap skipped at one pixel, a lost store lane, a wrong last row
of the M tail, truncation instead of round-to-nearest-even, a split-K slab
rounded through bf16, two output rows swapped.  Every mutation must raise under
the oracle; the ratio of the old check is recorded for the ones it misses.

The second half checks the BatchNorm + ReLU + pool and head oracles of
tests/kernels/exact_bn_head.py against fp64 autograd, shows that the integer
inputs tell the pool rule's wrong variants apart, and that a plain fp32
evaluation of the kernels' formulas stays inside the derived bounds while a
misrouted gradient or a dropped item does not.

The last part does the same for tests/kernels/exact_nhwc.py (the ResNet-50
path's channels-last BatchNorm, max pool and glue kernels): the BN formulas
against fp64 autograd, the pool reference against F.max_pool2d's indices, and
the wrong rules (last-maximum ties, a >= 0 ReLU decision, an unrounded residual
BN, a dropped row, a swapped stem tap) told apart from the right ones."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.kernels import exact
from tests.kernels import exact_bn_head as xb

BF16 = torch.bfloat16
SHAPES = [(8, 32, 8, 64), (8, 16, 64, 128), (3, 4, 256, 128)]  # (B, H, Cin, Cout), 5x5, pad 2
MUTATIONS = ["tap_dropped", "element_zeroed", "last_pixel_zeroed", "truncated", "slab_through_bf16", "rows_swapped"]
# the mutations whose old ratio stays under the old 8e-3 bound, per shape
OLD_CHECK_MISSES = {SHAPES[0]: ["tap_dropped", "element_zeroed", "last_pixel_zeroed", "truncated"],
                    SHAPES[1]: ["element_zeroed", "truncated"], SHAPES[2]: ["truncated"]}

# A rounding-sized mutation (at most one bf16 ulp, 2^-7 |y|) is below the
# per-element bound once its accumulation term 2 K 2^-24 S_abs passes a bf16
# ulp: with S_abs about 0.6 sqrt(K) |y| for these random operands that is K above
# about 2200.  At K = 6400 only the integer case catches these two.
BELOW_ELEMENTWISE_BOUND = {SHAPES[2]: ["truncated", "slab_through_bf16"]}


def _rel(a, b):  # the old check (tests/kernels/test_convnet_gpu.py _rel)
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))


def _truncate_bf16(t32):
    return (t32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)


class Case:
    """Operands, the fp64 reference and the two fp32 K slabs (input channels
    split in halves) of one conv."""

    def __init__(self, shape, kind):
        B, H, cin, cout = shape
        g = torch.Generator().manual_seed(B * H + cin + (kind == "int"))
        self.shape, self.kind, self.K = shape, kind, 25 * cin
        if kind == "int":
            a = exact.magnitude(self.K)
            exact.check_exact_range(self.K, a, a)
            self.x = exact.int_bf16((B, H, H, cin), -a, a, generator=g)
            self.w = exact.int_bf16((cout, 5, 5, cin), -a, a, density=0.75, generator=g)
        else:
            self.x = torch.randn(B, H, H, cin, generator=g).to(BF16)
            self.w = (torch.randn(cout, 5, 5, cin, generator=g) * 0.05).to(BF16)
        self.ref, self.S = exact.conv_ref64(self.x, self.w)
        h = cin // 2
        self.slabs = [exact.conv_ref64(self.x[..., s], self.w[..., s], with_abs=False)[0].float()
                      for s in (slice(0, h), slice(h, cin))]

    def check(self, y):
        if self.kind == "int":
            exact.assert_exact(y, self.ref, "y", tile=(128, 64))
        else:
            exact.assert_elementwise(y, self.ref, self.S, self.K, adds=2, what="y")

    def result(self, mutation=None):
        B, H, cin, cout = self.shape
        s0, s1 = self.slabs
        if mutation == "slab_through_bf16":
            s0 = s0.to(BF16).float()
        acc = s0 + s1
        if mutation == "tap_dropped":  # tap (0, 0) of output pixel (2, 2) reads x[0, 0]
            acc = acc.clone()
            acc[:, 2, 2, :] -= torch.einsum("bc,oc->bo", self.x[:, 0, 0, :].float(), self.w[:, 0, 0, :].float())
        if mutation == "truncated":
            return _truncate_bf16(acc)
        y = acc.to(BF16)
        if mutation == "element_zeroed":  # per image, the channel of median magnitude at one pixel
            for n in range(B):
                c = int(self.ref[n, H // 2, H // 3].abs().argsort()[cout // 2])
                y[n, H // 2, H // 3, c] = 0
        elif mutation == "last_pixel_zeroed":
            y[-1, -1, -1, :] = 0
        elif mutation == "rows_swapped":
            y[B // 2, [0, 1]] = y[B // 2, [1, 0]]
        return y


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    return Case(shape, kind)


def _id(p):
    return "x".join(map(str, p[0])) + "-" + p[1]


@pytest.fixture(params=[(s, k) for s in SHAPES for k in ("int", "randn")], ids=_id)
def case(request):
    return _case(*request.param)


def test_unmutated_result_passes(case):
    y = case.result()
    case.check(y)
    assert _rel(y, case.ref) < 8e-3
    if case.kind == "int":  # sums past 256: an intermediate in bf16 / fp16 would not hold them
        assert float((case.ref.abs() > 256).double().mean()) > 0.25
        exact.assert_exact(case.slabs[0] + case.slabs[1], case.ref, "fp32 sum")


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_mutation_raises(case, mutation):
    y = case.result(mutation)
    assert not torch.equal(y, case.result())
    if case.kind == "randn" and mutation in BELOW_ELEMENTWISE_BOUND.get(case.shape, ()):
        case.check(y)  # on record: only the integer case of this shape sees it
        return
    with pytest.raises(AssertionError):
        case.check(y)


@pytest.mark.parametrize("shape_mutation", [(s, m) for s in SHAPES for m in OLD_CHECK_MISSES[s]], ids=_id)
def test_old_ratio_misses(shape_mutation):
    """On record: the Frobenius ratio of the old check stays under its 8e-3
    bound for these mutations of a real-valued result (the same cases raise in
    test_mutation_raises)."""
    shape, mutation = shape_mutation
    case = _case(shape, "randn")
    r = _rel(case.result(mutation), case.ref)
    assert 1.66e-3 < r < 8e-3, r


def test_report_locates_the_fault():
    """The failure message names the count, the first / last index, the tile
    and row of the first wrong element and the border / last-tile flags."""
    c = Case(SHAPES[2], "int")
    with pytest.raises(AssertionError) as e:
        exact.assert_exact(c.result("last_pixel_zeroed"), c.ref, "y", tile=(32, 64))
    msg = str(e.value)
    assert "first (2, 3, 3, " in msg and "last (2, 3, 3, " in msg
    assert "M tile 1 of 2" in msg and "row 15 of the 32x64 tile" in msg
    assert "all in the last M tile: True" in msg and "all on the image border: True" in msg


def test_stats_oracle():
    """assert_stats: exact sums pass; a dropped row, a NaN row, a written row
    past the returned count and one pixel left out of the sums all raise."""
    g = torch.Generator().manual_seed(3)
    y = exact.int_bf16((2, 8, 8, 16), -64, 64, generator=g)
    yf = y.double().reshape(4, 32, 16)  # four M tiles of 32 rows
    rows = torch.full((6, 2, 16), float("nan"))
    rows[:4, 0], rows[:4, 1] = yf.sum(1).float(), (yf * yf).sum(1).float()
    exact.assert_stats(rows, y, 4)
    with pytest.raises(AssertionError):
        exact.assert_stats(rows, y, 3)
    with pytest.raises(AssertionError):
        exact.assert_stats(rows, y, 5)
    bad = rows.clone()
    bad[4] = 0.0
    with pytest.raises(AssertionError):
        exact.assert_stats(bad, y, 4)
    bad = rows.clone()
    bad[3, 0] -= yf[3, -1].float()  # the last pixel missing from the sums
    with pytest.raises(AssertionError):
        exact.assert_stats(bad, y, 4)


# ---------------------------------------------------------------------------
# BatchNorm + ReLU + pool / head oracles (tests/kernels/exact_bn_head.py)
# ---------------------------------------------------------------------------
def _autograd_bn_relu_pool(y, gamma, beta, dP, eps):
    """fp64 batch_norm -> relu -> max_pool2d and its gradients by autograd (NHWC in / out)."""
    yr = y.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    g, b = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    o = F.max_pool2d(F.relu(F.batch_norm(yr, None, None, g, b, True, 0.0, eps)), 2, 2)
    o.backward(dP.double().permute(0, 3, 1, 2))
    return o.detach().permute(0, 2, 3, 1), yr.grad.permute(0, 2, 3, 1), g.grad, b.grad


def test_bn_pool_references_match_autograd():
    """On tie-free real data with the coefficients taken in fp64 the reference
    formulas (forward, sums, apply) equal fp64 autograd to 1e-12 (relative to
    the largest magnitude of each output)."""
    B, H, C, eps = 3, 6, 16, 1e-3
    g = torch.Generator().manual_seed(11)
    y = torch.randn(B, H, H, C, generator=g, dtype=torch.float64) * 2 + 0.5
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5) * torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    dP = torch.randn(B, H // 2, H // 2, C, generator=g, dtype=torch.float64)
    M = B * H * H
    yf = y.reshape(-1, C)
    mean = yf.mean(0)
    invstd = ((yf * yf).mean(0) - mean * mean + eps).rsqrt()
    coef = torch.stack([mean, invstd, gamma * invstd, beta - mean * gamma * invstd])
    # fp64 coefficients: the fp32 rounding of z inside pool_select cannot change a tie-free choice
    best, sel = xb.pool_select(y, coef[2], coef[3])
    z = xb.windows(coef[2] * y + coef[3]).clamp_min(0)
    assert int((z == z.max(3, keepdim=True).values).sum(3).max()) == 1 or bool((z.max(3).values == 0).any())
    o, dy_ag, dg_ag, db_ag = _autograd_bn_relu_pool(y, gamma, beta, dP, eps)
    pooled = z.max(3).values
    assert float((pooled - o).abs().max()) <= 1e-12 * float(o.abs().max())
    assert float((best - pooled).abs().max()) <= 2.0 ** -23 * float(pooled.abs().max())
    s_dz, s_dzx, _, _ = xb.bwd_sums_ref(y, dP, coef)
    assert float((s_dz - db_ag).abs().max()) <= 1e-12 * float(db_ag.abs().max())
    assert float((s_dzx - dg_ag).abs().max()) <= 1e-12 * float(dg_ag.abs().max())
    dy, _, _, _ = xb.apply_ref(y, dP, coef, gamma, s_dz, s_dzx, M)
    assert float((dy - dy_ag).abs().max()) <= 1e-12 * float(dy_ag.abs().max())


def test_bn_coefficients_match_torch_running_stats():
    """bn_coefficients (train) equals fp64 F.batch_norm's running statistics
    (unbiased variance) and normalisation; eval mode uses rmean - bias."""
    g = torch.Generator().manual_seed(12)
    B, H, C, eps, mom = 4, 4, 8, 1e-3, 0.1
    y = torch.randn(B, H, H, C, generator=g, dtype=torch.float64) * 3 + 2
    gamma, beta = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    bias = torch.randn(C, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    yf = y.reshape(-1, C)
    M = yf.shape[0]
    sums = torch.stack([yf.sum(0), (yf * yf).sum(0)])
    mom32, eps32 = float(torch.tensor(mom, dtype=torch.float32)), float(torch.tensor(eps, dtype=torch.float32))
    r = xb.bn_coefficients(sums, M, gamma, beta, bias, eps, mom, (rm, rv), 0)
    trm, trv = rm.clone(), rv.clone()
    z = F.batch_norm((y + bias).permute(0, 3, 1, 2), trm, trv, gamma, beta, True, mom32, eps32).permute(0, 2, 3, 1)
    torch.testing.assert_close(r["rmean"], trm, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["rvar"], trv, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["scale"] * y + r["shift"], z, rtol=1e-9, atol=1e-9)
    e = xb.bn_coefficients(None, M, gamma, beta, bias, eps, mom, (rm, rv), 1)
    z = F.batch_norm((y + bias).permute(0, 3, 1, 2), rm, rv, gamma, beta, False, mom32, eps32).permute(0, 2, 3, 1)
    torch.testing.assert_close(e["scale"] * y + e["shift"], z, rtol=1e-9, atol=1e-9)
    assert torch.equal(e["rmean"], rm) and torch.equal(e["rvar"], rv)


def test_integer_inputs_tell_pool_rules_apart():
    """On the exact regime's integer inputs a last-index tie-break and a >= 0
    ReLU test both change dz (so every kernel copy of the rule is pinned), the
    windows hold ties, positive ties and all-nonpositive windows in numbers,
    and the regime's exactness checks pass; dy needs real bf16 roundings."""
    B, H, C = 4, 8, 64
    y, dP, coef, gamma = xb.int_bn_inputs(B, H, C, torch.Generator().manual_seed(1))
    dz, _ = xb.bwd_terms(y, dP, coef, exact_regime=True)
    dz_last, _ = xb.bwd_terms(y, dP, coef, tie="last")
    dz_ge, _ = xb.bwd_terms(y, dP, coef, positive="ge")
    assert int((dz != dz_last).sum()) > 100 and int((dz != dz_ge).sum()) > 100
    best, sel = xb.pool_select(y, coef[2], coef[3])
    r = (coef[2].double() * xb.windows(y.double()) + coef[3].double()).clamp_min(0)
    ties = (r == best.unsqueeze(3)).sum(3) > 1
    assert float(ties.double().mean()) > 0.2 and float((ties & (best > 0)).double().mean()) > 0.05
    assert float((best <= 0).double().mean()) > 0.1
    assert bool((sel[..., 0].sum(3) == 1).all()) and bool(sel[:, :, :, 0, 0].all())  # gamma = 0: position 0 wins
    s_dz, s_dzx, _, _ = xb.bwd_sums_ref(y, dP, coef, exact_regime=True)
    dy, _, _, _ = xb.apply_ref(y, dP, coef, gamma, s_dz, s_dzx, B * H * H, exact_regime=True)
    assert float((dy.float().to(BF16).double() != dy).double().mean()) > 0.1


def test_bn_bounds_hold_for_fp32_arithmetic_and_catch_misrouting():
    """A plain fp32 evaluation of the kernels' formulas stays inside the
    coefficient, sum and dy bounds on the hard channels (negative gamma, a
    constant channel, mean 64 with deviation 1/4); one gradient routed to the
    neighbouring window position, or one dropped item, is outside them."""
    B, H, C, eps, mom = 8, 16, 32, 1e-3, 0.1
    g = torch.Generator().manual_seed(13)
    y = torch.randn(B, H, H, C, generator=g) * 2 + 0.5
    y[..., 1] = 1.5
    y[..., 2] = 64 + 0.25 * torch.randn(B, H, H, generator=g)
    y = y.to(BF16)
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
    beta, bias = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    M = B * H * H
    yf = y.float().reshape(-1, C)
    sums = torch.stack([yf.sum(0), (yf * yf).sum(0)])
    mean = sums[0] / M
    var = (sums[1] / M - mean * mean).clamp_min(0)
    invstd = (var + torch.tensor(eps)).rsqrt()
    sc = gamma * invstd
    coef = torch.stack([mean, invstd, sc, beta - mean * sc])
    rm, rv = torch.zeros(C), torch.ones(C)
    rm2 = (1 - torch.tensor(mom)) * rm + torch.tensor(mom) * (mean + bias)
    rv2 = (1 - torch.tensor(mom)) * rv + torch.tensor(mom) * (var * M / (M - 1))
    xb.assert_coefficients(coef, (rm2, rv2), sums, M, gamma, beta, bias, eps, mom, (rm, rv))
    ref, bnd = xb.bn_coefficient_bounds(sums, M, gamma, beta, bias, eps, mom, (rm, rv))
    assert float(bnd["invstd"][2] / ref["invstd"][2]) < 0.05  # the mean-64 channel: percent, not ulps
    assert float((bnd["invstd"] / ref["invstd"])[3:].max()) < 1e-5
    bad = coef.clone()
    bad[1, 5] *= 1 + 1e-4
    with pytest.raises(AssertionError):
        xb.assert_coefficients(bad, None, sums, M, gamma, beta, bias, eps, mom, (rm, rv))
    # backward in fp32
    dP = torch.randn(B, H // 2, H // 2, C, generator=g).to(BF16)
    dz64, xhat64 = xb.bwd_terms(y, dP, coef)
    dz, yw = dz64.float(), xb.windows(y.float())
    s_dz, s_dzx = dz.sum((0, 1, 2, 3)), (dz * (yw - coef[0]) * coef[1]).sum((0, 1, 2, 3))
    r_dz, r_dzx, a_dz, a_dzx = xb.bwd_sums_ref(y, dP, coef)
    n_pix = B * (H // 2) ** 2
    xb.assert_within(s_dz, r_dz, xb.sums_bound(n_pix, a_dz), "sum dz")
    xb.assert_within(s_dzx, r_dzx, xb.sums_bound(n_pix, a_dzx), "sum dz*xhat")
    drop = s_dz - dz[-1, -1, -1].sum(0)  # the last item of a grid-stride loop left out
    with pytest.raises(AssertionError):
        xb.assert_within(drop, r_dz, xb.sums_bound(n_pix, a_dz), "sum dz")
    a = gamma * coef[1]
    kbi, kc = -a * s_dzx * (1.0 / M) * coef[1], -a * s_dz * (1.0 / M)
    dy = xb.unwindows(a * dz + kbi * (yw - coef[0]) + kc).to(BF16)
    ref_dy, m_a, m_b, m_c = xb.apply_ref(y, dP, coef, gamma, s_dz, s_dzx, M)
    xb.assert_within(dy, ref_dy, xb.apply_bound(ref_dy, m_a, m_b, m_c, 1), "dy")
    sel = dz64 != 0
    b_, i_, j_, c_ = [int(v[0]) for v in torch.nonzero(sel[:, :, :, 0, :] & (dz64[:, :, :, 0, :].abs() > 0.5), as_tuple=True)]
    wrong = xb.windows(dy.float()).clone()
    ka = float(a[c_] * dz[b_, i_, j_, 0, c_])
    wrong[b_, i_, j_, 0, c_] -= ka  # the gradient of one window lands on the next position
    wrong[b_, i_, j_, 1, c_] += ka
    with pytest.raises(AssertionError):
        xb.assert_within(xb.unwindows(wrong).to(BF16), ref_dy, xb.apply_bound(ref_dy, m_a, m_b, m_c, 1), "dy")


def test_head_exact_inputs_and_reference():
    """The head's exact regime holds at the largest shape (representability
    asserted inside), the reference equals fp64 autograd, and dh on those
    inputs is (W[max] - W[label]) / B."""
    g = torch.Generator().manual_seed(14)
    h, w, b, lab, k = xb.head_exact_inputs(128, 4096, g)
    r = xb.head_exact_ref(h, w, b, lab)
    assert bool((r["logits"].argmax(1) == k).all()) and {0, 9} <= set(lab.tolist()) and {0, 9} <= set(k.tolist())
    assert 0.3 < float((lab == k).double().mean()) < 0.7
    assert torch.equal(r["dh"], (w.double()[k] - w.double()[lab]) / 128)
    assert torch.equal(r["loss_b"], r["logits"].max(1).values - r["logits"][torch.arange(128), lab])
    h2 = torch.randn(5, 264, generator=g).to(BF16)
    w2, b2 = torch.randn(10, 264, generator=g) * 0.02, torch.randn(10, generator=g) * 0.1
    lab2 = torch.randint(0, 10, (5,), generator=g)
    r2 = xb.head_ref(h2, w2, b2, lab2)
    hr, wr, br = (t.double().requires_grad_(True) for t in (h2, w2, b2))
    lp = F.log_softmax(F.linear(hr, wr, br), 1)
    F.nll_loss(lp, lab2).backward()
    for got, want in ((r2["logp"], lp), (r2["dh"], hr.grad), (r2["dW"], wr.grad), (r2["db"], br.grad)):
        torch.testing.assert_close(got, want.detach(), rtol=1e-12, atol=1e-14)


# ---------------------------------------------------------------------------
# the update / slab-sum / pack / gather references (tests/kernels/exact_update.py)
# ---------------------------------------------------------------------------
import fractions  # noqa: E402

import numpy as np  # noqa: E402

from tests.kernels import exact_update as xu  # noqa: E402


def _round_fraction_to_f32(q):
    """fp32 nearest (ties to even) to the exact rational q, by integer arithmetic."""
    if q == 0:
        return np.float32(0.0)
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if fractions.Fraction(2) ** e > q:
        e -= 1
    assert fractions.Fraction(2) ** e <= q < fractions.Fraction(2) ** (e + 1)
    e = max(e, -126)  # subnormals share the smallest normal's spacing
    scaled = q / fractions.Fraction(2) ** (e - 23)  # integer part: the 24-bit significand
    n, rest = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rest
    if twice > scaled.denominator or (twice == scaled.denominator and n & 1):
        n += 1
    return np.float32(sign * float(n) * 2.0 ** (e - 23))


def test_fma32_matches_exact_rational_arithmetic():
    rng = np.random.default_rng(7)
    n = 3000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 12, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 12, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    c[::3] = (-a[::3].astype(np.float64) * b[::3]).astype(np.float32)  # cancellation: the low product bits decide
    got = xu.fma32(a, b, c)
    F = fractions.Fraction
    for i in range(n):
        want = _round_fraction_to_f32(F(float(a[i])) * F(float(b[i])) + F(float(c[i])))
        assert got[i].view(np.uint32) == want.view(np.uint32), (i, a[i], b[i], c[i], got[i], want)


def test_fma32_double_rounding_case():
    """a = b = 1 + 2^-12, c = 2^-60: a b = 1 + 2^-11 + 2^-24, an fp32 tie between
    1 + 2^-11 (even) and 1 + 2^-11 + 2^-23; c lifts it just above, so the one
    rounding goes up.  fp64(a b + c) loses c, and its fp32 rounding ties to
    even: down.  Mirrored below the tie with -c."""
    a = np.float32(1 + 2.0 ** -12)
    c = np.float32(2.0 ** -60)
    up, down = np.float32(1 + 2.0 ** -11 + 2.0 ** -23), np.float32(1 + 2.0 ** -11)
    assert xu.fma32(a, a, c) == up
    assert np.float32(np.float64(a) * np.float64(a) + np.float64(c)) == down  # the rejected reference
    assert xu.fma32(a, a, -c) == down
    # an odd neighbour: a b = 1 + 3 2^-12 + ... chosen so that the tie's even side is up
    a2, b2 = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -11 + 2.0 ** -12)
    exact = fractions.Fraction(float(a2)) * fractions.Fraction(float(b2))
    for cc in (c, -c):
        want = _round_fraction_to_f32(exact + fractions.Fraction(float(cc)))
        assert xu.fma32(a2, b2, cc) == want


@pytest.mark.parametrize("mu", [None, 0.5, 0.75])
@pytest.mark.parametrize("count", [1, 2, 4])
def test_sgd_ref_exact_regime_is_the_fp64_formula(mu, count):
    rng = np.random.default_rng(11)
    n = 4096
    p, m = (rng.integers(-64, 65, n).astype(np.float32) for _ in range(2))
    g = rng.integers(-64 * 129, 64 * 129 + 1, n).astype(np.float32)  # up to a 129-split sum of such integers
    m = None if mu is None else m
    s = xu.participation_scale(count)
    assert float(s) == 1.0 / count
    got_p, got_m = xu.sgd_ref(p, g, m, s, 2.0 ** -3, 2.0 ** -2, mu or 0.0)
    want_p, want_m = xu.sgd_formula64(p, g, m, count, 2.0 ** -3, 2.0 ** -2, mu or 0.0)
    assert np.array_equal(got_p.astype(np.float64), want_p)
    assert (got_m is None) == (want_m is None)
    if got_m is not None:
        assert np.array_equal(got_m.astype(np.float64), want_m)


def test_participation_scale():
    assert xu.participation_scale(1.0) == 1.0 and xu.participation_scale(0.0) == 1.0
    third = xu.participation_scale(3.0)
    assert third.dtype == np.float32 and third == np.float32(1.0 / 3.0)
    assert third.view(np.uint32) == 0x3EAAAAAB


@pytest.mark.parametrize("splits", sorted(set(xu.INPLACE_SPLITS + xu.TAIL_SPLITS)))
def test_slab_sum_ref_integer_slabs(splits):
    rng = np.random.default_rng(splits)
    slabs = rng.integers(-64, 65, (splits, 40)).astype(np.float32)
    for tpo in {xu.slab_tpo(splits), 8 if 8 <= splits < 32 else xu.slab_tpo(splits)}:
        got = xu.slab_sum_ref(slabs, tpo)
        assert np.array_equal(got.astype(np.int64), slabs.astype(np.int64).sum(0))


def test_slab_tpo_thresholds():
    assert [xu.slab_tpo(k) for k in (1, 7, 8, 31, 32, 129)] == [1, 1, 8, 8, 32, 32]


def test_slab_sum_ref_order_is_told_apart():
    """On real data the lane order matters: blocked instead of strided lanes,
    an ascending butterfly and a plain sequential sum all differ somewhere."""
    rng = np.random.default_rng(3)
    slabs = rng.standard_normal((25, 4096)).astype(np.float32)
    want = xu.slab_sum_ref(slabs, 8)

    def lanes(parts, orders):
        for o in orders:
            parts = [xu.add32(parts[t], parts[t ^ o]) for t in range(8)]
        return parts[0]

    def part(idx):
        acc = np.zeros(slabs.shape[1], np.float32)
        for sp in idx:
            acc = xu.add32(acc, slabs[sp])
        return acc

    strided = [part(range(t, 25, 8)) for t in range(8)]
    assert np.array_equal(lanes(strided, (4, 2, 1)), want)
    # the spelled-out association
    p = strided
    spelled = xu.add32(xu.add32(xu.add32(p[0], p[4]), xu.add32(p[2], p[6])),
                       xu.add32(xu.add32(p[1], p[5]), xu.add32(p[3], p[7])))
    assert np.array_equal(spelled, want)
    blocked = [part(range(4 * t, min(4 * t + 4, 25))) for t in range(8)]  # 7 lanes of 4 (the last: 1), sequential
    assert not np.array_equal(lanes(blocked, (4, 2, 1)), want)
    assert not np.array_equal(lanes(strided, (1, 2, 4)), want)
    assert not np.array_equal(xu.slab_sum_ref(slabs, 1), want)
    # ... and all agree to rounding
    assert np.allclose(xu.slab_sum_ref(slabs, 1), want, rtol=0, atol=1e-4)


@pytest.mark.parametrize("geom", xu.TAIL_GEOMS + [(4, 25, 8, 3), (4, 25, 16, 3)], ids=str)
def test_pack1_index_ref_partitions_the_packed_buffer(geom):
    cout, taps, cp, c = geom
    e = np.arange(cout * taps * c)
    idx = xu.pack1_index_ref(e, c, cp)
    size = xu.pack1_size(cout, taps, cp)
    assert idx.min() >= 0 and idx.max() < size
    assert len(np.unique(idx)) == len(e)  # injective
    pads = np.setdiff1d(np.arange(size), idx)
    assert len(pads) + len(e) == size
    if cp > 0:
        assert np.array_equal(idx, (e // c) * cp + e % c)
        assert np.all(pads % cp >= c)
    else:
        kw = -cp
        pos = pads % 8  # within a 16-byte pair chunk: [2][4]
        chunk = (pads // 8) % ((kw + 1) // 2)
        # a pad is a channel past C, or the second half of an odd row's last chunk
        assert np.all((pos % 4 >= c) | ((kw % 2 == 1) & (chunk == kw // 2) & (pos >= 4)))
        # horizontally adjacent taps (kx even, kx + 1) of one row share a chunk
        w = e.reshape(cout, kw, kw, c)
        i4 = idx.reshape(cout, kw, kw, c)
        assert w.shape == i4.shape
        for kx in range(0, kw - 1, 2):
            assert np.array_equal(i4[:, :, kx + 1, :], i4[:, :, kx, :] + 4)
            assert np.array_equal(i4[:, :, kx, 0] % 8, np.zeros_like(i4[:, :, kx, 0]))


def test_bf16_integer_rounding_is_torchs():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(20000) * 2.0 ** rng.integers(-20, 20, 20000)).astype(np.float32)
    ties = (np.arange(0x3F80, 0x3F80 + 512, dtype=np.uint32) << 16 | 0x8000).view(np.float32)  # exactly half way
    near = np.concatenate([(ties.view(np.uint32) + 1).view(np.float32), (ties.view(np.uint32) - 1).view(np.float32)])
    special = np.array([0.0, -0.0, np.inf, -np.inf, 3.3895314e38, 1e-40], dtype=np.float32)
    for v in (x, ties, -ties, near, special):
        want = torch.from_numpy(v.copy()).to(BF16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(xu.bf16_bits(v), want)
    # NaN stays NaN in both (the payload is the implementation's: torch's differs between its own code paths)
    nans = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)
    for got in (xu.bf16_bits(nans), torch.from_numpy(nans.copy()).to(BF16).view(torch.int16).numpy().view(np.uint16)):
        assert np.all((got & 0x7FFF) > 0x7F80)
    assert np.array_equal(xu.bf16_widen(xu.bf16_bits(ties)).view(np.uint32) & 0x10000, np.zeros(512, np.uint32))  # even
    # one rounding from fp64 agrees wherever fp32 holds the value
    assert np.array_equal(xu.bf16_round64(x.astype(np.float64)), xu.bf16_widen(xu.bf16_bits(x)).astype(np.float64))


def test_gather_reference_and_exemption_cap():
    from torch_distlearn_amd.data import CIFAR_MEAN, CIFAR_STD

    u = np.arange(256, dtype=np.uint8)
    img = np.broadcast_to(u[None, :, None, None], (1, 256, 1, 3)).copy()  # every (value, channel) pair
    x64, lab = xu.gather_ref(img, [0], np.array([9]), 0, 1, CIFAR_MEAN, CIFAR_STD)
    assert x64.shape == (1, 256, 1, 3) and lab.tolist() == [9]
    want = (u[:, None] / 255.0 - np.float32(CIFAR_MEAN).astype(np.float64)) / np.float32(CIFAR_STD).astype(np.float64)
    assert np.array_equal(x64.reshape(256, 3), want)
    lo, hi, exempt = xu.gather_allowed(x64, CIFAR_MEAN, CIFAR_STD)
    assert int(exempt.sum()) <= 8, int(exempt.sum())
    assert np.all(hi[~exempt] == xu.bf16_round64(x64)[~exempt])
    # the exempt pairs' two candidates are adjacent bf16 values around a boundary
    assert np.all(lo[exempt] < hi[exempt])
    # a plain fp32 evaluation (uncontracted and fma-contracted) lands on an allowed value everywhere
    r, q = np.float32(1.0 / 255.0), (np.float64(1.0) / np.float32(CIFAR_STD).astype(np.float64)).astype(np.float32)
    uf = img.astype(np.float32)
    mean = np.broadcast_to(np.float32(CIFAR_MEAN), uf.shape)
    for d in (xu.add32(xu.mul32(uf, r), -mean), xu.fma32(uf, r, -mean)):
        y = xu.bf16_widen(xu.bf16_bits(xu.mul32(d, np.broadcast_to(q, uf.shape)))).astype(np.float64)
        assert np.all((y == lo) | (y == hi))
    # the sample index in Python integers: a 32-bit product picks other samples
    order = list(range(7))
    step = 2 ** 33 + 5
    assert xu.gather_samples(order, step, 3) == [(step * 3 + b) % 7 for b in range(3)]
    assert xu.gather_samples(order, step, 3) != [(((step * 3) & 0xFFFFFFFF) + b) % 7 for b in range(3)]
    assert xu.gather_samples(order, 2, 3) == [6, 0, 1]  # wraps the ring in the middle of the batch


def test_slab_sum_lane_rotation_is_the_same_sum():
    """Which lane a split lands in matters only up to the butterfly's symmetry:
    rotating the assignment (split u into lane (u + k) mod 8) or xor-ing it
    with a constant keeps every pair {t, t ^ 4}, every quad and so -- fp32
    addition being commutative -- every bit.  A test cannot tell such an edit
    from the original, and need not.  Halving the lanes (u mod 4) or
    exchanging two lanes that are not partners is a different sum."""
    rng = np.random.default_rng(9)
    slabs = rng.standard_normal((25, 4096)).astype(np.float32)
    want = xu.slab_sum_ref(slabs, 8)

    def tree(lane_of):
        parts = [np.zeros(slabs.shape[1], np.float32) for _ in range(8)]
        for sp in range(slabs.shape[0]):
            t = lane_of(sp % 8)
            parts[t] = xu.add32(parts[t], slabs[sp])
        for o in (4, 2, 1):
            parts = [xu.add32(parts[t], parts[t ^ o]) for t in range(8)]
        return parts[0]

    for k in range(1, 8):
        assert np.array_equal(tree(lambda u: (u + k) % 8), want)
        assert np.array_equal(tree(lambda u: u ^ k), want)
    assert not np.array_equal(tree(lambda u: u % 4), want)
    assert not np.array_equal(tree(lambda u: {1: 2, 2: 1}.get(u, u)), want)


# --------------------------------------------------------------------------- tests/kernels/exact_nhwc.py
from tests.kernels import exact_nhwc as xn  # noqa: E402


@pytest.mark.parametrize("relu,with_res", [(False, False), (True, False), (True, True)])
def test_nhwc_bn_formulas_match_autograd(relu, with_res):
    """bn_train64 (built from bn_bwd_sums / bn_dx64, the references of the
    channels-last BN tests) against fp64 autograd of F.batch_norm, to 1e-12."""
    g = torch.Generator().manual_seed(3)
    M, Cc, eps = 77, 16, 1e-3
    x = torch.randn(M, Cc, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Cc, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Cc, generator=g, dtype=torch.float64, requires_grad=True)
    res = torch.randn(M, Cc, generator=g, dtype=torch.float64, requires_grad=True) if with_res else None
    dy = torch.randn(M, Cc, generator=g, dtype=torch.float64)
    z = F.batch_norm(x, None, None, w, b, True, 0.1, eps)
    z = z + res if with_res else z
    y = z.relu() if relu else z
    y.backward(dy)
    r = xn.bn_train64(x, w, b, eps, dy, relu, res)
    for k, want in (("y", y), ("dx", x.grad), ("dw", w.grad), ("db", b.grad)):
        assert float((r[k] - want.detach()).abs().max()) < 1e-12, k
    if with_res:
        assert float((r["dres"] - res.grad).abs().max()) < 1e-12


@pytest.mark.parametrize("K,S,P", [(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 3, 1), (5, 2, 2), (1, 1, 0)])
@pytest.mark.parametrize("H,W", [(7, 5), (8, 10), (2, 3)])
def test_nhwc_pool_reference_matches_torch(K, S, P, H, W):
    """pool_fwd_ref's values and argmax bytes against F.max_pool2d's indices
    (tied windows included), and pool_bwd_ref against autograd for integer dy."""
    g = torch.Generator().manual_seed(H * 100 + K)
    x = (torch.randint(-4, 5, (2, H, W, 8), generator=g).float() / 2)
    y, arg = xn.pool_fwd_ref(x, K, S, P)
    xt = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    yt, it = F.max_pool2d(xt, K, S, P, return_indices=True)
    assert np.array_equal(y, yt.detach().permute(0, 2, 3, 1).float().numpy())
    assert np.array_equal(xn.pool_arg_to_flat(arg, H, W, K, S, P), it.permute(0, 2, 3, 1).numpy())
    dy = torch.randint(-8, 9, tuple(y.shape), generator=g).float()
    yt.backward(dy.permute(0, 3, 1, 2).double())
    assert np.array_equal(xn.pool_bwd_ref(dy, arg, H, W, K, S, P), xt.grad.permute(0, 2, 3, 1).float().numpy())
    if K > 1:  # the last-maximum rule picks other bytes on these tied windows
        assert not np.array_equal(xn.pool_fwd_ref(x, K, S, P, tie="last")[1], arg)


def test_nhwc_pool_backward_order_matters():
    """Real dy: pool_bwd_ref adds in fp32, oh ascending then ow ascending; the
    reverse order differs in at least one element of a 3x3 / 1 pool, so the
    bitwise comparison pins the order."""
    g = torch.Generator().manual_seed(1)
    x = torch.zeros(1, 6, 6, 8)  # all tied: every window picks tap 0, so pixel (h, w) collects window (h + 1, w + 1) only
    x[0, 2, 2] = 5.0             # ... except around the peak, which 9 windows choose
    _, arg = xn.pool_fwd_ref(x, 3, 1, 1)
    # (a few bf16 values of one magnitude add exactly in fp32: the order shows only across a wide range)
    dy = (torch.randn(1, 6, 6, 8, generator=g) * torch.pow(2.0, torch.randint(-14, 15, (1, 6, 6, 8), generator=g))).bfloat16()
    ref = xn.pool_bwd_ref(dy, arg, 6, 6, 3, 1, 1)
    d = xn.np32(dy)[0, 1:4, 1:4].reshape(9, 8)
    fwd = np.zeros(8, np.float32)
    rev = np.zeros(8, np.float32)
    for i in range(9):
        fwd = xu.add32(fwd, d[i])
        rev = xu.add32(rev, d[8 - i])
    assert np.array_equal(ref[0, 2, 2], fwd) and not np.array_equal(fwd, rev)


def test_nhwc_wrong_rules_are_told_apart():
    """The >= 0 ReLU decision and an unrounded residual BN differ from the
    correct rule on the inputs the GPU tests use."""
    g = torch.Generator().manual_seed(7)
    d = xn.int_bn_bwd_inputs(300, 16, g)
    sc, sh = xn.coef_from_save(d["save"], d["w"], d["b"])
    gt, ge = xn.relu_mask(2, d["x"], sc, sh), xn.relu_mask(2, d["x"], sc, sh, positive="ge")
    assert (gt != ge).any() and not (gt & ~ge).any()
    sg, _ = xn.bn_bwd_sums(xb.cpu64(d["dy"]) * torch.from_numpy(gt), d["x"], d["save"], exact_regime=True)
    sw, _ = xn.bn_bwd_sums(xb.cpu64(d["dy"]) * torch.from_numpy(ge), d["x"], d["save"])
    assert not torch.equal(sg, sw)
    x, res = torch.randn(300, 16, generator=g).bfloat16(), torch.randn(300, 16, generator=g).bfloat16()
    one = np.ones(16, np.float32)
    rsc, rsh = (torch.randn(16, generator=g).numpy() for _ in range(2))
    a = xn.bn_fwd_ref(x, one, 0 * one, True, res, rsc, rsh)
    bnr = xn.bn_fwd_ref(x, one, 0 * one, True, res, rsc, rsh, round_res=False)
    assert not np.array_equal(a, bnr)
    # mask bits: bit k of byte (m, j) is channel 8 j + k
    y = np.zeros((2, 16), np.float32)
    y[1, 9] = 2.0
    assert xn.mask_bits_ref(y).tolist() == [[0, 0], [0, 2]] and xn.unpack_bits(xn.mask_bits_ref(y), 16)[1, 9]


def test_nhwc_bounds_reject_a_dropped_row_and_a_swapped_tap():
    """A plain fp32 evaluation of dx stays inside the derived bound; the same
    with one row left out of the sums' input, or the statistics of M - 1 rows,
    does not.  The stem unpack index with its parity bits exchanged moves taps."""
    g = torch.Generator().manual_seed(11)
    M, Cc = 333, 16
    x, dy = torch.randn(M, Cc, generator=g).bfloat16(), torch.randn(M, Cc, generator=g).bfloat16()
    w = torch.randn(Cc, generator=g)
    s = xn.bn_stats64(x) / M
    save = torch.cat([s[0], (s[1] - s[0] ** 2 + 1e-3).rsqrt()]).float()
    sums, sabs = xn.bn_bwd_sums(dy, x, save)
    acc32 = torch.stack([dy.float().sum(0), (dy.float() * ((x.float() - save[:Cc]) * save[Cc:])).sum(0)])
    bound = xn.bwd_sums_bound(M, sabs)
    assert bool(((acc32.double() - sums).abs() <= bound).all())
    dropped = xn.bn_bwd_sums(dy[:-1], x[:-1], save)[0]
    assert bool(((dropped - sums).abs() > bound).any())
    ref, E = xn.bn_dx64(dy, x, save, w, acc32, M)
    a = w * save[Cc:]
    got = (a * (dy.float() - acc32[0] / M - (x.float() - save[:Cc]) * save[Cc:] * (acc32[1] / M))).bfloat16()
    xb.assert_within(got, ref, xn.bf16_bound(ref, E), "fp32 dx")
    with pytest.raises(AssertionError):
        xb.assert_within(got[torch.randperm(M, generator=g)], ref, xn.bf16_bound(ref, E), "permuted rows")
    # statistics: exact sums of M rows vs M - 1 rows
    xi = exact.int_bf16((M, Cc), -4, 4, generator=g)
    with pytest.raises(AssertionError):
        exact.assert_exact(xn.bn_stats64(xi[:-1]).float(), xn.bn_stats_exact(xi), "a dropped row")
    # the swapped stem tap
    k, kw = xn.stem_unpack_index(), xn.stem_unpack_index(swap_parity=True)
    assert len(set(k.reshape(-1).tolist())) == 147 and (k != kw).any()
    slab = torch.arange(2 * 256).reshape(1, 2, 256).float()
    dw0 = torch.zeros(2, 3, 7, 7)
    assert not np.array_equal(xn.stem_unpack_ref(slab, dw0), xn.stem_unpack_ref(slab, dw0, swap_parity=True))
    # ... and the layouts invert each other: packing a 7x7 weight and reading it back through the unpack index
    w7 = torch.randn(2, 3, 7, 7, generator=g).bfloat16()
    assert np.array_equal(xn.stem_pack_ref(w7).reshape(2, 256)[:, k], xn.np32(w7))


def test_nhwc_geometry_model_and_layout_references():
    """bn_loops on hand-worked shapes (C = 64: RPI = 32), s2d against a direct
    loop, phase blocks against the documented taps."""
    assert xn.bn_geom(1, 64) == {"CVB": 8, "RPI": 32, "rpb": 32, "rb": 1, "groups": 1}
    assert xn.bn_loops(1, 64) == {"rem_only", "idle", "small"}
    assert xn.bn_loops(4 * 32 + 1, 64) == {"u+1", "idle"}
    assert xn.bn_loops(16 * 32 + 5, 64) == {"u+1", "u+3", "idle", "blocks"}
    assert xn.bn_geom(16 * 32 + 5, 64)["rpb"] == 9 * 32 and "groups" in xn.bn_loops(8, 512)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 5, 6, 3, generator=g).bfloat16()
    S = xn.s2d_ref(x, 6, 6, 3)
    for i, j, a, b, c in [(0, 0, 0, 0, 0), (1, 1, 1, 1, 2), (2, 3, 1, 0, 1), (3, 4, 0, 1, 0), (5, 5, 1, 1, 1)]:
        yy, xx = 2 * i + a - 3, 2 * j + b - 3
        want = float(x[0, yy, xx, c]) if 0 <= yy < 5 and 0 <= xx < 6 else 0.0
        assert float(S[0, i, j, (a * 2 + b) * 3 + c]) == want
    wt = torch.arange(2 * 9 * 8).reshape(2, 3, 3, 8).float()
    ph = xn.phase_ref(wt)
    assert ph[:8].tolist() == wt[0, 1, 1].tolist() and ph[2 * 8 + 8:2 * 8 + 16].tolist() == wt[0, 1, 2].tolist()
    assert ph.size == 9 * 2 * 8
    h = torch.randn(2, 50, 8, generator=g).bfloat16()
    f = xn.head_pool_ref(h)
    assert float(np.abs(f - xn.np32(h).astype(np.float64).mean(1)).max()) < 2.0 ** -8


def test_nhwc_out_row_corrections():
    """Which image sizes make out_row's float-reciprocal divisions come out one
    too small (plain fp32 arithmetic): the GPU tests rely on 5 x 11 and 3 x 41."""
    assert xn.out_row_corrections(5, 11, 165) == (True, False)
    assert xn.out_row_corrections(3, 41, 246) == (True, True)
    for H, W in ((1, 1), (3, 5), (7, 7), (13, 9), (56, 56)):
        assert xn.out_row_corrections(H, W, 4 * H * W) == (False, False)
    assert xn.out_row_corrections(57, 59, 4988 * 57 * 59) == (False, False)
