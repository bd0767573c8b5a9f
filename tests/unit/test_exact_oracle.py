"""The exact-integer / per-element oracles of tests/kernels/exact.py catch what
the whole-tensor Frobenius ratio of the older conv tests lets through.

A correct result is computed on the CPU (fp32 accumulation of exact bf16
products, two K slabs, one bf16 rounding), then mutated the way a kernel goes
wrong: a border tap skipped at one pixel, a lost store lane, a wrong last row
of the M tail, truncation instead of round-to-nearest-even, a split-K slab
rounded through bf16, two output rows swapped.  Every mutation must raise under
the oracle; the ratio of the old check is recorded for the ones it misses."""
import functools

import pytest
import torch

from tests.kernels import exact

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
