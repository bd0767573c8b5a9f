"""The launch that turns gradients into parameters -- the fused SGD update
(flat_ops.hip, sgd_dev.h), the split-K slab sums it consumes in place and in
its tail blocks (slab_reduce_dev.h), the reduce-only launch, the side jobs a
conv launch carries, the next-step preparation riding the update (prep_dev.h)
and the elastic-averaging kernels -- against the references of
tests/kernels/exact_update.py, bit for bit.

Exact regime: integers |v| <= 64 and dyadic constants (wd 2^-3, lr 2^-2,
mu 0.5 / 0.75, count 1 / 2 / 4): every intermediate is an fp32 number, the
reference is checked against the fp64 formula in each case, and a difference
is a wrong operand, index, range or scale.  Real regime: randn data, a rate
with a full mantissa, wd 1e-4, mu 0.9, count 3 (s = fp32(1/3)): bitwise
against the emulated fmas and the spelled-out summation order.  Only the
gather's normalisation has an exemption (exact_update.gather_allowed), and
its cap is asserted.

Every output buffer starts from a sentinel or a known state, and everything a
launch must not touch is compared bitwise with what it held before; gradient
elements the launch must take from slabs hold NaN, as do the slabs' pads."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.kernels import exact_update as xu

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
F32 = np.float32
NAN = np.float32("nan")
GRID_CAP, BLOCK = 2048, 256
# 4 elements; two ragged blocks; the smallest size at which a thread of the capped
# grid (dl_common.h stream_grid) takes its second float4: 8 MiB per buffer
SIZES = [4, 4 * 257, 4 * (GRID_CAP * BLOCK + 257)]
REGIMES = ["exact", "real"]
SH_SENT = 0x4110  # bf16 9.0: the shadow's sentinel
W1_SENT = 0xC0E0  # bf16 -7.0: the packed operand's sentinel


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from torch_distlearn_amd import _native

    return _native.native()


_KEEP = []  # the kernels get raw pointers: device tensors must outlive the launch


@pytest.fixture(autouse=True)
def _release():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _KEEP.clear()


@pytest.fixture(scope="module", autouse=True)
def _release_module():
    yield
    _CONV.clear()
    _KEEP.clear()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _d(a):
    """numpy array -> device tensor (uint16 arrays become bf16)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        t = torch.from_numpy(a.view(np.int16)).cuda().view(BF16)
    else:
        t = torch.from_numpy(a).cuda()
    _KEEP.append(t)
    return t


def _h(t):
    """device tensor -> numpy (bf16 as uint16 bit patterns)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == BF16 else t.numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_bits(got, want, what):
    """Bitwise equality (NaN payloads and the sign of zero included)."""
    got = _h(got) if isinstance(got, torch.Tensor) else got
    g, w = _bits(got).reshape(-1), _bits(np.asarray(want)).reshape(-1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero(g != w)[0]
    if bad.size:
        i = int(bad[0])
        gv, wv = np.asarray(got).reshape(-1)[i], np.asarray(want).reshape(-1)[i]
        raise AssertionError(f"{what}: {bad.size} of {g.size} elements differ; first at {i}, last at {int(bad[-1])}: "
                             f"got {gv!r} ({int(g[i]):#x}) want {wv!r} ({int(w[i]):#x})")


def _rate():
    from torch_distlearn_amd.schedules import as_fp32

    return as_fp32(0.0123)  # not a power of two: every mantissa bit of the rate matters


class State:
    """p / g / momentum / shadow of one update in one regime, the slabs that
    replace parts of g, and the expected result."""

    def __init__(self, n, regime, mom, shadow, seed, count=None, mu=None, g16=False):
        self.n, self.regime, self.rng = n, regime, np.random.default_rng(seed)
        if regime == "exact":
            self.wd, self.lr, self.mu, self.count = 2.0 ** -3, 2.0 ** -2, mu or 0.75, 2 if count is None else count
            assert self.mu in (0.5, 0.75) and self.count in (1, 2, 4)
        else:
            self.wd, self.lr, self.mu, self.count = 1e-4, _rate(), 0.9, 3 if count is None else count
        self.s = xu.participation_scale(self.count)
        self.p0, self.g = self.draw(n), self.draw(n)
        self.m0 = self.draw(n) if mom else None
        self.g16 = g16
        if g16:  # the bf16 wire copy of the gradient (integers up to 64 are bf16 numbers)
            self.gbits = xu.bf16_bits(self.g)
            self.g = xu.bf16_widen(self.gbits)
        self.geff = self.g.copy()  # what the update must use as the gradient
        self.has_shadow = shadow
        self.offs, self.lens, self.slabs, self.splits = [], [], [], []
        self.tail, self.tail_slab = [], None
        self.d = None

    def draw(self, *shape):
        if self.regime == "exact":
            return self.rng.integers(-64, 65, shape).astype(F32)
        return self.rng.standard_normal(shape).astype(F32)

    def add_range(self, off, ln, splits):
        """An in-place range: [splits][ln] slabs replace g[off, off + ln)."""
        data = self.draw(splits, ln)
        self.g[off:off + ln] = NAN  # never read
        self.geff[off:off + ln] = xu.slab_sum_ref(data, 8 if splits >= 8 else 1)
        self.offs.append(off), self.lens.append(ln), self.slabs.append(_d(data)), self.splits.append(splits)
        return data

    def set_tail(self, off, geom, splits):
        """The tail range: [splits] slabs in the padded / pair-packed layout
        (pads NaN) replace g[off, off + Cout taps C)."""
        cout, taps, cp, c = geom
        total = cout * taps * c
        data = self.draw(splits, total)
        slab = np.full((splits, xu.pack1_size(cout, taps, cp)), NAN, dtype=F32)
        slab[:, xu.pack1_index_ref(np.arange(total), c, cp)] = data
        self.g[off:off + total] = NAN
        self.geff[off:off + total] = xu.slab_sum_ref(data, xu.slab_tpo(splits))
        self.tail, self.tail_slab = [off, total, splits, cout, taps, cp, c], _d(slab)
        return data

    def upload(self):
        d = {"p": _d(self.p0), "g": _d(self.gbits if self.g16 else self.g),
             "m": None if self.m0 is None else _d(self.m0),
             "sh": _d(np.full(self.n, SH_SENT, np.uint16)) if self.has_shadow else None,
             "slot": _d(np.array([self.count], F32))}
        self.d = d
        return d

    def ptrs(self):
        d = self.d
        return (d["p"].data_ptr(), d["g"].data_ptr(), 0 if d["m"] is None else d["m"].data_ptr(),
                0 if d["sh"] is None else d["sh"].data_ptr(), d["slot"].data_ptr(), self.lr, self.mu, self.wd)

    def slab_args(self):
        return (self.offs, self.lens, [t.data_ptr() for t in self.slabs], self.splits)

    def update_slabs(self, C, skip=(0, 0), next_prep=None):
        if self.d is None:
            self.upload()
        C.sgd_update_slabs(*self.ptrs(), self.n, *self.slab_args(), self.tail,
                           0 if self.tail_slab is None else self.tail_slab.data_ptr(), skip[0], skip[1], _s(), 0,
                           next_prep)
        torch.cuda.synchronize()

    def expected(self, lo=0, hi=None, skip=None):
        """(p, m, shadow bits) after the update of [lo, hi) minus skip."""
        hi = self.n if hi is None else hi
        live = np.zeros(self.n, bool)
        live[lo:hi] = True
        if skip is not None and skip[1] > skip[0]:
            live[skip[0]:skip[1]] = False
        g = np.where(live, self.geff, F32(0))
        assert not np.isnan(g).any()
        pn, mn = xu.sgd_ref(self.p0, g, self.m0, self.s, self.wd, self.lr, self.mu)
        if self.regime == "exact":  # the regime proves itself: the fp64 formula in any order
            p64, m64 = xu.sgd_formula64(self.p0, g, self.m0, self.count, self.wd, self.lr, self.mu)
            assert np.array_equal(pn.astype(np.float64), p64)
            assert mn is None or np.array_equal(mn.astype(np.float64), m64)
        p = np.where(live, pn, self.p0)
        m = None if self.m0 is None else np.where(live, mn, self.m0)
        sh = np.where(live, xu.bf16_bits(pn), np.uint16(SH_SENT)) if self.has_shadow else None
        return p, m, sh

    def check(self, what, lo=0, hi=None, skip=None):
        p, m, sh = self.expected(lo, hi, skip)
        assert_bits(self.d["p"], p, f"{what}: p")
        if m is not None:
            assert_bits(self.d["m"], m, f"{what}: momentum")
        if sh is not None:
            assert_bits(self.d["sh"], sh, f"{what}: bf16 shadow")
            # the integer rounding rule against the framework's own cast of the device result
            assert torch.equal(self.d["sh"].cpu()[sh != SH_SENT], self.d["p"].cpu().to(BF16)[sh != SH_SENT])
        assert_bits(self.d["g"], self.gbits if self.g16 else self.g, f"{what}: the gradient is only read")
        assert float(self.d["slot"]) == self.count
        return p


# --------------------------------------------------------------------------- A: sgd_update / sgd_update_g16
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("g16", [False, True], ids=["fp32grad", "bf16grad"])
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("mom", [False, True])
@pytest.mark.parametrize("regime", REGIMES)
def test_sgd_update_bitwise(C, regime, mom, shadow, g16, n):
    count = {4: 1, 4 * 257: 2}.get(n, 4)  # exact regime: each scale once
    st = State(n, regime, mom, shadow, n + 7 * mom + 3 * shadow, count=count if regime == "exact" else 3,
               mu=0.5 if shadow else 0.75, g16=g16)
    st.upload()
    (C.sgd_update_g16 if g16 else C.sgd_update)(*st.ptrs(), n, _s())
    torch.cuda.synchronize()
    p = st.check(f"sgd_update {regime} n={n}")
    assert not np.array_equal(p, st.p0)


@pytest.mark.parametrize("count", [0.0, 1.0, 3.0, 5.0])
def test_sgd_update_participation_scale(C, count):
    """Real regime at 1 and at n > 1 participants: if only the latter differed
    in the last bit of s, the device division would not be correctly rounded."""
    st = State(4 * 257, "real", True, True, 31, count=count)
    st.upload()
    C.sgd_update(*st.ptrs(), st.n, _s())
    torch.cuda.synchronize()
    st.check(f"count {count}")


# --------------------------------------------------------------------------- B: in-place slab ranges
@pytest.mark.parametrize("splits", xu.INPLACE_SPLITS)
@pytest.mark.parametrize("regime", REGIMES)
def test_slab_range_splits(C, regime, splits):
    """One range of 4 * 257 floats (two ragged blocks) inside a buffer whose
    other elements take g."""
    st = State(4 * 300, regime, splits % 2 == 1, True, splits,
               count=(4 if splits % 2 else 2) if regime == "exact" else None, mu=0.5)
    st.add_range(4 * 3, 4 * 257, splits)
    st.update_slabs(C)
    st.check(f"{splits} splits {regime}")


@pytest.mark.parametrize("mom,shadow", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("regime", REGIMES)
def test_four_slab_ranges_with_gaps(C, regime, mom, shadow):
    st = State(4 * 700, regime, mom, shadow, 41 + mom + 2 * shadow)
    for off, ln, sp in ((8, 4, 5), (40, 256, 8), (400, 4 * 257, 17), (1600, 1028, 31)):
        st.add_range(off, ln, sp)
    st.update_slabs(C)
    st.check(f"four ranges {regime}")


@pytest.mark.parametrize("regime", REGIMES)
def test_slab_ranges_at_both_ends(C, regime):
    n = 4 * 300
    st = State(n, regime, True, True, 43)
    st.add_range(0, 4 * 33, 9)
    st.add_range(n - 4 * 65, 4 * 65, 4)
    st.update_slabs(C)
    st.check(f"ranges at the ends {regime}")
    # ... and one range that is the whole buffer
    st = State(4 * 257, regime, False, True, 44)
    st.add_range(0, 4 * 257, 25)
    st.update_slabs(C)
    st.check(f"whole-buffer range {regime}")


def test_slab_range_limits_throw(C):
    st = State(4 * 300, "exact", True, True, 45)
    st.add_range(16, 64, 32)  # 32 splits: the in-place sum has no 32-lane form
    with pytest.raises(RuntimeError, match="1..31 splits"):
        st.update_slabs(C)
    st.check("32 splits rejected", 0, 0)
    st = State(4 * 300, "exact", True, True, 46)
    for k in range(5):
        st.add_range(16 + 80 * k, 64, 2)
    with pytest.raises(RuntimeError, match="up to 4"):
        st.update_slabs(C)
    st.check("a fifth range rejected", 0, 0)


# --------------------------------------------------------------------------- C: the tail
_TAIL_CASES = ([(g, k) for g in (xu.TAIL_GEOMS[1], xu.TAIL_GEOMS[2]) for k in xu.TAIL_SPLITS] +
               [(g, k) for g in (xu.TAIL_GEOMS[0], xu.TAIL_GEOMS[3], xu.TAIL_GEOMS[4]) for k in (5, 25, 40)] +
               [(xu.TAIL_GEOMS[5], 33)])  # 4800 blocks wanted, 4096 given: slab_reduce_each<32> loops


@pytest.mark.parametrize("geom,splits", _TAIL_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("regime", REGIMES)
def test_tail(C, regime, geom, splits):
    cout, taps, cp, c = geom
    total = cout * taps * c
    off = 8
    st = State(off + total + 12, regime, splits % 2 == 1, True, 100 + splits + total,
               count=(1, 2, 4)[splits % 3] if regime == "exact" else None, mu=0.75)
    st.set_tail(off, geom, splits)
    st.update_slabs(C)
    st.check(f"tail {geom} x {splits} {regime}")


@pytest.mark.parametrize("mom,shadow", [(False, False), (True, True)])
@pytest.mark.parametrize("regime", REGIMES)
def test_tail_with_ranges(C, regime, mom, shadow):
    """The workload's shape: in-place ranges and the first layer's tail in one launch."""
    st = State(4 * 900, regime, mom, shadow, 51 + mom)
    st.set_tail(4, (8, 25, 8, 3), 128)
    st.add_range(4 + 600 + 8, 4 * 257, 19)
    st.add_range(2000, 256, 5)
    st.update_slabs(C)
    st.check(f"tail + ranges {regime}")


# --------------------------------------------------------------------------- D: the skip range
def _skips(n):
    return {"prefix": (0, 4 * 70), "middle": (4 * 70, 4 * 301), "suffix": (4 * 301, n), "whole": (0, n)}


@pytest.mark.parametrize("where", ["prefix", "middle", "suffix", "whole"])
@pytest.mark.parametrize("kind", ["plain", "ranges"])
@pytest.mark.parametrize("regime", REGIMES)
def test_skip(C, regime, kind, where):
    """plain: no slabs (sgd_plain_loop2's ``live``); ranges: two in-place
    ranges, the middle and the suffix skip cut the second (4 * 257 floats from
    4 * 200) in two, the prefix skip the first."""
    n = 4 * 600
    st = State(n, regime, True, True, 61)
    if kind == "ranges":
        st.add_range(4 * 40, 4 * 60, 8)
        st.add_range(4 * 200, 4 * 257, 7)
    skip = _skips(n)[where]
    st.update_slabs(C, skip=skip)
    st.check(f"skip {where} {kind} {regime}", skip=skip)


@pytest.mark.parametrize("regime", REGIMES)
def test_skip_with_tail_outside(C, regime):
    n = 4 * 600
    st = State(n, regime, True, True, 62)
    st.set_tail(8, (4, 25, -5, 3), 25)
    st.add_range(4 * 100, 4 * 64, 9)
    skip = (4 * 300, n)
    st.update_slabs(C, skip=skip)
    st.check(f"skip + tail {regime}", skip=skip)


def test_plain_path_second_item(C):
    """No slabs, a skip, and the size at which threads of the capped grid take
    a second float4 (sgd_plain_loop2's i2)."""
    n = SIZES[2]
    st = State(n, "real", True, True, 63)
    skip = (4 * 1000, 4 * 5000)
    st.update_slabs(C, skip=skip)
    st.check("plain path, two items", skip=skip)


def test_skip_over_the_tail_is_rejected(C):
    """The tail blocks do not consult the skip: the host refuses the pair
    before any launch.  (The executor never builds one: its skip starts at
    block >= 1's conv weight, after the first layer that is the tail.)"""
    for skip in ((0, 12), (8 + 296, 8 + 304), (0, 4 * 300)):
        st = State(4 * 300, "exact", True, True, 64)
        st.set_tail(8, (4, 25, 8, 3), 5)
        with pytest.raises(RuntimeError, match="skip overlaps the tail"):
            st.update_slabs(C, skip=skip)
        st.check("rejected", 0, 0)
    st = State(4 * 300, "exact", True, True, 64)
    st.set_tail(8, (4, 25, 8, 3), 5)
    st.update_slabs(C, skip=(0, 8))  # touching is fine
    st.check("skip up to the tail", skip=(0, 8))


# --------------------------------------------------------------------------- E: slab_reduce_multi
@pytest.mark.parametrize("kind", ["both", "tail", "ranges"])
@pytest.mark.parametrize("regime", REGIMES)
def test_slab_reduce_multi(C, regime, kind):
    n = 4 * 900
    st = State(n, regime, False, False, 71)
    ranges = [(8, 4, 5), (40, 256, 8), (400, 4 * 257, 17), (1600, 1028, 31)] if kind != "tail" else []
    data = [st.add_range(*r) for r in ranges]
    geom, tsp = (8, 25, -5, 3) if regime == "exact" else (8, 25, 8, 3), 40
    tdata = st.set_tail(2800, geom, tsp) if kind != "ranges" else None
    SENT = F32(-7.0)
    g = _d(np.full(n, SENT, F32))
    C.slab_reduce_multi(g.data_ptr(), n, *st.slab_args(), st.tail, 0 if tdata is None else st.tail_slab.data_ptr(),
                        _s())
    torch.cuda.synchronize()
    want = np.full(n, SENT, F32)
    written = np.isnan(st.g)
    want[written] = st.geff[written]
    if regime == "exact":
        for (off, ln, _), dd in zip(ranges, data):
            assert np.array_equal(want[off:off + ln].astype(np.int64), dd.astype(np.int64).sum(0))
    assert_bits(g, want, f"slab_reduce_multi {kind} {regime}")
    # ... and the stand-alone reduce of the same slabs
    for (off, ln, sp), t in zip(ranges, st.slabs):
        dst = _d(np.full(ln, SENT, F32))
        C.slab_reduce(t.data_ptr(), dst.data_ptr(), sp, 1, ln // 4, 4, 4, _s())
        torch.cuda.synchronize()
        assert_bits(dst, want[off:off + ln], f"slab_reduce {sp} splits {regime}")
    if tdata is not None:
        off, total, sp, cout, taps, cp, c = st.tail
        dst = _d(np.full(total + 4, SENT, F32))
        C.slab_reduce(st.tail_slab.data_ptr(), dst.data_ptr(), sp, cout, taps, cp, c, _s())
        torch.cuda.synchronize()
        assert_bits(dst, np.concatenate([want[off:off + total], np.full(4, SENT, F32)]), f"slab_reduce tail {regime}")


# --------------------------------------------------------------------------- F: side jobs of a conv launch
_CONV = {}  # host -> (operands, launch(side) -> output, output of the call without a job)


def _conv_host(C, host):
    """fwd: the smallest streaming conv_fwd (B 3, H 8, 16 -> 64, tile 1; region
    off for the call); wgrad: the smallest conv_wgrad (B 2, H 8, 64 -> 64,
    tile 1, 2 splits).  Returns launch(side) -> output tensor, and the output
    of the call without a job."""
    if host in _CONV:
        return _CONV[host]
    dev = torch.device("cuda")
    g0 = torch.Generator(device=dev).manual_seed(17)
    pad = lambda t: F.pad(t, (0, 0, 2, 2, 2, 2)).contiguous()  # noqa: E731
    if host == "fwd":
        B, H, cin, cout = 3, 8, 16, 64
        x = pad(torch.randn(B, H, H, cin, device=dev, generator=g0).to(BF16))
        w = (torch.randn(cout, 5, 5, cin, device=dev, generator=g0) * 0.05).to(BF16)

        def launch(side):
            y = torch.full((B, H, H, cout), float("nan"), dtype=BF16, device=dev)
            C.set_conv_region(0)  # the streaming kernel hosts side jobs
            try:
                C.conv_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), 0, 0, B, H, H, cin, cout, 5, 1, 1, _s(), side=side)
            finally:
                C.set_conv_region(1)
            torch.cuda.synchronize()
            return y
    else:
        B, H, cin, cout, splits = 2, 8, 64, 64, 2
        K = 25 * cin
        x = pad(torch.randn(B, H, H, cin, device=dev, generator=g0).to(BF16))
        dy = pad(torch.randn(B, H, H, cout, device=dev, generator=g0).to(BF16))

        def launch(side):
            out = torch.full((splits, cout, K), float("nan"), device=dev)
            C.conv_wgrad(dy.data_ptr(), x.data_ptr(), out.data_ptr(), B, H, H, cin, cout, 5, splits, K, 1, 0, _s(),
                         side=side)
            torch.cuda.synchronize()
            return out
    plain = launch(None)
    assert torch.isfinite(plain.float()).all()
    _CONV[host] = (launch, plain)
    return _CONV[host]


_SIDE_N, _SIDE_LO, _SIDE_HI = 4 * 1028, 4 * 100, 4 * 800  # 700 float4s: several trips of one or two workgroups


@pytest.mark.parametrize("nblk", [0, 1, 2])
@pytest.mark.parametrize("kind", ["ranges", "plain"])
@pytest.mark.parametrize("mom", [False, True])
@pytest.mark.parametrize("host", ["fwd", "wgrad"])
def test_side_sgd_job(C, host, mom, kind, nblk):
    """The update of [lo, hi) carried by a conv launch, sized by the launch
    (nblk 0) or forced into one or two workgroups (grid-stride trips of
    sgd_range_loop / sgd_plain_loop2, its second item included); both regimes."""
    launch, plain = _conv_host(C, host)
    for regime in REGIMES:
        st = State(_SIDE_N, regime, mom, True, 81 + nblk)
        if kind == "ranges":
            st.add_range(4 * 150, 4 * 257, 5)
            st.add_range(4 * 500, 4 * 64, 19)
        st.upload()
        job = C.side_sgd_job(*st.ptrs(), _SIDE_LO, _SIDE_HI, *st.slab_args(), nblk)
        out = launch(job)
        assert torch.equal(out, plain), "the conv's own output changed"
        st.check(f"side job {host} {kind} nblk={nblk} {regime}", _SIDE_LO, _SIDE_HI)


@pytest.mark.parametrize("nblk", [0, 1, 2])
@pytest.mark.parametrize("host", ["fwd", "wgrad"])
def test_side_reduce_job(C, host, nblk):
    launch, plain = _conv_host(C, host)
    for regime in REGIMES:
        st = State(_SIDE_N, regime, False, False, 91 + nblk)
        st.add_range(4 * 150, 4 * 257, 5)
        st.add_range(4 * 500, 4 * 64, 19)
        st.add_range(4 * 700, 4 * 100, 8)
        SENT = F32(-7.0)
        g = _d(np.full(_SIDE_N, SENT, F32))
        job = C.side_reduce_job(g.data_ptr(), _SIDE_LO, _SIDE_HI, *st.slab_args(), nblk)
        out = launch(job)
        assert torch.equal(out, plain), "the conv's own output changed"
        written = np.isnan(st.g)
        want = np.where(written, st.geff, SENT)
        assert_bits(g, want, f"side reduce {host} nblk={nblk} {regime}")


# --------------------------------------------------------------------------- G: next-step prep carried by the update
def _cifar_consts():
    from torch_distlearn_amd.data import CIFAR_MEAN, CIFAR_STD

    return list(CIFAR_MEAN), list(CIFAR_STD)


_ORDER = [0, 1, 2, 3, 3, 0, 1]  # the ring: steps 0 / 2 / 2^33 + 5 at B 3 read positions 012 / 601 / 456
_STEPS = [0, 2, 2 ** 33 + 5]
_W1 = (4, 25, 3)  # the first layer of these tests: [Cout 4][5 x 5][C 3] = 300 floats


def _dataset(H, W):
    """4 uint8 images [4, H, W, 3]; at H W = 64 the 256 pixels carry every
    byte value once per channel (a different permutation each)."""
    k = np.arange(4 * H * W)
    img = np.stack([(k * 37 + 11) % 256, (k * 91 + 200) % 256, (255 - k * 13) % 256], -1).astype(np.uint8)
    if 4 * H * W == 256:
        assert all(len(np.unique(img[:, c])) == 256 for c in range(3))
    return img.reshape(4, H, W, 3)


class Prep:
    """The buffers of one next-step preparation."""

    def __init__(self, H, W, Cp, step, B=3, sp=2):
        self.H, self.W, self.Cp, self.B, self.sp, self.step = H, W, Cp, B, sp, step
        self.img = _dataset(H, W)
        self.labels = np.array([100, 101, 102, 103], np.int64)
        self.mean, self.std = _cifar_consts()
        self.d_img, self.d_order = _d(self.img), _d(np.array(_ORDER, np.int32))
        self.d_lab = _d(self.labels)
        self.ctr0 = np.array([step, 77], np.int64)
        self.d_ctr = _d(self.ctr0)

    def fresh(self):
        xp = _d(np.full((self.B, self.H + 2 * self.sp, self.W + 2 * self.sp, self.Cp), SH_SENT, np.uint16))
        lab_out = _d(np.full(self.B + 3, -1, np.int64))
        return xp, lab_out

    def gather_args(self, xp, lab_out):
        return (self.d_img.data_ptr(), self.d_order.data_ptr(), self.d_lab.data_ptr(), lab_out.data_ptr(),
                self.d_ctr.data_ptr(), len(_ORDER), self.B, 3, self.mean, self.std, xp.data_ptr(), self.Cp, self.H,
                self.W, self.sp)

    def check(self, xp, lab_out, what):
        sp, H, W = self.sp, self.H, self.W
        x64, labs = xu.gather_ref(self.img, _ORDER, self.labels, self.step, self.B, self.mean, self.std)
        lo, hi, exempt = xu.gather_allowed(x64, self.mean, self.std)
        got = _h(xp)
        inner = got[:, sp:sp + H, sp:sp + W]
        val = xu.bf16_widen(inner[..., :3]).astype(np.float64)
        ok = (val == lo) | (val == hi)
        assert ok.all(), (f"{what}: {int((~ok).sum())} interior values are not the rounded fp64 value; first "
                          f"{val[~ok][0]!r} allowed {lo[~ok][0]!r} / {hi[~ok][0]!r}")
        assert not inner[..., 3:].any(), f"{what}: pad channels must be exactly zero"
        border = np.ones(got.shape[:3], bool)
        border[:, sp:sp + H, sp:sp + W] = False
        assert np.all(got[border] == SH_SENT), f"{what}: the spatial border was written"
        lab = _h(lab_out)
        assert lab[:self.B].tolist() == labs.tolist() and np.all(lab[self.B:] == -1), (what, lab)
        assert np.array_equal(_h(self.d_ctr), self.ctr0), f"{what}: the step counter changed"
        return exempt


def _w1_update(C, regime, source, w1_cp, prep_args, zero=((), ()), skip=(0, 0), extra_range=None, tail_off=None):
    """An update of a small buffer holding the first layer at pack_off,
    carrying a NextPrep.  source "tail": the layer's gradient is a slab tail
    (5 splits, channel-padded to 8); "main": it comes from g and the main loop
    packs it (pack_off 8: not a multiple of 3 * 4 elements, so float4s
    straddle tap rows and output channels).  Returns (state, w1p, run)."""
    cout, taps, c = _W1
    pack_off, pack_len = 8, cout * taps * c
    st = State(4 * 300, regime, True, True, 95 + (w1_cp > 0))
    if source == "tail":
        st.set_tail(pack_off if tail_off is None else tail_off, (cout, taps, 8, c), 5)
        st.add_range(4 * 100, 4 * 64, 9)
    else:
        st.add_range(4 * 100, 4 * 64, 9)
    if extra_range is not None:
        st.add_range(*extra_range)
    w1p = _d(np.full(xu.pack1_size(cout, taps, w1_cp), W1_SENT, np.uint16))
    st.upload()

    def run():
        nxt = C.next_prep(*prep_args, list(zero[0]), list(zero[1]), w1p.data_ptr(), w1_cp, pack_off, pack_len)
        st.update_slabs(C, skip=skip, next_prep=nxt)

    return st, w1p, run


def _check_w1p(w1p, p_after, w1_cp, what):
    cout, taps, c = _W1
    pack_off, pack_len = 8, cout * taps * c
    idx = xu.pack1_index_ref(np.arange(pack_len), c, w1_cp)
    want = np.full(xu.pack1_size(cout, taps, w1_cp), W1_SENT, np.uint16)
    want[idx] = xu.bf16_bits(p_after[pack_off:pack_off + pack_len])
    assert_bits(w1p, want, what)


@pytest.mark.parametrize("step", _STEPS, ids=["step0", "step2", "step2p33"])
@pytest.mark.parametrize("shape", [(8, 8, 8), (8, 8, 4), (4, 6, 8), (8, 8, 16)], ids=lambda s: "x".join(map(str, s)))
def test_gather_carried_by_update(C, shape, step):
    """(H, W, Cp): 8x8 with Cp 8 / 4 the quad path, 4x6 and Cp 16 the generic
    one.  Over the three steps the 8x8 cases read all four images: every
    (byte value, channel) pair.  The same launch updates the buffer and packs
    the first layer from its slab tail; all of it is checked."""
    H, W, Cp = shape
    pr = Prep(H, W, Cp, step)
    assert xu.gather_samples(_ORDER, step, 3) == {0: [0, 1, 2], 2: [1, 0, 1]}.get(step, [3, 0, 1])
    xp, lab_out = pr.fresh()
    st, w1p, run = _w1_update(C, "real", "tail", 8 if Cp != 4 else -5, pr.gather_args(xp, lab_out))
    run()
    exempt = pr.check(xp, lab_out, f"carried gather {shape} step {step}")
    assert int(exempt.sum()) <= 8
    p = st.check("update carrying the gather")
    _check_w1p(w1p, p, 8 if Cp != 4 else -5, "first-layer pack")
    # the stand-alone prep launch on the same inputs: bitwise the carried one
    xp2, lab2 = pr.fresh()
    C.prep_step_gather(*pr.gather_args(xp2, lab2), 0, w1p.data_ptr(), 0, 0, 3, 8, [], [], [], [], [], [], _s())
    torch.cuda.synchronize()
    assert_bits(xp2, _h(xp), "prep_step_gather vs the carried gather")
    assert_bits(lab2, _h(lab_out), "prep_step_gather labels")


def test_gather_exemptions_over_all_pairs(C):
    """All four images in one launch (B 4, identity order): the 768 (value,
    channel) pairs at once, at most 8 of them under the exemption."""
    pr = Prep(8, 8, 8, 0, B=4)
    pr.d_order = _d(np.arange(7, dtype=np.int32) % 4)
    xp, lab_out = pr.fresh()
    C.prep_step_gather(pr.d_img.data_ptr(), pr.d_order.data_ptr(), pr.d_lab.data_ptr(), lab_out.data_ptr(),
                       pr.d_ctr.data_ptr(), 7, 4, 3, pr.mean, pr.std, xp.data_ptr(), 8, 8, 8, 2,
                       0, xp.data_ptr(), 0, 0, 3, 8, [], [], [], [], [], [], _s())
    torch.cuda.synchronize()
    x64, _ = xu.gather_ref(pr.img, list(range(4)), pr.labels, 0, 4, pr.mean, pr.std)
    lo, hi, exempt = xu.gather_allowed(x64, pr.mean, pr.std)
    val = xu.bf16_widen(_h(xp)[:, 2:10, 2:10, :3]).astype(np.float64)
    assert ((val == lo) | (val == hi)).all()
    assert exempt.size == 768 and int(exempt.sum()) <= 8


@pytest.mark.parametrize("nz", [1, 3, 8])
def test_zero_job_carried_by_update(C, nz):
    sizes = [4, 4 * 1025, 4 * 257]
    lens = [sizes[j % 3] for j in range(nz)]
    SENT = F32(5.0)
    buf = _d(np.full(sum(lens) + 4 * (nz + 1), SENT, F32))
    want = np.full(buf.numel(), SENT, F32)
    ptrs, o = [], 4
    for ln in lens:  # guard floats on both sides of every range
        ptrs.append(buf.data_ptr() + 4 * o)
        want[o:o + ln] = 0
        o += ln + 4
    pr = Prep(8, 8, 8, 0)
    xp, lab_out = pr.fresh()
    st, w1p, run = _w1_update(C, "exact", "tail", 8, pr.gather_args(xp, lab_out), zero=(ptrs, lens))
    run()
    assert_bits(buf, want, f"zero job of {nz} ranges")
    pr.check(xp, lab_out, "gather beside the zero job")
    st.check("update beside the zero job")


def test_zero_job_nine_ranges_throw(C):
    buf = _d(np.full(4 * 20, F32(5.0), F32))
    pr = Prep(8, 8, 8, 0)
    xp, lab_out = pr.fresh()
    st, w1p, run = _w1_update(C, "exact", "tail", 8, pr.gather_args(xp, lab_out),
                              zero=([buf.data_ptr() + 32 * j for j in range(9)], [4] * 9))
    with pytest.raises(RuntimeError, match="up to 8 zero ranges"):
        run()
    torch.cuda.synchronize()
    assert bool((buf == 5.0).all())
    st.check("nothing launched", 0, 0)


@pytest.mark.parametrize("w1_cp", [8, -5])
@pytest.mark.parametrize("source", ["tail", "main"])
@pytest.mark.parametrize("regime", REGIMES)
def test_first_layer_pack(C, regime, source, w1_cp):
    pr = Prep(8, 8, 8 if w1_cp > 0 else 4, 2)
    xp, lab_out = pr.fresh()
    st, w1p, run = _w1_update(C, regime, source, w1_cp, pr.gather_args(xp, lab_out))
    run()
    p = st.check(f"update packing from the {source} {regime}")
    _check_w1p(w1p, p, w1_cp, f"w1p from the {source}, cp {w1_cp}, {regime}")
    pr.check(xp, lab_out, "gather beside the pack")


@pytest.mark.parametrize("case", ["tail_elsewhere", "pack_in_skip", "pack_over_range"])
def test_pack_rejections_throw_before_launch(C, case):
    pr = Prep(8, 8, 8, 0)
    xp, lab_out = pr.fresh()
    kw, match = {
        "tail_elsewhere": (dict(source="tail", tail_off=4 * 200), "not the first layer"),
        "pack_in_skip": (dict(source="main", skip=(4 * 50, 4 * 80)), "not updated by this launch"),
        "pack_over_range": (dict(source="main", extra_range=(4 * 70, 4 * 10, 2)), "overlaps a slab range"),
    }[case]
    if case == "pack_over_range":  # ranges ascend: build the overlapping one first
        cout, taps, c = _W1
        st = State(4 * 300, "exact", True, True, 97)
        st.add_range(4 * 70, 4 * 10, 2)
        st.add_range(4 * 100, 4 * 64, 9)
        w1p = _d(np.full(xu.pack1_size(cout, taps, 8), W1_SENT, np.uint16))
        st.upload()

        def run():
            nxt = C.next_prep(*pr.gather_args(xp, lab_out), [], [], w1p.data_ptr(), 8, 8, cout * taps * c)
            st.update_slabs(C, next_prep=nxt)
    else:
        st, w1p, run = _w1_update(C, "exact", kw.pop("source"), 8, pr.gather_args(xp, lab_out), **kw)
    with pytest.raises(RuntimeError, match=match):
        run()
    torch.cuda.synchronize()
    st.check(f"{case}: nothing launched", 0, 0)
    assert np.all(_h(w1p) == W1_SENT) and np.all(_h(xp) == SH_SENT) and np.all(_h(lab_out) == -1)


# --------------------------------------------------------------------------- H: elastic averaging
def _elastic_state(regime, n, seed):
    rng = np.random.default_rng(seed)
    if regime == "exact":
        draw = lambda: rng.integers(-64, 65, n).astype(F32)  # noqa: E731
        return draw(), draw(), draw(), F32(0.25)
    draw = lambda: rng.standard_normal(n).astype(F32)  # noqa: E731
    return draw(), draw(), draw(), F32(0.3)


@pytest.mark.parametrize("n", [4, 4 * 257, 4 * 2049])
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("pending", [False, True])
@pytest.mark.parametrize("regime", REGIMES)
def test_elastic_step(C, record_property, regime, pending, shadow, n):
    p0, c0, d0, alpha = _elastic_state(regime, n, n + pending)
    p, c, pend, out = _d(p0), _d(c0), _d(d0), _d(np.full(n, NAN, F32))
    sh = _d(np.full(n, SH_SENT, np.uint16)) if shadow else None
    C.elastic_step(p.data_ptr(), c.data_ptr(), pend.data_ptr() if pending else 0, out.data_ptr(),
                   0 if sh is None else sh.data_ptr(), float(alpha), n, _s())
    torch.cuda.synchronize()
    c1 = xu.add32(c0, d0) if pending else c0
    diff = xu.add32(p0, -c1)
    delta = xu.mul32(alpha, diff)
    assert_bits(c, c1, "center")
    assert_bits(pend, d0, "pending is only read")
    assert_bits(out, delta, "out = fp32(alpha fp32(p - c))")
    two_step, fused = xu.add32(p0, -delta), xu.fma32(-alpha, diff, p0)
    got = _h(p)
    if regime == "exact":
        want64 = p0.astype(np.float64) - 0.25 * (p0.astype(np.float64) - c1.astype(np.float64))
        assert np.array_equal(two_step.astype(np.float64), want64) and np.array_equal(fused, two_step)
        assert_bits(got, two_step, "p")
    else:
        # the kernel leaves this contraction to the compiler: one and the same form for every element
        forms = {"p - out": np.array_equal(_bits(got), _bits(two_step)),
                 "fma(-alpha, p - c, p)": np.array_equal(_bits(got), _bits(fused))}
        if n > 4:
            assert not np.array_equal(_bits(two_step), _bits(fused))  # the data tells the forms apart
        record_property("elastic_step_p_form", "; ".join(k for k, v in forms.items() if v))
        print("elastic_step p form:", [k for k, v in forms.items() if v])
        assert any(forms.values()), "p is neither fp32(p - out) nor fma(-alpha, fp32(p - c), p) throughout"
    if sh is not None:
        assert_bits(sh, xu.bf16_bits(got), "bf16 shadow of p")


@pytest.mark.parametrize("n", [4, 4 * 257])
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("regime", REGIMES)
def test_elastic_step_wire16(C, regime, shadow, n):
    """delta rounded to bf16 for the wire, p moved by the rounded delta (which
    no contraction can reach: it passes through the bf16 rounding)."""
    p0, c0, _, alpha = _elastic_state(regime, n, n + 5)
    p, c, out = _d(p0), _d(c0), _d(np.full(n, NAN, F32))
    out16 = _d(np.full(n, SH_SENT, np.uint16))
    sh = _d(np.full(n, SH_SENT, np.uint16)) if shadow else None
    C.elastic_step_wire16(p.data_ptr(), c.data_ptr(), out.data_ptr(), out16.data_ptr(),
                          0 if sh is None else sh.data_ptr(), float(alpha), n, _s())
    torch.cuda.synchronize()
    wire = xu.bf16_bits(xu.mul32(alpha, xu.add32(p0, -c0)))
    delta = xu.bf16_widen(wire)
    want_p = xu.add32(p0, -delta)
    if regime == "exact":  # |alpha (p - c)| <= 32 in quarters: 8 bits hold it
        assert np.array_equal(delta.astype(np.float64), 0.25 * (p0.astype(np.float64) - c0))
    assert_bits(c, c0, "center is only read")
    assert_bits(out16, wire, "bf16 wire delta")
    assert_bits(out, delta, "fp32 copy of the rounded delta")
    assert_bits(p, want_p, "p")
    if sh is not None:
        assert_bits(sh, xu.bf16_bits(want_p), "bf16 shadow of p")
