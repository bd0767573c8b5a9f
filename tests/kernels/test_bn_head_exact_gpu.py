"""The fused BatchNorm + ReLU + 2x2 max-pool kernels (bn_pool.hip,
bn_fin_dev.h) and the classifier head (head.hip, head_wgrad_dev.h) against the
fp64 oracles of tests/kernels/exact_bn_head.py.

Exact regime: integer activations / gradients and dyadic coefficients, every
output compared bit for bit (``exact.assert_exact``); the references assert
that every intermediate is an fp32 number, so the regime proves itself for
each shape.  Real-valued regime: the forward is still bitwise (the fp32 fma is
emulated), sums and ``dy`` are checked per element under bounds derived in the
oracle module's docstrings.  No kernel is compared with another kernel only,
and no bound is relative to a norm.

Shapes are (B, H, C) with W = H, the smallest that reach each path: (1, 2, 8)
one window; (2, 4, 512) the C == 2 * blockDim prologues; (2, 4, 1024) kFinMaxC;
(3, 6, 32) odd Ho / Wo, M not a power of two; (9, 8, 64) = 1152 items with the
grids forced to one block, so that every thread holds 4 or 5 items (the
reduce's batch of 4, its tail for half the threads, the prefetch path of the
apply and forward-fin loops), or to three blocks (1 or 2 items)."""
import functools

import pytest
import torch

from tests.kernels import exact
from tests.kernels import exact_bn_head as xb

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NAN = float("nan")
EPS, MOM = 1e-3, 0.1
NC = 10

EXACT_SHAPES = [(1, 2, 8), (4, 8, 64), (2, 4, 512), (2, 4, 1024), (3, 6, 32), (9, 8, 64)]
REAL_SHAPES = [(8, 16, 128), (16, 4, 512), (3, 8, 32)]


def _sid(s):
    return "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from torch_distlearn_amd import _native

    return _native.native()


@pytest.fixture(autouse=True)
def _process_settings(request):
    """The reduction mode and the BN grids are process-wide: every test starts
    in mode 0 and leaves mode 0 and the defaults of bn_pool.hip behind (fin
    grid 2048, 2 items per thread in the reduce, minw 4 / 4)."""
    if "C" not in request.fixturenames:
        yield
        return
    C = request.getfixturevalue("C")
    C.set_reduce_atomic(0)
    yield
    torch.cuda.synchronize()
    _KEEP.clear()
    C.set_reduce_atomic(0)
    C.set_bn_fin_grid(2048)
    C.set_bn_bwd_items(2)
    C.set_bn_minw(4, 4)


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """The cached cases hold device tensors: drop them when the file is done,
    so that nothing of it stays behind in the process."""
    yield
    _int_case.cache_clear()
    _REAL.clear()
    _KEEP.clear()


def _s():
    return torch.cuda.current_stream().cuda_stream


_KEEP = []  # device copies made by _d: the kernels get raw pointers, so they must outlive the launch


def _d(t):
    _KEEP.append(t.to("cuda").contiguous())
    return _KEEP[-1]


def _is_pow2(n):
    return n & (n - 1) == 0


def _bordered(B, H, W, Cc, opad):
    """bf16 [B][H + 2 opad][W + 2 opad][C]: NaN interior (must be fully
    overwritten), 3.0 border (must be kept)."""
    t = torch.full((B, H + 2 * opad, W + 2 * opad, Cc), 3.0, dtype=BF16, device="cuda")
    t[:, opad:opad + H, opad:opad + W] = NAN
    return t


def _check_bordered(t, opad, ref64, what, bound=None):
    t = t.cpu()
    H, W = t.shape[1] - 2 * opad, t.shape[2] - 2 * opad
    inner = t[:, opad:opad + H, opad:opad + W]
    if bound is None:
        exact.assert_exact(inner.contiguous(), ref64, what)
    else:
        xb.assert_within(inner, ref64, bound, what)
    if opad:
        mask = torch.ones(t.shape[1:3], dtype=torch.bool)
        mask[opad:opad + H, opad:opad + W] = False
        assert bool((t[:, mask] == 3.0).all()), f"{what}: the border was written"


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
class IntCase:
    """Integer operands, hand-set coefficients and the fp64 references of one shape."""

    def __init__(self, shape):
        B, H, Cc = shape
        g = torch.Generator().manual_seed(100 * B + 10 * H + Cc)
        self.shape, self.M, self.n_pix = shape, B * H * H, B * (H // 2) ** 2
        self.y, self.dP, self.coef, self.gamma = xb.int_bn_inputs(B, H, Cc, g)
        self.fwd = xb.pool_fwd_ref(self.y, self.coef)
        self.s_dz, self.s_dzx, _, _ = xb.bwd_sums_ref(self.y, self.dP, self.coef, exact_regime=True)
        self.exact_apply = _is_pow2(self.M)
        self.dy, self.m_a, self.m_b, self.m_c = xb.apply_ref(self.y, self.dP, self.coef, self.gamma, self.s_dz,
                                                             self.s_dzx, self.M, exact_regime=self.exact_apply)
        self.yd, self.dPd, self.coefd, self.gammad = _d(self.y), _d(self.dP), _d(self.coef), _d(self.gamma)

    def check_dy(self, dyp, rows, what):
        """Exact where M is a power of two; otherwise the per-element bound (the
        totals are exact integers either way, so the reference needs no rows)."""
        bound = None if self.exact_apply else xb.apply_bound(self.dy, self.m_a, self.m_b, self.m_c, rows)
        _check_bordered(dyp, 2, self.dy, what, bound)


@functools.lru_cache(maxsize=None)
def _int_case(shape):
    return IntCase(shape)


def _real_bn_inputs(shape, seed=0):
    """randn*2 + 0.5 activations, a third of the channels with negative gamma,
    channel 1 constant (var = 0, invstd = rsqrt(eps)), channel 2 with mean 64
    and standard deviation 1/4 (the sumsq/M - mean^2 cancellation), channel 3
    with gamma = 0 and beta = 1/2: its four window positions tie at 1/2 with
    different xhat, so sum dz*xhat and dy depend on the first-index rule in
    every kernel copy, the head's fused reduce included."""
    B, H, Cc = shape
    g = torch.Generator().manual_seed(7 * B + 3 * H + Cc + seed)
    y = torch.randn(B, H, H, Cc, generator=g) * 2 + 0.5
    y[..., 1] = 1.5
    y[..., 2] = 64 + 0.25 * torch.randn(B, H, H, generator=g)
    y = y.to(BF16)
    gamma = (torch.rand(Cc, generator=g) + 0.5) * torch.where(torch.arange(Cc) % 3 == 0, -1.0, 1.0)
    beta, bias = torch.randn(Cc, generator=g) * 0.1, torch.randn(Cc, generator=g) * 0.1
    gamma[3], beta[3] = 0.0, 0.5
    dP = torch.randn(B, H // 2, H // 2, Cc, generator=g).to(BF16)
    yf = y.float().reshape(-1, Cc)
    sums = torch.stack([yf.sum(0), (yf * yf).sum(0)])
    return y, dP, gamma, beta, bias, sums, g


class RealCase:
    """Real-valued operands; the coefficient table is bn_finalize's own output
    (checked in test_bn_finalize_real), every reference is evaluated from it."""

    def __init__(self, C, shape):
        B, H, Cc = shape
        self.shape, self.M, self.n_pix = shape, B * H * H, B * (H // 2) ** 2
        self.y, self.dP, self.gamma, self.beta, self.bias, self.sums, self.gen = _real_bn_inputs(shape)
        self.yd, self.dPd, self.gammad = _d(self.y), _d(self.dP), _d(self.gamma)
        coef = torch.full((4, Cc), NAN, device="cuda")
        C.set_reduce_atomic(0)
        C.bn_finalize(_d(self.sums).data_ptr(), 1, Cc, self.M, self.gammad.data_ptr(), _d(self.beta).data_ptr(), 0, 0, 0,
                      EPS, MOM, 0, coef.data_ptr(), _s())
        torch.cuda.synchronize()
        self.coefd, self.coef = coef, coef.cpu()
        self.fwd = xb.pool_fwd_ref(self.y, self.coef)
        self.s_dz, self.s_dzx, self.a_dz, self.a_dzx = xb.bwd_sums_ref(self.y, self.dP, self.coef)

    def check_rows(self, rows_dz, rows_dzx, what):
        xb.assert_within(rows_dz.double().sum(0), self.s_dz, xb.sums_bound(self.n_pix, self.a_dz), what + ": sum dz")
        xb.assert_within(rows_dzx.double().sum(0), self.s_dzx, xb.sums_bound(self.n_pix, self.a_dzx),
                         what + ": sum dz*xhat")

    def check_dy(self, dyp, rows_dz, rows_dzx, what):
        """dy against the reference evaluated from the rows the kernel read."""
        ref, m_a, m_b, m_c = xb.apply_ref(self.y, self.dP, self.coef, self.gamma, rows_dz, rows_dzx, self.M)
        _check_bordered(dyp, 2, ref, what, xb.apply_bound(ref, m_a, m_b, m_c, rows_dz.shape[0]))


_REAL = {}


def _real_case(C, shape):
    if shape not in _REAL:
        _REAL[shape] = RealCase(C, shape)
    return _REAL[shape]


def _reduce(C, case, mode, blocks=None, extra_rows=2):
    """bn_relu_pool_bwd_reduce in reduction mode ``mode`` (0 or R) -> (buffer
    on the device, rows of sum dz [T][C], rows of sum dz*xhat [T][C] on the CPU).
    Mode 0: rows past the block count must keep their NaN pre-fill."""
    B, H, Cc = case.shape
    G = C.bn_bwd_blocks(B, H, H, Cc) if blocks is None else blocks
    C.set_reduce_atomic(mode)
    if mode == 0:
        buf = torch.full((G + extra_rows, 2, Cc), NAN, device="cuda")
    else:
        buf = torch.zeros(mode, 2, Cc, device="cuda")
    C.bn_relu_pool_bwd_reduce(case.yd.data_ptr(), case.dPd.data_ptr(), case.coefd.data_ptr(), buf.data_ptr(), B, H, H,
                              Cc, G, _s())
    torch.cuda.synchronize()
    return (buf,) + _split_rows(buf, mode, G)


def _split_rows(buf, mode, T):
    """Mode 0 rows are [sum dz ; sum dz*xhat], T of them written; the atomic
    rows are [dgamma = sum dz*xhat ; dbeta = sum dz], rows >= T untouched zeros."""
    r = buf.cpu()
    if mode == 0:
        assert torch.isfinite(r[:T]).all(), "a written partial row is not finite"
        assert torch.isnan(r[T:]).all(), "rows past the block count were written"
        return r[:T, 0], r[:T, 1]
    assert torch.isfinite(r).all()
    assert bool((r[min(T, mode):] == 0).all()), "an atomic row that no block owns was written"
    return r[:, 1], r[:, 0]


def _assert_rows_exact(case, rows_dz, rows_dzx, what):
    exact.assert_exact(rows_dz.double().sum(0).float(), case.s_dz, what + ": sum dz")
    exact.assert_exact(rows_dzx.double().sum(0).float(), case.s_dzx, what + ": sum dz*xhat")


# ---------------------------------------------------------------------------
# 2. exact-integer regime
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("opad", [0, 2])
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_sid)
def test_fwd_exact(C, shape, opad):
    """bn_relu_pool_fwd: the interior (NaN pre-fill) is fully overwritten with
    the bf16 rounding of the fp64 reference, the border keeps its pre-fill."""
    case = _int_case(shape)
    B, H, Cc = shape
    out = _bordered(B, H // 2, H // 2, Cc, opad)
    C.bn_relu_pool_fwd(case.yd.data_ptr(), case.coefd.data_ptr(), out.data_ptr(), B, H, H, Cc, opad, _s())
    torch.cuda.synchronize()
    _check_bordered(out, opad, case.fwd, "pooled")


@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("mode", [0, 1, 16], ids=["rows", "atomic1", "atomic16"])
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_sid)
def test_bwd_reduce_exact(C, shape, mode, blocks):
    """bn_relu_pool_bwd_reduce: the integer totals are identical whatever the
    block partition and the atomic order; in mode 0 the rows past the block
    count keep their NaN.  One block at (9, 8, 64): 4 or 5 items per thread,
    one full batch of 4 and the tail; three blocks: the tail loop only."""
    case = _int_case(shape)
    _, rz, rzx = _reduce(C, case, mode, blocks)
    _assert_rows_exact(case, rz, rzx, "bwd_reduce")


@pytest.mark.parametrize("mode", [0, 16], ids=["rows", "atomic16"])
def test_bwd_reduce_exact_many_items(C, mode):
    """(36, 8, 64): 4608 items; one block gives every thread 18 items (four
    full batches of 4 and a tail of 2), three blocks 6 (one batch, tail of 2),
    and set_bn_bwd_items(0) takes the other grid rule of bn_bwd_blocks."""
    case = _int_case((36, 8, 64))
    for blocks in (1, 3, 2):
        _, rz, rzx = _reduce(C, case, mode, blocks)
        _assert_rows_exact(case, rz, rzx, f"bwd_reduce blocks={blocks}")
    C.set_bn_bwd_items(0)
    G = C.bn_bwd_blocks(36, 8, 8, 64)
    assert G == 18  # max(min(256, items / 256), items / 1024); the default rule gives 9
    _, rz, rzx = _reduce(C, case, mode)
    assert mode != 0 or rz.shape[0] == G
    _assert_rows_exact(case, rz, rzx, "bwd_reduce items=0")


@pytest.mark.parametrize("shape", EXACT_SHAPES + [(36, 8, 64)], ids=_sid)
def test_bwd_finalize_apply_exact(C, shape):
    """Mode 0: bn_relu_pool_bwd_reduce -> bn_bwd_finalize -> bn_relu_pool_bwd_apply.
    dgamma, dbeta and (M a power of two) the apply coefficients and dy are exact."""
    case = _int_case(shape)
    B, H, Cc = shape
    buf, rz, rzx = _reduce(C, case, 0, extra_rows=0)
    T = rz.shape[0]
    dg, db = torch.full((Cc,), NAN, device="cuda"), torch.full((Cc,), NAN, device="cuda")
    acoef = torch.full((3, Cc), NAN, device="cuda")
    C.bn_bwd_finalize(buf.data_ptr(), T, Cc, case.M, case.gammad.data_ptr(), case.coefd.data_ptr(), dg.data_ptr(),
                      db.data_ptr(), acoef.data_ptr(), _s())
    dyp = _bordered(B, H, H, Cc, 2)
    C.bn_relu_pool_bwd_apply(case.yd.data_ptr(), case.dPd.data_ptr(), case.coefd.data_ptr(), acoef.data_ptr(),
                             dyp.data_ptr(), B, H, H, Cc, 2, _s())
    torch.cuda.synchronize()
    exact.assert_exact(dg, case.s_dzx, "dgamma")
    exact.assert_exact(db, case.s_dz, "dbeta")
    a, b, c = xb.apply_coefficients(case.gamma, case.coef[1], case.s_dz, case.s_dzx, case.M)
    exact.assert_exact(acoef[0], a, "acoef a")
    if case.exact_apply:
        exact.assert_exact(acoef[1], b, "acoef b")
        exact.assert_exact(acoef[2], c, "acoef c")
    case.check_dy(dyp, 1, "dy")


@pytest.mark.parametrize("fin_grid", [None, 1], ids=["grid", "grid1"])
@pytest.mark.parametrize("R", [1, 16], ids=["rows1", "rows16"])
@pytest.mark.parametrize("shape", EXACT_SHAPES + [(36, 8, 64)], ids=_sid)
def test_bwd_apply_sums_exact(C, shape, R, fin_grid):
    """Atomic modes: reduce into R rows, then bn_relu_pool_bwd_apply_sums (one
    block when the fin grid is forced to 1: 4 or 5 items per thread at
    (9, 8, 64), 18 at (36, 8, 64), through the prefetch path).  dgamma_out / dbeta_out receive the exact totals."""
    case = _int_case(shape)
    B, H, Cc = shape
    buf, rz, rzx = _reduce(C, case, R, 3 if fin_grid else None)
    _assert_rows_exact(case, rz, rzx, "bwd_reduce")
    if fin_grid:
        C.set_bn_fin_grid(fin_grid)
    tot = torch.full((2, Cc), NAN, device="cuda")
    dyp = _bordered(B, H, H, Cc, 2)
    C.bn_relu_pool_bwd_apply_sums(case.yd.data_ptr(), case.dPd.data_ptr(), case.coefd.data_ptr(), buf.data_ptr(),
                                  case.gammad.data_ptr(), case.M, dyp.data_ptr(), B, H, H, Cc, 2, tot[0].data_ptr(),
                                  tot[1].data_ptr(), _s())
    torch.cuda.synchronize()
    exact.assert_exact(tot[0], case.s_dzx, "dgamma_out")
    exact.assert_exact(tot[1], case.s_dz, "dbeta_out")
    case.check_dy(dyp, R, "dy")


def test_bwd_apply_sums_exact_uncapped_and_null_totals(C):
    """set_bn_minw(1, 1) selects the uncapped instances of fwd_fin / apply_sums;
    null dgamma_out / dbeta_out (R = 1: the row is the gradient) are accepted."""
    C.set_bn_minw(1, 1)
    C.set_bn_fin_grid(1)
    case = _int_case((9, 8, 64))
    B, H, Cc = case.shape
    buf, _, _ = _reduce(C, case, 1)
    dyp = _bordered(B, H, H, Cc, 2)
    C.bn_relu_pool_bwd_apply_sums(case.yd.data_ptr(), case.dPd.data_ptr(), case.coefd.data_ptr(), buf.data_ptr(),
                                  case.gammad.data_ptr(), case.M, dyp.data_ptr(), B, H, H, Cc, 2, 0, 0, _s())
    torch.cuda.synchronize()
    case.check_dy(dyp, 1, "dy")
    case = _int_case((4, 8, 64))
    B, H, Cc = case.shape
    buf, _, _ = _reduce(C, case, 1)
    dyp = _bordered(B, H, H, Cc, 2)
    C.bn_relu_pool_bwd_apply_sums(case.yd.data_ptr(), case.dPd.data_ptr(), case.coefd.data_ptr(), buf.data_ptr(),
                                  case.gammad.data_ptr(), case.M, dyp.data_ptr(), B, H, H, Cc, 2, 0, 0, _s())
    torch.cuda.synchronize()
    case.check_dy(dyp, 1, "dy")


def _int_slabs(splits, shape, generator, top=700, part=300):
    """``splits`` integer-valued fp32 slabs whose sum is uniform in [-top, top]:
    past 256 in magnitude for more than half of the elements, so its bf16
    rounding is a real one; every partial sum is a small integer, exact in fp32
    in any order."""
    total = torch.randint(-top, top + 1, shape, generator=generator)
    parts = torch.randint(-part, part + 1, (splits - 1,) + tuple(shape), generator=generator)
    slabs = torch.cat([parts, (total - parts.sum(0)).unsqueeze(0)]).float()
    assert float(slabs.abs().max()) * splits < exact.EXACT_LIMIT
    return slabs, total.double()


@pytest.mark.parametrize("mode", [0, 16], ids=["rows", "atomic16"])
@pytest.mark.parametrize("splits", [2, 4, 8, 16])
@pytest.mark.parametrize("shape", [(1, 2, 8), (4, 8, 64), (2, 4, 512), (9, 8, 64), (3, 6, 32)], ids=_sid)
def test_combine_bwd_reduce_exact(C, shape, splits, mode):
    """combine_bwd_reduce<2|4|8|16>: dP is the single bf16 rounding of the slab
    sum, the rows are the exact reduce of that dP, the returned row count is
    honoured (rows past it keep their NaN)."""
    base = _int_case(shape)
    B, H, Cc = shape
    g = torch.Generator().manual_seed(splits + B + Cc)
    slabs, total = _int_slabs(splits, (B, H // 2, H // 2, Cc), g)
    dP_exp = exact.expected(total, BF16)
    assert float((dP_exp.double() != total).double().mean()) > 0.2 or total.numel() < 64
    s_dz, s_dzx, _, _ = xb.bwd_sums_ref(base.y, dP_exp, base.coef, exact_regime=True)
    nb = C.combine_bwd_reduce_blocks(B, H, H, Cc)
    C.set_reduce_atomic(mode)
    buf = torch.full((nb + 2, 2, Cc), NAN, device="cuda") if mode == 0 else torch.zeros(mode, 2, Cc, device="cuda")
    dP = torch.full(dP_exp.shape, NAN, dtype=BF16, device="cuda")
    got_nb = C.combine_bwd_reduce(_d(slabs).data_ptr(), splits, dP.data_ptr(), base.yd.data_ptr(), base.coefd.data_ptr(),
                                  buf.data_ptr(), B, H, H, Cc, _s())
    torch.cuda.synchronize()
    assert got_nb == nb
    exact.assert_exact(dP, total, "dP")
    rz, rzx = _split_rows(buf, mode, nb)
    exact.assert_exact(rz.double().sum(0).float(), s_dz, "sum dz")
    exact.assert_exact(rzx.double().sum(0).float(), s_dzx, "sum dz*xhat")


def _head_int(B, F, seed=0):
    g = torch.Generator().manual_seed(1000 * B + F + seed)
    h, w, b, lab, k = xb.head_exact_inputs(B, F, g)
    return h, w, b, lab, xb.head_exact_ref(h, w, b, lab)


def _check_wgrad_exact(ref, dw, db, loss, slot=None, ctr=None, launches=1):
    exact.assert_exact(dw, ref["dW"], "dW")
    exact.assert_exact(db, ref["db"], "db")
    exact.assert_exact(loss, ref["loss"].reshape(1), "loss")
    if slot is not None:
        assert float(slot) == 1.0
    if ctr is not None:
        assert ctr.tolist() == [launches, 0]


@pytest.mark.parametrize("mode", [0, 16], ids=["rows", "atomic16"])
@pytest.mark.parametrize("F", [264, 2048])
def test_bwd_reduce_head_exact(C, mode, F):
    """bn_bwd_reduce_head: the BN rows and the head's dW / db / loss, each
    against its own fp64 reference (the two halves share B)."""
    case = _int_case((8, 4, 512))
    B, H, Cc = case.shape
    h, w, b, lab, ref = _head_int(B, F)
    G = C.bn_bwd_blocks(B, H, H, Cc)
    C.set_reduce_atomic(mode)
    buf = torch.full((G + 2, 2, Cc), NAN, device="cuda") if mode == 0 else torch.zeros(mode, 2, Cc, device="cuda")
    dw, db = torch.full((NC, F), NAN, device="cuda"), torch.full((NC,), NAN, device="cuda")
    loss, slot = torch.full((1,), NAN, device="cuda"), torch.zeros(1, device="cuda")
    ctr = torch.zeros(2, dtype=torch.int64, device="cuda")
    C.bn_bwd_reduce_head(case.yd.data_ptr(), case.dPd.data_ptr(), case.coefd.data_ptr(), buf.data_ptr(), B, H, H, Cc, G,
                         _d(h).data_ptr(), _d(ref["dlogits"].float()).data_ptr(), _d(ref["loss_b"].float()).data_ptr(), F,
                         NC, dw.data_ptr(), db.data_ptr(), loss.data_ptr(), slot.data_ptr(), ctr.data_ptr(), _s())
    torch.cuda.synchronize()
    rz, rzx = _split_rows(buf, mode, G)
    _assert_rows_exact(case, rz, rzx, "bn_bwd_reduce_head")
    _check_wgrad_exact(ref, dw, db, loss, slot, ctr)


@pytest.mark.parametrize("splits", [2, 8, 32])
def test_bwd_reduce_slab_exact(C, splits):
    """bn_bwd_reduce_slab: BN rows exact; the slab destination is the exact
    fp64 sum of the integer slabs (pad channels c >= C left out) and equals the
    stand-alone slab_reduce bitwise; its three lanes-per-output instances."""
    case = _int_case((4, 8, 64))
    B, H, Cc = case.shape
    cout, taps, cp, creal = 16, 25, 16, 8
    g = torch.Generator().manual_seed(splits)
    slabs, total = _int_slabs(splits, (cout, taps, cp), g, top=5000, part=3000)
    G = C.bn_bwd_blocks(B, H, H, Cc)
    buf = torch.full((G + 2, 2, Cc), NAN, device="cuda")
    dst, alone = torch.full((cout, taps, creal), NAN, device="cuda"), torch.full((cout, taps, creal), NAN, device="cuda")
    sd = _d(slabs)
    C.bn_bwd_reduce_slab(case.yd.data_ptr(), case.dPd.data_ptr(), case.coefd.data_ptr(), buf.data_ptr(), B, H, H, Cc, G,
                         sd.data_ptr(), dst.data_ptr(), splits, cout, taps, cp, creal, _s())
    C.slab_reduce(sd.data_ptr(), alone.data_ptr(), splits, cout, taps, cp, creal, _s())
    torch.cuda.synchronize()
    rz, rzx = _split_rows(buf, 0, G)
    _assert_rows_exact(case, rz, rzx, "bn_bwd_reduce_slab")
    exact.assert_exact(dst, total[..., :creal], "slab destination")
    assert torch.equal(dst, alone)


@pytest.mark.parametrize("fin_grid", [None, 1], ids=["grid", "grid1"])
@pytest.mark.parametrize("R", [1, 16], ids=["rows1", "rows16"])
def test_bwd_apply_head_exact(C, R, fin_grid):
    """bn_bwd_apply_head at C = 512 (the two-channels-per-thread prologue):
    dy and the totals exact, and the head half's dW / db / loss exact."""
    case = _int_case((8, 4, 512))
    B, H, Cc = case.shape
    F = 264
    h, w, b, lab, ref = _head_int(B, F)
    buf, _, _ = _reduce(C, case, R)
    if fin_grid:
        C.set_bn_fin_grid(fin_grid)
    tot = torch.full((2, Cc), NAN, device="cuda")
    dyp = _bordered(B, H, H, Cc, 2)
    dw, db = torch.full((NC, F), NAN, device="cuda"), torch.full((NC,), NAN, device="cuda")
    loss, slot = torch.full((1,), NAN, device="cuda"), torch.zeros(1, device="cuda")
    ctr = torch.zeros(2, dtype=torch.int64, device="cuda")
    C.bn_bwd_apply_head(case.yd.data_ptr(), case.dPd.data_ptr(), case.coefd.data_ptr(), buf.data_ptr(),
                        case.gammad.data_ptr(), case.M, dyp.data_ptr(), B, H, H, Cc, 2, tot[0].data_ptr(),
                        tot[1].data_ptr(), _d(h).data_ptr(), _d(ref["dlogits"].float()).data_ptr(),
                        _d(ref["loss_b"].float()).data_ptr(), F, NC, dw.data_ptr(), db.data_ptr(), loss.data_ptr(),
                        slot.data_ptr(), ctr.data_ptr(), _s())
    torch.cuda.synchronize()
    exact.assert_exact(tot[0], case.s_dzx, "dgamma_out")
    exact.assert_exact(tot[1], case.s_dz, "dbeta_out")
    case.check_dy(dyp, R, "dy")
    _check_wgrad_exact(ref, dw, db, loss, slot, ctr)


def test_head_pool_exact(C):
    """head_fwd_bwd_pool: the pooled h it writes is the forward reference."""
    case = _int_case((8, 4, 512))
    B, H, Cc = case.shape
    F = 2048
    g = torch.Generator().manual_seed(3)
    w, b = torch.randint(-2, 3, (NC, F), generator=g).float() / 64, torch.zeros(NC)
    lab = torch.randint(0, NC, (B,), generator=g)
    hout = torch.full((B, F), NAN, dtype=BF16, device="cuda")
    logp, dlog = torch.full((B, NC), NAN, device="cuda"), torch.full((B, NC), NAN, device="cuda")
    lb, dh = torch.full((B,), NAN, device="cuda"), torch.full((B, F), NAN, dtype=BF16, device="cuda")
    C.head_fwd_bwd_pool(case.yd.data_ptr(), case.coefd.data_ptr(), H, H, Cc, hout.data_ptr(), _d(w).data_ptr(),
                        _d(b).data_ptr(), _d(lab).data_ptr(), B, NC, logp.data_ptr(), dlog.data_ptr(), lb.data_ptr(),
                        dh.data_ptr(), 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0, _s())
    torch.cuda.synchronize()
    exact.assert_exact(hout.reshape(B, H // 2, H // 2, Cc), case.fwd, "pooled h")
    for t in (logp, dlog, lb, dh):
        assert torch.isfinite(t.float()).all()


# ---------------------------------------------------------------------------
# 3. real-valued BN / ReLU / pool
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["train", "eval", "eval_nobias"])
@pytest.mark.parametrize("shape", REAL_SHAPES, ids=_sid)
def test_bn_finalize_real(C, shape, mode):
    """bn_finalize against bn_coefficients of the same fp32 sums, under
    bn_coefficient_bounds (the invstd bound of the mean-64 channel is a few
    percent, of every ordinary channel below 1e-5 relative); eval mode reads
    rmean - bias and rvar and leaves them alone."""
    B, H, Cc = shape
    y, _, gamma, beta, bias, sums, g = _real_bn_inputs(shape)
    M = B * H * H
    rm0, rv0 = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    rm, rv = _d(rm0), _d(rv0)
    # three partial rows whose fixed-order tree sum stands for the totals
    part = torch.stack([sums * 0.5, sums * 0.25, sums - sums * 0.5 - sums * 0.25])
    coef = torch.full((4, Cc), NAN, device="cuda")
    use_bias = mode != "eval_nobias"
    C.bn_finalize(_d(part).data_ptr(), 3, Cc, M, _d(gamma).data_ptr(), _d(beta).data_ptr(),
                  _d(bias).data_ptr() if use_bias else 0, rm.data_ptr(), rv.data_ptr(), EPS, MOM,
                  0 if mode == "train" else 1, coef.data_ptr(), _s())
    torch.cuda.synchronize()
    ref = xb.assert_coefficients(coef, (rm, rv), part, M, gamma, beta, bias if use_bias else None, EPS, MOM, (rm0, rv0),
                                 0 if mode == "train" else 1)
    if mode == "train":
        _, bnd = xb.bn_coefficient_bounds(part, M, gamma, beta, bias, EPS, MOM, (rm0, rv0))
        rel = bnd["invstd"] / ref["invstd"]
        assert float(rel[2]) < 0.1 and float(rel[3:].max()) < 1e-5, (float(rel[2]), float(rel[3:].max()))
        assert float(coef[2, 3]) == 0.0 and float(coef[3, 3]) == 0.5  # gamma = 0: scale 0, shift beta, exactly
        assert abs(float(ref["invstd"][1]) - EPS ** -0.5) < 0.05  # the constant channel


@pytest.mark.parametrize("R", [1, 16], ids=["rows1", "rows16"])
@pytest.mark.parametrize("shape", REAL_SHAPES + [(9, 8, 64), (2, 4, 1024)], ids=_sid)
def test_fwd_fin_real(C, shape, R):
    """bn_relu_pool_fwd_fin: the published table and running statistics against
    bn_coefficients of the R fp32 rows; the pooled output bitwise from the
    published table.  (9, 8, 64) runs on one block (set_bn_fin_grid(1)): 4 or 5
    items per thread through the prefetch path, with set_bn_minw(1, 1) at R = 1."""
    B, H, Cc = shape
    y, _, gamma, beta, bias, sums, g = _real_bn_inputs(shape)
    M = B * H * H
    frac = torch.rand(R, 1, 1, generator=g) + 0.1
    rows = (sums.unsqueeze(0) * (frac / frac.sum())).contiguous()
    rm0, rv0 = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    rm, rv = _d(rm0), _d(rv0)
    if shape == (9, 8, 64):
        C.set_bn_fin_grid(1)
        if R == 1:
            C.set_bn_minw(1, 1)
    C.set_reduce_atomic(R)
    coef = torch.full((4, Cc), NAN, device="cuda")
    out = _bordered(B, H // 2, H // 2, Cc, 2)
    C.bn_relu_pool_fwd_fin(_d(y).data_ptr(), _d(rows).data_ptr(), M, _d(gamma).data_ptr(), _d(beta).data_ptr(),
                           _d(bias).data_ptr(), rm.data_ptr(), rv.data_ptr(), EPS, MOM, coef.data_ptr(), out.data_ptr(),
                           B, H, H, Cc, 2, _s())
    torch.cuda.synchronize()
    xb.assert_coefficients(coef, (rm, rv), rows, M, gamma, beta, bias, EPS, MOM, (rm0, rv0))
    _check_bordered(out, 2, xb.pool_fwd_ref(y, coef.cpu()), "pooled")


@pytest.mark.parametrize("opad", [0, 2])
@pytest.mark.parametrize("shape", REAL_SHAPES, ids=_sid)
def test_fwd_real_bitwise(C, shape, opad):
    case = _real_case(C, shape)
    B, H, Cc = shape
    out = _bordered(B, H // 2, H // 2, Cc, opad)
    C.bn_relu_pool_fwd(case.yd.data_ptr(), case.coefd.data_ptr(), out.data_ptr(), B, H, H, Cc, opad, _s())
    torch.cuda.synchronize()
    _check_bordered(out, opad, case.fwd, "pooled")


@pytest.mark.parametrize("blocks", [None, 3])
@pytest.mark.parametrize("mode", [0, 1, 16], ids=["rows", "atomic1", "atomic16"])
@pytest.mark.parametrize("shape", REAL_SHAPES, ids=_sid)
def test_bwd_real(C, shape, mode, blocks):
    """Reduce rows within ``sums_bound`` of the fp64 sums of the exactly
    reproduced dz and dz*xhat; dy per element within ``apply_bound`` of the
    reference evaluated from the rows read back (mode 0 through
    bn_bwd_finalize, whose dgamma / dbeta are held to the same sums bound)."""
    case = _real_case(C, shape)
    B, H, Cc = shape
    buf, rz, rzx = _reduce(C, case, mode, blocks, extra_rows=0 if mode == 0 else 2)
    case.check_rows(rz, rzx, "bwd_reduce")
    dyp = _bordered(B, H, H, Cc, 2)
    if mode == 0:
        T = rz.shape[0]
        dg, db = torch.full((Cc,), NAN, device="cuda"), torch.full((Cc,), NAN, device="cuda")
        acoef = torch.full((3, Cc), NAN, device="cuda")
        C.bn_bwd_finalize(buf.data_ptr(), T, Cc, case.M, case.gammad.data_ptr(), case.coefd.data_ptr(), dg.data_ptr(),
                          db.data_ptr(), acoef.data_ptr(), _s())
        C.bn_relu_pool_bwd_apply(case.yd.data_ptr(), case.dPd.data_ptr(), case.coefd.data_ptr(), acoef.data_ptr(),
                                 dyp.data_ptr(), B, H, H, Cc, 2, _s())
        torch.cuda.synchronize()
        case.check_rows(db.cpu().unsqueeze(0), dg.cpu().unsqueeze(0), "bn_bwd_finalize")
    else:
        tot = torch.full((2, Cc), NAN, device="cuda")
        C.bn_relu_pool_bwd_apply_sums(case.yd.data_ptr(), case.dPd.data_ptr(), case.coefd.data_ptr(), buf.data_ptr(),
                                      case.gammad.data_ptr(), case.M, dyp.data_ptr(), B, H, H, Cc, 2, tot[0].data_ptr(),
                                      tot[1].data_ptr(), _s())
        torch.cuda.synchronize()
        case.check_rows(tot[1].cpu().unsqueeze(0), tot[0].cpu().unsqueeze(0), "apply_sums totals")
    case.check_dy(dyp, rz, rzx, "dy")


@pytest.mark.parametrize("mode", [0, 16], ids=["rows", "atomic16"])
@pytest.mark.parametrize("shape", REAL_SHAPES, ids=_sid)
def test_fused_reduces_real(C, shape, mode):
    """The fused forms of the reduce on real data, each within the sums bound:
    combine_bwd_reduce (dP the bf16 rounding of the fp32 slab sum, within one
    fp32 ulp per split of the fp64 sum before rounding), bn_bwd_reduce_slab and
    bn_bwd_reduce_head."""
    case = _real_case(C, shape)
    B, H, Cc = shape
    G = C.bn_bwd_blocks(B, H, H, Cc)
    C.set_reduce_atomic(mode)

    def rows_buf(n):
        return torch.full((n + 2, 2, Cc), NAN, device="cuda") if mode == 0 else torch.zeros(mode, 2, Cc, device="cuda")

    g = torch.Generator().manual_seed(B + Cc)
    # slab / head halves: integer operands (their real-valued checks are in the conv and head tests)
    slabs, total = _int_slabs(8, (16, 25, 16), g, top=5000, part=3000)
    buf, dst = rows_buf(G), torch.full((16, 25, 8), NAN, device="cuda")
    C.bn_bwd_reduce_slab(case.yd.data_ptr(), case.dPd.data_ptr(), case.coefd.data_ptr(), buf.data_ptr(), B, H, H, Cc, G,
                         _d(slabs).data_ptr(), dst.data_ptr(), 8, 16, 25, 16, 8, _s())
    torch.cuda.synchronize()
    case.check_rows(*_split_rows(buf, mode, G), "bn_bwd_reduce_slab")
    exact.assert_exact(dst, total[..., :8], "slab destination")
    F = 264
    if _is_pow2(B):  # the head half divides by B
        h, w, b, lab, ref = _head_int(B, F)
        buf = rows_buf(G)
        dw, db, loss = torch.full((NC, F), NAN, device="cuda"), torch.full((NC,), NAN, device="cuda"), torch.zeros(1).cuda()
        C.bn_bwd_reduce_head(case.yd.data_ptr(), case.dPd.data_ptr(), case.coefd.data_ptr(), buf.data_ptr(), B, H, H, Cc,
                             G, _d(h).data_ptr(), _d(ref["dlogits"].float()).data_ptr(),
                             _d(ref["loss_b"].float()).data_ptr(), F, NC, dw.data_ptr(), db.data_ptr(), loss.data_ptr(),
                             0, 0, _s())
        torch.cuda.synchronize()
        case.check_rows(*_split_rows(buf, mode, G), "bn_bwd_reduce_head")
        _check_wgrad_exact(ref, dw, db, loss)
    # combine: 4 real-valued slabs
    sl = torch.randn(4, B, H // 2, H // 2, Cc, generator=g) * 0.5
    tot64 = sl.double().sum(0)
    nb = C.combine_bwd_reduce_blocks(B, H, H, Cc)
    buf = rows_buf(nb)
    dP = torch.full(tot64.shape, NAN, dtype=BF16, device="cuda")
    assert C.combine_bwd_reduce(_d(sl).data_ptr(), 4, dP.data_ptr(), case.yd.data_ptr(), case.coefd.data_ptr(),
                                buf.data_ptr(), B, H, H, Cc, _s()) == nb
    torch.cuda.synchronize()
    E = 3 * xb.U32 * sl.double().abs().sum(0)  # three fp32 additions
    xb.assert_within(dP, tot64, exact.half_ulp_bf16(tot64.abs() + E) + E, "combined dP")
    s_dz, s_dzx, a_dz, a_dzx = xb.bwd_sums_ref(case.y, dP.cpu(), case.coef)
    rz, rzx = _split_rows(buf, mode, nb)
    xb.assert_within(rz.double().sum(0), s_dz, xb.sums_bound(case.n_pix, a_dz), "combine: sum dz")
    xb.assert_within(rzx.double().sum(0), s_dzx, xb.sums_bound(case.n_pix, a_dzx), "combine: sum dz*xhat")


# ---------------------------------------------------------------------------
# 4. head and head weight gradient
# ---------------------------------------------------------------------------
HEAD_F = [8, 264, 2048, 2056, 4096]


def _head_bufs(B, F):
    return {"logp": torch.full((B, NC), NAN, device="cuda"), "dlog": torch.full((B, NC), NAN, device="cuda"),
            "lb": torch.full((B,), NAN, device="cuda"), "dh": torch.full((B, F), NAN, dtype=BF16, device="cuda"),
            "dw": torch.full((NC, F), NAN, device="cuda"), "db": torch.full((NC,), NAN, device="cuda"),
            "loss": torch.full((1,), NAN, device="cuda"), "slot": torch.zeros(1, device="cuda"),
            "ctr": torch.zeros(2, dtype=torch.int64, device="cuda")}


def _run_head(C, h, w, b, lab, wgrad=True):
    B, F = h.shape
    o = _head_bufs(B, F)
    hd = _d(h)
    C.head_fwd_bwd(hd.data_ptr(), _d(w).data_ptr(), _d(b).data_ptr(), _d(lab).data_ptr() if lab is not None else 0, F, B,
                   NC, o["logp"].data_ptr(), o["dlog"].data_ptr(), o["lb"].data_ptr(), o["dh"].data_ptr(), _s())
    if wgrad:
        C.head_wgrad(hd.data_ptr(), o["dlog"].data_ptr(), o["lb"].data_ptr(), F, B, NC, o["dw"].data_ptr(),
                     o["db"].data_ptr(), o["loss"].data_ptr(), o["slot"].data_ptr(), o["ctr"].data_ptr(), _s())
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("B", [1, 8, 32, 128])
@pytest.mark.parametrize("F", HEAD_F)
def test_head_exact(C, F, B):
    """Saturated integer logits (the largest leads by >= 160): exp of every
    other term is 0 in fp32 and the sum of exponentials is 1, so logp = logit -
    max, loss_b = the gap or 0, dlogits in {0, +-1/B}, dh = (W[max] - W[label])
    / B rounded once, and dW, db, the mean loss are exact.  No NaN / inf."""
    h, w, b, lab, ref = _head_int(B, F)
    o = _run_head(C, h, w, b, lab)
    for k in ("logp", "dlog", "lb", "dh", "dw", "db", "loss"):
        assert torch.isfinite(o[k].float()).all(), k
    exact.assert_exact(o["logp"], ref["logp"], "logp")
    exact.assert_exact(o["dlog"], ref["dlogits"], "dlogits")
    exact.assert_exact(o["lb"], ref["loss_b"], "loss_b")
    exact.assert_exact(o["dh"], ref["dh"], "dh")
    _check_wgrad_exact(ref, o["dw"], o["db"], o["loss"], o["slot"], o["ctr"])


@pytest.mark.parametrize("F", [264, 2048])
def test_head_predict_mode(C, F):
    """labels == 0: log-probabilities only; dlogits, loss_b and dh keep their NaN pre-fill."""
    h, w, b, lab, ref = _head_int(8, F)
    o = _run_head(C, h, w, b, None, wgrad=False)
    exact.assert_exact(o["logp"], ref["logp"], "logp")
    for k in ("dlog", "lb", "dh"):
        assert torch.isnan(o[k].float()).all(), f"{k} was written in predict mode"


def test_head_wgrad_bookkeeping(C):
    """slot == 1.0; step_ctr advances by exactly one per launch; null db / loss
    / slot / step_ctr are accepted and dW is still exact."""
    B, F = 8, 264
    h, w, b, lab, ref = _head_int(B, F)
    hd, dl, lb = _d(h), _d(ref["dlogits"].float()), _d(ref["loss_b"].float())
    o = _head_bufs(B, F)
    for n in (1, 2, 3):
        C.head_wgrad(hd.data_ptr(), dl.data_ptr(), lb.data_ptr(), F, B, NC, o["dw"].data_ptr(), o["db"].data_ptr(),
                     o["loss"].data_ptr(), o["slot"].data_ptr(), o["ctr"].data_ptr(), _s())
        torch.cuda.synchronize()
        _check_wgrad_exact(ref, o["dw"], o["db"], o["loss"], o["slot"], o["ctr"], launches=n)
    dw = torch.full((NC, F), NAN, device="cuda")
    C.head_wgrad(hd.data_ptr(), dl.data_ptr(), lb.data_ptr(), F, B, NC, dw.data_ptr(), 0, 0, 0, 0, _s())
    torch.cuda.synchronize()
    exact.assert_exact(dw, ref["dW"], "dW")


# The fast __expf / __logf of head_fwd_bwd_kernel have no error bound that
# follows from the number formats.  Measured on an MI355X against the fp64
# reference over the 15 cases of test_head_real (F in HEAD_F x B in {5, 37,
# 137}), in units of 2^-23 max(1, largest |logit - max| of the sample): the
# largest error of logp / loss_b (it includes the fp32 dot products, which stay
# far below their worst-case ``logit_bound`` of 10 to 1100 such units) and of
# the softmax (B dlogits + onehot).  Per case logp ranged 1.31 .. 4.25, the
# softmax 0.18 .. 0.76.
MEASURED_LOGP_UNITS = 4.252
MEASURED_SOFTMAX_UNITS = 0.761
# Allowed: 4 x the measured value (one seed samples few arguments of the two
# intrinsics).  test_head_real asserts that this stays inside what test_head
# grants (rtol = atol = 1e-4): at most 17 x 2^-23 x 8 = 1.6e-5 here.
ALLOW_LOGP_UNITS = 4 * MEASURED_LOGP_UNITS
ALLOW_SOFTMAX_UNITS = 4 * MEASURED_SOFTMAX_UNITS


def _head_real_inputs(B, F):
    g = torch.Generator().manual_seed(B * 10000 + F)
    h = torch.randn(B, F, generator=g).to(BF16)
    w, b = torch.randn(NC, F, generator=g) * 0.02, torch.randn(NC, generator=g) * 0.1
    return h, w, b, torch.randint(0, NC, (B,), generator=g)


@pytest.mark.parametrize("B", [5, 37, 137])
@pytest.mark.parametrize("F", HEAD_F)
def test_head_real(C, F, B, record_property):
    """Real-valued inputs (those of test_head), per element against fp64.

    logp, loss_b and the softmax behind dlogits: the measured allowance above,
    in units u_b = 2^-23 max(1, spread_b) of the sample; dlogits = (softmax -
    onehot) / B scales it by 1 / B.  The derived worst case of the linear part
    alone (``logit_bound``, logit_depth(F) roundings; log-sum-exp is
    1-Lipschitz in the largest logit error, so logp carries twice that) is
    looser than the allowance from F = 264 on, which is asserted: the
    allowance is the binding check.
    dh, from the dlogits the kernel wrote: 10 products and 10 additions, 20
    2^-23 sum_c |d_c w_cj|, then one bf16 rounding.
    dW, from the same dlogits: ceil(B/8) products and additions per row group
    and the 8-group sum, (2 ceil(B/8) + 8) 2^-23 sum_b |d_bc h_bj|.
    db / loss: at most ceil(B/256) + 256 additions (+ the division).
    The figures are printed before anything is asserted."""
    h, w, b, lab = _head_real_inputs(B, F)
    ref = xb.head_ref(h, w, b, lab)
    o = _run_head(C, h, w, b, lab)
    e_b = 2 * xb.logit_bound(ref, F).max(1, keepdim=True).values
    u_b = xb.U32 * ref["spread"].clamp_min(1.0).unsqueeze(1)
    onehot = torch.nn.functional.one_hot(lab, NC).double()
    err_lp = (o["logp"].cpu().double() - ref["logp"]).abs()
    err_lb = (o["lb"].cpu().double() - ref["loss_b"]).abs().unsqueeze(1)
    err_sm = (o["dlog"].cpu().double() * B + onehot - ref["softmax"]).abs()
    meas = {"logp_units": float((torch.maximum(err_lp, err_lb) / u_b).max()),
            "softmax_units": float((err_sm / u_b).max()), "linear_bound_units": float((e_b / u_b).max())}
    print(f"head_real F={F} B={B}: " + " ".join(f"{k}={v:.3f}" for k, v in meas.items()))
    for k, v in meas.items():
        record_property(k, v)
    # the allowance stays inside what test_head grants (rtol = atol = 1e-4)
    assert float((ALLOW_LOGP_UNITS * u_b).max()) <= 1e-4 and float((ALLOW_SOFTMAX_UNITS * u_b).max()) <= 1e-4
    assert F < 264 or bool((ALLOW_LOGP_UNITS * u_b <= e_b).all())
    xb.assert_within(o["logp"], ref["logp"], ALLOW_LOGP_UNITS * u_b, "logp")
    xb.assert_within(o["lb"], ref["loss_b"], (ALLOW_LOGP_UNITS * u_b).squeeze(1), "loss_b")
    xb.assert_within(o["dlog"], ref["dlogits"], ALLOW_SOFTMAX_UNITS * u_b / B, "dlogits")
    gr = xb.head_grads_ref(h, w, o["dlog"])
    E = 20 * xb.U32 * gr["S_dh"]
    xb.assert_within(o["dh"], gr["dh"], exact.half_ulp_bf16(gr["dh"].abs() + E) + E, "dh")
    xb.assert_within(o["dw"], gr["dW"], (2 * ((B + 7) // 8) + 8) * xb.U32 * gr["S_dW"], "dW")
    n_sum = (B + 255) // 256 + 256
    xb.assert_within(o["db"], gr["db"], n_sum * xb.U32 * gr["S_db"], "db")
    lb64 = o["lb"].cpu().double()
    xb.assert_within(o["loss"], lb64.mean().reshape(1), (n_sum + 1) * xb.U32 * lb64.abs().mean().reshape(1), "loss")
    assert float(o["slot"]) == 1.0 and o["ctr"].tolist() == [1, 0]


def test_head_pool_fused_finalize_reduce_real(C):
    """head_fwd_bwd_pool with the fused finalize and the fused BN backward
    reduce (R = 16, C = 512, H = 4) on real data: the published table as in
    test_fwd_fin_real, h bitwise the forward reference from that table, the
    head's outputs within the bounds of test_head_real for that h, and the 16
    accumulated rows within the sums bound of the reference sums over the bf16
    dh the kernel wrote."""
    R, shape = 16, (16, 4, 512)
    B, H, Cc = shape
    F = 2048
    y, _, gamma, beta, bias, sums, g = _real_bn_inputs(shape, seed=1)
    M = B * H * H
    frac = torch.rand(R, 1, 1, generator=g) + 0.1
    rows = (sums.unsqueeze(0) * (frac / frac.sum())).contiguous()
    rm0, rv0 = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    rm, rv = _d(rm0), _d(rv0)
    w, b = torch.randn(NC, F, generator=g) * 0.02, torch.randn(NC, generator=g) * 0.1
    lab = torch.randint(0, NC, (B,), generator=g)
    C.set_reduce_atomic(R)
    coef = torch.full((4, Cc), NAN, device="cuda")
    o = _head_bufs(B, F)
    hout = torch.full((B, F), NAN, dtype=BF16, device="cuda")
    red = torch.zeros(R, 2, Cc, device="cuda")
    yd = _d(y)
    C.head_fwd_bwd_pool(yd.data_ptr(), coef.data_ptr(), H, H, Cc, hout.data_ptr(), _d(w).data_ptr(), _d(b).data_ptr(),
                        _d(lab).data_ptr(), B, NC, o["logp"].data_ptr(), o["dlog"].data_ptr(), o["lb"].data_ptr(),
                        o["dh"].data_ptr(), _d(rows).data_ptr(), M, _d(gamma).data_ptr(), _d(beta).data_ptr(),
                        _d(bias).data_ptr(), rm.data_ptr(), rv.data_ptr(), EPS, MOM, red.data_ptr(), _s())
    torch.cuda.synchronize()
    xb.assert_coefficients(coef, (rm, rv), rows, M, gamma, beta, bias, EPS, MOM, (rm0, rv0))
    coef = coef.cpu()
    exact.assert_exact(hout.reshape(B, H // 2, H // 2, Cc), xb.pool_fwd_ref(y, coef), "pooled h")
    hh = hout.cpu()
    ref = xb.head_ref(hh, w, b, lab)
    u_b = xb.U32 * ref["spread"].clamp_min(1.0).unsqueeze(1)
    xb.assert_within(o["logp"], ref["logp"], ALLOW_LOGP_UNITS * u_b, "logp")
    xb.assert_within(o["lb"], ref["loss_b"], (ALLOW_LOGP_UNITS * u_b).squeeze(1), "loss_b")
    xb.assert_within(o["dlog"], ref["dlogits"], ALLOW_SOFTMAX_UNITS * u_b / B, "dlogits")
    gr = xb.head_grads_ref(hh, w, o["dlog"])
    E = 20 * xb.U32 * gr["S_dh"]
    xb.assert_within(o["dh"], gr["dh"], exact.half_ulp_bf16(gr["dh"].abs() + E) + E, "dh")
    dP = o["dh"].cpu().reshape(B, H // 2, H // 2, Cc)
    s_dz, s_dzx, a_dz, a_dzx = xb.bwd_sums_ref(y, dP, coef)
    rz, rzx = _split_rows(red, R, B)
    n_pix = B * (H // 2) ** 2
    xb.assert_within(rz.double().sum(0), s_dz, xb.sums_bound(n_pix, a_dz), "fused reduce: sum dz")
    xb.assert_within(rzx.double().sum(0), s_dzx, xb.sums_bound(n_pix, a_dzx), "fused reduce: sum dz*xhat")


def test_leaves_defaults_behind(C):
    """After the file's tests the process is in reduction mode 0 (the fixture's
    teardown); the grid defaults are observable through bn_bwd_blocks."""
    assert C.reduce_atomic() == 0
    assert C.bn_bwd_blocks(36, 8, 8, 64) == (4608 + 511) // 512
