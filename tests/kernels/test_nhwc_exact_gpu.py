"""The ResNet-50 path's non-conv kernels -- channels-last BatchNorm
(bn_nhwc.hip), channels-last max pool (pool_nhwc.hip) and the glue kernels
(resnet_glue.hip) -- against the CPU references of tests/kernels/exact_nhwc.py.

The native launchers are called directly with raw pointers, so every argument
combination is reachable; a few cases go through ops.bn_nhwc.bn_act,
ops.pool.max_pool2d_nhwc and ops.head.ResNetHeadNLL to pin the pointer
arithmetic of the Python layer (ybase / dxbase of padded buffers, the
acc4[2C:] slice, the weight-gradient view).

Exact regime: integer bf16 data and dyadic parameters, every output bit for
bit.  Real regime: bitwise wherever the kernels spell their roundings out
(forward apply, ReLU decisions, pool, pool backward, the glue layouts and
sequential sums), per element under a derived bound elsewhere (BN statistics,
backward sums, dx).  The BN row counts come from ``exact_nhwc.bn_loops``, which
evaluates make_geom's formulas: each test asserts that its set of M reaches
every loop of the kernels."""
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.kernels import exact
from tests.kernels import exact_bn_head as xb
from tests.kernels import exact_nhwc as xn
from tests.kernels.exact_update import fma32

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NAN = float("nan")
EPS, MOM = 1e-3, 0.1
SENT = 3.0  # border sentinel of padded outputs


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from torch_distlearn_amd import _native

    return _native.native()


@pytest.fixture(autouse=True)
def _bn_settings(request):
    """set_bn_tuning / set_bn_reduce_blocks are process-wide: every test leaves the defaults behind."""
    yield
    if "C" in request.fixturenames:
        torch.cuda.synchronize()
        _KEEP.clear()
        nat = request.getfixturevalue("C")
        nat.set_bn_tuning(4, 256)
        nat.set_bn_reduce_blocks(256)


_KEEP = []  # the kernels get raw pointers: device tensors must outlive the launch


def _s():
    from torch_distlearn_amd._native import stream_handle

    return stream_handle()


def _d(t):
    _KEEP.append(t.to("cuda").contiguous())
    return _KEEP[-1]


def _new(shape, fill, dtype=torch.float32):
    _KEEP.append(torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), fill, dtype=dtype, device="cuda"))
    return _KEEP[-1]


def _p(t):
    return t.data_ptr() if t is not None else 0


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def _real_bf16(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(BF16)


# ---------------------------------------------------------------------------
# bn_nhwc.hip
# ---------------------------------------------------------------------------
ALL_LOOPS = {"rem_only", "u+1", "u+2", "u+3", "idle", "small", "blocks"}


def _edge_rows(Cc, nt=256, blocks=256):
    """Row counts, from make_geom's formulas with R = RPI = nt / min(C/8, 32)
    (one row block up to 16 R rows):
      1          M < RPI, single-row remainder loop only, idle lanes
      R - 1      the same with all but one lane busy
      3 R + 2    three or four single rows per lane, never the 4-row loop
      4 R + 1    lane 0: one 4-row iteration + 1 remainder row, the rest + 0
      6 R + 3    lanes 0..2: 4 + 3, the rest 4 + 2; the last iteration cut by min(M, ..)
      16 R + 5   two row blocks of 9 R rows: block 0 is 2 x 4 + 1 per lane, block 1
                 (7 R + 5 rows) 4 + 3 and 4 + 4 with idle lanes
    asserted against ``bn_loops`` rather than trusted."""
    R = xn.bn_geom(1, Cc, blocks, nt)["RPI"]
    rows = [1, R - 1, 3 * R + 2, 4 * R + 1, 6 * R + 3, 16 * R + 5]
    seen = set()
    for M in rows:
        seen |= xn.bn_loops(M, Cc, blocks, nt)
    want = ALL_LOOPS | ({"groups"} if Cc >= 512 else set())
    assert seen >= want, (Cc, nt, rows, want - seen)
    return rows


def _params(Cc, g, dyadic=False):
    """gamma with negative entries and gamma[2] = 0, beta; running statistics before the call."""
    if dyadic:
        w = torch.pow(2.0, torch.randint(-1, 2, (Cc,), generator=g).float())
        b = torch.randint(-4, 5, (Cc,), generator=g).float() / 2
    else:
        w, b = torch.randn(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g)
    w = w * torch.where(torch.rand(Cc, generator=g) < 0.3, -1.0, 1.0)
    w[2] = 0.0
    w[1] = -w[1].abs() - 0.25
    return w.float(), b.float(), (torch.linspace(-1, 1, Cc), torch.linspace(0.5, 2, Cc))


def _fwd(C, x, w, b, relu, res=None, acc=None, running=None, geom=None, opad=0, mbits=False, rbn=None):
    """One bn_nhwc_fwd_pad launch.  acc given: have_stats = 1.  geom = (N, H, W)
    with opad.  rbn: dict(acc, w, b, running) of the residual BN (ResBn)."""
    M, Cc = x.shape
    o = SimpleNamespace(M=M, C=Cc)
    xd, wd, bd = _d(x), _d(w), _d(b)
    resd = _d(res) if res is not None else None
    o.acc = _d(acc.float()) if acc is not None else _new(2 * Cc, 0.0)
    o.save = _new(2 * Cc, NAN)
    o.rm, o.rv = (_d(running[0].clone()), _d(running[1].clone())) if running is not None else (None, None)
    N, H, W = geom if opad else (1, 1, 1)
    o.ybuf = _new((N, H + 2 * opad, W + 2 * opad, Cc), SENT, BF16) if opad else _new((M, Cc), NAN, BF16)
    o.mbits = _new(M * Cc // 8, 0xAA, torch.uint8) if mbits else None
    kw = {}
    if rbn is not None:
        o.rsave = _new(2 * Cc, NAN)
        o.rrm, o.rrv = _d(rbn["running"][0].clone()), _d(rbn["running"][1].clone())
        kw = dict(rbn_acc=_d(rbn["acc"].float()).data_ptr(), rbn_w=_d(rbn["w"]).data_ptr(),
                  rbn_b=_d(rbn["b"]).data_ptr(), rbn_save=o.rsave.data_ptr(), rbn_rm=o.rrm.data_ptr(),
                  rbn_rv=o.rrv.data_ptr(), rbn_eps=2 * EPS, rbn_momentum=0.25)
    C.bn_nhwc_fwd_pad(xd.data_ptr(), _p(resd), o.ybuf.data_ptr(), o.acc.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                      o.save.data_ptr(), _p(o.rm), _p(o.rv), M, Cc, EPS, MOM, int(relu), int(acc is not None), H, W,
                      opad, _s(), _p(o.mbits), **kw)
    torch.cuda.synchronize()
    if opad:
        yb = o.ybuf.cpu()
        o.y = yb[:, opad:opad + H, opad:opad + W].reshape(M, Cc)
        border = torch.ones(yb.shape[1:3], dtype=torch.bool)
        border[opad:opad + H, opad:opad + W] = False
        assert bool((yb[:, border] == SENT).all()), "the border of the padded output was written"
    else:
        o.y = o.ybuf.cpu()
    return o


def _check_fwd(o, x, w, b, relu, running, res=None, rbn=None, exact_stats=False, what="fwd"):
    """Statistics, published values and y of one forward launch."""
    M, Cc = x.shape
    acc = o.acc.cpu()
    if exact_stats:
        exact.assert_exact(acc, xn.bn_stats_exact(x).reshape(-1), f"{what}: acc")
    else:  # fp32 summation in any order: M roundings of partial sums within sum |term| (+ the fma of x^2)
        s = xn.bn_stats64(x)
        sabs = torch.stack([xb.cpu64(x).abs().sum(0), (xb.cpu64(x) ** 2).sum(0)])
        xb.assert_within(acc.reshape(2, Cc), s, (M + 1) * xb.U32 * sabs, f"{what}: acc")
    ra = (o.rm.cpu(), o.rv.cpu()) if running is not None else None
    xn.assert_published(o.save, ra, acc, M, w, b, EPS, MOM, running, what)
    sc, sh = xn.coef_from_save(o.save, w, b)
    rsc = rsh = None
    if rbn is not None:
        xn_ref, bnd = xn.published_bounds(rbn["acc"].float(), M, rbn["w"], rbn["b"], 2 * EPS, 0.25, rbn["running"])
        rs = xb.cpu64(o.rsave)
        xb.assert_within(rs[:Cc], xn_ref["mean"], bnd["mean"], f"{what}: residual BN mean")
        xb.assert_within(rs[Cc:], xn_ref["invstd"], bnd["invstd"], f"{what}: residual BN invstd")
        xb.assert_within(o.rrm, xn_ref["rmean"], bnd["rmean"], f"{what}: residual BN running mean")
        xb.assert_within(o.rrv, xn_ref["rvar"], bnd["rvar"], f"{what}: residual BN running var")
        rsc, rsh = xn.coef_from_save(o.rsave, rbn["w"], rbn["b"])
    yref = xn.bn_fwd_ref(x, sc, sh, relu, res, rsc, rsh)
    xn.same_values(o.y, yref, f"{what}: y")
    if o.mbits is not None:
        assert np.array_equal(o.mbits.cpu().numpy().reshape(M, Cc // 8), xn.mask_bits_ref(yref)), f"{what}: mask bits"
    return yref


TUNINGS = [(256, 256, 4), (512, 256, 2), (1024, 256, 4), (256, 64, 4)]  # reduce threads, reduce blocks, apply rows


@pytest.mark.parametrize("Cc", [8, 16, 64, 256, 512])
def test_bn_fwd_integer_edges(C, Cc):
    """Integer x in [-4, 4] (channel 0 constant: var = 0) at every loop edge of
    the statistics and apply kernels: acc bit for bit, save / running within
    the coefficient bounds, y bitwise from the published save."""
    w, b, running = _params(Cc, _gen("p", Cc))
    for i, M in enumerate(_edge_rows(Cc)):
        x = exact.int_bf16((M, Cc), -4, 4, generator=_gen("x", Cc, M))
        x[:, 0] = 3.0
        o = _fwd(C, x, w, b, relu=i % 2 == 0, running=running)
        _check_fwd(o, x, w, b, i % 2 == 0, running, exact_stats=True, what=f"C={Cc} M={M}")


@pytest.mark.parametrize("nt,blocks,rows", TUNINGS[1:])
@pytest.mark.parametrize("Cc", [64, 256])
def test_bn_fwd_integer_tuned(C, Cc, nt, blocks, rows):
    """The other template instances: reduce threads 512 / 1024, apply rows 2,
    and 64 reduce blocks (a row count past 64 * 16 RPI, where the cap changes
    the geometry against the default, asserted)."""
    C.set_bn_tuning(rows, nt)
    C.set_bn_reduce_blocks(blocks)
    w, b, running = _params(Cc, _gen("p", Cc))
    Ms = _edge_rows(Cc, nt, blocks)
    if blocks == 64:
        R = xn.bn_geom(1, Cc, blocks, nt)["RPI"]
        big = 64 * 16 * R + 16 * R + 9  # more than 64 blocks of 16 R rows: capped at 64, not at 256
        assert xn.bn_geom(big, Cc, 64, nt)["rb"] != xn.bn_geom(big, Cc, 256, nt)["rb"]
        Ms = Ms[2:] + [big]
    else:
        Ms = Ms[1:]
        assert xn.bn_geom(Ms[0], Cc, blocks, nt)["RPI"] != xn.bn_geom(Ms[0], Cc, blocks, 256)["RPI"]
    for i, M in enumerate(Ms):
        x = exact.int_bf16((M, Cc), -4, 4, generator=_gen("x", Cc, M))
        o = _fwd(C, x, w, b, relu=i % 2 == 1, running=running)
        _check_fwd(o, x, w, b, i % 2 == 1, running, exact_stats=True, what=f"C={Cc} M={M} nt={nt}")


def _real_x(M, Cc, g):
    """Random bf16 rows; channel 0 constant, channel 1 the period-6 pattern
    63.75, 63.75, 64.5, 64, 64, 64 (mean 64 and variance 1/16 when 6 | M: the
    cancellation case of sumsq/M - mean^2)."""
    x = _real_bf16((M, Cc), g, 2.0)
    x[:, 0] = -1.5
    x[:, 1] = torch.tensor([63.75, 63.75, 64.5, 64.0, 64.0, 64.0]).repeat(M // 6 + 1)[:M].to(BF16)
    return x


@pytest.mark.parametrize("have_stats", [0, 1])
@pytest.mark.parametrize("resk", ["none", "plain", "resbn"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("M,Cc", [(1, 8), (774, 64), (301, 512)])
def test_bn_fwd_real(C, M, Cc, relu, resk, have_stats):
    """Real-valued data with the constant and the mean-64 channel, negative
    and zero gamma; residual none / plain / BN applied on load (ResBn); the
    statistics from the kernel or from the host; mask bits with a residual."""
    g = _gen("real", M, Cc)
    x = _real_x(M, Cc, g)
    w, b, running = _params(Cc, g)
    res = _real_bf16((M, Cc), g) if resk != "none" else None
    rbn = None
    if resk == "resbn":
        rw, rb_, rrun = _params(Cc, _gen("r", Cc))
        rbn = {"acc": xn.bn_stats64(res).reshape(-1), "w": rw, "b": rb_, "running": rrun}
    acc = xn.bn_stats64(x).reshape(-1) if have_stats else None
    o = _fwd(C, x, w, b, relu, res=res, acc=acc, running=running, mbits=bool(relu and res is not None), rbn=rbn)
    _check_fwd(o, x, w, b, relu, running, res, rbn, what=f"M={M} C={Cc}")


def test_bn_fwd_null_running_and_host_checks(C):
    """run_mean = 0: nothing but save is published; mask bits without the
    ReLU, unsupported channel counts and M >= 2^24 with a padded output raise
    before anything is launched (the outputs keep their fill)."""
    g = _gen("null")
    x = _real_x(37, 16, g)
    w, b, _ = _params(16, g)
    o = _fwd(C, x, w, b, True, running=None)
    _check_fwd(o, x, w, b, True, None, what="null running")
    y, acc, save = _new((64, 264), NAN, BF16), _new(2 * 264, 0.0), _new(2 * 264, NAN)
    xd, wd, mb = _new((64, 264), 1.0, BF16), _new(264, 1.0), _new(64 * 33, 0xAA, torch.uint8)
    for Cbad in (24, 264):
        with pytest.raises(RuntimeError):
            C.bn_nhwc_fwd_pad(xd.data_ptr(), 0, y.data_ptr(), acc.data_ptr(), wd.data_ptr(), wd.data_ptr(),
                              save.data_ptr(), 0, 0, 64, Cbad, EPS, MOM, 1, 0, 1, 1, 0, _s())
        with pytest.raises(RuntimeError):
            C.bn_nhwc_bwd_pad(xd.data_ptr(), 0, xd.data_ptr(), save.data_ptr(), wd.data_ptr(), wd.data_ptr(),
                              acc.data_ptr(), y.data_ptr(), 0, wd.data_ptr(), wd.data_ptr(), 64, Cbad, 0, 1, 1, 0, _s())
    with pytest.raises(RuntimeError):  # mask bits need the ReLU
        C.bn_nhwc_fwd_pad(xd.data_ptr(), 0, y.data_ptr(), acc.data_ptr(), wd.data_ptr(), wd.data_ptr(),
                          save.data_ptr(), 0, 0, 64, 8, EPS, MOM, 0, 0, 1, 1, 0, _s(), mb.data_ptr())
    with pytest.raises(RuntimeError):  # M >= 2^24 with opad: out_row's float division is not exact any more
        C.bn_nhwc_fwd_pad(xd.data_ptr(), 0, y.data_ptr(), acc.data_ptr(), wd.data_ptr(), wd.data_ptr(),
                          save.data_ptr(), 0, 0, 1 << 24, 8, EPS, MOM, 1, 1, 4096, 4096, 1, _s())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.float()).all()) and bool(torch.isnan(save).all()) and bool((acc == 0).all())
    assert bool((mb == 0xAA).all())


@pytest.mark.parametrize("opad", [1, 2])
@pytest.mark.parametrize("N,H,W,Cc", [(5, 1, 1, 64), (7, 3, 5, 64), (3, 7, 7, 16), (3, 13, 9, 8), (1, 56, 56, 16),
                                      (3, 5, 11, 8), (2, 3, 41, 16)])
def test_bn_fwd_padded_output(C, N, H, W, Cc, opad):
    """The padded output layout: the interior equals the (bitwise checked)
    unpadded result, every border element keeps the sentinel; mask bits stay
    indexed by the input row.  out_row's correction steps are needed by the
    last two shapes only (5 x 11: the image index comes out one too small from
    row 55 on; 3 x 41: so does the row inside the image), which is asserted."""
    M = N * H * W
    assert M % xn.bn_geom(M, Cc)["RPI"] != 0
    assert xn.out_row_corrections(H, W, M) == {(5, 11): (True, False), (3, 41): (True, True)}.get((H, W), (False, False))
    g = _gen("pad", N, H, W, Cc)
    x, res = _real_bf16((M, Cc), g, 2.0), _real_bf16((M, Cc), g)
    w, b, running = _params(Cc, g)
    for rows in (4, 2):
        C.set_bn_tuning(rows, 256)
        o = _fwd(C, x, w, b, True, res=res, running=running, geom=(N, H, W), opad=opad, mbits=True)
        _check_fwd(o, x, w, b, True, running, res, what=f"opad={opad} rows={rows}")


def test_bn_fwd_padded_output_large(C):
    """out_row's float-reciprocal division up to the largest row index the host
    admits: C = 8, opad = 1, 57 x 59 images (H W odd), M = 4988 * 3363 just
    below 2^24.  The rows encode their index (3 bits per channel), so no two
    rows agree; the reference is the kernel's own unpadded output (no out_row
    there; bitwise checked against the CPU at the small shapes) moved into the
    padded layout by torch indexing on the device."""
    N, H, W, Cc = 4988, 57, 59, 8
    M = N * H * W
    assert (1 << 24) - H * W < M < (1 << 24)
    m = torch.arange(M, dtype=torch.int32, device="cuda").unsqueeze(1)
    x = ((m >> (3 * torch.arange(8, dtype=torch.int32, device="cuda"))) & 7).to(BF16)
    del m
    w, b = _new(Cc, 1.0), _new(Cc, 0.5)
    acc = torch.stack([x.float().sum(0), (x.float() ** 2).sum(0)]).reshape(-1).contiguous()
    save = _new(2 * Cc, NAN)
    y0 = torch.empty((M, Cc), dtype=BF16, device="cuda")
    yp = torch.full((N, H + 2, W + 2, Cc), SENT, dtype=BF16, device="cuda")
    for y, opad in ((y0, 0), (yp, 1)):
        C.bn_nhwc_fwd_pad(x.data_ptr(), 0, y.data_ptr(), acc.data_ptr(), w.data_ptr(), b.data_ptr(), save.data_ptr(),
                          0, 0, M, Cc, EPS, MOM, 0, 1, H, W, opad, _s())
    torch.cuda.synchronize()
    s = save.cpu()
    approx = (x.float() - s[:Cc].cuda()) * s[Cc:].cuda() + 0.5
    assert float((y0.float() - approx).abs().max()) < 0.05  # the unpadded launch did apply the BN to every row
    assert torch.equal(yp[:, 1:-1, 1:-1].reshape(M, Cc), y0), "interior of the padded output"
    for edge in (yp[:, 0], yp[:, -1], yp[:, :, 0], yp[:, :, -1]):
        assert bool((edge == SENT).all()), "border of the padded output"


def _bwd(C, d, mode, y=None, bits=None, acc=None, want_dres=False, rb=False, geom=None, opad=0):
    """One bn_nhwc_bwd_pad launch on the case dict d (x, dy, save, w, b [, xr,
    rsave, rw]).  acc given: have_sums = 1."""
    M, Cc = d["x"].shape
    o = SimpleNamespace()
    o.acc = _d(acc.float()) if acc is not None else _new(2 * Cc, 0.0)
    N, H, W = geom if opad else (1, 1, 1)
    o.dxbuf = _new((N, H + 2 * opad, W + 2 * opad, Cc), SENT, BF16) if opad else _new((M, Cc), NAN, BF16)
    o.dres = _new((M, Cc), NAN, BF16) if (want_dres or rb) else None
    o.dw, o.db = _new(Cc, NAN), _new(Cc, NAN)
    kw = {}
    if rb:
        o.racc, o.rdw, o.rdb = _new(2 * Cc, 0.0), _new(Cc, NAN), _new(Cc, NAN)
        kw = dict(rbn_x=_d(d["xr"]).data_ptr(), rbn_save=_d(d["rsave"]).data_ptr(), rbn_w=_d(d["rw"]).data_ptr(),
                  rbn_acc=o.racc.data_ptr(), rbn_dw=o.rdw.data_ptr(), rbn_db=o.rdb.data_ptr())
    C.bn_nhwc_bwd_pad(_d(d["dy"]).data_ptr(), _p(_d(y) if y is not None else None), _d(d["x"]).data_ptr(),
                      _d(d["save"]).data_ptr(), _d(d["w"]).data_ptr(), _d(d["b"]).data_ptr(), o.acc.data_ptr(),
                      o.dxbuf.data_ptr(), _p(o.dres), o.dw.data_ptr(), o.db.data_ptr(), M, Cc, mode, H, W, opad, _s(),
                      int(acc is not None), _p(_d(bits) if bits is not None else None), **kw)
    torch.cuda.synchronize()
    if opad:
        b = o.dxbuf.cpu()
        o.dx = b[:, opad:opad + H, opad:opad + W].reshape(M, Cc)
        border = torch.ones(b.shape[1:3], dtype=torch.bool)
        border[opad:opad + H, opad:opad + W] = False
        assert bool((b[:, border] == SENT).all()), "the border of the padded dx was written"
    else:
        o.dx = o.dxbuf.cpu()
    return o


def _mode_inputs(d, mode, g):
    """(y, bits, mask) of relu mode ``mode``: mode 1 reads a y with zeros, mode 3 random bits."""
    M, Cc = d["x"].shape
    sc, sh = xn.coef_from_save(d["save"], d["w"], d["b"])
    y = exact.int_bf16((M, Cc), 0, 3, density=0.6, generator=g) if mode == 1 else None
    bits = torch.randint(0, 256, (M * Cc // 8,), generator=g, dtype=torch.uint8) if mode == 3 else None
    mask = xn.relu_mask(mode, d["x"], sc, sh, y, bits.numpy() if bits is not None else None)
    return y, bits, torch.from_numpy(mask)


def _check_bwd_exact(C, d, mode, g, what, geom=None):
    """The exact regime of one (case, mode): sums bit for bit, dw / db = acc,
    dres = g bitwise, dx = a g with zero sums (padded when geom is given), and
    at power-of-two M the whole dx; ResBnBwd alongside for modes 1 and 3."""
    M, Cc = d["x"].shape
    y, bits, mask = _mode_inputs(d, mode, g)
    if mode == 2:
        z = xb.cpu64(d["x"]) * xb.cpu64(d["w"]) * xb.cpu64(d["save"][Cc:]) + (
            xb.cpu64(d["b"]) - xb.cpu64(d["save"][:Cc]) * xb.cpu64(d["w"]) * xb.cpu64(d["save"][Cc:]))
        assert M < 64 or bool((z == 0).any()), "mode 2 needs pre-activations of exactly 0"
        assert bool((torch.from_numpy(xn.np32(z.float()) > 0) == mask).all())
    gv = xb.cpu64(d["dy"]) * mask
    sums, _ = xn.bn_bwd_sums(gv, d["x"], d["save"], exact_regime=True)
    pow2 = M & (M - 1) == 0
    rb = mode in (1, 3)
    o = _bwd(C, d, mode, y, bits, want_dres=rb, rb=False)
    exact.assert_exact(o.acc.cpu(), sums.reshape(-1), f"{what}: acc")
    assert torch.equal(o.db.cpu(), o.acc.cpu()[:Cc]) and torch.equal(o.dw.cpu(), o.acc.cpu()[Cc:]), f"{what}: dw / db"
    if rb:
        exact.assert_exact(o.dres.cpu(), gv, f"{what}: dres")
    if pow2:
        dx, _ = xn.bn_dx64(gv, d["x"], d["save"], d["w"], sums, M, exact_regime=True)
        exact.assert_exact(o.dx, dx, f"{what}: dx")
    if rb:  # the residual BN's backward riding this one
        r = _bwd(C, d, mode, y, bits, rb=True)
        rsums, _ = xn.bn_bwd_sums(gv, d["xr"], d["rsave"], exact_regime=True)
        exact.assert_exact(r.acc.cpu(), sums.reshape(-1), f"{what}: acc (ResBnBwd)")
        exact.assert_exact(r.racc.cpu(), rsums.reshape(-1), f"{what}: rb.acc")
        assert torch.equal(r.rdb.cpu(), r.racc.cpu()[:Cc]) and torch.equal(r.rdw.cpu(), r.racc.cpu()[Cc:])
        if pow2:
            dr, _ = xn.bn_dx64(gv, d["xr"], d["rsave"], d["rw"], rsums, M, exact_regime=True)
            exact.assert_exact(r.dres.cpu(), dr, f"{what}: dres (ResBnBwd)")
            exact.assert_exact(r.dx, xn.bn_dx64(gv, d["x"], d["save"], d["w"], sums, M)[0], f"{what}: dx (ResBnBwd)")
    # zero sums given: dx = a g exactly at any M -- routing, masks, tails, padding
    z = _bwd(C, d, mode, y, bits, acc=torch.zeros(2 * Cc), want_dres=rb, geom=geom, opad=1 if geom else 0)
    a = xb.cpu64(d["w"]) * xb.cpu64(d["save"][Cc:])
    exact.assert_exact(z.dx.contiguous(), a * gv, f"{what}: dx with zero sums")
    assert bool((z.dw.cpu() == 0).all()) and bool((z.db.cpu() == 0).all())
    if rb:
        exact.assert_exact(z.dres.cpu(), gv, f"{what}: dres with zero sums")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("Cc", [8, 16, 64, 256, 512])
def test_bn_bwd_exact_edges(C, Cc, mode):
    for M in _edge_rows(Cc):
        g = _gen("bwd", Cc, M)
        _check_bwd_exact(C, xn.int_bn_bwd_inputs(M, Cc, g), mode, g, f"C={Cc} M={M} mode={mode}")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("nt,blocks,rows", TUNINGS[1:])
def test_bn_bwd_exact_tuned(C, nt, blocks, rows, mode):
    C.set_bn_tuning(rows, nt)
    C.set_bn_reduce_blocks(blocks)
    Cc = 64
    Ms = _edge_rows(Cc, nt, blocks)[2:]
    if blocks == 64:
        Ms = Ms + [64 * 16 * 32 + 16 * 32 + 9]
    for M in Ms:
        g = _gen("bwd", Cc, M)
        _check_bwd_exact(C, xn.int_bn_bwd_inputs(M, Cc, g), mode, g, f"C={Cc} M={M} mode={mode} nt={nt}")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("N,H,W,Cc", [(1, 1, 1, 8), (4, 4, 4, 64), (16, 8, 8, 16), (2, 32, 32, 512), (3, 7, 5, 64),
                                      (3, 5, 11, 8), (2, 3, 41, 16)])
def test_bn_bwd_exact_pow2_and_padded(C, N, H, W, Cc, mode):
    """Power-of-two M (the first four shapes): the whole dx and the residual
    BN's input gradient are exact; every shape also writes the zero-sums dx
    into a padded buffer (opad = 1) with a sentinel border; the last two need
    out_row's correction steps (``out_row_corrections``)."""
    g = _gen("bwdp", N, H, W, Cc)
    M = N * H * W
    _check_bwd_exact(C, xn.int_bn_bwd_inputs(M, Cc, g), mode, g, f"{N}x{H}x{W}x{Cc} mode={mode}", geom=(N, H, W))


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("M,Cc", [(774, 64), (301, 512), (4101, 8)])
def test_bn_bwd_real(C, M, Cc, mode):
    """Real-valued data: the mode-2 mask is reproduced from the fp32 fma, the
    sums are held to ``bwd_sums_bound``, dx / the ResBnBwd dres to the derived
    per-element bound against fp64 formulas of the sums the kernel read back."""
    g = _gen("bwdr", M, Cc)
    x, dy, xr = _real_x(M, Cc, g), _real_bf16((M, Cc), g), _real_bf16((M, Cc), g)
    w, b, _ = _params(Cc, g)
    s = xn.bn_stats64(x) / M
    save = torch.cat([s[0], (s[1] - s[0] ** 2).clamp_min(0).add(EPS).rsqrt()]).float()
    sr = xn.bn_stats64(xr) / M
    rsave = torch.cat([sr[0], (sr[1] - sr[0] ** 2).clamp_min(0).add(EPS).rsqrt()]).float()
    d = {"x": x, "dy": dy, "xr": xr, "save": save, "w": w, "b": b, "rsave": rsave, "rw": _params(Cc, _gen("rw", Cc))[0]}
    sc, sh = xn.coef_from_save(save, w, b)
    y = xn.bn_fwd_ref(x, sc, sh, True, xr) if mode == 1 else None
    yt = torch.from_numpy(y).to(BF16) if y is not None else None
    bits = torch.from_numpy(xn.mask_bits_ref(xn.bn_fwd_ref(x, sc, sh, True, xr))).reshape(-1) if mode == 3 else None
    mask = torch.from_numpy(xn.relu_mask(mode, x, sc, sh, y, bits.numpy() if bits is not None else None))
    gv = xb.cpu64(dy) * mask
    rb = mode in (1, 3)
    o = _bwd(C, d, mode, yt, bits, want_dres=rb, rb=rb)
    sums, sabs = xn.bn_bwd_sums(gv, x, save)
    xb.assert_within(o.acc.cpu().reshape(2, Cc), sums, xn.bwd_sums_bound(M, sabs), "acc")
    assert torch.equal(o.db.cpu(), o.acc.cpu()[:Cc]) and torch.equal(o.dw.cpu(), o.acc.cpu()[Cc:])
    dx, E = xn.bn_dx64(gv, x, save, w, o.acc.cpu(), M)
    xb.assert_within(o.dx, dx, xn.bf16_bound(dx, E), "dx")
    if rb:
        rsums, rabs = xn.bn_bwd_sums(gv, xr, rsave)
        xb.assert_within(o.racc.cpu().reshape(2, Cc), rsums, xn.bwd_sums_bound(M, rabs), "rb.acc")
        dr, Er = xn.bn_dx64(gv, xr, rsave, d["rw"], o.racc.cpu(), M)
        xb.assert_within(o.dres.cpu(), dr, xn.bf16_bound(dr, Er), "dres (ResBnBwd)")
        assert torch.equal(o.rdb.cpu(), o.racc.cpu()[:Cc]) and torch.equal(o.rdw.cpu(), o.racc.cpu()[Cc:])
        p = _bwd(C, d, mode, yt, bits, want_dres=True)  # plain residual: dres = g bitwise
        exact.assert_exact(p.dres.cpu(), gv, "dres")


def test_bn_bwd_host_checks(C):
    d = xn.int_bn_bwd_inputs(16, 8, _gen("hc"))
    bits = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(RuntimeError):  # mode 3 without bits
        _bwd(C, d, 3)
    with pytest.raises(RuntimeError):  # bits without mode 3
        _bwd(C, d, 2, bits=bits)
    with pytest.raises(RuntimeError):  # mode 1 without y
        _bwd(C, d, 1)
    with pytest.raises(RuntimeError):  # the fused residual BN needs this launch's reduce pass
        _bwd(C, d, 0, acc=torch.zeros(16), rb=True)


@pytest.mark.parametrize("Cc", [8, 64, 72, 200])
def test_bn_rows_reduce(C, Cc):
    """Integer partial rows [T][2][C] added into a pre-loaded acc, bit for bit;
    C = 8, 72 and 200 leave lanes of a 64-channel group without a channel."""
    for T in (1, 3, 4, 15, 16, 17, 64, 65, 300):
        g = _gen("rows", T, Cc)
        rows = torch.randint(-50, 51, (T, 2, Cc), generator=g).float()
        acc0 = torch.randint(-9, 10, (2 * Cc,), generator=g).float()
        xb.check_sum_exact("rows", xb.cpu64(rows), (0,))
        acc = _d(torch.cat([acc0, torch.full((64,), NAN)]))  # (64 guard entries past acc)
        C.bn_rows_reduce(_d(rows).data_ptr(), T, Cc, acc.data_ptr(), _s())
        torch.cuda.synchronize()
        exact.assert_exact(acc.cpu()[:2 * Cc], xb.cpu64(acc0) + xb.cpu64(rows).sum(0).reshape(-1), f"T={T}")
        assert bool(torch.isnan(acc.cpu()[2 * Cc:]).all()), "written past acc"


# ---------------------------------------------------------------------------
# pool_nhwc.hip
# ---------------------------------------------------------------------------
STEM = (3, 2, 1)
STEM_SHAPES = [(1, 1, 1, 8), (2, 2, 3, 8), (1, 7, 5, 16), (2, 8, 8, 24), (3, 9, 13, 64)]
GENERIC = [(2, 2, 0), (3, 1, 1), (3, 3, 1), (5, 2, 2), (1, 1, 0)]
GENERIC_SHAPES = [(2, 7, 5, 16), (1, 8, 10, 8)]


def _pool_x(shape, g):
    """Values on a grid of 0.5 in [-2, 2]: windows hold ties."""
    return (torch.randint(-4, 5, shape, generator=g).float() / 2).to(BF16)


def _pool_fwd(C, x, K, S, P, bn=None):
    N, H, W, Cc = x.shape
    Ho, Wo = xn.pool_out(H, K, S, P), xn.pool_out(W, K, S, P)
    y, idx = _new((N, Ho, Wo, Cc), NAN, BF16), _new((N, Ho, Wo, Cc), 0xEE, torch.uint8)
    kw = {}
    if bn is not None:
        kw = dict(bn_acc=bn["acc"].data_ptr(), bn_w=bn["w"].data_ptr(), bn_b=bn["b"].data_ptr(),
                  bn_save=bn["save"].data_ptr(), bn_rm=bn["rm"].data_ptr(), bn_rv=bn["rv"].data_ptr(), bn_eps=EPS,
                  bn_momentum=MOM)
    C.maxpool_nhwc_fwd(_d(x).data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W, Cc, K, S, P, _s(), **kw)
    torch.cuda.synchronize()
    return y.cpu(), idx.cpu().numpy()


def _pool_bwd_check(C, arg, shape, K, S, P, g, what):
    """Integer dy exact, real dy bitwise in the kernels' summation order."""
    N, H, W, Cc = shape
    for kind in ("int", "real"):
        # (real dy over 28 binades: a few bf16 values of one magnitude would add exactly in any order)
        dy = exact.int_bf16(arg.shape, -8, 8, generator=g) if kind == "int" else (
            torch.randn(arg.shape, generator=g) * torch.pow(2.0, torch.randint(-14, 15, arg.shape, generator=g))).to(BF16)
        dx = _new(shape, NAN, BF16)
        C.maxpool_nhwc_bwd(_d(dy).data_ptr(), _d(torch.from_numpy(arg)).data_ptr(), dx.data_ptr(), N, H, W, Cc, K, S,
                           P, _s())
        torch.cuda.synchronize()
        ref = xn.pool_bwd_ref(dy, arg, H, W, K, S, P)  # (integer dy: at most K^2 integers, exact in any order)
        xn.same_values(dx.cpu(), xn.to_bf16(ref), f"{what}: dx ({kind} dy)")


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_stem(C, shape):
    """3x3 / 2 / 1 (maxpool3s2 kernels), forward and backward; the shapes
    include H = 1, W = 1 and even edges, where the second window of a row or
    column is the first one again (ohs[1] == ohs[0])."""
    g = _gen("pool", *shape)
    x = _pool_x(shape, g)
    y, idx = _pool_fwd(C, x, *STEM)
    yr, ar = xn.pool_fwd_ref(x, *STEM)
    xn.same_values(y, yr, "y")
    assert np.array_equal(idx, ar), "argmax bytes"
    _pool_bwd_check(C, ar, shape, *STEM, g, "stem")


@pytest.mark.parametrize("shape", GENERIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("K,S,P", GENERIC)
def test_pool_generic(C, K, S, P, shape):
    """maxpool_nhwc_fwd_kernel / maxpool_nhwc_bwd_kernel (any window), odd and even sizes."""
    g = _gen("poolg", K, S, P, *shape)
    x = _pool_x(shape, g)
    y, idx = _pool_fwd(C, x, K, S, P)
    yr, ar = xn.pool_fwd_ref(x, K, S, P)
    xn.same_values(y, yr, "y")
    assert np.array_equal(idx, ar), "argmax bytes"
    _pool_bwd_check(C, ar, shape, K, S, P, g, f"K={K} S={S} P={P}")


def test_pool_stem_grid_stride(C):
    """More items than 8192 * 256: the grid-stride loop of maxpool3s2_fwd_kernel
    runs a second, ragged pass.  Reference on the device (F.max_pool2d with
    indices); any 3x3 window holds 9 distinct values ((h % 4, w % 4) selects
    one of 16 levels of a per-channel permutation), so no tie rule is involved."""
    N, H, W, Cc = 4, 515, 515, 64
    Ho = Wo = xn.pool_out(H, *STEM)
    items = N * Ho * Wo * (Cc // 8)
    assert 8192 * 256 < items < 2 * 8192 * 256 and items % (8192 * 256) % 256 != 0
    g = torch.Generator().manual_seed(5)
    perm = torch.stack([torch.randperm(16, generator=g) for _ in range(Cc)], 1).float().cuda()  # [16][C]
    hh, ww = torch.arange(H, device="cuda"), torch.arange(W, device="cuda")
    lvl = ((hh % 4) * 4).unsqueeze(1) + (ww % 4).unsqueeze(0)  # [H][W]
    off = ((hh // 4).unsqueeze(1) + (ww // 4).unsqueeze(0)) % 3
    x = (perm[lvl] + 16.0 * off.unsqueeze(2)).unsqueeze(0).repeat(N, 1, 1, 1)
    x = (x - 8.0 * torch.arange(N, device="cuda").view(N, 1, 1, 1)).to(BF16).contiguous()
    y = torch.full((N, Ho, Wo, Cc), NAN, dtype=BF16, device="cuda")
    idx = torch.full((N, Ho, Wo, Cc), 0xEE, dtype=torch.uint8, device="cuda")
    C.maxpool_nhwc_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W, Cc, 3, 2, 1, _s())
    torch.cuda.synchronize()
    yr, ir = F.max_pool2d(x.permute(0, 3, 1, 2).float(), 3, 2, 1, return_indices=True)
    assert torch.equal(y.float(), yr.permute(0, 2, 3, 1)), "y"
    a = idx.long()
    oh = torch.arange(Ho, device="cuda").view(1, Ho, 1, 1)
    ow = torch.arange(Wo, device="cuda").view(1, 1, Wo, 1)
    flat = (2 * oh - 1 + a // 3) * W + (2 * ow - 1 + a % 3)
    assert torch.equal(flat, ir.permute(0, 2, 3, 1)), "argmax"


def test_pool_host_checks(C):
    x, y, idx = _new((1, 4, 4, 16), 1.0, BF16), _new((1, 4, 4, 16), NAN, BF16), _new((1, 4, 4, 16), 0xEE, torch.uint8)
    f = _new(64, 1.0)
    bn = dict(bn_acc=f.data_ptr(), bn_w=f.data_ptr(), bn_b=f.data_ptr(), bn_save=f.data_ptr())
    with pytest.raises(RuntimeError):  # 2P > K
        C.maxpool_nhwc_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(), 1, 4, 4, 16, 3, 1, 2, _s())
    with pytest.raises(RuntimeError):  # C % 8
        C.maxpool_nhwc_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(), 1, 4, 4, 12, 3, 2, 1, _s())
    with pytest.raises(RuntimeError):  # BN on load with another window
        C.maxpool_nhwc_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(), 1, 4, 4, 16, 2, 2, 0, _s(), **bn)
    with pytest.raises(RuntimeError):  # BN on load with C/8 = 3 not dividing 256
        C.maxpool_nhwc_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(), 1, 4, 2, 24, 3, 2, 1, _s(), **bn)
    with pytest.raises(RuntimeError):
        C.maxpool_nhwc_bwd(y.data_ptr(), idx.data_ptr(), x.data_ptr(), 1, 4, 4, 16, 3, 1, 2, _s())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.float()).all()) and bool((idx == 0xEE).all())


@pytest.mark.parametrize("N,H,W,Cc", [(2, 7, 5, 8), (3, 9, 13, 64), (1, 8, 8, 256)])
def test_pool_bn_on_load(C, N, H, W, Cc):
    """PoolBn: every window element is bf16(max(fma(x, sc, sh), 0)) with the
    coefficients of the published save; output and argmax bitwise, save and
    the running statistics within the coefficient bounds."""
    g = _gen("poolbn", N, H, W, Cc)
    M = N * H * W
    x = _real_x(M, Cc, g)
    w, b, running = _params(Cc, g)
    acc = xn.bn_stats64(x).reshape(-1).float()
    bn = {"acc": _d(acc), "w": _d(w), "b": _d(b), "save": _new(2 * Cc, NAN), "rm": _d(running[0].clone()),
          "rv": _d(running[1].clone())}
    y, idx = _pool_fwd(C, x.reshape(N, H, W, Cc), *STEM, bn=bn)
    xn.assert_published(bn["save"], (bn["rm"].cpu(), bn["rv"].cpu()), acc, M, w, b, EPS, MOM, running, "PoolBn")
    sc, sh = xn.coef_from_save(bn["save"], w, b)
    z = xn.bn_fwd_ref(x, sc, sh, True).reshape(N, H, W, Cc)
    yr, ar = xn.pool_fwd_ref(z, *STEM)
    xn.same_values(y, yr, "y")
    assert np.array_equal(idx, ar), "argmax bytes"


def _pool_bn_bwd(C, d, N, H, W, dy, arg):
    Cc = d["x"].shape[1]
    o = SimpleNamespace(acc=_new(2 * Cc, 0.0), dx=_new((N * H * W, Cc), NAN, BF16), dw=_new(Cc, NAN), db=_new(Cc, NAN))
    C.maxpool_bn_bwd(_d(dy).data_ptr(), _d(torch.from_numpy(arg)).data_ptr(), _d(d["x"]).data_ptr(),
                     _d(d["save"]).data_ptr(), _d(d["w"]).data_ptr(), _d(d["b"]).data_ptr(), o.acc.data_ptr(),
                     o.dx.data_ptr(), o.dw.data_ptr(), o.db.data_ptr(), N, H, W, Cc, _s())
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("N,H,W,Cc", [(1, 1, 1, 8), (4, 8, 8, 64), (2, 16, 8, 256), (3, 9, 13, 64), (2, 7, 5, 8)])
def test_pool_bn_bwd_exact(C, N, H, W, Cc):
    """maxpool_bn_bwd in the exact regime (the test supplies save): the sums of
    pass 0 bit for bit, dw / db = acc, and at power-of-two N H W the dx of pass
    1.  g = bf16(gathered dz) under the mode-2 mask; pre-activations of exactly
    0 occur and are masked."""
    g = _gen("pbb", N, H, W, Cc)
    M = N * H * W
    d = xn.int_bn_bwd_inputs(M, Cc, g)
    sc, sh = xn.coef_from_save(d["save"], d["w"], d["b"])
    z = xn.bn_fwd_ref(d["x"], sc, sh, True).reshape(N, H, W, Cc)
    _, arg = xn.pool_fwd_ref(z, *STEM)
    dy = exact.int_bf16(arg.shape, -4, 4, generator=g)
    dz = xn.to_bf16(xn.pool_bwd_ref(dy, arg, H, W, *STEM)).reshape(M, Cc)
    pre = fma32(xn.np32(d["x"]), sc, sh)
    assert (pre == 0).any() or M < 8
    gv = xn.t64(dz) * torch.from_numpy(pre > 0)
    sums, _ = xn.bn_bwd_sums(gv, d["x"], d["save"], exact_regime=True)
    o = _pool_bn_bwd(C, d, N, H, W, dy, arg)
    exact.assert_exact(o.acc.cpu(), sums.reshape(-1), "acc")
    assert torch.equal(o.db.cpu(), o.acc.cpu()[:Cc]) and torch.equal(o.dw.cpu(), o.acc.cpu()[Cc:])
    if M & (M - 1) == 0:
        dx, _ = xn.bn_dx64(gv, d["x"], d["save"], d["w"], sums, M, exact_regime=True)
        exact.assert_exact(o.dx.cpu(), dx, "dx")


@pytest.mark.parametrize("N,H,W,Cc", [(3, 9, 13, 64), (2, 16, 8, 256)])
def test_pool_bn_bwd_real(C, N, H, W, Cc):
    """Real-valued data: the gathered dz is rounded to bf16 before the mask, as
    the kernel does; sums and dx under the backward-apply bounds."""
    g = _gen("pbr", N, H, W, Cc)
    M = N * H * W
    x = _real_x(M, Cc, g)
    w, b, _ = _params(Cc, g)
    s = xn.bn_stats64(x) / M
    save = torch.cat([s[0], (s[1] - s[0] ** 2).clamp_min(0).add(EPS).rsqrt()]).float()
    d = {"x": x, "save": save, "w": w, "b": b}
    sc, sh = xn.coef_from_save(save, w, b)
    _, arg = xn.pool_fwd_ref(xn.bn_fwd_ref(x, sc, sh, True).reshape(N, H, W, Cc), *STEM)
    dy = _real_bf16(arg.shape, g)
    dz = xn.to_bf16(xn.pool_bwd_ref(dy, arg, H, W, *STEM)).reshape(M, Cc)
    gv = xn.t64(dz) * torch.from_numpy(fma32(xn.np32(x), sc, sh) > 0)
    o = _pool_bn_bwd(C, d, N, H, W, dy, arg)
    sums, sabs = xn.bn_bwd_sums(gv, x, save)
    xb.assert_within(o.acc.cpu().reshape(2, Cc), sums, xn.bwd_sums_bound(M, sabs), "acc")
    assert torch.equal(o.db.cpu(), o.acc.cpu()[:Cc]) and torch.equal(o.dw.cpu(), o.acc.cpu()[Cc:])
    dx, E = xn.bn_dx64(gv, x, save, w, o.acc.cpu(), M)
    xb.assert_within(o.dx.cpu(), dx, xn.bf16_bound(dx, E), "dx")


# ---------------------------------------------------------------------------
# resnet_glue.hip
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W", [(2, 9, 14), (1, 16, 7), (3, 5, 5)])
def test_s2d_stem_input(C, N, H, W):
    g = _gen("s2d", N, H, W)
    x = _real_bf16((N, H, W, 3), g)
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    Hs, Ws = Ho + 3, Wo + 3
    S = _new((N, Hs, Ws, 16), NAN, BF16)
    C.s2d_stem_input(_d(x).data_ptr(), S.data_ptr(), N, H, W, Hs, Ws, 3, _s())
    torch.cuda.synchronize()
    ref = xn.s2d_ref(x, Hs, Ws, 3)
    assert np.count_nonzero(ref) >= 0.5 * x.numel()  # the image is in there (every pixel appears exactly once)
    xn.same_values(S.cpu(), ref, "S")
    assert bool((S.cpu()[..., 12:] == 0).all())


@pytest.mark.parametrize("Cout", [8, 64])
def test_stem_weight_pack(C, Cout):
    w7 = _real_bf16((Cout, 3, 7, 7), _gen("w7", Cout))
    w4 = _new((Cout, 4, 4, 16), NAN, BF16)
    C.stem_weight_pack(_d(w7).data_ptr(), w4.data_ptr(), Cout, _s())
    torch.cuda.synchronize()
    got = w4.cpu().float()
    xn.same_values(got, xn.stem_pack_ref(w7), "w4")
    assert bool((got[:, 3, :, 6:12] == 0).all()) and bool((got[:, :, 3, 3:6] == 0).all())  # kh = 7, kw = 7
    assert bool((got[:, :, 3, 9:12] == 0).all()) and bool((got[..., 12:] == 0).all())
    assert sorted(got[got != 0].tolist()) == sorted(w7.float()[w7.float() != 0].tolist())  # a permutation of the taps


@pytest.mark.parametrize("Cin,Cout", [(1, 8), (8, 64), (24, 8), (24, 64)])
def test_phase_weights(C, Cin, Cout):
    wt = _real_bf16((Cin, 3, 3, Cout), _gen("ph", Cin, Cout))
    out = _new(9 * Cin * Cout + 8, NAN, BF16)
    C.phase_weights(_d(wt).data_ptr(), out.data_ptr(), Cin, Cout, _s())
    torch.cuda.synchronize()
    got = out.cpu().float()
    assert bool(torch.isnan(got[9 * Cin * Cout:]).all())
    ref = xn.phase_ref(wt)
    xn.same_values(got[:9 * Cin * Cout], ref, "phase arena")
    for p, off in enumerate((0, 1, 3, 5)):  # each block at its arena offset, in [Cin][KHp][KWp][Cout]
        kh, kw = xn.PHASE_TAPS[p]
        blk = got[off * Cin * Cout:(off + kh * kw) * Cin * Cout].reshape(Cin, kh, kw, Cout)
        th = [1] if kh == 1 else [0, 2]
        tw = [1] if kw == 1 else [0, 2]
        assert torch.equal(blk, wt.float()[:, th][:, :, tw]), f"phase {p}"


@pytest.mark.parametrize("B,HW,Cc", [(1, 1, 8), (3, 49, 64), (2, 50, 2048)])
def test_head_broadcast(C, B, HW, Cc):
    df = _real_bf16((B, Cc), _gen("hb", B, HW, Cc))
    dh = _new((B, HW, Cc), NAN, BF16)
    C.head_broadcast(_d(df).data_ptr(), dh.data_ptr(), B, HW, Cc, _s())
    torch.cuda.synchronize()
    assert torch.equal(dh.cpu(), df.unsqueeze(1).expand(B, HW, Cc))


@pytest.mark.parametrize("Cc", [64, 192])
@pytest.mark.parametrize("NC", [1, 100, 128, 1000])
def test_head_weight_prep(C, NC, Cc):
    NCp = (NC + 127) // 128 * 128
    w = torch.randn(NC, Cc, generator=_gen("hw", NC, Cc))
    wb, wbt = _new((NCp, Cc), NAN, BF16), _new((Cc, NCp), NAN, BF16)
    C.head_weight_prep(_d(w).data_ptr(), wb.data_ptr(), wbt.data_ptr(), NC, NCp, Cc, _s())
    torch.cuda.synchronize()
    assert torch.equal(wb.cpu()[:NC], w.to(BF16)), "wb"
    assert bool((wb.cpu()[NC:] == 0).all()), "padded rows of wb"
    assert torch.equal(wbt.cpu(), wb.cpu().t()), "wbt"


@pytest.mark.parametrize("Cout", [8, 64])
@pytest.mark.parametrize("splits", [1, 2, 5])
def test_stem_wgrad_unpack(C, splits, Cout):
    """Integer slabs with a distinct value in every one of the 147 Cout slots
    (exact, pre-loaded dw7), then real slabs bitwise against sequential fp32
    adds in split order."""
    g = _gen("su", splits, Cout)
    k = xn.stem_unpack_index()
    # slab 0: a distinct integer per used slot and output channel; the unused slots (kh or kw = 7,
    # channels 12..15) hold 2^20, which must not reach dw7
    slab = torch.full((splits, Cout, 256), float(2 ** 20))
    slab[:, :, torch.from_numpy(k.reshape(-1))] = 0.0
    vals = (torch.arange(Cout * 147).reshape(Cout, 147) + 1).float()
    slab[0][:, torch.from_numpy(k.reshape(-1))] = vals
    for q in range(1, splits):
        slab[q][:, torch.from_numpy(k.reshape(-1))] = torch.randint(-9, 10, (Cout, 147), generator=g).float()
    for kind in ("int", "real"):
        if kind == "real":
            slab = torch.randn(splits, Cout, 256, generator=g)
        dw0 = torch.randint(-5, 6, (Cout, 3, 7, 7), generator=g).float() if kind == "int" else torch.randn(
            Cout, 3, 7, 7, generator=g)
        dw = _d(dw0.clone())
        C.stem_wgrad_unpack(_d(slab).data_ptr(), dw.data_ptr(), splits, Cout, _s())
        torch.cuda.synchronize()
        ref = xn.stem_unpack_ref(slab, dw0)
        if kind == "int":
            want = xb.cpu64(dw0) + xb.cpu64(slab)[:, :, torch.from_numpy(k.reshape(-1))].sum(0).reshape(Cout, 3, 7, 7)
            xb.check_f32("integer dw7", want)
            assert np.array_equal(ref, want.float().numpy())
        xn.same_values(dw.cpu(), ref, f"dw7 ({kind})")


@pytest.mark.parametrize("NC,NCp,Cc,splits", [(1, 128, 64, 1), (100, 128, 64, 3), (1000, 1024, 192, 2)])
def test_head_wgrad_reduce(C, NC, NCp, Cc, splits):
    """dw += scale * sum of the slabs' first NC rows, exact with a dyadic
    scale; the slabs' padded rows hold 2^20, which must not reach dw: the
    buffer behind dw has NCp + 1 rows, and those past NC keep their fill."""
    g = _gen("hwr", NC, NCp, Cc)
    slab = torch.randint(-20, 21, (splits, NCp, Cc), generator=g).float()
    slab[:, NC:] = float(2 ** 20)
    dw0 = torch.randint(-9, 10, (NC, Cc), generator=g).float()
    dw = _d(torch.cat([dw0, torch.full((NCp - NC + 1, Cc), 7.0)]))  # (a finite guard: NaN would absorb an addition)
    C.head_wgrad_reduce(_d(slab).data_ptr(), dw.data_ptr(), splits, NC, NCp, Cc, 0.25, _s())
    torch.cuda.synchronize()
    want = xb.cpu64(dw0) + 0.25 * xb.cpu64(slab)[:, :NC].sum(0)
    xb.check_f32("dw", want)
    exact.assert_exact(dw.cpu()[:NC], want, "dw")
    assert bool((dw.cpu()[NC:] == 7.0).all()), "dw was written past its NC rows"


@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("HW,Cc", [(1, 8), (49, 2048), (50, 8), (49, 8), (50, 2048)])
def test_head_pool(C, B, HW, Cc):
    """Sequential fp32 sum over HW, one multiply by fl(1/HW), one bf16 rounding;
    loss[0] is zeroed, its neighbours are not touched.  B = 130 with C = 2048
    is more than one block."""
    h = _real_bf16((B, HW, Cc), _gen("hp", B, HW, Cc))
    f, loss = _new((B, Cc), NAN, BF16), _new(4, 7.0)
    C.head_pool(_d(h).data_ptr(), f.data_ptr(), B, HW, Cc, loss.data_ptr(), _s())
    torch.cuda.synchronize()
    xn.same_values(f.cpu(), xn.head_pool_ref(h), "f")
    assert loss.cpu().tolist() == [0.0, 7.0, 7.0, 7.0]


NLL_NC = [1, 10, 255, 256, 257, 1000, 1024]


def _nll(C, slab, bias, labels, B, NC, NCp, dscale=1.0, loss0=0.0):
    splits = slab.shape[0]
    o = SimpleNamespace(logp=_new((B, NC), NAN), loss_b=_new(B, NAN), dl=_new((B, NCp), NAN, BF16), db=_new(NC, 0.0),
                        loss=_new(2, loss0))
    train = labels is not None
    C.head_softmax_nll(_d(slab).data_ptr(), splits, B, NC, NCp, _d(bias).data_ptr(), _p(_d(labels) if train else None),
                       o.logp.data_ptr(), o.loss_b.data_ptr() if train else 0, o.dl.data_ptr() if train else 0, dscale,
                       o.db.data_ptr() if train else 0, o.loss.data_ptr() if train else 0, _s())
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("B,splits", [(1, 1), (4, 2), (4, 5)])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("NC", NLL_NC)
def test_head_softmax_nll_saturated(C, NC, wide, B, splits):
    """One logit leads by more than 104: every other __expf is 0, the sum of
    exponentials exactly 1 and its log 0, so logp, loss_b, dl (bf16 of g times
    a dyadic dscale), db (B a power of two) and the mean loss are exact; the
    padded dl columns are 0; eval mode writes logp only."""
    NCp = 1024 if wide else (NC + 127) // 128 * 128
    g = _gen("nll", NC, NCp, B, splits)
    slab, bias, lab, k = xn.saturated_slabs(B, NC, NCp, splits, g)
    lg = xn.head_logits_ref(slab, bias, NC)
    xb.check_sum_exact("logit terms", torch.cat([xb.cpu64(slab)[:, :, :NC], xb.cpu64(bias).expand(1, B, NC)]), (0,))
    top = np.sort(lg, 1)
    assert NC == 1 or float((top[:, -1] - top[:, -2]).min()) > 104.0
    r = xn.softmax_nll64(lg, lab)
    onehot_k = F.one_hot(k, NC).double()
    assert bool((r["logp"].exp().round() == onehot_k).all())
    logp = xn.t64(lg) - xn.t64(lg).max(1, keepdim=True).values  # lse = the leading logit exactly
    gg = onehot_k - F.one_hot(lab, NC).double()
    o = _nll(C, slab, bias, lab, B, NC, NCp, dscale=0.125)
    exact.assert_exact(o.logp.cpu(), logp, "logp")
    exact.assert_exact(o.loss_b.cpu(), -(logp * F.one_hot(lab, NC)).sum(1), "loss_b")
    exact.assert_exact(o.dl.cpu()[:, :NC].contiguous(), gg * 0.125, "dl")
    assert bool((o.dl.cpu()[:, NC:] == 0).all()), "padded dl columns"
    exact.assert_exact(o.db.cpu(), gg.sum(0) / B, "db")
    lb = -(logp * F.one_hot(lab, NC)).sum(1)
    xb.check_sum_exact("loss terms", lb / B, (0,))
    exact.assert_exact(o.loss.cpu()[:1], lb.mean().reshape(1), "mean loss")
    assert float(o.loss.cpu()[1]) == 0.0
    e = _nll(C, slab, bias, None, B, NC, NCp)
    exact.assert_exact(e.logp.cpu(), logp, "logp (eval)")
    assert bool(torch.isnan(e.loss_b).all()) and bool(torch.isnan(e.dl.float()).all()) and bool((e.db == 0).all())


# Allowance of the fast __expf / __logf in head_softmax_nll_kernel, in units
# u_b = 2^-23 max(1, spread_b) per sample (spread: the largest |logit - max|),
# measured against the fp64 reference of the SAME fp32 logits (sequential sums
# emulated bitwise, so the linear part carries no error) on the shapes of
# test_head_softmax_nll_real.  The intrinsics' accuracy depends on the argument
# range, so it is measured, as in the head.hip oracle, and 4 x the maximum is
# allowed.  Measured on an MI355X (printed by the test before it asserts): per
# case logp / loss_b 0.31 .. 0.70 units (0 at NC = 1), softmax - onehot (read
# from db, which is g itself at B = 1) 0.013 .. 0.046 units.
MEASURED_LOGP_UNITS = 0.703
MEASURED_SOFTMAX_UNITS = 0.046


@pytest.mark.parametrize("B,splits", [(1, 1), (4, 2), (4, 5)])
@pytest.mark.parametrize("NC", NLL_NC)
def test_head_softmax_nll_real(C, NC, B, splits, record_property):
    """Real-valued slabs: logp / loss_b and g = softmax - onehot (behind dl,
    db) against fp64 of the bitwise-emulated fp32 logits, within 4 x the
    measured allowance (logp 0.703, softmax 0.046 units of 2^-23 max(1,
    spread)); dl one bf16 rounding on top; db and the mean loss two more units
    for their B atomic additions and the division by B; figures printed first."""
    NCp = (NC + 127) // 128 * 128
    g = _gen("nllr", NC, B, splits)
    slab = torch.randn(splits, B, NCp, generator=g) * 2
    bias = torch.randn(NC, generator=g)
    lab = torch.randint(0, NC, (B,), generator=g)
    lg = xn.head_logits_ref(slab, bias, NC)
    r = xn.softmax_nll64(lg, lab)
    u_b = (xb.U32 * r["spread"].clamp_min(1.0)).unsqueeze(1)
    o = _nll(C, slab, bias, lab, B, NC, NCp, dscale=1.0)
    err_lp = ((xb.cpu64(o.logp) - r["logp"]).abs() / u_b).max()
    err_lb = ((xb.cpu64(o.loss_b) - r["loss_b"]).abs() / u_b.squeeze(1)).max()
    dl_ref = r["g"]  # (dscale = 1)
    # the fp32 g is visible in db = sum_b g / B only (dl is its bf16 rounding): with B = 1 db IS g
    err_db = ((xb.cpu64(o.db) - r["g"].sum(0) / B).abs() / u_b.max()).max()
    meas = {"logp_units": float(torch.maximum(err_lp, err_lb)), "softmax_units": float(err_db)}
    print(f"head_softmax_nll_real NC={NC} B={B} splits={splits}: " + " ".join(f"{k}={v:.3f}" for k, v in meas.items()))
    for k_, v in meas.items():
        record_property(k_, v)
    A_lp, A_sm = 4 * MEASURED_LOGP_UNITS, 4 * MEASURED_SOFTMAX_UNITS
    xb.assert_within(o.logp, r["logp"], A_lp * u_b, "logp")
    xb.assert_within(o.loss_b, r["loss_b"], (A_lp * u_b).squeeze(1), "loss_b")
    E = A_sm * u_b
    xb.assert_within(o.dl.cpu()[:, :NC], dl_ref, xn.bf16_bound(dl_ref, E.expand_as(dl_ref)), "dl")
    assert bool((o.dl.cpu()[:, NC:] == 0).all())
    xb.assert_within(o.db, r["g"].sum(0) / B, (A_sm + 2) * u_b.max() * torch.ones(NC), "db")
    xb.assert_within(o.loss.cpu()[:1], r["loss_b"].mean().reshape(1), (A_lp + 2) * u_b.max() * torch.ones(1), "loss")


# ---------------------------------------------------------------------------
# the Python layer's pointer arithmetic
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("out_pad,dx_pad", [(1, 1), (0, 1), (1, 0)])
def test_ops_bn_act_padded(C, out_pad, dx_pad):
    """ops.bn_nhwc.bn_act with padded output / input gradient: ybase / dxbase
    point at the buffer's origin (interior bitwise right, border zero), and the
    backward sums live in acc4[2C:] (dw / db equal that slice; acc4[:2C] still
    holds the forward statistics)."""
    from torch_distlearn_amd.ops import bn_nhwc as ob

    N, Cc, H, W = 3, 64, 5, 7
    M = N * H * W
    g = _gen("ops", out_pad, dx_pad)
    x2, dy2 = _real_bf16((M, Cc), g, 2.0), _real_bf16((M, Cc), g)
    w, b, running = _params(Cc, g)
    to4 = lambda t: t.reshape(N, H, W, Cc).cuda().permute(0, 3, 1, 2)  # noqa: E731  channels-last [N, C, H, W]
    x = to4(x2).requires_grad_(True)
    wd, bd = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    rm, rv = running[0].clone().cuda(), running[1].clone().cuda()
    y = ob.bn_act(x, wd, bd, rm, rv, relu=True, eps=EPS, momentum=MOM, out_pad=out_pad, dx_pad=dx_pad)
    saved = y.grad_fn.saved_tensors  # x, mask source, weight, bias, save, acc4
    save, acc4 = saved[4], saved[5]
    xn.assert_published(save, (rm, rv), acc4[:2 * Cc], M, w, b, EPS, MOM, running, "bn_act")
    sc, sh = xn.coef_from_save(save, w, b)
    xn.same_values(y.permute(0, 2, 3, 1).reshape(M, Cc), xn.bn_fwd_ref(x2, sc, sh, True), "y")

    def border_zero(v, p):
        buf = v.detach().as_strided((N, H + 2 * p, W + 2 * p, Cc), ((H + 2 * p) * (W + 2 * p) * Cc, (W + 2 * p) * Cc,
                                                                     Cc, 1), v.storage_offset() - (p * (W + 2 * p) + p) * Cc)
        m = torch.ones(H + 2 * p, W + 2 * p, dtype=torch.bool)
        m[p:p + H, p:p + W] = False
        return bool((buf.cpu()[:, m] == 0).all())

    assert not out_pad or border_zero(y, out_pad)
    fwd_acc = acc4[:2 * Cc].clone()
    dx, dw, db = torch.autograd.grad(y, (x, wd, bd), to4(dy2))  # (the raw dx: x.grad may be a re-laid-out copy)
    torch.cuda.synchronize()
    assert torch.equal(acc4[:2 * Cc], fwd_acc), "the backward wrote into the forward half of acc4"
    mask = torch.from_numpy(fma32(xn.np32(x2), sc, sh) > 0)
    gv = xb.cpu64(dy2) * mask
    sums, sabs = xn.bn_bwd_sums(gv, x2, save)
    xb.assert_within(acc4[2 * Cc:].cpu().reshape(2, Cc), sums, xn.bwd_sums_bound(M, sabs), "acc4[2C:]")
    assert torch.equal(db, acc4[2 * Cc:3 * Cc]) and torch.equal(dw, acc4[3 * Cc:])
    ref, E = xn.bn_dx64(gv, x2, save, w, acc4[2 * Cc:].cpu(), M)
    xb.assert_within(dx.permute(0, 2, 3, 1).reshape(M, Cc), ref, xn.bf16_bound(ref, E), "dx")
    assert not dx_pad or border_zero(dx, dx_pad)


@pytest.mark.parametrize("K,S,P", [STEM, (2, 2, 0)])
def test_ops_max_pool2d_nhwc(C, K, S, P):
    from torch_distlearn_amd.ops.pool import max_pool2d_nhwc

    N, H, W, Cc = 2, 9, 6, 16
    g = _gen("opool", K)
    x = _pool_x((N, H, W, Cc), g)
    xd = x.cuda().permute(0, 3, 1, 2).requires_grad_(True)
    y = max_pool2d_nhwc(xd, K, S, P)
    yr, ar = xn.pool_fwd_ref(x, K, S, P)
    xn.same_values(y.permute(0, 2, 3, 1), yr, "y")
    dy = _real_bf16(yr.shape, g)
    y.backward(dy.cuda().permute(0, 3, 1, 2))
    xn.same_values(xd.grad.permute(0, 2, 3, 1), xn.to_bf16(xn.pool_bwd_ref(dy, ar, H, W, K, S, P)), "dx")


def test_ops_resnet_head_saturated(C):
    """ops.head.ResNetHeadNLL end to end in the saturated integer regime of
    the head.hip oracle (``head_exact_inputs``: the largest logit leads by 160,
    every intermediate an fp32 number): loss, logp, dh and the accumulated
    weight / bias gradients are exact.  The weight gradient view sits inside a
    larger buffer with a finite fill: the rows past ncls must keep it."""
    from torch_distlearn_amd.ops.head import ResNetHeadNLL

    B, Cc, H, W, ncls = 8, 256, 2, 2, 100  # (a shape the head is used at: NCp = 128 > ncls)
    HW, NCp = H * W, 128
    g = _gen("ophead")
    f, w, bias, lab, _ = xb.head_exact_inputs(B, Cc, g, NC=ncls)
    ref = xb.head_exact_ref(f, w, bias, lab)
    # four positions with mean f exactly: f + 1, f - 1, f, f
    h = torch.stack([f.float() + 1, f.float() - 1, f.float(), f.float()], 1).to(BF16)  # [B][HW][C]
    xn.same_values(xn.head_pool_ref(h), f, "the pooled features are f")
    hd = h.reshape(B, H, W, Cc).cuda().permute(0, 3, 1, 2).requires_grad_(True)
    gw0 = torch.randint(-3, 4, (ncls, Cc), generator=g).float()
    gwbuf = _d(torch.cat([gw0, torch.full((NCp - ncls + 1, Cc), 7.0)]))
    gb0 = torch.randint(-3, 4, (ncls,), generator=g).float()
    gb = _d(gb0.clone())
    done = []
    loss, logp = ResNetHeadNLL.apply(hd, w.cuda(), bias.cuda(), lab.cuda(), (gwbuf[:ncls], gb, lambda: done.append(1)))
    loss.backward()
    torch.cuda.synchronize()
    assert done == [1]
    exact.assert_exact(loss.detach().reshape(1).cpu(), ref["loss"].reshape(1), "loss")
    exact.assert_exact(logp.detach().cpu(), ref["logp"], "logp")
    # dlogits carry 1 / (B HW): dh = ref dh / HW at every position; dW = HW * dl^T f = ref dW
    xb.check_f32("dh / HW", ref["dh"] / HW)
    dh = hd.grad.permute(0, 2, 3, 1).reshape(B, HW, Cc).cpu()
    exact.assert_exact(dh.contiguous(), (ref["dh"] / HW).unsqueeze(1).expand(B, HW, Cc), "dh")
    exact.assert_exact(gwbuf.cpu()[:ncls], xb.cpu64(gw0) + ref["dW"], "weight gradient")
    assert bool((gwbuf.cpu()[ncls:] == 7.0).all()), "rows past ncls of the weight gradient were written"
    exact.assert_exact(gb.cpu(), xb.cpu64(gb0) + ref["db"], "bias gradient")
