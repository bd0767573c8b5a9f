"""Every convolution kernel path against exact oracles (tests/kernels/exact.py).

Integer operands with sum |x||w| < 2**24 make every partial sum an exact
integer in fp32, in any order and across any split: an fp32 output must equal
the fp64 reference bit for bit and a bf16 output its single round-to-nearest-
even (``assert_exact``); BatchNorm partial rows are checked by ``assert_stats``;
one case per path also runs real-valued operands through the per-element bound
(``assert_elementwise``).  Every case asserts the kernel it was written for
through the read-only dispatch queries (conv_fwd_path / conv_region_ok /
conv_fix_ok): a case that silently falls back to another kernel fails.

Shapes are (B, H, W, Cin, Cout), the kernel 5x5 with pad 2 unless stated: the
smallest that reach each path, with M tails, several tiles, odd split counts
and non-square images.  All cases run in the deterministic reduction mode."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.kernels import exact

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NAN = float("nan")
_BM = {0: 128, 1: 64, 2: 128}
_BN = {0: 128, 1: 64, 2: 64}
IMAGES, KEEP, PAIR = 1 << 16, 1 << 20, 1 << 24  # bits of the tile word (ops.conv.pack_tile)


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from torch_distlearn_amd import _native

    return _native.native()


@pytest.fixture(autouse=True)
def _mode0(request):
    """Deterministic partial-row reduction mode for every test (a process-wide device global)."""
    if "C" in request.fixturenames:
        request.getfixturevalue("C").set_reduce_atomic(0)
    yield


def _paths():
    from torch_distlearn_amd.ops import conv

    return conv


def _s():
    return torch.cuda.current_stream().cuda_stream


def _dev(t):
    return t.to("cuda").contiguous()


def _pad(t, p=2):
    return F.pad(t, (0, 0, p, p, p, p)).contiguous()


def _sid(shape):
    return "x".join(map(str, shape))


class FwdCase:
    """Operands (CPU and padded device copies), fp64 reference and the
    expected bf16 output of one 5x5 forward conv.  real_c: input channels
    beyond it are zero in x (the channel-padded first layer); w_pads: nonzero
    integers in the weights' pad channels, which must never reach the result."""

    def __init__(self, shape, kind="int", real_c=None, w_pads=False):
        B, H, W, cin, cout = shape
        real_c = cin if real_c is None else real_c
        g = torch.Generator().manual_seed(1000 * B + 100 * H + 10 * W + cin + cout + (kind == "int"))
        self.shape, self.kind = shape, kind
        self.K = 25 * real_c  # products with the zero channels are exact zeros
        if kind == "int":
            a = exact.magnitude(25 * real_c)
            exact.check_exact_range(25 * real_c, a, a)
            x = exact.int_bf16((B, H, W, cin), -a, a, density=0.9, generator=g)
            w = exact.int_bf16((cout, 5, 5, cin), -a, a, generator=g)
        else:
            x = torch.randn(B, H, W, cin, generator=g).to(BF16)
            w = (torch.randn(cout, 5, 5, cin, generator=g) * 0.05).to(BF16)
        x[..., real_c:] = 0
        self.x, self.w = x, w
        self.ref, self.S = exact.conv_ref64(x[..., :real_c], w[..., :real_c], with_abs=kind != "int")
        if real_c < cin:
            w[..., real_c:] = exact.int_bf16((cout, 5, 5, cin - real_c), 1, 3, generator=g) if w_pads else 0
        self.y_exp = exact.expected(self.ref, BF16)
        self.xp, self.wd = _dev(_pad(x)), _dev(w)

    def check(self, y, tile, splits=1, what="y"):
        if self.kind == "int":
            exact.assert_exact(y, self.ref, what, tile=(_BM[tile & 15], _BN[tile & 15]), row_dims=3)
        else:
            exact.assert_elementwise(y, self.ref, self.S, self.K, adds=splits if splits > 1 else 0, what=what)

    def check_stats(self, rows, T, y):
        # the statistics are of exactly the stored bf16 values: the expected ones for integer operands
        exact.assert_stats(rows, self.y_exp if self.kind == "int" else y, T)


@functools.lru_cache(maxsize=None)
def _case(shape, kind="int", real_c=None, w_pads=False):
    return FwdCase(shape, kind, real_c, w_pads)


def _run_fwd(C, x_ptr, w_ptr, shape, tile, splits, stats=True, fix=False, cin_arg=None):
    """conv_fwd / conv_fwd_fix into NaN-filled y, statistics rows (two spare
    rows) and slabs -> (y, rows, returned row count, slab)."""
    B, H, W, cin, cout = shape
    cin = cin if cin_arg is None else cin_arg
    M = B * H * W
    y = torch.full((B, H, W, cout), NAN, dtype=BF16, device="cuda")
    n_rows = (M + 127) // 128 if fix else C.conv_fwd_stat_rows(B, H, W, max(cin, 8), cout, 5, tile, splits)
    rows = torch.full((n_rows + 2, 2, cout), NAN, device="cuda") if stats else None
    slab = torch.full((splits, M, cout), NAN, device="cuda") if splits > 1 else None
    args = (x_ptr, w_ptr, y.data_ptr(), rows.data_ptr() if stats else 0, slab.data_ptr() if splits > 1 else 0, B, H, W,
            cin, cout, 5, tile, splits)
    T = C.conv_fwd_fix(*args, 0, 0, 0, _s()) if fix else C.conv_fwd(*args, _s())
    torch.cuda.synchronize()
    if stats:
        assert T == n_rows
    return y, rows, T, slab


def _fwd_and_check(C, case, tile, splits, stats=True):
    y, rows, T, _ = _run_fwd(C, case.xp.data_ptr(), case.wd.data_ptr(), case.shape, tile, splits, stats)
    case.check(y, tile, splits)
    if stats:
        case.check_stats(rows, T, y)
    return y, rows


def _path(C, shape, tile, splits=1):
    B, H, W, cin, cout = shape
    return C.conv_fwd_path(B, H, W, cin, cout, 5, tile, splits)


# --------------------------------------------------------------------------- streaming, per-lane taps (Cin < 64)
LANE = [((3, 4, 4, 16, 64), 1), ((3, 4, 4, 16, 64), 2), ((5, 4, 4, 32, 128), 0), ((3, 4, 4, 8, 64), 2)]


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("shape,tile", LANE, ids=[f"{_sid(s)}-t{t}" for s, t in LANE])
def test_streaming_lane_taps(C, shape, tile, splits):
    """M = 48 is less than one tile, M = 80 not a multiple of one; Cin 8 on a
    shape the first-layer kernel does not take (H * W = 16)."""
    assert _path(C, shape, tile, splits) == _paths().PATH_STREAMING
    _fwd_and_check(C, _case(shape), tile, splits)
    if shape == (3, 4, 4, 16, 64) and tile == 2:
        _fwd_and_check(C, _case(shape, "randn"), tile, splits)


# --------------------------------------------------------------------------- streaming, uniform taps (Cin >= 64)
UNIFORM = [((3, 4, 4, 64, 64), (1, 2)), ((5, 8, 8, 128, 128), (0, 1, 2)), ((3, 4, 8, 64, 64), (1, 2))]
UNIFORM = [(s, t) for s, tiles in UNIFORM for t in tiles]


@pytest.mark.parametrize("splits", [1, 2, 3, 4])
@pytest.mark.parametrize("shape,tile", UNIFORM, ids=[f"{_sid(s)}-t{t}" for s, t in UNIFORM])
def test_streaming_uniform_taps(C, shape, tile, splits):
    """Every ring depth (2 / 3 / 4 stages) and workgroup size (4 / 8 waves) of
    the tile word, with the fragment-prefetch loop on and off; 25 * Cin / 64
    k-tiles do not divide by 3; M = 320 is two and a half tiles."""
    from torch_distlearn_amd.ops.conv import pack_tile

    case = _case(shape)
    try:
        for pf in (0, 1):
            C.set_conv_fwd_pf(pf)
            for stages in (2, 3, 4):
                for waves in (4, 8):
                    word = pack_tile(tile, stages=stages, waves=waves)
                    assert _path(C, shape, word, splits) == _paths().PATH_STREAMING
                    y, rows, T, _ = _run_fwd(C, case.xp.data_ptr(), case.wd.data_ptr(), shape, word, splits)
                    case.check(y, tile, splits, what=f"y (pf {pf}, {stages} stages, {waves} waves)")
                    case.check_stats(rows, T, y)
    finally:
        C.set_conv_fwd_pf(1)
    if shape == (5, 8, 8, 128, 128) and tile == 0 and splits in (1, 3):
        _fwd_and_check(C, _case(shape, "randn"), tile, splits)


# --------------------------------------------------------------------------- region row tiles
ROWS = [((2, 16, 16, 64, 64), 2, 1), ((1, 16, 16, 128, 128), 0, 1), ((1, 16, 16, 256, 64), 2, 2),
        ((1, 16, 16, 256, 64), 2, 4), ((3, 4, 32, 64, 64), 2, 1), ((2, 8, 16, 64, 64), 2, 1)]


@pytest.mark.parametrize("shape,tile,splits", ROWS, ids=[f"{_sid(s)}-t{t}-s{k}" for s, t, k in ROWS])
def test_region_row_tiles(C, shape, tile, splits):
    """One and two 64-channel chunks per workgroup, four chunks over 2 and 4
    splits, and non-square images (rows per tile come from W)."""
    assert _path(C, shape, tile, splits) == _paths().PATH_REGION_ROWS
    assert C.conv_region_ok(*shape, 5, tile, splits) == 1
    _fwd_and_check(C, _case(shape), tile, splits)
    if shape == (2, 16, 16, 64, 64):
        _fwd_and_check(C, _case(shape, "randn"), tile, splits)


def test_region_rows_four_chunks_unsplit_streams(C):
    """Four channel chunks do not fit one workgroup's LDS: the query reports
    the streaming kernel, and that kernel is exact on the shape."""
    shape = (1, 16, 16, 256, 64)
    assert _path(C, shape, 2, 1) == _paths().PATH_STREAMING
    assert C.conv_region_ok(*shape, 5, 2, 1) == 0
    _fwd_and_check(C, _case(shape), 2, 1)


# --------------------------------------------------------------------------- region image tiles (tile-word bit 16)
# (5, 4, 4, 128, 128) unsplit does not fit (eight images x two chunks of region
# exceed the LDS budget, region_geom): it reaches the image tiles with one
# chunk per workgroup, splits 2; Cin 64 covers eight images per tile unsplit.
IMG = [((3, 8, 8, 64, 64), 2, 1), ((3, 8, 8, 64, 128), 0, 1), ((5, 4, 4, 128, 128), 0, 2), ((5, 4, 4, 128, 128), 2, 2),
       ((5, 4, 4, 64, 128), 0, 1), ((5, 4, 4, 64, 128), 2, 1)]


@pytest.mark.parametrize("shape,tile,splits", IMG, ids=[f"{_sid(s)}-t{t}-s{k}" for s, t, k in IMG])
def test_region_image_tiles(C, shape, tile, splits):
    """Two images per tile with the last tile half empty (B = 3, 8x8), eight
    per tile with the last tile partly empty (B = 5, 4x4); statistics."""
    word = tile | IMAGES
    assert _path(C, shape, word, splits) == _paths().PATH_REGION_IMAGES
    assert _path(C, shape, tile, splits) == _paths().PATH_STREAMING  # without the bit: not a region shape
    _fwd_and_check(C, _case(shape), word, splits)
    if shape == (3, 8, 8, 64, 64):
        _fwd_and_check(C, _case(shape, "randn"), word, splits)


def test_region_images_two_chunks_eight_images_streams(C):
    shape = (5, 4, 4, 128, 128)
    for tile in (0, 2):
        assert _path(C, shape, tile | IMAGES, 1) == _paths().PATH_STREAMING
        _fwd_and_check(C, _case(shape), tile | IMAGES, 1)


# --------------------------------------------------------------------------- position-major tiles
POSM = [((128, 4, 4, 64, 64), 2), ((64, 4, 4, 64, 64), 1), ((128, 8, 8, 64, 64), 2), ((128, 4, 8, 64, 64), 2)]


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("shape,tile", POSM, ids=[f"{_sid(s)}-t{t}" for s, t in POSM])
def test_position_major_tiles(C, shape, tile, splits):
    """Exact, and bitwise the pixel-major tiles' result (set_conv_posm(0))."""
    P = _paths()
    case = _case(shape)
    assert _path(C, shape, tile, splits) == P.PATH_STREAMING | P.PATH_POSM
    y1, rows1 = _fwd_and_check(C, case, tile, splits)
    C.set_conv_posm(0)
    try:
        assert _path(C, shape, tile, splits) == P.PATH_STREAMING
        y0, rows0 = _fwd_and_check(C, case, tile, splits)
    finally:
        C.set_conv_posm(1)
    assert torch.equal(y0, y1)
    if shape == (128, 4, 4, 64, 64):
        _fwd_and_check(C, _case(shape, "randn"), tile, splits)


# --------------------------------------------------------------------------- first-layer (Cin 8 / pair-packed) kernel
C8 = [(1, 16, 16, 8, 64), (3, 8, 16, 8, 64), (1, 4, 32, 8, 64)]


def _pair_pack(w):  # [Cout][5][5][>=3] -> [Cout][5][3][2][4] (dl_common.h pack1_index, cp = -5); pads zero
    q = torch.zeros(w.shape[0], 5, 3, 2, 4, dtype=BF16)
    for kx in range(5):
        q[:, :, kx // 2, kx % 2, :3] = w[:, :, kx, :3]
    return q


C8_CASES = [(s, False) for s in C8] + [(C8[1], True)]
C8_IDS = [_sid(s) + ("-nonzero-pads" if p else "") for s, p in C8_CASES]


@pytest.mark.parametrize("shape,w_pads", C8_CASES, ids=C8_IDS)
def test_first_layer_kernel(C, shape, w_pads):
    """Three real channels of eight (x's channels 3..7 are zero); nonzero
    integers in the weights' pad channels never reach the result."""
    assert _path(C, shape, 2, 1) == _paths().PATH_FIRST_LAYER
    _fwd_and_check(C, _case(shape, "int", 3, w_pads), 2, 1)
    if shape == C8[1] and not w_pads:
        _fwd_and_check(C, _case(shape, "randn", 3), 2, 1)


@pytest.mark.parametrize("shape,w_pads", C8_CASES, ids=C8_IDS)
def test_first_layer_kernel_pair_packed(C, shape, w_pads):
    """The pair-packed form over the 4-channel input (x's channel 3 zero).  The
    packed weights' channel-3 pads may hold anything; the sixth half chunk (the
    partner of the odd last tap) multiplies a real pixel and stays zero."""
    B, H, W, _, cout = shape
    case = _case(shape, "int", 3)
    x4 = _dev(_pad(case.x[..., :4]))
    wq = _pair_pack(case.w)
    if w_pads:
        wq[..., 3] = exact.int_bf16(wq[..., 3].shape, 1, 3, generator=torch.Generator().manual_seed(5))
        wq[:, :, 2, 1, :] = 0
    wq = _dev(wq)
    word = 2 | PAIR
    assert C.conv_fwd_path(B, H, W, 4, cout, 5, word, 1) == _paths().PATH_FIRST_LAYER
    y, rows, T, _ = _run_fwd(C, x4.data_ptr(), wq.data_ptr(), shape, word, 1, cin_arg=4)
    case.check(y, 2)
    case.check_stats(rows, T, y)


# --------------------------------------------------------------------------- in-launch split-K combine
FIX = [(3, 4, 4, 64, 64), (5, 8, 8, 128, 128)]


@pytest.mark.parametrize("splits", [2, 3, 4])
@pytest.mark.parametrize("shape", FIX, ids=_sid)
def test_in_launch_combine(C, shape, splits):
    """conv_fwd_fix: y exact, statistics of the stored values, and two launches
    back to back identical (the arrival counters reset)."""
    case = _case(shape)
    assert C.conv_fix_ok(*shape, 5, 2, splits) == 1
    outs = []
    for _ in range(2):
        y, rows, T, _ = _run_fwd(C, case.xp.data_ptr(), case.wd.data_ptr(), shape, 2, splits, fix=True)
        case.check(y, 2, splits)
        case.check_stats(rows, T, y)
        outs.append((y, rows))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1][:T], outs[1][1][:T])
    if shape == FIX[1] and splits == 3:
        rcase = _case(shape, "randn")
        y, rows, T, _ = _run_fwd(C, rcase.xp.data_ptr(), rcase.wd.data_ptr(), shape, 2, splits, fix=True)
        rcase.check(y, 2, splits)
        rcase.check_stats(rows, T, y)


# --------------------------------------------------------------------------- keep_slabs (bit 20)
SLABS = [((3, 4, 4, 64, 64), 2, 3, "PATH_STREAMING"), ((5, 8, 8, 128, 128), 0, 4, "PATH_STREAMING"),
         ((1, 16, 16, 256, 64), 2, 2, "PATH_REGION_ROWS")]


@pytest.mark.parametrize("shape,tile,splits,path", SLABS, ids=[f"{_sid(s)}-t{t}-s{k}" for s, t, k, _ in SLABS])
def test_keep_slabs(C, shape, tile, splits, path):
    """The fp32 slabs left for the consumer: each an exact integer tensor,
    their fp64 sum the reference exactly; y is not written."""
    case = _case(shape)
    word = tile | KEEP
    assert _path(C, shape, word, splits) == getattr(_paths(), path)
    y, _, T, slab = _run_fwd(C, case.xp.data_ptr(), case.wd.data_ptr(), shape, word, splits, stats=False)
    assert T == 0
    assert torch.isnan(y.float()).all()
    s64 = slab.cpu().double()
    assert torch.isfinite(s64).all() and torch.equal(s64, s64.round())
    exact.assert_exact(s64.sum(0).float().reshape(case.ref.shape), case.ref, "slab sum", tile=(_BM[tile], _BN[tile]),
                       row_dims=3)
    assert float(s64.abs().amax()) < exact.EXACT_LIMIT


# --------------------------------------------------------------------------- conv_fwd_add
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("M,cin,cout,tile", [(200, 64, 64, 2), (200, 128, 128, 0), (70, 64, 64, 1)])
def test_fwd_add_1x1(C, M, cin, cout, tile, masked):
    """y = bf16(conv + addend) of a 1x1 conv (M pixels as 1x1 images), integer
    addend, with and without the per-channel mask bits (uint8 [M][Cout / 8])."""
    g = torch.Generator().manual_seed(M + cin + tile)
    a = exact.magnitude(cin)
    exact.check_exact_range(cin, a, a)
    x = exact.int_bf16((M, 1, 1, cin), -a, a, generator=g)
    w = exact.int_bf16((cout, 1, 1, cin), -a, a, generator=g)
    add = exact.int_bf16((M, 1, 1, cout), -200, 200, generator=g)
    ref, _ = exact.conv_ref64(x, w, pad=0, with_abs=False)
    bits = torch.randint(0, 256, (M, cout // 8), generator=g).to(torch.uint8)
    keep = ((bits.unsqueeze(-1).int() >> torch.arange(8)) & 1).reshape(M, 1, 1, cout).double()
    want = ref + add.double() * (keep if masked else 1.0)
    assert C.conv_fwd_path(M, 1, 1, cin, cout, 1, tile, 1) & 3 == _paths().PATH_STREAMING
    xd, wd, addd, bitsd = _dev(x), _dev(w), _dev(add), _dev(bits)
    y = torch.full((M, 1, 1, cout), NAN, dtype=BF16, device="cuda")
    C.conv_fwd_add(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), addd.data_ptr(), M, 1, 1, cin, cout, 1, tile, _s(),
                   bitsd.data_ptr() if masked else 0)
    torch.cuda.synchronize()
    exact.assert_exact(y, want, "y", tile=(_BM[tile], _BN[tile]), row_dims=3)


def test_fwd_add_5x5_streaming(C):
    """The addend epilogue of a 5x5 conv (region kernels off for the call)."""
    shape = (3, 4, 4, 64, 64)
    B, H, W, cin, cout = shape
    case = _case(shape)
    add = exact.int_bf16((B, H, W, cout), -200, 200, generator=torch.Generator().manual_seed(9))
    addd = _dev(add)
    y = torch.full((B, H, W, cout), NAN, dtype=BF16, device="cuda")
    C.set_conv_region(0)
    try:
        assert _path(C, shape, 2, 1) == _paths().PATH_STREAMING
        C.conv_fwd_add(case.xp.data_ptr(), case.wd.data_ptr(), y.data_ptr(), addd.data_ptr(), B, H, W, cin, cout, 5, 2,
                       _s(), 0)
        torch.cuda.synchronize()
    finally:
        C.set_conv_region(1)
    exact.assert_exact(y, case.ref + add.double(), "y", tile=(128, 64), row_dims=3)


# --------------------------------------------------------------------------- dgrad end to end
# (B, H, W, Cin, Cout) of the conv_fwd call: Cin = the channels of dy, Cout = those of dx
DGRAD = [((2, 16, 16, 128, 64), 2, "PATH_REGION_ROWS"), ((3, 4, 4, 64, 128), 0, "PATH_STREAMING")]


@pytest.mark.parametrize("shape,tile,path", DGRAD, ids=[f"{_sid(s)}-t{t}" for s, t, _ in DGRAD])
def test_dgrad_end_to_end(C, shape, tile, path):
    """weight_flip_transpose then conv_fwd gives the fp64 autograd dx exactly."""
    B, H, W, cdy, cdx = shape
    g = torch.Generator().manual_seed(cdy + cdx)
    a = exact.magnitude(25 * cdy)
    exact.check_exact_range(25 * cdy, a, a)
    dy = exact.int_bf16((B, H, W, cdy), -a, a, density=0.9, generator=g)
    w = exact.int_bf16((cdy, 5, 5, cdx), -a, a, generator=g)  # the forward layer's weights: cdx -> cdy channels
    dx_ref, _ = exact.dgrad_ref64(dy, w, (H, W), with_abs=False)
    wd = _dev(w)
    wt = torch.full((cdx, 5, 5, cdy), NAN, dtype=BF16, device="cuda")
    C.weight_flip_transpose(wd.data_ptr(), wt.data_ptr(), cdy, cdx, 5, _s())
    torch.cuda.synchronize()
    assert torch.equal(wt.cpu(), w.permute(3, 1, 2, 0).flip(1, 2).contiguous())
    assert _path(C, shape, tile, 1) == getattr(_paths(), path)
    dyp = _dev(_pad(dy))
    dx, _, _, _ = _run_fwd(C, dyp.data_ptr(), wt.data_ptr(), shape, tile, 1, stats=False)
    exact.assert_exact(dx, dx_ref, "dx", tile=(_BM[tile], _BN[tile]), row_dims=3)


# --------------------------------------------------------------------------- conv_wgrad + the slab reducers
def _split_rows(M, splits):
    """Rows [mbeg, mend) of each split (conv_wgrad: 64-row aligned shares)."""
    mps = ((M + splits - 1) // splits + 63) // 64 * 64
    return [(min(M, s * mps), min(M, (s + 1) * mps)) for s in range(splits)]


def _check_wgrad_slabs(slabs, x, dy, KH, KW, stride, pad, splits, view, tile):
    """Every slab equals the fp64 weight gradient of its own rows of dy exactly
    -- a split past the end of M writes zeros, and no element keeps the NaN
    pre-fill: each launch writes all of [splits][Cout][ldo] (conv_wgrad_dev.h
    stores every tile of every split).  view(slab) -> [Cout][KH][KW][C]."""
    B, Ho, Wo, cout = dy.shape
    M = B * Ho * Wo
    bm = 64 if tile == 1 else 128
    total = torch.zeros_like(view(slabs[0]).cpu().double())
    for s, (mbeg, mend) in enumerate(_split_rows(M, splits)):
        dys = torch.zeros_like(dy).reshape(M, cout)
        dys[mbeg:mend] = dy.reshape(M, cout)[mbeg:mend]
        part, _ = exact.wgrad_ref64(x, dys.reshape(dy.shape), KH, KW, stride, pad, with_abs=False)
        got = view(slabs[s]).cpu()
        exact.assert_exact(got, part[..., :got.shape[-1]], f"slab {s} (rows {mbeg}..{mend})", tile=(bm, bm), row_dims=1)
        total += part[..., :got.shape[-1]]
    return total


def _check_reducers(C, slabs, dw_ref, splits, cout, taps, Cp, Creal):
    """slab_reduce exact against dW; slab_reduce_add exact onto integers;
    slab_reduce_add_oihw exact onto an OIHW destination."""
    ref = dw_ref[..., :Creal].reshape(cout, taps, Creal)
    dw = torch.full((cout, taps, Creal), NAN, device="cuda")
    C.slab_reduce(slabs.data_ptr(), dw.data_ptr(), splits, cout, taps, Cp, Creal, _s())
    g = torch.Generator().manual_seed(cout + taps)
    base = exact.int_bf16((cout, taps, Creal), -100, 100, generator=g).float()
    acc, acc_oihw = _dev(base), _dev(base.permute(0, 2, 1))
    C.slab_reduce_add(slabs.data_ptr(), acc.data_ptr(), splits, cout, taps, Cp, Creal, _s())
    C.slab_reduce_add_oihw(slabs.data_ptr(), acc_oihw.data_ptr(), splits, cout, taps, Cp, Creal, _s())
    torch.cuda.synchronize()
    exact.assert_exact(dw, ref, "slab_reduce", row_dims=1)
    exact.assert_exact(acc, ref + base.double(), "slab_reduce_add", row_dims=1)
    exact.assert_exact(acc_oihw, (ref + base.double()).permute(0, 2, 1), "slab_reduce_add_oihw", row_dims=1)


def _wgrad_operands(B, H, W, cin, cout, real_c, seed):
    g = torch.Generator().manual_seed(seed)
    a = exact.magnitude(B * H * W)  # the reduction runs over the M = B*H*W pixels
    exact.check_exact_range(B * H * W, a, a)
    x = exact.int_bf16((B, H, W, cin), -a, a, generator=g)
    x[..., real_c:] = 0
    dy = exact.int_bf16((B, H, W, cout), -a, a, density=0.9, generator=g)
    return x, dy


# (B, H, W, Cin, Cout), tile, real input channels: M = 48, 80, 320, 512, 96
WGRAD = [((3, 4, 4, 8, 64), 1, 3), ((5, 4, 4, 16, 64), 1, 16), ((5, 8, 8, 64, 128), 2, 64), ((5, 8, 8, 64, 128), 1, 64),
         ((2, 16, 16, 64, 128), 2, 64), ((3, 4, 4, 256, 128), 2, 256), ((3, 4, 8, 64, 64), 1, 64)]


@pytest.mark.parametrize("splits", [1, 3, 4])
@pytest.mark.parametrize("shape,tile,real_c", WGRAD, ids=[f"{_sid(s)}-t{t}" for s, t, _ in WGRAD])
def test_wgrad_and_reducers(C, shape, tile, real_c, splits):
    B, H, W, cin, cout = shape
    x, dy = _wgrad_operands(B, H, W, cin, cout, real_c, B * H + cin + cout)
    K = 25 * cin
    xp, dyp = _dev(_pad(x)), _dev(_pad(dy))
    slabs = torch.full((splits, cout, K), NAN, device="cuda")
    C.conv_wgrad(dyp.data_ptr(), xp.data_ptr(), slabs.data_ptr(), B, H, W, cin, cout, 5, splits, K, tile, 0, _s())
    torch.cuda.synchronize()
    dw_ref = _check_wgrad_slabs(slabs, x, dy, 5, 5, 1, 2, splits, lambda s: s.view(cout, 5, 5, cin), tile)
    assert not dw_ref[..., real_c:].any()  # zero input channels: zero gradient
    _check_reducers(C, slabs, dw_ref, splits, cout, 25, cin, real_c)


def test_wgrad_row_stride_past_k(C):
    """ldo > K: the columns between K and ldo inside the last K tile are
    written as zeros (K-tail lanes load zeros), in every split."""
    B, H, W, cin, cout, splits = 5, 4, 4, 16, 64, 3
    x, dy = _wgrad_operands(B, H, W, cin, cout, cin, 21)
    K, ldo = 25 * cin, 25 * cin + 8  # the 64-wide K tiles reach 448 > ldo
    xp, dyp = _dev(_pad(x)), _dev(_pad(dy))
    slabs = torch.full((splits, cout, ldo), NAN, device="cuda")
    C.conv_wgrad(dyp.data_ptr(), xp.data_ptr(), slabs.data_ptr(), B, H, W, cin, cout, 5, splits, ldo, 1, 0, _s())
    torch.cuda.synchronize()
    _check_wgrad_slabs(slabs, x, dy, 5, 5, 1, 2, splits, lambda s: s[:, :K].reshape(cout, 5, 5, cin), 1)
    assert not slabs[:, :, K:].any() and torch.isfinite(slabs).all()


@pytest.mark.parametrize("splits", [1, 3])
def test_wgrad_pair_packed(C, splits):
    """The pair-packed first layer (tile bit 24): the B chunk is two adjacent
    pixels of the 4-channel input, K = 120; slab_reduce with Cp = -5."""
    B, H, W, cout = 2, 8, 16, 64
    x, dy = _wgrad_operands(B, H, W, 4, cout, 3, 77)
    x4p, dyp = _dev(_pad(x)), _dev(_pad(dy))
    slabs = torch.full((splits, cout, 120), NAN, device="cuda")
    C.conv_wgrad(dyp.data_ptr(), x4p.data_ptr(), slabs.data_ptr(), B, H, W, 4, cout, 5, splits, 120, 1 | PAIR, 0, _s())
    torch.cuda.synchronize()

    def unpack(s):  # [Cout][5][3][2][4] -> [Cout][5][5][4]: tap kx = chunk kx // 2, half kx % 2
        p = s.view(cout, 5, 3, 2, 4)
        return torch.stack([p[:, :, kx // 2, kx % 2, :] for kx in range(5)], 2)

    dw_ref = _check_wgrad_slabs(slabs, x, dy, 5, 5, 1, 2, splits, unpack, 1)
    assert torch.isfinite(slabs).all()
    _check_reducers(C, slabs, dw_ref, splits, cout, 25, -5, 3)


# --------------------------------------------------------------------------- conv_fwd_ex / conv_wgrad_ex
# Generalised geometry never takes the region / first-layer kernels or the
# position-major tiles (make_geom_ex: pow2 = 0; fwd_posm needs the "same"
# padding), so these cases have no dispatch to assert.
# (N, Hi, Cin, Cout, K, stride, pad)
EX = [(3, 8, 64, 128, 1, 2, 0), (2, 7, 64, 128, 3, 2, 1), (3, 14, 64, 64, 3, 2, 1)]


def _ex_operands(N, Hi, cin, cout, k, red, seed):
    g = torch.Generator().manual_seed(seed)
    a = exact.magnitude(red)
    exact.check_exact_range(red, a, a)
    x = exact.int_bf16((N, Hi, Hi, cin), -a, a, generator=g)
    w = exact.int_bf16((cout, k, k, cin), -a, a, generator=g)
    return x, w, a, g


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("shape", EX, ids=_sid)
def test_fwd_ex_strided(C, shape, splits):
    N, Hi, cin, cout, k, S, p = shape
    x, w, _, _ = _ex_operands(N, Hi, cin, cout, k, k * k * cin, sum(shape))
    Ho = (Hi + 2 * p - k) // S + 1
    ref, _ = exact.conv_ref64(x, w, stride=S, pad=p, with_abs=False)
    xp, wd = _dev(_pad(x, p)), _dev(w)
    tile = 0 if cout % 128 == 0 else 2
    M = N * Ho * Ho
    y = torch.full((N, Ho, Ho, cout), NAN, dtype=BF16, device="cuda")
    rows = torch.full(((M + 127) // 128 + 2, 2, cout), NAN, device="cuda")
    slab = torch.full((splits, M, cout), NAN, device="cuda")
    T = C.conv_fwd_ex(xp.data_ptr(), wd.data_ptr(), y.data_ptr(), rows.data_ptr() if splits == 1 else 0,
                      slab.data_ptr() if splits > 1 else 0, N, Ho, Ho, Hi + 2 * p, Hi + 2 * p, cin, cout, k, k, S, 0, 0,
                      0, 0, 0, 0, tile, splits, _s())
    torch.cuda.synchronize()
    exact.assert_exact(y, ref, "y", tile=(128, _BN[tile]), row_dims=3)
    if splits == 1:
        exact.assert_stats(rows, exact.expected(ref, BF16), T)


@pytest.mark.parametrize("cin", [16, 64])
def test_fwd_ex_output_map_accumulate(C, cin):
    """A 4x4 'valid' conv stored through the output map at (2 oh + 1, 2 ow) of
    a larger tensor, accumulated onto its integer content; every other pixel
    is unchanged (Cin 16: per-lane taps, 64: uniform taps)."""
    N, Ho, cout, k = 3, 6, 64, 4
    Hp = Ho + k - 1
    x, w, _, g = _ex_operands(N, Hp, cin, cout, k, k * k * cin, cin)
    ref, _ = exact.conv_ref64(x, w, pad=0, with_abs=False)
    Hf = 2 * Ho + 1
    before = exact.int_bf16((N, Hf, Hf, cout), -200, 200, generator=g)
    full = _dev(before)
    xd, wd = _dev(x), _dev(w)
    C.conv_fwd_ex(xd.data_ptr(), wd.data_ptr(), full.data_ptr(), 0, 0, N, Ho, Ho, Hp, Hp, cin, cout, k, k, 1, 2, 1, 0,
                  Hf, Hf * Hf, full.data_ptr(), 2, 1, _s())
    torch.cuda.synchronize()
    want = before.double()
    want[:, 1::2, 0:2 * Ho:2, :] += ref
    exact.assert_exact(full, want, "mapped output", tile=(128, 64), row_dims=3)


# (N, Hi, Cin, Cout, K, stride, pad, dy interior pad); Hi of the 4x4 cases is the buffer (valid conv)
WG_EX = [(3, 8, 64, 128, 1, 2, 0, 0), (2, 7, 64, 128, 3, 2, 1, 0), (2, 7, 64, 128, 3, 2, 1, 1),
         (2, 9, 16, 64, 4, 1, 0, 0), (2, 9, 64, 64, 4, 1, 0, 1)]


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("shape", WG_EX, ids=_sid)
def test_wgrad_ex(C, shape, splits):
    N, Hi, cin, cout, k, S, p, dp = shape
    Ho = (Hi + 2 * p - k) // S + 1
    g = torch.Generator().manual_seed(sum(shape))
    a = exact.magnitude(N * Ho * Ho)
    exact.check_exact_range(N * Ho * Ho, a, a)
    x = exact.int_bf16((N, Hi, Hi, cin), -a, a, generator=g)
    dy = exact.int_bf16((N, Ho, Ho, cout), -a, a, density=0.9, generator=g)
    xp, dyp = _dev(_pad(x, p)), _dev(_pad(dy, dp))
    K = k * k * cin
    tile = 2 if cout % 128 == 0 else 1
    slabs = torch.full((splits, cout, K), NAN, device="cuda")
    C.conv_wgrad_ex(dyp.data_ptr(), xp.data_ptr(), slabs.data_ptr(), N, Ho, Ho, Hi + 2 * p, Hi + 2 * p, Ho + 2 * dp,
                    Ho + 2 * dp, dp, cin, cout, k, k, S, splits, K, tile, _s())
    torch.cuda.synchronize()
    dw_ref = _check_wgrad_slabs(slabs, x, dy, k, k, S, p, splits, lambda s: s.view(cout, k, k, cin), tile)
    _check_reducers(C, slabs, dw_ref, splits, cout, k * k, cin, cin)
