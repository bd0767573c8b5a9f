"""The learning rate read from device memory (csrc/kernels/sgd_dev.h sgd_rate):
every update kernel given ``lr_dev`` -> value v produces BITWISE what it
produces with the immediate ``lr = v`` (the parent's kernels, checked against
PyTorch in test_flat_ops_gpu.py), and ``lr_ring_set`` writes exactly the
values it is given, nothing beside them."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# 4 elements; two ragged 256-thread blocks; the smallest size at which a thread
# of the capped grid (csrc dl_common.h stream_grid: at most 2048 blocks of 256)
# takes a second float4: 4 * (2048 * 256 + 257) floats = 8 MiB per buffer
GRID_CAP, BLOCK = 2048, 256
SIZES = [4, 4 * 257, 4 * (GRID_CAP * BLOCK + 257)]
COUNTS = [1.0, 3.0]
MU, WD = 0.9, 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from torch_distlearn_amd import _native

    _native.native()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rate():
    from torch_distlearn_amd.schedules import as_fp32

    return as_fp32(0.0123)  # not a power of two: every mantissa bit of the rate matters


def _s():
    return torch.cuda.current_stream().cuda_stream


def _state(dev, n, seed, mom, shadow):
    g0 = torch.Generator(device=dev).manual_seed(seed)
    p = torch.randn(n, device=dev, generator=g0)
    g = torch.randn(n, device=dev, generator=g0)
    m = torch.randn(n, device=dev, generator=g0) if mom else None
    sh = torch.zeros(n, dtype=torch.bfloat16, device=dev) if shadow else None
    return p, g, m, sh


def _same(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y)


# --------------------------------------------------------------------------- lr_ring_set
@pytest.mark.parametrize("offset", [0, 5])
@pytest.mark.parametrize("count", [1, 16, 32, 33])
def test_lr_ring_set(dev, offset, count):
    """1, 16, 32 values in one launch and 33 in two, at offsets 0 and 5: read
    back exactly, the neighbouring floats untouched."""
    from torch_distlearn_amd.ops.flat import lr_ring_set_

    ring = torch.full((64,), -7.0, device=dev)
    vals = torch.randn(count, generator=torch.Generator().manual_seed(count + offset)).tolist()
    lr_ring_set_(ring, offset, vals)
    torch.cuda.synchronize()
    want = torch.full((64,), -7.0)
    want[offset:offset + count] = torch.tensor(vals, dtype=torch.float32)
    assert torch.equal(ring.cpu(), want)


def test_lr_ring_set_checks_bounds(dev):
    from torch_distlearn_amd import _native
    from torch_distlearn_amd.ops.flat import lr_ring_set_

    C = _native.native()
    ring = torch.zeros(64, device=dev)
    with pytest.raises(RuntimeError):
        C.lr_ring_set(ring.data_ptr(), 64, 0, [0.1] * 33, _s())  # one launch carries 32
    with pytest.raises(RuntimeError):
        C.lr_ring_set(ring.data_ptr(), 64, 40, [0.1] * 25, _s())  # past the end
    with pytest.raises(RuntimeError):
        C.lr_ring_set(ring.data_ptr(), 64, -1, [0.1], _s())
    with pytest.raises(RuntimeError):
        C.lr_ring_set(ring.data_ptr(), 64, 0, [], _s())
    with pytest.raises(ValueError):
        lr_ring_set_(ring, 60, [0.1] * 5)
    torch.cuda.synchronize()
    assert not ring.any()


# --------------------------------------------------------------------------- sgd_update / _g16
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mom", [False, True])
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("g16", [False, True], ids=["fp32grad", "bf16grad"])
def test_device_rate_is_bitwise_immediate(dev, rate, n, mom, shadow, count, g16):
    from torch_distlearn_amd.ops.flat import sgd_update_

    slot = torch.tensor([count], device=dev)
    lr_dev = torch.tensor([rate], device=dev)
    outs = []
    for lr in (rate, lr_dev):
        p, g, m, sh = _state(dev, n, n + 1, mom, shadow)
        if g16:
            g = g.to(torch.bfloat16)
        p0 = p.clone()
        sgd_update_(p, g, lr, slot=slot, mom=m, momentum=MU, weight_decay=WD, shadow=sh)
        torch.cuda.synchronize()
        assert not torch.equal(p, p0)
        outs.append((p, m, sh))
    _same(*outs)
    assert float(lr_dev) == rate  # the kernels only read it


def test_device_rate_matches_fp64_formula(dev, rate):
    """One variant (momentum + shadow, 3 participants) against the update formula in
    fp64, with test_flat_ops_gpu.py's tolerance for the immediate path."""
    from torch_distlearn_amd.ops.flat import sgd_update_

    n, count = SIZES[1], 3.0
    p, g, m, sh = _state(dev, n, 99, True, True)
    d = g.double() / count + WD * p.double()
    mref = MU * m.double() + d
    pref = p.double() - rate * mref
    sgd_update_(p, g, torch.tensor([rate], device=dev), slot=torch.tensor([count], device=dev), mom=m, momentum=MU,
                weight_decay=WD, shadow=sh)
    torch.cuda.synchronize()
    torch.testing.assert_close(p, pref.float(), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(m, mref.float(), rtol=1e-6, atol=1e-6)
    assert torch.equal(sh, p.to(torch.bfloat16))


def test_tensor_rate_is_validated(dev, rate):
    from torch_distlearn_amd.ops.flat import sgd_update_

    p, g, _, _ = _state(dev, 8, 1, False, False)
    for bad in (torch.tensor([rate, rate], device=dev), torch.tensor([rate], dtype=torch.float64, device=dev),
                torch.tensor([rate])):
        with pytest.raises(ValueError):
            sgd_update_(p, g, bad)
    # CPU parameters: a tensor rate is read with float()
    pc, gc = p.cpu(), g.cpu()
    want = pc - rate * gc
    sgd_update_(pc, gc, torch.tensor([rate]))
    torch.testing.assert_close(pc, want, rtol=1e-6, atol=1e-6)


# --------------------------------------------------------------------------- sgd_update_slabs
def _slab_case(dev, n, kind, seed):
    """(slabs, tail, skip) for a buffer of n floats.  ranges: one in-place range
    of 5 splits (summed sequentially); ranges+skip: one of 19 splits (8 lanes +
    shuffle tree) and a skipped suffix; tail: a channel-padded range (3 of 8
    channels, 40 splits: 32 lanes) reduced by extra blocks of the launch."""
    g0 = torch.Generator(device=dev).manual_seed(seed)
    n4 = n // 4
    off, ln = 4 * (n4 // 3), min(256, n - 4 * (n4 // 3))
    if kind == "ranges":
        return [(off, ln, torch.randn(5 * ln, device=dev, generator=g0), 5)], None, None
    if kind == "ranges+skip":
        lo = n - 4 * (n4 // 4)
        return [(off, ln, torch.randn(19 * ln, device=dev, generator=g0), 19)], None, ((lo, n) if lo < n else None)
    cout, taps, cp, c = (8, 25, 8, 3) if n >= 604 else (1, 1, 8, 4)
    o = 4 if n >= 604 else 0
    t = torch.randn(40 * cout * taps * cp, device=dev, generator=g0)
    return None, (o, cout * taps * c, t, 40, cout, taps, cp, c), None


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["ranges", "ranges+skip", "tail"])
@pytest.mark.parametrize("mom", [False, True])
@pytest.mark.parametrize("count", COUNTS)
def test_device_rate_slabs_is_bitwise_immediate(dev, rate, n, kind, mom, count):
    from torch_distlearn_amd.ops.flat import sgd_update_

    slabs, tail, skip = _slab_case(dev, n, kind, n + 3)
    slot = torch.tensor([count], device=dev)
    outs = []
    for lr in (rate, torch.tensor([rate], device=dev)):
        p, g, m, sh = _state(dev, n, n + 2, mom, True)
        p0 = p.clone()
        sgd_update_(p, g, lr, slot=slot, mom=m, momentum=MU, weight_decay=WD, shadow=sh, slabs=slabs, tail=tail,
                    skip=skip)
        torch.cuda.synchronize()
        if skip is not None:
            assert torch.equal(p[skip[0]:skip[1]], p0[skip[0]:skip[1]])
        assert not torch.equal(p, p0)
        outs.append((p, m, sh))
    _same(*outs)


# --------------------------------------------------------------------------- side job of a conv launch
@pytest.mark.parametrize("mom", [False, True])
def test_side_job_device_rate_is_bitwise_immediate(dev, rate, mom):
    """A streaming conv_fwd launch carrying the update of elements [lo, hi) as
    extra workgroups (side_sgd_job), built with lr_dev and with the
    immediate value: the updated range is bitwise equal (and so is the conv).
    Shape: the smallest of test_convnet_gpu.py's streaming shapes."""
    from torch_distlearn_amd import _native

    C = _native.native()
    B, H, cin, cout, tile = 3, 8, 16, 64, 1
    g0 = torch.Generator(device=dev).manual_seed(17)
    x = F.pad(torch.randn(B, H, H, cin, device=dev, generator=g0).to(torch.bfloat16), (0, 0, 2, 2, 2, 2)).contiguous()
    w = (torch.randn(cout, 5, 5, cin, device=dev, generator=g0) * 0.05).to(torch.bfloat16)
    n, lo, hi = 4 * 257 * 3, 4 * 100, 4 * 700  # three blocks of side work, ragged
    off, ln = 4 * 300, 256
    slab = torch.randn(5 * ln, device=dev, generator=g0)
    slot = torch.tensor([3.0], device=dev)
    lr_dev = torch.tensor([rate], device=dev)
    outs = []
    for imm, ptr in ((rate, 0), (0.0, lr_dev.data_ptr())):
        p, g, m, sh = _state(dev, n, 23, mom, True)
        p0 = p.clone()
        y = torch.empty(B, H, H, cout, dtype=torch.bfloat16, device=dev)
        C.set_conv_region(0)  # the streaming kernel hosts side jobs
        try:
            job = C.side_sgd_job(p.data_ptr(), g.data_ptr(), 0 if m is None else m.data_ptr(), sh.data_ptr(),
                                 slot.data_ptr(), imm, MU, WD, lo, hi, [off], [ln], [slab.data_ptr()], [5], 0, ptr)
            C.conv_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), 0, 0, B, H, H, cin, cout, 5, tile, 1, _s(),
                       side=job)
        finally:
            C.set_conv_region(1)
        torch.cuda.synchronize()
        assert torch.equal(p[:lo], p0[:lo]) and torch.equal(p[hi:], p0[hi:])
        assert not torch.equal(p[lo:hi], p0[lo:hi])
        outs.append((p, m, sh, y))
    _same(*outs)
