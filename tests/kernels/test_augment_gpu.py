"""Random crop / flip inside the device-side gather (csrc/kernels/prep_dev.h
prep_pad_block_aug), bit for bit.

The oracle does not depend on how the normalisation rounds: the un-augmented
kernel runs on the same inputs (its output is checked by the existing
``Prep.check``), tests/kernels/augment_ref.py shifts / mirrors / zero-fills
each sample of its interior on the CPU with the parameters of
``augment_params``, and the augmented launch must produce exactly those bits
-- pad channels zero, the sentinel border of ``xp`` untouched, labels and the
step counter as without augmentation.  The buffers, the ring order (which
holds the dataset's last sample) and the update state come from
tests/kernels/test_update_exact_gpu.py and exact_update.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.kernels import augment_ref as ar
from tests.kernels import exact_update as xu
from tests.kernels import test_update_exact_gpu as tu
from torch_distlearn_amd.data import Augment, augment_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS = tu._STEPS  # 0, 2, 2^33 + 5
BASE = 1000  # the loader's draw count ahead of the device counter (non-zero: a resumed run)
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from torch_distlearn_amd import _native

    return _native.native()


@pytest.fixture(autouse=True)
def _release():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    tu._KEEP.clear()


def _signed(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def _params(seed, base, step, B, pad, flip):
    return [augment_params(seed, ((base + step) * B + b) & M64, pad, bool(flip)) for b in range(B)]


def _gather(C, pr, xp, lab, aug=None):
    """The stand-alone prep launch: gather only (no pack, no transposes, no zero job)."""
    extra = () if aug is None else (aug,)
    C.prep_step_gather(*pr.gather_args(xp, lab), 0, xp.data_ptr(), 0, 0, 3, 8, [], [], [], [], [], [], tu._s(), *extra)
    torch.cuda.synchronize()


def _reference(C, pr):
    """(xp bits, labels) of the un-augmented kernel, checked against fp64."""
    xp, lab = pr.fresh()
    _gather(C, pr, xp, lab)
    pr.check(xp, lab, "un-augmented reference")
    return tu._h(xp), tu._h(lab)


def _want(ref, pr, prm, pad):
    sp, H, W = pr.sp, pr.H, pr.W
    want = ref.copy()
    want[:, sp:sp + H, sp:sp + W] = ar.augment_batch(ref[:, sp:sp + H, sp:sp + W], prm, pad)
    return want


def _check(pr, xp, lab, ref, ref_lab, prm, pad, what):
    sp, H, W = pr.sp, pr.H, pr.W
    got = tu._h(xp)
    tu.assert_bits(got, _want(ref, pr, prm, pad), what)
    assert not got[:, sp:sp + H, sp:sp + W, 3:].any(), f"{what}: pad channels must be exactly zero"
    border = np.ones(got.shape[:3], bool)
    border[:, sp:sp + H, sp:sp + W] = False
    assert np.all(got[border] == tu.SH_SENT), f"{what}: the spatial border was written"
    tu.assert_bits(lab, ref_lab, f"{what}: labels")
    assert np.array_equal(tu._h(pr.d_ctr), pr.ctr0), f"{what}: the step counter changed"


QUAD = [((8, 8, 8), p) for p in range(4)] + [((8, 8, 4), p) for p in range(4)]
GENERIC = [((4, 6, 8), p) for p in range(2)] + [((8, 8, 16), p) for p in range(2)]


@pytest.mark.parametrize("step", STEPS, ids=["step0", "step2", "step2p33"])
@pytest.mark.parametrize("shape,pad", QUAD + GENERIC,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"pad{v}")
def test_augmented_gather_exact(C, shape, pad, step):
    """Quad path (8x8, Cp 8 / 4) at pads 0..3, generic path (4x6; Cp 16) at
    pads 0 and 1; flip on and off; B 6 rows over the 7-entry ring."""
    H, W, Cp = shape
    pr = tu.Prep(H, W, Cp, step, B=6)
    assert 3 in xu.gather_samples(tu._ORDER, step, 6)  # the dataset's last sample is gathered
    ref, ref_lab = _reference(C, pr)
    for flip in (1, 0):
        seed = 0x1234567 * (pad + 1) + flip
        d_aug = tu._d(np.array([seed, BASE], np.int64))
        prm = _params(seed, BASE, step, 6, pad, flip)
        xp, lab = pr.fresh()
        _gather(C, pr, xp, lab, C.augment(d_aug.data_ptr(), pad, flip, 4))
        _check(pr, xp, lab, ref, ref_lab, prm, pad, f"{shape} pad {pad} flip {flip} step {step}")
        assert np.array_equal(tu._h(d_aug), [seed, BASE])
        if pad == 0 and flip == 0:
            tu.assert_bits(xp, ref, "pad 0, flip 0 = the un-augmented kernel")


@pytest.mark.parametrize("Cp", [8, 4])
def test_every_triple_at_pad2(C, Cp):
    """Seed 0, B 40, steps 0..14 = draw indices 0..599: all 50 (flip, dx, dy)
    of pad 2 on 8x8 (asserted from augment_params before any launch)."""
    draws = [_params(0, 0, s, 40, 2, 1) for s in range(15)]
    assert {t for d in draws for t in d} == ar.triples(2) and len(ar.triples(2)) == 50
    d_aug = tu._d(np.array([0, 0], np.int64))
    for s in range(15):
        pr = tu.Prep(8, 8, Cp, s, B=40)
        ref, ref_lab = _reference(C, pr)
        xp, lab = pr.fresh()
        _gather(C, pr, xp, lab, C.augment(d_aug.data_ptr(), 2, 1, 4))
        _check(pr, xp, lab, ref, ref_lab, draws[s], 2, f"coverage step {s}")


def test_seed_uses_all_64_bits(C):
    """A seed with the top bit set and a base that wraps the draw index."""
    seed, base, step = 2 ** 63 + 5, 2 ** 64 - 3, 2
    pr = tu.Prep(8, 8, 8, step, B=6)
    ref, ref_lab = _reference(C, pr)
    d_aug = tu._d(np.array([_signed(seed), _signed(base)], np.int64))
    xp, lab = pr.fresh()
    _gather(C, pr, xp, lab, C.augment(d_aug.data_ptr(), 3, 1, 4))
    _check(pr, xp, lab, ref, ref_lab, _params(seed, base, step, 6, 3, 1), 3, "64-bit seed")


def test_pad_not_smaller_than_the_image_throws(C):
    pr = tu.Prep(4, 6, 8, 0)
    xp, lab = pr.fresh()
    d_aug = tu._d(np.array([1, 0], np.int64))
    with pytest.raises(RuntimeError, match="smaller than the image"):
        _gather(C, pr, xp, lab, C.augment(d_aug.data_ptr(), 4, 1, 4))
    assert np.all(tu._h(xp) == tu.SH_SENT) and np.all(tu._h(lab) == -1)


@pytest.mark.parametrize("step", STEPS, ids=["step0", "step2", "step2p33"])
@pytest.mark.parametrize("shape", [(8, 8, 8), (8, 8, 4), (4, 6, 8)], ids=lambda s: "x".join(map(str, s)))
def test_augmented_gather_carried_by_update(C, shape, step):
    """The update launch carrying next_prep(..., aug) = the stand-alone
    prep_step_gather(..., aug) in bits (quad and generic shape), and the
    update and the first-layer pack of the same launch are still exact."""
    H, W, Cp = shape
    pad, seed = 1, 77
    w1_cp = 8 if Cp != 4 else -5
    pr = tu.Prep(H, W, Cp, step)
    ref, ref_lab = _reference(C, pr)
    d_aug = tu._d(np.array([seed, BASE], np.int64))
    aug = C.augment(d_aug.data_ptr(), pad, 1, 4)
    xp, lab = pr.fresh()
    prep_args = pr.gather_args(xp, lab)
    st, w1p, _ = tu._w1_update(C, "real", "tail", w1_cp, prep_args)
    cout, taps, c = tu._W1
    st.update_slabs(C, next_prep=C.next_prep(*prep_args, [], [], w1p.data_ptr(), w1_cp, 8, cout * taps * c, aug))
    torch.cuda.synchronize()
    _check(pr, xp, lab, ref, ref_lab, _params(seed, BASE, step, 3, pad, 1), pad, f"carried {shape} step {step}")
    p = st.check("update carrying the augmented gather")
    tu._check_w1p(w1p, p, w1_cp, "first-layer pack")
    xp2, lab2 = pr.fresh()
    _gather(C, pr, xp2, lab2, aug)
    tu.assert_bits(xp2, tu._h(xp), "prep_step_gather(aug) vs the carried gather")
    tu.assert_bits(lab2, tu._h(lab), "labels")


# --------------------------------------------------------------------------- through the executor and the trainer
@pytest.fixture
def deterministic(monkeypatch):
    monkeypatch.setenv("DISTLEARN_REDUCE_ATOMIC", "0")  # as tests/kernels/test_engine_gpu.py


AUG = Augment(pad=4, flip=True, seed=11)


def _loader(dev, aug=None):
    from torch_distlearn_amd.data import DeviceLoader, PartitionedDataset, synthetic_cifar10

    imgs, labels = synthetic_cifar10(200, seed=5)
    return DeviceLoader(PartitionedDataset(imgs, labels, device=dev), "permutation", 32, seed=3, augment=aug)


def test_executor_gathers_augmented_batches(C, deterministic):
    from torch_distlearn_amd.models import CifarConvNet, make_executor
    from torch_distlearn_amd.ops.flat import FlatParams

    dev = torch.device("cuda:0")
    model = CifarConvNet(seed=1).to(dev)
    ex = make_executor(model, FlatParams(model, grads=True, shadow_bf16=True), max_batch=32)
    la, lt = _loader(dev, AUG), _loader(dev)
    assert la.steps_per_epoch == 6
    for k in range(8):  # crosses the epoch boundary
        ex.forward_backward(lt, None)
        torch.cuda.synchronize()
        plain = tu._h(ex.x8[:32, 2:34, 2:34])
        lab_t = lt.labels_out.clone()
        ex.forward_backward(la, None)
        torch.cuda.synchronize()
        assert int(la.ctr[0]) == k + 1 and int(la.ctr[1]) == 0 and la.aug.tolist() == [11, 0]
        prm = [augment_params(11, k * 32 + b, 4, True) for b in range(32)]
        tu.assert_bits(tu._h(ex.x8[:32, 2:34, 2:34]), ar.augment_batch(plain, prm, 4), f"x8 after step {k}")
        assert torch.equal(la.labels_out, lab_t)
        la.step_done()
        lt.step_done()
    assert la.epoch == 1


def test_trainer_graphs_replay_the_augmented_stream(C, deterministic):
    """trainer.run over unrolled graphs (the update launches carry next_prep
    with the augmentation) = 8 eager steps, to the tolerance of
    test_device_loader_graph_matches_eager; the run without augmentation differs."""
    dev = torch.device("cuda:0")
    res = {}
    for name, graph, aug in (("eager", False, AUG), ("plain", False, None)):
        tr = tu_trainer(dev, graph)
        ld = _loader(dev, aug)
        losses = [float(tr.step(ld)) for _ in range(8)]
        torch.cuda.synchronize()
        res[name] = (tr.flat.data.clone(), losses)
    tr = tu_trainer(dev, True)
    ld = _loader(dev, AUG)
    last = float(tr.run(ld, 8, unroll=3))
    torch.cuda.synchronize()
    assert (int(ld.ctr[0]), ld.epoch, tr.steps) == (8, 1, 8)
    assert tr.executor.prepared_ahead > 0  # update launches carried the gather
    p0, l0 = res["eager"]
    assert abs(last - l0[-1]) < 1e-3
    assert float((tr.flat.data - p0).abs().max()) < 1e-3
    assert float((res["plain"][0] - p0).abs().max()) > 1e-2
    assert max(abs(a - b) for a, b in zip(l0, res["plain"][1])) > 1e-2


def tu_trainer(dev, graph):
    from tests.kernels.test_engine_gpu import _trainer

    return _trainer(dev, "hip", graph, 29741)


def test_cifar10_example_with_augmentation(C):
    r = subprocess.run([sys.executable, "examples/cifar10.py", "--cuda", "--augment", "crop4flip", "--trainSize", "512",
                        "--testSize", "256", "--epochs", "1"], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "augment: crop4flip" in r.stdout
    loss = [float(m) for m in re.findall(r"loss[ =:]+([-+0-9.eE]+|nan|inf)", r.stdout)]
    assert loss and all(np.isfinite(v) for v in loss), r.stdout[-2000:]
