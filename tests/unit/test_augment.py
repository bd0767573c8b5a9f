"""Random crop / flip in the device data path, host side (no GPU needed): the
counter-based parameter hash against the issue's check vectors, its coverage,
``DeviceLoader.getBatch`` with augmentation against an independent numpy
shift / flip / zero-fill of an un-augmented twin loader's batches
(tests/kernels/augment_ref.py), stream properties (epochs, partitions, resume)
and the native ``Augment`` value's argument checks."""
import pytest
import torch

from tests.kernels import augment_ref as ar
from torch_distlearn_amd.data import (Augment, DeviceEvalLoader, DeviceLoader, PartitionedDataset, augment_from_name,
                                      augment_params, synthetic_images)

P = 0x10000  # an aligned stand-in for a device pointer: the builders never dereference


@pytest.fixture(scope="module")
def C():
    from torch_distlearn_amd import _native

    return _native.native()


def _ds(n=200, hw=8, partition=1, partitions=1):
    imgs, labels = synthetic_images(n, hw, 3, 10, seed=3)
    return PartitionedDataset(imgs, labels, partition=partition, partitions=partitions)


def _pair(kind="permutation", batch=32, aug=Augment(pad=2, flip=True, seed=0), **kw):
    """(augmented loader, un-augmented twin) over equal datasets."""
    return (DeviceLoader(_ds(**kw), kind, batch, seed=5, augment=aug), DeviceLoader(_ds(**kw), kind, batch, seed=5))


# --------------------------------------------------------------------------- the hash
VECTORS = [(0, 0, 4, (1, 6, 0)), (0, 1, 4, (0, 4, 0)), (12345, 777, 4, (1, 6, 1)), (12345, 777, 2, (1, 3, 2)),
           (2 ** 63 + 5, 2 ** 40 + 3, 4, (0, 5, 2))]


@pytest.mark.parametrize("seed,idx,pad,want", VECTORS)
def test_check_vectors(seed, idx, pad, want):
    assert augment_params(seed, idx, pad, True) == want
    assert augment_params(seed, idx, pad, False) == (0,) + want[1:]


def test_coverage():
    assert {augment_params(0, i, 2, True) for i in range(600)} == ar.triples(2)
    got = [augment_params(0, i, 4, True) for i in range(4096)]
    assert set(got) == ar.triples(4) and len(ar.triples(4)) == 162
    assert 0.45 <= sum(t[0] for t in got) / 4096 <= 0.55
    assert {augment_params(0, i, 2, False) for i in range(600)} == ar.triples(2, flip=False)


# --------------------------------------------------------------------------- getBatch
@pytest.mark.parametrize("aug", [Augment(pad=2, flip=True, seed=0), Augment(pad=0, flip=True, seed=9),
                                 Augment(pad=3, flip=False, seed=2 ** 63 + 5)], ids=["crop2flip", "flip", "crop3"])
def test_get_batch_matches_numpy(aug):
    a, t = _pair(aug=aug)
    seen = set()
    for step in range(8):  # 6 steps per epoch: crosses the boundary
        (xa, ya), (xt, yt) = a.getBatch(), t.getBatch()
        a.step_done()
        t.step_done()
        prm = [augment_params(aug.seed, step * 32 + b, aug.pad, aug.flip) for b in range(32)]
        seen |= set(prm)
        want = torch.from_numpy(ar.augment_batch(xt.numpy(), prm, aug.pad))
        assert torch.equal(xa, want), step
        assert torch.equal(ya, yt) and torch.equal(a.labels_out, t.labels_out)
    assert len(seen) > 1
    assert a.drawn == t.drawn == 8


def test_epochs_differ():
    """The linear sampler repeats the sample order every epoch; the draw index
    does not repeat, so a sample's parameters change."""
    a, t = _pair(kind="linear", batch=40)  # 5 steps per epoch
    e0 = [a.getBatch()[0].clone() for _ in range(5)]
    e1 = [a.getBatch()[0].clone() for _ in range(5)]
    t0 = [t.getBatch()[0].clone() for _ in range(5)]
    t1 = [t.getBatch()[0].clone() for _ in range(5)]
    assert all(torch.equal(u, v) for u, v in zip(t0, t1))  # same samples ...
    assert not any(torch.equal(u, v) for u, v in zip(e0, e1))  # ... other crops
    p0 = [augment_params(0, i, 2, True) for i in range(200)]
    p1 = [augment_params(0, 200 + i, 2, True) for i in range(200)]
    assert sum(u != v for u, v in zip(p0, p1)) > 150


def test_partitions_differ():
    aug = Augment(pad=2, flip=True)  # seed derived from the loader seed and the partition
    a = DeviceLoader(_ds(partition=1, partitions=2), "linear", 20, seed=5, augment=aug)
    b = DeviceLoader(_ds(partition=2, partitions=2), "linear", 20, seed=5, augment=aug)
    c = DeviceLoader(_ds(partition=1, partitions=2), "linear", 20, seed=6, augment=aug)
    assert len({a.aug_seed, b.aug_seed, c.aug_seed}) == 3
    pa = [augment_params(a.aug_seed, i, 2, True) for i in range(100)]
    pb = [augment_params(b.aug_seed, i, 2, True) for i in range(100)]
    assert sum(u != v for u, v in zip(pa, pb)) > 75
    again = DeviceLoader(_ds(partition=1, partitions=2), "linear", 20, seed=5, augment=aug)
    assert again.aug_seed == a.aug_seed and torch.equal(again.getBatch()[0], a.getBatch()[0])


def test_augment_none_is_todays_loader():
    a = DeviceLoader(_ds(), "permutation", 32, seed=5, augment=None)
    t = DeviceLoader(_ds(), "permutation", 32, seed=5)
    assert a.augment_args() is None and t.augment_args() is None and a.aug is None
    assert len(a.gather_args()) == 9
    for _ in range(8):
        (xa, ya), (xt, yt) = a.getBatch(), t.getBatch()
        assert torch.equal(xa, xt) and torch.equal(ya, yt)
    assert torch.equal(a.ctr, t.ctr)
    assert not hasattr(DeviceEvalLoader(_ds(), 32), "augment_args")


@pytest.mark.parametrize("k", [4, 9], ids=["inside_epoch", "past_boundary"])
def test_resume_continues_the_stream(k):
    """6 steps per epoch.  The eager loop reports each step (step_done) as the
    trainers do; the resumed loader starts from skip(k)."""
    a, _ = _pair()
    for _ in range(k):
        a.getBatch()
        a.step_done()
    b, _ = _pair()
    b.skip(k)
    assert b.drawn == a.drawn == k
    assert int(b.ctr[1]) == 0 and int(b.aug[1]) + int(b.ctr[0]) == k
    for step in range(12):
        (xa, ya), (xb, yb) = a.getBatch(), b.getBatch()
        a.step_done()
        b.step_done()
        assert torch.equal(xa, xb) and torch.equal(ya, yb), step


def test_names():
    assert augment_from_name("none") is None
    assert augment_from_name("flip") == Augment(pad=0, flip=True)
    assert augment_from_name("crop4") == Augment(pad=4, flip=False)
    assert augment_from_name("crop4flip") == Augment(pad=4, flip=True)
    with pytest.raises(ValueError):
        augment_from_name("cutout")
    with pytest.raises(ValueError):
        Augment(pad=9)
    with pytest.raises(ValueError, match="smaller than the image"):
        DeviceLoader(_ds(), "linear", 32, augment=Augment(pad=8))


def test_launch_flag_rejects_the_host_batcher():
    import argparse

    from torch_distlearn_amd.launch import add_augment_flag, augment_of

    ap = add_augment_flag(argparse.ArgumentParser())
    assert augment_of(ap.parse_args([]), False) is None
    assert augment_of(ap.parse_args(["--augment", "crop4flip"]), True) == Augment(pad=4, flip=True)
    with pytest.raises(SystemExit, match="device data path"):
        augment_of(ap.parse_args(["--augment", "flip"]), False)


# --------------------------------------------------------------------------- the native value (host code only)
def _next_prep(C, *extra, H=32):
    return C.next_prep(P, P, P, P, P, 1024, 128, 3, [0.5] * 3, [0.25] * 3, P, 4, H, H, 2, [P], [64], P, -5, 64,
                       64 * 25 * 3, *extra)


def test_native_value_builds(C):
    assert type(C.augment(P, 4, 1, 50000)).__name__ == "Augment"
    assert type(C.augment(P, 0, 0, 1)).__name__ == "Augment"
    assert type(C.augment(P, 8, 1, 1)).__name__ == "Augment"


@pytest.mark.parametrize("args,match", [((0, 4, 1, 10), "null"), ((P, -1, 1, 10), "pad"), ((P, 9, 1, 10), "pad"),
                                        ((P, 4, 2, 10), "flip"), ((P, 4, -1, 10), "flip"), ((P, 4, 1, 0), "sample"),
                                        ((P, 4, 1, -3), "sample")])
def test_native_value_rejections(C, args, match):
    with pytest.raises(RuntimeError, match=match):
        C.augment(*args)


def test_next_prep_accepts_the_value(C):
    aug = C.augment(P, 4, 1, 50000)
    assert type(_next_prep(C, aug)).__name__ == "NextPrep"
    assert type(_next_prep(C, None)).__name__ == "NextPrep"
    assert type(_next_prep(C)).__name__ == "NextPrep"  # the old positional form
    with pytest.raises(RuntimeError, match="smaller than the image"):
        _next_prep(C, C.augment(P, 8, 1, 50000), H=8)
    with pytest.raises(TypeError):
        _next_prep(C, 5)


def test_loader_builds_the_native_value(C):
    a, _ = _pair()
    assert type(a.augment_args()).__name__ == "Augment"
    assert a.aug.dtype == torch.int64 and a.aug.tolist() == [0, 0]
    big = DeviceLoader(_ds(), "linear", 32, augment=Augment(pad=1, seed=2 ** 63 + 5))
    assert int(big.aug[0]) == 2 ** 63 + 5 - 2 ** 64  # the same 64 bits, as the signed element type


def test_prep_step_gather_rejects_before_launching(C):
    """Old positional form and the augmented form run their checks on the
    host: a zero batch is refused before anything touches the (fake) pointers."""
    args = (P, P, P, P, P, 1024, 0, 3, [0.5] * 3, [0.25] * 3, P, 4, 32, 32, 2, 0, P, 0, 0, 3, 8, [], [], [], [], [],
            [], 0)
    with pytest.raises(RuntimeError, match="empty order / batch"):
        C.prep_step_gather(*args)
    with pytest.raises(RuntimeError, match="empty order / batch"):
        C.prep_step_gather(*args, C.augment(P, 4, 1, 10))
    with pytest.raises(RuntimeError, match="empty order / batch"):
        C.prep_step_gather(*args, None)
