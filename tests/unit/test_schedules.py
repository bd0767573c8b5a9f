"""Learning-rate schedules (torch_distlearn_amd/schedules.py) against their
closed forms, the fp32-once rule, the launcher flags, the trainer's eager
bookkeeping on the CPU and the checkpoint round trip of ``sched_step``."""
import argparse
import math
import struct

import pytest
import torch

from torch_distlearn_amd import constant, cosine, schedules, step_decay
from torch_distlearn_amd.schedules import as_fp32


def _is_fp32(v):
    return struct.unpack("f", struct.pack("f", v))[0] == v


def test_constant_and_warmup_end():
    s = constant(0.1)
    assert [s(t) for t in (0, 1, 1000)] == [as_fp32(0.1)] * 3
    w = constant(0.1, warmup_steps=5)  # update t runs at lr * (t + 1) / 5
    assert [w(t) for t in range(5)] == [as_fp32(0.1 * (t + 1) / 5) for t in range(5)]
    assert w(4) == w(5) == as_fp32(0.1)  # the last warm-up update is the first at the full rate
    f = constant(0.1, warmup_steps=4, warmup_from=0.02)
    assert f(0) == as_fp32(0.02 + 0.08 / 4) and f(3) == as_fp32(0.1)


def test_step_decay_at_each_milestone():
    s = step_decay(0.1, [30, 10, 20], gamma=0.5)  # any order
    for t, k in ((0, 0), (9, 0), (10, 1), (19, 1), (20, 2), (29, 2), (30, 3), (99, 3)):
        assert s(t) == as_fp32(0.1 * 0.5 ** k), t
    w = step_decay(0.1, [2], gamma=0.1, warmup_steps=4)  # a milestone inside the warm-up scales its target
    assert w(1) == as_fp32(0.1 * 2 / 4) and w(2) == as_fp32(0.01 * 3 / 4) and w(4) == as_fp32(0.1 * 0.1)


def test_cosine_ends():
    s = cosine(0.2, 100, floor=0.01)
    assert s(0) == as_fp32(0.2)
    assert s(50) == as_fp32(0.01 + 0.5 * 0.19 * (1.0 + math.cos(math.pi * 0.5)))
    assert s(99) == as_fp32(0.01 + 0.5 * 0.19 * (1.0 + math.cos(math.pi * 99 / 100)))  # the last step
    assert s(100) == s(12345) == as_fp32(0.01)
    assert all(s(t) > s(t + 1) for t in range(100))
    w = cosine(0.2, 100, warmup_steps=10)
    assert w(9) == as_fp32(0.1 * (1.0 + math.cos(math.pi * 9 / 100)))
    with pytest.raises(ValueError):
        cosine(0.1, 0)


def test_values_are_fp32_once():
    for s in (constant(0.1), step_decay(0.3, [3], 0.7, warmup_steps=2), cosine(0.123, 17, 0.001, warmup_steps=3)):
        for t in range(20):
            v = s(t)
            assert isinstance(v, float) and _is_fp32(v) and as_fp32(v) == v
    assert not _is_fp32(0.1) and as_fp32(0.1) == float(torch.tensor(0.1, dtype=torch.float32))
    with pytest.raises(ValueError):
        constant(0.1)(-1)


def test_launcher_flags():
    from torch_distlearn_amd.launch import add_schedule_flags

    ap = add_schedule_flags(argparse.ArgumentParser())
    assert schedules.from_options(ap.parse_args([]), 0.1) is None  # defaults: today's constant rate
    s = schedules.from_options(ap.parse_args(["--lrSchedule", "step", "--lrMilestones", "8,16", "--warmupSteps", "4"]),
                               0.1)
    want = step_decay(0.1, [8, 16], 0.1, warmup_steps=4)
    assert [s(t) for t in range(20)] == [want(t) for t in range(20)] and s(19) == as_fp32(0.1 * 0.1 ** 2)
    c = schedules.from_options(ap.parse_args(["--lrSchedule", "cosine", "--totalSteps", "50"]), 0.1)
    assert c(25) == cosine(0.1, 50)(25)
    with pytest.raises(ValueError):
        schedules.from_options(ap.parse_args(["--lrSchedule", "cosine"]), 0.1)
    w = schedules.from_options(ap.parse_args(["--warmupSteps", "2"]), 0.1)
    assert [w(0), w(1), w(2)] == [as_fp32(0.05), as_fp32(0.1), as_fp32(0.1)]


def _trainer(**kw):
    from torch_distlearn_amd import Tree
    from torch_distlearn_amd.engine import DataParallelTrainer
    from torch_distlearn_amd.models import MnistConvNet

    tree = Tree(1, 1, host="127.0.0.1", port=0)
    return DataParallelTrainer(MnistConvNet(seed=0), tree, lr=0.05, compute_dtype=torch.float32, **kw)


def _batch(g):
    return torch.randn(4, 1024, generator=g), torch.randint(0, 10, (4,), generator=g)


def test_eager_cpu_trainer_follows_the_schedule():
    """Eager steps (torch backend, CPU): lr is set from the schedule before
    every step body -- bitwise a trainer without a schedule whose lr the
    caller assigns; set_lr switches to a constant."""
    sched = step_decay(0.05, [2, 4], 0.5, warmup_steps=2)
    a, b = _trainer(lr_schedule=sched), _trainer()
    ga, gb = torch.Generator().manual_seed(1), torch.Generator().manual_seed(1)
    for t in range(6):
        a.step(*_batch(ga))
        assert a.lr == sched(t) and a.sched_step == t + 1
        b.lr = sched(t)
        b.step(*_batch(gb))
    assert torch.equal(a.flat.data, b.flat.data)
    a.set_lr(0.01)
    a.step(*_batch(ga))
    assert a.lr == as_fp32(0.01) and a.sched_step == 7
    b.set_lr(0.01)  # no graphs: plain assignment
    b.step(*_batch(gb))
    assert b.lr == 0.01 and b.sched_step == 0
    torch.testing.assert_close(a.flat.data, b.flat.data, rtol=1e-6, atol=1e-7)


def test_checkpoint_round_trip_of_sched_step(tmp_path):
    from torch_distlearn_amd.checkpoint import load_checkpoint, restore_trainer_state, save_checkpoint, trainer_state

    sched = cosine(0.05, 40, warmup_steps=3)
    a = _trainer(lr_schedule=sched)
    g = torch.Generator().manual_seed(2)
    for _ in range(5):
        a.step(*_batch(g))
    st = trainer_state(a)
    assert st["sched_step"] == 5
    save_checkpoint(str(tmp_path), a.model, st)
    b = _trainer(lr_schedule=sched)
    loaded = load_checkpoint(str(tmp_path), b.model)
    restore_trainer_state(b, loaded)
    assert b.sched_step == 5 and b.lr == a.lr
    x, y = _batch(g)
    a.step(x, y)
    b.step(x, y)
    assert b.lr == sched(5) and torch.equal(a.flat.data, b.flat.data)
    # a state written before schedules existed: the schedule starts over
    old = {k: v for k, v in loaded.items() if k != "sched_step"}
    c = _trainer(lr_schedule=sched)
    c.sched_step = 9
    restore_trainer_state(c, old)
    assert c.sched_step == 0
