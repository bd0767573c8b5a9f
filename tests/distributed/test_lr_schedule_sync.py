"""Nodes agree on the position in the learning-rate schedule (gloo, world 2,
torch backend): after uneven epochs (5 and 8 steps) the parameter
synchronisation gives every node the winner's parameters AND the winner's
``sched_step``, so the next epoch runs at identical rates on every node.
Without the max agreement rank 0 would stay 3 steps behind for ever."""
import pytest
import torch

from tests import mp

STEPS = (5, 8)


def _schedule(t):
    return 0.05 * 0.9 ** t


def _worker(rank, world, port, algo, epoch_end):
    from torch_distlearn_amd import Tree
    from torch_distlearn_amd.engine import DataParallelTrainer
    from torch_distlearn_amd.models import MnistConvNet

    tree = Tree(rank + 1, world, host="127.0.0.1", port=port)
    tr = DataParallelTrainer(MnistConvNet(seed=0), tree, lr=0.05, algo=algo, tau=2, alpha=0.3,
                             compute_dtype=torch.float32, bucket_bytes=8 << 10, lr_schedule=_schedule)
    tr.synchronize_parameters()
    g = torch.Generator().manual_seed(rank)

    def step():
        tr.step(torch.randn(4, 1024, generator=g), torch.randint(0, 10, (4,), generator=g))
        return tr.lr

    first = [step() for _ in range(STEPS[rank])]
    before = tr.sched_step
    if epoch_end:
        tr.synchronize()
    else:
        tr.synchronize_parameters()
    after = tr.sched_step
    second = [step() for _ in range(3)]
    tr.synchronize()
    return {"before": before, "after": after, "first": first, "second": second, "end": tr.sched_step,
            "p": tr.flat.data.clone()}


@pytest.mark.parametrize("algo,epoch_end", [("sgd", False), ("sgd", True), ("ea", False), ("ea", True)])
def test_sched_step_follows_the_winner(algo, epoch_end):
    from torch_distlearn_amd.schedules import as_fp32

    res = mp.run(_worker, 2, algo, epoch_end)
    assert [r["before"] for r in res] == list(STEPS)
    assert [r["after"] for r in res] == [8, 8]
    for r, n in zip(res, STEPS):
        assert r["first"] == [as_fp32(_schedule(t)) for t in range(n)]
        assert r["second"] == [as_fp32(_schedule(t)) for t in (8, 9, 10)]
        assert r["end"] == 11
    if algo == "sgd":  # replicas stay bitwise identical
        assert (res[0]["p"] == res[1]["p"]).all()


def _bucket_worker(rank, world, port, tensor_rate):
    """AllReduceSGD.step and the per-bucket updates pass a tensor rate straight
    through (CPU: read with float() at every update)."""
    from torch_distlearn_amd import AllReduceSGD, FlatParams, GradBucketer, Tree

    tree = Tree(rank + 1, world, host="127.0.0.1", port=port)
    outs = []
    for early in (False, True):
        torch.manual_seed(3)
        w, b = torch.nn.Parameter(torch.randn(7, 3)), torch.nn.Parameter(torch.randn(5))
        flat = FlatParams([w, b])
        bucketer = GradBucketer(tree.comm, flat, bucket_bytes=64, hooks=False)
        sgd = AllReduceSGD(tree, bucketer=bucketer)
        rate = torch.zeros(1) if tensor_rate else [0.0]
        if early:
            assert sgd.enable_bucket_updates(flat, (lambda: rate) if tensor_rate else (lambda: rate[0]))
        sgd.synchronizeParameters(flat)
        for t in range(4):
            rate[0] = _schedule(t)
            flat.zero_grad()
            w.grad.fill_(0.25 * (rank + 1))
            b.grad.fill_(-0.5)
            for k in range(bucketer.nb):
                bucketer.mark_bucket_ready(k)
            sgd.step(flat, lr=rate if tensor_rate else rate[0])
        outs.append(flat.data.clone())
    return outs


def test_tensor_rate_passes_through_step_and_bucket_updates():
    from torch_distlearn_amd.schedules import as_fp32

    assert as_fp32(_schedule(3)) != _schedule(3)
    ten, flt = mp.run(_bucket_worker, 2, True), mp.run(_bucket_worker, 2, False)
    for r in range(2):
        assert (ten[r][0] == ten[r][1]).all() and (ten[0][0] == ten[r][0]).all()
    # the fp32 tensor carries the rate rounded once; the float path the double: equal to fp32 rounding
    torch.testing.assert_close(torch.from_numpy(ten[0][0]), torch.from_numpy(flt[0][0]), rtol=1e-6, atol=1e-7)
