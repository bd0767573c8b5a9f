"""Learning-rate schedules inside replayed step graphs (engine lr_schedule=):
the captured update kernels read the rate from the trainer's device ring, step
i of a graph from ring[i], filled before every replay.

Setup: CIFAR convnet, HIP backend, batch 16, a 200-image synthetic set (12
steps per epoch), momentum 0 and weight decay 0 unless stated; deterministic
reduction mode wherever bits are compared."""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
V = 0.05


@pytest.fixture(autouse=True)
def deterministic(monkeypatch):
    monkeypatch.setenv("DISTLEARN_REDUCE_ATOMIC", "0")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from torch_distlearn_amd import _native

    _native.native()
    return torch.device("cuda:0")


def _trainer(dev, port, graph=True, lr=V, **kw):
    from torch_distlearn_amd import Tree
    from torch_distlearn_amd.engine import DataParallelTrainer
    from torch_distlearn_amd.models import CifarConvNet

    tree = Tree(1, 1, host="127.0.0.1", port=port, device=dev)
    model = CifarConvNet(seed=7).to(dev)
    tr = DataParallelTrainer(model, tree, lr=lr, backend="hip", compute_dtype=torch.bfloat16, graph=graph,
                             max_batch=16, **kw)
    tr.synchronize_parameters()
    return tr


def _loader(dev, skip=0):
    from torch_distlearn_amd.data import DeviceLoader, PartitionedDataset, synthetic_cifar10

    imgs, labels = synthetic_cifar10(200, seed=5)
    ld = DeviceLoader(PartitionedDataset(imgs, labels, device=dev), "permutation", 16, seed=3)
    if skip:
        ld.skip(skip)
    return ld


def _one_hot(j):
    return lambda t: V if t == j else 0.0


def _oracle(dev, port, j, **kw):
    """The parent's path: no schedule, constant lr = V, graph=True, exactly
    one step on batch j (the loader's resume skip)."""
    tr = _trainer(dev, port, **kw)
    tr.step(_loader(dev, skip=j))
    torch.cuda.synchronize()
    return tr.flat.data.clone()


def test_all_zero_schedule_changes_nothing(dev):
    """fma(-0, g, p) == p: six steps at rate 0 through the 4-, 2-step graphs
    leave the parameters bitwise unchanged (a graph that ignores the ring
    trains at the constructor's rate and fails this)."""
    tr = _trainer(dev, 29731, lr_schedule=lambda t: 0.0)
    ld = _loader(dev)
    p0 = tr.flat.data.clone()
    tr.run(ld, 6, unroll=4)
    torch.cuda.synchronize()
    assert tr.sched_step == 6 and tr.steps == 6 and int(ld.ctr[0]) == 6
    assert torch.equal(tr.flat.data, p0)


@pytest.mark.parametrize("j", [0, 3, 4, 5])
def test_one_hot_step_lands_on_its_slot(dev, j):
    """Rate V at step j only -- the first and last slot of the 4-step graph
    and both slots of the 2-step graph: bitwise one step of the parent's path
    on batch j."""
    tr = _trainer(dev, 29732, lr_schedule=_one_hot(j))
    tr.run(_loader(dev), 6, unroll=4)
    torch.cuda.synchronize()
    assert tr.sched_step == 6
    assert torch.equal(tr.flat.data, _oracle(dev, 29732, j))


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_one_hot_step_forced_rccl_world1(dev, monkeypatch, wire):
    """Collectives forced through RCCL at world 1: no slab deferral, no side
    jobs, the full update launch reads the ring -- from the fp32 gradient, or
    (bf16 wire) the update that reads the all-reduced bf16 copy."""
    monkeypatch.setenv("DISTLEARN_RCCL_WORLD1", "1")
    tr = _trainer(dev, 29733, lr_schedule=_one_hot(3), grad_comm_dtype=wire)
    assert tr._slabs is None and tr._side is None and tr.grad_comm_dtype == wire
    tr.run(_loader(dev), 6, unroll=4)
    torch.cuda.synchronize()
    assert torch.equal(tr.flat.data, _oracle(dev, 29733, 3, grad_comm_dtype=wire))


def test_ea_tau_graph_reads_its_slots(dev):
    """AllReduceEA, tau = 3: the tau-step graph (three local steps, slots 0-2,
    then the elastic round) and the local-step graphs under trainer.run are
    bitwise one captured step at a time (each reading slot 0), and track an
    eager trainer whose lr the test sets, within 1e-3."""
    from torch_distlearn_amd.schedules import as_fp32

    outs = []
    for mode in ("run", "step", "eager"):
        tr = _trainer(dev, 29738, graph=mode != "eager", algo="ea", tau=3, alpha=0.3,
                      lr_schedule=None if mode == "eager" else _warmup_halving)
        ld = _loader(dev)
        if mode == "run":
            tr.run(ld, 8, unroll=2)
            assert ("ea", 3) in tr._multi
        else:
            for t in range(8):
                if mode == "eager":
                    tr.lr = as_fp32(_warmup_halving(t))
                tr.step(ld)
        torch.cuda.synchronize()
        assert mode == "eager" or (tr.sched_step == 8 and tr.lr == as_fp32(_warmup_halving(7)))
        outs.append((tr.flat.data.clone(), tr.ea.center.clone()))
    (p0, c0), (p1, c1), (p2, c2) = outs
    assert torch.equal(p0, p1) and torch.equal(c0, c1)
    assert float((p0 - p2).abs().max()) < 1e-3 and float((c0 - c2).abs().max()) < 1e-3


def _warmup_halving(t):
    """Warm-up over 3 steps to 0.05, then halved every 2 steps."""
    return V * (t + 1) / 3 if t < 3 else V * 0.5 ** ((t - 3) // 2)


def test_general_schedule_graph_tracks_eager(dev):
    """Momentum 0.9, 11 steps from batch 5 (the epoch ends after batch 11): the
    graph run against an eager trainer WITHOUT a schedule whose lr the test
    sets from the same schedule before every step, within 1e-3 (the bound of
    test_engine_gpu.py's graph-versus-eager tests)."""
    from torch_distlearn_amd.schedules import as_fp32

    tg = _trainer(dev, 29734, momentum=0.9, lr_schedule=_warmup_halving)
    ld = _loader(dev, skip=5)
    p0 = tg.flat.data.clone()
    tg.run(ld, 11, unroll=4)
    torch.cuda.synchronize()
    assert ld.epoch == 1  # crossed the epoch boundary
    assert float((tg.flat.data - p0).abs().max()) > 1e-2  # it trained
    assert tg.sched_step == 11 and tg.lr == as_fp32(_warmup_halving(10))
    te = _trainer(dev, 29734, graph=False, momentum=0.9)
    le = _loader(dev, skip=5)
    for t in range(11):
        te.lr = as_fp32(_warmup_halving(t))
        te.step(le)
    torch.cuda.synchronize()
    diff = float((tg.flat.data - te.flat.data).abs().max())
    print(f"graph vs eager after 11 scheduled steps: max |dp| = {diff:.3e}")
    assert diff < 1e-3
    # the eager path of the same schedule object: same bound, same bookkeeping
    ts = _trainer(dev, 29734, graph=False, momentum=0.9, lr_schedule=_warmup_halving)
    ls = _loader(dev, skip=5)
    for _ in range(11):
        ts.step(ls)
    torch.cuda.synchronize()
    assert ts.sched_step == 11 and ts.lr == tg.lr
    assert torch.equal(ts.flat.data, te.flat.data)


def test_prepare_and_comm_profile_leave_the_schedule_alone(dev, monkeypatch):
    """prepare()'s trial replays and comm_profile(replay=True) read valid
    rates from the ring, leave sched_step where it was, and the training
    afterwards is bitwise the run that never called them."""
    monkeypatch.setenv("DISTLEARN_RCCL_WORLD1", "1")  # comm_profile needs collectives that run
    outs = []
    for extra in (False, True):
        tr = _trainer(dev, 29735, momentum=0.9, lr_schedule=_warmup_halving)
        ld = _loader(dev)
        if extra:
            p0 = tr.flat.data.clone()
            tr.prepare(ld, 4)
            torch.cuda.synchronize()
            assert tr.sched_step == 0 and torch.equal(tr.flat.data, p0)
        tr.run(ld, 3, unroll=4)
        if extra:
            rp = tr.comm_profile(ld, steps=2, replay=True)
            assert rp["source"].startswith("graph replays"), rp.get("replay_error")
            assert tr.sched_step == 3
        tr.run(ld, 5, unroll=4)
        torch.cuda.synchronize()
        outs.append((tr.flat.data.clone(), tr.sched_step, tr.lr, int(ld.ctr[0])))
    assert outs[0][1:] == outs[1][1:] and outs[0][1] == 8
    assert torch.equal(outs[0][0], outs[1][0])


def test_set_lr(dev):
    """Without a schedule the captured graphs hold their rate: set_lr raises
    once they exist (and names lr_schedule=).  With one it switches to a
    constant from the next step on."""
    from torch_distlearn_amd.schedules import as_fp32

    tr = _trainer(dev, 29736)
    tr.set_lr(0.01)
    assert tr.lr == 0.01
    ld = _loader(dev)
    tr.step(ld)
    with pytest.raises(RuntimeError, match="lr_schedule="):
        tr.set_lr(0.02)
    torch.cuda.synchronize()
    ts = _trainer(dev, 29736, lr_schedule=lambda t: 0.0)
    ls = _loader(dev)
    ts.run(ls, 2, unroll=2)
    ts.set_lr(V)  # steps 2.. at V: one step on batch 2 from untouched parameters
    ts.step(ls)
    torch.cuda.synchronize()
    assert ts.sched_step == 3 and ts.lr == as_fp32(V)
    assert torch.equal(ts.flat.data, _oracle(dev, 29736, 2))


def test_graph_longer_than_the_ring_is_refused(dev):
    from torch_distlearn_amd.engine import LR_RING

    tr = _trainer(dev, 29737, algo="ea", tau=LR_RING + 1, lr_schedule=lambda t: V)
    with pytest.raises(ValueError, match="ring"):
        tr.prepare(_loader(dev), 2)
    torch.cuda.synchronize()


def test_cifar10_example_step_schedule(dev):
    """The example's flags: 20 steps, warm-up over 4, x0.1 at 8 and 16 -> the
    last step ran at 0.1 * 0.1^2 (rounded to fp32 once)."""
    from torch_distlearn_amd.schedules import as_fp32, step_decay

    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "examples/cifar10.py", "--cuda", "--epochs", "1", "--maxSteps", "20",
                        "--lrSchedule", "step", "--lrMilestones", "8,16", "--warmupSteps", "4", "--batchSize", "32",
                        "--trainSize", "1024", "--testSize", "64"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rates = [float(m) for m in re.findall(r"Epoch 1: learning rate ([0-9.e+-]+)", r.stdout)]
    want = step_decay(0.1, [8, 16], 0.1, warmup_steps=4)(19)
    assert want == as_fp32(0.1 * 0.1 ** 2)
    assert rates == [float(f"{want:.8g}")], r.stdout[-2000:]
