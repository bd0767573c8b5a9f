"""Device-resident evaluation on one MI355X: the evaluation head kernel and
DataParallelTrainer.evaluate (eager and replayed forward-only hipGraphs)
against the predict path -- bitwise log-probabilities, exact tail handling,
the counter advance, the tie rule, the other convolution plans, untouched
training state, and the example's --testPath device."""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.fixture(scope="module", autouse=True)
def deterministic():
    """The deterministic reduction mode (as tests/kernels/test_engine_gpu.py):
    the training runs compared here are bitwise reproducible."""
    old = os.environ.get("DISTLEARN_REDUCE_ATOMIC")
    os.environ["DISTLEARN_REDUCE_ATOMIC"] = "0"
    yield
    if old is None:
        os.environ.pop("DISTLEARN_REDUCE_ATOMIC", None)
    else:
        os.environ["DISTLEARN_REDUCE_ATOMIC"] = old


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from torch_distlearn_amd import _native

    _native.native()
    return torch.device("cuda:0")


def _trainer(dev, graph, max_batch=32, port=29741, **kw):
    from torch_distlearn_amd import Tree
    from torch_distlearn_amd.engine import DataParallelTrainer
    from torch_distlearn_amd.models import CifarConvNet

    tree = Tree(1, 1, host="127.0.0.1", port=port, device=dev)
    model = CifarConvNet(seed=7).to(dev)
    tr = DataParallelTrainer(model, tree, lr=0.02, backend="hip", compute_dtype=torch.bfloat16, graph=graph,
                             max_batch=max_batch, **kw)
    tr.synchronize_parameters()
    return tr


def _train_loader(dev, batch=32):
    from torch_distlearn_amd.data import DeviceLoader, PartitionedDataset, synthetic_cifar10

    imgs, labels = synthetic_cifar10(200, seed=5)
    return DeviceLoader(PartitionedDataset(imgs, labels, device=dev), "permutation", batch, seed=3)


def _eval_loader(dev, n, batch):
    from torch_distlearn_amd.data import DeviceEvalLoader, PartitionedDataset, synthetic_cifar10

    imgs, labels = synthetic_cifar10(n, seed=9)
    return DeviceEvalLoader(PartitionedDataset(imgs, labels, device=dev), batch)


@pytest.fixture(scope="module")
def trained(dev):
    """Parameters and running statistics after a few eager training steps
    (the statistics are no longer at their initial values), computed once."""
    tr = _trainer(dev, False)
    ld = _train_loader(dev)
    for _ in range(3):
        tr.step(ld)
    torch.cuda.synchronize()
    return tr.flat.data.clone(), [b.detach().clone() for b in tr.model.buffers()]


def _load(tr, trained):
    data, bufs = trained
    tr.flat.data.copy_(data)
    tr.flat.refresh_shadow()
    for b, v in zip(tr.model.buffers(), bufs):
        b.detach().copy_(v)
    return tr


def _argmax_first(logp):
    """Larger value wins, a tie goes to the smaller class."""
    nc = logp.shape[1]
    cls = torch.arange(nc, device=logp.device).expand_as(logp)
    return torch.where(logp == logp.max(1, keepdim=True).values, cls, nc).min(1).values.to(torch.int32)


def _predict_path(tr, n, batch):
    """The evaluation the example's loop performs, tail honoured: predict on
    the very batches the device gather produces (read back from the
    executor's input buffer), ConfusionMatrix.add over the valid rows."""
    from torch_distlearn_amd._native import stream_handle
    from torch_distlearn_amd.utils.metrics import ConfusionMatrix

    dev = tr.device
    aux = _eval_loader(dev, n, batch)
    ex = tr.executor
    conf = ConfusionMatrix(10, device=dev)
    logps, preds, nlls = [], [], []
    for k in range(aux.steps):
        aux.ctr[0:1].fill_(k)
        ex._prep(aux, stream_handle(), train=False)
        x = ex.x8[:batch, 2:2 + aux.H, 2:2 + aux.W, :3].contiguous()
        y = aux.labels_out.clone()
        valid = min(batch, n - k * batch)
        logp = tr.predict(x)[:valid]
        conf.add(logp, y[:valid])
        logps.append(logp)
        preds.append(_argmax_first(logp))
        nlls.append(-logp[torch.arange(valid, device=dev), y[:valid]])
    torch.cuda.synchronize()
    return {"logp": logps, "pred": torch.cat(preds), "nll": torch.cat(nlls), "mat": conf.mat.clone()}


_REFS = {}


def _reference(dev, trained, n, batch):
    """One predict-path reference per shape, shared by the tests and left unchanged."""
    key = (n, batch)
    if key not in _REFS:
        _REFS[key] = _predict_path(_load(_trainer(dev, False, max_batch=batch), trained), n, batch)
    return _REFS[key]


def _same(res, ref, n):
    assert res["count"] == n and int(res["mat"].sum()) == n
    assert torch.equal(res["mat"], ref["mat"])
    assert torch.equal(res["pred"], ref["pred"])
    assert torch.equal(res["nll"], ref["nll"])  # bitwise
    assert torch.equal(res["loss_sum"], ref["nll"].sum())


def test_eval_head_matches_predict_bitwise(dev, trained):
    n, batch = 200, 32
    ref = _reference(dev, trained, n, batch)
    tr = _load(_trainer(dev, False), trained)
    ex = tr.executor
    ld = _eval_loader(dev, n, batch)
    assert (ld.steps, ld.n_order) == (7, 224)
    state = lambda: [t.detach().view(torch.int32).clone() for t in ex.coef + ex.rm + ex.rv + [ex.logits]]  # noqa: E731
    saved = state()  # (as bits: the workspaces start uninitialised)
    ld.reset()
    ex.eval_begin()
    for k in range(ld.steps):
        out = torch.full((batch, 10), float("nan"), device=dev)
        ex.eval_step(ld, logits_out=out)
        valid = min(batch, n - k * batch)
        assert torch.equal(out[:valid], ref["logp"][k])  # bitwise predict's log-probabilities
        assert bool(out[valid:].isnan().all())           # a padded row writes nothing
    torch.cuda.synchronize()
    assert ld.ctr.tolist() == [7, 0]
    assert torch.equal(ld.pred[:n], ref["pred"])
    assert torch.equal(ld.nll[:n], ref["nll"])
    assert torch.equal(ld.mat, ref["mat"]) and int(ld.mat.sum()) == n
    assert bool((ld.pred[n:] == ld.PRED_RESET).all()) and not ld.nll[n:].any()
    for t, v in zip(state(), saved):
        assert torch.equal(t, v)
    # a batch above the executor's capacity raises
    with pytest.raises(ValueError):
        ex.eval_step(_eval_loader(dev, 100, 64))


def test_evaluate_graphs_match_eager_and_predict(dev, trained):
    """unroll=3 over 7 steps replays graphs of 3 + 3 + 1 steps.  A block that saw
    the counter its own launch advanced would land in another step's positions:
    mat.sum() or the pred of the step's own positions would be wrong."""
    n, batch = 200, 32
    ref = _reference(dev, trained, n, batch)
    eager = _load(_trainer(dev, False), trained)
    _same(eager.evaluate(_eval_loader(dev, n, batch), unroll=3), ref, n)
    assert eager.eval_captures == 0

    tr = _load(_trainer(dev, True), trained)
    ld = _eval_loader(dev, n, batch)
    tr.prepare_eval(ld, 3)
    assert sorted(tr._eval_graphs) == [1, 2, 3] and tr.eval_captures == 3 and tr.captures == 0
    replayed = []

    class Counted:
        def __init__(self, k, g):
            self.k, self.g = k, g

        def replay(self):
            replayed.append(self.k)
            self.g.replay()

    tr._eval_graphs = {k: Counted(k, g) for k, g in tr._eval_graphs.items()}
    from torch_distlearn_amd.utils.metrics import ConfusionMatrix

    conf = ConfusionMatrix(10, device=dev)
    r1 = tr.evaluate(ld, conf, unroll=3)
    r2 = tr.evaluate(ld, conf, unroll=3)
    torch.cuda.synchronize()
    assert replayed == [3, 3, 1, 3, 3, 1]
    assert tr.eval_captures == 3 and tr.captures == 0
    assert ld.ctr.tolist() == [7, 0]
    _same(r1, ref, n)
    _same(r2, ref, n)
    assert torch.equal(conf.mat, 2 * ref["mat"])
    assert bool((ld.pred[n:] == ld.PRED_RESET).all()) and not ld.nll[n:].any()


def test_tie_goes_to_the_smaller_class(dev, trained):
    tr = _load(_trainer(dev, False), trained)
    views = tr.flat.param_views()
    w, b = views[-2], views[-1]
    assert tuple(w.shape) == (10, 2048) and tuple(b.shape) == (10,)
    ld = _eval_loader(dev, 40, 32)
    w.zero_()
    b.fill_(0.25)
    res = tr.evaluate(ld)
    assert res["count"] == 40 and not res["pred"].any()
    b[3] = 1.0
    b[7] = 1.0
    res = tr.evaluate(ld)
    assert bool((res["pred"] == 3).all()) and int(res["mat"][:, 3].sum()) == 40


@pytest.mark.parametrize("n,batch", [(300, 128), (10, 4)])
def test_other_conv_plans_match_predict(dev, trained, n, batch):
    """Batch 128: the region / in-launch-combine plans; batch 4: the batch-aware small plans."""
    ref = _reference(dev, trained, n, batch)
    tr = _load(_trainer(dev, False, max_batch=batch), trained)
    ld = _eval_loader(dev, n, batch)
    assert ld.steps == 3 and n - 2 * batch in (44, 2)
    _same(tr.evaluate(ld), ref, n)
    assert ld.ctr.tolist() == [3, 0]


def test_evaluate_leaves_training_state_untouched(dev, trained):
    from torch_distlearn_amd import schedules

    n, batch = 200, 32
    outs = []
    for with_eval in (True, False):
        tr = _trainer(dev, True, momentum=0.9, lr_schedule=schedules.step_decay(0.02, [5, 11], 0.5))
        ld = _train_loader(dev)
        tr.run(ld, 8, unroll=4)
        if with_eval:
            ev = _eval_loader(dev, n, batch)
            caps = tr.captures
            res = tr.evaluate(ev, unroll=4)
            assert int(res["mat"].sum()) == n and tr.captures == caps and tr.eval_captures == 3
        tr.run(ld, 8, unroll=4)
        torch.cuda.synchronize()
        outs.append((tr.flat.data.clone(), tr.mom.clone(), [b.detach().clone() for b in tr.model.buffers()],
                     ld.ctr.clone(), ld.epoch, tr.steps, tr.lr, tr.sched_step, tr.sgd.stepsPerNode.clone(),
                     tr._lr_ring.clone()))
        if with_eval:
            keep = tr, ev
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert torch.equal(a[3], b[3]) and a[4:8] == b[4:8] and a[5] == 16
    assert torch.equal(a[8], b[8]) and torch.equal(a[9], b[9])
    # a policy change reallocates the executor's workspaces: the evaluation graphs go
    # with the training graphs, and the next evaluation captures again and is correct
    tr, ev = keep
    before = tr.evaluate(ev, unroll=4)
    assert tr.eval_captures == 3
    tr._set_policy({"dgrad_stages": tr.executor.dgrad_stages, "cu_reserve": tr.executor.cu_reserve})
    assert tr._eval_graphs == {} and tr._multi == {}
    after = tr.evaluate(ev, unroll=4)
    torch.cuda.synchronize()
    assert tr.eval_captures == 6
    for key in ("mat", "pred", "nll"):
        assert torch.equal(after[key], before[key])
    eager = _trainer(dev, False)
    eager.flat.data.copy_(tr.flat.data)
    eager.flat.refresh_shadow()
    for x, y in zip(eager.model.buffers(), tr.model.buffers()):
        x.detach().copy_(y)
    ref = eager.evaluate(_eval_loader(dev, n, batch))
    for key in ("mat", "pred", "nll"):
        assert torch.equal(after[key], ref[key])


def _example(*args):
    env = dict(os.environ, PYTHONPATH=ROOT, DISTLEARN_REDUCE_ATOMIC="0")
    r = subprocess.run([sys.executable, "examples/cifar10.py", "--cuda", "--epochs", "1", "--batchSize", "32",
                        "--maxSteps", "4", "--trainSize", "1024", "--unroll", "4", *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_example_device_path_prints_the_batcher_accuracy(dev):
    """64 test images = 2 full batches: the old loop's tail does not differ."""
    acc = {}
    for path in ("batcher", "device"):
        out = _example("--testSize", "64", "--testPath", path)
        acc[path] = re.findall(r"test accuracy ([0-9.]+)%", out)
        assert len(acc[path]) == 1, out[-2000:]
        assert ("evaluated 64 test samples" in out) == (path == "device"), out[-2000:]
    assert acc["device"] == acc["batcher"]


def test_example_device_path_counts_each_sample_once(dev):
    """80 test images = 3 batches of 32 with a tail of 16: 80 counted, not 96."""
    out = _example("--testSize", "80", "--testPath", "device")
    assert "evaluated 80 test samples" in out, out[-2000:]
    assert re.search(r"mean NLL [0-9.]+", out), out[-2000:]
