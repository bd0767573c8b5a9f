"""GPU integration: data pipeline kernels, the DataParallelTrainer on one
MI355X (HIP executor eager vs hipGraph replay vs the PyTorch path), the
examples with --cuda, and bench.py's JSON contract."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.fixture(autouse=True)
def deterministic(monkeypatch):
    """Graph-vs-eager and side-effect checks compare runs bitwise / to 1e-3:
    they use the deterministic reduction mode (partial rows + finalize
    kernels).  The atomic modes (2 = the executor default) are covered by
    test_atomic_modes_train_and_graph_tracks_eager and tests/kernels/test_convnet_gpu.py."""
    monkeypatch.setenv("DISTLEARN_REDUCE_ATOMIC", "0")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from torch_distlearn_amd import _native

    _native.native()
    return torch.device("cuda:0")


def test_gather_normalize_and_confusion(dev):
    from torch_distlearn_amd.data import PartitionedDataset, synthetic_cifar10
    from torch_distlearn_amd.utils.metrics import ConfusionMatrix

    imgs, labels = synthetic_cifar10(256)
    ds_cpu = PartitionedDataset(imgs, labels, 2, 3)
    ds_gpu = PartitionedDataset(imgs, labels, 2, 3, device=dev)
    bc = ds_cpu.sampledBatcher("linear", 16, channels_out=8, dtype=torch.float32)
    bg = ds_gpu.sampledBatcher("linear", 16, channels_out=8, dtype=torch.bfloat16)
    for _ in range(3):
        xc, yc = bc.getBatch()
        xg, yg = bg.getBatch()
        torch.cuda.synchronize()
        torch.testing.assert_close(xg.float().cpu(), xc.to(torch.bfloat16).float(), rtol=0, atol=1e-2)
        assert torch.equal(yg.cpu(), yc)
    pred = torch.randn(300, 10, device=dev)
    tgt = torch.randint(0, 10, (300,), device=dev)
    cg, cc = ConfusionMatrix(10, device=dev), ConfusionMatrix(10)
    cg.add(pred, tgt)
    cg.add(pred.to(torch.bfloat16), tgt)
    cc.add(pred.cpu(), tgt.cpu())
    cc.add(pred.to(torch.bfloat16).float().cpu(), tgt.cpu())
    torch.cuda.synchronize()
    assert torch.equal(cg.mat.cpu(), cc.mat)


def _trainer(dev, backend, graph, port, **kw):
    from torch_distlearn_amd import Tree
    from torch_distlearn_amd.engine import DataParallelTrainer
    from torch_distlearn_amd.models import CifarConvNet

    tree = Tree(1, 1, host="127.0.0.1", port=port, device=dev)
    model = CifarConvNet(seed=7).to(dev)
    tr = DataParallelTrainer(model, tree, lr=0.02, backend=backend, compute_dtype=torch.bfloat16, graph=graph,
                             max_batch=32, **kw)
    tr.synchronize_parameters()
    return tr


def test_hip_graph_replay_matches_eager(dev):
    g = torch.Generator(device=dev).manual_seed(0)
    xs = torch.randn(4, 32, 32, 32, 3, device=dev, generator=g).to(torch.bfloat16)
    ys = torch.randint(0, 10, (4, 32), device=dev, generator=g)
    outs = []
    for graph, port in ((False, 29701), (True, 29701)):
        tr = _trainer(dev, "hip", graph, port)
        losses = [float(tr.step(xs[i], ys[i])) for i in range(4)]
        torch.cuda.synchronize()
        outs.append((tr.flat.data.clone(), losses, tr.sgd.stepsPerNode.clone()))
    (p0, l0, s0), (p1, l1, s1) = outs
    assert torch.equal(s0, s1) and int(s0.sum()) == 4
    assert max(abs(a - b) for a, b in zip(l0, l1)) < 1e-3
    assert float((p0 - p1).abs().max()) < 1e-3


def test_rccl_collectives_inside_hipgraph(dev, monkeypatch):
    """World-1 collectives are normally skipped (identity); forcing them
    through RCCL puts ncclAllReduce (3 bucket all-reduces per step, on the
    comm stream) inside the captured hipGraph: replay must match eager."""
    monkeypatch.setenv("DISTLEARN_RCCL_WORLD1", "1")
    g = torch.Generator(device=dev).manual_seed(3)
    xs = torch.randn(3, 32, 32, 32, 3, device=dev, generator=g).to(torch.bfloat16)
    ys = torch.randint(0, 10, (3, 32), device=dev, generator=g)
    outs = []
    for graph, port in ((False, 29703), (True, 29703)):
        tr = _trainer(dev, "hip", graph, port)
        assert not tr.tree.comm._skip1 and len(tr.bucketer.ranges) >= 2
        for i in range(3):
            tr.step(xs[i], ys[i])
        torch.cuda.synchronize()
        outs.append(tr.flat.data.clone())
    assert float((outs[0] - outs[1]).abs().max()) < 1e-3


def test_hip_and_torch_backends_train_alike(dev):
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(32, 32, 32, 3, device=dev, generator=g).to(torch.bfloat16)
    y = torch.randint(0, 10, (32,), device=dev, generator=g)
    res = {}
    for backend in ("hip", "torch"):
        tr = _trainer(dev, backend, False, 29702)
        losses = [float(tr.step(x, y)) for _ in range(6)]
        res[backend] = losses
    assert res["hip"][-1] < res["hip"][0]  # fits the repeated batch
    for a, b in zip(res["hip"], res["torch"]):
        assert abs(a - b) < 0.1 * max(1.0, abs(b))


def _loader(dev, batch=32, seed=3, kind="permutation"):
    from torch_distlearn_amd.data import DeviceLoader, PartitionedDataset, synthetic_cifar10

    imgs, labels = synthetic_cifar10(200, seed=5)
    return DeviceLoader(PartitionedDataset(imgs, labels, device=dev), kind, batch, seed=seed)


def test_device_loader_gather_in_prep(dev):
    """prep_step_gather = the eager gather of the same batch; the device-side
    step counter advances once per step and runs on into the next epoch's half
    of the order ring (uploaded ahead, asynchronously)."""
    from torch_distlearn_amd.models import make_executor, CifarConvNet
    from torch_distlearn_amd.ops.flat import FlatParams

    model = CifarConvNet(seed=1).to(dev)
    flat = FlatParams(model, grads=True, shadow_bf16=True)
    ex = make_executor(model, flat, max_batch=32)
    la, lb = _loader(dev), _loader(dev)  # identical sample streams
    assert la.steps_per_epoch == 6
    seen = []
    for k in range(8):  # crosses the epoch boundary
        xe, ye = lb.getBatch()
        ex.forward_backward(la, None)
        torch.cuda.synchronize()
        assert int(la.ctr[0]) == k + 1 and int(la.ctr[1]) == 0
        inner = ex.x8[:32, 2:34, 2:34]
        torch.testing.assert_close(inner[..., :3].float(), xe.to(torch.bfloat16).float(), rtol=0, atol=2e-2)
        assert not inner[..., 3:].any()
        assert torch.equal(la.labels_out, ye)
        seen.append(ye)
        la.step_done()
        lb.step_done()
    assert la.epoch == 1


def test_device_loader_graph_matches_eager(dev):
    outs = []
    for graph, port in ((False, 29703), (True, 29703)):
        tr = _trainer(dev, "hip", graph, port)
        ld = _loader(dev)
        losses = [float(tr.step(ld)) for _ in range(8)]
        torch.cuda.synchronize()
        outs.append((tr.flat.data.clone(), losses, int(ld.ctr[0]), ld.epoch))
    (p0, l0, c0, e0), (p1, l1, c1, e1) = outs
    assert (c0, e0) == (c1, e1) == (8, 1)
    assert max(abs(a - b) for a, b in zip(l0, l1)) < 1e-3
    assert float((p0 - p1).abs().max()) < 1e-3
    # unrolled multi-step graphs (trainer.run): same 8 steps, same parameters
    tr = _trainer(dev, "hip", True, 29703)
    ld = _loader(dev)
    tr.run(ld, 8, unroll=3)
    torch.cuda.synchronize()
    assert (int(ld.ctr[0]), ld.epoch, tr.steps, int(tr.sgd.stepsPerNode.sum())) == (8, 1, 8, 8)
    assert float((tr.flat.data - p1).abs().max()) < 1e-3


def _run(args, timeout=600, env=None):
    env = dict(os.environ, PYTHONPATH=ROOT, **(env or {}))
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("batch", [32, 128])
def test_cifar10_example_cuda_test_accuracy(dev, batch):
    """examples/cifar10.py --cuda on the HIP fast path (device sampler,
    unrolled hipGraphs, eval-mode predict from the running statistics): one
    epoch of 64 steps on the synthetic CIFAR-shaped data classifies the
    held-out split (>= 95 %; the reference example exists to print this
    matrix, examples/cifar10.lua:213-236).  Round 3's chance-level record was
    measured with the older synthetic test split whose class prototypes
    differed from the training split's (profiles/r4_accuracy_regime.txt)."""
    import re

    out = _run(["examples/cifar10.py", "--cuda", "--epochs", "1", "--batchSize", str(batch),
                "--trainSize", str(64 * batch), "--testSize", "1024"])
    acc = [float(m) for m in re.findall(r"test accuracy ([0-9.]+)%", out)]
    assert acc and acc[-1] >= 95.0, out[-2000:]


def test_cifar10_example_cuda(dev):
    out = _run(["-m", "torch_distlearn_amd.launch", "--nproc", "1", "--gpus", "examples/cifar10.py", "--epochs", "2",
                "--maxSteps", "20", "--batchSize", "64", "--trainSize", "2048", "--testSize", "256",
                "--learningRate", "0.05"])
    assert "test accuracy" in out
    # the reference example runs on bench.py's path: device sampler + unrolled graph
    # replays, every capture made before the first epoch (same count after epoch 2)
    eps = [ln for ln in out.splitlines() if ln.startswith("Epoch") and "img/s" in ln]
    assert len(eps) == 2 and all("unrolled hipGraphs x16" in ln for ln in eps), eps
    assert eps[0].split("x16, ")[1] == eps[1].split("x16, ")[1]


def test_cifar10_example_resume_bitwise_mode0(dev, tmp_path):
    """The CIFAR-10 example on the HIP fast path (unrolled graphs, device
    sampler) in the deterministic reduction mode 0: 2 epochs straight ==
    1 epoch + --save, then a fresh process --resume + epoch 2, BITWISE.
    (Mode 2, the default, accumulates BN statistics with fp32 atomics: not
    run-to-run reproducible, so a resumed run matches only statistically.)"""
    root = str(tmp_path)
    common = ["-m", "torch_distlearn_amd.launch", "--nproc", "1", "--gpus", "examples/cifar10.py", "--maxSteps", "19",
              "--batchSize", "32", "--trainSize", "1024", "--testSize", "64", "--resultsRoot", root]
    env = {"DISTLEARN_REDUCE_ATOMIC": "0"}
    _run(common + ["--epochs", "2", "--save", "straight"], env=env)
    _run(common + ["--epochs", "1", "--save", "split"], env=env)
    out = _run(common + ["--epochs", "2", "--save", "split", "--resume"], env=env)
    assert "resumed from" in out
    a = torch.load(os.path.join(root, "straight", "Net"), weights_only=True)
    b = torch.load(os.path.join(root, "split", "Net"), weights_only=True)
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_cifar10_example_confusion_counts_every_sample(dev):
    """The captured confusion-matrix hook sees every training sample exactly
    once per step (steps x per-node batch entries per epoch)."""
    import re

    out = _run(["-m", "torch_distlearn_amd.launch", "--nproc", "1", "--gpus", "examples/cifar10.py", "--epochs", "1",
                "--maxSteps", "37", "--batchSize", "32", "--trainSize", "4096", "--testSize", "64"])
    rows = [ln for ln in out.split("Epoch 1: train loss")[1].split("Epoch 1: test")[0].splitlines()
            if ln.strip().startswith(("[[", "["))]
    total = sum(sum(int(v) for v in re.findall(r"\d+", ln.split("]")[0])) for ln in rows)
    assert total == 37 * 32, (total, rows)


def test_mnist_examples_cuda(dev):
    out = _run(["-m", "torch_distlearn_amd.launch", "--nproc", "1", "--gpus", "examples/mnist.py", "--epochs", "1",
                "--trainSize", "256", "--batchSize", "8"])
    assert "Epoch 1" in out
    out = _run(["-m", "torch_distlearn_amd.launch", "--nproc", "1", "--gpus", "examples/mnist_ea.py", "--epochs",
                "1", "--trainSize", "256", "--batchSize", "8"])
    assert "Epoch 1" in out


@pytest.mark.parametrize("algo", ["sgd", "ea"])
def test_bench_json_contract(dev, algo):
    out = _run(["bench.py", "--steps", "5", "--warmup", "2", "--algo", algo])
    rec = json.loads(out.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in rec
    assert rec["n_gpus"] == 1 and rec["steps"] == 5 and rec["value"] > 0 and rec["dtype"] == "bf16"


def _bench_dump(out_dir, mode=None, args=("--steps", "1", "--warmup", "0")):
    """One ``bench.py --gpus 1 --dump-outputs`` run with DISTLEARN_REDUCE_ATOMIC
    unset (``mode`` None) or set: (result record, {file: array}, stderr)."""
    import numpy as np

    env = {k: v for k, v in os.environ.items() if k != "DISTLEARN_REDUCE_ATOMIC"}
    env["PYTHONPATH"] = ROOT
    if mode is not None:
        env["DISTLEARN_REDUCE_ATOMIC"] = str(mode)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", *args, "--dump-outputs", str(out_dir)], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    return rec, {f: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}, r.stderr


@pytest.fixture(scope="module")
def bench_dump(dev, tmp_path_factory):
    """The dump of one benchmark step with no reduction mode in the environment
    (shared, read-only)."""
    return _bench_dump(tmp_path_factory.mktemp("dump") / "o")


def test_bench_dump_outputs(dev, bench_dump, tmp_path):
    """--dump-outputs writes what the last timed step left as float32 .npy
    files: its loss (the result line's final_loss), the flat parameter vector
    (4.33M floats, inside the 64 MB budget unsampled) and the batch's
    log-probabilities (rows sum to 1 in probability).  With no reduction mode
    in the environment such a run takes the deterministic one by itself and
    says so: two runs with the same arguments write bitwise identical files."""
    import numpy as np

    rec, got, err = bench_dump
    assert "comm" not in rec  # measurements beyond the headline are behind --full
    assert rec["config"]["reduce_mode"] == 0 and "deterministic reduction mode 0" in err
    rec2, again, _ = _bench_dump(tmp_path / "p")
    assert sorted(got) == sorted(again) == ["logits.npy", "loss.npy", "params.npy"]
    for f in got:
        assert np.array_equal(got[f], again[f]), f
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    assert got["loss.npy"].shape == (1,) and abs(float(got["loss.npy"][0]) - rec["final_loss"]) <= 1e-4
    assert got["params.npy"].shape == (4329088,) and float(np.abs(got["params.npy"]).max()) > 0
    assert got["logits.npy"].shape == (128, 10)
    np.testing.assert_allclose(np.exp(got["logits.npy"].astype(np.float64)).sum(1), 1.0, atol=1e-3)  # fp32 log-softmax


def test_bench_dump_default_mode(dev, bench_dump, tmp_path):
    """DISTLEARN_REDUCE_ATOMIC=2 --dump-outputs dumps the default (fp32-atomic)
    reduction mode, the one a run without the option times.  One step from the
    same seeded state differs from the deterministic mode only in the order of
    fp32 sums (BatchNorm statistics and parameter gradients), which can flip
    roundings of the step's bf16 operands: each output stays within one bf16
    rounding (2^-8) of the other mode's, in norm.  (Two mode-2 runs of one
    step measured 2e-6 of the parameters apart; more steps amplify that.)"""
    import numpy as np

    _, ref, _ = bench_dump
    rec, got, err = _bench_dump(tmp_path / "m2", mode=2)
    assert rec["config"]["reduce_mode"] == 2 and "deterministic reduction mode" not in err
    assert sorted(got) == sorted(ref)
    for f in got:
        a, b = got[f].astype(np.float64), ref[f].astype(np.float64)
        d = float(np.linalg.norm(a - b) / np.linalg.norm(b))
        print(f"{f}: mode 2 vs mode 0, relative difference {d:.3g}")
        assert got[f].dtype == np.float32 and a.shape == b.shape and d <= 2.0 ** -8, (f, d)


def test_bench_full_reports_comm(dev):
    """--full brings back what a plain run leaves out: the communication
    profile of the multi-node step configuration (--nworld-path 1), read from
    graph replays outside the timed region.  (The overlap policy is forced:
    timing its candidates is not what this test is about.)"""
    args = ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--nworld-path", "1", "--full"]
    rec = json.loads(_run(args, env={"DISTLEARN_POLICY": "full"}).strip().splitlines()[-1])
    comm = rec["comm"]
    assert comm["buckets"] == 3 and comm["bytes_per_step"] == 4329088 * 4 and comm["steps"] == 6
    assert comm["comm_ms"] > 0 and 0.0 <= comm["overlap_fraction"] <= 1.0
    assert rec["steps"] == 5 and rec["ms_per_step"] > 0


def test_run_captures_only_before_timed_steps(dev):
    """trainer.run captures the single-step and the unrolled graph before the
    first step, whatever nsteps is (the driver's --warmup 5 < unroll 8 case):
    later calls replay only (bench.py asserts the same on its timed region)."""
    tr = _trainer(dev, "hip", True, 29704)
    ld = _loader(dev, batch=16)
    tr.run(ld, 2, unroll=8)
    assert tr.captures == 4  # 1-, 2-, 4- and 8-step graphs
    tr.run(ld, 9, unroll=8)
    torch.cuda.synchronize()
    assert tr.captures == 4 and tr.steps == 11


def test_comm_profile_is_side_effect_free(dev, monkeypatch):
    """comm_profile runs eager calibration steps with HIP events around the
    bucket all-reduces (world-1 collectives forced through RCCL) and restores
    the training state: the next steps match a run that never profiled."""
    monkeypatch.setenv("DISTLEARN_RCCL_WORLD1", "1")
    outs = []
    for prof in (False, True):
        tr = _trainer(dev, "hip", True, 29705)
        ld = _loader(dev, batch=16)
        tr.run(ld, 3)
        if prof:
            st = tr.comm_profile(ld, steps=3)
            assert st["steps"] == 3 and st["buckets"] == len(tr.bucketer.ranges)
            assert st["comm_ms"] > 0 and 0.0 <= st["overlap_fraction"] <= 1.0
            assert st["bytes_per_step"] == tr.flat.total * 4
        tr.run(ld, 5)
        torch.cuda.synchronize()
        outs.append((tr.flat.data.clone(), int(ld.ctr[0]), int(tr.sgd.stepsPerNode.sum())))
    assert outs[0][1:] == outs[1][1:]
    assert torch.equal(outs[0][0], outs[1][0])


def test_comm_profile_from_graph_replays(dev, monkeypatch):
    """comm_profile(replay=True) reads the bucket timings from device-timestamp
    nodes of a captured one-step graph after each replay (the timed
    schedule): labelled as such, side-effect free like the eager profile, and
    within noise of the eager calibration (same buckets, same bytes, comm time
    within 3x -- a world-1 RCCL all-reduce is a few microseconds either way)."""
    monkeypatch.setenv("DISTLEARN_RCCL_WORLD1", "1")
    outs = []
    for prof in (False, True):
        tr = _trainer(dev, "hip", True, 29706)
        ld = _loader(dev, batch=16)
        tr.run(ld, 3)
        if prof:
            ev = tr.comm_profile(ld, steps=4)
            rp = tr.comm_profile(ld, steps=4, replay=True)
            assert "replay_error" not in ev
            assert rp["source"].startswith("graph replays"), rp.get("replay_error")
            assert rp["steps"] == 4 and rp["buckets"] == ev["buckets"] == len(tr.bucketer.ranges)
            assert rp["bytes_per_step"] == ev["bytes_per_step"] == tr.flat.total * 4
            assert rp["comm_ms"] > 0 and 0.0 <= rp["overlap_fraction"] <= 1.0
            # the eager calibration also times the host issuing each collective into
            # an idle comm stream (0.01-0.12 ms measured at world 1), the replay
            # does not: never more than eager plus noise
            assert rp["comm_ms"] <= ev["comm_ms"] + 0.02, (ev, rp)
        tr.run(ld, 5)
        torch.cuda.synchronize()
        outs.append((tr.flat.data.clone(), int(ld.ctr[0]), int(tr.sgd.stepsPerNode.sum())))
    assert outs[0][1:] == outs[1][1:]
    assert torch.equal(outs[0][0], outs[1][0])


def test_capture_timestamps_match_hip_events(dev):
    """The timestamp nodes comm_profile(replay=True) uses time a fixed GPU
    workload like HIP events do: 8 copies of 64 MB between two stamps in a
    replayed graph vs the same copies between two events, eagerly, within 10 %."""
    from torch_distlearn_amd.parallel.buckets import _Stamp

    a = torch.empty(16 << 20, device=dev)
    b = torch.ones(16 << 20, device=dev)
    stamps = [torch.zeros(4, dtype=torch.int64, device=dev), 0]
    s = torch.cuda.Stream()

    def work():
        for _ in range(8):
            a.copy_(b)

    with torch.cuda.stream(s):
        work()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        t0 = _Stamp.record(stamps, torch.cuda.current_stream())
        work()
        t1 = _Stamp.record(stamps, torch.cuda.current_stream())
    ev = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        work()
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    st = []
    for _ in range(5):
        g.replay()
        torch.cuda.synchronize()
        st.append(t0.elapsed_time(t1))
    ev_ms, st_ms = sorted(ev)[2], sorted(st)[2]
    assert ev_ms > 0.05 and abs(st_ms - ev_ms) <= 0.1 * ev_ms, (ev, st)


@pytest.mark.parametrize("mode", ["2"])
def test_atomic_modes_train_and_graph_tracks_eager(dev, monkeypatch, mode):
    """Reduction mode 2 (fp32 atomics: not bitwise reproducible run to
    run): the model fits a repeated batch, and graph replay tracks eager within
    the run-to-run noise of the atomics (measured with a one-off probe, since removed)."""
    monkeypatch.setenv("DISTLEARN_REDUCE_ATOMIC", mode)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(32, 32, 32, 3, device=dev, generator=g).to(torch.bfloat16)
    y = torch.randint(0, 10, (32,), device=dev, generator=g)
    res = []
    for graph in (False, True):
        tr = _trainer(dev, "hip", graph, 29706)
        assert tr.executor.atomic
        res.append([float(tr.step(x, y)) for _ in range(8)])
    for losses in res:
        assert losses[-1] < 0.5 * losses[0]
    assert max(abs(a - b) for a, b in zip(*res)) < 0.05 * res[0][0]


@pytest.mark.parametrize("rccl", ["0", "1"])
def test_ea_run_unrolled_matches_stepwise(dev, monkeypatch, rccl):
    """AllReduceEA under trainer.run: tau-step graphs that end with the
    elastic round (fused elastic kernel + delta all-reduce + center update)
    plus local-step graphs == one captured step at a time with the round run
    eagerly every tau steps (deterministic reduction mode: bitwise).
    rccl = 1: the world-1 delta all-reduce goes through RCCL (inside the
    captured tau-step graph)."""
    monkeypatch.setenv("DISTLEARN_RCCL_WORLD1", rccl)
    from torch_distlearn_amd import Tree
    from torch_distlearn_amd.engine import DataParallelTrainer
    from torch_distlearn_amd.models import CifarConvNet

    outs = []
    for unrolled in (False, True):
        tree = Tree(1, 1, host="127.0.0.1", port=29708, device=dev)
        assert tree.comm._skip1 == (rccl == "0")
        model = CifarConvNet(seed=9).to(dev)
        tr = DataParallelTrainer(model, tree, lr=0.02, algo="ea", tau=3, alpha=0.3, backend="hip",
                                 compute_dtype=torch.bfloat16, graph=True, max_batch=16)
        tr.synchronize_parameters()
        ld = _loader(dev, batch=16)
        if unrolled:
            tr.run(ld, 11, unroll=4)
            assert ("ea", 3) in tr._multi and tr.captures == 4  # 1-, 2-, 4-step graphs + the tau graph
        else:
            for _ in range(11):
                tr.step(ld)
        torch.cuda.synchronize()
        outs.append((tr.flat.data.clone(), tr.ea.center.clone(), tr.ea.step, int(ld.ctr[0]), tr.steps))
    (p0, c0, s0, k0, n0), (p1, c1, s1, k1, n1) = outs
    assert (s0, k0, n0) == (s1, k1, n1) == (11, 11, 11)
    assert not torch.equal(c0, p0)  # the rounds moved the center
    assert torch.equal(p0, p1) and torch.equal(c0, c1)


def test_bf16_grad_wire_through_rccl(dev, monkeypatch):
    """grad_comm_dtype="bf16" (world-1 collectives forced through RCCL, inside
    the captured graph): the bucket all-reduces move half the bytes, the fp32
    participation count rides in the same group, and the update (the fused
    SGD reading the bf16 wire copy) matches the fp32 wire to bf16 tolerance
    (one step from the same state: later steps add chaotic training drift)."""
    monkeypatch.setenv("DISTLEARN_RCCL_WORLD1", "1")
    g = torch.Generator(device=dev).manual_seed(4)
    xs = torch.randn(3, 32, 32, 32, 3, device=dev, generator=g).to(torch.bfloat16)
    ys = torch.randint(0, 10, (3, 32), device=dev, generator=g)
    res = {}
    for wire in ("fp32", "bf16"):
        tr = _trainer(dev, "hip", True, 29707, grad_comm_dtype=wire)
        assert tr.grad_comm_dtype == wire
        before = tr.flat.data.clone()
        tr.step(xs[0], ys[0])
        torch.cuda.synchronize()
        assert float(tr.flat.slot) == 1.0
        delta = tr.flat.data - before
        for i in range(1, 3):  # keeps training (replays) with the wire
            tr.step(xs[i], ys[i])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(tr.flat.data).all())
        ld = _loader(dev, batch=16)
        st = tr.comm_profile(ld, steps=2)
        res[wire] = (delta, st["bytes_per_step"])
    (d32, b32), (d16, b16) = res["fp32"], res["bf16"]
    assert b16 * 2 == b32
    rel = float((d16 - d32).norm() / d32.norm())
    assert rel < 0.01, rel


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_deferred_slab_reduce_is_bitwise(dev, monkeypatch, momentum):
    """One node: the split-K weight-gradient slabs of blocks 1-3 are summed by
    the fused SGD itself (no slab_reduce launches; engine.py _slabs) -- the
    parameters after unrolled-graph training are BITWISE those of the path with
    the stand-alone reduce (deterministic reduction mode; batch 128: 19 splits
    summed on 8 lanes + a shuffle tree, 5 sequentially, and the first layer's
    channel-padded 128 splits on 32 lanes in extra blocks of the launch);
    with the side jobs, blocks 3-4 and the classifier are updated by extra
    workgroups of block 3's dgrad launch and block 2 by extra workgroups of
    the first layer's weight-gradient launch -- still bitwise the same; and with
    the update launch preparing the next step of the unrolled graph (its
    batch gathered, accumulators zeroed, first-layer operand packed: the
    executor's next_prep) -- still bitwise, across an epoch boundary."""
    from torch_distlearn_amd import Tree
    from torch_distlearn_amd.data import DeviceLoader, PartitionedDataset, synthetic_cifar10
    from torch_distlearn_amd.engine import DataParallelTrainer
    from torch_distlearn_amd.models import CifarConvNet

    imgs, labels = synthetic_cifar10(1024, seed=5)
    outs = []
    for defer, side, nxt in (("0", "0", "0"), ("1", "0", "0"), ("1", "1", "0"), ("1", "1", "1")):
        monkeypatch.setenv("DISTLEARN_DEFER_SLABS", defer)
        monkeypatch.setenv("DISTLEARN_SIDE_SGD", side)
        monkeypatch.setenv("DISTLEARN_PREP_NEXT", nxt)
        tree = Tree(1, 1, host="127.0.0.1", port=29712, device=dev)
        model = CifarConvNet(seed=4).to(dev)
        tr = DataParallelTrainer(model, tree, lr=0.02, momentum=momentum, backend="hip",
                                 compute_dtype=torch.bfloat16, graph=True, max_batch=128)
        tr.synchronize_parameters()
        if defer == "1":
            blocks = sorted(e[0] // 4 for e in tr._slabs)
            # block 4's wgrad has split-K slabs only with the position-major plan (4 splits)
            assert blocks in ([0, 1, 2], [0, 1, 2, 3]), blocks
            ks = {e[0] // 4: e[2] for e in tr._slabs}
            assert ks[2] < 8 <= ks[1] < 32 <= ks[0], ks  # sequential, 8 lanes + tree, 32 lanes (padded tail)
            # side == "1": blocks 3-4 + classifier updated inside block 3's dgrad launch,
            # block 2 inside the first layer's weight-gradient launch
            assert (tr._side is not None) == (side == "1")
            if side == "1":
                assert tr._side == (tr.flat.offsets[4], tr.flat.total)
                assert tr.executor._side["w"]["range"] == (tr.flat.offsets[4], tr.flat.offsets[8])
        else:
            assert tr._slabs is None and tr._side is None
        assert tr.grads_materialized == (defer == "0")  # flat.grad is not written for deferred slabs
        ld = DeviceLoader(PartitionedDataset(imgs, labels, device=dev), "permutation", 128, seed=2)
        tr.run(ld, 11, unroll=4)  # 8 steps per epoch: graphs of 4, 2, 1 steps, then a new epoch
        torch.cuda.synchronize()
        assert (tr.executor.prepared_ahead > 0) == (nxt == "1")
        assert not tr.executor._prepared  # no step is left marked as prepared
        assert not hasattr(tr.executor.C, "arm_sgd_next_prep")
        outs.append(tr.flat.data.clone())
    assert all(torch.equal(outs[0], o) for o in outs[1:])


def test_policy_selected_on_the_machine(dev, monkeypatch):
    """the world > 1 overlap policy is measured, not guessed.
    Forced RCCL at world 1 with DISTLEARN_POLICY_SELECT=1: prepare() captures
    each candidate as a one-step graph, times its replays, keeps the faster
    (recorded with both timings), restores the training state, and the run
    afterwards trains normally on the chosen policy."""
    monkeypatch.setenv("DISTLEARN_RCCL_WORLD1", "1")
    monkeypatch.setenv("DISTLEARN_POLICY_SELECT", "1")
    tr = _trainer(dev, "hip", True, 29714)
    ld = _loader(dev)
    p0 = tr.flat.data.clone()
    tr.prepare(ld, 4)
    torch.cuda.synchronize()
    pol = tr.policy
    names = {f"{p}@{c}" for p in ("full", "reserve", "wreserve") for c in (16, 32)}  # x the measured channel caps
    assert pol is not None and pol["chosen"] in names, pol
    assert set(pol["ms_per_step"]) == names and all(v > 0 for v in pol["ms_per_step"].values())
    assert pol["chosen"] == min(pol["ms_per_step"], key=pol["ms_per_step"].get)
    want = pol["candidates"][pol["chosen"]]
    assert (tr.executor.dgrad_stages, tr.executor.cu_reserve) == (want["dgrad_stages"], want["cu_reserve"])
    assert tr.tree.comm.channel_cap == want["channel_cap"] == pol["channel_cap"]
    assert tr.tree.comm._c.max_ctas == want["channel_cap"]  # the communicator was rebuilt with the chosen cap
    assert torch.equal(tr.flat.data, p0) and int(ld.ctr[0]) == 0  # selection changed no training state
    loss = tr.run(ld, 6, unroll=4)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and int(tr.sgd.stepsPerNode.sum()) == 6


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_multinode_fused_reduce_is_bitwise(dev, monkeypatch, momentum):
    """The multi-node step configuration (gradients all-reduced: world-1
    collectives forced through RCCL, so no one-node slab deferral): the
    split-K slab sums ride block 3's dgrad launch and ONE reduce-only launch
    sums blocks 1-2 (executor fuse_slab_reduces), and the full-buffer update
    launch prepares the next step of the unrolled graph (its batch, zeroed
    accumulators, the first layer's packed operand from the main loop) --
    parameters after unrolled training across an epoch boundary are BITWISE
    those of the plain path (a slab_reduce launch per layer, a prep launch
    per step)."""
    from torch_distlearn_amd import Tree
    from torch_distlearn_amd.data import DeviceLoader, PartitionedDataset, synthetic_cifar10
    from torch_distlearn_amd.engine import DataParallelTrainer
    from torch_distlearn_amd.models import CifarConvNet

    monkeypatch.setenv("DISTLEARN_RCCL_WORLD1", "1")
    imgs, labels = synthetic_cifar10(1024, seed=5)
    outs = []
    for fuse, nxt in (("0", "0"), ("1", "0"), ("1", "1")):
        monkeypatch.setenv("DISTLEARN_FUSE_REDUCE", fuse)
        monkeypatch.setenv("DISTLEARN_PREP_NEXT", nxt)
        tree = Tree(1, 1, host="127.0.0.1", port=29716, device=dev)
        model = CifarConvNet(seed=4).to(dev)
        tr = DataParallelTrainer(model, tree, lr=0.02, momentum=momentum, backend="hip",
                                 compute_dtype=torch.bfloat16, graph=True, max_batch=128)
        tr.synchronize_parameters()
        assert tr.reduces_grads and tr._slabs is None and tr._side is None and tr.grads_materialized
        if fuse == "1":
            # (block 4's slabs exist with the position-major wgrad plan; its dgrad hosts their sums)
            ride = [2] if tr.executor.wplan[3][2] else [2, 3]
            assert tr._fused_reduce == {"ride": ride, "merged": [0, 1]}, tr._fused_reduce
        else:
            assert tr._fused_reduce is None
        ld = DeviceLoader(PartitionedDataset(imgs, labels, device=dev), "permutation", 128, seed=2)
        tr.run(ld, 11, unroll=4)
        torch.cuda.synchronize()
        assert (tr.executor.prepared_ahead > 0) == (nxt == "1")
        assert not tr.executor._prepared  # no step is left marked as prepared
        assert not hasattr(tr.executor.C, "arm_sgd_next_prep")
        outs.append(tr.flat.data.clone())
    assert all(torch.equal(outs[0], o) for o in outs[1:])


def test_policy_change_drops_captured_graphs(dev, monkeypatch):
    """a policy switch re-allocates the executor's workspaces, so
    graphs captured before it (step() with graph=True) must never replay:
    select_policy with a forced policy after a captured step drops them and
    the next run() recaptures and trains on the new buffers."""
    monkeypatch.setenv("DISTLEARN_POLICY", "reserve")
    tr = _trainer(dev, "hip", True, 29717)
    ld = _loader(dev)
    tr.step(ld)
    assert tr._graph is not None
    old = tr._graph
    tr.run(ld, 4, unroll=2)
    torch.cuda.synchronize()
    assert tr.policy["chosen"] == "reserve" and tr._graph is not old
    assert (tr.executor.dgrad_stages, tr.executor.cu_reserve) == (2, tr.executor.policies()["reserve"]["cu_reserve"])
    assert torch.isfinite(tr.flat.data).all() and int(tr.sgd.stepsPerNode.sum()) == 5
