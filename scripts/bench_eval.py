#!/usr/bin/env python3
"""A/B of the test-set evaluation on one GPU: the example's host-driven loop
against the device-resident pass.

  path A   examples/cifar10.py --testPath batcher: per batch a host sampler
           call, a pinned index copy, gather_normalize + index_select,
           trainer.predict (eager launches, the eval BN coefficients derived
           again per batch) and the confusion kernel
  path B   trainer.evaluate on a DeviceEvalLoader: forward-only hipGraphs of
           up to --unroll steps, the coefficients derived once, metrics in the
           head kernel, no host work per batch

Both run in ONE process, interleaved (A, B, train, A, B, train, ...): one
warm-up round, then --rounds timed rounds, each path timed with device events
around its whole pass and a synchronise; medians and the min..max spread are
reported.  For scale, each round also times a training epoch's worth of steps
(--trainImages / batch) through trainer.run at the same batch, and
evaluation's share of epoch + evaluation is printed for both paths.

    python scripts/bench_eval.py --out profiles/eval_graph_ab.txt
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from torch_distlearn_amd import Tree  # noqa: E402
from torch_distlearn_amd.data import (DeviceEvalLoader, DeviceLoader, PartitionedDataset,  # noqa: E402
                                      synthetic_cifar10)
from torch_distlearn_amd.engine import DataParallelTrainer  # noqa: E402
from torch_distlearn_amd.models import CifarConvNet  # noqa: E402
from torch_distlearn_amd.utils.metrics import ConfusionMatrix  # noqa: E402


def timed(fn):
    """(device ms between events around fn, fn's result); ends in a synchronise."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def bench_batch(dev, batch, opt, port, say):
    tree = Tree(1, 1, host="127.0.0.1", port=port, device=dev)
    trainer = DataParallelTrainer(CifarConvNet(seed=0).to(dev), tree, lr=0.05, backend="hip",
                                  compute_dtype=torch.bfloat16, graph=True, max_batch=batch)
    trainer.synchronize_parameters()
    train = PartitionedDataset(*synthetic_cifar10(opt.trainSet, seed=0), device=dev)
    test = PartitionedDataset(*synthetic_cifar10(opt.n, seed=1), device=dev)
    train_l = DeviceLoader(train, "label-uniform", batch, seed=1)
    test_b = test.sampledBatcher("linear", batch, dtype=torch.bfloat16)
    test_l = DeviceEvalLoader(test, batch)
    epoch_steps = opt.trainImages // batch
    trainer.prepare(train_l, opt.unroll)
    trainer.prepare_eval(test_l, opt.unroll)
    caps = (trainer.captures, trainer.eval_captures)

    def path_a():  # the example's loop, as it stands
        conf = ConfusionMatrix(10, device=dev)
        test_b.reset()
        for _ in range(test_b.numBatches()):
            x, y = test_b.getBatch()
            conf.add(trainer.predict(x), y)
        return conf.mat

    def path_b():
        conf = ConfusionMatrix(10, device=dev)
        trainer.evaluate(test_l, conf, unroll=opt.unroll)
        return conf.mat

    ms = {"A": [], "B": [], "train": []}
    for r in range(opt.rounds + 1):  # round 0 warms every path up
        ta, ma = timed(path_a)
        tb, mb = timed(path_b)
        tt, _ = timed(lambda: trainer.run(train_l, epoch_steps, unroll=opt.unroll))
        if r:
            ms["A"].append(ta)
            ms["B"].append(tb)
            ms["train"].append(tt)
        acc = [float(m.diagonal().sum()) / float(m.sum()) for m in (ma, mb)]
    assert (trainer.captures, trainer.eval_captures) == caps, "a capture inside the timed rounds"
    med = {k: statistics.median(v) for k, v in ms.items()}
    say(f"batch {batch}: {opt.n} test images = {test_l.steps} batches; training epoch = {epoch_steps} steps "
        f"({opt.trainImages} images); {opt.rounds} timed rounds after 1 warm-up, interleaved A, B, train")
    for k, name in (("A", "A  batcher + predict loop   "), ("B", "B  evaluate (device graphs) "),
                    ("train", "   training epoch (run)     ")):
        v = ms[k]
        say(f"  {name} median {med[k]:9.2f} ms   min {min(v):9.2f}   max {max(v):9.2f}   "
            f"spread {100 * (max(v) - min(v)) / med[k]:5.1f} %")
    spread_a = max(ms["A"]) - min(ms["A"])
    if abs(med["A"] - med["B"]) <= spread_a:
        verdict = "a tie (within path A's run-to-run spread)"
    else:
        verdict = f"path B is {med['A'] / med['B']:.2f}x path A's speed" if med["B"] < med["A"] else \
            f"path B is SLOWER: {med['B'] / med['A']:.2f}x path A's time"
    say(f"  verdict: {verdict}; per batch A {1e3 * med['A'] / test_l.steps:.1f} us, "
        f"B {1e3 * med['B'] / test_l.steps:.1f} us; training step {1e3 * med['train'] / epoch_steps:.1f} us")
    say(f"  evaluation's share of (training epoch + evaluation): A {100 * med['A'] / (med['A'] + med['train']):.1f} %, "
        f"B {100 * med['B'] / (med['B'] + med['train']):.1f} %")
    say(f"  samples counted: A {int(ma.sum())} (the padded tail of the last batch counts again), B {int(mb.sum())}; "
        f"accuracy A {100 * acc[0]:.2f} %, B {100 * acc[1]:.2f} %")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10000, help="synthetic test images")
    ap.add_argument("--trainImages", type=int, default=50000, help="images of the training epoch timed for scale")
    ap.add_argument("--trainSet", type=int, default=10000, help="synthetic training images resident (epochs wrap)")
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--unroll", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the report here (first line: the command)")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures on the GPU: no device found")
    if opt.rounds < 1:
        raise SystemExit("--rounds must be at least 1")
    dev = torch.device("cuda:0")
    lines = ["$ python " + " ".join(["scripts/bench_eval.py"] + sys.argv[1:]),
             f"{torch.cuda.get_device_name(0)}; torch {torch.__version__}; times are device-event ms around a whole "
             f"pass (synchronised), one process"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for ln in lines:
        print(ln, flush=True)
    for i, b in enumerate(opt.batches):
        bench_batch(dev, b, opt, 29760 + i, say)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
