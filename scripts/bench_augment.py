"""Cost of the crop / flip augmentation in the device data path, at batch 128:
augmentation on (crop4flip) against off, interleaved round by round, two ways:

* the stand-alone prep launch (gather + normalise + pad + layer-1 pack),
  graph-replayed like scripts/bench_prep.py: us per launch;
* ms per step of ``trainer.run(loader, 64, unroll=16)`` (replayed 16-step
  hipGraphs whose update launches carry the next step's gather).

Prints every round, then the medians and each side's spread (max - min).

Usage:  python scripts/bench_augment.py [--rounds 7] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from torch_distlearn_amd import Tree, _native  # noqa: E402
from torch_distlearn_amd.data import Augment, DeviceLoader, PartitionedDataset  # noqa: E402
from torch_distlearn_amd.engine import DataParallelTrainer  # noqa: E402
from torch_distlearn_amd.models import CifarConvNet, make_executor  # noqa: E402
from torch_distlearn_amd.ops.flat import FlatParams  # noqa: E402

BATCH = 128
AUG = Augment(pad=4, flip=True, seed=1)


def dataset(dev):
    g = torch.Generator(device=dev).manual_seed(0)
    imgs = torch.randint(0, 256, (50000, 32, 32, 3), dtype=torch.uint8, device=dev, generator=g)
    labs = torch.randint(0, 10, (50000,), device=dev, generator=g)
    return PartitionedDataset(imgs, labs, device=dev)


def prep_graph(ex, ld, iters=1000):
    """A graph of ``iters`` stand-alone prep launches on ``ld``."""
    s = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    for _ in range(3):
        ex._prep(ld, s(), with_transposes=False)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            ex._prep(ld, s(), with_transposes=False)
    g.replay()
    torch.cuda.synchronize()
    return g, iters


def time_graph(g, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us per launch


def time_run(tr, ld, steps=64):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.run(ld, steps, unroll=16)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps  # ms per step


def summary(name, unit, off, on):
    so, sn = max(off) - min(off), max(on) - min(on)
    mo, mn = statistics.median(off), statistics.median(on)
    return (f"{name}: off median {mo:.4f} {unit} (spread {so:.4f}), on median {mn:.4f} {unit} (spread {sn:.4f}), "
            f"on - off = {mn - mo:+.4f} {unit} ({100 * (mn - mo) / mo:+.2f}%)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment needs the GPU")
    _native.native()
    dev = torch.device("cuda", 0)
    ds = dataset(dev)
    lines = [f"batch {BATCH}, 50000 random 32x32x3 images, augmentation on = pad {AUG.pad} + flip; "
             f"{opt.rounds} rounds, off / on alternating"]

    # 1. the stand-alone prep launch
    model = CifarConvNet(seed=0).to(dev)
    ex = make_executor(model, FlatParams(model, grads=True, shadow_bf16=True), max_batch=BATCH)
    sides = {name: prep_graph(ex, DeviceLoader(ds, "permutation", BATCH, seed=0, augment=aug))
             for name, aug in (("off", None), ("on", AUG))}
    res = {"off": [], "on": []}
    for r in range(opt.rounds):
        for name in ("off", "on"):
            res[name].append(time_graph(*sides[name]))
        lines.append(f"prep launch round {r}: off {res['off'][-1]:.3f} us  on {res['on'][-1]:.3f} us")
    lines.append(summary("prep launch", "us", res["off"], res["on"]))
    del sides, ex

    # 2. trainer.run over unrolled graphs
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    runs = {}
    for i, (name, aug) in enumerate((("off", None), ("on", AUG))):
        tree = Tree(1, 1, host="127.0.0.1", port=29760 + i, device=dev)
        tr = DataParallelTrainer(CifarConvNet(seed=0).to(dev), tree, lr=0.05, backend="hip",
                                 compute_dtype=torch.bfloat16, graph=True, max_batch=BATCH)
        tr.synchronize_parameters()
        ld = DeviceLoader(ds, "permutation", BATCH, seed=0, augment=aug)
        tr.prepare(ld, 16)
        for _ in range(2):
            time_run(tr, ld)  # warm-up
        runs[name] = (tr, ld)
    res = {"off": [], "on": []}
    for r in range(opt.rounds):
        for name in ("off", "on"):
            res[name].append(time_run(*runs[name]))
        lines.append(f"trainer.run round {r}: off {res['off'][-1]:.4f} ms/step  on {res['on'][-1]:.4f} ms/step")
    lines.append(summary("trainer.run(loader, 64, unroll=16)", "ms/step", res["off"], res["on"]))
    assert runs["on"][0].executor.prepared_ahead > 0, "the update launches did not carry the gather"

    print("\n".join(lines))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
