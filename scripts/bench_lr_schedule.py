#!/usr/bin/env python3
"""What a learning-rate schedule costs on the graph path: the CIFAR-10 convnet
of bench.py (HIP executor, batch 128, one GPU), 16-step graphs, 50 timed steps
per round, a trainer with ``lr_schedule=constant(lr)`` against one without a
schedule, rounds interleaved in one process.  The expected extra is one small
launch (lr_ring_set) per graph replay.  Prints one JSON line; reported, not gated.

    python scripts/bench_lr_schedule.py [--rounds 7] [--steps 50] [--unroll 16]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--unroll", type=int, default=16)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--lr", type=float, default=0.1)
    a = ap.parse_args()

    from torch_distlearn_amd import Tree, constant
    from torch_distlearn_amd.data import DeviceLoader, PartitionedDataset
    from torch_distlearn_amd.engine import DataParallelTrainer
    from torch_distlearn_amd.models import CifarConvNet
    from torch_distlearn_amd.utils.color_print import set_verbose

    set_verbose(False)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tree = Tree(1, 1, host="127.0.0.1", port=int(os.environ.get("MASTER_PORT", "29518")), device=dev)
    g = torch.Generator(device=dev).manual_seed(1234)
    imgs = torch.randint(0, 256, (50000, 32, 32, 3), dtype=torch.uint8, device=dev, generator=g)
    labs = torch.randint(0, 10, (50000,), device=dev, generator=g)

    runs = {}
    for name, sched in (("none", None), ("constant", constant(a.lr))):
        tr = DataParallelTrainer(CifarConvNet(seed=0).to(dev), tree, lr=a.lr, backend="hip",
                                 compute_dtype=torch.bfloat16, graph=True, max_batch=a.batch, lr_schedule=sched)
        tr.synchronize_parameters()
        ld = DeviceLoader(PartitionedDataset(imgs, labs, device=dev), "permutation", a.batch, seed=0)
        tr.run(ld, a.warmup, unroll=a.unroll)
        runs[name] = (tr, ld, [])
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, (tr, ld, ms) in runs.items():
            c0 = tr.captures
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.run(ld, a.steps, unroll=a.unroll)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
            assert tr.captures == c0, "a capture fell into the timed region"
    med = {n: statistics.median(ms) for n, (_, _, ms) in runs.items()}
    replays = a.steps // a.unroll + bin(a.steps % a.unroll).count("1")  # graphs of unroll, then of the powers of two
    out = {"metric": "ms_per_step", "batch": a.batch, "steps": a.steps, "unroll": a.unroll, "rounds": a.rounds,
           "replays_per_round": replays,
           "median_ms_per_step": {n: round(v, 4) for n, v in med.items()},
           "schedule_extra_us_per_step": round((med["constant"] - med["none"]) * 1e3, 2),
           "ms_per_step": {n: [round(v, 4) for v in ms] for n, (_, _, ms) in runs.items()},
           "final_loss": {n: round(float(tr.last_loss), 4) for n, (tr, _, _) in runs.items()}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
