"""DeviceEvalLoader's order logic on CPU tensors, and
DataParallelTrainer.evaluate on the generic (predict-loop) path: every sample
of the partition exactly once, the padded tail of the last batch not counted."""
import pytest
import torch

from torch_distlearn_amd.data import DeviceEvalLoader, PartitionedDataset, synthetic_cifar10


def _ds(n, partition=1, partitions=1, seed=5):
    imgs, labels = synthetic_cifar10(n, seed=seed)
    return PartitionedDataset(imgs, labels, partition, partitions)


# (N, batch, partition, partitions) -> (lo, hi, steps, tail rows of the last batch)
SHAPES = [
    ((200, 32, 1, 1), (0, 200, 7, 8)),
    ((256, 16, 2, 3), (85, 170, 6, 5)),
    ((64, 64, 1, 1), (0, 64, 1, 64)),   # one full step, no padding
    ((5, 32, 1, 1), (0, 5, 1, 5)),      # one partial step
]


@pytest.mark.parametrize("shape,want", SHAPES)
def test_order_covers_partition_once_then_repeats_last(shape, want):
    n, batch, part, parts = shape
    lo, hi, steps, tail = want
    ld = DeviceEvalLoader(_ds(n, part, parts), batch)
    assert (ld.n_valid, ld.steps, ld.n_order) == (hi - lo, steps, steps * batch)
    assert ld.numBatches() == steps
    assert ld.n_valid - (steps - 1) * batch == tail
    assert ld.order.dtype == torch.int32 and tuple(ld.order.shape) == (steps * batch,)
    assert torch.equal(ld.order[:ld.n_valid], torch.arange(lo, hi, dtype=torch.int32))
    assert bool((ld.order[ld.n_valid:] == hi - 1).all())
    assert ld.ctr.dtype == torch.int64 and tuple(ld.ctr.shape) == (2,)
    assert ld.labels_out.dtype == torch.int64 and tuple(ld.labels_out.shape) == (batch,)
    assert ld.pred.dtype == torch.int32 and ld.nll.dtype == torch.float32
    assert tuple(ld.pred.shape) == tuple(ld.nll.shape) == (steps * batch,)
    assert ld.mat.dtype == torch.int64 and tuple(ld.mat.shape) == (10, 10)
    args = ld.gather_args()
    assert len(args) == 9 and args[1] == ld.order.data_ptr() and args[4] == ld.ctr.data_ptr()
    assert args[5] == steps * batch and args[6] == 3
    # the last batch's valid rows
    x, y, valid = ld.host_batch(steps - 1)
    assert valid == tail and tuple(x.shape) == (batch, 32, 32, 3) and tuple(y.shape) == (batch,)
    assert torch.equal(y[:valid], ld.ds.labels[hi - tail:hi])


def test_partitions_cover_every_sample_exactly_once():
    seen = []
    for p in (1, 2, 3):
        ld = DeviceEvalLoader(_ds(256, p, 3), 16)
        seen.append(ld.order[:ld.n_valid])
    assert torch.equal(torch.cat(seen), torch.arange(256, dtype=torch.int32))


def test_reset_rewinds_counter_matrix_and_results():
    ld = DeviceEvalLoader(_ds(40), 16)
    ld.ctr += 3
    ld.mat += 1
    ld.pred.fill_(4)
    ld.nll.fill_(1.5)
    ld.reset()
    assert not ld.ctr.any() and not ld.mat.any() and not ld.nll.any()
    assert bool((ld.pred == DeviceEvalLoader.PRED_RESET).all())


def test_evaluate_generic_backend_honours_the_tail():
    from torch_distlearn_amd import Tree
    from torch_distlearn_amd.engine import DataParallelTrainer
    from torch_distlearn_amd.models import CifarConvNet
    from torch_distlearn_amd.utils.metrics import ConfusionMatrix

    tree = Tree(1, 1, host="127.0.0.1", port=0)
    model = CifarConvNet(seed=3)
    tr = DataParallelTrainer(model, tree, lr=0.05, backend="torch", compute_dtype=torch.float32)
    ds = _ds(200)
    # a few training steps: running statistics off their initial values
    g = torch.Generator().manual_seed(0)
    for _ in range(2):
        idx = torch.randint(0, 200, (16,), generator=g)
        x = (ds.images[idx].float() / 255.0 - 0.5) / 0.25
        tr.step(x, ds.labels[idx])
    params = tr.flat.data.clone()
    bufs = [b.detach().clone() for b in model.buffers()]
    steps_before = tr.steps

    ld = DeviceEvalLoader(ds, 32)
    conf = ConfusionMatrix(10)
    res = tr.evaluate(ld, conf)
    assert res["count"] == 200 and int(res["mat"].sum()) == 200
    assert torch.equal(conf.mat, res["mat"])

    # hand-written loop over predict, first `valid` rows of the last batch only
    ref = ConfusionMatrix(10)
    preds, nlls = [], []
    for k in range(ld.steps):
        x, y, valid = ld.host_batch(k)
        logp = tr.predict(x)[:valid]
        ref.add(logp, y[:valid])
        preds.append(logp.argmax(1).to(torch.int32))
        nlls.append(-logp[torch.arange(valid), y[:valid]])
    assert valid == 8
    assert torch.equal(res["mat"], ref.mat)
    assert torch.equal(res["pred"], torch.cat(preds))
    assert torch.equal(res["nll"], torch.cat(nlls))
    assert torch.equal(res["loss_sum"], torch.cat(nlls).sum())

    again = tr.evaluate(ld)
    for key in ("mat", "pred", "nll", "loss_sum"):
        assert torch.equal(again[key], res[key])
    assert torch.equal(conf.mat, res["mat"])  # no conf given: untouched

    assert torch.equal(tr.flat.data, params)
    for b, v in zip(model.buffers(), bufs):
        assert torch.equal(b, v)
    assert tr.steps == steps_before and model.training
