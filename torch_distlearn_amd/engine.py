"""Data-parallel training engine: one object that owns the flat parameter
storage, the communicator-facing algorithm (AllReduceSGD / AllReduceEA), the
bucketed gradient all-reduce and the per-step execution (eager or
hipGraph-captured).

Reference equivalent: the hand-written loop of examples/cifar10.lua:172-208
(df -> sumAndNormalizeGradients -> per-tensor SGD -> epoch-end
synchronizeParameters) and examples/mnist-ea.lua:91-122 (SGD ->
averageParameters -> synchronizeCenter).  The algorithms keep the reference's
exact API (they are usable without this class); the engine is the MI355X-fast
way to drive them:

* parameters live in ONE flat fp32 buffer with a bf16 shadow
  (:class:`~torch_distlearn_amd.ops.flat.FlatParams`), gradients in one flat
  fp32 buffer whose header carries the participation count ``n``;
* ``backend="hip"`` runs the model through the hand-written gfx950 kernels
  (:mod:`torch_distlearn_amd.models.cifar_hip`) which write fp32 gradients
  straight into the flat buffer and signal each bucket as soon as its last
  gradient is written, so its RCCL all-reduce overlaps the rest of backward on
  a high-priority comm stream;
* ``backend="torch"`` runs the same parameters through PyTorch ops (CPU tests,
  numerics reference, MIOpen baseline);
* the update is ONE fused kernel (1/n + SGD + bf16 shadow refresh);
* ``graph=True`` captures forward + backward + all-reduce + update into one
  hipGraph and replays it (RCCL collectives are capturable), removing the
  per-kernel host launch cost that dominates a 4-layer convnet step;
* ``lr_schedule=`` (:mod:`torch_distlearn_amd.schedules`): the learning rate
  follows a host-side schedule in every mode.  A kernel argument is frozen
  when a step is captured, so the captured update kernels read the rate from
  a small device ring instead (step ``i`` of a graph reads ``ring[i]``) and
  the trainer writes the next rates into it with one small launch before
  every replay.
"""
from __future__ import annotations

import os

import contextlib
from typing import Any, Callable, Optional

import torch

from .ops.flat import FlatParams, fill_, lr_ring_set_
from .parallel.allreduce_ea import AllReduceEA
from .parallel.allreduce_sgd import AllReduceSGD
from .parallel.buckets import GradBucketer
from .parallel.comm import runs_collectives
from .parallel.tree import Tree
from .schedules import as_fp32, constant

LR_RING = 64  # floats in the device ring of learning rates: the longest graph a schedule can feed


def agree_on_policy(comm, local_ms: dict) -> tuple:
    """Pick one executor policy on every rank from each rank's measured
    step times: a step is as slow as its slowest rank, so the times are
    max-reduced over the ranks (control plane) and the policy with the
    smallest maximum wins.  Collective: every rank calls it with the same
    policy names.  Returns (name, {name: max ms})."""
    names = sorted(local_ms)
    t = torch.tensor([float(local_ms[n]) for n in names], dtype=torch.float64)
    comm.all_reduce_host(t, "max")
    table = {n: round(float(v), 4) for n, v in zip(names, t.tolist())}
    best = min(names, key=lambda n: (table[n], n))
    return best, table


# hipGraph capture mode: "thread_local" -- only this thread's unsafe HIP calls
# may invalidate a capture (see _capturing for the other threads / finalizers)
_CAPTURE_MODE = os.environ.get("DISTLEARN_CAPTURE_MODE", "thread_local")


@contextlib.contextmanager
def _capturing(comm):
    """Around a hipGraph capture: the communicator's watchdog stops polling
    (its hipEventQuery / RCCL async-error query from another thread) and the
    cyclic garbage collector is off (a finaliser of an unreachable CUDA
    object -- a stream, an event, another trainer's communicator -- would
    issue HIP calls on this thread mid-capture).  Either invalidated captures
    intermittently ("operation not permitted when stream is capturing")."""
    import gc

    pause = getattr(comm, "pause_watch", None)
    if pause is not None:
        pause(True)
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()
        if pause is not None:
            pause(False)


@torch.no_grad()
def predict_module(model: torch.nn.Module, x: torch.Tensor, compute_dtype, batch_stats: bool = False):
    """Forward of a PyTorch-path model without training side effects: eval
    mode, or train-mode BatchNorm on the batch's statistics with the running
    statistics restored afterwards."""
    was = model.training
    saved = [(b, b.detach().clone()) for b in model.buffers()] if batch_stats else []
    model.train(batch_stats)
    try:
        return model(x, compute_dtype=compute_dtype)
    finally:
        for b, v in saved:
            b.detach().copy_(v)
        model.train(was)


class DataParallelTrainer:
    def __init__(self, model: torch.nn.Module, tree: Tree, lr: float = 0.1, momentum: float = 0.0,
                 weight_decay: float = 0.0, algo: str = "sgd", tau: int = 10, alpha: float = 0.2,
                 backend: str = "torch", compute_dtype: torch.dtype = torch.bfloat16,
                 bucket_bytes: int = 4 << 20, overlap: bool = True, graph: bool = False,
                 loss_fn: Optional[Callable] = None, max_batch: Optional[int] = None,
                 async_ea: Optional[Any] = None, grad_comm_dtype: str = "fp32",
                 lr_schedule: Optional[Callable[[int], float]] = None):
        self.model = model
        self.tree = tree
        self.lr, self.momentum, self.weight_decay = lr, momentum, weight_decay
        self.algo = algo
        self.backend = backend
        self.compute_dtype = compute_dtype
        dev = next(model.parameters()).device
        self.device = dev
        # lr_schedule: t -> rate of update t (schedules.py); sched_step = updates
        # applied so far.  Eager steps set self.lr from it before the step body;
        # captured steps read the rate from the device ring (allocated once:
        # policy changes that drop graphs do not move it), _advance_lr.
        self.lr_schedule = lr_schedule
        self.sched_step = 0
        self._cap_slot: Optional[int] = None  # ring slot of the step body being captured
        self._lr_ring = None
        if lr_schedule is not None:
            self.lr = self._rate(0)
            if dev.type == "cuda":
                self._lr_ring = torch.full((LR_RING,), self.lr, dtype=torch.float32, device=dev)
        bf16_shadow = dev.type == "cuda" and compute_dtype == torch.bfloat16
        self.flat = FlatParams(model, grads=True, shadow_bf16=bf16_shadow)
        self.mom = self.flat.like(0.0) if momentum else None
        self.loss_fn = loss_fn or getattr(model, "loss", None) or torch.nn.functional.nll_loss
        # a model's fused forward_loss (ResNet-50: mean NLL with the classifier
        # backward in the same node) trains the model's own loss, so it is used
        # only when the caller did not pass a loss_fn of their own
        self._fused_loss_ok = loss_fn is None
        hooks = overlap and backend == "torch"
        # grad_comm_dtype="bf16": the bucketed all-reduce sends a bf16 copy of the
        # gradient (half the xGMI bytes) with the participation count in fp32
        self.bucketer = GradBucketer(tree.comm, self.flat, bucket_bytes=bucket_bytes, hooks=hooks,
                                     wire=grad_comm_dtype) \
            if (tree.numNodes > 1 or dev.type == "cuda") and algo == "sgd" else None
        self.grad_comm_dtype = self.bucketer.wire if self.bucketer is not None else "fp32"
        self.aea = None
        if algo == "sgd":
            self.sgd = AllReduceSGD(tree, bucketer=self.bucketer)
            self.ea = None
        elif algo == "ea":
            self.sgd = None
            self.ea = AllReduceEA(tree, tau, alpha)
            self.ea._one_time_init(self.flat)
        elif algo == "async":
            # AsyncEA client (examples/EASGD_client.lua:97-119): grads, then the
            # elastic sync every tau steps, then SGD with the pre-move grads
            from .parallel.async_ea import AsyncEA

            self.sgd = self.ea = None
            # (grad_comm_dtype="bf16" here: the delta push goes bf16, AsyncEA delta_wire)
            self.aea = async_ea or AsyncEA(tree, None, None, None, None, None, tree.numNodes - 1,
                                           tree.nodeIndex - 1, tau, alpha, delta_wire=grad_comm_dtype)
            self.aea._one_time_init(self.flat)
        else:
            raise ValueError(f"unknown algo {algo!r}")
        if backend == "torch" and bf16_shadow and callable(getattr(model, "attach_flat", None)):
            # convolutions read the bf16 shadow and write fp32 grads into the flat buffer
            model.attach_flat(self.flat, self.bucketer.mark_leaf_ready if self.bucketer is not None else None)
        self.executor = None
        if backend == "hip":
            from .models import make_executor

            self.executor = make_executor(model, self.flat, bucketer=self.bucketer if algo == "sgd" else None,
                                          max_batch=max_batch)
        # per-bucket SGD on the comm stream right after each bucket's all-reduce
        # (parallel/buckets.py set_early_update): only for executors whose
        # backward never reads a parameter once its bucket is complete.  Off by
        # default: inside the replayed hipGraph every fork/join edge between the
        # compute and comm streams stalled the compute stream by 5-15 us, so the
        # overlapped updates cost 0.378-0.401 vs 0.328-0.330 ms/step at N = 1
        # (profiles/r3_bucket_update_ab.txt)
        self.bucket_updates = False
        if (algo == "sgd" and getattr(self.executor, "bucket_updates_safe", False)
                and os.environ.get("DISTLEARN_BUCKET_UPDATE", "0") == "1"):
            self.bucket_updates = self.sgd.enable_bucket_updates(
                self.flat, self._lr_arg, momentum=momentum, weight_decay=weight_decay, momentum_buf=self.mom)
        # Whether the gradients go through a collective: AllReduceSGD at N > 1
        # (or at world 1 with the collectives forced through RCCL -- the
        # multi-node configuration rehearsed on one GPU, bench.py --nworld-path).
        # AllReduceEA all-reduces elastic deltas, never gradients.
        self.reduces_grads = algo == "sgd" and runs_collectives(tree.comm)
        # Gradients nobody all-reduces: the conv executor leaves the split-K
        # weight gradients of the layers whose slabs the update can read in
        # their slabs, and the fused SGD sums them itself (bitwise the same
        # update, two launches fewer per step).  DISTLEARN_DEFER_SLABS=0: off (A/B).
        # Gradients that are all-reduced: the slab sums ride the dgrad launches /
        # one merged reduce launch (executor fuse_slab_reduces; DISTLEARN_FUSE_REDUCE=0: off).
        self._slabs = None
        self._fused_reduce = None
        if (not self.reduces_grads and algo in ("sgd", "ea", "async") and not self.bucket_updates
                and self.grad_comm_dtype == "fp32"  # a bf16 wire copy would be cast from the stale fp32 grads
                and callable(getattr(self.executor, "defer_slab_reduce", None))
                and os.environ.get("DISTLEARN_DEFER_SLABS", "1") == "1"):
            self._slabs = self.executor.defer_slab_reduce() or None
        elif (self.reduces_grads and callable(getattr(self.executor, "fuse_slab_reduces", None))
              and os.environ.get("DISTLEARN_FUSE_REDUCE", "1") == "1"):
            self._fused_reduce = self.executor.fuse_slab_reduces() or None
        self._side = None
        self._arm_side_update()
        # Whether flat.grad holds this step's gradients after a step:
        # False while the one-node update sums split-K slabs itself (their
        # weights' flat.grad entries are never written) or a conv launch's side
        # job updates part of the parameters inside forward_backward -- gradient
        # readers (norm logging, clipping, hooks) then need DISTLEARN_DEFER_SLABS=0.
        self.grads_materialized = self._slabs is None and self._side is None
        # executor policy for the world > 1 overlap (select_policy): None until chosen
        self.policy: Optional[dict] = None
        self._policy_done = False
        self.graph = graph
        self._graph = None
        self._static = None
        self._multi = {}     # unroll -> (graph, loss) (run())
        self._seqs = {}      # id(graph) -> collectives recorded at its capture (DISTLEARN_DEBUG_SYNC)
        self.captures = 0    # hipGraph captures so far (none may happen in a timed region)
        self._eval_graphs = {}     # steps -> forward-only graph on _eval_loader (evaluate())
        self._eval_loader = None
        self.eval_captures = 0     # captures of those (``captures`` counts training graphs only)
        self.last_loss: Optional[torch.Tensor] = None
        self.steps = 0
        # callables hook(logits, labels) run INSIDE every step body, after the
        # backward (so they are captured into the step's hipGraphs): e.g. the
        # examples' every-sample training confusion matrix (one GPU kernel)
        self.step_hooks: list = []

    # ------------------------------------------------------------------ learning rate
    def _rate(self, t: int) -> float:
        """The schedule's value for update ``t``, rounded to fp32 once: the
        one value the eager kernel argument, the ring and ``lr`` all carry."""
        return as_fp32(self.lr_schedule(int(t)))

    def _lr_arg(self):
        """The rate the update of the step body being run takes: the host
        float, or -- a body captured under a schedule -- its ring slot (a
        1-element view the kernels read on the device at replay time)."""
        if self._cap_slot is not None and self._lr_ring is not None:
            return self._lr_ring[self._cap_slot:self._cap_slot + 1]
        return self.lr

    @contextlib.contextmanager
    def _ring_slot(self, i: int):
        """Capture a step body whose update reads ``ring[i]`` (no schedule:
        the host float, as ever)."""
        prev, self._cap_slot = self._cap_slot, (i if self._lr_ring is not None else None)
        try:
            yield
        finally:
            self._cap_slot = prev

    def _advance_lr(self, k: int = 1, ring: bool = False, advance: bool = True) -> None:
        """Schedule mode, before ``k`` updates run: ``ring`` -- the next ``k``
        rates go into the device ring on the current stream, right before the
        replay that reads them; ``advance`` -- count the updates and leave
        ``lr`` at the last rate used (a trial replay whose state is restored
        feeds the ring without counting)."""
        if self.lr_schedule is None:
            return
        vals = [self._rate(self.sched_step + i) for i in range(k)]
        if ring and self._lr_ring is not None:
            lr_ring_set_(self._lr_ring, 0, vals)
        if advance:
            self.sched_step += k
            self.lr = vals[-1]

    def set_lr(self, value: float) -> None:
        """Change the learning rate from now on.  With ``lr_schedule=`` the
        schedule becomes the constant ``value``.  Without one the rate is a
        kernel argument frozen into every captured hipGraph, so this raises
        once graphs exist (plain ``trainer.lr = v`` keeps its old meaning:
        it reaches eager steps and later captures only)."""
        if self.lr_schedule is not None:
            self.lr_schedule = constant(value)
            self.lr = as_fp32(value)
            return
        if self._graph is not None or self._multi:
            raise RuntimeError("set_lr: the captured hipGraphs hold the learning rate they were captured with; "
                               "construct the trainer with lr_schedule= (torch_distlearn_amd.schedules) to change "
                               "the rate of a graph run")
        self.lr = value

    def _agree_sched_step(self) -> None:
        """After a parameter synchronisation every node holds the winner's
        parameters (the node with the most steps): it takes the winner's
        place in the schedule too, or uneven epochs would leave the nodes on
        different rates for ever after.  One max on the control plane.  Not
        for AsyncEA (the server never joins; each client follows its own count)."""
        if self.lr_schedule is None or self.algo not in ("sgd", "ea") or self.tree.numNodes <= 1:
            return
        t = torch.tensor([self.sched_step], dtype=torch.int64)
        self.tree.comm.all_reduce_host(t, "max")
        self.sched_step = int(t[0])

    # ------------------------------------------------------------------
    def _forward_backward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        if self.executor is not None:
            return self.executor.forward_backward(x, y)
        self.model.train()
        fused = getattr(self.model, "forward_loss", None) if self._fused_loss_ok else None
        out = fused(x, y, compute_dtype=self.compute_dtype) if (fused is not None and x.is_cuda) else None
        if out is not None:  # the model computes its loss (and the head's backward) itself
            loss, logp = out
        else:
            logp = self.model(x, compute_dtype=self.compute_dtype)
            loss = self.loss_fn(logp, y)
        self._last_logp = logp.detach()
        loss.backward()
        return loss.detach()

    def _step_body(self, x: torch.Tensor, y: torch.Tensor, prep_next: bool = False,
                   local: bool = False) -> torch.Tensor:
        """The capturable part of a step: zero grads, forward, backward and
        the update (SGD: bucketed all-reduce + fused 1/n SGD; EA: the local
        SGD step -- the elastic round every tau steps runs after it; AsyncEA:
        the local SGD step only when ``local`` -- a step that syncs with the
        server runs its update after the sync, EASGD_client.lua:106-117).
        ``prep_next``: another step on the same DeviceLoader follows in the
        same graph; the update launch prepares it (executor next_prep)."""
        f = self.flat
        # zero grads, participation slot = 1 (this node contributes this round);
        # a native executor that overwrites every gradient sets the slot itself
        if not getattr(self.executor, "overwrites_grads", False):
            fill_(f.grad, 0.0, slot_value=1.0)
        loss = self._forward_backward(x, y)
        if self.step_hooks:
            labels = x.labels_out if hasattr(x, "gather_args") else y
            for h in self.step_hooks:
                h(self.last_logits(), labels)
        updates = self.algo in ("sgd", "ea") or (self.algo == "async" and local)
        nxt = None
        if (prep_next and updates and self._update_preps_next()
                and os.environ.get("DISTLEARN_PREP_NEXT", "1") == "1" and hasattr(self.executor, "next_prep")):
            nxt = self.executor.next_prep(x)
        if self.algo == "sgd":
            self.sgd.step(f, self._lr_arg(), momentum=self.momentum, weight_decay=self.weight_decay,
                          momentum_buf=self.mom, slabs=self._slabs, skip=self._side, next_prep=nxt)
        elif updates:
            self._local_update(nxt)
        if nxt is not None:
            self.executor.mark_prepared()  # its launch is enqueued: the next step skips its prep
        return loss

    def _update_preps_next(self) -> bool:
        """Whether the step's final update is ONE fused fp32 SGD launch that can
        also prepare the next step of an unrolled graph (flat_sgd_
        ``next_prep``): not per-bucket updates, not the bf16 gradient wire
        (its update reads the bf16 copy).  An AsyncEA client's local-step
        updates inside its unrolled graph carry the preparation too; a
        syncing step (update after syncClient, outside the graph) never does."""
        return (self.algo in ("sgd", "ea", "async") and not self.bucket_updates and self.grad_comm_dtype == "fp32"
                and (self._slabs is not None or self.reduces_grads or self.algo != "sgd"))

    def _local_update(self, next_prep=None) -> None:
        from .ops.flat import flat_sgd_

        flat_sgd_(self.flat, self._lr_arg(), slot=None, mom=self.mom, momentum=self.momentum,
                  weight_decay=self.weight_decay, slabs=self._slabs, skip=self._side, next_prep=next_prep)

    def step(self, x, y: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One training step on this node's mini-batch; returns the loss
        (a device tensor; no host synchronisation).  ``x`` is an NHWC batch
        with labels ``y``, or a :class:`~torch_distlearn_amd.data.DeviceLoader`
        (the native executor then gathers the batch on the device inside the
        step, so a captured graph needs no per-step host work)."""
        self.steps += 1
        loader = x if hasattr(x, "gather_args") else None
        if loader is not None and not getattr(self.executor, "takes_loader", False):
            x, y = loader.getBatch()
            x = x.to(self.compute_dtype)
            dev_loader = None
        else:
            dev_loader = loader
        # AsyncEA: a step that does not sync with the server runs its local
        # update in the step body; a syncing step updates after syncClient
        # (EASGD_client.lua:106-117).  The single-step graph is the syncing
        # step's body (run() replays the local steps as unrolled graphs).
        local = self.aea is not None and (self.aea.step + 1) % self.aea.tau != 0
        if not self.graph:
            self._advance_lr()
            loss = self._step_body(x, y, local=local)
        else:
            if self._graph is None:
                self._capture(x, y)
            if dev_loader is None:
                if x.data_ptr() != self._static[0].data_ptr():
                    self._static[0].copy_(x, non_blocking=True)
                if y.data_ptr() != self._static[1].data_ptr():
                    self._static[1].copy_(y, non_blocking=True)
            elif self._static[0] is not dev_loader:
                raise ValueError("the captured step is bound to another DeviceLoader")
            # (an AsyncEA client's graph holds no update: its eager _local_update
            # below takes the host float this leaves in self.lr)
            self._advance_lr(ring=True)
            self._replay(self._graph)
            self._track()
            if self.sgd is not None:
                # the captured body counted one step at capture time only
                self.sgd._count_step()
            loss = self._static[2]
        if self.ea is not None:
            # every tau steps: fused elastic kernel + one all-reduce (lua/AllReduceEA.lua:25-47)
            self.ea.averageParameters(self.flat)
        elif self.aea is not None:
            if local:  # no sync this step (AsyncEA.lua:49-59)
                self.aea.step += 1
                if self.graph:
                    self._local_update()
            else:
                self.aea.syncClient(self.flat)   # EASGD_client.lua:109
                self._local_update()             # :113-117 (pre-move grads)
        if loader is not None:
            loader.step_done()
        self.last_loss = loss
        return loss

    def run(self, loader, nsteps: int, unroll: int = 8) -> torch.Tensor:
        """``nsteps`` training steps on a :class:`DeviceLoader`; returns the
        last step's loss.  With the native executor, hipGraph capture and
        AllReduceSGD, up to ``unroll`` consecutive steps (forward, backward,
        bucketed all-reduce and update each) are captured into ONE graph, so
        the per-replay launch latency is paid once per graph: graphs of
        unroll, unroll/2, ... 2 steps are kept and the largest that fits the
        remaining steps is replayed (epoch boundaries included: the
        DeviceLoader holds the next epoch's order already), the single-step graph
        covers the rest.  Every step is still a complete step (the same
        kernels and collectives as :meth:`step`).

        AllReduceEA: the local-step graphs cover the steps between elastic
        rounds, and when a tau-step cycle starts on a step boundary ONE graph
        holds the tau local steps plus the elastic round (fused elastic kernel,
        delta all-reduce, center update: lua/AllReduceEA.lua:25-47); a round
        that falls elsewhere runs through :meth:`step`."""
        loss = None
        fast = self._unrolled(unroll) and getattr(self.executor, "takes_loader", False)
        if fast:
            # every graph this loop can replay is captured (and replayed once,
            # state restored) before the first step runs, whatever nsteps is: a
            # later call never captures (bench.py's timed region asserts that
            # through ``captures``)
            self.prepare(loader, unroll)
        while nsteps > 0:
            # a graph may run into the next epoch (its order is already in the
            # loader's two-epoch ring) but not past it.  (Replaying a small graph
            # first -- the device starts before the big graph's submission ends --
            # measured within noise or slower: the extra graph boundary costs
            # more, profiles/r6_replay_order_ab.txt.)
            left = 2 * loader.steps_per_epoch - loader._host_steps
            cap = min(nsteps, left)
            key = None
            if fast and self.ea is not None:
                phase = self.ea.step % self.ea.tau
                if phase == 0 and cap >= self.ea.tau and self._ea_key() in self._multi:
                    key = self._ea_key()
                cap = min(cap, self.ea.tau - 1 - phase)  # local steps before the round-triggering one
            elif fast and self.aea is not None:
                # the local steps before the next syncing one: one graph of all
                # tau - 1 of them when the cycle starts here, else the largest fitting
                phase = self.aea.step % self.aea.tau
                cap = min(cap, self.aea.tau - 1 - phase)
                if phase == 0 and cap == self.aea.tau - 1 and self._async_key() in self._multi:
                    key = self._async_key()
            if key is not None:
                k = key[1]
            else:
                k = max((u for u in self._multi if isinstance(u, int) and u <= cap), default=1) if fast else 1
            if k > 1 or (key is not None and k >= 1):
                g, loss = self._multi[key if key is not None else k]
                self._advance_lr(k, ring=True)
                self._replay(g)
                if self.ea is not None:
                    self.ea.step += k  # the graph ran k local steps (+ the round when key is set)
                elif self.aea is not None:
                    self.aea.step += k  # k local steps (updates inside the graph), no sync
                for _ in range(k):
                    if self.sgd is not None:
                        self.sgd._count_step()
                    loader.step_done()
                self.steps += k
                self._track()
                self.last_loss = loss
                nsteps -= k
            else:
                loss = self.step(loader)
                nsteps -= 1
        return loss

    def _unrolled(self, unroll: int) -> bool:
        return self.graph and self.algo in ("sgd", "ea", "async") and self.executor is not None and unroll > 1

    def _ea_key(self):
        return ("ea", self.ea.tau)

    def _async_key(self):
        return ("async", self.aea.tau - 1)

    @staticmethod
    def _unroll_sizes(unroll: int):
        sizes, u = [], 2
        while u < unroll:
            sizes.append(u)
            u *= 2
        return sizes + [unroll]

    def prepare(self, loader, unroll: int = 8) -> None:
        """Capture every hipGraph that :meth:`run` replays on ``loader`` (the
        single-step graph and the 2..``unroll``-step graphs), then replay each
        once with the training state saved and restored, so the first timed
        replay of a graph pays no one-time upload/instantiation cost.
        Idempotent; changes no training state."""
        if not self.graph:
            return
        self.select_policy(loader)
        if self._graph is None:
            self._capture(loader, None)
        if not self._unrolled(unroll):
            return
        new = [k for k in self._unroll_sizes(unroll) if k not in self._multi]
        if self.ea is not None and self.ea.tau > 1 and self._ea_key() not in self._multi:
            new.append(self._ea_key())
        if self.aea is not None and self.aea.tau > 1 and self._async_key() not in self._multi:
            new.append(self._async_key())
        for k in new:
            self._capture_multi(loader, k)
        if new:
            saved = self._snapshot(loader)
            # (trial replays: valid rates in the ring, the schedule's position untouched)
            self._advance_lr(ring=True, advance=False)
            self._replay(self._graph)
            for k in new:
                self._advance_lr(k[1] if isinstance(k, tuple) else k, ring=True, advance=False)
                self._replay(self._multi[k][0])
            self._restore(saved, loader)
            torch.cuda.current_stream().synchronize()

    def select_policy(self, loader, reps: int = 10) -> Optional[dict]:
        """Choose the executor's overlap policy on THIS machine, before any
        graph is captured (README "Compute / all-reduce co-residency").  With
        world > 1 the bucketed all-reduce runs beside the backward convs and
        RCCL's workgroups hold CUs; the candidates are the executor's
        ``policies()`` -- full-chip grids with 3-stage dgrads, wgrad grids
        that leave the channel cap of CUs free with 2- or 3-stage dgrads.  Each is
        captured as a one-step graph and replayed ``reps`` times, timed with
        HIP events, training state restored; every rank takes the policy
        whose slowest rank is fastest (:func:`agree_on_policy`).  Runs once;
        ``DISTLEARN_POLICY=<name>`` forces a candidate, one node keeps the
        executor default unless ``DISTLEARN_POLICY_SELECT=1``.  The choice
        and every timing lands in :attr:`policy` (bench.py's JSON config).

        With an RCCL communicator whose collectives run, the candidates are
        also crossed with the channel caps of
        :func:`~torch_distlearn_amd.parallel.comm.channel_cap_candidates`
        ("full@16", "reserve@32", ...: the communicator is rebuilt with each
        cap, ``reserve`` leaves that many CUs): more channels move a bucket
        faster, fewer leave more CUs to the backward -- the measured step
        decides."""
        ex = self.executor
        if self._policy_done or not self.graph or ex is None or not callable(getattr(ex, "policies", None)):
            return self.policy
        self._policy_done = True
        cands = self._policy_candidates()
        want = os.environ.get("DISTLEARN_POLICY", "auto")
        if want not in cands and "@" not in want:
            # a base policy name ("full" / "reserve") forces it at the communicator's current cap
            cap = getattr(self.tree.comm, "channel_cap", None)
            want = f"{want}@{cap}" if f"{want}@{cap}" in cands else want
        if want in cands:
            self._apply_candidate(*cands[want])
            self.policy = {"chosen": want, "how": "forced (DISTLEARN_POLICY)", **self._cap_record()}
            return self.policy
        # only a step whose gradient all-reduce overlaps the backward has a policy to
        # choose (AllReduceEA / AsyncEA clients: no collective beside the backward; an
        # AsyncEA server would never join the agreement collective)
        if (len(cands) < 2 or not self.reduces_grads
                or (self.tree.numNodes == 1 and os.environ.get("DISTLEARN_POLICY_SELECT", "0") != "1")):
            if len(cands) == 1:  # a single candidate (pinned policy knobs / channel cap): nothing to measure
                self._apply_candidate(*next(iter(cands.values())))
            return self.policy
        local = {}
        # caps outermost: the communicator is rebuilt once per cap; a second pass in
        # reverse order, each candidate keeping its faster pass, so the clock warm-up
        # of the first candidates does not favour the last ones (one GPU, no CU held:
        # one pass chose wreserve@32, timed last, in 3 of 3 runs although full ran
        # 0.5-1 % faster, profiles/r6_nworld_policy_hold.txt)
        order = sorted(cands.items(), key=lambda it: (it[1][1] or 0, it[0]))
        for name, (kw, cap) in order + order[::-1]:
            self._apply_candidate(kw, cap)
            ms = self._time_step_graph(loader, reps)
            local[name] = min(ms, local.get(name, ms))
        name, table = agree_on_policy(self.tree.comm, local)
        self._apply_candidate(*cands[name])
        self.policy = {"chosen": name, "ms_per_step": table,
                       "how": f"measured (2 passes x {reps} graph replays per policy)",
                       "candidates": {n: dict(kw, **({"channel_cap": cap} if cap else {}))
                                      for n, (kw, cap) in cands.items()}, **self._cap_record()}
        return self.policy

    def _policy_candidates(self) -> dict:
        """name -> (executor policy kwargs, channel cap or None)."""
        from .parallel.comm import agree_channel_caps, channel_cap_candidates

        base = self.executor.policies()
        comm = self.tree.comm
        caps = [None]
        if base and callable(getattr(comm, "set_channel_cap", None)) and runs_collectives(comm):
            caps = agree_channel_caps(comm, channel_cap_candidates())
        out = {}
        for cap in caps:
            for p, kw in base.items():
                kw = dict(kw)
                if cap is not None and kw.get("cu_reserve", 0) > 0:
                    kw["cu_reserve"] = int(cap)  # the reserve policy leaves the cap's CUs free
                out[p if len(caps) == 1 else f"{p}@{cap}"] = (kw, cap)
        return out

    def _apply_candidate(self, kw: dict, cap) -> None:
        comm = self.tree.comm
        if cap is not None and cap != getattr(comm, "channel_cap", None):
            # graphs holding the old communicator's collectives go first
            self._graph, self._static = None, None
            self._multi = {}
            self._drop_eval_graphs()
            comm.set_channel_cap(cap)
        self._set_policy(kw)

    def _cap_record(self) -> dict:
        cap = getattr(self.tree.comm, "channel_cap", None)
        return {"channel_cap": cap} if cap else {}

    def _arm_side_update(self) -> None:
        """One node, slabs deferred: the update of the last blocks' parameters
        rides the dgrad launch of the block that produces them last (extra
        workgroups on the CUs that conv leaves free, models/cifar_hip.py
        side_update); the final update skips that range.
        DISTLEARN_SIDE_SGD=0: off (A/B)."""
        self._side = None
        ex = self.executor
        if (self._slabs is None or os.environ.get("DISTLEARN_SIDE_SGD", "1") != "1"
                or self.algo == "async"  # a syncing step's update must follow the elastic move
                or not callable(getattr(ex, "side_update", None))):
            return
        rng = ex.side_update(self._lr_arg, self.momentum, self.weight_decay, self.mom,
                             self.flat.slot if self.algo == "sgd" else None)
        self._side = rng

    def _set_policy(self, kw: dict) -> None:
        """Switch the executor's policy.  It re-allocates the workspaces, so
        every graph captured before would replay on freed buffers: they are
        dropped, and the slab plans are redone for the new slabs."""
        self.executor.set_policy(**kw)
        self._graph, self._static = None, None
        self._multi = {}
        self._drop_eval_graphs()  # they would replay on the freed workspaces too
        if self._slabs is not None:  # the re-planned workspaces have new slabs
            self._slabs = self.executor.defer_slab_reduce() or None
            self._arm_side_update()
        if self._fused_reduce is not None:
            self._fused_reduce = self.executor.fuse_slab_reduces() or None
        self.grads_materialized = self._slabs is None and self._side is None

    def _time_step_graph(self, loader, reps: int) -> float:
        """ms per replay of a freshly captured one-step graph (state restored;
        the graph is dropped)."""
        saved = self._snapshot(loader)
        self._capture(loader, None)
        g = self._graph
        self._advance_lr(ring=True, advance=False)  # every replay below reads the same valid rate
        self._replay(g)
        torch.cuda.synchronize()
        self.tree.comm.barrier()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            self._replay(g)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        self._track()
        self._restore(saved, loader)
        torch.cuda.synchronize()
        self._graph, self._static = None, None
        del g
        return ms

    def _snapshot(self, loader=None):
        return (self.flat.data.clone(), None if self.mom is None else self.mom.clone(),
                [b.detach().clone() for b in self.model.buffers()],
                loader.ctr.clone() if hasattr(loader, "gather_args") else None,
                None if self.ea is None or self.ea.center is None else self.ea.center.clone())

    def _restore(self, saved, loader=None) -> None:
        data, mom, bufs, ctr, center = saved
        if center is not None:
            self.ea.center.copy_(center)
        self.flat.data.copy_(data)
        self.flat.refresh_shadow()
        if mom is not None:
            self.mom.copy_(mom)
        for b, v in zip(self.model.buffers(), bufs):
            b.detach().copy_(v)
        if ctr is not None:
            loader.ctr.copy_(ctr)

    @contextlib.contextmanager
    def _seq_record(self, g):
        """Record the collectives a capture of ``g`` issues (every replay
        counts them: Communicator.seq_replay, DISTLEARN_DEBUG_SYNC)."""
        rec_fn = getattr(self.tree.comm, "seq_record", None)
        if rec_fn is None:
            yield
            return
        with rec_fn() as rec:
            yield
        # keyed by id (no reference: a dropped graph must be freed); every graph
        # this engine replays was recorded here, so a reused id is overwritten
        self._seqs[id(g)] = rec

    def _replay(self, g) -> None:
        g.replay()
        rec = self._seqs.get(id(g))
        if rec:
            self.tree.comm.seq_replay(rec)

    def _track(self) -> None:
        """Let the communicator's watchdog time the collectives of the work
        just enqueued (a replayed graph's collectives are invisible to it)."""
        track = getattr(self.tree.comm, "track", None)
        if track is not None and self.device.type == "cuda":
            track()

    def _capture_multi(self, loader, k):
        """Capture k consecutive step bodies on ``loader`` into one graph
        (capture records kernels without running them; replay counts the steps).
        k = ("ea", tau): tau local steps followed by the AllReduceEA elastic round;
        ("async", n) or an int k for an AsyncEA client: k local steps (each with
        its local update), no sync."""
        self.captures += 1
        ea_round = isinstance(k, tuple) and k[0] == "ea"
        n = k[1] if isinstance(k, tuple) else k
        if self.lr_schedule is not None and n > LR_RING:
            raise ValueError(f"lr_schedule: a captured graph of {n} steps does not fit the device ring of "
                             f"{LR_RING} learning rates (tau above {LR_RING}: use a smaller tau or graph=False)")
        local = self.aea is not None
        g = torch.cuda.CUDAGraph()
        with _capturing(self.tree.comm), self._seq_record(g), torch.cuda.graph(g, capture_error_mode=_CAPTURE_MODE):
            for j in range(n):
                with self._ring_slot(j):
                    loss = self._step_body(loader, None, prep_next=j + 1 < n, local=local)
            if ea_round:
                self.ea.elastic_round()
        if self.sgd is not None:
            self.sgd.stepsPerNode[self.tree.nodeIndex - 1] -= n  # capture counted n (not executed)
        self._multi[k] = (g, loss)
        return self._multi[k]

    def comm_profile(self, batch, steps: int = 6, replay: bool = False) -> dict:
        """Measure the bucketed all-reduce with HIP events: communication time,
        the part of it exposed after the backward, and the overlap fraction
        (utils/profiling.comm_summary), over ``steps`` training steps
        (``batch``: a DeviceLoader, or a callable i -> (x, y)).  Collective:
        every rank calls it at the same point; the training state is restored
        afterwards, so the measured run continues as if this had not been
        called.

        ``replay=True`` (a graph trainer on a DeviceLoader): the timings are
        device-timestamp kernel nodes INSIDE a captured one-step graph, read
        after each of ``steps`` replays -- the schedule the timed loop runs,
        fork / join edges of the replayed graph included (VERDICT r5 weak #5;
        HIP refuses external event-record nodes in a capture).  Otherwise (or
        if the capture fails) eager steps; the result's ``source`` says which."""
        from .utils.profiling import comm_summary

        if self.bucketer is None or self.device.type != "cuda" or self.algo != "sgd":
            return {}
        loader = batch if hasattr(batch, "gather_args") else None
        err = None
        if replay and self.graph and loader is not None:
            try:
                return self._comm_profile_replay(loader, steps)
            except RuntimeError as e:
                err = str(e)[:200]
                torch.cuda.synchronize()
        out = self._comm_profile_eager(batch, loader, steps)
        if out:
            out["source"] = "eager steps"
            if err is not None:
                out["replay_error"] = err
        return out

    def _comm_profile_replay(self, loader, steps: int) -> dict:
        from .utils.profiling import comm_summary

        bk = self.bucketer
        saved = self._snapshot(loader)
        g = torch.cuda.CUDAGraph()
        bk.start_capture_profile()
        try:
            with _capturing(self.tree.comm), self._seq_record(g), \
                    torch.cuda.graph(g, capture_error_mode=_CAPTURE_MODE), self._ring_slot(0):
                self._step_body(loader, None)
        finally:
            recs = bk.stop_capture_profile()
        self.sgd.stepsPerNode[self.tree.nodeIndex - 1] -= 1  # the capture counted a step (not executed)
        runs = []
        self._advance_lr(ring=True, advance=False)  # the replays read a valid rate; the schedule stays put
        try:
            for i in range(steps + 1):  # the first replay is a warm-up
                self._replay(g)
                torch.cuda.synchronize()
                if i:
                    runs.append(comm_summary(recs, self.tree.numNodes))
        finally:
            self._track()
            self._restore(saved, loader)
            torch.cuda.synchronize()
            del g
        if not runs or not runs[0]:
            return {}
        out = dict(runs[0])
        for k in ("comm_ms", "exposed_comm_ms", "overlap_fraction", "busbw_GBps"):
            out[k] = round(sum(r[k] for r in runs) / len(runs), 4)
        out["steps"] = len(runs)
        out["source"] = "graph replays (device-timestamp nodes in a captured one-step graph)"
        return out

    def _comm_profile_eager(self, batch, loader, steps: int) -> dict:
        from .utils.profiling import comm_summary

        saved = self._snapshot(loader)
        self.bucketer.profile = []
        try:
            for i in range(steps + 1):  # the first step is a warm-up
                x, y = (loader, None) if loader is not None else batch(i)
                self._step_body(x, y)
                if i == 0:
                    self.bucketer.profile.clear()
            out = comm_summary(self.bucketer.profile, self.tree.numNodes)
        finally:
            self.bucketer.profile = None
        self.sgd.stepsPerNode[self.tree.nodeIndex - 1] -= steps + 1
        self._restore(saved, loader)
        return out

    def static_inputs(self):
        """The graph's input buffers (after the first step): a data loader
        that writes batches straight into them skips the per-step copy."""
        return None if self._static is None else self._static[:2]

    def _capture(self, x, y):
        self.captures += 1
        dev_loader = hasattr(x, "gather_args")
        sx, sy = (x, None) if dev_loader else (x.clone(), y.clone())
        # warm up on a side stream (allocations, autotuning), as torch.cuda.graphs requires;
        # everything the warm-up steps change is restored afterwards
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        saved = self._snapshot(x)
        with torch.cuda.stream(s):
            for _ in range(2):
                self._step_body(sx, sy)
        torch.cuda.current_stream().wait_stream(s)
        self._restore(saved, x)
        g = torch.cuda.CUDAGraph()
        with _capturing(self.tree.comm), self._seq_record(g), torch.cuda.graph(g, capture_error_mode=_CAPTURE_MODE), \
                self._ring_slot(0):
            loss = self._step_body(sx, sy)
        if self.sgd is not None:
            # the warm-up + capture bodies counted steps; undo (replay() counts itself)
            self.sgd.stepsPerNode[self.tree.nodeIndex - 1] -= 3
        self._restore(saved, x)
        self._graph, self._static = g, (sx, sy, loss)

    # ------------------------------------------------------------------ evaluation
    def _drop_eval_graphs(self) -> None:
        self._eval_graphs, self._eval_loader = {}, None

    def _eval_native(self) -> bool:
        """Whether evaluation runs on the executor's device path (eval_step)."""
        return callable(getattr(self.executor, "eval_step", None))

    def _eval_sizes(self, unroll: int):
        return sorted(set(self._unroll_sizes(max(1, int(unroll)))) | {1})

    def prepare_eval(self, loader, unroll: int = 16) -> None:
        """Capture the forward-only hipGraphs :meth:`evaluate` replays on
        ``loader`` (a :class:`~torch_distlearn_amd.data.DeviceEvalLoader`):
        ``_unroll_sizes(unroll)`` and 1 evaluation steps each, single-stream,
        no collective.  Idempotent; a no-op off the native graph path.
        Changes no training state; leaves ``loader`` rewound."""
        if not (self.graph and self._eval_native()):
            return
        if self._eval_loader is not loader:
            self._drop_eval_graphs()
            self._eval_loader = loader
        new = [k for k in self._eval_sizes(unroll) if k not in self._eval_graphs]
        if not new:
            return
        ex = self.executor
        # a training graph never ends on a step that prepared the next one (prep_next
        # applies inside a graph only), so the input buffers are free between two runs
        assert not getattr(ex, "_prepared", False), "evaluation inside a prepared-ahead training step"
        # one eager step first: nothing is loaded or allocated for the first time inside a capture
        loader.reset()
        ex.eval_begin()
        ex.eval_step(loader)
        for k in new:
            g = torch.cuda.CUDAGraph()
            with _capturing(self.tree.comm), torch.cuda.graph(g, capture_error_mode=_CAPTURE_MODE):
                for _ in range(k):
                    ex.eval_step(loader)
            self.eval_captures += 1
            self._eval_graphs[k] = g
        loader.reset()

    @torch.no_grad()
    def evaluate(self, loader, conf=None, unroll: int = 16) -> dict:
        """One pass over ``loader``'s partition, every sample exactly once (the
        padded rows of the last batch do not count): the reference's per-epoch
        test loop (examples/cifar10.lua:213-231).  Returns ``{"mat": int64
        [C, C] confusion counts, "count": samples evaluated (host int),
        "loss_sum": summed negative log-likelihood, "pred": [count] predicted
        classes, "nll": [count] per-sample losses}`` as device tensors; nothing
        waits for the device.  ``conf`` (a ConfusionMatrix): ``conf.mat +=
        mat`` (the caller all-reduces it).  Changes no training state.

        Native executor: the loader's device step counter selects each batch,
        the evaluation head writes the results in place; ``graph=True``
        replays forward-only graphs of up to ``unroll`` steps (captured on
        first use, or ahead of time by :meth:`prepare_eval`), else the same
        steps run eagerly.  Any other backend: a loop over the partition in
        order with :meth:`predict`."""
        if not hasattr(loader, "n_valid"):
            raise TypeError("evaluate needs a DeviceEvalLoader")
        n = loader.n_valid
        if self._eval_native():
            ex = self.executor
            if self.graph:
                self.prepare_eval(loader, unroll)
            assert not getattr(ex, "_prepared", False), "evaluation inside a prepared-ahead training step"
            loader.reset()
            ex.eval_begin()
            left = loader.steps
            while left > 0:
                k = max((u for u in self._eval_graphs if u <= left), default=0) if self.graph else 0
                if k:
                    self._eval_graphs[k].replay()
                else:
                    ex.eval_step(loader)
                    k = 1
                left -= k
            mat, pred, nll = loader.mat.clone(), loader.pred[:n].clone(), loader.nll[:n].clone()
        else:
            preds, nlls = [], []
            for k in range(loader.steps):
                x, y, valid = loader.host_batch(k)
                logp = self.predict(x.to(self.compute_dtype)).float()[:valid]
                preds.append(logp.argmax(dim=1).to(torch.int32))
                nlls.append(-logp.gather(1, y[:valid].unsqueeze(1)).squeeze(1))
            pred, nll = torch.cat(preds), torch.cat(nlls)
            nc = loader.mat.shape[0]
            mat = torch.zeros_like(loader.mat)
            idx = loader.ds.labels[loader.lo:loader.hi] * nc + pred.to(torch.int64)
            mat.view(-1).index_add_(0, idx, torch.ones_like(idx))
        if conf is not None:
            if conf.mat.device != mat.device:
                conf.mat = conf.mat.to(mat.device)
            conf.mat += mat
        return {"mat": mat, "count": n, "loss_sum": nll.sum(), "pred": pred, "nll": nll}

    # ------------------------------------------------------------------ epoch end
    def synchronize(self) -> None:
        """Epoch-end synchronisation (examples/cifar10.lua:208 /
        examples/mnist-ea.lua:121).  AsyncEA clients have none."""
        if self.algo == "sgd":
            self.sgd.synchronizeParameters(self.flat)
        elif self.algo == "ea":
            self.ea.synchronizeCenter(self.flat)
        self._agree_sched_step()

    def synchronize_parameters(self) -> None:
        """Initial synchronisation (AsyncEA: receive the server's center,
        AsyncEA.lua:64-78)."""
        if self.algo == "sgd":
            self.sgd.synchronizeParameters(self.flat)
        elif self.algo == "ea":
            self.ea.synchronizeParameters(self.flat)
        else:
            self.aea.initClient(self.flat)
        self._agree_sched_step()

    def finish(self) -> None:
        """AsyncEA client: tell the server this client is done."""
        if self.aea is not None:
            self.aea.finishClient()

    def last_logits(self) -> torch.Tensor:
        """Log-probabilities of the last training batch (train-mode forward),
        what the reference feeds its training confusion matrix
        (examples/cifar10.lua:194-196)."""
        if self.executor is not None:
            return self.executor.last_logits()
        return self._last_logp

    @torch.no_grad()
    def predict(self, x: torch.Tensor, batch_stats: bool = False) -> torch.Tensor:
        """Log-probabilities of ``x``: eval-mode BatchNorm (running
        statistics), or ``batch_stats=True`` -- the batch's own statistics,
        running statistics untouched (the reference AsyncEA tester's mode)."""
        if self.executor is not None:
            return self.executor.predict(x, batch_stats=batch_stats)
        return predict_module(self.model, x, self.compute_dtype, batch_stats)
