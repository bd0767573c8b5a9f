"""Learning-rate schedules.

A schedule is any callable ``t -> float``; ``t`` is the 0-based number of
updates already applied (the first update of a run uses ``schedule(0)``).
:class:`~torch_distlearn_amd.engine.DataParallelTrainer` takes one as
``lr_schedule=``: eager steps pass the value as the update kernel's argument,
captured hipGraphs read it from a device ring the trainer fills before every
replay, so the rate follows the schedule in every mode.

A value is computed in Python double and rounded to fp32 exactly once
(:func:`as_fp32`); that fp32 value is what every path uses -- the eager kernel
argument, the device ring and ``trainer.lr`` -- so a graph run and an eager
run of the same schedule apply the same rates bit for bit.

Stock schedules (each with an optional linear warm-up):

* ``constant(lr)``
* ``step_decay(lr, milestones, gamma)``: ``lr * gamma ** #{m in milestones: m <= t}``
* ``cosine(lr, total_steps, floor)``:
  ``floor + (lr - floor) * (1 + cos(pi * t / total_steps)) / 2``, ``floor`` from ``total_steps`` on

Warm-up (``warmup_steps=w``, ``warmup_from=a``): for ``t < w`` the value is
``a + (base(t) - a) * (t + 1) / w`` -- update ``w - 1`` is the first at the
full rate, the companion of all-reduce SGD with a scaled batch.
"""
from __future__ import annotations

import math
import struct
from typing import Callable, Iterable, Sequence

Schedule = Callable[[int], float]


def as_fp32(x: float) -> float:
    """``x`` rounded to the nearest fp32 (returned as a Python float)."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def _with_warmup(base: Schedule, warmup_steps: int, warmup_from: float) -> Schedule:
    w, a = int(warmup_steps), float(warmup_from)
    if w < 0:
        raise ValueError("warmup_steps must be >= 0")

    def schedule(t: int) -> float:
        t = int(t)
        if t < 0:
            raise ValueError("schedule: t is the number of updates already applied (>= 0)")
        v = float(base(t))
        if t < w:
            v = a + (v - a) * (t + 1) / w
        return as_fp32(v)

    return schedule


def constant(lr: float, warmup_steps: int = 0, warmup_from: float = 0.0) -> Schedule:
    lr = float(lr)
    return _with_warmup(lambda t: lr, warmup_steps, warmup_from)


def step_decay(lr: float, milestones: Iterable[int], gamma: float = 0.1, warmup_steps: int = 0,
               warmup_from: float = 0.0) -> Schedule:
    """``lr`` times ``gamma`` for every milestone already reached (``m <= t``)."""
    lr, gamma = float(lr), float(gamma)
    ms: Sequence[int] = sorted(int(m) for m in milestones)
    return _with_warmup(lambda t: lr * gamma ** sum(1 for m in ms if m <= t), warmup_steps, warmup_from)


def cosine(lr: float, total_steps: int, floor: float = 0.0, warmup_steps: int = 0,
           warmup_from: float = 0.0) -> Schedule:
    """Half a cosine from ``lr`` at ``t = 0`` down to ``floor`` at ``total_steps`` (and after)."""
    lr, floor, total = float(lr), float(floor), int(total_steps)
    if total < 1:
        raise ValueError("cosine: total_steps must be >= 1")

    def base(t: int) -> float:
        if t >= total:
            return floor
        return floor + 0.5 * (lr - floor) * (1.0 + math.cos(math.pi * t / total))

    return _with_warmup(base, warmup_steps, warmup_from)


def from_options(opt, lr: float) -> Schedule | None:
    """The schedule the launcher flags describe (launch.add_schedule_flags),
    or None for the defaults: today's constant rate, no schedule object."""
    kind = getattr(opt, "lrSchedule", "constant")
    warm = int(getattr(opt, "warmupSteps", 0) or 0)
    if kind == "constant":
        return constant(lr, warmup_steps=warm) if warm > 0 else None
    if kind == "step":
        ms = [int(m) for m in str(getattr(opt, "lrMilestones", "") or "").split(",") if m.strip()]
        return step_decay(lr, ms, float(getattr(opt, "lrDecay", 0.1)), warmup_steps=warm)
    if kind == "cosine":
        total = int(getattr(opt, "totalSteps", 0) or 0)
        if total < 1:
            raise ValueError("--lrSchedule cosine needs --totalSteps")
        return cosine(lr, total, warmup_steps=warm)
    raise ValueError(f"unknown --lrSchedule {kind!r}")
