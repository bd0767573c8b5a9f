"""The per-call values of the native module -- a conv launch's SideJob and the
update launch's NextPrep (host code only: no GPU needed): every argument check
runs when the value is built, and the armed-global protocol they replace is gone."""
import pytest
import torch

P = 0x10000  # a 16-byte aligned stand-in for a device pointer: the builders never dereference


@pytest.fixture(scope="module")
def C():
    from torch_distlearn_amd import _native

    return _native.native()


def _sgd_job(C, p16=P, lo=400, hi=2800, k=1):
    offs = [1200 + 256 * j for j in range(k)]
    return C.side_sgd_job(P, P, 0, p16, P, 0.1, 0.9, 1e-4, lo, hi, offs, [256] * k, [P] * k, [5] * k, 0)


def _next_prep(C, pack_off=64):
    return C.next_prep(P, P, P, P, P, 1024, 128, 3, [0.5] * 3, [0.25] * 3, P, 4, 32, 32, 2, [P], [64], P, -5, pack_off,
                       64 * 25 * 3)


@pytest.mark.parametrize("name", ["set_conv_side_sgd", "set_conv_side_reduce", "arm_sgd_next_prep",
                                  "sgd_next_prep_armed", "disarm_sgd_next_prep", "set_sgd_trim", "take_side_job"])
def test_armed_protocol_is_gone(C, name):
    assert not hasattr(C, name)


def test_valid_values_build(C):
    assert type(_sgd_job(C)).__name__ == "SideJob"
    assert type(_sgd_job(C, k=4)).__name__ == "SideJob"
    assert type(C.side_reduce_job(P, 1200, 1456, [1200], [256], [P], [5], 0)).__name__ == "SideJob"
    assert type(_next_prep(C)).__name__ == "NextPrep"


def test_side_sgd_job_needs_the_shadow(C):
    with pytest.raises(RuntimeError, match="shadow"):
        _sgd_job(C, p16=0)


def test_side_sgd_job_unaligned_range(C):
    with pytest.raises(RuntimeError, match="aligned"):
        _sgd_job(C, lo=402)


def test_side_sgd_job_five_ranges(C):
    with pytest.raises(RuntimeError, match="up to 4"):
        _sgd_job(C, k=5)


def test_side_reduce_job_without_a_range(C):
    with pytest.raises(RuntimeError, match="no slab range"):
        C.side_reduce_job(P, 1200, 1456, [], [], [], [], 0)


def test_next_prep_unaligned_pack_range(C):
    with pytest.raises(RuntimeError, match="aligned"):
        _next_prep(C, pack_off=66)


def test_sgd_update_on_cpu_cannot_carry_next_prep(C):
    from torch_distlearn_amd.ops.flat import sgd_update_

    p, g = torch.ones(8), torch.ones(8)
    with pytest.raises(ValueError, match="fp32 gradient on the GPU"):
        sgd_update_(p, g, 0.1, next_prep=_next_prep(C))
    assert torch.equal(p, torch.ones(8))


@pytest.mark.parametrize("skip", [(0, 12), (304, 312), (0, 1200)])
def test_skip_over_the_slab_tail_is_rejected(C, skip):
    """The tail blocks do not consult the skip range, so the host refuses a
    skip that overlaps the tail before it launches anything."""
    with pytest.raises(RuntimeError, match="skip overlaps the tail"):
        C.sgd_update_slabs(P, P, 0, 0, 0, 0.1, 0.0, 0.0, 1200, [], [], [], [], [8, 300, 5, 4, 25, 8, 3], P,
                           skip[0], skip[1], 0)
