"""FusedCAME through the host backend: three steps against the fp64 restatement, exact first
statistics on integer grads, run-to-run bit identity, and the constructor's validation."""
import pytest
import torch

import distributed_training_amd as D
from tests import _came_common as C


@pytest.mark.parametrize("weight_decay,clip_threshold,lr", C.STEP_CASES)
def test_three_steps_against_fp64(weight_decay, clip_threshold, lr):
    C.check_three_steps("cpu", weight_decay, clip_threshold, lr)


def test_exact_first_statistics():
    C.check_exact_stats("cpu")


def test_two_runs_are_bit_identical():
    a, b = C.final_state("cpu"), C.final_state("cpu")
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kw", [dict(), dict(lr=0.0), dict(lr=1e-3, betas=(0.9, 1.5, 0.9999))])
def test_validation(kw):
    with pytest.raises(ValueError, match="FusedCAME"):
        D.FusedCAME([torch.nn.Parameter(torch.zeros(3))], **kw)
