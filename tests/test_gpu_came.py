"""FusedCAME on the GPU: three steps against the fp64 restatement on the CPU, exact first
statistics on integer grads (any tile-edge, stride, pitch or fold mistake is a wrong value), and
bit-identical results run to run."""
import pytest
import torch

from tests import _came_common as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("weight_decay,clip_threshold,lr", C.STEP_CASES)
def test_three_steps_against_fp64(cuda_device, weight_decay, clip_threshold, lr):
    C.check_three_steps(cuda_device, weight_decay, clip_threshold, lr)


def test_exact_first_statistics(cuda_device):
    C.check_exact_stats(cuda_device)


def test_two_runs_are_bit_identical(cuda_device):
    a, b = C.final_state(cuda_device), C.final_state(cuda_device)
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
