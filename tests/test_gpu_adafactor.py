"""FusedAdafactor on the GPU: exact factor sums on integer grads (any tile-edge, stride, pitch
or fold mistake is a wrong value), three steps against torch.optim.Adafactor in fp64 on the
CPU, and bit-identical results run to run."""
import pytest
import torch

from tests import _adafactor_common as C
from tests.test_adafactor_cpu import STEP_CASES

pytestmark = pytest.mark.gpu


def test_exact_sums(cuda_device):
    C.check_exact_sums(cuda_device)


@pytest.mark.parametrize("weight_decay,maximize,d,lr", STEP_CASES)
def test_three_steps_against_fp64(cuda_device, weight_decay, maximize, d, lr):
    C.check_three_steps(cuda_device, weight_decay, maximize, d, lr)


def test_two_runs_are_bit_identical(cuda_device):
    a, b = C.final_state(cuda_device), C.final_state(cuda_device)
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
