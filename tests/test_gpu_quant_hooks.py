"""The uint8 quantization kernels and hooks on the GPU against torch's own fp32 functions on CPU tensors, bit for bit."""
import pytest
import torch.distributed as dist

from distributed_training_amd.comm import destroy_communicators
from tests._dist_util import free_port, init_pg
from tests._quant_ref import NS, check_dequant_mean, check_nonfinite, check_quant, run_hooks, spawn_ws2

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bs", [0, 16, 272, 512, 4096])  # 0: the per-tensor form
@pytest.mark.parametrize("n", NS)
def test_quantize(cuda_device, n, bs):
    check_quant(cuda_device, n, bs)
    if n == 4 * 512 + 5:
        check_quant(cuda_device, n, bs, misaligned=True)


@pytest.mark.parametrize("ws", [1, 2, 3, 8])  # 3: a division, not a multiplication by 1 / ws
def test_dequant_mean(cuda_device, ws):
    check_dequant_mean(cuda_device, ws)


def test_nonfinite(cuda_device):
    check_nonfinite(cuda_device)


def test_hooks_ws1_rccl(cuda_device):
    owned = not dist.is_initialized()
    if owned:
        init_pg("nccl", 0, 1, free_port())
    try:
        if dist.get_backend() != "nccl":
            pytest.skip("another module left a non-RCCL default group")
        run_hooks(0, 1, cuda_device)
    finally:
        if owned:
            destroy_communicators()
            dist.destroy_process_group()


def test_hooks_ws2_one_gpu_gloo(cuda_device):
    spawn_ws2(run_hooks, cuda_device)
