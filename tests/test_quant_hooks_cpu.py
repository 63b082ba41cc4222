"""The uint8 quantization hooks without a GPU, bit for bit: the host kernels against torch's fp32 functions, and
both hooks over gloo on CPU buckets (world size 2) against torch's own hooks on a clone of the bucket."""
import functools
import types

import pytest
import torch
import torch.distributed as dist
from torch.distributed.algorithms.ddp_comm_hooks import quantization_hooks as TQ

from tests._quant_ref import NS, check_dequant_mean, check_nonfinite, check_quant, planted, spawn_ws2

CPU = torch.device("cpu")


@pytest.mark.parametrize("bs", [0, 16, 512, 4096])
@pytest.mark.parametrize("n", NS)
def test_host_quantize(n, bs):
    check_quant(CPU, n, bs, misaligned=n == 513)


@pytest.mark.parametrize("ws", [1, 3])
def test_host_dequant_mean_and_nonfinite(ws):
    check_dequant_mean(CPU, ws)
    check_nonfinite(CPU)


def _all_gather_as_nccl(outs, t, group=None, async_op=True):
    # torch's hooks index the future as [one tensor of all ranks' outputs]; gloo's holds the list: stack it
    fut = dist.all_gather(outs, t, group=group, async_op=True).get_future().then(lambda _: [torch.stack(outs)])
    return types.SimpleNamespace(get_future=lambda: fut)


def _against_torchs_hooks(rank, ws, dev):
    import distributed_training_amd as D

    TQ.dist = types.SimpleNamespace(group=dist.group, get_rank=dist.get_rank, all_gather=_all_gather_as_nccl)
    pairs = [(D.quantization_pertensor_hook, TQ.quantization_pertensor_hook),
             (D.quantization_perchannel_hook, TQ.quantization_perchannel_hook),
             (functools.partial(D.quantization_perchannel_hook, bucket_size=128),
              functools.partial(TQ.quantization_perchannel_hook, bucket_size=128))]
    for n in (5, 1024, 70001):  # 1024: torch pads a whole zero channel, which is not sent here
        for k, (ours, theirs) in enumerate(pairs):
            x = planted(n, 128, seed=1 + rank).clone()
            want = theirs(None, D.GradBucket(k, x.clone(), [], [], True)).wait()
            bucket = D.GradBucket(k, x, [], [], True)
            for _ in range(2):  # the second call reuses the cached launches and buffers
                x.copy_(planted(n, 128, seed=1 + rank))
                got = ours(None, bucket).wait()
                assert got is bucket.buffer() and torch.equal(got, want), (n, k)


def test_hooks_ws2_gloo_cpu_equal_torchs():
    spawn_ws2(_against_torchs_hooks, CPU)


def test_limits():
    import distributed_training_amd as D

    with pytest.raises(ValueError, match="fp32 bucket"):
        D.quantization_pertensor_hook(None, D.GradBucket(0, torch.zeros(8, dtype=torch.bfloat16), [], [], True))
    for bad in (0, 8, 24, 4112):
        with pytest.raises(ValueError, match="multiple of 16"):
            D.quantization_perchannel_hook(None, D.GradBucket(0, torch.zeros(8), [], [], True), bucket_size=bad)
