"""The ReLU mask as bits, through fused_bn: GSYNC_BN_MASK=1 (the default) against GSYNC_BN_MASK=0.

The mask-writing forward tails and the bits-reading backward passes replace kernels that are bit-identical
to them (tests/test_gpu_bn_mask_kernels.py), and MIOpen's BatchNorm forward is repeatable, so everything
here is compared with torch.equal on bit patterns: the output, the running statistics, dx, grad_weight,
grad_bias and the identity gradient of bn_relu, bn_add_relu, bn_add_relu with fork=True (both halves used,
one half used) and bn_relu_pool; one micro_resnet step (loss, every parameter gradient, every buffer); and a
capture of forward + backward replays equal to eager.  last_path is "fused" throughout.
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF16 = torch.bfloat16

SHAPES = [(2, 8, 1, 1), (3, 8, 7, 7), (2, 24, 5, 3), (2, 64, 56, 56), (4, 2048, 7, 7)]
STEM_SHAPES = [(2, 8, 9, 5), (2, 64, 16, 16)]
_id = lambda v: v if isinstance(v, str) else "x".join(map(str, v))  # noqa: E731


def _bn(C, dev, seed=0):
    gen = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5, generator=gen)
        bn.bias.uniform_(-0.3, 0.3, generator=gen)
        bn.weight[0], bn.weight[1] = -0.75, 0.0
    return bn.to(dev)


def _rand(shape, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=gen).to(BF16).to(dev).contiguous(memory_format=CL)


def _leaf(t):
    return t.detach().clone(memory_format=torch.preserve_format).requires_grad_()


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _equal(a, b, what=""):
    assert a.keys() == b.keys()
    for k, v in a.items():
        if v is not None:
            assert torch.equal(_bits(b[k]), _bits(v)), (what, k)


def _act(dev, variant, shape, mask, monkeypatch):
    """one bn_act forward + backward with GSYNC_BN_MASK = mask"""
    from distributed_training_amd import fused_bn

    monkeypatch.setenv("GSYNC_BN_MASK", mask)
    C = shape[1]
    res = variant != "bn_relu"
    fork = variant.startswith("fork")
    bn, xs = _bn(C, dev), _leaf(_rand(shape, dev, 1))
    ids = _leaf(_rand(shape, dev, 2)) if res else None
    dA, dB = _rand(shape, dev, 3), _rand(shape, dev, 4)
    out = fused_bn.bn_act(bn, xs, residual=ids, fork=fork)
    assert fused_bn.last_path == "fused"
    if variant == "fork_both":
        y = out[0]
        torch.autograd.backward(list(out), [dA, dB])
    elif variant == "fork_one":
        y = out[1]
        y.backward(dB)
    else:
        y = out
        y.backward(dA)
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xs.grad, gw=bn.weight.grad, gb=bn.bias.grad, g=ids.grad if res else None,
                rm=bn.running_mean.clone(), rv=bn.running_var.clone(), nbt=bn.num_batches_tracked.clone())


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("variant", ["bn_relu", "bn_add_relu", "fork_both", "fork_one"])
def test_bn_act_bits_against_y(cuda_device, monkeypatch, variant, shape):
    ref = _act(cuda_device, variant, shape, "0", monkeypatch)
    got = _act(cuda_device, variant, shape, "1", monkeypatch)
    _equal(ref, got, variant)
    if ref["y"].numel() >= 256:  # the ReLU cut something and kept something
        assert bool((ref["y"] == 0).any()) and bool((ref["y"] > 0).any())


def test_the_mask_is_saved_in_place_of_y(cuda_device, monkeypatch):
    """what the change is for: with the bits the saved tensors hold a uint8 mask of numel / 8 bytes and no y"""
    from distributed_training_amd import fused_bn

    shape = (2, 24, 5, 3)
    for mask, want in (("1", [torch.uint8]), ("0", [])):
        monkeypatch.setenv("GSYNC_BN_MASK", mask)
        xs = _leaf(_rand(shape, cuda_device, 1))
        out = fused_bn.bn_act(_bn(24, cuda_device), xs)
        assert fused_bn.last_path == "fused"
        saved = out.grad_fn.saved_tensors
        assert [t.dtype for t in saved if t is not None and t.dtype == torch.uint8] == want
        if mask == "1":
            m = next(t for t in saved if t is not None and t.dtype == torch.uint8)
            assert m.numel() == xs.numel() // 8
            assert not any(t is not None and t.data_ptr() == out.data_ptr() for t in saved)


def _stem(dev, shape, mask, two, monkeypatch):
    from distributed_training_amd import fused_bn

    monkeypatch.setenv("GSYNC_BN_MASK", mask)
    C = shape[1]
    oshape = (shape[0], C, (shape[2] - 1) // 2 + 1, (shape[3] - 1) // 2 + 1)
    bn, xs = _bn(C, dev), _leaf(_rand(shape, dev, 5))
    dA, dB = _rand(oshape, dev, 6), _rand(oshape, dev, 7)
    out = fused_bn.bn_relu_pool(bn, xs, nn.MaxPool2d(3, 2, 1), fork=two)
    assert fused_bn.last_path == "fused"
    if two:
        y = out[0]
        torch.autograd.backward(list(out), [dA, dB])
    else:
        y = out
        y.backward(dA)
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xs.grad, gw=bn.weight.grad, gb=bn.bias.grad, rm=bn.running_mean.clone(),
                rv=bn.running_var.clone(), nbt=bn.num_batches_tracked.clone())


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=_id)
@pytest.mark.parametrize("two", [True, False], ids=["fork", "single"])
def test_bn_relu_pool_bits_against_y(cuda_device, monkeypatch, two, shape):
    ref = _stem(cuda_device, shape, "0", two, monkeypatch)
    got = _stem(cuda_device, shape, "1", two, monkeypatch)
    _equal(ref, got, "stem")


def test_micro_resnet_step_bits_against_y(cuda_device, monkeypatch):
    from distributed_training_amd import fused_bn
    from distributed_training_amd.resnet import micro_resnet

    torch.manual_seed(0)
    base = micro_resnet().to(cuda_device).to(memory_format=CL)
    x = torch.rand(8, 3, 32, 32, device=cuda_device).contiguous(memory_format=CL)
    t = torch.randint(0, 10, (8,), device=cuda_device)

    def run(mask):
        monkeypatch.setenv("GSYNC_BN_MASK", mask)
        was = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True  # the convolutions' backward: repeatable solvers, both runs alike
        try:
            model = copy.deepcopy(base)
            with torch.autocast("cuda", dtype=BF16):
                loss = F.cross_entropy(model(x), t)
            assert fused_bn.last_path == "fused"
            loss.backward()
            torch.cuda.synchronize()
        finally:
            torch.backends.cudnn.deterministic = was
        return loss.detach(), {n: p.grad for n, p in model.named_parameters()}, dict(model.named_buffers())

    loss0, g0, b0 = run("0")
    loss1, g1, b1 = run("1")
    assert torch.equal(_bits(loss0), _bits(loss1))
    for n, v in g0.items():
        assert torch.equal(_bits(g1[n]), _bits(v)), n
    for n, v in b0.items():
        assert torch.equal(_bits(b1[n]), _bits(v)), n


@pytest.mark.parametrize("variant", ["bn_relu", "fork_both", "stem"])
def test_capture_replays_equal_to_eager(cuda_device, monkeypatch, variant):
    from distributed_training_amd import fused_bn

    monkeypatch.setenv("GSYNC_BN_MASK", "1")
    dev = cuda_device
    shape = (2, 64, 16, 16)
    oshape = (2, 64, 8, 8) if variant == "stem" else shape
    bn, xs, ids, pool = _bn(64, dev), _leaf(_rand(shape, dev, 8)), _leaf(_rand(shape, dev, 9)), nn.MaxPool2d(3, 2, 1)
    dA, dB = _rand(oshape, dev, 10), _rand(oshape, dev, 11)

    def step():
        if variant == "bn_relu":
            a = fused_bn.bn_act(bn, xs)
            return (a.detach(),) + torch.autograd.grad([a], [xs, bn.weight, bn.bias], [dA])
        if variant == "fork_both":
            a, b = fused_bn.bn_act(bn, xs, residual=ids, fork=True)
            return (a.detach(),) + torch.autograd.grad([a, b], [xs, ids, bn.weight, bn.bias], [dA, dB])
        a, b = fused_bn.bn_relu_pool(bn, xs, pool, fork=True)
        return (a.detach(),) + torch.autograd.grad([a, b], [xs, bn.weight, bn.bias], [dA, dB])

    eager = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    assert fused_bn.last_path == "fused"
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for i, (o, e) in enumerate(zip(outs, eager)):
        assert torch.equal(_bits(o), _bits(e)), i
