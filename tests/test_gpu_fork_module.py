"""The fork gradient sum folded into the BatchNorm backward, through the modules.

* fused_bn.bn_act(..., fork=True): two tensors over one storage; with gradients dA and dB their backward
  is bit for bit the single-output backward of dA + dB (ATen's bf16 add), with and without a residual
  and a ReLU; one unused half takes the single-gradient path; a capture replays equal to eager;
* the stock path (fp32, NCHW, eval, the switch off) returns the same tensor twice and is the stock
  modules bitwise;
* micro_resnet and a width-8 Bottleneck net of [1, 1, 1, 1] blocks, 8 x 3 x 32 x 32: fused against
  GSYNC_FUSED_BN=0 the loss and the buffers are bitwise equal and every parameter gradient is within the
  bound of test_gpu_fused_bn.test_micro_resnet_step_fused_against_stock (twice the difference of two
  stock runs, floor one bf16 ulp of the gradient's scale per BatchNorm): MIOpen's non-repeatable
  backward is the only source of difference left;
* block(x) with one tensor equals the pair form; the state_dict keys are what they were;
* fused_bn.bn_relu_pool: the fused stem (BatchNorm, ReLU taken while pooling, byte indices, the fork's
  sum in the pool backward) against the same BatchNorm kernels around ATen's relu_, max_pool2d and add
  (a pool with a hook, or with other parameters, takes that path): output, dx, grad_weight, grad_bias and
  the buffers bit for bit, one gradient or two; a capture replays equal to eager.
"""
import copy
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF16 = torch.bfloat16


def _bn(C, dev, seed=0):
    gen = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5, generator=gen)
        bn.bias.uniform_(-0.3, 0.3, generator=gen)
        bn.weight[0], bn.weight[1] = -0.75, 0.0
    return bn.to(dev)


def _rand(shape, dev, seed, dtype=BF16, fmt=CL):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=gen).to(dtype).to(dev).contiguous(memory_format=fmt)


def _leaf(t):
    return t.detach().clone(memory_format=torch.preserve_format).requires_grad_()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


FORK_CASES = [("bn", (3, 8, 7, 7)), ("bn_relu", (2, 24, 5, 3)), ("bn_add_relu", (2, 64, 28, 28)),
              ("bn_add_relu", (4, 520, 3, 3))]


@pytest.mark.parametrize("variant,shape", FORK_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_fork_backward_equals_the_summed_gradient(cuda_device, variant, shape):
    from distributed_training_amd import fused_bn

    dev, C = cuda_device, shape[1]
    relu, res = variant != "bn", variant == "bn_add_relu"
    x, idn = _rand(shape, dev, 1), (_rand(shape, dev, 2) if res else None)
    dA, dB = _rand(shape, dev, 3), _rand(shape, dev, 4)

    def run(fork, unused=None):
        bn, xs, ids = _bn(C, dev), _leaf(x), (_leaf(idn) if res else None)
        out = fused_bn.bn_act(bn, xs, relu=relu, residual=ids, fork=fork)
        assert fused_bn.last_path == "fused"
        if fork:
            a, b = out
            assert a.data_ptr() == b.data_ptr() and a is not b and torch.equal(a, b)
            if unused is None:
                torch.autograd.backward([a, b], [dA, dB])
            else:
                (b if unused == "a" else a).backward(dA)
            y = a
        else:
            y = out
            y.backward(dA + dB if unused is None else dA)
        torch.cuda.synchronize()
        return dict(y=y.detach(), dx=xs.grad, gw=bn.weight.grad, gb=bn.bias.grad, g=ids.grad if res else None,
                    rm=bn.running_mean.clone(), rv=bn.running_var.clone())

    one, two = run(False), run(True)
    for k, v in one.items():
        if v is not None:
            assert torch.equal(_bits(two[k]), _bits(v)), k
    single = run(False, unused="b")
    for unused in ("a", "b"):
        half = run(True, unused=unused)
        for k, v in single.items():
            if v is not None:
                assert torch.equal(_bits(half[k]), _bits(v)), (unused, k)


def test_fork_with_non_contiguous_gradients(cuda_device):
    """the two gradients are made channels_last-contiguous, as the single one is"""
    from distributed_training_amd import fused_bn

    dev, shape = cuda_device, (2, 16, 6, 5)
    x = _rand(shape, dev, 5)
    dA, dB = _rand(shape, dev, 6, fmt=torch.contiguous_format), _rand(shape, dev, 7)
    res = []
    for fork in (False, True):
        bn, xs = _bn(16, dev), _leaf(x)
        out = fused_bn.bn_act(bn, xs, fork=fork)
        if fork:
            torch.autograd.backward(list(out), [dA, dB])
        else:
            out.backward(dA + dB)
        res.append((xs.grad, bn.weight.grad, bn.bias.grad))
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("case", ["fp32", "nchw", "eval", "env_off"])
def test_fork_fallback_is_the_stock_path_bitwise(cuda_device, monkeypatch, case):
    from distributed_training_amd import fused_bn

    dev, shape = cuda_device, (2, 16, 6, 5)
    dtype = torch.float32 if case == "fp32" else BF16
    fmt = torch.contiguous_format if case == "nchw" else CL
    x, idn = _rand(shape, dev, 8, dtype, fmt), _rand(shape, dev, 9, dtype, fmt)
    dA, dB = _rand(shape, dev, 10, dtype, fmt), _rand(shape, dev, 11, dtype, fmt)
    if case == "env_off":
        monkeypatch.setenv("GSYNC_FUSED_BN", "0")
    outs = []
    for fork in (True, False):
        bn, xs, ids = _bn(16, dev), _leaf(x), _leaf(idn)
        if case == "eval":
            bn.eval()
        if fork:
            a, b = fused_bn.bn_act(bn, xs, residual=ids, fork=True)
            assert fused_bn.last_path == "stock" and a is b
            torch.autograd.backward([a, b], [dA, dB])
        else:
            a = F.relu(bn(xs) + ids)
            a.backward(dA + dB)
        outs.append((a.detach(), xs.grad, ids.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var))
    for i, (p, q) in enumerate(zip(*outs)):
        assert torch.equal(p, q), i


def test_fork_capture_replays_equal_to_eager(cuda_device):
    from distributed_training_amd import fused_bn

    dev, shape = cuda_device, (2, 64, 28, 28)
    x, idn, dA, dB = (_rand(shape, dev, s) for s in (12, 13, 14, 15))
    bn, xs, ids = _bn(64, dev), _leaf(x), _leaf(idn)

    def step():
        a, b = fused_bn.bn_act(bn, xs, residual=ids, fork=True)
        return (a.detach(),) + torch.autograd.grad([a, b], [xs, ids, bn.weight, bn.bias], [dA, dB])

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
    for k, o, e in zip(("y", "dx", "g", "gw", "gb"), outs, eager):
        assert torch.equal(_bits(o), _bits(e)), k


# ---- whole models -----------------------------------------------------------------------------------
def _models():
    from distributed_training_amd.resnet import Bottleneck, ResNet, micro_resnet

    return {"micro": micro_resnet, "bottleneck": lambda: ResNet(Bottleneck, [1, 1, 1, 1], num_classes=10, width=8)}


def _bf16_ulp(v: float) -> float:
    return 2.0 ** (math.floor(math.log2(v)) - 7) if v > 0 else 0.0


@pytest.mark.parametrize("name", ["micro", "bottleneck"])
def test_model_step_fused_against_stock(cuda_device, monkeypatch, name):
    from distributed_training_amd import fused_bn

    torch.manual_seed(0)
    base = _models()[name]().to(cuda_device).to(memory_format=CL)
    x = torch.rand(8, 3, 32, 32, device=cuda_device).contiguous(memory_format=CL)
    t = torch.randint(0, 10, (8,), device=cuda_device)
    depth = sum(isinstance(m, nn.BatchNorm2d) for m in base.modules())

    def run(fused):
        monkeypatch.setenv("GSYNC_FUSED_BN", "1" if fused else "0")
        model = copy.deepcopy(base)
        with torch.autocast("cuda", dtype=BF16):
            loss = F.cross_entropy(model(x), t)
        assert fused_bn.last_path == ("fused" if fused else "stock")
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach(), [p.grad for p in model.parameters()], [b.clone() for b in model.buffers()]

    loss_s1, gs1, buf_s = run(False)
    loss_s2, gs2, _ = run(False)
    loss_f, gf, buf_f = run(True)
    assert torch.equal(loss_f, loss_s1) and torch.equal(loss_s1, loss_s2)
    for a, b in zip(buf_f, buf_s):
        assert torch.equal(a, b)
    worst = 0.0
    for (pname, _), a, s1, s2 in zip(base.named_parameters(), gf, gs1, gs2):
        noise = float((s1 - s2).abs().max())
        floor = _bf16_ulp(float(s1.abs().max())) * depth
        diff = float((a - s1).abs().max())
        bound = max(2.0 * noise, floor)
        worst = max(worst, diff / bound if bound else float(diff > 0))
        print(f"[fork] {name} {pname}: |fused-stock| {diff:.3e}  stock noise {noise:.3e}  floor {floor:.3e}")
        assert diff <= bound, (pname, diff, noise, floor)
    print(f"[fork] {name}: depth {depth}, worst diff/bound {worst:.3f}")


@pytest.mark.parametrize("name", ["micro", "bottleneck"])
def test_block_with_one_tensor_equals_the_pair_form(cuda_device, name):
    torch.manual_seed(1)
    model = _models()[name]().to(cuda_device).to(memory_format=CL)
    keys = list(model.state_dict().keys())
    with torch.device("meta"):
        assert list(_models()[name]().state_dict().keys()) == keys
    assert "layer2.0.downsample.1.running_var" in keys and "layer4.0.conv1.weight" in keys and not any(
        "pair" in k or "fork" in k for k in keys)
    block = model.layer2[0]
    C = block.conv1.in_channels
    x = _rand((4, C, 8, 8), cuda_device, 16)
    with torch.autocast("cuda", dtype=BF16):
        snap = copy.deepcopy(block.state_dict())
        one = block(x)
        block.load_state_dict(snap)
        a, b = block.forward_pair((x, x), True)
        block.load_state_dict(snap)
        seq = model.layer2(x)
    assert isinstance(one, torch.Tensor) and torch.equal(one, a) and torch.equal(a, b) and a.data_ptr() == b.data_ptr()
    assert isinstance(seq, torch.Tensor) and torch.equal(seq, one)


# ---- the stem ---------------------------------------------------------------------------------------
POOL_CASES = [(2, 8, 1, 1), (2, 16, 7, 6), (3, 64, 30, 28), (1, 72, 9, 8)]


def _stem(bn, x, pool, dA, dB):
    """bn_relu_pool forward + backward on fresh leaves; dB None: fork=False"""
    from distributed_training_amd import fused_bn

    xs = _leaf(x)
    out = fused_bn.bn_relu_pool(bn, xs, pool, fork=dB is not None)
    if dB is None:
        y = out
        y.backward(dA)
    else:
        y = out[0]
        assert torch.equal(out[0], out[1])
        torch.autograd.backward(list(out), [dA, dB])
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xs.grad, gw=bn.weight.grad, gb=bn.bias.grad, rm=bn.running_mean.clone(),
                rv=bn.running_var.clone(), nbt=bn.num_batches_tracked.clone())


@pytest.mark.parametrize("shape", POOL_CASES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("two", [True, False], ids=["fork", "single"])
def test_stem_fused_equals_aten_pool_around_the_same_bn(cuda_device, two, shape):
    from distributed_training_amd import fused_bn

    dev, C = cuda_device, shape[1]
    x = _rand(shape, dev, 20)
    oshape = (shape[0], C, (shape[2] - 1) // 2 + 1, (shape[3] - 1) // 2 + 1)
    dA, dB = _rand(oshape, dev, 21), (_rand(oshape, dev, 22) if two else None)
    fused = _stem(_bn(C, dev), x, nn.MaxPool2d(3, 2, 1), dA, dB)
    assert fused_bn.last_path == "fused" and fused["y"].shape == oshape
    assert fused["y"].is_contiguous(memory_format=CL)
    hooked = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
    seen = []
    hooked.register_forward_hook(lambda m, i, o: seen.append(1))
    ref = _stem(_bn(C, dev), x, hooked, dA, dB)
    assert seen == [1]
    for k, v in ref.items():
        assert torch.equal(_bits(fused[k]) if v.is_floating_point() else fused[k], _bits(v) if v.is_floating_point() else v), k


@pytest.mark.parametrize("case", ["fp32", "nchw", "eval", "env_off", "kernel2", "ceil", "dilation", "indices", "avg"])
def test_stem_fallback_is_the_stock_path_bitwise(cuda_device, monkeypatch, case):
    from distributed_training_amd import fused_bn

    dev, shape = cuda_device, (2, 16, 9, 10)
    dtype = torch.float32 if case == "fp32" else BF16
    x = _rand(shape, dev, 23, dtype, torch.contiguous_format if case == "nchw" else CL)
    pool = {"kernel2": nn.MaxPool2d(2, 2, 1), "ceil": nn.MaxPool2d(3, 2, 1, ceil_mode=True),
            "dilation": nn.MaxPool2d(3, 2, 1, dilation=2), "avg": nn.AvgPool2d(3, 2, 1),
            "indices": nn.MaxPool2d(3, 2, 1, return_indices=True)}.get(case, nn.MaxPool2d(3, 2, 1))
    if case == "env_off":
        monkeypatch.setenv("GSYNC_FUSED_BN", "0")
    bn_a, bn_b = _bn(16, dev), _bn(16, dev)
    if case == "eval":
        bn_a.eval(), bn_b.eval()
    xs_a, xs_b = _leaf(x), _leaf(x)
    if case == "indices":
        a = fused_bn.bn_relu_pool(bn_a, xs_a, pool, fork=False)
        b = pool(F.relu(bn_b(xs_b)))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        return
    a, a2 = fused_bn.bn_relu_pool(bn_a, xs_a, pool, fork=True)
    assert a is a2
    if case in ("fp32", "nchw", "eval", "env_off"):
        assert fused_bn.last_path == "stock"
        b = pool(F.relu(bn_b(xs_b)))
    else:
        monkeypatch.setenv("GSYNC_FUSED_BN", "1")
        b = pool(fused_bn.bn_act(bn_b, xs_b))  # the BatchNorm stays fused, the pool is the module's
    dA, dB = _rand(tuple(b.shape), dev, 24, dtype), _rand(tuple(b.shape), dev, 25, dtype)
    torch.autograd.backward([a, a2], [dA, dB])
    b.backward(dA + dB)
    for p, q in ((a, b), (xs_a.grad, xs_b.grad), (bn_a.weight.grad, bn_b.weight.grad), (bn_a.bias.grad, bn_b.bias.grad),
                 (bn_a.running_mean, bn_b.running_mean), (bn_a.running_var, bn_b.running_var)):
        assert torch.equal(p, q)


def test_stem_capture_replays_equal_to_eager(cuda_device):
    from distributed_training_amd import fused_bn

    dev, shape = cuda_device, (2, 64, 30, 28)
    x, dA, dB = _rand(shape, dev, 26), _rand((2, 64, 15, 14), dev, 27), _rand((2, 64, 15, 14), dev, 28)
    bn, xs, pool = _bn(64, dev), _leaf(x), nn.MaxPool2d(3, 2, 1)

    def step():
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
    for k, o, e in zip(("y", "dx", "gw", "gb"), outs, eager):
        assert torch.equal(_bits(o), _bits(e)), k
