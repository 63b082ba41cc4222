"""fused_bn.bn_act on the GPU: the fused NHWC BatchNorm backward (gs_bn_bwd_reduce /
gs_bn_bwd_dx) and the fused forward add + ReLU (gs_add_relu_fwd).

* forward (y, running statistics, num_batches_tracked) and the identity branch's
  gradient g are bitwise the stock path's (MIOpen BN + ATen add_ / relu_ /
  threshold_backward);
* dx, grad_weight and grad_bias are judged against an fp64 evaluation of
      dx = w * invstd * (g - sum(g)/R - xhat * sum(g*xhat)/R),  g = dy * [y > 0]
  from the same bf16 x and dy, the mask from the forward's actual y, mean and
  invstd from fp64 statistics of x: the fused path's max error is at most twice
  the stock path's error against that same truth (the summation order differs);
* every case outside the fused path's conditions runs the stock path, bitwise;
* the backward is deterministic and one forward + backward recorded into a
  hipGraph replays bitwise equal to eager;
* micro_resnet, one bf16-autocast channels_last step, fused on and off: equal
  losses, parameter gradients within the stock path's own run-to-run bound.

Measured on an MI355X (fused max error / stock max error against the fp64 truth, 15 cases each):
dx 0.84 - 1.19 (1.000 on the 12 cases with more than two rows: dx is truncated to bf16 as MIOpen
truncates it; with round-to-nearest, -DGS_BN_DX_RNE=1, 0.32 - 0.84), grad_weight 0.35 - 1.20,
grad_bias 0.50 - 1.00 (both exact on 9 cases).  micro_resnet: two stock runs agree bitwise, so the
floor (one bf16 ulp of the gradient's max times 12 BatchNorms) is the bound; the fused gradients are
bit-identical to the stock path's (worst difference / bound 0.000; with round-to-nearest dx 0.50).
"""
import copy
import functools
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
VARIANTS = ["bn", "bn_relu", "bn_add_relu"]
SHAPES = [
    (2, 8, 1, 1),      # two rows, one vector
    (3, 8, 7, 7),      # 147 rows, a multiple of no tile
    (2, 24, 5, 3),     # a channel-tile tail
    (2, 64, 56, 56),   # many row-blocks: the partial fold
    (4, 2048, 7, 7),   # many channel tiles with few rows
]


def _inputs(variant, shape, dtype=torch.bfloat16, memory_format=CL):
    """x with its own mean and scale per channel, weights with a negative and a zero, random dy."""
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(1234 + C * 7 + H)
    mu = torch.linspace(-2.0, 2.0, C).view(1, C, 1, 1)
    sc = torch.linspace(0.5, 2.0, C).flip(0).view(1, C, 1, 1)
    dev = torch.device("cuda", 0)
    x = (torch.randn(shape, generator=gen) * sc + mu).to(dtype).to(dev).contiguous(memory_format=memory_format)
    w = torch.empty(C).uniform_(0.5, 1.5, generator=gen)
    w[0], w[1] = -0.75, 0.0
    b = torch.empty(C).uniform_(-0.3, 0.3, generator=gen)
    idn = None
    if variant == "bn_add_relu":
        idn = torch.randn(shape, generator=gen).to(dtype).to(dev).contiguous(memory_format=memory_format)
    dy = torch.randn(shape, generator=gen).to(dtype).to(dev).contiguous(memory_format=memory_format)
    return x, w.to(dev), b.to(dev), idn, dy


def _module(C, w, b, dtype=torch.float32):
    bn = nn.BatchNorm2d(C).to(w.device)
    with torch.no_grad():
        bn.weight.copy_(w)
        bn.bias.copy_(b)
    return bn.to(dtype)


def _stock(bn, x, relu, idn):
    out = bn(x)
    if idn is not None:
        out += idn
    return F.relu(out, inplace=True) if relu else out


def _run(fn, bn, x, idn, dy):
    """forward + backward of fn on fresh leaves -> dict of everything a test compares"""
    x = x.detach().clone(memory_format=torch.preserve_format).requires_grad_()
    idn = None if idn is None else idn.detach().clone(memory_format=torch.preserve_format).requires_grad_()
    bn.zero_grad(set_to_none=True)
    y = fn(bn, x, idn)
    y.backward(dy)
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=x.grad, gw=bn.weight.grad, gb=bn.bias.grad, g=None if idn is None else idn.grad,
                rm=bn.running_mean.clone(), rv=bn.running_var.clone(), nbt=int(bn.num_batches_tracked))


@functools.lru_cache(maxsize=None)
def _case(variant, shape):
    """fused run, stock run and fp64 truth of one (variant, shape), computed once"""
    from distributed_training_amd import fused_bn

    relu = variant != "bn"
    x, w, b, idn, dy = _inputs(variant, shape)
    C = shape[1]
    fused = _run(lambda m, xx, ii: fused_bn.bn_act(m, xx, relu=relu, residual=ii), _module(C, w, b), x, idn, dy)
    path = fused_bn.last_path
    stock = _run(lambda m, xx, ii: _stock(m, xx, relu, ii), _module(C, w, b), x, idn, dy)
    # fp64 truth
    xd, dyd, wd = x.double(), dy.double(), w.double().view(1, C, 1, 1)
    R = xd.numel() // C
    mean = xd.mean(dim=(0, 2, 3), keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    xhat = (xd - mean) * invstd
    g = dyd * (fused["y"] > 0) if relu else dyd
    sg = g.sum(dim=(0, 2, 3), keepdim=True)
    sgx = (g * xhat).sum(dim=(0, 2, 3), keepdim=True)
    truth = dict(dx=wd * invstd * (g - sg / R - xhat * sgx / R), gw=sgx.flatten(), gb=sg.flatten())
    return path, fused, stock, truth


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_and_identity_gradient_equal_the_stock_path(cuda_device, variant, shape):
    path, fused, stock, _ = _case(variant, shape)
    assert path == "fused"
    assert torch.equal(fused["y"], stock["y"])
    assert torch.equal(fused["rm"], stock["rm"]) and torch.equal(fused["rv"], stock["rv"])
    assert fused["nbt"] == stock["nbt"] == 1
    if variant != "bn" and fused["y"].numel() >= 1000:
        zeros = float((fused["y"] == 0).float().mean())
        assert 0.2 < zeros < 0.8, zeros  # the mask is exercised both ways
    if variant == "bn_add_relu":
        assert torch.equal(fused["g"], stock["g"])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", VARIANTS)
def test_backward_error_within_twice_the_stock_paths(cuda_device, variant, shape):
    path, fused, stock, truth = _case(variant, shape)
    assert path == "fused"
    errs = {}
    for k in ("dx", "gw", "gb"):
        ef = float((fused[k].double() - truth[k]).abs().max())
        es = float((stock[k].double() - truth[k]).abs().max())
        errs[k] = (ef, es)
        print(f"[fused_bn] {variant} {shape} {k}: fused err {ef:.4e}  stock err {es:.4e}  "
              f"ratio {ef / es if es else float('inf'):.3f}")
    for k, (ef, es) in errs.items():
        assert ef <= 2.0 * es, (k, ef, es)


def _fallback_pair(shape, *, dtype=torch.bfloat16, memory_format=CL, wdtype=torch.float32, train=True):
    from distributed_training_amd import fused_bn

    x, w, b, idn, dy = _inputs("bn_add_relu", shape, dtype=dtype, memory_format=memory_format)
    bn_a, bn_b = _module(shape[1], w, b, wdtype).train(train), _module(shape[1], w, b, wdtype).train(train)
    a = _run(lambda m, xx, ii: fused_bn.bn_act(m, xx, relu=True, residual=ii), bn_a, x, idn, dy)
    path = fused_bn.last_path
    s = _run(lambda m, xx, ii: _stock(m, xx, True, ii), bn_b, x, idn, dy)
    return path, a, s


@pytest.mark.parametrize("case", ["c_mod_8", "nchw", "fp32", "eval", "bf16_weights", "env_off"])
def test_fallback_is_the_stock_path_bitwise(cuda_device, monkeypatch, case):
    kw, shape = {}, (2, 16, 4, 4)
    if case == "c_mod_8":
        shape = (2, 12, 4, 4)
    elif case == "nchw":
        kw = dict(memory_format=torch.contiguous_format)
    elif case == "fp32":
        kw = dict(dtype=torch.float32)
    elif case == "eval":
        kw = dict(train=False)
    elif case == "bf16_weights":
        kw = dict(wdtype=torch.bfloat16)
    elif case == "env_off":
        monkeypatch.setenv("GSYNC_FUSED_BN", "0")
    path, a, s = _fallback_pair(shape, **kw)
    assert path == "stock"
    for k in ("y", "dx", "gw", "gb", "g", "rm", "rv"):
        assert torch.equal(a[k], s[k]), k
    assert a["nbt"] == s["nbt"]


def test_fused_conditions_without_the_switch(cuda_device):
    """the shape the fallback cases vary does take the fused path when nothing is varied"""
    path, a, s = _fallback_pair((2, 16, 4, 4))
    assert path == "fused"
    assert torch.equal(a["y"], s["y"]) and torch.equal(a["g"], s["g"])


@pytest.mark.parametrize("variant", VARIANTS)
def test_backward_is_deterministic(cuda_device, variant):
    from distributed_training_amd import fused_bn

    shape = (2, 64, 56, 56)
    x, w, b, idn, dy = _inputs(variant, shape)
    relu = variant != "bn"
    runs = [_run(lambda m, xx, ii: fused_bn.bn_act(m, xx, relu=relu, residual=ii), _module(64, w, b), x, idn, dy)
            for _ in range(2)]
    for k in ("y", "dx", "gw", "gb") + (("g",) if idn is not None else ()):
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_capture_replays_equal_to_eager(cuda_device):
    from distributed_training_amd import fused_bn

    shape = (2, 64, 56, 56)
    x, w, b, idn, dy = _inputs("bn_add_relu", shape)
    eager = _run(lambda m, xx, ii: fused_bn.bn_act(m, xx, residual=ii), _module(64, w, b), x, idn, dy)
    bn = _module(64, w, b)
    xs, ids = x.clone(memory_format=torch.preserve_format).requires_grad_(), \
        idn.clone(memory_format=torch.preserve_format).requires_grad_()

    def step():
        y = fused_bn.bn_act(bn, xs, residual=ids)
        return (y.detach(),) + torch.autograd.grad(y, [xs, ids, bn.weight, bn.bias], dy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # a linear chain: BN forward, add+ReLU, reduce, dx
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
    for k, o in zip(("y", "dx", "g", "gw", "gb"), outs):
        assert torch.equal(o, eager[k]), k


def _bf16_ulp(v: float) -> float:
    return 2.0 ** (math.floor(math.log2(v)) - 7) if v > 0 else 0.0


def test_micro_resnet_step_fused_against_stock(cuda_device, monkeypatch):
    """Bound per parameter gradient: twice the difference between two stock runs, with a floor of one
    bf16 ulp of the gradient's scale (its max magnitude) times the model's depth (its BatchNorm count):
    each BN backward rounds dx to bf16 once, so two correct paths differ by up to an ulp per layer."""
    from distributed_training_amd import fused_bn
    from distributed_training_amd.resnet import micro_resnet

    torch.manual_seed(0)
    base = micro_resnet().to(cuda_device).to(memory_format=CL)
    x = torch.rand(8, 3, 32, 32, device=cuda_device).contiguous(memory_format=CL)
    t = torch.randint(0, 10, (8,), device=cuda_device)
    depth = sum(isinstance(m, nn.BatchNorm2d) for m in base.modules())

    def run(fused):
        monkeypatch.setenv("GSYNC_FUSED_BN", "1" if fused else "0")
        model = copy.deepcopy(base)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = F.cross_entropy(model(x), t)
        assert fused_bn.last_path == ("fused" if fused else "stock")
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach(), [p.grad for p in model.parameters()], \
            [b.clone() for b in model.buffers()]

    loss_s1, gs1, buf_s = run(False)
    loss_s2, gs2, _ = run(False)
    loss_f, gf, buf_f = run(True)
    assert torch.equal(loss_f, loss_s1) and torch.equal(loss_s1, loss_s2)
    for a, b in zip(buf_f, buf_s):
        assert torch.equal(a, b)
    worst = 0.0
    for (name, _), a, s1, s2 in zip(base.named_parameters(), gf, gs1, gs2):
        noise = float((s1 - s2).abs().max())
        floor = _bf16_ulp(float(s1.abs().max())) * depth
        diff = float((a - s1).abs().max())
        bound = max(2.0 * noise, floor)
        worst = max(worst, diff / bound if bound else float(diff > 0))
        print(f"[fused_bn] micro {name}: |fused-stock| {diff:.3e}  stock noise {noise:.3e}  floor {floor:.3e}")
        assert diff <= bound, (name, diff, noise, floor)
    print(f"[fused_bn] micro: depth {depth}, worst diff/bound {worst:.3f}")
