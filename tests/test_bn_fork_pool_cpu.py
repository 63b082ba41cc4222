"""The fork form of the BatchNorm backward and the stem's pool kernels without a GPU.

1. the argument checks of gs_bn_bwd_reduce_fork, gs_relu_maxpool_fwd and gs_maxpool_bwd, all of which sit
   before any launch (the pointers are made-up values that are never dereferenced);
2. bn_act(..., fork=True) on the stock path is the same tensor twice, and autograd sums its two gradients;
3. resnet.py's pair plumbing on the CPU is the previous forward and backward bit for bit: the model
   driven block by block through forward_pair against the same modules called layer by layer with one
   tensor, for BasicBlock and Bottleneck nets; a hook on a layer still runs;
4. the pure-torch pool reference of tests/test_gpu_pool_kernels.py names the elements ATen's CPU
   max_pool2d names, on every shape and data set the GPU test uses; bn_relu_pool on the CPU is the
   stock modules.
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from distributed_training_amd import fused_bn
from distributed_training_amd.resnet import Bottleneck, ResNet, micro_resnet


@pytest.fixture(scope="module")
def lib():
    from distributed_training_amd import _lib as L

    return L.lib()


# ---- 1. argument checks ------------------------------------------------------------------------
A = 0x7F0000001000  # made-up addresses, 16-byte aligned, never dereferenced
R0, C0 = 777, 24
BYTES = R0 * C0 * 2


def _fork_args(lib, **kw):
    P = lib.gs_bn_bwd_partials(R0, C0)
    a = dict(x=A, dy_a=A + 0x100000, dy_b=A + 0x200000, y=A + 0x300000, g_out=A + 0x400000, mean=A + 0x500000,
             ws=A + 0x600000, ws_floats=P * C0 * 2, R=R0, C=C0)
    a.update(kw)
    return [a[k] for k in ("x", "dy_a", "dy_b", "y", "g_out", "mean", "ws", "ws_floats", "R", "C")] + [None]


FORK_BAD = (
    [{k: None} for k in ("x", "dy_a", "g_out", "mean", "ws")]
    + [{k: A + 0x700008} for k in ("x", "dy_a", "dy_b", "y", "g_out", "ws")]
    + [dict(g_out=A + d) for d in (0, 0x100000, 0x200000, 0x300000)]  # g_out on x, dy_a, dy_b, y
    + [dict(g_out=A + 0x100000 + BYTES - 16), dict(g_out=A + 0x200000 - BYTES + 16)]  # partial overlaps
    + [dict(dy_b=None, y=None)]  # one gradient, no mask: nothing to write into g_out
    + [dict(ws_floats=-1), dict(C=12), dict(C=0), dict(R=0), dict(R=2 ** 60)]
)


@pytest.mark.parametrize("bad", FORK_BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_reduce_fork_rejects(lib, bad):
    from distributed_training_amd import _lib as L

    if bad == dict(ws_floats=-1):
        bad = dict(ws_floats=lib.gs_bn_bwd_partials(R0, C0) * C0 * 2 - 1)
    lib.gs_bn_bwd_partials(64, 64)
    assert lib.gs_bn_bwd_reduce_fork(*_fork_args(lib, **bad)) == L.GS_EINVAL
    assert lib.gs_last_error()


# ---- 2. the stock path -----------------------------------------------------------------------------
@pytest.mark.parametrize("res", [True, False])
def test_fork_on_cpu_is_the_same_tensor_twice(res):
    torch.manual_seed(0)
    bn_a = nn.BatchNorm2d(16)
    bn_b = copy.deepcopy(bn_a)
    x_a, id_a = torch.randn(3, 16, 5, 5, requires_grad=True), torch.randn(3, 16, 5, 5, requires_grad=True)
    x_b, id_b = x_a.detach().clone().requires_grad_(), id_a.detach().clone().requires_grad_()
    dA, dB = torch.randn(3, 16, 5, 5), torch.randn(3, 16, 5, 5)
    a, b = fused_bn.bn_act(bn_a, x_a, residual=id_a if res else None, fork=True)
    assert fused_bn.last_path == "stock" and a is b
    ref = bn_b(x_b)
    ref = F.relu(ref + id_b if res else ref)
    assert torch.equal(a, ref)
    torch.autograd.backward([a, b], [dA, dB])
    ref.backward(dA + dB)
    assert torch.equal(x_a.grad, x_b.grad) and torch.equal(bn_a.weight.grad, bn_b.weight.grad)
    assert torch.equal(bn_a.bias.grad, bn_b.bias.grad)
    if res:
        assert torch.equal(id_a.grad, id_b.grad)


# ---- 3. the pair plumbing ---------------------------------------------------------------------------
def _layer_by_layer(model, x):
    """the forward as it was before the blocks took pairs: every layer called with one tensor"""
    x = model.maxpool(F.relu(model.bn1(model.conv1(x))))
    x = model.layer4(model.layer3(model.layer2(model.layer1(x))))
    return model.fc(torch.flatten(model.avgpool(x), 1))


@pytest.mark.parametrize("make", [micro_resnet, lambda: ResNet(Bottleneck, [2, 1, 1, 2], num_classes=10, width=8)],
                         ids=["basic", "bottleneck"])
def test_pair_plumbing_equals_the_layer_calls(make):
    torch.manual_seed(0)
    m_a = make()
    m_b = copy.deepcopy(m_a)
    x = torch.randn(4, 3, 32, 32)
    t = torch.tensor([1, 7, 3, 0])
    out_a, out_b = m_a(x), _layer_by_layer(m_b, x)
    assert torch.equal(out_a, out_b)
    F.cross_entropy(out_a, t).backward()
    F.cross_entropy(out_b, t).backward()
    for (n, p), q in zip(m_a.named_parameters(), m_b.parameters()):
        assert torch.equal(p.grad, q.grad), n
    for (n, p), q in zip(m_a.named_buffers(), m_b.buffers()):
        assert torch.equal(p, q), n
    # one tensor in, one tensor out, for a block and for a layer
    m_a.eval()
    h = torch.randn(2, m_a.layer1[0].conv1.in_channels, 8, 8)
    one = m_a.layer1[0](h)
    a, b = m_a.layer1[0].forward_pair((h, h), True)
    assert isinstance(one, torch.Tensor) and torch.equal(one, a) and a is b
    assert torch.equal(m_a.layer1(h), nn.Sequential(*m_a.layer1)(h))


def test_a_hook_on_a_layer_still_runs():
    torch.manual_seed(0)
    model = micro_resnet()
    ref = copy.deepcopy(model)
    seen = []
    model.layer3.register_forward_hook(lambda m, i, o: seen.append("layer3"))
    model.layer2[0].register_forward_pre_hook(lambda m, i: seen.append("block"))
    x = torch.randn(2, 3, 32, 32)
    assert torch.equal(model(x), ref(x))
    assert seen == ["block", "layer3"]


# ---- 1b. the pool entries' argument checks ------------------------------------------------------------
PN, PH, PW, PC = 2, 7, 6, 16  # in 2 * 7 * 6 * 16 * 2 = 2688 bytes, out 2 * 4 * 3 * 16 * 2 = 768 bytes, idx 384


def _fwd_args(**kw):
    a = dict(y=A, pooled=A + 0x10000, idx=A + 0x20000, N=PN, H=PH, W=PW, C=PC)
    a.update(kw)
    return [a[k] for k in ("y", "pooled", "idx", "N", "H", "W", "C")] + [None]


def _bwd_args(**kw):
    a = dict(d_a=A, d_b=A + 0x10000, idx=A + 0x20000, dx=A + 0x30000, N=PN, H=PH, W=PW, C=PC)
    a.update(kw)
    return [a[k] for k in ("d_a", "d_b", "idx", "dx", "N", "H", "W", "C")] + [None]


POOL_SHAPE_BAD = [dict(N=0), dict(H=0), dict(W=-1), dict(C=12), dict(C=0), dict(N=2 ** 58)]
FWD_BAD = ([{k: None} for k in ("y", "pooled", "idx")] + [{k: A + 0x70008} for k in ("y", "pooled", "idx")]
           + [dict(pooled=A + 2688 - 16), dict(idx=A + 16), dict(idx=A + 0x10000 + 768 - 16)] + POOL_SHAPE_BAD)
BWD_BAD = ([{k: None} for k in ("d_a", "idx", "dx")] + [{k: A + 0x70008} for k in ("d_a", "d_b", "idx", "dx")]
           + [dict(dx=A + 768 - 16), dict(dx=A + 0x10000 - 2688 + 16), dict(dx=A + 0x20000 + 384 - 16)]
           + POOL_SHAPE_BAD)
_ids = lambda d: "-".join(f"{k}={v}" for k, v in d.items())  # noqa: E731


@pytest.mark.parametrize("bad", FWD_BAD, ids=_ids)
def test_relu_maxpool_fwd_rejects(lib, bad):
    from distributed_training_amd import _lib as L

    lib.gs_bn_bwd_partials(64, 64)
    assert lib.gs_relu_maxpool_fwd(*_fwd_args(**bad)) == L.GS_EINVAL
    assert lib.gs_last_error()


@pytest.mark.parametrize("bad", BWD_BAD, ids=_ids)
def test_maxpool_bwd_rejects(lib, bad):
    from distributed_training_amd import _lib as L

    lib.gs_bn_bwd_partials(64, 64)
    assert lib.gs_maxpool_bwd(*_bwd_args(**bad)) == L.GS_EINVAL
    assert lib.gs_last_error()


# ---- 4. the pool reference, and the stock stem ----------------------------------------------------------
def test_pool_reference_names_what_aten_names():
    from tests import test_gpu_pool_kernels as P

    for shape in P.POOL_SHAPES:
        for kind in P.DATA:
            y = P.make_y(shape, kind)
            best, code = P.pool_ref(y)
            want, idx = F.max_pool2d(F.relu(y.float().permute(0, 3, 1, 2)), 3, 2, 1, return_indices=True)
            want, idx = want.permute(0, 2, 3, 1), idx.permute(0, 2, 3, 1)
            assert torch.equal(torch.isnan(best), torch.isnan(want)), (shape, kind)
            assert torch.equal(torch.nan_to_num(best, nan=0.0), torch.nan_to_num(want, nan=0.0)), (shape, kind)
            assert torch.equal(P.code_to_flat_index(code, shape[1], shape[2]), idx), (shape, kind)
            if kind == "special":
                assert bool(torch.isnan(best).any()) and not bool(torch.isnan(best).all())


@pytest.mark.parametrize("fork", [True, False])
def test_bn_relu_pool_on_cpu_is_the_stock_modules(fork):
    torch.manual_seed(0)
    bn_a, pool = nn.BatchNorm2d(16), nn.MaxPool2d(3, 2, 1)
    bn_b = copy.deepcopy(bn_a)
    x_a = torch.randn(3, 16, 9, 10, requires_grad=True)
    x_b = x_a.detach().clone().requires_grad_()
    out = fused_bn.bn_relu_pool(bn_a, x_a, pool, fork=fork)
    assert fused_bn.last_path == "stock"
    ref = pool(F.relu(bn_b(x_b)))
    dA, dB = torch.randn_like(ref), torch.randn_like(ref)
    if fork:
        assert out[0] is out[1] and torch.equal(out[0], ref)
        torch.autograd.backward(list(out), [dA, dB])
        ref.backward(dA + dB)
    else:
        assert torch.equal(out, ref)
        out.backward(dA)
        ref.backward(dA)
    assert torch.equal(x_a.grad, x_b.grad) and torch.equal(bn_a.weight.grad, bn_b.weight.grad)
    assert torch.equal(bn_a.running_var, bn_b.running_var)
