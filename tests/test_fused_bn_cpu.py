"""fused_bn.bn_act without a GPU: it is the stock path (relu(bn(x) + identity),
outputs and gradients exact), the models keep their state_dict keys, and a
ResNet-18 still trains on CPU."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from distributed_training_amd import fused_bn
from distributed_training_amd.resnet import MODELS


@pytest.mark.parametrize("relu,res", [(True, True), (True, False), (False, False)])
def test_bn_act_on_cpu_is_the_stock_path(relu, res):
    torch.manual_seed(0)
    bn_a = nn.BatchNorm2d(16)
    with torch.no_grad():
        bn_a.weight.uniform_(-1, 1)
        bn_a.bias.uniform_(-1, 1)
    bn_b = copy.deepcopy(bn_a)
    x_a = torch.randn(3, 16, 5, 5, requires_grad=True)
    id_a = torch.randn(3, 16, 5, 5, requires_grad=True)
    x_b, id_b = x_a.detach().clone().requires_grad_(), id_a.detach().clone().requires_grad_()
    dy = torch.randn(3, 16, 5, 5)

    out_a = fused_bn.bn_act(bn_a, x_a, relu=relu, residual=id_a if res else None)
    assert fused_bn.last_path == "stock"
    ref = bn_b(x_b)
    if res:
        ref = ref + id_b
    if relu:
        ref = F.relu(ref)
    assert torch.equal(out_a, ref)
    out_a.backward(dy)
    ref.backward(dy)
    assert torch.equal(x_a.grad, x_b.grad)
    assert torch.equal(bn_a.weight.grad, bn_b.weight.grad)
    assert torch.equal(bn_a.bias.grad, bn_b.bias.grad)
    if res:
        assert torch.equal(id_a.grad, id_b.grad)
    assert torch.equal(bn_a.running_mean, bn_b.running_mean)
    assert torch.equal(bn_a.running_var, bn_b.running_var)
    assert int(bn_a.num_batches_tracked) == int(bn_b.num_batches_tracked) == 1


def _expected_keys(block_bns, layers, expansion):
    keys = ["conv1.weight"] + [f"bn1.{s}" for s in _BN]
    inplanes = 64
    for li, n in enumerate(layers, 1):
        planes = 64 * 2 ** (li - 1)
        for b in range(n):
            p = f"layer{li}.{b}."
            for k in range(1, block_bns + 1):
                keys.append(f"{p}conv{k}.weight")
                keys += [f"{p}bn{k}.{s}" for s in _BN]
            if b == 0 and (li > 1 or inplanes != planes * expansion):
                keys.append(f"{p}downsample.0.weight")
                keys += [f"{p}downsample.1.{s}" for s in _BN]
        inplanes = planes * expansion
    return keys + ["fc.weight", "fc.bias"]


_BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


@pytest.mark.parametrize("name,block_bns,layers,expansion", [
    ("resnet18", 2, [2, 2, 2, 2], 1), ("resnet50", 3, [3, 4, 6, 3], 4), ("resnet152", 3, [3, 8, 36, 3], 4),
    ("micro", 2, [1, 1, 1, 1], 1)])
def test_models_keep_their_state_dict_keys(name, block_bns, layers, expansion):
    with torch.device("meta"):
        model = MODELS[name](num_classes=10)
    assert list(model.state_dict().keys()) == _expected_keys(block_bns, layers, expansion)
    # the ReLU modules stay registered too (module names are part of the layout)
    assert isinstance(model.relu, nn.ReLU) and isinstance(model.layer1[0].relu, nn.ReLU)


def test_resnet18_forward_backward_on_cpu():
    torch.manual_seed(0)
    model = MODELS["resnet18"](num_classes=10, width=16)
    x = torch.randn(2, 3, 32, 32)
    loss = F.cross_entropy(model(x), torch.tensor([1, 7]))
    loss.backward()
    assert fused_bn.last_path == "stock"
    assert torch.isfinite(loss)
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert int(model.bn1.num_batches_tracked) == 1
