"""torchvision-0.15-equivalent ResNet-18/50/152 (torchvision is absent here).

The reference builds ``torchvision.models.resnet18(num_classes=10)``
(R:resnet/pytorch_ddp/ddp_train.py:95, deepspeed_train.py:223,
colossal_train.py:149); the BASELINE configs use ResNet-50/152.  This module
restates that topology (v1.5: stride on the 3x3 conv of the bottleneck) with
the same module names, so ``state_dict`` keys — the checkpoint layout — are
identical (``conv1.weight``, ``bn1.running_mean``, ``layer1.0.downsample.0.weight``,
``fc.bias`` ...), and the same initialisation (kaiming_normal_ fan_out for
convs, BN weight 1 / bias 0, default Linear init).  ``width`` scales every
channel count for the small parity fixtures.

Every BatchNorm runs through ``fused_bn.bn_act`` together with the ReLU and the
residual add that follow it: on an MI355X training step (bf16, channels_last)
that takes libgsync's fused backward kernels; everywhere else it is the stock
``relu(bn(x) + identity)``.

A block's output has two consumers, the next block's first convolution and its
identity (or downsample) branch.  ``ResNet.forward`` therefore drives the blocks
of ``layer1..4`` through ``forward_pair``: every block but the last returns its
output as the pair ``bn_act(..., fork=True)`` gives, whose two gradients the
fused BatchNorm backward sums in its first pass (no separate add).  Called with
one tensor, a block or a layer is what it always was.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .fused_bn import bn_act, bn_relu_pool


def conv3x3(in_planes, out_planes, stride=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=False)


def conv1x1(in_planes, out_planes, stride=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=1, stride=stride, bias=False)


def _downsample(seq, x):
    """The block's downsample branch, Sequential(conv1x1, BatchNorm2d): the BN through bn_act."""
    return bn_act(seq[1], seq[0](x), relu=False)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(planes, planes)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward_pair(self, pair, fork_out):
        """pair: the input twice (main path, identity path); fork_out: return the output as a pair too"""
        x, identity = pair
        if self.downsample is not None:
            identity = _downsample(self.downsample, identity)
        out = bn_act(self.bn1, self.conv1(x))
        return bn_act(self.bn2, self.conv2(out), residual=identity, fork=fork_out)

    def forward(self, x):
        return self.forward_pair((x, x), False)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv1x1(inplanes, planes)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = conv3x3(planes, planes, stride)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = conv1x1(planes, planes * self.expansion)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward_pair(self, pair, fork_out):
        """pair: the input twice (main path, identity path); fork_out: return the output as a pair too"""
        x, identity = pair
        if self.downsample is not None:
            identity = _downsample(self.downsample, identity)
        out = bn_act(self.bn1, self.conv1(x))
        out = bn_act(self.bn2, self.conv2(out))
        return bn_act(self.bn3, self.conv3(out), residual=identity, fork=fork_out)

    def forward(self, x):
        return self.forward_pair((x, x), False)


class ResNet(nn.Module):
    def __init__(self, block, layers, num_classes=1000, width=64):
        super().__init__()
        self.inplanes = width
        self.conv1 = nn.Conv2d(3, self.inplanes, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(self.inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, width, layers[0])
        self.layer2 = self._make_layer(block, width * 2, layers[1], stride=2)
        self.layer3 = self._make_layer(block, width * 4, layers[2], stride=2)
        self.layer4 = self._make_layer(block, width * 8, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(width * 8 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                conv1x1(self.inplanes, planes * block.expansion, stride),
                nn.BatchNorm2d(planes * block.expansion),
            )
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes))
        return nn.Sequential(*layers)

    def _hooked(self):
        """a forward hook on a layer or a block: only their own calls run it"""
        return any(m._forward_hooks or m._forward_pre_hooks
                   for layer in (self.layer1, self.layer2, self.layer3, self.layer4) for m in (layer, *layer))

    def forward(self, x):
        x = self.conv1(x)
        if self._hooked():
            x = bn_relu_pool(self.bn1, x, self.maxpool, fork=False)
            x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        else:
            blocks = [b for layer in (self.layer1, self.layer2, self.layer3, self.layer4) for b in layer]
            pair = bn_relu_pool(self.bn1, x, self.maxpool, fork=True)
            for b in blocks[:-1]:
                pair = b.forward_pair(pair, True)
            x = blocks[-1].forward_pair(pair, False)
        x = torch.flatten(self.avgpool(x), 1)
        return self.fc(x)


def resnet18(num_classes=1000, width=64, **_):
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes, width)


def resnet50(num_classes=1000, width=64, **_):
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, width)


def resnet152(num_classes=1000, width=64, **_):
    return ResNet(Bottleneck, [3, 8, 36, 3], num_classes, width)


def micro_resnet(num_classes=10, width=8):
    """BasicBlock [1,1,1,1] at width 8: the full-tensor parity fixture model."""
    return ResNet(BasicBlock, [1, 1, 1, 1], num_classes, width)


MODELS = {"resnet18": resnet18, "resnet50": resnet50, "resnet152": resnet152, "micro": micro_resnet}
