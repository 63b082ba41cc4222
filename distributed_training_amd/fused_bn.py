"""BatchNorm2d (+ residual add) (+ ReLU) with libgsync's fused NHWC backward.

``bn_act(bn, x, relu=True, residual=None)`` computes ``relu(bn(x) + residual)``
(either part optional) for a ``nn.BatchNorm2d`` in training mode.

Forward: the BatchNorm itself is ATen's — ``torch._batch_norm_impl_index``, the
entry ``F.batch_norm`` dispatches through (MIOpen on this platform) — with
``nn.BatchNorm2d.forward``'s bookkeeping, so the output, the running statistics
and ``num_batches_tracked`` are bit for bit the stock module's.  The tail is the
in-place ReLU, or one ``gs_add_relu_fwd`` launch for add + ReLU (bit-identical to
``add_`` then ``relu_``).

Backward: two launches, ``gs_bn_bwd_reduce`` and ``gs_bn_bwd_dx``
(csrc/gs_bn_kernels.hip), which take the ReLU mask from the saved output instead
of a separate threshold_backward pass and, for a residual block, write the
masked gradient once: it is the identity branch's gradient and the dx pass's
input.  Saved for backward are x, y, weight, mean and invstd — what the stock
path keeps alive too.  Deterministic, no host synchronisation, capturable.

The fused path engages only for: CUDA, training mode, 4-D channels_last bf16
input, fp32 affine weights, C % 8 == 0, no forward hooks on the module, the
library loaded, and ``GSYNC_FUSED_BN`` not ``0``.  Everything else (CPU, fp32,
eval, bf16 weights, NCHW) runs the stock modules.  ``last_path`` names the path
the latest call took: ``"fused"`` or ``"stock"``.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib as L

last_path: str | None = None

_CL = torch.channels_last
_partials: dict = {}  # (R, C) -> P


def _n_partials(R: int, C: int) -> int:
    P = _partials.get((R, C))
    if P is None:
        P = _partials[(R, C)] = L.check(L.lib().gs_bn_bwd_partials(R, C), "gs_bn_bwd_partials")
    return P


def _eligible(bn, x, relu, residual) -> bool:
    if os.environ.get("GSYNC_FUSED_BN", "1") == "0":
        return False
    if not (x.is_cuda and bn.training and x.dim() == 4 and x.dtype == torch.bfloat16 and x.numel() > 0):
        return False
    w, b = bn.weight, bn.bias
    if w is None or b is None or w.dtype != torch.float32 or b.dtype != torch.float32:
        return False
    if x.shape[1] % 8 != 0 or not x.is_contiguous(memory_format=_CL):
        return False
    if bn._forward_pre_hooks or bn._forward_hooks:  # e.g. ZeRO's all-gather waits: keep the module call
        return False
    if residual is not None and not (relu and residual.shape == x.shape and residual.dtype == x.dtype
                                     and residual.device == x.device and residual.is_contiguous(memory_format=_CL)):
        return False
    return L.available()


class _BnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, bn, momentum, relu):
        y, mean, invstd, _, _ = torch._batch_norm_impl_index(
            x, weight, bias, bn.running_mean, bn.running_var, True, momentum, bn.eps, torch.backends.cudnn.enabled)
        if not y.is_contiguous(memory_format=_CL):
            raise RuntimeError("fused_bn: batch_norm returned a layout other than its channels_last input's")
        if residual is not None:
            L.check(L.lib().gs_add_relu_fwd(y.data_ptr(), residual.data_ptr(), y.numel(), L.stream_ptr(y.device)),
                    "gs_add_relu_fwd")
        elif relu:
            torch.relu_(y)
        ctx.relu = relu
        ctx.has_residual = residual is not None
        ctx.save_for_backward(x, weight, mean, invstd, y if relu else None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight, mean, invstd, y = ctx.saved_tensors
        if not dy.is_contiguous(memory_format=_CL):
            dy = dy.contiguous(memory_format=_CL)
        C = x.shape[1]
        R = x.numel() // C
        ws = torch.empty(_n_partials(R, C) * C * 2, dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        gw = torch.empty_like(weight)
        gb = torch.empty_like(weight)
        lib, stream = L.lib(), L.stream_ptr(x.device)
        yp = y.data_ptr() if ctx.relu else None
        g = None
        if ctx.has_residual:
            g = torch.empty_like(x)
            L.check(lib.gs_bn_bwd_reduce(x.data_ptr(), dy.data_ptr(), yp, g.data_ptr(), mean.data_ptr(),
                                         ws.data_ptr(), ws.numel(), R, C, stream), "gs_bn_bwd_reduce")
            dy, yp = g, None  # the dx pass reads the masked gradient
        else:
            L.check(lib.gs_bn_bwd_reduce(x.data_ptr(), dy.data_ptr(), yp, None, mean.data_ptr(), ws.data_ptr(),
                                         ws.numel(), R, C, stream), "gs_bn_bwd_reduce")
        L.check(lib.gs_bn_bwd_dx(x.data_ptr(), dy.data_ptr(), yp, mean.data_ptr(), invstd.data_ptr(),
                                 weight.data_ptr(), ws.data_ptr(), ws.numel(), dx.data_ptr(), gw.data_ptr(),
                                 gb.data_ptr(), R, C, stream), "gs_bn_bwd_dx")
        return dx, gw, gb, g, None, None, None


def bn_act(bn, x, relu: bool = True, residual=None):
    """``relu(bn(x) + residual)``; ``relu=False`` / ``residual=None`` drop that part."""
    global last_path
    if _eligible(bn, x, relu, residual):
        # nn.BatchNorm2d.forward's bookkeeping (T:nn/modules/batchnorm.py, _BatchNorm.forward)
        momentum = 0.0 if bn.momentum is None else bn.momentum
        if bn.track_running_stats and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
            if bn.momentum is None:
                momentum = 1.0 / float(bn.num_batches_tracked)
        last_path = "fused"
        return _BnAct.apply(x, bn.weight, bn.bias, residual, bn, momentum, relu)
    last_path = "stock"
    out = bn(x)
    if residual is not None:
        out += residual
    return F.relu(out, inplace=True) if relu else out
