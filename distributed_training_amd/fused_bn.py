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

``fork=True`` returns the output as two tensors over one storage, for an output
with two consumers (a residual block's: the next block's first convolution and
its identity branch).  Autograd then hands ``backward`` the two gradients
unsummed and ``gs_bn_bwd_reduce_fork`` adds them (bf16 round-to-nearest, ATen's
``add``) in the pass that reads them anyway.  ``bn_relu_pool(bn, x, pool)`` is
the stem: the BatchNorm forward, then ``gs_relu_maxpool_fwd`` pools over relu(.)
and keeps a byte per output (no in-place ReLU pass, no int64 indices); backward,
``gs_maxpool_bwd`` writes the BatchNorm's dy once from those bytes and the one
or two pooled gradients (no zero fill, no atomics, no add).

The ReLU mask travels as bits (``GSYNC_BN_MASK``, default ``1``): the forward tail — ``gs_relu_mask_fwd`` in place
of ``relu_``, ``gs_add_relu_mask_fwd``, ``gs_relu_maxpool_mask_fwd`` — also writes one byte per 8 elements
(bit j set iff the element is not <= 0), that ``uint8`` tensor of ``numel / 8`` bytes is saved in place of ``y``,
and ``gs_bn_bwd_reduce_bits`` / ``gs_bn_bwd_reduce_fork_bits`` / ``gs_bn_bwd_dx_bits`` read a byte where they read
16 of ``y``.  Every result is bit for bit the same; ``GSYNC_BN_MASK=0`` runs the calls described above.

The fused path engages only for: CUDA, training mode, 4-D channels_last bf16
input, fp32 affine weights, C % 8 == 0, no forward hooks on the module, the
library loaded, and ``GSYNC_FUSED_BN`` not ``0``.  Everything else (CPU, fp32,
eval, bf16 weights, NCHW) runs the stock modules.  ``last_path`` names the path
the latest call took: ``"fused"``, ``"fused_eval"`` or ``"stock"``.

Evaluation: inside ``fused_eval()`` an eval-mode call that needs no gradient (grad mode
off, or neither the input nor the parameters require grad), on a module with running
statistics and under the conditions above, is one launch: ``gs_bn_infer_act`` reads x
(and the identity) and writes ``relu(x * s + t + identity)`` rounded to bf16 once, s and
t formed from the live running statistics inside the kernel; the stem is
``gs_bn_infer_relu_maxpool`` (no un-pooled output, no indices).  The output is out of
place; ``fork=True`` returns it twice.  Outside the context, and for every training-mode
call inside it, nothing changes.
"""
from __future__ import annotations

import contextlib
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


def _mask_bits() -> bool:
    """the ReLU mask as one bit per element instead of the saved bf16 output (``GSYNC_BN_MASK``, default on)"""
    return os.environ.get("GSYNC_BN_MASK", "1") != "0"


def _eligible(bn, x, relu, residual) -> bool:
    return bn.training and _shape_eligible(bn, x, relu, residual)


def _shape_eligible(bn, x, relu, residual) -> bool:
    """what the training path and the evaluation path both ask of a call"""
    if os.environ.get("GSYNC_FUSED_BN", "1") == "0":
        return False
    if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16 and x.numel() > 0):
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


_fused_eval = False


@contextlib.contextmanager
def fused_eval(enabled: bool = True):
    """Inside, an eval-mode ``bn_act`` / ``bn_relu_pool`` call that needs no gradient runs the one-pass
    inference kernels (``gs_bn_infer_act``, ``gs_bn_infer_relu_maxpool``).  Off by default; training-mode
    calls are not affected.  ``evaluation.evaluate`` enters it."""
    global _fused_eval
    prev, _fused_eval = _fused_eval, bool(enabled)
    try:
        yield
    finally:
        _fused_eval = prev


def _eval_eligible(bn, x, relu, residual) -> bool:
    if not _fused_eval or bn.training:
        return False
    rm, rv = bn.running_mean, bn.running_var
    if rm is None or rv is None or rm.dtype != torch.float32 or rv.dtype != torch.float32:
        return False  # no running statistics: an eval-mode call normalises with the batch's
    if not _shape_eligible(bn, x, relu, residual):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or bn.weight.requires_grad or bn.bias.requires_grad
                                    or (residual is not None and residual.requires_grad)):
        return False  # the inference kernels have no backward
    ptrs = [x.data_ptr(), rm.data_ptr(), rv.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr()]
    if residual is not None:
        ptrs.append(residual.data_ptr())
    return all(p % 16 == 0 for p in ptrs)


def _infer_act(bn, x, relu, residual):
    y = torch.empty_like(x)  # out of place: x may be another consumer's input
    C = x.shape[1]
    L.check(L.lib().gs_bn_infer_act(x.data_ptr(), None if residual is None else residual.data_ptr(),
                                    bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.weight.data_ptr(),
                                    bn.bias.data_ptr(), bn.eps, int(bool(relu)), y.data_ptr(), x.numel() // C, C,
                                    L.stream_ptr(x.device)), "gs_bn_infer_act")
    return y


def _infer_relu_pool(bn, x):
    N, C, H, W = x.shape
    out = torch.empty((N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=x.dtype, device=x.device, memory_format=_CL)
    L.check(L.lib().gs_bn_infer_relu_maxpool(x.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                                             bn.weight.data_ptr(), bn.bias.data_ptr(), bn.eps, out.data_ptr(), N, H,
                                             W, C, L.stream_ptr(x.device)), "gs_bn_infer_relu_maxpool")
    return out


class _BnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, bn, momentum, relu, fork=False):
        y, mean, invstd, _, _ = torch._batch_norm_impl_index(
            x, weight, bias, bn.running_mean, bn.running_var, True, momentum, bn.eps, torch.backends.cudnn.enabled)
        if not y.is_contiguous(memory_format=_CL):
            raise RuntimeError("fused_bn: batch_norm returned a layout other than its channels_last input's")
        mask = None
        if relu and _mask_bits():
            mask = torch.empty(y.numel() // 8, dtype=torch.uint8, device=y.device)
        if residual is not None and mask is not None:
            L.check(L.lib().gs_add_relu_mask_fwd(y.data_ptr(), residual.data_ptr(), mask.data_ptr(), y.numel(),
                                                 L.stream_ptr(y.device)), "gs_add_relu_mask_fwd")
        elif residual is not None:
            L.check(L.lib().gs_add_relu_fwd(y.data_ptr(), residual.data_ptr(), y.numel(), L.stream_ptr(y.device)),
                    "gs_add_relu_fwd")
        elif mask is not None:
            L.check(L.lib().gs_relu_mask_fwd(y.data_ptr(), mask.data_ptr(), y.numel(), L.stream_ptr(y.device)),
                    "gs_relu_mask_fwd")
        elif relu:
            torch.relu_(y)
        ctx.relu = relu
        ctx.bits = mask is not None
        ctx.has_residual = residual is not None
        # the mask in place of y (the next convolution keeps y alive anyway)
        ctx.save_for_backward(x, weight, mean, invstd, mask if mask is not None else (y if relu else None))
        if fork:
            # two tensors over one storage: autograd hands backward their gradients unsummed
            ctx.set_materialize_grads(False)
            return y, y.view_as(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, dy_b=None):
        x, weight, mean, invstd, y = ctx.saved_tensors
        if dy is None:
            dy, dy_b = dy_b, None
        if dy is None:  # neither half of a fork was used
            return None, None, None, None, None, None, None, None
        if not dy.is_contiguous(memory_format=_CL):
            dy = dy.contiguous(memory_format=_CL)
        if dy_b is not None and not dy_b.is_contiguous(memory_format=_CL):
            dy_b = dy_b.contiguous(memory_format=_CL)
        C = x.shape[1]
        R = x.numel() // C
        ws = torch.empty(_n_partials(R, C) * C * 2, dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        gw = torch.empty_like(weight)
        gb = torch.empty_like(weight)
        lib, stream = L.lib(), L.stream_ptr(x.device)
        yp = y.data_ptr() if ctx.relu else None  # y: the saved output, or its mask bits (ctx.bits)
        bits = ctx.bits
        g = None
        if dy_b is not None:
            # the fork's sum, the mask and the sums in one pass; g is what ATen's add + threshold_backward left
            g = torch.empty_like(x)
            fn = "gs_bn_bwd_reduce_fork_bits" if bits else "gs_bn_bwd_reduce_fork"
            L.check(getattr(lib, fn)(x.data_ptr(), dy.data_ptr(), dy_b.data_ptr(), yp, g.data_ptr(), mean.data_ptr(),
                                     ws.data_ptr(), ws.numel(), R, C, stream), fn)
            dy, yp = g, None
        elif ctx.has_residual:
            g = torch.empty_like(x)
            fn = "gs_bn_bwd_reduce_bits" if bits else "gs_bn_bwd_reduce"
            L.check(getattr(lib, fn)(x.data_ptr(), dy.data_ptr(), yp, g.data_ptr(), mean.data_ptr(), ws.data_ptr(),
                                     ws.numel(), R, C, stream), fn)
            dy, yp = g, None  # the dx pass reads the masked gradient
        else:
            fn = "gs_bn_bwd_reduce_bits" if bits else "gs_bn_bwd_reduce"
            L.check(getattr(lib, fn)(x.data_ptr(), dy.data_ptr(), yp, None, mean.data_ptr(), ws.data_ptr(),
                                     ws.numel(), R, C, stream), fn)
        fn = "gs_bn_bwd_dx_bits" if bits and yp is not None else "gs_bn_bwd_dx"
        L.check(getattr(lib, fn)(x.data_ptr(), dy.data_ptr(), yp, mean.data_ptr(), invstd.data_ptr(),
                                 weight.data_ptr(), ws.data_ptr(), ws.numel(), dx.data_ptr(), gw.data_ptr(),
                                 gb.data_ptr(), R, C, stream), fn)
        return dx, gw, gb, g if ctx.has_residual else None, None, None, None, None


class _BnReluPool(torch.autograd.Function):
    """MaxPool2d(3, 2, 1)(relu(bn(x))): the ReLU is taken while pooling, the BatchNorm output stays
    un-ReLU'd (its sign is the ReLU mask), the pool keeps one byte per output instead of int64 indices.
    With ``GSYNC_BN_MASK`` the pool also writes that mask as bits, which are saved in place of the output."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn, momentum, fork):
        y, mean, invstd, _, _ = torch._batch_norm_impl_index(
            x, weight, bias, bn.running_mean, bn.running_var, True, momentum, bn.eps, torch.backends.cudnn.enabled)
        if not y.is_contiguous(memory_format=_CL):
            raise RuntimeError("fused_bn: batch_norm returned a layout other than its channels_last input's")
        N, C, H, W = y.shape
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        out = torch.empty((N, C, OH, OW), dtype=y.dtype, device=y.device, memory_format=_CL)
        idx = torch.empty((N, OH, OW, C), dtype=torch.uint8, device=y.device)
        ctx.bits = _mask_bits()
        if ctx.bits:
            mask = torch.empty(y.numel() // 8, dtype=torch.uint8, device=y.device)
            L.check(L.lib().gs_relu_maxpool_mask_fwd(y.data_ptr(), out.data_ptr(), idx.data_ptr(), mask.data_ptr(), N,
                                                     H, W, C, L.stream_ptr(y.device)), "gs_relu_maxpool_mask_fwd")
            y = mask
        else:
            L.check(L.lib().gs_relu_maxpool_fwd(y.data_ptr(), out.data_ptr(), idx.data_ptr(), N, H, W, C,
                                                L.stream_ptr(y.device)), "gs_relu_maxpool_fwd")
        ctx.save_for_backward(x, weight, mean, invstd, y, idx)
        if fork:
            ctx.set_materialize_grads(False)
            return out, out.view_as(out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_a, d_b=None):
        x, weight, mean, invstd, y, idx = ctx.saved_tensors
        if d_a is None:
            d_a, d_b = d_b, None
        if d_a is None:
            return None, None, None, None, None, None
        if not d_a.is_contiguous(memory_format=_CL):
            d_a = d_a.contiguous(memory_format=_CL)
        if d_b is not None and not d_b.is_contiguous(memory_format=_CL):
            d_b = d_b.contiguous(memory_format=_CL)
        N, C, H, W = x.shape
        R = N * H * W
        lib, stream = L.lib(), L.stream_ptr(x.device)
        dy = torch.empty_like(x)
        L.check(lib.gs_maxpool_bwd(d_a.data_ptr(), None if d_b is None else d_b.data_ptr(), idx.data_ptr(),
                                   dy.data_ptr(), N, H, W, C, stream), "gs_maxpool_bwd")
        ws = torch.empty(_n_partials(R, C) * C * 2, dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        gw = torch.empty_like(weight)
        gb = torch.empty_like(weight)
        fn = "gs_bn_bwd_reduce_bits" if ctx.bits else "gs_bn_bwd_reduce"  # y: the output, or its mask bits
        L.check(getattr(lib, fn)(x.data_ptr(), dy.data_ptr(), y.data_ptr(), None, mean.data_ptr(), ws.data_ptr(),
                                 ws.numel(), R, C, stream), fn)
        fn = "gs_bn_bwd_dx_bits" if ctx.bits else "gs_bn_bwd_dx"
        L.check(getattr(lib, fn)(x.data_ptr(), dy.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                 weight.data_ptr(), ws.data_ptr(), ws.numel(), dx.data_ptr(), gw.data_ptr(),
                                 gb.data_ptr(), R, C, stream), fn)
        return dx, gw, gb, None, None, None


def _bookkeeping(bn) -> float:
    """nn.BatchNorm2d.forward's bookkeeping (T:nn/modules/batchnorm.py, _BatchNorm.forward) -> momentum"""
    momentum = 0.0 if bn.momentum is None else bn.momentum
    if bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
        if bn.momentum is None:
            momentum = 1.0 / float(bn.num_batches_tracked)
    return momentum


def _pool_eligible(pool) -> bool:
    def is_(v, k):
        return v == k or v == (k, k) or v == [k, k]

    return (type(pool) is torch.nn.MaxPool2d and is_(pool.kernel_size, 3) and is_(pool.stride, 2)
            and is_(pool.padding, 1) and is_(pool.dilation, 1) and not pool.ceil_mode and not pool.return_indices
            and not (pool._forward_pre_hooks or pool._forward_hooks))


def bn_relu_pool(bn, x, pool, fork: bool = True):
    """``pool(relu(bn(x)))`` for the stem; ``fork`` as in ``bn_act``.

    Fused (under ``bn_act``'s conditions, for a hook-free ``MaxPool2d(3, 2, 1)``): the BatchNorm forward,
    then one launch that pools over relu(.) and keeps the winner's window position in a byte; backward,
    one launch from those bytes and the one or two pooled gradients to the BatchNorm backward's dy.
    Anything else is the stock ``pool(bn_act(bn, x))``."""
    global last_path
    if _pool_eligible(pool) and _eval_eligible(bn, x, True, None):
        last_path = "fused_eval"
        out = _infer_relu_pool(bn, x)
        return (out, out) if fork else out
    if _pool_eligible(pool) and _eligible(bn, x, True, None):
        momentum = _bookkeeping(bn)
        last_path = "fused"
        return _BnReluPool.apply(x, bn.weight, bn.bias, bn, momentum, fork)
    out = pool(bn_act(bn, x))
    return (out, out) if fork else out


def bn_act(bn, x, relu: bool = True, residual=None, fork: bool = False):
    """``relu(bn(x) + residual)``; ``relu=False`` / ``residual=None`` drop that part.

    ``fork=True`` returns the result twice, for a caller that feeds it to two consumers (a block's
    output: the next block's first convolution and its identity branch).  On the fused path the two
    tensors alias one storage and their gradients are summed inside the BatchNorm backward's first
    pass; on the stock path it is the same tensor twice and autograd sums as ever."""
    global last_path
    if _eval_eligible(bn, x, relu, residual):
        last_path = "fused_eval"
        out = _infer_act(bn, x, relu, residual)
        return (out, out) if fork else out
    if _eligible(bn, x, relu, residual):
        momentum = _bookkeeping(bn)
        last_path = "fused"
        return _BnAct.apply(x, bn.weight, bn.bias, residual, bn, momentum, relu, fork)
    last_path = "stock"
    out = bn(x)
    if residual is not None:
        out += residual
    if relu:
        out = F.relu(out, inplace=True)
    return (out, out) if fork else out
