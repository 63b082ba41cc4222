"""The training criterion: cross-entropy with label smoothing in three launches.

``CrossEntropyLoss`` and ``cross_entropy`` have ``torch.nn.CrossEntropyLoss``'s and
``F.cross_entropy``'s signatures.  For ``[B, K]`` logits (fp32, bf16 or fp16, on the CPU or a
HIP device) against integer class labels ``[B]``, with no class weights, the loss is one
autograd ``Function`` over ``gs_xent_fwd`` and ``gs_xent_bwd`` (include/gsync.h): one wavefront
per row forward, one workgroup that folds the rows in a fixed order, one backward kernel that
writes the gradient in the logits' dtype.  No ``[B, K]`` fp32 temporary is made and nothing is
read back; scratch (16 bytes per row) comes from torch's allocator per call, so the criterion
can be recorded into a hipGraph.

Differences from torch, both on the fused path only:

* the loss is **fp32** whatever the logits' dtype.  That is what torch returns under
  autocast (it casts the logits to fp32 first); without autocast torch would return a bf16
  loss for bf16 logits.  The gradient has the logits' dtype either way.
* a label outside ``[0, K)`` that is not ``ignore_index`` does not assert on the device: the
  reduced loss is NaN (``"none"``: that row's loss is 0) and the row's gradient is zero.

A ``MixedTarget`` (data.py: the pair targets of a MixUp / CutMix batch, two labels and one weight per row)
in place of the labels runs ``gs_xent_mix_fwd`` / ``gs_xent_mix_bwd`` under the same conditions, in the same
three launches; the three tensors are read on the device, so a captured criterion replays with new targets.
A row with ``lam == 1`` or equal labels is bit for bit the one-label row.  ``metrics`` count top-k against a
row's dominant label (``a`` if ``lam >= 0.5`` else ``b``) and add the unsmoothed mixed loss.  Off the fused
path a ``MixedTarget`` is the torch composition ``lam * CE(z, a, "none") + (1 - lam) * CE(z, b, "none")``
reduced over the counted rows (those where neither label is ``ignore_index``).

Everything else (class-probability targets, ``weight``, inputs of more than two dimensions, the
legacy ``size_average`` / ``reduce`` arguments) and ``GSYNC_FUSED_LOSS=0`` run
``F.cross_entropy``.  ``last_path`` names the path of the last call: ``"fused"`` or ``"torch"``.
Double backward is not supported on the fused path.

``metrics``: a ``Metrics`` (evaluation.py) that every forward in training mode advances by the
batch's rows, top-k hits and **unsmoothed** loss, inside ``gs_xent_fwd`` on the fused path, so a
training loop reports its running loss and accuracy from one ``metrics.compute()`` per epoch and
never reads the device in between.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib as L
from .data import MixedTarget
from .evaluation import Metrics

last_path: str | None = None

_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}
_FLOATS = (torch.float32, torch.bfloat16, torch.float16)
_INTS = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8)


def _rows_of(t: torch.Tensor) -> tuple[torch.Tensor, int]:
    """``t`` [B, K] as the library reads it (unit column stride, row stride >= K) and its row stride"""
    B, K = t.shape
    if t.stride(1) != 1 or (B > 1 and t.stride(0) < K):
        t = t.contiguous()
    return t, (t.stride(0) if B > 1 else K)


class _FusedCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, eps, reduction, metrics):
        B, K = logits.shape
        z, stride = _rows_of(logits.detach())
        mixed = isinstance(target, MixedTarget)
        if mixed:
            labels = target.labels_a.to(torch.int64).contiguous()
            pair = (target.labels_b.to(torch.int64).contiguous(), target.lam.contiguous())
        else:
            labels, pair = target.to(torch.int64).contiguous(), ()
        # rows (16 bytes each), then the 16 bytes of the reduced result
        scratch = torch.empty(4 * (B + 1), dtype=torch.float32, device=z.device)
        kind, dt, stream = L.device_kind(z), L.gs_dtype(z.dtype), L.stream_ptr(z.device)
        red_ptr = scratch.data_ptr() + 16 * B
        topk, n_topk, acc = (None, 0, None) if metrics is None else (metrics._topk, len(metrics.topk),
                                                                      metrics._acc.data_ptr())
        if mixed:
            L.check(L.lib().gs_xent_mix_fwd(kind, z.data_ptr(), dt, labels.data_ptr(), pair[0].data_ptr(),
                                            pair[1].data_ptr(), B, K, stride, ignore_index, eps, scratch.data_ptr(),
                                            red_ptr, topk, n_topk, acc, stream), "gs_xent_mix_fwd")
        else:
            L.check(L.lib().gs_xent_fwd(kind, z.data_ptr(), dt, labels.data_ptr(), B, K, stride, ignore_index, eps,
                                        scratch.data_ptr(), red_ptr, topk, n_topk, acc, stream), "gs_xent_fwd")
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(z, labels, scratch, *pair)
            ctx.args = (stride, ignore_index, eps, reduction)
        if reduction == 0:
            return scratch[:4 * B].view(B, 4)[:, 0]
        return scratch[4 * B + (1 if reduction == 1 else 0)]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        z, labels, scratch, *pair = ctx.saved_tensors
        stride, ignore_index, eps, reduction = ctx.args
        B, K = z.shape
        g = grad_out.to(torch.float32).contiguous()
        dz = torch.empty((B, K), dtype=z.dtype, device=z.device)
        if pair:
            L.check(L.lib().gs_xent_mix_bwd(L.device_kind(z), z.data_ptr(), L.gs_dtype(z.dtype), labels.data_ptr(),
                                            pair[0].data_ptr(), pair[1].data_ptr(), B, K, stride, ignore_index, eps,
                                            reduction, scratch.data_ptr(), scratch.data_ptr() + 16 * B, g.data_ptr(),
                                            dz.data_ptr(), K, L.stream_ptr(z.device)), "gs_xent_mix_bwd")
            return dz, None, None, None, None, None
        L.check(L.lib().gs_xent_bwd(L.device_kind(z), z.data_ptr(), L.gs_dtype(z.dtype), labels.data_ptr(), B, K, stride,
                                    ignore_index, eps, reduction, scratch.data_ptr(), scratch.data_ptr() + 16 * B,
                                    g.data_ptr(), dz.data_ptr(), K, L.stream_ptr(z.device)), "gs_xent_bwd")
        return dz, None, None, None, None, None


def _labels_ok(input, t) -> bool:
    return t.dim() == 1 and t.dtype in _INTS and t.shape[0] == input.shape[0] and t.device == input.device


def _fusable(input, target, weight, size_average, reduce, reduction, label_smoothing) -> bool:
    if isinstance(target, MixedTarget):
        lam = target.lam
        target_ok = (input.dim() == 2 and _labels_ok(input, target.labels_a) and _labels_ok(input, target.labels_b)
                     and lam.dim() == 1 and lam.dtype == torch.float32 and lam.shape[0] == input.shape[0]
                     and lam.device == input.device)
    else:
        target_ok = input.dim() == 2 and _labels_ok(input, target)
    return (os.environ.get("GSYNC_FUSED_LOSS", "1") != "0"
            and weight is None and size_average is None and reduce is None and reduction in _REDUCTIONS
            and input.dim() == 2 and input.shape[1] >= 1 and input.dtype in _FLOATS
            and input.device.type in ("cpu", "cuda") and target_ok and 0.0 <= label_smoothing <= 1.0)


def _torch_mixed(input, target, weight, size_average, ignore_index, reduce, reduction, label_smoothing):
    """the torch composition of a MixedTarget: the two per-row losses blended, reduced over the counted rows"""
    if size_average is not None or reduce is not None:
        reduction = torch.nn._reduction.legacy_get_string(size_average, reduce)
    a, b = target.labels_a, target.labels_b
    lam = target.lam.to(input.dtype if input.dtype.is_floating_point else torch.float32)
    la = F.cross_entropy(input, a, weight, ignore_index=ignore_index, reduction="none", label_smoothing=label_smoothing)
    lb = F.cross_entropy(input, b, weight, ignore_index=ignore_index, reduction="none", label_smoothing=label_smoothing)
    counted = (a != ignore_index) & (b != ignore_index)
    rows = torch.where(counted, lam * la + (1 - lam) * lb, torch.zeros_like(la))
    if reduction == "none":
        return rows
    if reduction == "sum":
        return rows.sum()
    return rows.sum() / counted.sum()


def cross_entropy(input, target, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean",
                  label_smoothing=0.0, *, metrics: Metrics | None = None):
    """``F.cross_entropy`` with the fused path of this module (see the module's docstring).  ``metrics``, if
    given, is advanced by this batch."""
    global last_path
    if metrics is not None and metrics.ignore_index != ignore_index:
        raise ValueError("cross_entropy: metrics.ignore_index differs from ignore_index")
    if _fusable(input, target, weight, size_average, reduce, reduction, label_smoothing):
        if metrics is not None and metrics.device != input.device:
            raise ValueError(f"cross_entropy: metrics live on {metrics.device}, the logits on {input.device}")
        last_path = "fused"
        return _FusedCrossEntropy.apply(input, target, int(ignore_index), float(label_smoothing),
                                        _REDUCTIONS[reduction], metrics)
    last_path = "torch"
    if isinstance(target, MixedTarget):
        if metrics is not None:
            dominant = torch.where(target.lam >= 0.5, target.labels_a, target.labels_b)
            skipped = (target.labels_a == ignore_index) | (target.labels_b == ignore_index)
            metrics.update(input.detach(), torch.where(skipped, torch.full_like(dominant, ignore_index), dominant))
        return _torch_mixed(input, target, weight, size_average, ignore_index, reduce, reduction, label_smoothing)
    if metrics is not None:
        metrics.update(input.detach(), target)
    return F.cross_entropy(input, target, weight, size_average, ignore_index, reduce, reduction, label_smoothing)


class CrossEntropyLoss(torch.nn.Module):
    """Drop-in for ``torch.nn.CrossEntropyLoss``; ``metrics`` is advanced by every forward in training mode."""

    def __init__(self, weight=None, size_average=None, ignore_index: int = -100, reduce=None, reduction: str = "mean",
                 label_smoothing: float = 0.0, *, metrics: Metrics | None = None):
        super().__init__()
        if metrics is not None and metrics.ignore_index != ignore_index:
            raise ValueError("CrossEntropyLoss: metrics.ignore_index differs from ignore_index")
        self.register_buffer("weight", weight)
        self.size_average = size_average
        self.reduce = reduce
        self.ignore_index = ignore_index
        self.reduction = reduction
        self.label_smoothing = label_smoothing
        self.metrics = metrics

    def forward(self, input, target):
        return cross_entropy(input, target, self.weight, self.size_average, self.ignore_index, self.reduce,
                             self.reduction, self.label_smoothing, metrics=self.metrics if self.training else None)
