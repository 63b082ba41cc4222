"""Distributed evaluation: exact metrics and the fused inference forward.

The reference trainers build a ``test_dataloader`` (``DistributedSampler``,
``drop_last=False``) and never drain it (R:resnet/pytorch_ddp/ddp_train.py:47,
R:resnet/colossalai/colossal_train.py:77).  This module is the loop they leave out.

``Metrics`` keeps the evaluation's sums on the model's device: ``update`` is one
``gs_eval_accumulate`` (include/gsync.h) per batch — the cross-entropy, the top-k
hits with a deterministic tie rule, integer counts — and nothing is read back until
``compute``.  ``reduce`` sums the accumulator over the ranks.

``evaluate(model, loader)`` runs the loop: eval mode (restored afterwards), no grad,
the one-pass inference BatchNorm kernels (``fused_bn.fused_eval``), and every dataset
sample counted once.  With ``drop_last=False`` a ``DistributedSampler`` pads each rank
to ``ceil(N / ws)`` samples by repeating samples from the front of the epoch's order;
rank r's sample at position p is global position ``r + p * ws``, real iff that is
below N, so the rank's first ``max(0, ceil((N - r) / ws))`` samples are the real ones
and the rest reach ``update`` as rows past ``n_valid``.  A hand-written loop counts the
padding twice and divides by ``ceil(N / ws) * ws``.
"""
from __future__ import annotations

import contextlib
import math

import torch
import torch.distributed as dist

from . import _lib as L
from . import fused_bn
from .comm import get_communicator


class Metrics:
    """Loss and top-k accuracy of a classification run, accumulated on ``device``.

    The accumulator is eight 8-byte words (``gs_eval_accumulate``): rows counted, rows
    with a label outside ``[0, K)``, the loss sum (fp64), a reserved word, and the rows
    correct at each of up to four ``topk`` values.  Ties go to the lower class index."""

    def __init__(self, topk=(1, 5), device=None, ignore_index: int = -100):
        self.topk = tuple(int(k) for k in topk)
        if not 0 < len(self.topk) <= 4 or any(k < 1 for k in self.topk):
            raise ValueError("topk: one to four values >= 1")
        self.device = torch.device("cpu" if device is None else device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.ignore_index = int(ignore_index)
        self._kind = L.GS_DEV_HIP if self.device.type == "cuda" else L.GS_DEV_HOST
        L.lib()  # a missing library is an error here, not at the first batch
        self._topk = L.i32_array(self.topk)
        self._acc = torch.zeros(8, dtype=torch.int64, device=self.device)
        self._ws = torch.empty(0, dtype=torch.int64, device=self.device)

    def reset(self) -> None:
        self._acc.zero_()

    def update(self, logits: torch.Tensor, labels: torch.Tensor, n_valid: int | None = None) -> None:
        """Adds ``logits`` [B, K] (fp32, bf16 or fp16) against ``labels`` [B]; rows from ``n_valid`` on are
        padding and are skipped.  One library call: no copy, no host read."""
        if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
            raise ValueError("Metrics.update: logits [B, K] and labels [B] expected")
        if logits.device != self.device or labels.device != self.device:
            raise ValueError(f"Metrics.update: tensors must live on {self.device}")
        B, K = logits.shape
        if K < 1:
            raise ValueError("Metrics.update: K >= 1 expected")
        if B == 0:
            return
        if logits.stride(1) != 1 or (B > 1 and logits.stride(0) < K):
            logits = logits.contiguous()
        if labels.dtype != torch.int64 or not labels.is_contiguous():
            labels = labels.to(torch.int64).contiguous()
        if self._ws.numel() < B:  # the scratch grows to the largest batch seen
            self._ws = torch.empty(B, dtype=torch.int64, device=self.device)
        n_valid = B if n_valid is None else int(n_valid)
        L.check(L.lib().gs_eval_accumulate(self._kind, logits.data_ptr(), L.gs_dtype(logits.dtype), labels.data_ptr(),
                                           B, K, logits.stride(0) if B > 1 else K, n_valid, self._topk,
                                           len(self.topk), self.ignore_index, self._ws.data_ptr(),
                                           self._acc.data_ptr(), L.stream_ptr(self.device)), "gs_eval_accumulate")

    def reduce(self, process_group=None) -> None:
        """Sums the accumulator over the ranks of ``process_group`` (no-op without a process group):
        the integer words in one SUM collective, the fp64 loss sum in another."""
        if not (dist.is_available() and dist.is_initialized()):
            return
        pg = dist.group.WORLD if process_group is None else process_group
        counts = self._acc.clone()
        counts[2] = 0
        loss = self._acc[2:3].view(torch.float64).clone()
        if self.device.type == "cuda" and dist.get_backend(pg) == "nccl":
            comm = get_communicator(None if pg is dist.group.WORLD else pg, self.device)
            stream = L.stream_ptr(self.device)
            comm.all_reduce(counts, "sum", stream=stream)
            comm.all_reduce(loss, "sum", stream=stream)
        elif self.device.type == "cuda":
            # device tensors over gloo (ranks sharing a GPU): staged through host memory, as DDP's buckets are
            hc, hl = counts.cpu(), loss.cpu()
            dist.all_reduce(hc, group=pg)
            dist.all_reduce(hl, group=pg)
            counts.copy_(hc)
            loss.copy_(hl)
        else:
            dist.all_reduce(counts, group=pg)
            dist.all_reduce(loss, group=pg)
        self._acc.copy_(counts)
        self._acc[2:3].view(torch.float64).copy_(loss)

    def compute(self) -> dict:
        """The one host read.  ``n`` and ``correct<k>`` are exact integers; ``loss`` is the mean
        cross-entropy and ``top<k>`` the fraction correct at k (NaN over no rows)."""
        acc = self._acc.cpu()
        n, bad = int(acc[0]), int(acc[1])
        if bad:
            raise ValueError(f"Metrics: {bad} label(s) outside [0, K) that are not ignore_index={self.ignore_index}")
        loss_sum = float(acc[2:3].view(torch.float64)[0])
        out = {"n": n, "loss": loss_sum / n if n else math.nan, "loss_sum": loss_sum}
        for i, k in enumerate(self.topk):
            c = int(acc[4 + i])
            out[f"correct{k}"] = c
            out[f"top{k}"] = c / n if n else math.nan
        return out


def _real_samples(loader) -> int | None:
    """How many of this rank's samples are dataset samples and not a DistributedSampler's padding
    (None: the loader's sampler pads nothing)."""
    from .data import DistributedSampler as OurSampler

    s = getattr(loader, "sampler", None)
    if not isinstance(s, (torch.utils.data.distributed.DistributedSampler, OurSampler)) or s.drop_last:
        return None
    n = len(s.dataset)
    return max(0, -((s.rank - n) // s.num_replicas))  # ceil((n - rank) / ws)


def _unwrap(model):
    from .ddp import DistributedDataParallel as OurDDP

    if isinstance(model, (OurDDP, torch.nn.parallel.DistributedDataParallel)):
        return model.module
    return model


def evaluate(model, loader, *, topk=(1, 5), process_group=None, autocast_dtype=None, fused: bool = True,
             dedup_padding: bool = True, max_batches: int | None = None) -> dict:
    """Evaluates ``model`` over ``loader`` and returns ``Metrics.compute()`` summed over the ranks.

    A ``DistributedDataParallel`` (this package's or torch's) is unwrapped, so the loop holds no
    collective and ranks may run different numbers of batches.  The model runs in eval mode under
    ``no_grad`` and ``fused_eval(fused)`` (and autocast to ``autocast_dtype`` if given); afterwards every
    module has the ``training`` flag it had.  Parameters, buffers and ``.grad`` are not touched.
    Batches are moved to the model's device (floating inputs to the parameters' dtype and memory
    format when autocast is off).  ``dedup_padding``: the samples a ``DistributedSampler`` with
    ``drop_last=False`` repeats to pad the ranks are not counted."""
    module = _unwrap(model)
    ref = next(iter(module.parameters()), None)
    if ref is None:
        ref = next(iter(module.buffers()), torch.empty(0))
    device = ref.device
    conv_like = next((p for p in module.parameters() if p.dim() == 4), None)
    channels_last = (conv_like is not None and conv_like.is_contiguous(memory_format=torch.channels_last)
                     and not conv_like.is_contiguous())
    metrics = Metrics(topk, device)
    real = _real_samples(loader) if dedup_padding else None
    flags = [(m, m.training) for m in module.modules()]
    module.eval()
    amp = (torch.autocast(device.type, dtype=autocast_dtype) if autocast_dtype is not None
           else contextlib.nullcontext())
    seen = 0
    try:
        with torch.no_grad(), fused_bn.fused_eval(fused), amp:
            for i, (x, y) in enumerate(loader):
                if max_batches is not None and i >= max_batches:
                    break
                x = x.to(device, non_blocking=True)
                y = y.to(device, non_blocking=True)
                if autocast_dtype is None and x.is_floating_point() and ref.is_floating_point():
                    x = x.to(ref.dtype)
                    if channels_last and x.dim() == 4:
                        x = x.contiguous(memory_format=torch.channels_last)
                B = x.shape[0]
                n_valid = B if real is None else min(B, max(0, real - seen))
                seen += B
                metrics.update(module(x), y, n_valid)
    finally:
        for m, f in flags:
            m.training = f
    metrics.reduce(process_group)
    return metrics.compute()
