"""DDP communication hooks that run on libgsync's kernels.

``powerSGD_hook`` / ``PowerSGDState`` are drop-ins for torch's
(T:distributed/algorithms/ddp_comm_hooks/powerSGD_hook.py): the same state fields,
defaults and validation, the same sequence and rounding points per bucket, registered the
same way::

    state = PowerSGDState(process_group=None, matrix_approximation_rank=2, start_powerSGD_iter=10)
    ddp.register_comm_hook(state, powerSGD_hook)

torch runs one ``bmm`` per tensor three times over, a Python loop over columns for every
orthogonalisation, a clone of the bucket and a device synchronize per bucket.  Here a
bucket is 6 grouped launches over all its compressed tensors (``gs_psgd_*``,
include/gsync.h) plus one pack and one unpack for the rest, in stream order on the stream
the hook is called on, with no host synchronisation and no device-to-host read.

``quantization_pertensor_hook`` / ``quantization_perchannel_hook`` are drop-ins for torch's
uint8 quantization hooks (T:distributed/algorithms/ddp_comm_hooks/quantization_hooks.py),
with torch's results bit for bit: three launches (``gs_quant_*``, ``gs_dequant_mean``) and
one all-gather per bucket.
"""
from __future__ import annotations

import logging

import numpy as np
import torch
import torch.distributed as dist

from . import _lib as L
from .multi_tensor import QuantPlan, TensorListPlan, is_dense

logger = logging.getLogger(__name__)

MAX_RANK = 8


def _should_compress(num_rows, num_cols, matrix_approximation_rank, min_compression_rate):
    """torch's rule: (worth compressing, uncompressed elements, compressed elements)."""
    uncompressed_size = num_rows * num_cols
    compressed_size = (num_rows + num_cols) * matrix_approximation_rank
    return compressed_size * min_compression_rate < uncompressed_size, uncompressed_size, compressed_size


def _as_matrix(t: torch.Tensor):
    """(n, m) of the row-major matrix a gradient is in memory order, or None when dim 0 is
    not its outermost dimension in memory (FusedMuon's rule: contiguous and channels_last
    filters both pass)."""
    if t.ndim < 2 or t.numel() == 0 or not is_dense(t) or t.stride(0) * t.shape[0] != t.numel():
        return None
    return t.shape[0], t.numel() // t.shape[0]


class PowerSGDState:
    """torch's ``PowerSGDState``: hyper-parameters and per-bucket memory of
    :func:`powerSGD_hook`.  Fields, defaults, validation, ``maybe_increase_iter``,
    ``compression_stats`` and pickling (everything but the process group and the launch
    plans) are torch's.  There is no ``batch_tensors_with_same_shape``: the grouped launch
    serves every shape at once.  ``p_memory_dict[bucket]`` / ``q_memory_dict[bucket]`` are
    laid out as torch lays them out with that option off: the compressed tensors in bucket
    order, ``n*r`` / ``m*r`` elements each, ``r = min(n, m, rank)``.  ``error_dict[bucket]``
    holds the error of the COMPRESSED tensors only, in bucket order (see
    :func:`powerSGD_hook`)."""

    __slots__ = [
        "process_group", "matrix_approximation_rank", "start_powerSGD_iter", "min_compression_rate",
        "orthogonalization_epsilon", "use_error_feedback", "warm_start", "rng", "error_dict", "p_memory_dict",
        "q_memory_dict", "iter", "total_numel_before_compression", "total_numel_after_compression",
        "compression_stats_logging_frequency", "next_stats_report", "_ctx", "_plain",
    ]
    _UNPICKLED = ("process_group", "_ctx", "_plain")

    def __init__(self, process_group, matrix_approximation_rank=1, start_powerSGD_iter=1_000, min_compression_rate=2,
                 use_error_feedback=True, warm_start=True, orthogonalization_epsilon=0, random_seed=0,
                 compression_stats_logging_frequency=10_000):
        if (use_error_feedback or warm_start) and start_powerSGD_iter <= 1:
            raise ValueError(
                "Expect `start_powerSGD_iter` > 1 if `use_error_feedback` or `warm_start` is enabled, "
                "because PowerSGD can only be applied after the first two iterations in DDP.")
        if not 1 <= int(matrix_approximation_rank) <= MAX_RANK:
            raise ValueError(f"powerSGD_hook supports matrix_approximation_rank 1..{MAX_RANK}, "
                             f"got {matrix_approximation_rank}")
        self.process_group = process_group
        self.matrix_approximation_rank = int(matrix_approximation_rank)
        self.start_powerSGD_iter = start_powerSGD_iter
        self.min_compression_rate = min_compression_rate
        self.use_error_feedback = use_error_feedback
        self.warm_start = warm_start
        self.orthogonalization_epsilon = orthogonalization_epsilon
        # seeds the host randn of Q, in the same order on every replica (torch's scheme)
        self.rng = np.random.RandomState(random_seed)
        self.error_dict: dict[int, torch.Tensor] = {}
        self.p_memory_dict: dict[int, torch.Tensor] = {}
        self.q_memory_dict: dict[int, torch.Tensor] = {}
        self.iter = 0
        self.total_numel_before_compression = 0
        self.total_numel_after_compression = 0
        self.compression_stats_logging_frequency = max(1, compression_stats_logging_frequency)
        self.next_stats_report = 0
        self._ctx: dict[int, _BucketPlans] = {}
        self._plain: dict = {}

    def __getstate__(self):
        logger.warning("NOTE: Process group is not serializable and excluded from a saved state.")
        return {slot: getattr(self, slot) for slot in self.__slots__ if slot not in self._UNPICKLED}

    def __setstate__(self, state):
        self.process_group = dist.distributed_c10d._get_default_group()
        logger.warning("NOTE: Process group will be set to a default group (i.e. the world size).")
        self._ctx, self._plain = {}, {}
        for slot, value in state.items():
            setattr(self, slot, value)

    def maybe_increase_iter(self, bucket):
        if bucket.is_last():
            self.iter += 1
        if self.iter == self.start_powerSGD_iter:
            logger.info("Start to apply PowerSGD after %s iterations.", self.iter)

    def compression_stats(self):
        """(compression rate, elements before compression, elements after)."""
        rate = (self.total_numel_before_compression / self.total_numel_after_compression
                if self.total_numel_after_compression > 0 else 0)
        return rate, self.total_numel_before_compression, self.total_numel_after_compression


class _BucketPlans:
    """What a bucket's layout fixes: which tensors are compressed, the two launch plans
    (compressed: slot 0 = the views inside the bucket, slot 1 = the views of one E buffer;
    the rest: slot 0 = the views, packed into ``flat``) and the stats increments."""

    def __init__(self, state: PowerSGDState, bucket, signature):
        grads = bucket.gradients()
        buf = bucket.buffer()
        self.signature = signature
        comp, rest, rows = [], [], []
        self.before = self.after = 0
        for g in grads:
            n = g.shape[0] if g.ndim else 1  # torch's tensor.view(shape[0], -1)
            m = g.numel() // max(1, n)
            r = min(n, m, state.matrix_approximation_rank)
            ok, before, after = _should_compress(n, m, r, state.min_compression_rate)
            self.before += before
            if ok and _as_matrix(g) is not None:  # else (never a dense filter) it travels uncompressed
                comp.append(g)
                rows.append(n)
                self.after += after
            else:
                rest.append(g)
                self.after += before
        dev = buf.device
        self.n_comp = len(comp)
        self.plan = TensorListPlan([g.numel() for g in comp], dev)
        self.layout = self.plan.psgd_layout(rows, state.matrix_approximation_rank)
        self.plan.set_ptrs(0, comp)
        self.error = torch.zeros(sum(g.numel() for g in comp), dtype=torch.float32, device=dev)
        off, views = 0, []
        for g in comp:
            views.append(self.error[off:off + g.numel()])
            off += g.numel()
        self.plan.set_ptrs(1, views)
        self.rest_plan = TensorListPlan([g.numel() for g in rest], dev)
        self.rest_plan.set_ptrs(0, rest)
        self.flat = torch.zeros(self.rest_plan.flat_numel, dtype=torch.float32, device=dev)
        self._keep = (comp, rest, views)


def _backend(group) -> str:
    return dist.get_backend(group)


def _all_reduce_sum(group, t: torch.Tensor):
    """SUM all-reduce of ``t`` in place, ordered on the current stream: libgsync's
    communicator of the group over RCCL (the one the DDP uses); a device tensor over gloo is
    staged through host memory as the DDP's own bucket all-reduces are; CPU tensors go to
    the process group."""
    if t.numel() == 0:
        return
    if t.is_cuda and _backend(group) in ("nccl", "rccl"):
        from .comm import get_communicator

        pg = None if group is None or group is dist.group.WORLD else group
        get_communicator(pg, t.device).all_reduce(t, stream=L.stream_ptr(t.device))
    elif t.is_cuda:
        host = t.to("cpu")
        dist.all_reduce(host, group=group)
        t.copy_(host)
    else:
        dist.all_reduce(t, group=group)


def _future(buf: torch.Tensor):
    fut = torch.futures.Future(devices=[buf.device]) if buf.is_cuda else torch.futures.Future()
    fut.set_result(buf)
    return fut


def _signature(bucket):
    buf = bucket.buffer()
    return (buf.data_ptr(), buf.numel(),
            tuple((g.data_ptr(), tuple(g.shape), tuple(g.stride())) for g in bucket.gradients()))


def powerSGD_hook(state: PowerSGDState, bucket) -> torch.futures.Future:
    """torch's ``powerSGD_hook`` on libgsync's grouped kernels.

    Per bucket, with ``M`` the row-major ``[n, m]`` matrix a gradient is in memory order
    (``n = shape[0]``, ``m = numel / n``):

    * before ``state.start_powerSGD_iter``: the plain averaged all-reduce, as in torch;
    * a tensor is compressed when torch's ``_should_compress(n, m, r, min_compression_rate)``
      says so and dim 0 is its outermost dimension in memory (FusedMuon's rule).  For a
      ``channels_last`` filter ``M`` is therefore a column permutation of the matrix torch
      would form from a contiguous one; a low-rank approximation commutes with a column
      permutation (``(MΠ)Q' = M(ΠQ')``, and Gram-Schmidt acts on P's and Q's columns, which
      the permutation of Q's rows does not mix), so the result is the same approximation,
      permuted — where torch's hook raises on the ``view``;
    * the other tensors are packed into one flat buffer (divided by the world size on the
      way), all-reduced together and unpacked, by the pack / unpack kernels;
    * the compressed ones follow torch's sequence and rounding points: ``M' = M + E``; Q is
      the warm-start Q or torch's seeded host ``randn`` (``state.rng``, CPU generator, copied
      over), orthogonalised by modified Gram-Schmidt; ``P = M'Q``; all-reduce P;
      orthogonalise P; ``Q = M'ᵀP``; all-reduce Q; ``Q /= ws``; the bucket receives
      ``PQᵀ`` and ``E = M' - PQᵀ``.

    Departures from torch, both deliberate: (1) E is kept for the compressed tensors only.
    torch also stores "local minus mean" of the uncompressed ones and adds it to their next
    gradient; that quantity is not a compression error, and it is zero at world size 1.
    (2) Every rank orthogonalises by Gram-Schmidt; torch switches to a QR factorisation for
    fp32 at rank > 2 (the same subspace, another basis of it).

    Limits (each raises): ranks 1..8; fp32 bucket buffers; a bucket layout that changes
    after its state was created (only DDP's rebuild after iteration 0 does that, which
    ``start_powerSGD_iter >= 2`` already excludes)."""
    buf = bucket.buffer()
    if buf.dtype != torch.float32:
        raise ValueError(f"powerSGD_hook supports fp32 bucket buffers only, got {buf.dtype}")
    if not 1 <= state.matrix_approximation_rank <= MAX_RANK:
        raise ValueError(f"powerSGD_hook supports matrix_approximation_rank 1..{MAX_RANK}, "
                         f"got {state.matrix_approximation_rank}")
    group = state.process_group if state.process_group is not None else dist.group.WORLD
    ws = dist.get_world_size(group)
    index = bucket.index()

    if state.iter < state.start_powerSGD_iter:
        key = (index, buf.data_ptr(), buf.numel())
        plan = state._plain.get(key)
        if plan is None:
            plan = state._plain[key] = TensorListPlan([buf.numel()], buf.device)
            plan.set_ptrs(0, [buf])
        plan.scale(0, torch.float32, float(ws), L.GS_SCALE_DIV)
        _all_reduce_sum(group, buf)
        state.maybe_increase_iter(bucket)
        return _future(buf)

    sig = _signature(bucket)
    ctx = state._ctx.get(index)
    if ctx is None:
        state._plain.clear()
        ctx = state._ctx[index] = _BucketPlans(state, bucket, sig)
        if state.use_error_feedback:
            state.error_dict[index] = ctx.error
    elif ctx.signature != sig:
        raise RuntimeError(f"powerSGD_hook: the layout of bucket {index} changed after its PowerSGD state was created "
                           "(buckets are rebuilt after iteration 0: keep start_powerSGD_iter >= 2)")
    state.total_numel_before_compression += ctx.before
    state.total_numel_after_compression += ctx.after
    if bucket.is_last() and state.iter >= state.next_stats_report:
        logger.info("Compression stats: iter %s, total before compression %s, total after compression %s, rate %s",
                    state.iter, state.total_numel_before_compression, state.total_numel_after_compression,
                    state.compression_stats()[0])
        state.next_stats_report = state.iter + state.compression_stats_logging_frequency

    # the uncompressed tensors: one pack (/ ws), one collective, one unpack
    if ctx.rest_plan.n:
        ctx.rest_plan.pack(0, torch.float32, ctx.flat, float(ws), L.GS_SCALE_DIV)
        _all_reduce_sum(group, ctx.flat)
        ctx.rest_plan.unpack(ctx.flat, 0, torch.float32)

    if ctx.n_comp:
        plan, lay = ctx.plan, ctx.layout
        fresh = not state.warm_start or index not in state.p_memory_dict
        if fresh:
            state.p_memory_dict[index] = torch.empty(lay["p_total"], dtype=torch.float32, device=buf.device)
            state.q_memory_dict[index] = torch.empty(lay["q_total"], dtype=torch.float32, device=buf.device)
            host = torch.empty(lay["q_total"], dtype=torch.float32, pin_memory=buf.is_cuda)
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(state.rng.randint(1_000_000_000))
                for t in lay["tensors"]:
                    host[t["q"]:t["q"] + t["m"] * t["r"]].view(1, t["m"], t["r"]).copy_(
                        torch.randn(1, t["m"], t["r"], device="cpu", dtype=torch.float32))
            state.q_memory_dict[index].copy_(host, non_blocking=True)
        p, q = state.p_memory_dict[index], state.q_memory_dict[index]
        eps = state.orthogonalization_epsilon
        plan.psgd_orthogonalize(1, q, eps)
        plan.psgd_project(state.use_error_feedback, p, q)
        _all_reduce_sum(group, p)  # orthogonalised next: no division by the world size
        plan.psgd_orthogonalize(0, p, eps)
        plan.psgd_backproject(p, q)
        _all_reduce_sum(group, q)
        plan.psgd_reconstruct(p, q, 1.0 / ws)
        if not state.warm_start:
            state.p_memory_dict.clear()
            state.q_memory_dict.clear()

    state.maybe_increase_iter(bucket)
    return _future(buf)


# ---------------------------------------------------------------------- uint8 quantization
# (group, bucket index, buffer address, numel, bucket_size) -> (launches, payload, receive
# buffer): a changed layout simply makes a new entry
_QUANT_CACHE: dict = {}


def _all_gather_bytes(group, send: torch.Tensor, recv: torch.Tensor, ws: int):
    """``recv`` = every rank's ``send`` back to back, ordered on the current stream; the
    transports are :func:`_all_reduce_sum`'s."""
    if send.is_cuda and _backend(group) in ("nccl", "rccl"):
        from .comm import get_communicator

        pg = None if group is None or group is dist.group.WORLD else group
        get_communicator(pg, send.device).all_gather(send, recv, stream=L.stream_ptr(send.device))
    elif send.is_cuda:
        host = torch.empty(recv.numel(), dtype=torch.uint8)
        dist.all_gather(list(host.view(ws, -1).unbind(0)), send.to("cpu"), group=group)
        recv.copy_(host)
    else:
        dist.all_gather(list(recv.view(ws, -1).unbind(0)), send, group=group)


def _quantization_hook(name, process_group, bucket, bucket_size):
    buf = bucket.buffer()
    if buf.dtype != torch.float32:
        raise ValueError(f"{name} supports fp32 bucket buffers only, got {buf.dtype}")
    if bucket_size and not (16 <= bucket_size <= 4096 and bucket_size % 16 == 0):
        raise ValueError(f"{name} supports a bucket_size that is a multiple of 16 in 16..4096, got {bucket_size}")
    group = process_group if process_group is not None else dist.group.WORLD
    ws = dist.get_world_size(group)
    key = (id(group), ws, bucket.index(), buf.data_ptr(), buf.numel(), bucket_size)
    ctx = _QUANT_CACHE.get(key)
    if ctx is None:
        nbytes = QuantPlan.payload_bytes(buf.numel(), bucket_size)
        ctx = _QUANT_CACHE[key] = (QuantPlan(buf.device), torch.zeros(nbytes, dtype=torch.uint8, device=buf.device),
                                   torch.zeros(ws * nbytes, dtype=torch.uint8, device=buf.device))
    plan, payload, gathered = ctx
    if buf.numel():
        if bucket_size:
            plan.quant_perchannel(buf, payload, bucket_size)
        else:
            plan.quant_pertensor(buf, payload)
        _all_gather_bytes(group, payload, gathered, ws)
        plan.dequant_mean(gathered, ws, buf, bucket_size)
    return _future(buf)


def quantization_pertensor_hook(process_group, bucket) -> torch.futures.Future:
    """torch's ``quantization_pertensor_hook``
    (T:distributed/algorithms/ddp_comm_hooks/quantization_hooks.py) on libgsync's kernels,
    registered the same way (``ddp.register_comm_hook(process_group, quantization_pertensor_hook)``):
    the bucket travels as uint8 with one MinMaxObserver ``(scale, zero point)`` per rank, and
    comes back as the mean of all ranks' dequantized buckets, written in place.

    The arithmetic is torch's, bit for bit in fp32 (``gs_quant_pertensor``, ``gs_dequant_mean``
    in include/gsync.h).  Per bucket: a min/max pass, a quantize pass, ONE all-gather of a
    payload that carries the bytes and the qparams (torch: two all-gathers, an observer module
    and ``ws`` dequantize-and-add temporaries), one dequantize-and-average launch; in stream
    order on the calling stream, with no host synchronisation over RCCL.  Over gloo a device
    payload is staged through host memory; CPU buckets run on the host backend.  A value that
    is not finite anywhere makes the whole bucket NaN on every rank.  fp32 buckets only."""
    return _quantization_hook("quantization_pertensor_hook", process_group, bucket, 0)


def quantization_perchannel_hook(process_group, bucket, bucket_size=512) -> torch.futures.Future:
    """torch's ``quantization_perchannel_hook`` on libgsync's kernels: as
    :func:`quantization_pertensor_hook`, with one ``(scale, zero point)`` per channel of
    ``bucket_size`` consecutive elements of the flat bucket (``functools.partial(
    quantization_perchannel_hook, bucket_size=128)`` as with torch's).  One quantize launch
    (``gs_quant_perchannel``: a channel is read once and stays in registers between its
    min/max and its quantization), one all-gather, one dequantize-and-average launch, where
    torch loops over the channels in Python twice.  A channel that holds a value that is not
    finite comes out NaN on every rank; the others are unaffected.  ``bucket_size``: a
    multiple of 16 in 16..4096 (``ValueError`` otherwise); torch's extra all-zero channel
    when the bucket is a multiple of ``bucket_size`` is not sent."""
    if not bucket_size:
        raise ValueError(f"quantization_perchannel_hook supports a bucket_size that is a multiple of 16 in 16..4096, "
                         f"got {bucket_size}")
    return _quantization_hook("quantization_perchannel_hook", process_group, bucket, int(bucket_size))
