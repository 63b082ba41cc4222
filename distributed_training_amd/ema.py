"""Fused EMA / SWA weight averaging: drop-ins for ``torch.optim.swa_utils``.

``torch.optim.swa_utils.AveragedModel.update_parameters`` reads ``n_averaged`` on the
host twice per call (two synchronisations, so it cannot be captured), averages with
``torch._foreach_lerp_`` and copies every buffer with its own ``copy_``.  Here one
update is three launches on the current stream and no host synchronisation:

  gs_ema_hyper            the weight and the first-update flag from the device counter
  gs_ema_step             a = lerp(a, s, w) over every averaged tensor (one per source dtype)
  gs_ema_step(copy=1)     the buffers torch keeps "in sync", moved as 32-bit words

The arithmetic is torch.lerp's CPU kernel bit for bit (include/gsync.h, gs_ema_step), on
the host and on the GPU.  A bf16 / fp16 model is averaged in an fp32 shadow and the
module's parameters are the low-precision copy written by the same pass; under ZeRO the
average lives on this rank's fp32 master shards (:class:`ShardedAveragedModel`).
"""
from __future__ import annotations

import contextlib
import itertools

import torch
from torch.optim import swa_utils as _swa

from . import _lib as L
from .multi_tensor import TensorListPlan, ema_hyper, is_dense, update_task_units

_FLOAT = (torch.float32, torch.bfloat16, torch.float16)
_LOWP = (torch.bfloat16, torch.float16)


# ------------------------------------------------------------------ avg functions
class _TaggedAvgFn:
    """A ``multi_avg_fn`` that :class:`AveragedModel` recognises by ``mode`` / ``decay``
    and runs fused; called directly it updates the tensor lists in place."""

    def __init__(self, mode: int, decay: float):
        self.mode = mode
        self.decay = float(decay)

    def weight(self, num_averaged) -> float:
        n = int(num_averaged)
        if self.mode == L.GS_EMA_SWA:
            return float(1 / (torch.tensor(n, dtype=torch.int64) + 1))  # torch's fp32 1 / (n + 1)
        if self.mode == L.GS_EMA_WARMUP:
            return 1 - min(self.decay, (1 + n) / (10 + n))
        return 1 - self.decay

    @torch.no_grad()
    def __call__(self, averaged_param_list, current_param_list, num_averaged) -> None:
        avg, cur = list(averaged_param_list), list(current_param_list)
        if not avg:
            return
        w = self.weight(num_averaged)
        fusable = L.available() and all(
            a.dtype == torch.float32 and c.dtype in _FLOAT and c.dtype == cur[0].dtype and a.device == c.device
            and a.device == avg[0].device and a.device.type in ("cpu", "cuda") and a.shape == c.shape
            and is_dense(a) and a.stride() == c.stride() for a, c in zip(avg, cur))
        if fusable:
            plan = TensorListPlan([a.numel() for a in avg], avg[0].device)
            plan.set_ptrs(0, avg)
            plan.set_ptrs(1, cur)
            plan.ema(cur[0].dtype, w)
            plan.close()
        elif torch.is_floating_point(avg[0]):
            torch._foreach_lerp_(avg, cur, w)
        else:
            for a, c in zip(avg, cur):
                a.copy_(a * (1 - w) + c * w)


def get_ema_multi_avg_fn(decay=0.999, warmup=False):
    """``torch.optim.swa_utils.get_ema_multi_avg_fn``: a ← lerp(a, p, 1 - decay).  With
    ``warmup`` the decay of update n is min(decay, (1 + n) / (10 + n))."""
    if decay < 0.0 or decay > 1.0:
        raise ValueError(f"Invalid decay value {decay} provided. Please provide a value in [0,1] range.")
    return _TaggedAvgFn(L.GS_EMA_WARMUP if warmup else L.GS_EMA_EMA, decay)


def get_swa_multi_avg_fn():
    """``torch.optim.swa_utils.get_swa_multi_avg_fn``: a ← lerp(a, p, 1 / (n + 1))."""
    return _TaggedAvgFn(L.GS_EMA_SWA, 0.0)


# ------------------------------------------------------------------ the fused update
def _words(t: torch.Tensor):
    """(pointer, 32-bit word count) of a dense tensor that can ride as fp32 words."""
    nbytes = t.numel() * t.element_size()
    if nbytes % 4 or t.data_ptr() % 4 or not is_dense(t):
        return None
    return t.data_ptr(), nbytes // 4


class _FusedAverager:
    """The launches of one update over fixed tensor lists.

    ``avg``: (average fp32, source, low-precision copy or None) triples, one plan per
    (source dtype, copy dtype); ``sync``: (destination, source) pairs of one dtype moved
    bit for bit; ``ints``: integer (destination, source) pairs that are averaged, with
    torch's own arithmetic (its non-lerp branch), by small torch launches."""

    def __init__(self, mode: int, decay: float, n_averaged: torch.Tensor):
        self.mode, self.decay, self.n = mode, float(decay), n_averaged
        self.device = n_averaged.device
        self.hyper = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.plans: list = []
        self.sync_plan = None
        self.sync_rest: list = []
        self.ints: list = []

    def bind(self, avg, sync, ints=()):
        if L._capturing():
            raise RuntimeError("weight averaging: take one update outside the graph before capturing it")
        for pl in self.all_plans():
            pl.close()
        self.plans, self.sync_plan, self.sync_rest, self.ints = [], None, [], list(ints)
        groups: dict = {}
        for a, s, lo in avg:
            groups.setdefault((s.dtype, None if lo is None else lo.dtype), []).append((a, s, lo))
        tu = update_task_units(self.device)
        for (sd, ld), items in groups.items():
            plan = TensorListPlan([a.numel() for a, _, _ in items], self.device, task_units=tu)
            plan.set_ptrs(0, [a for a, _, _ in items])
            plan.set_ptrs(1, [s for _, s, _ in items])
            if ld is not None:
                plan.set_ptrs(2, [lo for _, _, lo in items])
            plan.set_hyper_source(self.hyper)
            self.plans.append((plan, sd, ld))
        riders = []
        for d, s in sync:
            wd, ws = _words(d), _words(s)
            if wd is None or ws is None or d.dtype != s.dtype or d.shape != s.shape or d.stride() != s.stride():
                self.sync_rest.append((d, s))
            else:
                riders.append((wd[0], ws[0], wd[1]))
        if riders:
            self.sync_plan = TensorListPlan([n for _, _, n in riders], self.device, task_units=tu)
            self.sync_plan.set_ptrs(0, [d for d, _, _ in riders])
            self.sync_plan.set_ptrs(1, [s for _, s, _ in riders])

    def all_plans(self):
        return [p for p, _, _ in self.plans] + ([self.sync_plan] if self.sync_plan is not None else [])

    @torch.no_grad()
    def step(self):
        if self.ints:
            # before the counter advances: torch's arithmetic for non-floating tensors
            first = self.n == 0
            for a, s in self.ints:
                if self.mode == L.GS_EMA_SWA:
                    new = a + (s - a) / (self.n + 1)
                elif self.mode == L.GS_EMA_WARMUP:
                    n = self.n.double()
                    d = torch.clamp((1 + n) / (10 + n), max=self.decay)
                    new = a * d + s * (1 - d)
                else:
                    new = a * self.decay + s * (1 - self.decay)
                a.copy_(torch.where(first, s, new.to(a.dtype)))
        ema_hyper(self.n, self.mode, self.decay, self.hyper)
        for plan, sd, ld in self.plans:
            plan.ema(sd, lowp_dtype=ld)
        if self.sync_plan is not None:
            self.sync_plan.ema(torch.float32, copy=True)
        for d, s in self.sync_rest:
            d.copy_(s)

    def close(self):
        for pl in self.all_plans():
            pl.close()
        self.plans, self.sync_plan = [], None


def _signature(tensors):
    tensors = list(tensors)
    return [t.data_ptr() for t in tensors], [t.numel() for t in tensors]


class _Members:
    """A module's parameters and buffers in ``parameters()`` / ``buffers()`` order, re-read on
    every call from the owning modules' own dicts: a replaced tensor is seen, at a tenth of
    the cost of walking the module tree (0.2 ms per walk on a ResNet-50).  Submodules added
    or removed after the first update need :meth:`AveragedModel.rebind`."""

    def __init__(self, module):
        self.module = module
        self.p, self.b = self._slots(module, "_parameters"), self._slots(module, "_buffers")

    @staticmethod
    def _slots(module, attr):
        seen, out = set(), []
        for mod in module.modules():
            for k, v in getattr(mod, attr).items():
                if v is not None and id(v) not in seen:
                    seen.add(id(v))
                    out.append((getattr(mod, attr), k))
        return out

    def params(self):
        return [d[k] for d, k in self.p]

    def buffers(self):
        return [d[k] for d, k in self.b]


# ------------------------------------------------------------------ AveragedModel
class AveragedModel(_swa.AveragedModel):
    """Drop-in for ``torch.optim.swa_utils.AveragedModel`` (same attributes, ``forward``
    and — for an fp32 model — ``state_dict`` keys; works with ``update_bn`` / ``SWALR``)
    whose ``update_parameters`` is three launches and no host synchronisation, so it can
    sit inside ``CapturedStep`` (take the first update outside the capture).

    ``multi_avg_fn``: this module's :func:`get_ema_multi_avg_fn` / :func:`get_swa_multi_avg_fn`
    run fused.  With neither function given the average is SWA through lerp — what torch
    does on a GPU; torch's CPU default takes its non-lerp ``avg_fn`` and differs from this
    in the last bits.  Any other ``avg_fn`` / ``multi_avg_fn`` (torch's own included), a
    missing library, or a model the kernels do not cover (parameters that are not dense
    fp32 / bf16 / fp16 on one cpu or cuda device shared with this copy) runs torch's
    ``update_parameters`` unchanged; ``last_path`` says which ran: "fused" or "stock".

    ``master_dtype=torch.float32``: a bf16 / fp16 model is averaged in an fp32 shadow (in
    its own dtype an increment of (1 - decay)·(p - a) below half an ulp never moves the
    average) and ``module`` holds the rounded copy, written by the same pass.  The shadow
    travels in ``state_dict`` as the module's extra state.  ``master_dtype=None`` keeps
    torch's behaviour: the average in the model's dtype, on the stock path.

    ``n_averaged`` lives on the module's device (torch leaves it on the CPU when
    ``device`` is None).  With ``use_buffers=True`` integer buffers are averaged by
    torch's arithmetic for them, a few small launches each, also without a host read.
    """

    def __init__(self, model, device=None, avg_fn=None, multi_avg_fn=None, use_buffers=False, *,
                 master_dtype=torch.float32):
        super().__init__(model, device, avg_fn, multi_avg_fn, use_buffers)
        if master_dtype not in (torch.float32, None):
            raise ValueError("master_dtype: torch.float32 or None")
        self.master_dtype = master_dtype
        self.last_path: str | None = None
        self._averager: _FusedAverager | None = None
        self._sig = None
        self._members = None
        self._shadow: dict = {}  # id(module tensor) -> fp32 shadow
        if avg_fn is None and multi_avg_fn is None:
            self._mode, self._decay = L.GS_EMA_SWA, 0.0
        elif isinstance(multi_avg_fn, _TaggedAvgFn):
            self._mode, self._decay = multi_avg_fn.mode, multi_avg_fn.decay
        else:
            self._mode = None
        first = next(iter(self.module.parameters()), None)
        if self._mode is not None and first is not None and self.n_averaged.device != first.device:
            self.n_averaged = self.n_averaged.to(first.device)
        if self._mode is not None and master_dtype is not None:
            for t in self._averaged_tensors(self.module):
                if t.dtype in _LOWP:
                    self._shadow[id(t)] = t.detach().float()
            if self._shadow:
                self.__class__ = _ShadowedAveragedModel

    # ---- which tensors
    def _averaged_tensors(self, m):
        return list(itertools.chain(m.parameters(), m.buffers())) if self.use_buffers else list(m.parameters())

    def _fusable(self, mine, theirs, my_bufs, their_bufs) -> bool:
        if self._mode is None or not L.available() or len(mine) != len(theirs) or len(my_bufs) != len(their_bufs):
            return False
        dev = self.n_averaged.device
        if dev.type not in ("cpu", "cuda"):
            return False
        for a, s in itertools.chain(zip(mine, theirs), zip(my_bufs, their_bufs)):
            if a.device != dev or s.device != dev or a.shape != s.shape or a.dtype != s.dtype or \
                    a.stride() != s.stride() or not is_dense(a) or a.data_ptr() == s.data_ptr() and a.numel():
                return False
        for a in mine:
            if torch.is_floating_point(a):
                if a.dtype not in _FLOAT or (a.dtype in _LOWP and id(a) not in self._shadow):
                    return False
            elif torch.is_complex(a) or a.dtype == torch.bool:
                return False
        return True

    def _bind(self, mine, theirs, my_bufs, their_bufs):
        avg, ints = [], []
        for t, s in zip(mine, theirs):
            a, s = t.detach(), s.detach()
            if not torch.is_floating_point(a):
                ints.append((a, s))
            elif a.dtype == torch.float32:
                avg.append((a, s, None))
            else:
                avg.append((self._shadow[id(t)], s, a))
        sync = [] if self.use_buffers else [(a.detach(), s.detach()) for a, s in zip(my_bufs, their_bufs)]
        if self._averager is None:
            self._averager = _FusedAverager(self._mode, self._decay, self.n_averaged)
        self._averager.n = self.n_averaged
        self._averager.bind(avg, sync, ints)

    # ---- copy.deepcopy / pickle: plans are rebuilt by the copy's first update, the shadows
    # (keyed by the module's tensor objects) travel in module order
    def __getstate__(self):
        state = dict(self.__dict__)
        state["_averager"], state["_members"], state["_sig"] = None, None, None
        state["_shadow"] = [self._shadow.get(id(t)) for t in self._averaged_tensors(self.module)]
        return state

    def __setstate__(self, state):
        shadows = state.pop("_shadow")
        super().__setstate__(state)
        self._shadow = {id(t): s for t, s in zip(self._averaged_tensors(self.module), shadows) if s is not None}

    def rebind(self):
        """Forget the cached tensor lists and plans (after submodules were added or removed)."""
        self._members = None
        self._sig = None

    def _lists(self, model):
        mem = self._members
        if mem is None or mem[1].module is not model or mem[0].module is not self.module:
            mem = self._members = (_Members(self.module), _Members(model))
        try:
            out = [mem[0].params(), mem[1].params(), mem[0].buffers(), mem[1].buffers()]
            if any(t is None for t in itertools.chain(*out)):
                raise KeyError
        except KeyError:  # a registered tensor went away: walk again
            mem = self._members = (_Members(self.module), _Members(model))
            out = [mem[0].params(), mem[1].params(), mem[0].buffers(), mem[1].buffers()]
        if self.use_buffers:
            out[0], out[1] = out[0] + out[2], out[1] + out[3]
        return out

    def update_parameters(self, model) -> None:
        if self._mode is None:
            self.last_path = "stock"
            super().update_parameters(model)
            return
        mine, theirs, my_bufs, their_bufs = self._lists(model)
        sig = _signature(itertools.chain(mine, theirs, my_bufs, their_bufs, (self.n_averaged,)))
        if sig != self._sig:
            # shadows of tensors the module no longer holds (a .to() replaced them) are dropped
            ids = {id(t) for t in mine}
            self._shadow = {k: v for k, v in self._shadow.items() if k in ids}
            if self._fusable(mine, theirs, my_bufs, their_bufs):
                self._bind(mine, theirs, my_bufs, their_bufs)
            elif self._averager is not None:
                self._averager.close()
                self._averager = None
            self._sig = sig
        if self._averager is None:
            self.last_path = "stock"
            super().update_parameters(model)
            return
        self._averager.step()
        self.last_path = "fused"


class _ShadowedAveragedModel(AveragedModel):
    """An :class:`AveragedModel` of a low-precision model: the fp32 shadow of the average
    is part of its ``state_dict`` (an fp32 model keeps exactly torch's keys)."""

    def get_extra_state(self):
        return {"shadow": [self._shadow[id(t)].detach().cpu().clone()
                           for t in self._averaged_tensors(self.module) if id(t) in self._shadow]}

    def set_extra_state(self, state):
        mine = [t for t in self._averaged_tensors(self.module) if id(t) in self._shadow]
        if len(mine) != len(state["shadow"]):
            raise RuntimeError(f"averaged model: {len(mine)} fp32 shadows, the checkpoint holds {len(state['shadow'])}")
        with torch.no_grad():
            for t, v in zip(mine, state["shadow"]):
                self._shadow[id(t)].copy_(v)


# ------------------------------------------------------------------ ZeRO
class ShardedAveragedModel:
    """The weight average of a :class:`~distributed_training_amd.zero.ZeroDataParallel`
    engine, kept on this rank's fp32 master shards: 4 B/param/world, one plan over the
    engine's shards (slot 0 the average, slot 1 ``engine.master``) and no collective per
    update — the operation is elementwise, so sharding cannot change a bit.  Buffers are
    copied (or, with ``use_buffers``, averaged) as :class:`AveragedModel` does.

    ``state_dict`` / ``load_state_dict`` are this rank's shard, with the layout rules of
    ``ZeroDataParallel.state_dict``; :meth:`consolidated_state_dict` is collective and
    returns the full averaged model; ``with avg.swapped():`` evaluates it in place."""

    def __init__(self, engine, multi_avg_fn=None, use_buffers=False):
        if multi_avg_fn is None:
            multi_avg_fn = get_swa_multi_avg_fn()
        if not isinstance(multi_avg_fn, _TaggedAvgFn):
            raise TypeError("ShardedAveragedModel: multi_avg_fn from this module's get_ema_multi_avg_fn / "
                            "get_swa_multi_avg_fn (closures are not fused)")
        self.engine = engine
        self.use_buffers = bool(use_buffers)
        self.device = engine.device
        self.n_averaged = torch.zeros((), dtype=torch.int64, device=self.device)
        self.ema = [m.detach().float().clone() for m in engine.master]
        self.buffers = {k: b.detach().clone() for k, b in engine.module.named_buffers()}
        self._averager = _FusedAverager(multi_avg_fn.mode, multi_avg_fn.decay, self.n_averaged)
        self._sig = None

    def _bind(self):
        live = dict(self.engine.module.named_buffers())
        avg = [(e, m.detach(), None) for e, m in zip(self.ema, self.engine.master)]
        sync, ints = [], []
        for k, b in self.buffers.items():
            if not self.use_buffers:
                sync.append((b, live[k].detach()))
            elif torch.is_floating_point(b) and b.dtype == torch.float32:
                avg.append((b, live[k].detach(), None))
            elif torch.is_floating_point(b):
                raise TypeError(f"ShardedAveragedModel(use_buffers=True): buffer {k} is {b.dtype}; only fp32 and "
                                "integer buffers are averaged")
            else:
                ints.append((b, live[k].detach()))
        self._averager.bind(avg, sync, ints)

    def update_parameters(self, model=None) -> None:
        """One update from the engine's master shards (``model`` is accepted for the
        drop-in's signature and ignored)."""
        live = [b for _, b in self.engine.module.named_buffers()]
        sig = _signature(itertools.chain(self.engine.master, live))
        if sig != self._sig:
            self._bind()
            self._sig = sig
        self._averager.step()

    # ---- checkpoints
    def state_dict(self) -> dict:
        e = self.engine
        return {"n_averaged": int(self.n_averaged), "rank": e.rank, "world": e.world,
                "bucket_numel": list(e.bucket_numel), "ema": [t.detach().cpu().clone() for t in self.ema],
                "buffers": {k: b.detach().cpu().clone() for k, b in self.buffers.items()}}

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        e = self.engine
        if sd["world"] != e.world or sd["rank"] != e.rank or list(sd["bucket_numel"]) != list(e.bucket_numel):
            raise RuntimeError(f"averaged shard is for rank {sd['rank']}/{sd['world']} with buckets "
                               f"{sd['bucket_numel']}; this engine is rank {e.rank}/{e.world} with "
                               f"{list(e.bucket_numel)}")
        self.n_averaged.fill_(int(sd["n_averaged"]))
        for t, v in zip(self.ema, sd["ema"]):
            t.copy_(v.to(t.device))
        for k, b in self.buffers.items():
            b.copy_(sd["buffers"][k].to(b.device))

    def consolidated_state_dict(self) -> dict:
        """The full averaged model (torchvision keys, fp32 values), gathered as the
        engine's ``consolidated_state_dict``.  Collective."""
        return self.engine._consolidate(self.ema, buffers=self.buffers)

    @contextlib.contextmanager
    def swapped(self):
        """The average inside the engine's model for evaluation: every parameter is
        cast(average) and the buffers are the averaged model's; the live weights (from
        the master) and buffers come back on exit.  Collective (two all-gathers)."""
        e = self.engine
        e.wait_allgather()
        live = dict(e.module.named_buffers())
        with torch.no_grad():
            saved_bufs = {k: b.detach().clone() for k, b in live.items()}
            saved = None if e.lowp else [m.detach().clone() for m in e.master]
            for shard, a in zip(e.param_shards, self.ema):
                shard.copy_(a.to(shard.dtype))
            for b, flat in enumerate(e.param_flats):
                e._all_gather_flat(b, flat)
            for k, b in live.items():
                b.copy_(self.buffers[k])
        try:
            yield e.module
        finally:
            with torch.no_grad():
                if e.lowp:
                    for shard, m in zip(e.param_shards, e.master):
                        shard.copy_(m.to(shard.dtype))
                else:
                    for m, v in zip(e.master, saved):
                        m.copy_(v)
                for b, flat in enumerate(e.param_flats):
                    e._all_gather_flat(b, flat)
                for k, b in live.items():
                    b.copy_(saved_bufs[k])

    def close(self):
        self._averager.close()
