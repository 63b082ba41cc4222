"""Fused multi-tensor optimizers on libgsync kernels (drop-ins for torch.optim).

* :class:`FusedSGD`  — ``torch.optim.SGD`` semantics (T:optim/sgd.py:322-381
  ``_single_tensor_sgd``; :383-470 ``_multi_tensor_sgd``): one HIP pass over
  (param, grad, momentum_buffer) = 20 B/param fp32 instead of >=3 foreach passes.
* :class:`FusedAdam` — ``torch.optim.Adam`` / ``AdamW`` semantics
  (T:optim/adam.py:554-800 ``_multi_tensor_adam``, the reference's default on
  GPU, ``R:resnet/pytorch_ddp/ddp_train.py:97``): one pass over
  (p, g, m, v) = 28 B/param instead of the ~72 B/param of 7 foreach passes.
* :class:`FusedLARS` — layer-wise adaptive SGD for large global batches (no
  torch counterpart; the arithmetic is ``include/gsync.h``'s contract): the
  per-tensor ‖w‖², ‖g‖² of the whole list in one deterministic pass
  (8 B/param), then one update pass (20 B/param) that forms each tensor's trust
  ratio itself.
* :class:`FusedLAMB` — layer-wise adaptive Adam (DeepSpeed's FusedLamb,
  ColossalAI's Lamb / FusedLAMB; no torch counterpart): one pass that advances
  the moments and publishes the per-tensor ‖w‖², ‖update‖² (24 B/param), then
  one update pass (16 B/param) that recomputes the update and applies each
  tensor's trust ratio.
* :class:`FusedMuon` — ``torch.optim.Muon`` semantics (T:optim/_muon.py): momentum,
  then ``ns_steps`` Newton-Schulz iterations on bf16 MFMA, every stage one grouped
  launch over the whole list of matrices (``3 * ns_steps + 3`` operations per step
  instead of ~20 launches per parameter).
* :class:`FusedAdafactor` — ``torch.optim.Adafactor`` semantics (T:optim/_adafactor.py):
  factored second moments, at most 7 grouped launches per step and no host read instead
  of ~15 launches and two ``.item()`` synchronisations per parameter.
* :func:`clip_grad_norm_` — ``torch.nn.utils.clip_grad_norm_``
  (T:nn/utils/clip_grad.py:50-186) with a wave-level Σg² reduction and the
  clip coefficient kept on the device (no host sync).

``state_dict`` layouts are torch's (``momentum_buffer``; ``step`` /
``exp_avg`` / ``exp_avg_sq``), so checkpoints move between the two.

Extras used by the engine: ``grad_scale`` (a 1-element device tensor the
update multiplies grads by — clip coefficient or AMP 1/scale), ``found_inf``
(skip the step when non-zero) and ``max_grad_norm`` (DeepSpeed-style
``gradient_clipping``: Σg² + coefficient computed on device, folded into the
update kernel).

``capturable=True`` (torch's Adam flag, also offered on SGD) makes ``step()``
safe to record into a hipGraph (see :mod:`.graphs`): the step-varying
hyper-parameters live in a small device buffer the update kernel reads when it
runs (``gs_plan_set_hyper_source``) — SGD's lr; Adam's step_size, sqrt(bc2)
and 1-lr·wd, produced on the device from a device step counter that does not
advance on an AMP overflow (``gs_adam_hyper``, T:optim/adam.py capturable
branch).  :meth:`refresh_hyper` copies a changed ``group["lr"]`` into that
buffer outside the graph, so LR schedulers keep working across replays.
"""
from __future__ import annotations

import math
import os
from typing import Iterable

import torch
from torch.autograd.graph import increment_version

from . import _lib as L
from .multi_tensor import TensorListPlan, clip_coef, is_dense, update_task_units


# the gradient-norm clip folded into the update kernels (gs_plan_set_clip);
# GSYNC_CLIP_FUSED=0 keeps the separate Σg² / coefficient launches (A/B runs)
CLIP_FUSED = os.environ.get("GSYNC_CLIP_FUSED", "1") not in ("", "0")


def _capturing() -> bool:
    """Is torch's current stream recording a graph (False without a GPU)?"""
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


class _PlanCache:
    """One TensorListPlan per (param list, grad dtype) signature."""

    def __init__(self):
        self._plans: dict = {}
        self.timer_slots = 0

    def get(self, params):
        key = tuple(id(p) for p in params) + (params[0].device,)
        plan = self._plans.get(key)
        if plan is None:
            plan = TensorListPlan([p.numel() for p in params], params[0].device,
                                  task_units=update_task_units(params[0].device))
            if self.timer_slots and plan.kind == L.GS_DEV_HIP:
                plan.timer_enable(self.timer_slots)
            self._plans[key] = plan
        return plan

    def plans(self):
        return list(self._plans.values())


def _check_dense(p: torch.Tensor, g: torch.Tensor, what: str, seen: dict | None = None):
    """p dense and g in p's layout.  ``seen`` (id(p) -> strides found dense)
    skips the walk over the dims for a parameter already checked — a grad with
    the same strides (and shape) is then dense too."""
    ps = p.stride()
    if g.stride() != ps:
        raise RuntimeError(f"{what}: grad layout must match its parameter's (param {ps}, grad {g.stride()})")
    if seen is not None and seen.get(id(p)) == ps:
        return
    if not is_dense(p):
        raise RuntimeError(f"{what}: parameters must be dense (got strides {ps})")
    if seen is not None:
        seen[id(p)] = ps


def _sq_norms(self) -> list:
    """[(params, norms)] per plan of the last step (FusedLARS, FusedLAMB): ``norms`` is
    the fp32[2n] tensor the step published, [2t] = Σp², [2t+1] = Σg² (LARS) or Σu² (LAMB)
    of ``params[t]`` (of the values before the update; overwritten by the next step)."""
    return list(self._last_norms)


def _bind_adapt(self, plan, group, ps):
    """The plan's per-tensor adaptation flags from ``group["adapt"]`` and its 2n norm
    scratch ``plan._norms`` (FusedLARS, FusedLAMB), set when the flags change."""
    adapt = group.get("adapt")
    flags = tuple((p.ndim > 1) if adapt is None else bool(adapt) for p in ps)
    if getattr(plan, "_adapt", None) != flags:
        if _capturing():
            raise RuntimeError(f"{self._name}: take one eager step before capturing "
                               "(the plan's adaptation flags and scratch are set there)")
        plan.set_adapt(flags)
        plan._adapt = flags
        plan._norms = torch.zeros(2 * len(ps), dtype=torch.float32, device=ps[0].device)


class _FusedBase(torch.optim.Optimizer):
    _name: str  # the class in error messages (a subclass under another name keeps its parent's)
    _timer_kinds: tuple  # GS_OP_* of the launches kernel_ms() reports

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._plans = _PlanCache()
        self.grad_scale: torch.Tensor | None = None
        self.found_inf: torch.Tensor | None = None
        self._clip_buf: dict = {}
        self._norm_ddp = None  # fuse_grad_norm_into: (ddp, its parameter ids)
        self._dev_hyper: dict = {}  # param-group index -> device hyper-parameter buffers
        self._dense_seen: dict = {}  # id(param) -> strides already checked dense

    @property
    def capturable(self) -> bool:
        return bool(self.defaults.get("capturable"))

    def _group_hyper(self, gi, group, device):
        """Device buffers of group `gi` (capturable mode): ``hyper`` fp32[3]
        read by the update kernel, ``lr`` fp64[1] (Adam's hyper producer)."""
        h = self._dev_hyper.get(gi)
        if h is None or h["hyper"].device != device:
            if _capturing():
                raise RuntimeError("capturable optimizer: take one step outside the graph before capturing it")
            h = {"hyper": torch.zeros(3, dtype=torch.float32, device=device),
                 "lr": torch.zeros(1, dtype=torch.float64, device=device), "lr_host": None}
            self._dev_hyper[gi] = h
        return h

    def refresh_hyper(self):
        """Write each group's host ``lr`` into its device buffer when it changed
        (an eager fill, never recorded: call it outside a capture, before a
        replay — graphs.CapturedStep does)."""
        if _capturing():
            return
        for gi, group in enumerate(self.param_groups):
            h = self._dev_hyper.get(gi)
            if h is not None and h["lr_host"] != group["lr"]:
                lr = float(group["lr"])
                h["lr"].fill_(lr)
                h["hyper"][0:1].fill_(lr)  # SGD reads hyper[0] = fp32(lr); Adam overwrites it
                h["lr_host"] = group["lr"]

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._dev_hyper = {}  # device step counters are re-derived from the loaded state

    def enable_kernel_timer(self, n_slots: int = 256):
        """Time every update-kernel launch with HIP events recorded on its
        launch stream right around the kernel (bench.py's roofline)."""
        self._plans.timer_slots = int(n_slots)
        for plan in self._plans.plans():
            if plan.kind == L.GS_DEV_HIP:
                plan.timer_enable(n_slots)

    def kernel_ms(self) -> list:
        """Durations (ms) of the class's kernels (the updates; LARS / LAMB: the norm /
        moments passes, then the updates) since the last call, all plans (the Σg²
        launches of max_grad_norm are left out)."""
        return [ms for plan in self._plans.plans() if plan.kind == L.GS_DEV_HIP
                for k, v in plan.timer_read_by_kind().items() if k in self._timer_kinds for ms in v]

    def _check_param(self, p):
        """A parameter with a grad: dense grad in the parameter's layout, fp32 parameter."""
        if p.grad.is_sparse:
            raise RuntimeError(f"{self._name} does not support sparse gradients")
        _check_dense(p, p.grad, self._name, self._dense_seen)
        if p.dtype != torch.float32:
            raise RuntimeError(f"{self._name} expects fp32 parameters (keep a fp32 master copy)")

    def _clip_buffer(self, device):
        """[published Σg², coef, norm | accumulated raw Σg² (several plans)] of `device`"""
        buf = self._clip_buf.get(device)
        if buf is None:
            buf = self._clip_buf[device] = torch.zeros(4, dtype=torch.float32, device=device)
        return buf

    def _collect(self, group, by_first=False):
        """{key: (params, grads, momentum buffers)} of the group's parameters with a grad
        (FusedSGD, FusedLARS); a missing buffer is created as zeros.  key = the grad dtype;
        by_first (FusedSGD): (grad dtype, this step created the buffer) — its kernel has a
        first-step form — and every parameter gets its (maybe empty) state entry."""
        out = {}
        for p in group["params"]:
            if p.grad is None:
                continue
            self._check_param(p)
            buf, first = None, False
            st = self.state[p] if group["momentum"] != 0 or by_first else None
            if group["momentum"] != 0:
                buf = st.get("momentum_buffer")
                first = buf is None
                if first:
                    if _capturing():
                        raise RuntimeError(f"{self._name}: momentum buffers must exist before capture "
                                           "(take an eager step first)")
                    buf = st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            ps, gs, bs = out.setdefault((p.grad.dtype, first) if by_first else p.grad.dtype, ([], [], []))
            ps.append(p)
            gs.append(p.grad)
            bs.append(buf)
        return out

    def _device_state(self) -> bool:
        """Step-varying state on the device: capturable mode, the AMP path
        (``found_inf`` set: torch skips ``optimizer.step()`` entirely on an
        overflow, T:amp/grad_scaler.py ``_maybe_opt_step`` — here the kernels
        skip on the device and SGD's first-step flag / Adam's step counter
        advance only on a clean step, so nothing is read on the host), or once
        a group already keeps its counters there."""
        return self.capturable or self.found_inf is not None or bool(self._dev_hyper)

    def fuse_grad_norm_into(self, ddp):
        """Let ``ddp`` (libgsync DistributedDataParallel over exactly this
        optimizer's parameters) compute Σg² of the averaged grads inside its
        bucket unpacks ("partial ‖g‖² fused into unpack"); the
        clipped step then folds that scalar and runs no Σg² pass of its own —
        the clip path's exposed end is the update alone.  The sum runs in bucket
        order instead of the plan's, so the coefficient equals the unfused one
        to fp32 rounding.  Steps without a fresh synchronising backward (no_sync
        accumulation, ``gradient_as_bucket_view``, another parameter set) take
        the unfused path."""
        if not self.defaults.get("max_grad_norm"):
            raise ValueError("fuse_grad_norm_into: the optimizer has no max_grad_norm")
        ddp.set_grad_sqnorm_target(self._clip_buffer(ddp.device)[3:4])
        self._norm_ddp = (ddp, frozenset(id(p) for p in ddp._params))

    def _ddp_sqnorm(self, device):
        """The DDP's fused Σg² when it covers this step's grads, unchanged since
        the unpacks formed it (consumed).  A grad changed in place after backward
        (``GradScaler.unscale_``, ``clip_grad_norm_``, any torch in-place op: the
        grads' version counters moved) leaves the optimizer's own Σg² pass to run."""
        if self._norm_ddp is None:
            return None
        ddp, ids = self._norm_ddp
        if not ddp._sqnorm_valid or ddp.device != device:
            return None
        mine, ver = set(), 0
        for g in self.param_groups:
            for p in g["params"]:
                gr = p.grad
                if gr is not None:
                    mine.add(id(p))
                    ver += gr._version
        ddp._sqnorm_valid = False
        if mine != ids or ver != ddp._sqnorm_versions:
            return None
        return self._clip_buf[device][3:4]

    def _clip_scale(self, device, all_plans):
        """DeepSpeed-style gradient_clipping folded into the update: returns the
        grad multiplier the update launches get.

        Folded path (default): the coefficient min(1, max_norm/(‖g‖+1e-6))
        (times grad_scale) is formed by the update kernel's own workgroups
        (gs_plan_set_clip) — one plan: from the plan's Σg² partial sums
        (gs_sqnorm_partial), so Σg² -> update is two launches with no combine
        and no coefficient launch between them; several plans (grad dtypes):
        Σg² accumulated into one scalar first.  Those two forms are
        bit-identical to the separate path (GSYNC_CLIP_FUSED=0: Σg² + combine,
        gs_clip_coef, mul_ launches).  The DDP-fed form (fuse_grad_norm_into,
        ``last_clip_source == "ddp_unpack"``) sums the same squares in bucket
        order: its coefficient equals the others only to fp32 rounding."""
        max_norm = self.defaults.get("max_grad_norm")
        if not max_norm:
            for plan, _ in all_plans:
                if getattr(plan, "_clip_on", False):
                    plan.set_clip(None)
                    plan._clip_on = False
            return self.grad_scale
        buf = self._clip_buffer(device)
        self.last_grad_norm = buf[2:3]
        if CLIP_FUSED:
            fused = self._ddp_sqnorm(device)
            if fused is not None:
                # Σg² already formed by the DDP's unpacks: no pass over the grads here
                for plan, _ in all_plans:
                    plan.set_clip(float(max_norm), 1e-6, fused, out=buf[0:3])
                    plan._clip_on = True
                self.last_clip_source = "ddp_unpack"
                return self.grad_scale
            self.last_clip_source = "optimizer"
            if len(all_plans) == 1:
                plan, gdt = all_plans[0]
                plan.sqnorm_partial(1, gdt)
                plan.set_clip(float(max_norm), 1e-6, None, out=buf[0:3])
                plan._clip_on = True
            else:
                # the raw sum lives apart from the published triple: every update
                # launch reads it while workgroup 0 of each writes the (scaled) Σg²
                raw = buf[3:4]
                for i, (plan, gdt) in enumerate(all_plans):
                    plan.sqnorm(1, gdt, raw, accumulate=i > 0)
                for plan, _ in all_plans:
                    plan.set_clip(float(max_norm), 1e-6, raw, out=buf[0:3])
                    plan._clip_on = True
            return self.grad_scale  # the kernels fold it into the coefficient
        return self._clip_scale_separate(device, all_plans)

    def _clip_scale_separate(self, device, all_plans):
        """The separate clip path: Σg² over all plans (gs_sqnorm + combine), the
        coefficient min(1, max_norm/(‖g‖+1e-6)) (times grad_scale) by gs_clip_coef
        into the clip buffer [Σg², coef, norm, -], returned as the grad multiplier."""
        max_norm = self.defaults.get("max_grad_norm")
        buf = self._clip_buffer(device)
        sq, coef, norm = buf[0:1], buf[1:2], buf[2:3]
        self.last_grad_norm = norm
        for plan, _ in all_plans:
            if getattr(plan, "_clip_on", False):
                plan.set_clip(None)
                plan._clip_on = False
        for i, (plan, gdt) in enumerate(all_plans):
            plan.sqnorm(1, gdt, sq, accumulate=i > 0)
        if self.grad_scale is not None:
            # norm of the unscaled grads: ‖g·s‖² = s²‖g‖²
            sq.mul_(self.grad_scale * self.grad_scale)
        clip_coef(sq, float(max_norm), 1e-6, coef, norm)
        if self.grad_scale is not None:
            coef.mul_(self.grad_scale)
        return coef


class FusedSGD(_FusedBase):
    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
                 *, maximize=False, foreach=None, differentiable=False, fused=None, max_grad_norm=None,
                 capturable=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if differentiable:
            raise ValueError("FusedSGD does not support differentiable=True")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                        nesterov=nesterov, maximize=maximize, foreach=foreach, differentiable=False,
                        fused=fused, max_grad_norm=max_grad_norm, capturable=bool(capturable))
        super().__init__(params, defaults)

    _name = "FusedSGD"
    _timer_kinds = (L.GS_OP_SGD,)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        dev_state = self._device_state()
        work = []
        for gi, group in enumerate(self.param_groups):
            for (gdt, first), (ps, gs, bs) in self._collect(group, by_first=True).items():
                plan = self._plans.get(ps)
                plan.set_ptrs(0, ps)
                plan.set_ptrs(1, gs)
                plan.set_ptrs(2, [b.data_ptr() if b is not None else 0 for b in bs])
                flag = None
                if dev_state:
                    h = self._group_hyper(gi, group, ps[0].device)
                    if getattr(plan, "_hyper", None) is not h["hyper"]:
                        plan.set_hyper_source(h["hyper"])
                    if group["momentum"] != 0:
                        # first-step flag on the device (hyper[1]): set when this
                        # step creates the buffers, cleared after a step that ran
                        flag = h.setdefault("first_flags", {}).setdefault(
                            id(plan), torch.zeros(1, dtype=torch.float32, device=ps[0].device))
                        if first:
                            flag.fill_(1.0)
                work.append((group, plan, gdt, first, h if dev_state else None, flag))
        if dev_state:
            self.refresh_hyper()
        if not work:
            return loss
        scale = self._clip_scale(work[0][1].device, [(w[1], w[2]) for w in work])
        for group, plan, gdt, first, h, flag in work:
            if flag is not None:
                h["hyper"][1:2].copy_(flag)
            plan.sgd(gdt, group["lr"], group["momentum"], group["dampening"], group["weight_decay"],
                     group["nesterov"], group["maximize"], -1 if flag is not None else first,
                     grad_scale=scale, found_inf=self.found_inf)
            if flag is not None:
                if self.found_inf is not None:
                    flag.mul_(self.found_inf)  # kept only when the step was skipped
                else:
                    flag.zero_()
        return loss


class FusedLARS(_FusedBase):
    """LARS (You et al. 2017; the MLPerf ResNet-50 large-batch optimizer): SGD
    with momentum whose learning rate is multiplied, per tensor, by the trust
    ratio ``trust_coefficient * ‖w‖ / (‖g‖ + weight_decay * ‖w‖ + eps)``.

    Two kernels per (param group, grad dtype): the per-tensor Σp², Σg² of the
    whole list in one pass (``gs_lars_norms``, 8 B/param), then the update
    (``gs_lars_step``, 20 B/param) whose workgroups form their tensor's ratio
    themselves — instead of two ``torch.norm`` per parameter plus the foreach
    update.  The per-tensor sums are deterministic (an order the parameter list
    alone fixes), so data-parallel replicas that hold the same averaged grads
    stay bit-identical.  There is no torch LARS to match: the arithmetic is the
    contract in ``include/gsync.h`` (fp32, every multiply and add rounded once)::

        wn = sqrt(Σp²); gn = sqrt(Σg²) (* grad_scale)
        adapted:    wd_t = wd; ratio = (eta*wn) / ((gn + wd*wn) + eps) if wn > 0 and gn > 0 else 1
        unadapted:  wd_t = 0;  ratio = 1
        g = g (* grad_scale) (+ wd_t*p); buf = buf*momentum + g; p = p - (lr*ratio)*buf

    The param-group key ``adapt`` chooses the adapted tensors: ``None``
    (default) those with ``p.ndim > 1`` — biases and BatchNorm weights get
    neither the trust ratio nor weight decay — ``True`` all, ``False`` none.
    Parameters are fp32 and dense; grads fp32, bf16 or fp16; a parameter whose
    grad is None is skipped.  State is ``momentum_buffer`` (torch SGD's key),
    created as zeros.  ``grad_scale`` / ``found_inf`` behave as in the other
    fused optimizers (``amp.GradScaler`` drives it unchanged), and
    ``capturable=True`` with :meth:`refresh_hyper` lets ``graphs.CapturedStep``
    record it (take one eager step first: state and scratch must exist).

    Under ZeRO-1/2 or with a 16-bit model, LARS is ``ZeroDataParallel(optimizer="lars")``
    (zero.py: per-tensor sums of each rank's pieces, one all-reduce of them).
    Out of scope here: ``max_grad_norm``, nesterov, ``DDP._register_fused_optim``.
    """

    def __init__(self, params, lr=1e-3, momentum=0.9, weight_decay=0.0, trust_coefficient=1e-3, eps=1e-8,
                 *, capturable=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if trust_coefficient < 0.0:
            raise ValueError(f"Invalid trust_coefficient value: {trust_coefficient}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, trust_coefficient=trust_coefficient,
                        eps=eps, adapt=None, capturable=bool(capturable))
        super().__init__(params, defaults)
        self._last_norms: list = []

    _name = "FusedLARS"
    _timer_kinds = (L.GS_OP_LARS_NORM, L.GS_OP_LARS)
    sq_norms = _sq_norms
    _bind_adapt = _bind_adapt

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        dev_state = self._device_state()
        work = []
        for gi, group in enumerate(self.param_groups):
            for gdt, (ps, gs, bs) in self._collect(group).items():
                plan = self._plans.get(ps)
                plan.set_ptrs(0, ps)
                plan.set_ptrs(1, gs)
                if group["momentum"] != 0:
                    plan.set_ptrs(2, bs)
                self._bind_adapt(plan, group, ps)
                if dev_state:
                    h = self._group_hyper(gi, group, ps[0].device)
                    if getattr(plan, "_hyper", None) is not h["hyper"]:
                        plan.set_hyper_source(h["hyper"])
                work.append((group, plan, gdt, ps))
        if dev_state:
            self.refresh_hyper()
        self._last_norms = [(ps, plan._norms) for _, plan, _, ps in work]
        for group, plan, gdt, ps in work:
            plan.lars_norms(gdt, plan._norms)
            plan.lars(gdt, group["lr"], group["momentum"], group["weight_decay"], group["trust_coefficient"],
                      group["eps"], plan._norms, grad_scale=self.grad_scale, found_inf=self.found_inf)
        return loss


class _DeviceSteps:
    """The Adam-family state and step counters (FusedAdam, FusedLAMB)."""

    def _gather(self, cap):
        """Create missing state, advance the host steps (not `cap`) or adopt / split the
        device-counter cohorts (`cap`), and bind one plan per (group, grad dtype, step |
        cohort): slots 0..3 = p, g, exp_avg, exp_avg_sq, and under `cap` the cohort's hyper
        source.  Returns the work list in launch order, entries (group, plan, gdt, step,
        params): plan None = advance the counter of cohort c and form its hyper source
        (step = (h, c)); else step = the host step value, None under `cap` (the kernels
        read the hyper source)."""
        work = []
        for gi, group in enumerate(self.param_groups):
            buckets: dict = {}
            by_cohort: dict = {}
            h = None
            live = []

            def add(key, p):
                st = self.state[p]
                for lst, x in zip(buckets.setdefault(key, ([], [], [], [])),
                                  (p, p.grad, st["exp_avg"], st["exp_avg_sq"])):
                    lst.append(x)

            for p in group["params"]:
                if p.grad is None:
                    continue
                self._check_param(p)
                st = self.state[p]
                if "exp_avg" not in st:
                    if _capturing():
                        raise RuntimeError(f"{self._name}: state must exist before capture (take an eager step first)")
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                live.append(p)
            # every state of this step exists before cohorts are formed: parameters
            # whose state starts together share one cohort (one counter, one plan)
            for p in live:
                st = self.state[p]
                if cap:
                    if h is None:
                        h = self._group_hyper(gi, group, p.device)
                    if id(st["step"]) not in h.get("cohorts", {}):
                        self._adopt_cohorts(h, group)
                    by_cohort.setdefault(id(st["step"]), []).append(p)
                else:
                    st["step"] += 1
                    add((p.grad.dtype, float(st["step"].item())), p)
            for cid, ps in by_cohort.items():
                c = h["cohorts"][cid]
                if len(ps) < len(c["members"]):
                    c = self._split_cohort(h, c, ps)
                work.append((group, None, None, (h, c), None))
                for p in ps:
                    add((p.grad.dtype, id(c["step"])), p)
            cohort_hyper = {id(c["step"]): c["hyper"] for c in h["cohorts"].values()} if h is not None else {}
            for (gdt, step), lists in buckets.items():
                plan = self._plans.get(lists[0])
                for slot, lst in enumerate(lists):
                    plan.set_ptrs(slot, lst)
                if cap:
                    hyper = cohort_hyper[step]
                    if getattr(plan, "_hyper", None) is not hyper:
                        plan.set_hyper_source(hyper)
                    step = None
                work.append((group, plan, gdt, step, lists[0]))
        return work

    # ---- device step counters (capturable / AMP): one fp64 counter per cohort of
    # parameters that have advanced together so far.  torch keeps one step per
    # parameter (T:optim/adam.py: state_steps[i] += 1 only for params with a
    # grad); a cohort shares one counter while all its members get grads, and is
    # split (its counter cloned on the device, no host read) the first step some
    # members have none — so every parameter's bias correction is its own.
    def _adopt_cohorts(self, h, group):
        """Give every stateful parameter of `group` without a device counter one:
        parameters whose (host) step values are equal share a new cohort."""
        cohorts = h.setdefault("cohorts", {})
        by_value: dict = {}
        for p in group["params"]:
            st = self.state.get(p)
            if not st or "exp_avg" not in st:
                continue
            t = st.get("step")
            if t is not None and id(t) in cohorts:
                continue
            if _capturing():
                raise RuntimeError(f"{self._name}: state must exist before capture (take an eager step first)")
            v = 0.0 if t is None else float(t)
            c = by_value.get(v)
            if c is None:
                c = by_value[v] = {"step": torch.full((1,), v, dtype=torch.float64, device=p.device),
                                   "hyper": torch.zeros(3, dtype=torch.float32, device=p.device),
                                   "members": set()}
                cohorts[id(c["step"])] = c
            c["members"].add(id(p))
            st["step"] = c["step"]

    def _split_cohort(self, h, c, ps):
        """Members `ps` (with grads) leave cohort `c` (some of whose members have
        none this step) for a new one starting at the same count."""
        if _capturing():
            raise RuntimeError(f"{self._name}: the set of parameters with grads changed inside a capture")
        n = {"step": c["step"].clone(), "hyper": torch.zeros_like(c["hyper"]), "members": {id(p) for p in ps}}
        c["members"] -= n["members"]
        h["cohorts"][id(n["step"])] = n
        for p in ps:
            self.state[p]["step"] = n["step"]
        return n

    def state_dict(self):
        """torch's layout: one ``step`` tensor per parameter (fp32; on the CPU,
        or on the device when capturable, as torch's Adam keeps it) — device
        counters shared by a cohort are read out here (host read, checkpoint time)."""
        sd = super().state_dict()
        vals: dict = {}
        for k, st in list(sd["state"].items()):
            t = st.get("step")
            if torch.is_tensor(t) and t.dtype == torch.float64:
                v = vals.get(id(t))
                if v is None:
                    v = vals[id(t)] = float(t.item())
                dev = t.device if self.capturable else torch.device("cpu")
                sd["state"][k] = dict(st, step=torch.tensor(v, dtype=torch.float32, device=dev))
        return sd


class FusedAdam(_DeviceSteps, _FusedBase):
    """Adam (``adamw=False``) or AdamW (``adamw=True`` / ``decoupled_weight_decay=True``)."""

    _name = "FusedAdam"
    _timer_kinds = (L.GS_OP_ADAM,)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False,
                 *, foreach=None, maximize=False, capturable=False, differentiable=False, fused=None,
                 decoupled_weight_decay=False, adamw=None, max_grad_norm=None):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if amsgrad:
            raise NotImplementedError("FusedAdam: amsgrad is not on the reference path")
        if differentiable:
            raise ValueError("FusedAdam does not support differentiable=True")
        adamw = bool(decoupled_weight_decay if adamw is None else adamw)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False,
                        foreach=foreach, maximize=maximize, capturable=bool(capturable), differentiable=False,
                        fused=fused, decoupled_weight_decay=adamw, max_grad_norm=max_grad_norm)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        cap = self._device_state()  # device step counters: capturable or AMP (no host read of found_inf)
        work = self._gather(cap)
        plans = [(w[1], w[2]) for w in work if w[1] is not None]
        if not plans:
            return loss
        if cap:
            self.refresh_hyper()
        scale = self._clip_scale(plans[0][0].device, plans)
        for group, plan, gdt, step, _ in work:
            beta1, beta2 = group["betas"]
            if plan is None:  # device counters: advance the cohort's step, form its hyper source
                h, c = step
                L.check(L.lib().gs_adam_hyper(
                    L.GS_DEV_HIP if c["step"].is_cuda else L.GS_DEV_HOST, c["step"].data_ptr(), h["lr"].data_ptr(),
                    float(beta1), float(beta2), float(group["weight_decay"]),
                    None if self.found_inf is None else self.found_inf.data_ptr(), c["hyper"].data_ptr(),
                    L.stream_ptr(c["step"].device) if c["step"].is_cuda else None), "gs_adam_hyper")
                continue
            if step is None:  # the kernel reads step_size / bc2 / decay from the hyper source
                plan.adam(gdt, group["lr"], beta1, beta2, group["eps"], group["weight_decay"],
                          group["decoupled_weight_decay"], group["maximize"], -1.0, 1.0,
                          grad_scale=scale, found_inf=self.found_inf)
                continue
            lr = group["lr"]
            # python-double bias corrections, as torch's foreach path computes them
            bias_correction1 = 1 - beta1 ** step
            bias_correction2 = 1 - beta2 ** step
            step_size = (lr / bias_correction1) * -1
            bias_correction2_sqrt = bias_correction2 ** 0.5
            plan.adam(gdt, lr, beta1, beta2, group["eps"], group["weight_decay"],
                      group["decoupled_weight_decay"], group["maximize"], step_size, bias_correction2_sqrt,
                      grad_scale=scale, found_inf=self.found_inf)
        return loss


class FusedAdamW(FusedAdam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, **kw):
        kw.pop("decoupled_weight_decay", None)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, adamw=True, **kw)


class FusedLAMB(_DeviceSteps, _FusedBase):
    """LAMB (You et al. 2019; DeepSpeed's ``FusedLamb``, ColossalAI's ``Lamb`` /
    ``FusedLAMB``, apex's ``FusedLAMB``): Adam whose update is multiplied, per
    tensor, by the trust ratio ``‖w‖ / ‖update‖``.

    Two kernels per (param group, grad dtype): ``gs_lamb_moments`` advances
    ``exp_avg`` / ``exp_avg_sq`` and publishes the per-tensor Σp², Σu² in one
    deterministic pass (24 B/param), then ``gs_lamb_step`` recomputes the update
    from the stored moments and writes p (16 B/param) — instead of a
    ``torch.norm`` pair per parameter plus the foreach moments and update.  There
    is no torch LAMB to match: the arithmetic is the contract in
    ``include/gsync.h`` (fp32, every operation rounded once)::

        g = g (* grad multiplier); m = m*b1 + (1-b1)*g; v = v*b2 + ((1-b2)*g)*g
        u = (m/bc1) / (sqrt(v)/sqrt(bc2) + eps) (+ wd*p on adapted tensors)
        adapted:   ratio = clamp(‖p‖/‖u‖, min_trust, max_trust) if ‖p‖ > 0 and ‖u‖ > 0 else 1
        unadapted: ratio = 1 (plain Adam, no decay)
        p = p - (lr*ratio)*u

    The param-group key ``adapt`` works as in :class:`FusedLARS`: ``None``
    (default) adapts the tensors with ``p.ndim > 1``, ``True`` all, ``False``
    none.  State is ``step``, ``exp_avg``, ``exp_avg_sq`` (torch Adam's keys).
    Parameters are fp32 and dense; grads fp32, bf16 or fp16, one plan per (group,
    grad dtype).  ``grad_scale`` / ``found_inf`` behave as in the other fused
    optimizers (``amp.GradScaler`` drives it unchanged).  ``max_grad_norm`` is
    apex / DeepSpeed LAMB's global pre-normalisation: Σg² over all plans, the
    clip coefficient on the device, passed as the grad multiplier (the separate
    clip path; LAMB does not take the clip folded into the update).
    ``capturable=True`` with :meth:`refresh_hyper` lets ``graphs.CapturedStep``
    record it (take one eager step first: state and scratch must exist).

    Under ZeRO-1/2 or with a 16-bit model, LAMB is ``ZeroDataParallel(optimizer="lamb")``
    (zero.py: per-tensor sums of each rank's pieces, one all-reduce of them).
    Out of scope here: ``DDP._register_fused_optim``, amsgrad.
    """

    _name = "FusedLAMB"
    _timer_kinds = (L.GS_OP_LAMB_MOMENTS, L.GS_OP_LAMB)
    sq_norms = _sq_norms
    _bind_adapt = _bind_adapt

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, bias_correction=True,
                 min_trust=None, max_trust=None, max_grad_norm=None, *, capturable=False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        lo = 0.0 if min_trust is None else float(min_trust)
        hi = math.inf if max_trust is None else float(max_trust)
        if not 0.0 <= lo <= hi:
            raise ValueError(f"Invalid trust-ratio clamp: [{min_trust}, {max_trust}]")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                        bias_correction=bool(bias_correction), min_trust=min_trust, max_trust=max_trust,
                        max_grad_norm=max_grad_norm, adapt=None, capturable=bool(capturable))
        super().__init__(params, defaults)
        self._last_norms: list = []

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        cap = self._device_state()  # device step counters: capturable or AMP (no host read of found_inf)
        work = self._gather(cap)
        plans = [(w[1], w[2]) for w in work if w[1] is not None]
        if not plans:
            return loss
        for group, plan, _, _, ps in work:
            if plan is not None:
                self._bind_adapt(plan, group, ps)
        if cap:
            self.refresh_hyper()
        self._last_norms = [(w[4], w[1]._norms) for w in work if w[1] is not None]
        scale = self.grad_scale
        if self.defaults.get("max_grad_norm"):
            scale = self._clip_scale_separate(plans[0][0].device, plans)
        for group, plan, gdt, step, _ in work:
            beta1, beta2 = group["betas"]
            if plan is None:  # device counters: advance the cohort's step, form its hyper source
                h, c = step
                L.check(L.lib().gs_lamb_hyper(
                    L.GS_DEV_HIP if c["step"].is_cuda else L.GS_DEV_HOST, c["step"].data_ptr(), h["lr"].data_ptr(),
                    float(beta1), float(beta2), int(group["bias_correction"]),
                    None if self.found_inf is None else self.found_inf.data_ptr(), c["hyper"].data_ptr(),
                    L.stream_ptr(c["step"].device) if c["step"].is_cuda else None), "gs_lamb_hyper")
                continue
            bc1 = bc2s = 1.0  # step is None: the kernels read lr, bc1, bc2s from the hyper source
            if step is not None and group["bias_correction"]:
                bc1 = 1 - beta1 ** step
                bc2s = math.sqrt(1 - beta2 ** step)
            lo = 0.0 if group["min_trust"] is None else group["min_trust"]
            hi = math.inf if group["max_trust"] is None else group["max_trust"]
            norms = plan._norms
            plan.lamb_moments(gdt, beta1, beta2, group["eps"], group["weight_decay"], bc1, bc2s, norms,
                              grad_scale=scale, found_inf=self.found_inf)
            plan.lamb(group["lr"], group["eps"], group["weight_decay"], bc1, bc2s, norms, lo, hi,
                      found_inf=self.found_inf)
        return loss


class FusedMuon(_FusedBase):
    """Muon (``torch.optim.Muon``: signature, defaults, validation and the
    ``momentum_buffer`` state key, so ``state_dict()`` moves between the two): SGD
    momentum whose update matrix is orthogonalised by ``ns_steps`` quintic
    Newton-Schulz iterations on bf16 operands.

    torch runs about 20 launches per parameter and step (two lerps, cast, norm, div,
    three GEMMs per iteration, two updates) and refuses ``foreach``.  Here every stage is
    one grouped launch over the whole (param group, grad dtype) list, so a step is
    ``3 * ns_steps + 3`` timed operations whatever the number of tensors:
    ``gs_muon_prep`` (the segmented per-tensor Σu² pass LARS and LAMB share, which also
    advances the momentum, then the pass that writes ``X = bf16(u / max(‖u‖, eps))``),
    per iteration ``gs_muon_gram`` / ``gs_muon_poly`` / ``gs_muon_apply`` (bf16 MFMA,
    fp32 accumulation, symmetric stages computed on the upper triangle only), and
    ``gs_muon_update``.  The arithmetic is the contract in ``include/gsync.h``: torch's
    rounding points, except that the norm is taken in fp32; the accumulation order
    inside a product is the kernel's own, so results agree with torch to bf16 rounding,
    not bit for bit, and are bit-reproducible run to run.

    Parameters are fp32 and dense: 2-D, or — an extension over torch — 4-D conv filters
    whose dim 0 has the largest stride.  Such a weight is the row-major matrix
    ``[shape[0], numel / shape[0]]`` in memory order; for a ``channels_last`` filter
    that is a column permutation of the logical flattening, which Newton-Schulz
    commutes with.  Anything else raises ``ValueError``.  Grads are fp32, bf16 or fp16
    in the parameter's layout; a parameter whose grad is None is skipped.
    ``adjust_lr_fn`` is torch's (``None`` / ``"original"``, ``"match_rms_adamw"``) with
    ``A = shape[0]``, ``B = numel / shape[0]``.

    The usual composition keeps everything that is not a filter off Muon::

        filters = [p for p in model.parameters() if p.ndim == 4]
        rest = [p for p in model.parameters() if p.ndim != 4]   # BatchNorm, biases, fc
        opts = [FusedMuon(filters, lr=0.02), FusedAdamW(rest, lr=1e-3)]   # or FusedSGD

    Out of scope, each an error: ``grad_scale`` / ``found_inf`` (AMP), ``capturable=True``,
    ``max_grad_norm``, ZeRO sharding of Muon (a matrix split across ranks), the DeepSpeed /
    ColossalAI shims, ``DDP._register_fused_optim``.
    """

    _name = "FusedMuon"
    _timer_kinds = (L.GS_OP_MUON_PREP, L.GS_OP_MUON_GRAM, L.GS_OP_MUON_POLY, L.GS_OP_MUON_APPLY,
                    L.GS_OP_MUON_UPDATE)

    def __init__(self, params, lr=1e-3, weight_decay=0.1, momentum=0.95, nesterov=True,
                 ns_coefficients=(3.4445, -4.7750, 2.0315), eps=1e-7, ns_steps=5, adjust_lr_fn=None,
                 *, capturable=False, max_grad_norm=None):
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if not 0.0 <= lr:
            raise ValueError(f"Learning rate should be >= 0 but is: {lr}")
        if not 0.0 <= momentum:
            raise ValueError(f"momentum should be >= 0 but is: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"weight decay should be >= 0 but is: {weight_decay}")
        if adjust_lr_fn is not None and adjust_lr_fn not in ["original", "match_rms_adamw"]:
            raise ValueError(f"Adjust learning rate function {adjust_lr_fn} is not supported")
        if capturable:
            raise ValueError("FusedMuon does not support capturable=True")
        if max_grad_norm:
            raise ValueError("FusedMuon does not support max_grad_norm (clip the grads before the step)")
        defaults = dict(lr=lr, weight_decay=weight_decay, momentum=momentum, nesterov=nesterov,
                        ns_coefficients=ns_coefficients, eps=eps, ns_steps=ns_steps, adjust_lr_fn=adjust_lr_fn)
        super().__init__(params, defaults)
        for group in self.param_groups:
            for p in group["params"]:
                if p.ndim not in (2, 4):
                    raise ValueError("FusedMuon only supports 2D parameters and 4D conv filters whereas we found "
                                     f"a parameter with size: {p.size()}")
                if p.numel() == 0 or not is_dense(p) or p.stride(0) * p.shape[0] != p.numel():
                    raise ValueError("FusedMuon: dim 0 of a parameter must be its outermost dimension in memory "
                                     f"(size {tuple(p.size())}, strides {p.stride()})")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.grad_scale is not None or self.found_inf is not None:
            raise RuntimeError("FusedMuon does not support grad_scale / found_inf (unscale the grads and skip "
                               "the step on the host)")
        for group in self.param_groups:
            coef = tuple(group["ns_coefficients"])
            if group["ns_steps"] >= 100:
                raise ValueError("Number of steps must be less than 100 for computational efficiency")
            if len(coef) != 3:
                raise ValueError("Coefficients must be a tuple of exactly 3 values")
            a, b, c = coef
            # torch's Muon keeps the buffer whatever the momentum (lerp with weight 1 at 0)
            for gdt, (ps, gs, bs) in self._collect(dict(group, momentum=1.0)).items():
                plan = self._plans.get(ps)
                for slot, lst in enumerate((ps, gs, bs)):
                    plan.set_ptrs(slot, lst)
                ws = getattr(plan, "_muon_space", None)
                if ws is None:
                    plan.muon_layout([p.shape[0] for p in ps])
                    ws = plan._muon_space = plan.muon_workspace()
                    plan._norms = torch.zeros(2 * len(ps), dtype=torch.float32, device=ps[0].device)
                plan.muon_prep(gdt, group["momentum"], group["nesterov"], group["eps"], plan._norms, ws)
                x = 0
                for _ in range(int(group["ns_steps"])):
                    plan.muon_gram(ws, x)
                    plan.muon_poly(ws, b, c)
                    plan.muon_apply(ws, x, a)
                    x ^= 1
                plan.muon_update(ws, x, group["lr"], group["weight_decay"], group["adjust_lr_fn"])
        return loss


def _adafactor_descriptor(p: torch.Tensor):
    """((O, I, R, C, so, si, sr, sc), is a vector) of a parameter FusedAdafactor supports:
    torch factors the last two dims and batches the ones before them."""
    what = f"size {tuple(p.size())}, strides {p.stride()}, {p.dtype}"
    if p.dtype != torch.float32 or p.layout != torch.strided:
        raise ValueError(f"FusedAdafactor only supports dense fp32 parameters (got {what})")
    if p.numel() == 0:
        raise ValueError(f"FusedAdafactor does not support empty parameters (got {what})")
    if p.ndim == 0:
        return (1, 1, 1, 1, 0, 0, 0, 0), True
    if p.ndim == 1 and (p.numel() == 1 or p.stride(0) == 1):
        return (1, p.numel(), 1, 1, 0, 1, 0, 0), True
    if p.ndim == 2 and p.is_contiguous():
        return (1, 1, p.shape[0], p.shape[1], 0, 0, p.shape[1], 1), False
    if p.ndim == 4 and (p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last)):
        if p.shape[2] * p.shape[3] > 64 and p.shape[3] > 1 and p.stride(3) != 1:
            raise ValueError("FusedAdafactor: a filter of more than 64 taps must be contiguous, not channels_last "
                             f"(got {what})")
        return tuple(p.shape) + tuple(p.stride()), False
    raise ValueError("FusedAdafactor supports 0-D, 1-D, contiguous 2-D and contiguous or channels_last 4-D "
                     f"parameters (got {what})")


class FusedAdafactor(_FusedBase):
    """Adafactor (``torch.optim.Adafactor``: signature, defaults, validation and the ``step``
    / ``row_var`` / ``col_var`` / ``variance`` state keys, so ``state_dict()`` moves between
    the two): a row factor and a column factor in place of a full second moment.

    torch runs about fifteen launches per parameter and step and reads ``param.norm(2)`` and
    ``update.norm(2)`` back with ``.item()`` — two host synchronisations per parameter, with
    ``foreach`` too.  Here a step over a (param group, step value) list is at most 7 grouped
    launches whatever the number of tensors and nothing is read back: ``gs_adafactor_stats``
    (the factors advance and the per-tensor Σp², Σu² are summed in a fixed order, no
    atomics) and ``gs_adafactor_step`` (alpha and the update clip formed on the device).
    The arithmetic is the contract in ``include/gsync.h``: torch's ``_single_tensor_adafactor``
    in fp32 with the row / column means taken as Σg² / n; the sums' order is the kernels'
    own, so results agree with torch to fp32 rounding, not bit for bit, and are
    bit-reproducible run to run.

    Parameters are dense fp32 with fp32 grads in the same layout: 0-D, 1-D, contiguous 2-D,
    and 4-D filters, contiguous or ``channels_last`` (factored over ``(kh, kw)`` with
    ``(O, I)`` as the batch, as torch does; a ``channels_last`` filter of more than 64 taps is
    refused).  Anything else raises ``ValueError``.  A parameter whose grad is None is
    skipped and its ``step`` does not advance.  ``foreach`` is accepted and ignored.

    Out of scope, each an error: 16-bit parameters or grads, ``grad_scale`` / ``found_inf``
    (AMP), ``capturable``, ZeRO sharding, the DeepSpeed / ColossalAI shims,
    ``DDP._register_fused_optim``.
    """

    _name = "FusedAdafactor"
    _timer_kinds = (L.GS_OP_ADAFACTOR_STATS, L.GS_OP_ADAFACTOR_STEP)

    def __init__(self, params, lr=1e-2, beta2_decay=-0.8, eps=(None, 1e-3), d=1.0, weight_decay=0.0, *,
                 foreach=None, maximize=False):
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if not 0.0 <= lr:
            raise ValueError(f"Learning rate should be >= 0 but is: {lr}")
        if not 0.0 >= beta2_decay:
            raise ValueError(f"beta2_decay should be <= 0 but is: {beta2_decay}")
        if eps[0] is not None and not 0.0 <= eps[0]:
            raise ValueError(f"epsilon1 should be >= 0 but is: {eps[0]}")
        if not 0.0 <= eps[1]:
            raise ValueError(f"epsilon2 should be >= 0 but is: {eps[1]}")
        if not 1.0 <= d:
            raise ValueError(f"Clipping threshold d should be >= 1 but is: {d}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"weight_decay should be >= 0 but is: {weight_decay}")
        defaults = dict(lr=lr, beta2_decay=beta2_decay, eps=eps, d=d, weight_decay=weight_decay, foreach=foreach,
                        maximize=maximize)
        super().__init__(params, defaults)
        for group in self.param_groups:
            for p in group["params"]:
                _adafactor_descriptor(p)

    def _factors(self, p):
        """The parameter's state, created as torch creates it; (slot 2, slot 3) of its plan."""
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.get_default_dtype())
            if p.grad.dim() > 1:
                shape = list(p.grad.shape)
                st["row_var"] = p.grad.new_zeros(shape[:-1] + [1])
                st["col_var"] = p.grad.new_zeros(shape[:-2] + [1, shape[-1]])
            else:
                st["variance"] = torch.zeros_like(p.grad, memory_format=torch.preserve_format)
        for key in ("row_var", "col_var", "variance"):  # a loaded state: the kernels index it contiguously
            if key in st and not (st[key].is_contiguous() and st[key].dtype == torch.float32):
                st[key] = st[key].to(torch.float32).contiguous()
        if p.grad.dim() > 1:
            return st["row_var"], st["col_var"]
        return st["variance"], None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.grad_scale is not None or self.found_inf is not None:
            raise RuntimeError("FusedAdafactor does not support grad_scale / found_inf (unscale the grads and skip "
                               "the step on the host)")
        for group in self.param_groups:
            eps1, eps2 = group["eps"]
            if eps1 is None:
                eps1 = torch.finfo(torch.float32).eps
            lr = group["lr"].item() if isinstance(group["lr"], torch.Tensor) else group["lr"]
            cohorts: dict = {}  # step value -> (params, grads, slot 2, slot 3): w and rho are launch scalars
            for p in group["params"]:
                if p.grad is None:
                    continue
                self._check_param(p)
                if p.grad.dtype != torch.float32:
                    raise RuntimeError(f"FusedAdafactor expects fp32 grads (got {p.grad.dtype})")
                s2, s3 = self._factors(p)
                st = self.state[p]
                st["step"] += 1
                lists = cohorts.setdefault(st["step"].item(), ([], [], [], []))  # a CPU scalar: no device read
                for lst, x in zip(lists, (p, p.grad, s2, s3)):
                    lst.append(x)
            for step, (ps, gs, s2, s3) in cohorts.items():
                plan = self._plans.get(ps)
                plan.set_ptrs(0, ps)
                plan.set_ptrs(1, gs)
                for slot, lst in ((2, s2), (3, s3)):  # the factors are smaller than their tensor: raw pointers
                    plan.set_ptrs(slot, [None if x is None else x.data_ptr() for x in lst])
                ws = getattr(plan, "_adafactor_space", None)
                if ws is None:
                    descs, vectors = zip(*(_adafactor_descriptor(p) for p in ps))
                    plan.adafactor_layout(descs, vectors)
                    ws = plan._adafactor_space = plan.adafactor_workspace()
                    plan._norms = torch.zeros(2 * len(ps), dtype=torch.float32, device=ps[0].device)
                plan.adafactor_stats(step ** group["beta2_decay"], eps1, plan._norms, ws)
                plan.adafactor_step(min(lr, 1 / (step ** 0.5)), lr, group["weight_decay"], eps1, eps2, group["d"],
                                    group["maximize"], plan._norms, ws)
        return loss


class FusedCAME(_FusedBase):
    """CAME (Luo et al., ACL 2023; ``colossalai.nn.optimizer.CAME``: signature, defaults,
    validation and state keys, so a ``state_dict()`` moves across): Adafactor's factored second
    moment, a full-size momentum ``exp_avg`` of the clipped direction, and a second pair of
    factors over the instability ``(û - m)²`` that scales the momentum into the update.

    The published code runs about 30 launches per parameter and step.  Here a step over a
    param group is at most 9 grouped launches whatever the number of tensors and nothing is
    read back: ``gs_came_stats`` (r, c and the per-tensor Σu²), ``gs_came_moment`` and
    ``gs_came_step``.  The arithmetic is the contract in ``include/gsync.h``; every sum's order
    is fixed by the layout, so results agree with the published code to fp32 rounding and are
    bit-reproducible run to run.

    State per parameter: ``step`` (an int), ``exp_avg``, and ``exp_avg_sq_row`` /
    ``exp_avg_sq_col`` / ``exp_avg_res_row`` / ``exp_avg_res_col`` for ``ndim >= 2``, else
    ``exp_avg_sq``.  The published code's informational ``RMS`` entry is not kept.

    Parameters are those ``FusedAdafactor`` accepts: dense fp32 with fp32 grads in the same
    layout, 0-D, 1-D (not factored), contiguous 2-D, and 4-D filters, contiguous or
    ``channels_last`` (factored over ``(kh, kw)`` with ``(O, I)`` as the batch, 1x1 filters
    included).  A parameter whose grad is None is skipped and its ``step`` does not advance.

    Errors: 16-bit parameters or grads, ``grad_scale`` / ``found_inf`` (AMP), capture.  Not
    supported: ZeRO sharding, the DeepSpeed / ColossalAI shims, ``DDP._register_fused_optim``.
    """

    _name = "FusedCAME"
    _timer_kinds = (L.GS_OP_CAME_STATS, L.GS_OP_CAME_MOMENT, L.GS_OP_CAME_STEP)
    _FACTORS = ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_res_row", "exp_avg_res_col")

    def __init__(self, params, lr=None, eps=(1e-30, 1e-16), clip_threshold=1.0, betas=(0.9, 0.999, 0.9999),
                 weight_decay=0.0):
        if lr is None or not lr > 0.0:
            raise ValueError(f"FusedCAME: lr is required and must be > 0 (got {lr})")
        if len(betas) != 3 or not all(0.0 <= beta <= 1.0 for beta in betas):
            raise ValueError(f"FusedCAME: the three betas must lie in [0, 1] (got {betas})")
        defaults = dict(lr=lr, eps=eps, clip_threshold=clip_threshold, betas=betas, weight_decay=weight_decay)
        super().__init__(params, defaults)
        for group in self.param_groups:
            for p in group["params"]:
                _adafactor_descriptor(p)

    def _state(self, p):
        """The parameter's state, created as the published code creates it; slots 2 to 6 of its plan."""
        st = self.state[p]
        g = p.grad
        if len(st) == 0:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(g, memory_format=torch.preserve_format)
            if g.dim() >= 2:
                for key in self._FACTORS:
                    st[key] = g.new_zeros(g.shape[:-2] + g.shape[-1:] if key.endswith("col") else g.shape[:-1])
            else:
                st["exp_avg_sq"] = torch.zeros_like(g)
        if st["exp_avg"].stride() != p.stride() or st["exp_avg"].dtype != torch.float32:  # a loaded state
            m = torch.empty_like(p, memory_format=torch.preserve_format)
            st["exp_avg"] = m.copy_(st["exp_avg"])
        keys = self._FACTORS if g.dim() >= 2 else ("exp_avg_sq",)
        for key in keys:  # the kernels index the factors contiguously
            if not (st[key].is_contiguous() and st[key].dtype == torch.float32):
                st[key] = st[key].to(torch.float32).contiguous()
        if g.dim() >= 2:
            return [st[k] for k in self._FACTORS[:2]] + [st["exp_avg"]] + [st[k] for k in self._FACTORS[2:]]
        return [st["exp_avg_sq"], None, st["exp_avg"], None, None]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.grad_scale is not None or self.found_inf is not None:
            raise RuntimeError("FusedCAME does not support grad_scale / found_inf (unscale the grads and skip "
                               "the step on the host)")
        if _capturing():
            raise RuntimeError("FusedCAME does not support graph capture")
        for group in self.param_groups:
            ps, slots = [], ([], [], [], [], [], [])  # slots 1 to 6
            for p in group["params"]:
                if p.grad is None:
                    continue
                self._check_param(p)
                if p.grad.dtype != torch.float32:
                    raise RuntimeError(f"FusedCAME expects fp32 grads (got {p.grad.dtype})")
                state = self._state(p)
                self.state[p]["step"] += 1
                ps.append(p)
                for lst, x in zip(slots, [p.grad] + state):
                    lst.append(x)
            if not ps:
                continue
            plan = self._plans.get(ps)
            plan.set_ptrs(0, ps)
            plan.set_ptrs(1, slots[0])
            for slot, lst in enumerate(slots[1:], start=2):  # the factors are smaller than their tensor: raw pointers
                plan.set_ptrs(slot, [None if x is None else x.data_ptr() for x in lst])
            ws = getattr(plan, "_adafactor_space", None)
            if ws is None:
                descs, vectors = zip(*(_adafactor_descriptor(p) for p in ps))
                plan.adafactor_layout(descs, vectors)
                ws = plan._adafactor_space = plan.adafactor_workspace()
                plan._norms = torch.zeros(len(ps), dtype=torch.float32, device=ps[0].device)
            (eps1, eps2), (beta1, beta2, beta3) = group["eps"], group["betas"]
            plan.came_stats(beta2, eps1, plan._norms, ws)
            plan.came_moment(beta1, beta3, eps2, group["clip_threshold"], plan._norms, ws)
            plan.came_step(beta1, beta3, eps2, group["clip_threshold"], group["lr"], group["weight_decay"],
                           plan._norms, ws)
        return loss


_NORM_PLANS: dict = {}


@torch.no_grad()
def clip_grad_norm_(parameters: torch.Tensor | Iterable[torch.Tensor], max_norm: float, norm_type: float = 2.0,
                    error_if_nonfinite: bool = False, foreach=None) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ for the L2 norm on libgsync kernels.

    total_norm = ‖concat(g)‖₂ ; coef = clamp(max_norm / (total_norm + 1e-6), max=1);
    grads *= coef (T:nn/utils/clip_grad.py:165-174).  Everything stays on the
    device; only error_if_nonfinite forces a host read, as in torch.

    One grad dtype (the common case) is two launches: the Σg² partial sums
    (gs_sqnorm_partial, left in the plan), then the scale pass whose every
    workgroup folds them into the coefficient itself (gs_clip_scale; it writes
    nothing when the coefficient is 1).  No combine launch, no coefficient
    launch, no flag fill.  Several grad dtypes: Σg² accumulated over the groups
    (gs_sqnorm), then each group's scale pass folds that scalar.
    """
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if float(norm_type) != 2.0:
        raise NotImplementedError("clip_grad_norm_: only norm_type=2 is on the gradient-sync path")
    if len(grads) == 0:
        return torch.tensor(0.0)
    dev = grads[0].device
    groups: dict = {}
    for g in grads:
        if not is_dense(g):
            raise RuntimeError("clip_grad_norm_: grads must be dense")
        groups.setdefault(g.dtype, []).append(g)
    # [Σg², coef, norm | accumulated Σg² (several dtypes)]: written by the kernels before
    # any read (workgroup 0 of the scale pass publishes the first three), so no fill
    buf = torch.empty(4, dtype=torch.float32, device=dev)
    plans = []
    for dt, gl in groups.items():
        key = tuple(g.numel() for g in gl) + (dev,)  # sizes + device: grad ids are reused after zero_grad
        plan = _NORM_PLANS.get(key)
        if plan is None:
            plan = TensorListPlan([g.numel() for g in gl], dev)
            if len(_NORM_PLANS) > 64:
                _NORM_PLANS.clear()
            _NORM_PLANS[key] = plan
        plan.set_ptrs(0, gl)
        plans.append((plan, dt))
    if len(plans) == 1 and not error_if_nonfinite:
        plan, dt = plans[0]
        plan.sqnorm_partial(0, dt)
        plan.set_clip(float(max_norm), 1e-6, None, out=buf[0:3])
    else:
        raw = buf[3:4]
        for i, (plan, dt) in enumerate(plans):
            plan.sqnorm(0, dt, raw, accumulate=i > 0)
        # torch raises before touching the grads (T:nn/utils/clip_grad.py:96-109)
        if error_if_nonfinite and not torch.isfinite(raw).item():
            raise RuntimeError(
                f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, "
                "so it cannot be clipped. To disable this error and scale the gradients by the non-finite "
                "norm anyway, set `error_if_nonfinite=False`")
        for plan, _ in plans:
            plan.set_clip(float(max_norm), 1e-6, raw, out=buf[0:3])
    for plan, dt in plans:
        plan.clip_scale(0, dt)
        plan.set_clip(None)
    norm = buf[2:3]
    # the kernel wrote the grads in place: tell autograd's version counters, as a
    # torch in-place op would (a DDP's fused Σg² of these grads is stale now)
    increment_version(grads)
    return norm.reshape(())
