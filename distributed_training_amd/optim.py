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
