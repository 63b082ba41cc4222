"""Shared by tests/test_lamb_cpu.py and tests/test_gpu_lamb.py: a numpy float32
restatement of the LAMB contract (include/gsync.h, gs_lamb_moments / gs_lamb_step),
written from the contract alone — it never calls the library — and the runs both
modules make, on CPU tensors (host backend) or on the GPU.  The tensor list is
tests/_lars_common.py's (SIZES, ADAPT).

The restatement has two halves: :func:`ref_moments` (pass 1: the new moments and
the update u, whose squares the library sums) and :func:`ref_update` (pass 2 given
the per-tensor sums).  Every numpy operation works on float32 operands and rounds
once, which is the contract's "no fma" arithmetic op for op.
"""
import math

import numpy as np
import torch

from tests._lars_common import (ADAPT, ADAPT2, I_OFFSET, I_ZERO_G, I_ZERO_P, SIZES, SIZES2, F,  # noqa: F401
                                assert_lists_equal, assert_sums_close, small_model, synthetic_grads, to_np)


def bias_corrections(beta1, beta2, step, on=True):
    """(bc1, bc2s) formed in double, as the host forms them."""
    if not on:
        return 1.0, 1.0
    return 1.0 - beta1 ** step, math.sqrt(1.0 - beta2 ** step)


def _u(p, m, v, bc1, bc2s, eps, wd_t):
    with np.errstate(invalid="ignore", divide="ignore"):
        u = (m / bc1) / (np.sqrt(v) / bc2s + eps)
    if wd_t != 0:
        u = u + wd_t * p
    assert u.dtype == F
    return u


def ref_moments(p, g, m, v, adapt, beta1, beta2, eps, wd, bc1, bc2s, mult=None):
    """Pass 1 on numpy float32 lists: returns the new (m, v) and u."""
    b1, b2, w1, w2 = F(beta1), F(beta2), F(1.0 - beta1), F(1.0 - beta2)
    bc1, bc2s, eps, wd = F(bc1), F(bc2s), F(eps), F(wd)
    nm, nv, us = [], [], []
    for t in range(len(p)):
        gt = g[t]
        if mult is not None:
            gt = gt * F(mult)
        mt = m[t] * b1 + w1 * gt
        vt = v[t] * b2 + (w2 * gt) * gt
        assert mt.dtype == F and vt.dtype == F
        nm.append(mt)
        nv.append(vt)
        us.append(_u(p[t], mt, vt, bc1, bc2s, eps, wd if adapt[t] else F(0)))
    return nm, nv, us


def ref_ratios(sums, adapt, lo=0.0, hi=math.inf):
    lo, hi = F(lo), F(hi)
    out = []
    for t in range(len(adapt)):
        ratio = F(1)
        if adapt[t]:
            wn, un = np.sqrt(F(sums[2 * t])), np.sqrt(F(sums[2 * t + 1]))
            if wn > 0 and un > 0:
                ratio = wn / un
                if ratio < lo:
                    ratio = lo
                if ratio > hi:
                    ratio = hi
        out.append(F(ratio))
    return out


def ref_update(p, m, v, sums, adapt, lr, eps, wd, bc1, bc2s, lo=0.0, hi=math.inf):
    """Pass 2 given the per-tensor sums [2t] = Σp², [2t+1] = Σu²: returns the new p."""
    lr, bc1, bc2s, eps, wd = F(lr), F(bc1), F(bc2s), F(eps), F(wd)
    ratios = ref_ratios(sums, adapt, lo, hi)
    out = []
    for t in range(len(p)):
        slr = lr * ratios[t]
        u = _u(p[t], m[t], v[t], bc1, bc2s, eps, wd if adapt[t] else F(0))
        pt = p[t] - slr * u
        assert slr.dtype == F and pt.dtype == F
        out.append(pt)
    return out


def ref_sums(p, u):
    """[2t] = Σp², [2t+1] = Σu² in float32 (exact, hence order-free, on the exact-sum inputs)."""
    out = np.zeros(2 * len(p), dtype=F)
    for t, (x, y) in enumerate(zip(p, u)):
        out[2 * t] = np.sum(x * x, dtype=F)
        out[2 * t + 1] = np.sum(y * y, dtype=F)
    return out


# ---- the tensor list
def _place(x, i, device):
    if i == I_OFFSET:  # one element into its storage: not 16-B aligned
        store = torch.zeros(x.numel() + 1, dtype=x.dtype, device=device)
        store[1:].copy_(x)
        x = store[1:]
        assert x.data_ptr() % 16 != 0
        return x
    return x.to(device)


def make_tensors(device, gdt, exact, seed, what="pgmv", sizes=SIZES):
    """Lists of the tensor list drawn on the CPU from `seed` (the zero tensors and the
    offset one are SIZES' alone).

    exact: p in multiples of 0.5 in [-2, 2], g in non-zero multiples of 0.5 in [-2, 2]
    (no zero-g tensor), m = v = 0.  Otherwise normal draws, v as squares (>= 0); the
    zero-g tensor has m = v = 0 too, so its update is the decay term alone."""
    gen = torch.Generator().manual_seed(seed)
    out = {k: [] for k in what}
    special = sizes is SIZES
    for i, n in enumerate(sizes):
        for k in what:
            if exact:
                if k == "p":
                    x = torch.randint(-4, 5, (n,), generator=gen).float() * 0.5
                elif k == "g":
                    x = torch.randint(1, 5, (n,), generator=gen).float() * 0.5
                    x = x * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1)
                else:
                    x = torch.zeros(n)
            else:
                x = torch.randn(n, generator=gen)
                if k == "v":
                    x = x * x
                if special and k in "gmv" and i == I_ZERO_G:
                    x = torch.zeros(n)
            if special and k == "p" and i == I_ZERO_P:
                x = torch.zeros(n)
            out[k].append(_place(x.to(gdt if k == "g" else torch.float32), i if special else -1, device))
    return [out[k] for k in what]


def make_plan(device, p, g, m, v, adapt=ADAPT, sizes=SIZES):
    from distributed_training_amd.multi_tensor import TensorListPlan

    plan = TensorListPlan(sizes, device)
    for s, ts in enumerate((p, g, m, v)):
        plan.set_ptrs(s, ts)
    plan.set_adapt(adapt)
    return plan


def new_norms(device, n=len(SIZES)):
    return torch.zeros(2 * n, dtype=torch.float32, device=device)


def plan_step(plan, gdt, norms, hp, step, mult=None, found_inf=None, lo=0.0, hi=math.inf):
    """Both library calls of one step; hp = dict(lr, betas, eps, wd, bias_correction)."""
    bc1, bc2s = bias_corrections(*hp["betas"], step, hp["bias_correction"])
    plan.lamb_moments(gdt, *hp["betas"], hp["eps"], hp["wd"], bc1, bc2s, norms, grad_scale=mult, found_inf=found_inf)
    plan.lamb(hp["lr"], hp["eps"], hp["wd"], bc1, bc2s, norms, lo, hi, found_inf=found_inf)


def ref_plan_step(rp, rg, rm, rv, adapt, hp, step, sums=None, mult=None, lo=0.0, hi=math.inf):
    """The restated step; sums=None: the restatement's own float32 sums.  Returns (p, m, v, u, sums)."""
    bc1, bc2s = bias_corrections(*hp["betas"], step, hp["bias_correction"])
    nm, nv, u = ref_moments(rp, rg, rm, rv, adapt, *hp["betas"], hp["eps"], hp["wd"], bc1, bc2s, mult)
    if sums is None:
        sums = ref_sums(rp, u)
    np_ = ref_update(rp, nm, nv, sums, adapt, hp["lr"], hp["eps"], hp["wd"], bc1, bc2s, lo, hi)
    return np_, nm, nv, u, sums


EXACT_HP = dict(lr=0.125, betas=(0.5, 0.75), eps=0.0, wd=0.5, bias_correction=True)


def run_exact_step(device, gdt, mult=None, sizes=SIZES, adapt=None):
    """Issue check 1: every intermediate is exact (u = ±1 + 0.5 p, u² in multiples of
    1/16, sums < 2^24/16), so Σp², Σu² equal the restatement's bit for bit whatever the
    order, and so do p, m, v.  A multiplier of 0.5 keeps everything on the grid."""
    p, g, m, v = make_tensors(device, gdt, True, seed=31, sizes=sizes)
    rp, rg, rm, rv = to_np(p), to_np(g), to_np(m), to_np(v)
    adapt = [True] * len(sizes) if adapt is None else adapt
    plan = make_plan(device, p, g, m, v, adapt, sizes)
    norms = new_norms(device, len(sizes))
    mt = None if mult is None else torch.tensor([mult], dtype=torch.float32, device=device)
    plan_step(plan, gdt, norms, EXACT_HP, 1, mt)
    wp, wm, wv, u, sums = ref_plan_step(rp, rg, rm, rv, adapt, EXACT_HP, 1, mult=mult)
    # the restatement's own float32 sums are exact: they equal the float64 ones
    want64 = np.zeros(2 * len(sizes))
    for t in range(len(sizes)):
        want64[2 * t] = np.sum(rp[t].astype(np.float64) ** 2)
        want64[2 * t + 1] = np.sum(u[t].astype(np.float64) ** 2)
    assert np.array_equal(sums.astype(np.float64), want64)
    got = norms.cpu().numpy()
    assert np.array_equal(got, sums), np.nonzero(got != sums)
    assert_lists_equal(to_np(m), wm, "m")
    assert_lists_equal(to_np(v), wv, "v")
    assert_lists_equal(to_np(p), wp, "p")
    plan.close()


def run_group_shapes(device, gdt):
    """The exact-sum step on SIZES2 (tests/_lars_common.py: group shapes of the segmented
    pass that SIZES never forms), alternating adapt flags (an unadapted tensor's u is ±1)."""
    run_exact_step(device, gdt, sizes=SIZES2, adapt=ADAPT2)


def run_shared_order(device, gdt):
    """LARS's and LAMB's per-tensor passes add Σp² in one order: on random inputs and the
    same p, gs_lars_norms and gs_lamb_moments (fresh plans) publish the same Σp² bits."""
    from tests import _lars_common as LC

    hp = dict(betas=(0.9, 0.999), eps=1e-6, wd=0.01)
    for sizes, adapt in ((SIZES, ADAPT), (SIZES2, ADAPT2)):
        p, g, m, v = make_tensors(device, gdt, False, seed=41, sizes=sizes)
        lars = LC.make_plan(device, p, g, None, 0.0, sizes, adapt)
        n_lars = new_norms(device, len(sizes))
        lars.lars_norms(gdt, n_lars)
        lamb = make_plan(device, p, g, m, v, adapt, sizes)
        n_lamb = new_norms(device, len(sizes))
        lamb.lamb_moments(gdt, *hp["betas"], hp["eps"], hp["wd"], 0.1, 0.03, n_lamb)
        a, b = n_lars.cpu().numpy()[0::2], n_lamb.cpu().numpy()[0::2]
        assert np.count_nonzero(a) >= len(sizes) // 2  # the passes ran
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), np.nonzero(a != b)
        lars.close()
        lamb.close()


def run_random_steps(device, gdt, wd, bias_correction, steps=3):
    """Issue check 2: three consecutive steps on random inputs, fresh grads per step.
    m', v' bit-exact; Σp², Σu² within numel * 2^-23 relative of float64 sums of the
    restated values; p bit-exact against the restatement fed the published sums.

    Ratio 1: the all-zero-p tensor at the first step (‖p‖ = 0; the step then moves it),
    and the all-zero-g tensor (m = v = 0, so u = wd*p) at every step when wd == 0
    (‖u‖ = 0) — with wd != 0 its u is the decay term and its ratio is 1/wd by the
    contract.  Both are checked explicitly as p - lr*u."""
    hp = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-6, wd=wd, bias_correction=bias_correction)
    p, g, m, v = make_tensors(device, gdt, False, seed=11)
    rp, rg, rm, rv = to_np(p), to_np(g), to_np(m), to_np(v)
    plan = make_plan(device, p, g, m, v)
    norms = new_norms(device)
    for s in range(steps):
        if s > 0:
            (g2,) = make_tensors(device, gdt, False, seed=11 + s, what="g")
            for dst, src in zip(g, g2):
                dst.copy_(src)
            rg = to_np(g)
        plan_step(plan, gdt, norms, hp, s + 1)
        got = norms.cpu().numpy()
        old_p = rp
        rp, rm, rv, u, _ = ref_plan_step(rp, rg, rm, rv, ADAPT, hp, s + 1, sums=got)
        assert_lists_equal(to_np(m), rm, f"step {s}: m")
        assert_lists_equal(to_np(v), rv, f"step {s}: v")
        assert_sums_close(got, old_p, u)
        assert_lists_equal(to_np(p), rp, f"step {s}: p")
        ones = ([I_ZERO_P] if s == 0 else []) + ([I_ZERO_G] if wd == 0 else [])
        for t in ones:
            assert ADAPT[t] and np.array_equal(to_np([p[t]])[0], old_p[t] - F(hp["lr"]) * u[t]), (s, t)
    plan.close()


def run_clamp(device):
    """Issue check 3: min_ratio / max_ratio inside the observed range of ratios: a
    clamped tensor moves by exactly lr*lo or lr*hi times u."""
    hp = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-6, wd=0.01, bias_correction=True)
    gdt = torch.float32
    p, g, m, v = make_tensors(device, gdt, False, seed=17)
    rp, rg, rm, rv = to_np(p), to_np(g), to_np(m), to_np(v)
    # the unclamped ratios, from the restatement's own sums (any order gives these to ~1e-5)
    _, _, _, u, sums = ref_plan_step(rp, rg, rm, rv, ADAPT, hp, 1)
    free = ref_ratios(sums, ADAPT)
    seen = sorted(float(free[t]) for t in range(len(SIZES))
                  if ADAPT[t] and sums[2 * t] > 0 and sums[2 * t + 1] > 0)
    lo, hi = seen[len(seen) // 4] * 1.001, seen[(3 * len(seen)) // 4] * 0.999
    assert seen[0] < lo < hi < seen[-1]
    plan = make_plan(device, p, g, m, v)
    norms = new_norms(device)
    plan_step(plan, gdt, norms, hp, 1, lo=lo, hi=hi)
    got = norms.cpu().numpy()
    want, _, _, u, _ = ref_plan_step(rp, rg, rm, rv, ADAPT, hp, 1, sums=got, lo=lo, hi=hi)
    newp = to_np(p)
    assert_lists_equal(newp, want, "p")
    unclamped = ref_ratios(got, ADAPT)
    n_lo = n_hi = 0
    for t in range(len(SIZES)):
        if not ADAPT[t] or not (got[2 * t] > 0 and got[2 * t + 1] > 0):
            continue
        if unclamped[t] < F(lo):
            n_lo += 1
            assert np.array_equal(newp[t], rp[t] - (F(hp["lr"]) * F(lo)) * u[t]), t
        elif unclamped[t] > F(hi):
            n_hi += 1
            assert np.array_equal(newp[t], rp[t] - (F(hp["lr"]) * F(hi)) * u[t]), t
    assert n_lo > 0 and n_hi > 0
    plan.close()


def run_found_inf(device, gdt=torch.float32):
    """Issue check 4: found_inf = 1: p, m, v unchanged bit for bit after both calls."""
    hp = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-6, wd=0.01, bias_correction=True)
    p, g, m, v = make_tensors(device, gdt, False, seed=5)
    before = [to_np(x) for x in (p, m, v)]
    plan = make_plan(device, p, g, m, v)
    plan_step(plan, gdt, new_norms(device), hp, 1, found_inf=torch.ones(1, dtype=torch.float32, device=device))
    for name, x, b in zip("pmv", (p, m, v), before):
        assert_lists_equal(to_np(x), b, f"found_inf: {name}")
    plan.close()


def run_determinism(device):
    """Issue check 5: two fresh plans on the same inputs publish identical norms, p, m, v."""
    hp = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-6, wd=0.01, bias_correction=True)
    outs = []
    for _ in range(2):
        p, g, m, v = make_tensors(device, torch.float32, False, seed=21)
        plan = make_plan(device, p, g, m, v)
        norms = new_norms(device)
        plan_step(plan, torch.float32, norms, hp, 1)
        outs.append([norms.cpu().numpy()] + to_np(p) + to_np(m) + to_np(v))
        plan.close()
    assert_lists_equal(outs[0], outs[1], "fresh plans")


# ---- FusedLAMB on the small model
LAMB_KW = dict(lr=0.02, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)


def _set_grads(params, grads):
    for p, gr in zip(params, grads):
        p.grad = gr.clone()


def _state(opt, params, key):
    return to_np([opt.state[p][key] for p in params])


def run_fused_lamb(device, max_grad_norm=None):
    """Issue check 6: three steps (lr changed before the third), bit-exact against the
    restatement fed sq_norms(); BatchNorm and bias tensors unadapted; torch Adam's state
    keys; a state_dict round trip continues bit-identically.  With max_grad_norm the
    restatement takes the multiplier read back from the optimizer's clip buffer."""
    import copy

    import distributed_training_amd as D

    model = small_model(device)
    params = list(model.parameters())
    adapt = [p.ndim > 1 for p in params]
    assert adapt == [True, False, False, False, True, False]
    opt = D.FusedLAMB(params, max_grad_norm=max_grad_norm, **LAMB_KW)
    rp = to_np(params)
    rm, rv = [np.zeros_like(x) for x in rp], [np.zeros_like(x) for x in rp]
    for s in range(3):
        if s == 2:
            opt.param_groups[0]["lr"] = 0.005
        grads = synthetic_grads(model, 100 + s)
        _set_grads(params, grads)
        opt.step()
        ((ps, norms),) = opt.sq_norms()
        assert [id(x) for x in ps] == [id(x) for x in params]
        mult = None
        if max_grad_norm is not None:
            buf = opt._clip_buf[params[0].device].cpu().numpy()  # [Σg², coef, norm, -]
            mult = buf[1]
            total = math.sqrt(sum(float(np.sum(x.astype(np.float64) ** 2)) for x in to_np(grads)))
            assert total > max_grad_norm and abs(float(mult) - max_grad_norm / (total + 1e-6)) <= 1e-5 * float(mult)
        hp = dict(lr=opt.param_groups[0]["lr"], betas=LAMB_KW["betas"], eps=LAMB_KW["eps"],
                  wd=LAMB_KW["weight_decay"], bias_correction=True)
        sums = norms.cpu().numpy()
        old_p = rp
        rp, rm, rv, u, _ = ref_plan_step(rp, to_np(grads), rm, rv, adapt, hp, s + 1, sums=sums, mult=mult)
        assert_sums_close(sums, old_p, u)
        assert_lists_equal(to_np(params), rp, f"step {s}: p")
        assert_lists_equal(_state(opt, params, "exp_avg"), rm, f"step {s}: exp_avg")
        assert_lists_equal(_state(opt, params, "exp_avg_sq"), rv, f"step {s}: exp_avg_sq")
    sd = opt.state_dict()
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 3.0
               for st in sd["state"].values()) and len(sd["state"]) == len(params)
    model2 = copy.deepcopy(model)
    opt2 = D.FusedLAMB(model2.parameters(), max_grad_norm=max_grad_norm, **LAMB_KW)
    opt2.load_state_dict(copy.deepcopy(sd))
    assert opt2.param_groups[0]["lr"] == 0.005
    grads = synthetic_grads(model, 200)
    for m_, o_ in ((model, opt), (model2, opt2)):
        _set_grads(m_.parameters(), grads)
        o_.step()
    p2 = list(model2.parameters())
    assert_lists_equal(to_np(p2), to_np(params), "round trip: p")
    for key in ("exp_avg", "exp_avg_sq"):
        assert_lists_equal(_state(opt2, p2, key), _state(opt, params, key), f"round trip: {key}")
