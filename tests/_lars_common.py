"""Shared by tests/test_lars_cpu.py and tests/test_gpu_lars.py: a numpy float32
restatement of the LARS contract (include/gsync.h, gs_lars_step), written from
the contract alone — it never calls the library — and the one tensor list both
modules run, on CPU tensors (host backend) or on the GPU.

The restatement has two forms: :func:`ref_step` given the per-tensor sums, and
:func:`ref_sums` computing them.  Every numpy operation below works on float32
operands and rounds once, which is the contract's "no fma" arithmetic op for op.
"""
import numpy as np
import torch

F = np.float32

# ~1e5 elements: a full-group tensor, one whose tail shares a chunk with the next,
# tiny and empty ones, BatchNorm-like runs, a mixed chunk of more than 64 tensors,
# one tensor at a 1-element offset in its storage (not 16-B aligned; large enough
# to own full chunks), an all-zero p and an all-zero g (ratio 1)
SIZES = [16384 + 4096, 70001, 1024, 5, 3, 1, 0, 64, 64, 65] + [3] * 80 + [2500, 300, 300]
I_OFFSET, I_ZERO_P, I_ZERO_G = len(SIZES) - 3, len(SIZES) - 2, len(SIZES) - 1
ADAPT = [i % 2 == 0 for i in range(len(SIZES))]
ADAPT[I_ZERO_P] = ADAPT[I_ZERO_G] = True  # the ratio-1 rule is only reached on adapted tensors

# Group shapes of the segmented pass (4 chunks of 1 Ki elements per group) that SIZES never
# forms: there the only tensor of >= 4 Ki elements behind another one starts on a group
# boundary, so a group of 4 full chunks is always one tensor's.  By build_chunk_map
# (gs_plan.cpp: tensors >= 4 Ki start on a multiple of 4 Ki, >= 1 Ki on a multiple of 1 Ki)
# these start at 0, 2048, 4096, 7168, 8192, 12288, 16384:
#   group 0  chunks 0-3    full, tensors 0 and 1
#   group 1  chunks 4-7    full, tensors 2 and 3
#   group 2  chunks 8-11   one full chunk (tensor 4), then three empty ones (the 4 Ki tensor's alignment gap)
#   group 3  chunks 12-15  full (tensor 5): the fast path right before ...
#   group 4  chunks 16-17  ... a short last group: one full chunk and tensor 6's 476-element tail
SIZES2 = [2048, 2048, 3072, 1024, 1024, 4096, 1500]
ADAPT2 = [i % 2 == 0 for i in range(len(SIZES2))]


def _draw(n, exact, gen):
    if exact:  # multiples of 0.5 in [-2, 2]: every square and every partial sum is exact in fp32
        return torch.randint(-4, 5, (n,), generator=gen).float() * 0.5
    return torch.randn(n, generator=gen)


def make_tensors(device, gdt, exact, seed, what="pgb", sizes=SIZES):
    """Lists p, g (dtype gdt), b of the tensor list, drawn on the CPU from `seed` (the
    zero tensors and the offset one are SIZES' alone)."""
    gen = torch.Generator().manual_seed(seed)
    out = {k: [] for k in what}
    special = sizes is SIZES
    for i, n in enumerate(sizes):
        for k in what:
            x = _draw(n, exact, gen)
            if special and ((k == "p" and i == I_ZERO_P) or (k == "g" and i == I_ZERO_G)):
                x = torch.zeros(n)
            x = x.to(gdt if k == "g" else torch.float32)
            if special and i == I_OFFSET:
                store = torch.zeros(n + 1, dtype=x.dtype, device=device)
                store[1:].copy_(x)
                x = store[1:]
                assert x.data_ptr() % 16 != 0
            else:
                x = x.to(device)
            out[k].append(x)
    return [out[k] for k in what]


def to_np(ts):
    return [t.detach().float().cpu().numpy().reshape(-1).copy() for t in ts]


def ref_sums(p, g):
    """[2t] = Σp², [2t+1] = Σg² in float32 (exact, hence order-free, on the exact-sum inputs)."""
    out = np.zeros(2 * len(p), dtype=F)
    for t, (x, y) in enumerate(zip(p, g)):
        out[2 * t] = np.sum(x * x, dtype=F)
        out[2 * t + 1] = np.sum(y * y, dtype=F)
    return out


def sums_f64(p, g):
    out = np.zeros(2 * len(p), dtype=np.float64)
    for t, (x, y) in enumerate(zip(p, g)):
        out[2 * t] = np.sum(x.astype(np.float64) ** 2)
        out[2 * t + 1] = np.sum(y.astype(np.float64) ** 2)
    return out


def ref_step(p, g, b, sums, adapt, lr, mom, wd, eta, eps, m=None):
    """One step on numpy float32 lists given the per-tensor sums; returns new (p, b)."""
    lr, mom, wd, eta, eps = F(lr), F(mom), F(wd), F(eta), F(eps)
    new_p, new_b = [], []
    for t in range(len(p)):
        ratio, wd_t = F(1), F(0)
        if adapt[t]:
            wd_t = wd
            wn, gn = np.sqrt(F(sums[2 * t])), np.sqrt(F(sums[2 * t + 1]))
            if m is not None:
                gn = gn * F(m)
            if wn > 0 and gn > 0:
                ratio = (eta * wn) / ((gn + wd * wn) + eps)
        slr = lr * ratio
        assert slr.dtype == F
        gt = g[t]
        if m is not None:
            gt = gt * F(m)
        if wd_t != 0:
            gt = gt + wd_t * p[t]
        if mom != 0:
            bt = b[t] * mom + gt
            d = bt
        else:
            bt = b[t]
            d = gt
        pt = p[t] - slr * d
        assert pt.dtype == F and bt.dtype == F
        new_p.append(pt)
        new_b.append(bt)
    return new_p, new_b


def assert_lists_equal(got, want, what):
    for t, (a, r) in enumerate(zip(got, want)):
        assert np.array_equal(a, r, equal_nan=True), f"{what}: tensor {t} ({a.size} elements) differs"


def assert_sums_close(got, p, g, cols=(0, 1)):
    """Per-tensor sums against float64: relative error <= numel * 2^-23 — the worst case
    for n rounded squares added in any order, doubled; it holds for any implementation."""
    want = sums_f64(p, g)
    for t in range(len(p)):
        for c in cols:
            tol = p[t].size * 2.0 ** -23 * want[2 * t + c]
            assert abs(float(got[2 * t + c]) - want[2 * t + c]) <= tol, (t, c, got[2 * t + c], want[2 * t + c])


HYPER = dict(lr=0.1, eta=1e-3, eps=1e-8)


def make_plan(device, p, g, b, mom, sizes=SIZES, adapt=ADAPT):
    from distributed_training_amd.multi_tensor import TensorListPlan

    plan = TensorListPlan(sizes, device)
    plan.set_ptrs(0, p)
    plan.set_ptrs(1, g)
    if mom != 0:
        plan.set_ptrs(2, b)
    plan.set_adapt(adapt)
    return plan


def plan_step(plan, gdt, norms, mom, wd, mult=None, found_inf=None, lr=None):
    plan.lars_norms(gdt, norms)
    plan.lars(gdt, HYPER["lr"] if lr is None else lr, mom, wd, HYPER["eta"], HYPER["eps"], norms,
              grad_scale=mult, found_inf=found_inf)


def run_plan_steps(device, gdt, mom, wd, mult, exact, steps=3, sizes=SIZES, adapt=ADAPT):
    """`steps` consecutive steps at plan level, each checked against the restatement.

    Exact-sum inputs: the grads of every step are fresh exact-sum draws, so Σg² is
    bit-exact at every step; p is on the grid only before the first step (an update
    leaves it), so Σp² is bit-exact at step 0 and held to the float64 bound after;
    p and buf are bit-exact at every step — at step 0 against the restatement that
    computes its own sums (the whole step), later against it fed its own Σg² and
    the published Σp².  Random inputs: sums to the float64 bound, p and buf
    bit-exact against the restatement fed the published sums."""
    p, g, b = make_tensors(device, gdt, exact, seed=11, sizes=sizes)
    rp, rg, rb = to_np(p), to_np(g), to_np(b)
    plan = make_plan(device, p, g, b, mom, sizes, adapt)
    norms = torch.zeros(2 * len(sizes), dtype=torch.float32, device=device)
    mt = None if mult is None else torch.tensor([mult], dtype=torch.float32, device=device)
    for s in range(steps):
        if s > 0:
            (g2,) = make_tensors(device, gdt, exact, seed=11 + s, what="g", sizes=sizes)
            for dst, src in zip(g, g2):
                dst.copy_(src)
            rg = to_np(g)
        plan_step(plan, gdt, norms, mom, wd, mt)
        got = norms.cpu().numpy()
        if exact:
            own = ref_sums(rp, rg)
            assert np.array_equal(got[1::2], own[1::2]), f"step {s}: Σg²"
            if s == 0:
                assert np.array_equal(got[0::2], own[0::2]), f"step {s}: Σp²"
                sums = own
            else:
                assert_sums_close(got, rp, rg, cols=(0,))
                sums = own.copy()
                sums[0::2] = got[0::2]
        else:
            assert_sums_close(got, rp, rg)
            sums = got
        rp, rb = ref_step(rp, rg, rb, sums, adapt, HYPER["lr"], mom, wd, HYPER["eta"], HYPER["eps"], mult)
        assert_lists_equal(to_np(p), rp, f"step {s}: p")
        assert_lists_equal(to_np(b), rb, f"step {s}: buf")
    plan.close()


def run_group_shapes(device, gdt):
    """One exact-sum step on SIZES2 (the group shapes above), alternating adapt flags:
    Σp², Σg², p and buf bit for bit against the restatement."""
    run_plan_steps(device, gdt, 0.9, 1e-4, None, True, steps=1, sizes=SIZES2, adapt=ADAPT2)


def run_found_inf(device, gdt=torch.float32):
    p, g, b = make_tensors(device, gdt, False, seed=5)
    p0, b0 = to_np(p), to_np(b)
    plan = make_plan(device, p, g, b, 0.9)
    norms = torch.zeros(2 * len(SIZES), dtype=torch.float32, device=device)
    plan_step(plan, gdt, norms, 0.9, 1e-4, found_inf=torch.ones(1, dtype=torch.float32, device=device))
    assert_lists_equal(to_np(p), p0, "found_inf: p")
    assert_lists_equal(to_np(b), b0, "found_inf: buf")
    plan.close()


# ---- the small model of the FusedLARS tests
def small_model(device, seed=0):
    import torch.nn as nn

    torch.manual_seed(seed)
    return nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8), nn.Flatten(), nn.Linear(8 * 6 * 6, 10)).to(device)


def synthetic_grads(model, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(p.shape, generator=gen).to(p.device) for p in model.parameters()]


def run_fused_lars(device):
    """FusedLARS on the small model: three steps (lr changed before the third),
    bit-exact against the restatement fed sq_norms(); BatchNorm and bias tensors
    unadapted and undecayed; a state_dict round trip continues bit-identically."""
    import copy

    import distributed_training_amd as D

    kw = dict(lr=0.2, momentum=0.9, weight_decay=1e-4, trust_coefficient=1e-3, eps=1e-8)
    model = small_model(device)
    params = list(model.parameters())
    adapt = [p.ndim > 1 for p in params]
    assert adapt == [True, False, False, False, True, False]
    opt = D.FusedLARS(params, **kw)
    rp = to_np(params)
    rb = [np.zeros_like(x) for x in rp]
    for s in range(3):
        if s == 2:
            opt.param_groups[0]["lr"] = 0.05
        grads = synthetic_grads(model, 100 + s)
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        opt.step()
        ((ps, norms),) = opt.sq_norms()
        assert [id(x) for x in ps] == [id(x) for x in params]
        sums = norms.cpu().numpy()
        assert_sums_close(sums, rp, to_np(grads))
        rp, rb = ref_step(rp, to_np(grads), rb, sums, adapt, opt.param_groups[0]["lr"], kw["momentum"],
                          kw["weight_decay"], kw["trust_coefficient"], kw["eps"])
        assert_lists_equal(to_np(params), rp, f"step {s}: p")
        assert_lists_equal(to_np([opt.state[p]["momentum_buffer"] for p in params]), rb, f"step {s}: buf")
    # unadapted tensors took plain momentum SGD without weight decay: restate the last step that way
    # (covered by ref_step's adapt=False branch above; here the state_dict round trip)
    model2 = copy.deepcopy(model)
    opt2 = D.FusedLARS(model2.parameters(), **kw)
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert opt2.param_groups[0]["lr"] == 0.05
    grads = synthetic_grads(model, 200)
    for m_, o_ in ((model, opt), (model2, opt2)):
        for p, gr in zip(m_.parameters(), grads):
            p.grad = gr.clone()
        o_.step()
    assert_lists_equal(to_np(model2.parameters()), to_np(model.parameters()), "round trip: p")
    assert_lists_equal(to_np([opt2.state[p]["momentum_buffer"] for p in model2.parameters()]),
                       to_np([opt.state[p]["momentum_buffer"] for p in model.parameters()]), "round trip: buf")
