"""Shared by tests/test_zero_lamb_cpu.py and tests/test_gpu_zero_lamb.py: the update
kernels with the low-precision copy (gs_lars_step_lowp / gs_lamb_step_lowp), and the
sharded LAMB / LARS step of ZeroDataParallel (optimizer="lamb" | "lars") against the
numpy float32 restatements of tests/_lamb_common.py and tests/_lars_common.py, which are
imported unchanged and never call the library.

The sharded harness follows tests/test_zero_ds_step.py::ds_step_vs_oracle: synthetic
per-rank grads through the real hooks (the loss is Σ_i <p_i, r_i>), the averaged grads
re-assembled from every rank's ``grad_shards``; the restatement is then fed exactly what
the engine published — those grads, the clip multiplier and the all-reduced per-tensor
sums — and has to reproduce the consolidated fp32 master bit for bit.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.distributed as dist

from tests import _lamb_common as CL
from tests import _lars_common as CR
from tests._lars_common import SIZES, F, assert_lists_equal, to_np

# ------------------------------------------------------------------ 1. the update kernels with the copy
SENTINEL = 7.25  # exact in bf16 and fp16


PLACEMENTS = ("aligned", "offset")


def _copy_slots(device, dtype, placement, fill=SENTINEL):
    """One sentinel-filled copy tensor per SIZES entry.

    "aligned": every copy starts its own allocation (16-byte aligned), except the I_OFFSET
    tensor's, which sits one element into its storage like that tensor's other streams (2-byte
    aligned): the 20480- and 70001-element tensors pass fast_ok and take the full-chunk path
    with the copy store.  "offset": every copy one element into its storage, so every tensor
    takes the checked path with a 2-byte-aligned copy pointer."""
    assert placement in PLACEMENTS
    out = []
    for i, n in enumerate(SIZES):
        if placement == "offset" or i == CR.I_OFFSET:
            x = torch.full((n + 1,), fill, dtype=dtype, device=device)[1:]
            assert n == 0 or x.data_ptr() % 4 == 2
        else:
            x = torch.full((n,), fill, dtype=dtype, device=device)
            assert n == 0 or x.data_ptr() % 16 == 0
        out.append(x)
    return out


def _bits(ts):
    return [t.detach().cpu().contiguous().view(torch.int16).numpy().copy() for t in ts]


def _lamb_hp(step=1):
    hp = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-6, wd=0.01, bias_correction=True)
    return hp, CL.bias_corrections(*hp["betas"], step, True)


def run_lamb_lowp(device, ldt, placement):
    """gs_lamb_step_lowp: fp32 p bit-identical to gs_lamb_step on equal inputs, the copy ==
    p_new.to(ldt) bit for bit (2-byte-aligned copy pointers), found_inf leaves a sentinel-filled
    copy alone, and lowp_dtype = -1 through the new entry point equals the old entry point."""
    from distributed_training_amd import _lib as L

    hp, (bc1, bc2s) = _lamb_hp()
    outs = {}
    for mode in ("old", "copy", "none"):
        p, g, m, v = CL.make_tensors(device, torch.float32, False, seed=11)
        plan = CL.make_plan(device, p, g, m, v)
        norms = CL.new_norms(device)
        plan.lamb_moments(torch.float32, *hp["betas"], hp["eps"], hp["wd"], bc1, bc2s, norms)
        lp = None
        if mode == "old":
            plan.lamb(hp["lr"], hp["eps"], hp["wd"], bc1, bc2s, norms)
        elif mode == "copy":
            lp = _copy_slots(device, ldt, placement)
            plan.set_ptrs(4, lp)
            plan.lamb(hp["lr"], hp["eps"], hp["wd"], bc1, bc2s, norms, lowp_dtype=ldt)
        else:  # the new entry point without a copy
            L.check(L.lib().gs_lamb_step_lowp(plan.handle, -1, hp["lr"], hp["eps"], hp["wd"], bc1, bc2s, 0.0,
                                              math.inf, norms.data_ptr(), None, plan._stream(None)),
                    "gs_lamb_step_lowp")
        outs[mode] = (to_np(p), to_np(m), to_np(v), p, lp)
        plan.close()
    for mode in ("copy", "none"):
        for k, name in enumerate("pmv"):
            assert_lists_equal(outs[mode][k], outs["old"][k], f"lamb {mode}: {name}")
    _, _, _, p, lp = outs["copy"]
    assert_lists_equal(_bits(lp), _bits([x.to(ldt) for x in p]), "lamb: copy == p_new.to(dtype)")
    # found_inf = 1: nothing is written, the copy included
    p, g, m, v = CL.make_tensors(device, torch.float32, False, seed=11)
    before = to_np(p)
    plan = CL.make_plan(device, p, g, m, v)
    lp = _copy_slots(device, ldt, placement)
    plan.set_ptrs(4, lp)
    norms = CL.new_norms(device)
    plan.lamb_moments(torch.float32, *hp["betas"], hp["eps"], hp["wd"], bc1, bc2s, norms)
    plan.lamb(hp["lr"], hp["eps"], hp["wd"], bc1, bc2s, norms, lowp_dtype=ldt,
              found_inf=torch.ones(1, dtype=torch.float32, device=device))
    assert_lists_equal(to_np(p), before, "lamb found_inf: p")
    assert_lists_equal(_bits(lp), _bits(_copy_slots("cpu", ldt, placement)), "lamb found_inf: copy")
    plan.close()


def run_lars_lowp(device, ldt, mom, placement):
    """The same four checks for gs_lars_step_lowp (copy in slot 3)."""
    from distributed_training_amd import _lib as L

    wd = 1e-4
    outs = {}
    for mode in ("old", "copy", "none"):
        p, g, b = CR.make_tensors(device, torch.float32, False, seed=11)
        plan = CR.make_plan(device, p, g, b, mom)
        norms = torch.zeros(2 * len(SIZES), dtype=torch.float32, device=device)
        plan.lars_norms(torch.float32, norms)
        lp = None
        if mode == "old":
            plan.lars(torch.float32, CR.HYPER["lr"], mom, wd, CR.HYPER["eta"], CR.HYPER["eps"], norms)
        elif mode == "copy":
            lp = _copy_slots(device, ldt, placement)
            plan.set_ptrs(3, lp)
            plan.lars(torch.float32, CR.HYPER["lr"], mom, wd, CR.HYPER["eta"], CR.HYPER["eps"], norms, lowp_dtype=ldt)
        else:
            L.check(L.lib().gs_lars_step_lowp(plan.handle, L.gs_dtype(torch.float32), -1, CR.HYPER["lr"], mom, wd,
                                              CR.HYPER["eta"], CR.HYPER["eps"], norms.data_ptr(), None, None,
                                              plan._stream(None)), "gs_lars_step_lowp")
        outs[mode] = (to_np(p), to_np(b), p, lp)
        plan.close()
    for mode in ("copy", "none"):
        assert_lists_equal(outs[mode][0], outs["old"][0], f"lars {mode}: p")
        assert_lists_equal(outs[mode][1], outs["old"][1], f"lars {mode}: buf")
    _, _, p, lp = outs["copy"]
    assert_lists_equal(_bits(lp), _bits([x.to(ldt) for x in p]), "lars: copy == p_new.to(dtype)")
    p, g, b = CR.make_tensors(device, torch.float32, False, seed=11)
    before = to_np(p)
    plan = CR.make_plan(device, p, g, b, mom)
    lp = _copy_slots(device, ldt, placement)
    plan.set_ptrs(3, lp)
    norms = torch.zeros(2 * len(SIZES), dtype=torch.float32, device=device)
    plan.lars_norms(torch.float32, norms)
    plan.lars(torch.float32, CR.HYPER["lr"], mom, wd, CR.HYPER["eta"], CR.HYPER["eps"], norms, lowp_dtype=ldt,
              found_inf=torch.ones(1, dtype=torch.float32, device=device))
    assert_lists_equal(to_np(p), before, "lars found_inf: p")
    assert_lists_equal(_bits(lp), _bits(_copy_slots("cpu", ldt, placement)), "lars found_inf: copy")
    plan.close()


# ------------------------------------------------------------------ 2./3. the sharded step
# >= 3 buckets of the micro ResNet (78 042 parameters); at ws 2 and 3 this size gives tensors
# with pieces on two ranks and (rank, tensor) pairs of zero elements (assert_piece_preconditions;
# checked on the CPU at both world sizes by test_zero_lamb_cpu.py::test_bucket_size_gives_the_piece_cases).
#
# A piece that starts off a 4-element boundary cannot come out of ZeroDataParallel: the bucketer
# places every parameter on a multiple of BUCKET_ALIGN_ELEMS = 64 elements and pads every bucket to
# world * 64, so both ends of every piece are multiples of 64 elements whatever the bucket size.
# assert_piece_preconditions asserts that instead, and run_unaligned_pieces below runs the same
# two passes + the sum of the per-tensor vectors on a hand-made sharding whose pieces start at
# odd element offsets (the engine's unaligned path), against the same restatement.
BUCKET = 30000
CLIP = 1.0
TARGET_NORMS = (4.0, 0.5, 2.0)  # ‖avg g‖ per step: clip on, off, on
CLAMP = (0.05, 0.3)  # a finite trust-ratio clamp (DeepSpeed's min_coeff / max_coeff), for the clamp case
LAMB = dict(lr=0.02, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)
LARS = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, trust_coefficient=1e-3, eps=1e-8)


def model_of(kind):
    from distributed_training_amd.resnet import MODELS, BasicBlock, ResNet

    torch.manual_seed(0)
    if kind == "micro":
        return ResNet(BasicBlock, [1, 1, 1, 1], num_classes=10, width=8)
    return MODELS[kind](num_classes=1000)


def piece_cases(z):
    """(tensors with pieces on >= 2 ranks, (rank, tensor) pairs of zero elements, pieces that
    start off a 4-element boundary of their shard) of engine z's layout, from shard_pieces."""
    per_rank = [z.shard_pieces(r) for r in range(z.world)]
    n = len(z.params)
    for i, p in enumerate(z.params):  # the pieces of a tensor tile it
        assert sum(per_rank[r][i][2] for r in range(z.world)) == p.numel()
    split = sum(1 for i in range(n) if sum(1 for r in range(z.world) if per_rank[r][i][2] > 0) >= 2)
    empty = sum(1 for r in range(z.world) for i in range(n) if per_rank[r][i][2] == 0)
    odd = sum(1 for r in range(z.world) for i in range(n) if per_rank[r][i][2] > 0 and per_rank[r][i][1] % 4)
    return split, empty, odd


def assert_piece_preconditions(z):
    split, empty, odd = piece_cases(z)
    assert len(z.buckets) >= 3, len(z.buckets)
    if z.world >= 2:
        assert split >= 1, "no tensor has pieces on two ranks"
        assert empty >= 1, "no (rank, tensor) pair of zero elements"
    from distributed_training_amd.ddp import BUCKET_ALIGN_ELEMS

    assert odd == 0  # the layout's alignment (see BUCKET above); run_unaligned_pieces covers the other case
    for r in range(z.world):
        assert all(off % BUCKET_ALIGN_ELEMS == 0 for _, off, n in z.shard_pieces(r) if n)


def _assert_sums(got, ws, cols, what):
    """Each sum within (numel + ws) * 2^-23 relative of the float64 sum of the restated values:
    assert_sums_close's bound for numel rounded squares added in any order, plus the ws - 1
    adds of the all-reduce."""
    for t, xs in enumerate(zip(*cols)):
        for c, x in enumerate(xs):
            want = float(np.sum(x.astype(np.float64) ** 2))
            tol = (x.size + ws) * 2.0 ** -23 * want
            assert abs(float(got[2 * t + c]) - want) <= tol, (what, t, c, got[2 * t + c], want)


def _same_on_all_ranks(x: np.ndarray, ws, what):
    allx = [None] * ws
    dist.all_gather_object(allx, x)
    for other in allx[1:]:
        assert np.array_equal(allx[0], other, equal_nan=True), f"{what} differs between ranks"


def engine_avg_grads(z, ws):
    """The engine's averaged grads per parameter (fp32 numpy): every rank's shard, re-assembled."""
    mine = [s.detach().float().cpu().numpy() for s in z.grad_shards]
    all_shards = [None] * ws
    dist.all_gather_object(all_shards, mine)
    out = []
    for i, p in enumerate(z.params):
        b, off = z.loc[i]
        flat = np.concatenate([all_shards[r][b] for r in range(ws)])
        out.append(flat[off:off + p.numel()].copy())
    return out


def backward_synthetic(z, params, rs, scale=1.0):
    z.prepare_backward()
    z.wait_allgather()  # the loss reads the parameters outside a module forward
    loss = sum((p.float() * r).sum() for p, r in zip(params, rs))
    (loss * scale).backward()


def draw_rs(params, gen, norm, ws, dev):
    n_total = sum(p.numel() for p in params)
    sigma = norm * math.sqrt(ws / n_total)
    return [torch.randn(p.shape, device=dev, generator=gen) * sigma for p in params]


class Restated:
    """The float32 restatement's state for one engine: p (the fp32 master), and m, v (lamb)
    or the momentum buffer (lars)."""

    def __init__(self, kind, params, adapt):
        self.kind, self.adapt = kind, list(adapt)
        self.p = to_np(params)
        self.s1 = [np.zeros_like(x) for x in self.p]
        self.s2 = [np.zeros_like(x) for x in self.p]

    def step(self, grads, sums, mult, t, ws, lr=None, lo=0.0, hi=math.inf):
        """One restated step fed the published sums and multiplier; checks the sums against
        float64 and the unadapted tensors against plain Adam / momentum SGD without decay."""
        old = self.p
        mf = None if mult is None else F(mult)
        if self.kind == "lamb":
            hp = dict(lr=LAMB["lr"] if lr is None else lr, betas=LAMB["betas"], eps=LAMB["eps"],
                      wd=LAMB["weight_decay"], bias_correction=True)
            self.p, self.s1, self.s2, u, _ = CL.ref_plan_step(old, grads, self.s1, self.s2, self.adapt, hp, t,
                                                              sums=sums, mult=mf, lo=lo, hi=hi)
            _assert_sums(sums, ws, (old, u), f"step {t}")
            bc1, bc2s = (F(x) for x in CL.bias_corrections(*hp["betas"], t, True))
            for i, ad in enumerate(self.adapt):
                if not ad:  # plain Adam, no decay, ratio 1
                    adam = (self.s1[i] / bc1) / (np.sqrt(self.s2[i]) / bc2s + F(hp["eps"]))
                    assert np.array_equal(self.p[i], old[i] - F(hp["lr"]) * adam), f"step {t}: unadapted tensor {i}"
        else:
            hp = dict(LARS, lr=LARS["lr"] if lr is None else lr)
            old_b = self.s1
            self.p, self.s1 = CR.ref_step(old, grads, old_b, sums, self.adapt, hp["lr"], hp["momentum"],
                                          hp["weight_decay"], hp["trust_coefficient"], hp["eps"], mf)
            _assert_sums(sums, ws, (old, grads), f"step {t}")
            for i, ad in enumerate(self.adapt):
                if not ad:  # momentum SGD, no decay, ratio 1
                    g = grads[i] if mf is None else grads[i] * mf
                    assert np.array_equal(self.p[i], old[i] - F(hp["lr"]) * (old_b[i] * F(hp["momentum"]) + g)), \
                        f"step {t}: unadapted tensor {i}"


def make_engine(model, kind, stage, **kw):
    from distributed_training_amd.zero import ZeroDataParallel

    hp = LAMB if kind == "lamb" else LARS
    kw.setdefault("reduce_bucket_size", BUCKET)
    kw.setdefault("gradient_clipping", CLIP)
    return ZeroDataParallel(model, stage=stage, optimizer=kind, **hp, **kw)


def check_engine_vs_restated(z, params, names, ref, dtype, ws, t):
    """Consolidated master == the restatement bit for bit; 16-bit parameters == master.to(dtype);
    parameters identical on every rank."""
    full = z.consolidated_state_dict()
    masters = [full[n].float().numpy().reshape(-1) for n in names]
    assert_lists_equal(masters, ref.p, f"step {t}: master vs the restatement")
    if dtype != torch.float32:
        for n, p in zip(names, params):
            assert torch.equal(p.detach().cpu(), full[n].to(dtype).reshape(p.shape)), f"step {t} {n}: model copy"
    w = torch.cat([p.detach().float().reshape(-1).cpu() for p in params]).numpy()
    _same_on_all_ranks(w, ws, f"step {t}: parameters")


def sharded_step_vs_restatement(rank, ws, dev, kind="lamb", stage=2, dtype=torch.float32, model="micro", steps=3,
                                bucket=BUCKET, clamp=None):
    """clamp = (min_trust, max_trust) (lamb): handed to the engine and to the restatement; the
    run then also asserts that at every step some adapted tensor's free ratio lies outside the
    clamp, so an update that ignored it would miss the bit-for-bit master check."""
    model = model_of(model).to(dev).to(dtype)
    params = list(model.parameters())
    names = [n for n, _ in model.named_parameters()]
    lo, hi = (0.0, math.inf) if clamp is None else clamp
    kw = {} if clamp is None else dict(min_trust=lo, max_trust=hi)
    z = make_engine(model, kind, stage, reduce_bucket_size=bucket, **kw)
    assert z.kind == kind and z.piece_plan is not None
    assert_piece_preconditions(z)
    adapt = [p.ndim > 1 for p in params]
    assert z.adapt == adapt and not all(adapt) and any(adapt)
    ref = Restated(kind, params, adapt)
    gen = torch.Generator(device=dev).manual_seed(100 + rank)
    for it in range(steps):
        t = it + 1
        target = TARGET_NORMS[it % len(TARGET_NORMS)]
        backward_synthetic(z, params, draw_rs(params, gen, target, ws, dev))
        assert z.step() is True
        z.wait_allgather()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        grads = engine_avg_grads(z, ws)
        # the published clip multiplier: min(1, clip / (‖g‖ + 1e-6)), on exactly when it should be
        mult = float(z._scratch[5])
        gn = math.sqrt(sum(float(np.sum(x.astype(np.float64) ** 2)) for x in grads))
        want = min(1.0, CLIP / (gn + 1e-6))
        assert abs(mult - want) <= 1e-5 * want, (t, mult, want)
        assert (mult < 1.0) == (target > CLIP), (t, mult, gn)
        ps, norms = z.sq_norms()
        assert [id(x) for x in ps] == [id(x) for x in params]
        sums = norms.cpu().numpy().copy()
        _same_on_all_ranks(np.concatenate([sums, np.float32([mult])]), ws, f"step {t}: sq_norms / multiplier")
        if clamp is not None:
            free = [float(r) for r, ad in zip(CL.ref_ratios(sums, adapt), adapt) if ad]
            assert any(r < lo or r > hi for r in free), (t, min(free), max(free))
        ref.step(grads, sums, mult, t, ws, lo=lo, hi=hi)
        check_engine_vs_restated(z, params, names, ref, dtype, ws, t)
    z.close()


# ------------------------------------------------------------------ 4. fp16 overflow
def overflow_skips_the_step(rank, ws, dev, kind="lamb"):
    """A non-finite grad on one rank: master, states and parameters bitwise unchanged on every
    rank, step_count unchanged, the scale halved per its hysteresis (2: the first overflow
    spends the hysteresis, the second halves); the next clean step is the restatement's step 1."""
    from distributed_training_amd.zero import DynamicLossScaler

    dtype = torch.float16
    model = model_of("micro").to(dev).to(dtype)
    params = list(model.parameters())
    names = [n for n, _ in model.named_parameters()]
    scaler = DynamicLossScaler(init_scale=2.0 ** 8, hysteresis=2)
    z = make_engine(model, kind, 2, loss_scaler=scaler)
    ref = Restated(kind, params, [p.ndim > 1 for p in params])
    gen = torch.Generator(device=dev).manual_seed(300 + rank)

    def snapshot():
        return [x.detach().cpu().clone() for x in list(z.master) + list(z.state1) + list(z.state2) + params]

    before = snapshot()
    for n_over, want_scale in ((1, 2.0 ** 8), (2, 2.0 ** 7)):
        rs = draw_rs(params, gen, 0.5, ws, dev)
        if rank == ws - 1:
            rs[3].view(-1)[0] = float("inf")
        backward_synthetic(z, params, rs, scale=scaler.scale)
        assert z.step() is False
        z.wait_allgather()
        for a, b in zip(snapshot(), before):
            assert torch.equal(a, b), "an overflow step wrote something"
        assert z.step_count == 0 and scaler.scale == want_scale, (n_over, z.step_count, scaler.scale)
    scale = scaler.scale
    backward_synthetic(z, params, draw_rs(params, gen, 2.0, ws, dev), scale=scale)
    assert z.step() is True and z.step_count == 1
    z.wait_allgather()
    grads = engine_avg_grads(z, ws)  # scaled by `scale`
    mult = float(z._scratch[5])      # clip coefficient * (1 / scale)
    assert 0 < mult < 1.0 / scale
    sums = z.sq_norms()[1].cpu().numpy().copy()
    _same_on_all_ranks(np.concatenate([sums, np.float32([mult])]), ws, "sq_norms / multiplier")
    ref.step(grads, sums, mult, 1, ws)
    check_engine_vs_restated(z, params, names, ref, dtype, ws, 1)
    z.close()


# ------------------------------------------------------------------ 6. checkpoints
def checkpoint_round_trips(rank, ws, dev, kind="lamb", dtype=torch.bfloat16):
    """A shard state_dict into a fresh engine continues bit-identically for one more step;
    consolidated_state_dict -> load_consolidated_state_dict preserves the masters."""
    import copy

    def fresh():
        m = model_of("micro").to(dev).to(dtype)
        return m, list(m.parameters()), make_engine(m, kind, 2)

    def snap(z):
        return [x.detach().cpu().clone() for x in list(z.master) + list(z.state1) + list(z.state2) + list(z.params)]

    _, pa, za = fresh()
    gen = torch.Generator(device=dev).manual_seed(400 + rank)
    for it in range(2):
        backward_synthetic(za, pa, draw_rs(pa, gen, TARGET_NORMS[it], ws, dev))
        za.step()
    sd = copy.deepcopy(za.state_dict())
    assert sd["kind"] == kind and sd["step"] == 2
    assert set(sd) == {"step", "rank", "world", "stage", "bucket_numel", "kind", "master", "exp_avg", "exp_avg_sq",
                       "param_groups", "loss_scaler"}
    if kind == "lars":  # no second state in memory; the checkpoint keeps its place with zeros
        assert za.state2 == [] and [t.numel() for t in sd["exp_avg_sq"]] == za.shard_sizes
        assert all(not t.any() for t in sd["exp_avg_sq"])
    _, pb, zb = fresh()
    zb.load_state_dict(sd)
    assert zb.step_count == 2
    rs = draw_rs(pa, gen, 2.0, ws, dev)
    for z_, p_ in ((za, pa), (zb, pb)):
        backward_synthetic(z_, p_, rs)
        z_.step()
        z_.wait_allgather()
    for i, (a, b) in enumerate(zip(snap(za), snap(zb))):
        assert torch.equal(a, b), f"shard round trip: tensor {i} differs after one more step"
    assert torch.equal(za.sq_norms()[1].cpu(), zb.sq_norms()[1].cpu())
    full = za.consolidated_state_dict()
    _, _, zc = fresh()
    zc.load_consolidated_state_dict(full)
    for a, c in zip(za.master, zc.master):
        assert torch.equal(a.detach().cpu(), c.detach().cpu()), "consolidated round trip: master"
    for a, c in zip(za.params, zc.params):
        assert torch.equal(a.detach().cpu(), c.detach().cpu()), "consolidated round trip: parameters"
    for z_ in (za, zb, zc):
        z_.close()


# ------------------------------------------------------------------ pieces off a 4-element boundary
def run_unaligned_pieces(device, ldt, ws=3):
    """The sharded LAMB step on a hand-made layout: the SIZES tensors back to back in flat
    buffers (no alignment), cut into `ws` shards at element offsets that are not multiples of
    4.  One piece plan per "rank" (zero-element entries where a rank holds nothing), pass 1
    on each, the per-tensor vectors added in rank order (what a SUM all-reduce does), pass 2
    with the low-precision copy on each.  Checked as the engine test: sums within
    (numel + ws) * 2^-23 of float64, p bit for bit against the restatement fed the summed
    vector, the copy == p.to(ldt); and at least one piece does start off a 4-element boundary
    and at least one tensor is split."""
    from distributed_training_amd.multi_tensor import TensorListPlan

    hp, (bc1, bc2s) = _lamb_hp()
    p, g, m, v = CL.make_tensors("cpu", torch.float32, False, seed=23)
    offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    total = int(offs[-1])
    cuts = [0] + [total * (r + 1) // ws + 1 for r in range(ws - 1)] + [total]  # odd offsets
    assert all(c % 4 for c in cuts[1:-1])
    flat = {k: torch.cat(x).to(device) for k, x in (("p", p), ("g", g), ("m", m), ("v", v))}
    low = torch.full((total,), SENTINEL, dtype=ldt, device=device)
    rp, rg, rm, rv = to_np(p), to_np(g), to_np(m), to_np(v)
    n = len(SIZES)
    plans, vecs = [], []
    split = [0] * n
    odd = 0
    for r in range(ws):
        lo, hi = cuts[r], cuts[r + 1]
        pieces = []
        for t in range(n):
            a, e = max(int(offs[t]), lo), min(int(offs[t + 1]), hi)
            pieces.append((a, e - a) if e > a else (0, 0))
            split[t] += e > a
            odd += e > a and a % 4 != 0
        plan = TensorListPlan([k for _, k in pieces], device)
        for s_, key in enumerate("pgmv"):
            plan.set_ptrs(s_, [flat[key].data_ptr() + 4 * a if k else 0 for a, k in pieces])
        plan.set_ptrs(4, [low.data_ptr() + 2 * a if k else 0 for a, k in pieces])
        plan.set_adapt(CL.ADAPT)
        vec = torch.zeros(2 * n, dtype=torch.float32, device=device)
        plan.lamb_moments(torch.float32, *hp["betas"], hp["eps"], hp["wd"], bc1, bc2s, vec)
        plans.append(plan)
        vecs.append(vec)
    assert odd >= 1 and max(split) >= 2 and min(split[t] for t in range(n) if SIZES[t]) >= 1
    norms = vecs[0].clone()
    for vec in vecs[1:]:
        norms += vec
    for plan in plans:
        plan.lamb(hp["lr"], hp["eps"], hp["wd"], bc1, bc2s, norms, lowp_dtype=ldt)
        plan.close()
    sums = norms.cpu().numpy()
    want_p, want_m, want_v, u, _ = CL.ref_plan_step(rp, rg, rm, rv, CL.ADAPT, hp, 1, sums=sums)
    _assert_sums(sums, ws, (rp, u), "unaligned pieces")
    cut = lambda x: [x[int(offs[t]):int(offs[t + 1])] for t in range(n)]  # noqa: E731
    assert_lists_equal(to_np(cut(flat["m"])), want_m, "unaligned pieces: m")
    assert_lists_equal(to_np(cut(flat["v"])), want_v, "unaligned pieces: v")
    assert_lists_equal(to_np(cut(flat["p"])), want_p, "unaligned pieces: p")
    assert np.array_equal(_bits([low])[0], _bits([flat["p"].to(ldt)])[0]), "unaligned pieces: copy"
