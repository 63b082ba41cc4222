"""LARS on the host backend (CPU tensors): gs_plan_set_adapt / gs_lars_norms /
gs_lars_step and FusedLARS against the numpy float32 restatement of the contract
(tests/_lars_common.py), the argument errors, and two gloo ranks that must stay
bit-identical through DDP + FusedLARS."""

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import _lars_common as C
from tests.test_ddp_cpu import _run

CPU = torch.device("cpu")
GRID = [(gdt, mom, wd) for gdt in (torch.float32, torch.bfloat16) for mom in (0.9, 0.0) for wd in (1e-4, 0.0)]


@pytest.mark.parametrize("mult", [None, 0.5])
@pytest.mark.parametrize("gdt,mom,wd", GRID)
def test_plan_exact_sum_inputs(gdt, mom, wd, mult):
    C.run_plan_steps(CPU, gdt, mom, wd, mult, exact=True)


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_plan_exact_sum_group_shapes(gdt):
    C.run_group_shapes(CPU, gdt)


@pytest.mark.parametrize("gdt,mom,wd", GRID)
def test_plan_random_inputs(gdt, mom, wd):
    C.run_plan_steps(CPU, gdt, mom, wd, None, exact=False)


def test_found_inf_writes_nothing():
    C.run_found_inf(CPU)


def test_fused_lars_small_model():
    C.run_fused_lars(CPU)


def test_fused_lars_adapt_key_and_skipped_grads():
    """adapt=True adapts (and decays) every tensor, False none; a parameter without a grad is skipped."""
    import distributed_training_amd as D

    for adapt in (True, False):
        model = C.small_model(CPU)
        params = list(model.parameters())
        opt = D.FusedLARS([{"params": params, "adapt": adapt}], lr=0.1, momentum=0.0, weight_decay=1e-2)
        grads = C.synthetic_grads(model, 7)
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        params[1].grad = None
        before = C.to_np(params)
        opt.step()
        ((ps, norms),) = opt.sq_norms()
        live = [i for i in range(len(params)) if i != 1]
        assert [id(x) for x in ps] == [id(params[i]) for i in live]
        rp, _ = C.ref_step([before[i] for i in live], C.to_np([grads[i] for i in live]),
                           [np.zeros_like(before[i]) for i in live],
                           norms.numpy(), [adapt] * len(live), 0.1, 0.0, 1e-2, 1e-3, 1e-8)
        C.assert_lists_equal(C.to_np([params[i] for i in live]), rp, f"adapt={adapt}")
        assert np.array_equal(params[1].detach().numpy().reshape(-1), before[1])
        assert "momentum_buffer" not in opt.state[params[0]]


def test_argument_errors():
    from distributed_training_amd import _lib as L

    p, g, b = C.make_tensors(CPU, torch.float32, False, seed=1)
    plan = C.make_plan(CPU, p, g, b, 0.9)
    norms = torch.zeros(2 * len(C.SIZES))
    lib, h, nptr = L.lib(), plan.handle, norms.data_ptr()

    def step(handle=h, gdt=L.GS_F32, lr=0.1, mom=0.9, wd=0.0, eta=1e-3, eps=1e-8, norms_ptr=nptr):
        return lib.gs_lars_step(handle, gdt, lr, mom, wd, eta, eps, norms_ptr, None, None, None)

    assert lib.gs_plan_set_adapt(None, L.i32_array([1])) == L.GS_EINVAL
    assert lib.gs_plan_set_adapt(h, None) == L.GS_EINVAL
    assert lib.gs_lars_norms(None, L.GS_F32, nptr, None) == L.GS_EINVAL
    assert lib.gs_lars_norms(h, L.GS_F32, None, None) == L.GS_EINVAL
    assert lib.gs_lars_norms(h, L.GS_I64, nptr, None) == L.GS_EINVAL
    assert step(handle=None) == L.GS_EINVAL
    assert step(gdt=L.GS_F64) == L.GS_EINVAL
    assert step(norms_ptr=None) == L.GS_EINVAL
    assert step(mom=-0.1) == L.GS_EINVAL
    assert step(wd=-1.0) == L.GS_EINVAL
    assert step(eta=-1.0) == L.GS_EINVAL
    assert step(eps=-1.0) == L.GS_EINVAL
    # momentum without a bound buffer slot
    plan2 = C.make_plan(CPU, p, g, b, 0.0)
    assert lib.gs_lars_norms(plan2.handle, L.GS_F32, nptr, None) == L.GS_OK
    assert step(handle=plan2.handle, mom=0.9) == L.GS_EINVAL
    assert step(handle=plan2.handle, mom=0.0) == L.GS_OK
    # a clip configured on the plan: clipping is not part of LARS
    sq = torch.ones(1)
    plan.set_clip(1.0, 1e-6, sq)
    before = C.to_np(p)
    assert step() == L.GS_ESTATE
    assert b"clip" in lib.gs_last_error()
    C.assert_lists_equal(C.to_np(p), before, "rejected step wrote nothing")
    plan.set_clip(None)
    assert lib.gs_lars_norms(h, L.GS_F32, nptr, None) == L.GS_OK
    assert step() == L.GS_OK
    with pytest.raises(ValueError):
        plan.set_adapt([1, 0])
    with pytest.raises(ValueError):
        plan.lars_norms(torch.float32, torch.zeros(3))


def _ddp_lars_worker(rank, ws):
    import torch.distributed as dist

    import distributed_training_amd as D

    model = C.small_model(CPU, seed=40 + rank)  # DDP broadcasts rank 0's init
    ddp = D.DistributedDataParallel(model)
    opt = D.FusedLARS(ddp.parameters(), lr=0.5, momentum=0.9, weight_decay=1e-4, trust_coefficient=1e-2)
    crit = nn.CrossEntropyLoss()
    gen = torch.Generator().manual_seed(900 + rank)  # different inputs per rank
    for _ in range(3):
        x = torch.randn(4, 3, 8, 8, generator=gen)
        y = torch.randint(0, 10, (4,), generator=gen)
        crit(ddp(x), y).backward()
        opt.step()
        opt.zero_grad()
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()] +
                     [opt.state[p]["momentum_buffer"].reshape(-1) for p in model.parameters()])
    both = [torch.empty_like(flat) for _ in range(ws)]
    dist.all_gather(both, flat)
    assert flat.abs().sum() > 0 and torch.isfinite(flat).all()
    assert torch.equal(both[0].view(torch.int32), both[1].view(torch.int32)), "ranks diverged"


def test_ddp_ranks_stay_bit_identical_gloo():
    _run(_ddp_lars_worker, 2)
