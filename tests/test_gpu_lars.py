"""LARS on the GPU: the segmented per-tensor Σp², Σg² kernels (gs_lars_norms) and the
fused update (gs_lars_step) against the numpy float32 restatement of the contract
(tests/_lars_common.py), the found_inf skip, determinism across fresh plans, FusedLARS
on a small model, and one hipGraph recording of its step."""
import numpy as np
import pytest
import torch

from tests import _lars_common as C

pytestmark = pytest.mark.gpu

GRID = [(gdt, mom, wd) for gdt in (torch.float32, torch.bfloat16) for mom in (0.9, 0.0) for wd in (1e-4, 0.0)]


@pytest.mark.parametrize("mult", [None, 0.5])
@pytest.mark.parametrize("gdt,mom,wd", GRID)
def test_plan_exact_sum_inputs(cuda_device, gdt, mom, wd, mult):
    C.run_plan_steps(cuda_device, gdt, mom, wd, mult, exact=True)


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_plan_exact_sum_group_shapes(cuda_device, gdt):
    C.run_group_shapes(cuda_device, gdt)


@pytest.mark.parametrize("gdt,mom,wd", GRID)
def test_plan_random_inputs(cuda_device, gdt, mom, wd):
    C.run_plan_steps(cuda_device, gdt, mom, wd, None, exact=False)


def test_plan_fp16_grads(cuda_device):
    C.run_plan_steps(cuda_device, torch.float16, 0.9, 1e-4, 0.5, exact=True, steps=1)


def test_found_inf_writes_nothing(cuda_device):
    C.run_found_inf(cuda_device)


def test_two_fresh_plans_agree_bit_for_bit(cuda_device):
    outs = []
    for _ in range(2):
        p, g, b = C.make_tensors(cuda_device, torch.float32, False, seed=21)
        plan = C.make_plan(cuda_device, p, g, b, 0.9)
        norms = torch.zeros(2 * len(C.SIZES), dtype=torch.float32, device=cuda_device)
        C.plan_step(plan, torch.float32, norms, 0.9, 1e-4)
        outs.append((norms.cpu().numpy(), C.to_np(p), C.to_np(b)))
        plan.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    C.assert_lists_equal(outs[0][1], outs[1][1], "p")
    C.assert_lists_equal(outs[0][2], outs[1][2], "buf")


def test_fused_lars_small_model(cuda_device):
    C.run_fused_lars(cuda_device)


def test_recorded_step_follows_lr(cuda_device):
    """One torch.cuda.graph recording of FusedLARS(capturable=True).step() on a single
    stream (a linear graph), replayed with lr changed between replays through
    refresh_hyper(): bit-exact against an eager optimizer given the same grads."""
    import copy

    import distributed_training_amd as D

    kw = dict(lr=0.2, momentum=0.9, weight_decay=1e-4, trust_coefficient=1e-3)
    me = C.small_model(cuda_device)
    mg = copy.deepcopy(me)
    pe, pg = list(me.parameters()), list(mg.parameters())
    oe, og = D.FusedLARS(pe, capturable=False, **kw), D.FusedLARS(pg, capturable=True, **kw)
    static = [torch.zeros_like(p) for p in pg]
    for p, s in zip(pg, static):
        p.grad = s
    graph = None
    for it in range(3):
        if it == 2:
            for o in (oe, og):
                o.param_groups[0]["lr"] = 0.05
        grads = C.synthetic_grads(me, 300 + it)
        for p, gr in zip(pe, grads):
            p.grad = gr.clone()
        oe.step()
        for s, gr in zip(static, grads):
            s.copy_(gr)
        if it == 0:
            og.step()  # the eager step creates the state, the flags and the scratch
            continue
        if graph is None:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                og.step()
        og.refresh_hyper()
        graph.replay()
    torch.cuda.synchronize()
    C.assert_lists_equal(C.to_np(pg), C.to_np(pe), "p")
    C.assert_lists_equal(C.to_np([og.state[p]["momentum_buffer"] for p in pg]),
                         C.to_np([oe.state[p]["momentum_buffer"] for p in pe]), "buf")
    assert og.kernel_ms() == []  # no timer enabled: nothing recorded
