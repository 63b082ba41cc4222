"""LAMB on the GPU: the fused moments pass with its segmented per-tensor Σp², Σu²
(gs_lamb_moments) and the trust-ratio update (gs_lamb_step) against the numpy float32
restatement of the contract (tests/_lamb_common.py), the clamp, the found_inf skip,
determinism across fresh plans, FusedLAMB on a small model, and one hipGraph recording
of its step."""
import pytest
import torch

from tests import _lamb_common as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("gdt,mult", [(torch.float32, None), (torch.bfloat16, None), (torch.float16, 0.5)])
def test_exact_sum_step(cuda_device, gdt, mult):
    C.run_exact_step(cuda_device, gdt, mult)


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_exact_sum_step_group_shapes(cuda_device, gdt):
    C.run_group_shapes(cuda_device, gdt)


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_lars_and_lamb_passes_share_one_order(cuda_device, gdt):
    C.run_shared_order(cuda_device, gdt)


@pytest.mark.parametrize("bias_correction", [True, False])
@pytest.mark.parametrize("wd", [0.01, 0.0])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_random_inputs_three_steps(cuda_device, gdt, wd, bias_correction):
    C.run_random_steps(cuda_device, gdt, wd, bias_correction)


def test_trust_ratio_clamp(cuda_device):
    C.run_clamp(cuda_device)


def test_found_inf_writes_nothing(cuda_device):
    C.run_found_inf(cuda_device)


def test_two_fresh_plans_agree_bit_for_bit(cuda_device):
    C.run_determinism(cuda_device)


def test_fused_lamb_small_model(cuda_device):
    C.run_fused_lamb(cuda_device)


def test_fused_lamb_max_grad_norm(cuda_device):
    C.run_fused_lamb(cuda_device, max_grad_norm=0.5)


def test_recorded_step_follows_lr(cuda_device):
    """One torch.cuda.graph recording of FusedLAMB(capturable=True).step() on a single
    stream (a linear graph), replayed with lr changed between replays through
    refresh_hyper(): bit-exact against an eager twin given the same grads."""
    import copy

    import distributed_training_amd as D

    me = C.small_model(cuda_device)
    mg = copy.deepcopy(me)
    pe, pg = list(me.parameters()), list(mg.parameters())
    oe, og = D.FusedLAMB(pe, capturable=False, **C.LAMB_KW), D.FusedLAMB(pg, capturable=True, **C.LAMB_KW)
    static = [torch.zeros_like(p) for p in pg]
    for p, s in zip(pg, static):
        p.grad = s
    graph = None
    for it in range(4):
        if it == 2:
            for o in (oe, og):
                o.param_groups[0]["lr"] = 0.005
        grads = C.synthetic_grads(me, 300 + it)
        C._set_grads(pe, grads)
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
    for key in ("exp_avg", "exp_avg_sq"):
        C.assert_lists_equal(C._state(og, pg, key), C._state(oe, pe, key), key)
    assert float(og.state_dict()["state"][0]["step"]) == 4.0
    assert og.kernel_ms() == []  # no timer enabled: nothing recorded

