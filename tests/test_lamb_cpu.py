"""LAMB on the host backend (CPU tensors): gs_lamb_moments / gs_lamb_step / gs_lamb_hyper
and FusedLAMB against the numpy float32 restatement of the contract
(tests/_lamb_common.py), the argument errors, and the DeepSpeed / ColossalAI shims."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import _lamb_common as C
from tests.test_ddp_cpu import _run

CPU = torch.device("cpu")
SHIMS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distributed_training_amd",
                     "compat", "shims")


@pytest.mark.parametrize("gdt,mult", [(torch.float32, None), (torch.bfloat16, None), (torch.float16, 0.5)])
def test_exact_sum_step(gdt, mult):
    C.run_exact_step(CPU, gdt, mult)


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_exact_sum_step_group_shapes(gdt):
    C.run_group_shapes(CPU, gdt)


def test_lars_and_lamb_passes_share_one_order():
    C.run_shared_order(CPU, torch.float32)


@pytest.mark.parametrize("bias_correction", [True, False])
@pytest.mark.parametrize("wd", [0.01, 0.0])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_random_inputs_three_steps(gdt, wd, bias_correction):
    C.run_random_steps(CPU, gdt, wd, bias_correction)


def test_trust_ratio_clamp():
    C.run_clamp(CPU)


def test_found_inf_writes_nothing():
    C.run_found_inf(CPU)


def test_two_fresh_plans_agree_bit_for_bit():
    C.run_determinism(CPU)


def test_fused_lamb_small_model():
    C.run_fused_lamb(CPU)


def test_fused_lamb_max_grad_norm():
    C.run_fused_lamb(CPU, max_grad_norm=0.5)


def test_fused_lamb_device_counters_match_host_counters():
    """found_inf set (the AMP path): the step counter and the bias corrections live in
    memory the kernels read (gs_lamb_hyper); a skipped step advances nothing, and the
    clean steps equal an optimizer that counts on the host."""
    import distributed_training_amd as D

    ma = C.small_model(CPU)
    mb = copy.deepcopy(ma)
    pa, pb = list(ma.parameters()), list(mb.parameters())
    oa, ob = D.FusedLAMB(pa, **C.LAMB_KW), D.FusedLAMB(pb, **C.LAMB_KW)
    ob.found_inf = torch.zeros(1)
    ob.grad_scale = torch.ones(1)
    for s in range(4):
        grads = C.synthetic_grads(ma, 400 + s)
        skip = s == 1
        ob.found_inf.fill_(1.0 if skip else 0.0)
        before = C.to_np(pb)
        C._set_grads(pb, grads)
        ob.step()
        if skip:
            C.assert_lists_equal(C.to_np(pb), before, "skipped step")
            continue
        C._set_grads(pa, grads)
        oa.step()
        C.assert_lists_equal(C.to_np(pb), C.to_np(pa), f"step {s}: p")
    assert float(ob.state_dict()["state"][0]["step"]) == 3.0
    assert ob.kernel_ms() == []


def test_fused_lamb_adapt_key_and_constructor_errors():
    import distributed_training_amd as D

    for adapt in (True, False):
        model = C.small_model(CPU)
        params = list(model.parameters())
        opt = D.FusedLAMB([{"params": params, "adapt": adapt}], **C.LAMB_KW)
        grads = C.synthetic_grads(model, 7)
        C._set_grads(params, grads)
        params[1].grad = None
        before = C.to_np(params)
        opt.step()
        ((ps, norms),) = opt.sq_norms()
        live = [i for i in range(len(params)) if i != 1]
        assert [id(x) for x in ps] == [id(params[i]) for i in live]
        hp = dict(lr=C.LAMB_KW["lr"], betas=C.LAMB_KW["betas"], eps=C.LAMB_KW["eps"],
                  wd=C.LAMB_KW["weight_decay"], bias_correction=True)
        zeros = [np.zeros_like(before[i]) for i in live]
        rp, *_ = C.ref_plan_step([before[i] for i in live], C.to_np([grads[i] for i in live]), zeros, zeros,
                                 [adapt] * len(live), hp, 1, sums=norms.numpy())
        C.assert_lists_equal(C.to_np([params[i] for i in live]), rp, f"adapt={adapt}")
        assert np.array_equal(params[1].detach().numpy().reshape(-1), before[1])
        assert "exp_avg" not in opt.state[params[1]]
    p = [nn.Parameter(torch.zeros(3))]
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(weight_decay=-0.1),
               dict(min_trust=2.0, max_trust=1.0)):
        with pytest.raises(ValueError):
            D.FusedLAMB(p, **kw)


def test_argument_errors():
    from distributed_training_amd import _lib as L

    p, g, m, v = C.make_tensors(CPU, torch.float32, False, seed=1)
    plan = C.make_plan(CPU, p, g, m, v)
    norms = C.new_norms(CPU)
    lib, h, nptr = L.lib(), plan.handle, norms.data_ptr()

    def mom(handle=h, gdt=L.GS_F32, b1=0.9, b2=0.999, eps=1e-6, wd=0.01, bc1=0.1, bc2s=0.03, norms_ptr=nptr):
        return lib.gs_lamb_moments(handle, gdt, b1, b2, eps, wd, bc1, bc2s, norms_ptr, None, None, None)

    def upd(handle=h, lr=0.1, eps=1e-6, wd=0.01, bc1=0.1, bc2s=0.03, lo=0.0, hi=float("inf"), norms_ptr=nptr):
        return lib.gs_lamb_step(handle, lr, eps, wd, bc1, bc2s, lo, hi, norms_ptr, None, None)

    assert mom(handle=None) == L.GS_EINVAL
    assert mom(gdt=L.GS_I64) == L.GS_EINVAL
    assert mom(norms_ptr=None) == L.GS_EINVAL
    assert mom(b1=1.0) == L.GS_EINVAL
    assert mom(eps=-1.0) == L.GS_EINVAL
    assert mom(bc1=0.0) == L.GS_EINVAL
    assert upd(handle=None) == L.GS_EINVAL
    assert upd(norms_ptr=None) == L.GS_EINVAL
    assert upd(wd=-1.0) == L.GS_EINVAL
    assert upd(lo=2.0, hi=1.0) == L.GS_EINVAL
    assert upd(bc2s=0.0) == L.GS_EINVAL
    assert lib.gs_lamb_hyper(L.GS_DEV_HOST, None, None, 0.9, 0.999, 1, None, None, None) == L.GS_EINVAL
    # the moments need all four slots
    from distributed_training_amd.multi_tensor import TensorListPlan

    plan2 = TensorListPlan(C.SIZES, CPU)
    for s, ts in enumerate((p, g, m)):
        plan2.set_ptrs(s, ts)
    assert mom(handle=plan2.handle) == L.GS_EINVAL
    # a clip configured on the plan: LAMB's pre-normalisation is the grad multiplier
    plan.set_clip(1.0, 1e-6, torch.ones(1))
    before = [C.to_np(x) for x in (p, m, v)]
    assert mom() == L.GS_ESTATE and b"clip" in lib.gs_last_error()
    assert upd() == L.GS_ESTATE
    for x, b in zip((p, m, v), before):
        C.assert_lists_equal(C.to_np(x), b, "rejected calls wrote nothing")
    plan.set_clip(None)
    assert mom() == L.GS_OK and upd() == L.GS_OK
    with pytest.raises(ValueError):
        plan.lamb_moments(torch.float32, 0.9, 0.999, 1e-6, 0.0, 1.0, 1.0, torch.zeros(3))


def test_lamb_hyper_host():
    """gs_lamb_hyper on host memory: the step advances unless found_inf, hyper = [lr, bc1, bc2s]."""
    from distributed_training_amd import _lib as L

    step, lr = torch.tensor([2.0], dtype=torch.float64), torch.tensor([0.25], dtype=torch.float64)
    hyper, fi = torch.zeros(3), torch.zeros(1)

    def call(bias_correction=1):
        L.check(L.lib().gs_lamb_hyper(L.GS_DEV_HOST, step.data_ptr(), lr.data_ptr(), 0.9, 0.999, bias_correction,
                                      fi.data_ptr(), hyper.data_ptr(), None), "gs_lamb_hyper")

    call()
    bc1, bc2s = C.bias_corrections(0.9, 0.999, 3.0)
    assert step.item() == 3.0 and np.array_equal(hyper.numpy(), np.array([0.25, bc1, bc2s], dtype=np.float32))
    fi.fill_(1.0)
    call(0)
    assert step.item() == 3.0 and hyper.tolist() == [0.25, 1.0, 1.0]


# ---- the wrapper APIs
def _ds_lamb_worker(rank, ws):
    sys.path.insert(0, SHIMS)
    import deepspeed

    import distributed_training_amd as D

    lamb = {"lr": 0.01, "max_coeff": 0.3, "min_coeff": 0.05}
    cfg = {"train_batch_size": 4, "optimizer": {"type": "Lamb", "params": dict(lamb)},
           "zero_optimization": {"stage": 0}}
    me = C.small_model(CPU)
    mh = copy.deepcopy(me)
    engine, opt, _, _ = deepspeed.initialize(args=None, model=me, model_parameters=me.parameters(), config=cfg)
    assert type(opt) is D.FusedLAMB and opt.param_groups[0]["adapt"] is True
    dev = engine.device  # the engine moves its module to the rank's device
    mh = mh.to(dev)
    # DeepSpeed's defaults: eps 1e-8, no decay, bias correction, no pre-normalisation
    hand = D.FusedLAMB([{"params": list(mh.parameters()), "adapt": True}], lr=0.01, eps=1e-8, weight_decay=0.0,
                       bias_correction=True, min_trust=0.05, max_trust=0.3)
    crit = nn.CrossEntropyLoss()
    gen = torch.Generator().manual_seed(3)
    for _ in range(2):
        x, y = torch.randn(4, 3, 8, 8, generator=gen).to(dev), torch.randint(0, 10, (4,), generator=gen).to(dev)
        engine.backward(crit(me(x), y))
        engine.step()
        crit(mh(x), y).backward()
        hand.step()
        hand.zero_grad()
    C.assert_lists_equal(C.to_np(me.parameters()), C.to_np(mh.parameters()), "engine vs hand-built")
    # the clamp was in force: some ratio of the last step lies outside [0.05, 0.3]
    ((_, norms),) = hand.sq_norms()
    free = np.array(C.ref_ratios(norms.cpu().numpy(), [True] * 6))
    assert (free < 0.05).any() or (free > 0.3).any()
    for key in ("FusedLamb", "LAMB"):
        cfg2 = copy.deepcopy(cfg)
        cfg2["optimizer"]["type"] = key
        cfg2["gradient_clipping"] = 0.5
        e2, o2, _, _ = deepspeed.initialize(args=None, model=C.small_model(CPU), config=cfg2)
        assert type(o2) is D.FusedLAMB and o2.defaults["max_grad_norm"] == 0.5
    for bad in ({"zero_optimization": {"stage": 2}}, {"bf16": {"enabled": True}}):
        with pytest.raises(NotImplementedError, match="span ranks"):
            deepspeed.initialize(args=None, model=C.small_model(CPU), config=dict(cfg, **bad))


def test_deepspeed_lamb():
    _run(_ds_lamb_worker, 1)


def test_colossalai_lamb_shims():
    import subprocess

    import distributed_training_amd as D
    from distributed_training_amd.compat import colossalai as CA

    # through the shim path, in a fresh interpreter (this one may hold another `colossalai`)
    code = ("import sys; sys.path.insert(0, sys.argv[1]);"
            "from colossalai.nn.optimizer import Lamb, FusedLAMB, HybridAdam;"
            "import distributed_training_amd as D;"
            "assert issubclass(Lamb, D.FusedLAMB) and issubclass(FusedLAMB, D.FusedLAMB);"
            "assert 'shims' in sys.modules['colossalai'].__file__")
    subprocess.run([sys.executable, "-c", code, SHIMS], check=True,
                   cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    model = C.small_model(CPU)
    a = CA.Lamb(model.parameters(), lr=0.01, weight_decay=0.01)
    assert isinstance(a, D.FusedLAMB) and a.param_groups[0]["adapt"] is True
    assert a.defaults["bias_correction"] is False and a.defaults["eps"] == 1e-6
    assert CA.Lamb(model.parameters(), adam=True).param_groups[0]["adapt"] is False
    b = CA.FusedLAMB(model.parameters(), lr=0.01)
    assert b.defaults["max_grad_norm"] == 1.0 and b.defaults["weight_decay"] == 0.01
    assert b.param_groups[0]["adapt"] is None
    assert CA.FusedLAMB(model.parameters(), use_nvlamb=True, max_grad_norm=0.0).defaults["max_grad_norm"] is None
    with pytest.raises(NotImplementedError):
        CA.FusedLAMB(model.parameters(), amsgrad=True)
    # a step through each runs the library
    for opt in (a, b):
        C._set_grads(model.parameters(), C.synthetic_grads(model, 1))
        opt.step()
    with pytest.raises(NotImplementedError, match="span ranks"):
        CA.LowLevelZeroPlugin().configure(model, b, None)


def _colossal_ddp_worker(rank, ws):
    from distributed_training_amd.compat import colossalai as CA

    model = C.small_model(CPU)
    opt = CA.Lamb(model.parameters(), lr=0.01)
    booster = CA.Booster(plugin=CA.TorchDDPPlugin())
    model, opt, crit, _, _ = booster.boost(model, opt, criterion=nn.CrossEntropyLoss())
    before = C.to_np(CA._unwrap(model).parameters())
    dev = next(model.parameters()).device  # the plugin moves the model to the rank's device
    x, y = torch.randn(4, 3, 8, 8).to(dev), torch.randint(0, 10, (4,)).to(dev)
    booster.backward(crit(model(x), y), opt)
    opt.step()
    opt.zero_grad()
    after = C.to_np(CA._unwrap(model).parameters())
    assert any(not np.array_equal(a, b) for a, b in zip(after, before))


def test_colossalai_ddp_plugin_accepts_lamb():
    _run(_colossal_ddp_worker, 1)
