"""FusedMuon through the host backend: the step against the fp64 restatement of torch's
formulae (tests/_muon_ref.py), the state_dict exchange with torch.optim.Muon, the
parameters and settings it refuses, and a parameter without a grad."""
import pytest
import torch

import distributed_training_amd as D
from tests import _muon_ref as R


@pytest.mark.parametrize("nesterov,adjust", [(True, None), (False, "match_rms_adamw")])
def test_step_against_fp64(nesterov, adjust):
    lr, wd, mom = 0.02, 0.1, 0.95
    gen = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(R.make(s, "cpu", gen)) for s in R.CPU_SHAPES]
    opt = D.FusedMuon(ps, lr=lr, weight_decay=wd, momentum=mom, nesterov=nesterov, adjust_lr_fn=adjust)
    p64 = [R.matrix(p) for p in ps]
    b64 = [torch.zeros_like(m) for m in p64]
    for _ in range(2):
        us = []
        for i, (p, s) in enumerate(zip(ps, R.CPU_SHAPES)):
            p.grad = R.make(s, "cpu", gen)
            b64[i], u = R.direction(R.matrix(p.grad), b64[i], mom, nesterov)
            us.append(u)
        opt.step()
        plan = opt._plans.plans()[0]
        for i, u in enumerate(us):
            A, B = u.shape
            o = R.fused_x(plan, plan._muon_space, i, 1, A, B)
            err = R.rel_err(o, R.newton_schulz(u, 5, 1e-7))
            assert err <= 1.5 * R.torch_ns_err(u, 5, 1e-7, "cpu"), (R.CPU_SHAPES[i], err)
            p64[i] = p64[i] * (1 - lr * wd) - R.adjusted_lr(lr, adjust, A, B) * o
    for p, pr, br in zip(ps, p64, b64):
        torch.testing.assert_close(R.matrix(opt.state[p]["momentum_buffer"]), br, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(R.matrix(p), pr, rtol=1e-6, atol=1e-6)


def test_state_dict_round_trip_with_torch():
    gen = torch.Generator().manual_seed(5)
    mine = [torch.nn.Parameter(R.make(s, "cpu", gen)) for s in [(96, 40), (33, 65)]]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    fused, ref = D.FusedMuon(mine, lr=0.02), torch.optim.Muon(theirs, lr=0.02)
    for p in mine:
        p.grad = R.make(tuple(p.shape), "cpu", gen)
    fused.step()
    ref.load_state_dict(fused.state_dict())
    for p, q in zip(mine, theirs):
        assert torch.equal(ref.state[q]["momentum_buffer"], fused.state[p]["momentum_buffer"])
        q.grad = p.grad.clone()
    ref.step()
    fused.load_state_dict(ref.state_dict())
    assert fused.param_groups[0]["ns_steps"] == 5
    for p, q in zip(mine, theirs):
        assert torch.equal(fused.state[p]["momentum_buffer"], ref.state[q]["momentum_buffer"])
    fused.step()  # the loaded buffers are the ones the next step advances


@pytest.mark.parametrize("bad", ["1d", "dim0_inner", "bf16_param", "found_inf", "capturable", "max_grad_norm"])
def test_refused(bad):
    w = torch.nn.Parameter(torch.randn(8, 4))
    if bad == "1d":
        with pytest.raises(ValueError):
            D.FusedMuon([torch.nn.Parameter(torch.randn(8))])
    elif bad == "dim0_inner":
        with pytest.raises(ValueError):
            D.FusedMuon([torch.nn.Parameter(torch.randn(3, 3, 4, 8).permute(3, 2, 0, 1))])
    elif bad in ("capturable", "max_grad_norm"):
        with pytest.raises(ValueError):
            D.FusedMuon([w], **{bad: 1.0})
    else:
        if bad == "bf16_param":
            w = torch.nn.Parameter(torch.randn(8, 4).bfloat16())
        opt = D.FusedMuon([w])
        w.grad = torch.randn_like(w)
        if bad == "found_inf":
            opt.found_inf = torch.zeros(1)
        with pytest.raises(RuntimeError):
            opt.step()


def test_grad_none_is_skipped():
    a, b = torch.nn.Parameter(torch.randn(8, 4)), torch.nn.Parameter(torch.randn(4, 8))
    before = b.detach().clone()
    opt = D.FusedMuon([a, b])
    a.grad = torch.randn_like(a)
    opt.step()
    assert torch.equal(b, before) and "momentum_buffer" not in opt.state[b] and "momentum_buffer" in opt.state[a]
