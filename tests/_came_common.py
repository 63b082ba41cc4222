"""Checks shared by tests/test_came_cpu.py (host backend) and tests/test_gpu_came.py: FusedCAME
against the per-tensor arithmetic of include/gsync.h restated in plain torch (`came_reference`),
run on float64 CPU copies, with the same restatement in float32 as the yardstick.  Shapes:
tests/_adafactor_common.py's CASES, unchanged."""
import torch

import distributed_training_amd as D
from tests._adafactor_common import CASES, NO_GRAD, ZERO_GRAD, ZERO_ROW, copies, grads, masters, rel, set_grads

STATE_KEYS = ("exp_avg", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_res_row", "exp_avg_res_col", "exp_avg_sq")
STEP_CASES = [(0.0, 1.0, 1e-2), (0.1, 1.0, 1e-3), (0.0, 4.0, 1e-2), (0.0, 1000.0, 1e-2)]


def _factors(row, col):
    return (row / row.mean(-1, keepdim=True)).rsqrt().unsqueeze(-1) * col.unsqueeze(-2).rsqrt()


@torch.no_grad()
def came_reference(params, state, lr, eps=(1e-30, 1e-16), clip_threshold=1.0, betas=(0.9, 0.999, 0.9999),
                   weight_decay=0.0):
    """One CAME step per parameter with a grad, in the parameters' own dtype; state: {index: dict}."""
    for i, p in enumerate(params):
        if p.grad is None:
            continue
        g, st = p.grad, state.setdefault(i, {})
        if not st:
            st["exp_avg"] = torch.zeros_like(g)
            if g.dim() >= 2:
                for k in STATE_KEYS[1:5]:
                    st[k] = g.new_zeros(g.shape[:-2] + g.shape[-1:] if k.endswith("col") else g.shape[:-1])
            else:
                st["exp_avg_sq"] = torch.zeros_like(g)
        s = g * g + eps[0]
        if g.dim() >= 2:
            st["exp_avg_sq_row"].mul_(betas[1]).add_(s.mean(-1) * (1 - betas[1]))
            st["exp_avg_sq_col"].mul_(betas[1]).add_(s.mean(-2) * (1 - betas[1]))
            u = g * _factors(st["exp_avg_sq_row"], st["exp_avg_sq_col"])
        else:
            st["exp_avg_sq"].mul_(betas[1]).add_(s * (1 - betas[1]))
            u = g * st["exp_avg_sq"].rsqrt()
        u = u / ((u * u).sum() / u.numel()).sqrt().div(clip_threshold).clamp(min=1.0)
        m = st["exp_avg"].mul_(betas[0]).add_(u * (1 - betas[0]))
        upd = m
        if g.dim() >= 2:
            q = (u - m) ** 2 + eps[1]
            st["exp_avg_res_row"].mul_(betas[2]).add_(q.mean(-1) * (1 - betas[2]))
            st["exp_avg_res_col"].mul_(betas[2]).add_(q.mean(-2) * (1 - betas[2]))
            upd = m * _factors(st["exp_avg_res_row"], st["exp_avg_res_col"])
        if weight_decay != 0:
            p.add_(p * (-weight_decay * lr))
        p.sub_(lr * upd)


def check_three_steps(device, weight_decay, clip_threshold, lr):
    """e(fused) <= 4 * e(reference fp32) + 8 * 2**-23 per parameter and state tensor, e against fp64."""
    gen = torch.Generator().manual_seed(13)
    m = masters(gen)
    kw = dict(lr=lr, weight_decay=weight_decay, clip_threshold=clip_threshold)
    pf, p32, p64 = copies(m, device), copies(m), copies(m, dtype=torch.float64)
    of, s32, s64 = D.FusedCAME(pf, **kw), {}, {}
    for _ in range(3):
        gs = grads(gen)
        for ps in (pf, p32, p64):
            set_grads(ps, gs)
        of.step()
        came_reference(p32, s32, **kw)
        came_reference(p64, s64, **kw)
    for i, (a, b, c) in enumerate(zip(pf, p32, p64)):
        if i == NO_GRAD:
            assert len(of.state[a]) == 0 and torch.equal(a.cpu(), m[i])
            continue
        assert of.state[a]["step"] == 3 and "RMS" not in of.state[a]
        assert set(of.state[a]) == set(s64[i]) | {"step"}
        assert of.state[a]["exp_avg"].stride() == a.stride()
        triples = [("param", a, b, c)] + [(k, of.state[a][k], s32[i][k], s64[i][k]) for k in s64[i]]
        for name, x, y32, y64 in triples:
            assert x.shape == y64.shape, (CASES[i], name)
            ef, et = rel(x, y64.detach()), rel(y32, y64.detach())
            print(f"{CASES[i]} {name}: e(fused) {ef:.3e} e(reference fp32) {et:.3e}")
            assert ef <= 4 * et + 8 * 2.0 ** -23, (CASES[i], name, ef, et)


def check_exact_stats(device):
    """beta2 = beta3 = 0, eps = 0, grads from +-{1, 2, 3}: the first statistics are exact means."""
    cases = [c for i, c in enumerate(CASES) if i not in (ZERO_ROW, ZERO_GRAD, NO_GRAD)]
    gen = torch.Generator().manual_seed(11)
    ps = copies(masters(gen, cases), device)
    gs = grads(gen, cases, ints=True)
    for g in gs:  # in place: the layout stays
        g.copy_(torch.randint(1, 4, g.shape, generator=gen) * (2 * torch.randint(0, 2, g.shape, generator=gen) - 1))
    opt = D.FusedCAME(ps, lr=1e-2, betas=(0.9, 0.0, 0.0), eps=(0.0, 0.0))
    set_grads(ps, gs)
    opt.step()
    for case, p, g in zip(cases, ps, gs):
        st = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in opt.state[p].items()}
        assert st["step"] == 1
        if g.dim() >= 2:
            assert torch.equal(st["exp_avg_sq_row"], (g * g).sum(-1) / g.shape[-1]), case
            assert torch.equal(st["exp_avg_sq_col"], (g * g).sum(-2) / g.shape[-2]), case
        else:
            assert torch.equal(st["exp_avg_sq"], g * g), case


def final_state(device, seed=17):
    """Parameters and state tensors after three steps from a seeded state."""
    gen = torch.Generator().manual_seed(seed)
    ps = copies(masters(gen), device)
    opt = D.FusedCAME(ps, lr=1e-2, weight_decay=0.1)
    for _ in range(3):
        set_grads(ps, grads(gen))
        opt.step()
    return [p.detach() for p in ps] + [opt.state[p][k] for p in ps for k in STATE_KEYS if k in opt.state[p]]
