"""Shapes and checks shared by tests/test_adafactor_cpu.py (host backend) and
tests/test_gpu_adafactor.py: FusedAdafactor against torch.optim.Adafactor itself on float64
CPU copies, with torch.optim.Adafactor in fp32 on the CPU as the yardstick."""
import torch

import distributed_training_amd as D

EPS1 = torch.finfo(torch.float32).eps
EPS2 = 1e-3
_LANE = [(5, 3, 1, 1), (3, 5, 3, 3), (65, 4, 3, 3), (4, 65, 3, 3), (4, 3, 7, 7), (2, 3, 1, 7), (2, 2, 8, 8)]
# (shape, channels_last): vectors, a lane per matrix in both layouts, tiled
CASES = [(s, False) for s in [(), (1,), (63,), (65,), (1000,)]] + \
        [(s, cl) for s in _LANE for cl in (False, True)] + \
        [(s, False) for s in [(9, 8), (1, 65), (65, 1), (65, 257), (10, 512), (2, 3, 9, 8)]]
# ... then a tensor whose gradient has an all-zero row, one whose gradient is all zero, one without a grad
ZERO_ROW, ZERO_GRAD, NO_GRAD = len(CASES), len(CASES) + 1, len(CASES) + 2
CASES = CASES + [((6, 70), False), ((3, 5, 3, 3), True), ((7,), False)]
STATE_KEYS = ("row_var", "col_var", "variance")


def _tensor(shape, cl, gen, ints):
    x = torch.randint(-3, 4, shape, generator=gen).float() if ints else torch.randn(shape, generator=gen)
    return x.contiguous(memory_format=torch.channels_last) if cl else x


def masters(gen, cases=CASES):
    return [_tensor(s, cl, gen, False) for s, cl in cases]


def grads(gen, cases=CASES, ints=False):
    out = [_tensor(s, cl, gen, ints) * (1.0 if ints else 0.1) for s, cl in cases]
    if cases is CASES:
        out[ZERO_ROW][2] = 0
        out[ZERO_GRAD].zero_()
        out[NO_GRAD] = None
    return out


def copies(tensors, device="cpu", dtype=torch.float32):
    """Parameters holding the tensors' values, in their layout."""
    return [torch.nn.Parameter(t.detach().to(device=device, dtype=dtype, copy=True)) for t in tensors]


def set_grads(params, gs):
    for p, g in zip(params, gs):
        p.grad = None if g is None else g.to(device=p.device, dtype=p.dtype, copy=True)
        assert p.grad is None or p.grad.stride() == p.stride()


def torch_opt(params, **kw):
    return torch.optim.Adafactor(params, eps=(EPS1, EPS2), foreach=False, **kw)


def rel(x, ref64):
    return ((x.detach().double().cpu() - ref64).abs().max() / ref64.abs().max().clamp_min(1e-300)).item()


def assert_within_bound(fused, t32, t64, cases):
    """e(fused) <= 4 * e(torch fp32) + 8 * 2**-23 per parameter and state tensor, e against fp64."""
    (pf, of), (p32, o32), (p64, o64) = fused, t32, t64
    for i, (a, b, c) in enumerate(zip(pf, p32, p64)):
        triples = [("param", a, b, c.detach())]
        triples += [(k, of.state[a][k], o32.state[b][k], o64.state[c][k]) for k in STATE_KEYS if k in o64.state[c]]
        for name, x, y32, y64 in triples:
            assert x.shape == y64.shape
            ef, et = rel(x, y64), rel(y32, y64)
            print(f"{cases[i]} {name}: e(fused) {ef:.3e} e(torch fp32) {et:.3e}")
            assert ef <= 4 * et + 8 * 2.0 ** -23, (cases[i], name, ef, et)


def check_exact_sums(device):
    gen = torch.Generator().manual_seed(11)
    ps = copies(masters(gen), device)
    before = [p.detach().clone() for p in ps]
    gs = grads(gen, ints=True)
    opt = D.FusedAdafactor(ps)
    set_grads(ps, gs)
    opt.step()
    for i, (p, g) in enumerate(zip(ps, gs)):
        if g is None:
            assert len(opt.state[p]) == 0 and torch.equal(p, before[i])
            continue
        st = {k: v.cpu() for k, v in opt.state[p].items()}
        assert st["step"].item() == 1 and not st["step"].is_cuda
        if g.dim() > 1:
            assert torch.equal(st["row_var"], (g * g).sum(-1, keepdim=True) / g.shape[-1]), CASES[i]
            assert torch.equal(st["col_var"], (g * g).sum(-2, keepdim=True) / g.shape[-2]), CASES[i]
        else:
            assert torch.equal(st["variance"], g * g), CASES[i]


def check_three_steps(device, weight_decay, maximize, d, lr):
    gen = torch.Generator().manual_seed(13)
    m = masters(gen)
    kw = dict(lr=lr, weight_decay=weight_decay, maximize=maximize, d=d)
    pf, p32, p64 = copies(m, device), copies(m), copies(m, dtype=torch.float64)
    of, o32, o64 = D.FusedAdafactor(pf, eps=(None, EPS2), **kw), torch_opt(p32, **kw), torch_opt(p64, **kw)
    for _ in range(3):
        gs = grads(gen)
        for ps, opt in ((pf, of), (p32, o32), (p64, o64)):
            set_grads(ps, gs)
            opt.step()
    assert_within_bound((pf, of), (p32, o32), (p64, o64), CASES)


def final_state(device, seed=17):
    """Parameters and state tensors after three default steps from a seeded state."""
    gen = torch.Generator().manual_seed(seed)
    ps = copies(masters(gen), device)
    opt = D.FusedAdafactor(ps, weight_decay=0.1)
    for _ in range(3):
        set_grads(ps, grads(gen))
        opt.step()
    return [p.detach() for p in ps] + [opt.state[p][k] for p in ps for k in STATE_KEYS if k in opt.state[p]]
