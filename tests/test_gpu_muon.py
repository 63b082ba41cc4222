"""Muon on the GPU.  The three Newton-Schulz stages alone, on small-integer workspaces
where every fp32 partial sum is exact (any fragment-layout, tile-mapping, mirror, K-tail
or padding error is a wrong integer), then FusedMuon's whole step against the fp64
restatement of torch's formulae (tests/_muon_ref.py)."""
import pytest
import torch

import distributed_training_amd as D
from distributed_training_amd.multi_tensor import TensorListPlan
from tests import _muon_ref as R

pytestmark = pytest.mark.gpu


def _dims(shape):
    dims = tuple(int(v) for v in shape[3:].split(",")) if isinstance(shape, str) else shape
    numel = 1
    for v in dims:
        numel *= v
    return dims[0], numel // dims[0]


@pytest.fixture(scope="module")
def stages(cuda_device):
    """One plan over SHAPES, its X0 / Agram / Bpoly regions filled with integers of
    {-2..2} (Agram symmetric), and the three stages run once each: (layout, workspace
    before, workspace after Gram, after Poly, after Apply), on the CPU as fp64."""
    ab = [_dims(s) for s in R.SHAPES]
    plan = TensorListPlan([a * b for a, b in ab], cuda_device)
    lay = plan.muon_layout([a for a, _ in ab])
    gen = torch.Generator().manual_seed(7)
    ws = torch.zeros(lay["total"], dtype=torch.float64)
    for t in lay["tensors"]:
        m, n, ldx, lda = t["m"], t["n"], t["ldx"], t["lda"]
        ws[t["x0"]:t["x0"] + lda * ldx].view(lda, ldx)[:m, :n] = torch.randint(-2, 3, (m, n), generator=gen).double()
        s = torch.randint(-2, 3, (m, m), generator=gen).double().tril()
        ws[t["agram"]:t["agram"] + lda * lda].view(lda, lda)[:m, :m] = s + s.T - torch.diag(s.diagonal())
        ws[t["bpoly"]:t["bpoly"] + lda * lda].view(lda, lda)[:m, :m] = torch.randint(-2, 3, (m, m), generator=gen).double()
    out = []
    for stage in ("gram", "poly", "apply"):
        dev = ws.to(torch.bfloat16).to(cuda_device)
        if stage == "gram":
            plan.muon_gram(dev, 0)
        elif stage == "poly":
            plan.muon_poly(dev, 2.0, 0.5)
        else:
            plan.muon_apply(dev, 0, -1.0)
        out.append(dev.double().cpu())
    return (lay, ws, *out)


def _region(ws, off, rows, ld):
    return ws[off:off + rows * ld].view(rows, ld)


@pytest.mark.parametrize("t", range(len(R.SHAPES)), ids=[str(s) for s in R.SHAPES])
def test_stages_exact(stages, t):
    lay, ws, gram, poly, apply = stages
    d = lay["tensors"][t]
    ldx, lda = d["ldx"], d["lda"]
    x = _region(ws, d["x0"], lda, ldx)  # padded: the expected outputs carry the zero padding
    a = _region(ws, d["agram"], lda, lda)
    b = _region(ws, d["bpoly"], lda, lda)

    def bf16(v):
        return v.float().to(torch.bfloat16).double()

    assert torch.equal(_region(gram, d["agram"], lda, lda), bf16(x @ x.T))
    assert torch.equal(_region(poly, d["bpoly"], lda, lda), bf16(2.0 * a + 0.5 * (a @ a)))
    assert torch.equal(_region(apply, d["x1"], lda, ldx), bf16(b @ x - x))
    # a stage writes its own output and nothing else
    for after, key in ((gram, "agram"), (poly, "bpoly"), (apply, "x1")):
        keep = torch.ones_like(ws, dtype=torch.bool)
        for u in lay["tensors"]:
            rows = u["lda"] * (u["ldx"] if key == "x1" else u["lda"])
            keep[u[key]:u[key] + rows] = False
        assert torch.equal(after[keep], ws[keep])


def _run(device, gdt, nesterov, adjust, ns_steps, steps=2, lr=0.02, wd=0.1, momentum=0.95, eps=1e-7):
    """FusedMuon over SHAPES for ``steps`` steps beside the fp64 reference, which takes the
    fused O of each step for its own p (so p pins the update pass to fp32 rounding and O is
    judged on its own).  Returns per step and tensor (fused O, u) and the end state."""
    gen = torch.Generator().manual_seed(11)
    ps = [torch.nn.Parameter(R.make(s, device, gen)) for s in R.SHAPES]
    if gdt != torch.float32:
        for p in ps:
            p.grad_dtype = None  # torch 2.10: a grad of another dtype needs this
    opt = D.FusedMuon(ps, lr=lr, weight_decay=wd, momentum=momentum, nesterov=nesterov, eps=eps, ns_steps=ns_steps,
                      adjust_lr_fn=adjust)
    p64 = [R.matrix(p) for p in ps]
    b64 = [torch.zeros_like(m) for m in p64]
    seen = []
    for _ in range(steps):
        us = []
        for i, (p, s) in enumerate(zip(ps, R.SHAPES)):
            p.grad = R.make(s, device, gen, gdt)
            b64[i], u = R.direction(R.matrix(p.grad), b64[i], momentum, nesterov)
            us.append(u)
        opt.step()
        plan = opt._plans.plans()[0]
        for i, u in enumerate(us):
            A, B = u.shape
            o = R.fused_x(plan, plan._muon_space, i, ns_steps % 2, A, B)
            p64[i] = p64[i] * (1 - lr * wd) - R.adjusted_lr(lr, adjust, A, B) * o
            seen.append((i, o, u))
    return opt, ps, p64, b64, seen


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("nesterov,adjust", [(True, None), (False, "match_rms_adamw")])
def test_step_against_fp64(cuda_device, gdt, nesterov, adjust):
    opt, ps, p64, b64, seen = _run(cuda_device, gdt, nesterov, adjust, ns_steps=5)
    for p, pr, br in zip(ps, p64, b64):
        # fp32 rounding: a few ulps of values of order 1 (atol for the elements near zero)
        torch.testing.assert_close(R.matrix(opt.state[p]["momentum_buffer"]), br, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(R.matrix(p), pr, rtol=1e-6, atol=1e-6)
    for i, o, u in seen:
        ref = R.newton_schulz(u, 5, 1e-7)
        err, terr = R.rel_err(o, ref), R.torch_ns_err(u, 5, 1e-7, cuda_device)
        print(f"muon ratio {R.SHAPES[i]} fused {err:.4f} torch {terr:.4f} ratio {err / terr:.3f}")
        assert err <= 1.5 * terr, (R.SHAPES[i], err, terr)


def test_ns_steps_zero_is_the_scaled_direction(cuda_device):
    """O = bf16(u * s): prep, the transpose and the update without GEMM noise."""
    lr = 0.02
    opt, ps, _, _, seen = _run(cuda_device, torch.float32, True, None, ns_steps=0, steps=1, lr=lr, wd=0.0)
    for (i, o, u), p in zip(seen, ps):
        ref = u / u.norm().clamp(min=1e-7)
        assert bool(((o - ref).abs() <= 2.0 ** -8 * ref.abs()).all()), R.SHAPES[i]
    # and p itself, from its own start: p0 - adj*O within bf16 rounding of the update
    gen = torch.Generator().manual_seed(11)
    for (i, o, u), p in zip(seen, ps):
        p0 = R.matrix(R.make(R.SHAPES[i], "cpu", gen))
        A, B = u.shape
        adj = R.adjusted_lr(lr, None, A, B)
        ref = u / u.norm().clamp(min=1e-7)
        bound = 2.0 ** -8 * adj * ref.abs() + 4 * 2.0 ** -24 * p0.abs()
        assert bool(((R.matrix(p) - (p0 - adj * ref)).abs() <= bound).all()), R.SHAPES[i]


def test_same_state_same_bits(cuda_device):
    a = _run(cuda_device, torch.float32, True, None, ns_steps=5)[1]
    b = _run(cuda_device, torch.float32, True, None, ns_steps=5)[1]
    for x, y in zip(a, b):
        assert torch.equal(x, y)
