"""The pair-target criterion without a GPU: gs_xent_mix_fwd / gs_xent_mix_bwd on the host backend against the fp64
restatement built on ``xent_ref`` and against the torch composition in fp64 (tests/_mix_ref.py derives the
bounds), their bit identity with the one-label entries, the special rows, the metrics and the ``loss`` module."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _eval_ref as E
from tests import _mix_ref as M
from tests import _xent_ref as X

BF16 = torch.bfloat16
ALL = ("none", "mean", "sum")
SHAPES = [(Bn, K) for Bn in (1, 5, 257) for K in (1, 2, 10, 63, 65, 1000, 2049)]
DTYPES = [torch.float32, BF16, torch.float16]


@pytest.fixture(scope="module")
def lib():
    from distributed_training_amd import _lib as L

    return L.lib()


def check_shape(lib, Bn, K, dtype, eps, device=None):
    """shared with tests/test_gpu_xent_mix.py"""
    logits, a, b, lam = M.mix_case(Bn, K, dtype, seed=Bn * 1009 + K)
    assert logits.stride(0) > K  # a row stride above K, NaN in the padding
    out = M.run_xent_mix(lib, logits, a, b, lam, eps, ALL, device=device)
    M.check_xent_mix(logits, a, b, lam, eps, out)
    return logits, a, b, lam, out


@pytest.mark.parametrize("eps", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_and_gradient(lib, shape, dtype, eps):
    check_shape(lib, *shape, dtype, eps)


def check_one_label_identity(lib, device=None):
    """rows with lam == 1 or a == b: the 16-byte row and the gradient bits of gs_xent_fwd / gs_xent_bwd on label a;
    with every row such, the reduced result too.  Shared with tests/test_gpu_xent_mix.py."""
    for Bn, K, dtype in ((257, 65, BF16), (5, 2049, torch.float32), (64, 1000, torch.float16)):
        for eps in (0.0, 0.1):
            logits, a, b, lam = M.mix_case(Bn, K, dtype, seed=K)
            one = (torch.arange(Bn) % 3) != 2  # a third of the rows stay mixed
            half = torch.arange(Bn) % 2 == 0
            lam = torch.where(one & half, torch.ones(Bn), lam)
            b = torch.where(one & ~half, a, b)
            plain = X.run_xent(lib, logits, a, eps, ALL, device=device)
            mixed = M.run_xent_mix(lib, logits, a, b, lam, eps, ALL, device=device)
            same = one | (a == -100)
            assert torch.equal(mixed["rows"].view(torch.int32)[same], plain["rows"].view(torch.int32)[same])
            assert not torch.equal(mixed["rows"].view(torch.int32)[~same], plain["rows"].view(torch.int32)[~same])
            for name in ("none", "sum"):  # the mean's c is the same too: the same rows are counted
                assert M.same_bits(mixed["dz"][name][same], plain["dz"][name][same])
            assert M.same_bits(mixed["dz"]["mean"][same], plain["dz"]["mean"][same])
            # every row a one-label row
            lam_all = torch.where(half, torch.ones(Bn), lam)
            b_all = torch.where(half, b, a)
            mixed = M.run_xent_mix(lib, logits, a, b_all, lam_all, eps, ALL, device=device)
            assert torch.equal(mixed["rows"].view(torch.int32), plain["rows"].view(torch.int32))
            assert str(mixed["red"]) == str(plain["red"])
            for name in ALL:
                assert M.same_bits(mixed["dz"][name], plain["dz"][name])


def test_one_label_rows_are_the_one_label_entries_bits(lib):
    check_one_label_identity(lib)


def special_case():
    logits, a, b, lam = M.mix_case(12, 10, torch.float32, seed=6, specials=False)
    a, b, lam = a.clone(), b.clone(), lam.clone()
    b = torch.where(b == a, (a + 1) % 10, b)
    a[1] = 3  # xent_case's ignored row: counted again here
    a[2], b[3] = -100, -100  # ignore on a only, on b only
    a[4], b[4] = -100, -100  # on both
    a[5], b[6] = 10, -3  # a bad label on either side
    lam[7], lam[8] = math.nan, 1.5  # a bad weight
    a[9], b[9] = -100, 11  # ignore wins over a bad label
    return logits, a, b, lam


def check_special_rows(lib, device=None):
    logits, a, b, lam = special_case()
    acc = torch.zeros(8, dtype=torch.int64, device="cpu" if device is None else device)
    out = M.run_xent_mix(lib, logits, a, b, lam, 0.1, ALL, device=device, topk=(1, 5), acc=acc)
    M.check_xent_mix(logits, a, b, lam, 0.1, out)
    assert out["code"][[2, 3, 4, 9]].tolist() == [-1] * 4 and out["code"][[5, 6, 7, 8]].tolist() == [-2] * 4
    assert out["red"][2:] == (4, 4) and math.isnan(out["red"][0]) and math.isnan(out["red"][1])
    assert E.acc_words(acc)[:2] == [4, 4]
    for dz in out["dz"].values():
        assert not dz[2:10, :10].any() and bool(dz[[0, 1, 10, 11], :10].any(dim=1).all())
    # a NaN logit row: its loss, m, logS and gradient NaN, the reduced loss NaN, the other rows in their bounds
    logits, a, b, lam = M.mix_case(8, 10, torch.float32, seed=5, specials=False)
    a[1] = 2
    logits[3, 7] = math.nan
    out = M.run_xent_mix(lib, logits, a, b, lam, 0.1, ALL, device=device)
    M.check_xent_mix(logits, a, b, lam, 0.1, out)
    assert int(out["code"][3]) == 2 ** 31 - 1 and out["rows"][3, :3].isnan().all()
    assert math.isnan(out["red"][0]) and math.isnan(out["red"][1]) and out["red"][2:] == (8, 0)
    for dz in out["dz"].values():
        assert dz[3, :10].isnan().all() and not dz[[0, 1, 2, 4, 5, 6, 7], :10].isnan().any()
    # all rows skipped
    a[:] = -100
    out = M.run_xent_mix(lib, logits, a, b, lam, 0.1, ALL, device=device)
    M.check_xent_mix(logits, a, b, lam, 0.1, out)
    assert out["red"][0] == 0.0 and math.isnan(out["red"][1]) and out["red"][2:] == (0, 0)
    assert not any(dz[:, :10].any() for dz in out["dz"].values())


def test_special_rows(lib):
    check_special_rows(lib)


def test_twice_gives_identical_bits(lib):
    logits, a, b, lam = M.mix_case(64, 65, BF16, seed=12)
    x = M.run_xent_mix(lib, logits, a, b, lam, 0.1, ALL)
    y = M.run_xent_mix(lib, logits, a, b, lam, 0.1, ALL)
    assert torch.equal(x["rows"].view(torch.int32), y["rows"].view(torch.int32)) and str(x["red"]) == str(y["red"])
    assert all(M.same_bits(x["dz"][k], y["dz"][k]) for k in ALL)


def check_metrics(lib, device=None):
    """the accumulator: counts as Metrics.update on the dominant labels, the loss word within the derived bound of
    the fp64 unsmoothed mixed loss.  Shared with tests/test_gpu_xent_mix.py."""
    import distributed_training_amd as D

    dev = torch.device("cpu") if device is None else device
    for eps in (0.0, 0.1):
        acc = torch.zeros(8, dtype=torch.int64, device=dev)
        ref = D.Metrics(topk=E.TOPK, device=dev)
        want_loss = bound = 0.0
        for Bn, K in ((64, 10), (5, 65), (257, 7)):
            logits, a, b, lam = M.mix_case(Bn, K, BF16, seed=Bn + K)
            if Bn > 2:
                b[2] = -100  # skipped through b alone
            M.run_xent_mix(lib, logits, a, b, lam, eps, (), device=device, topk=E.TOPK, acc=acc)
            dominant = torch.where(lam >= 0.5, a, b)
            dominant = torch.where((a == -100) | (b == -100), torch.full_like(a, -100), dominant)
            ref.update(logits.contiguous().to(dev), dominant.to(dev))
            r0 = M.xent_mix_ref(E.values64(logits), a.numpy(), b.numpy(), lam.numpy(), 0.0, BF16)
            want_loss += r0["total"]
            bound += r0["total_bound"]
        got, want = E.acc_words(acc), ref.compute()
        assert got[0] == want["n"] == 64 + 5 + 257 - 6 and got[1] == 0  # rows 1 and 2 of each batch are skipped
        assert got[3:] == [want[f"correct{k}"] for k in E.TOPK]
        assert abs(got[2] - want_loss) <= bound


def test_metrics(lib):
    check_metrics(lib)


# ---- the argument checks ---------------------------------------------------------------------------------------
A = 0x7F0000001000  # made-up addresses, never dereferenced


@pytest.mark.parametrize("bad", [dict(lb=None), dict(lam=None), dict(lb=A + 0x60004), dict(lam=A + 0x70002), dict(K=0),
                                 dict(eps=1.5), dict(stride=9), dict(la=None)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_entries_reject(lib, bad):
    from distributed_training_amd import _lib as L

    p = dict(la=A + 0x10000, lb=A + 0x60000, lam=A + 0x70000, K=10, eps=0.1, stride=10)
    p.update(bad)
    rc = lib.gs_xent_mix_fwd(L.GS_DEV_HOST, A, L.GS_F32, p["la"], p["lb"], p["lam"], 4, p["K"], p["stride"], -100,
                             p["eps"], A + 0x20000, A + 0x28000, None, 0, None, None)
    assert rc == L.GS_EINVAL and lib.gs_last_error()
    rc = lib.gs_xent_mix_bwd(L.GS_DEV_HOST, A, L.GS_F32, p["la"], p["lb"], p["lam"], 4, p["K"], p["stride"], -100,
                             p["eps"], 1, A + 0x20000, A + 0x28000, A + 0x50000, A + 0x40000, 10, None)
    assert rc == L.GS_EINVAL and lib.gs_last_error()


def test_empty_batch(lib):
    from distributed_training_amd import _lib as L

    red = torch.full((4,), 7.0)
    rc = lib.gs_xent_mix_fwd(L.GS_DEV_HOST, None, L.GS_F32, None, None, None, 0, 10, 10, -100, 0.1, None,
                             red.data_ptr(), None, 0, None, None)
    assert rc == 0, lib.gs_last_error()
    assert float(red[0]) == 0.0 and math.isnan(float(red[1])) and red.view(torch.int32)[2:].tolist() == [0, 0]
    assert lib.gs_xent_mix_bwd(L.GS_DEV_HOST, None, L.GS_F32, None, None, None, 0, 10, 10, -100, 0.1, 1, None, None,
                               None, None, 10, None) == 0


# ---- the module ------------------------------------------------------------------------------------------------
def composition(z, t, eps, reduction="mean", ignore_index=-100):
    la = F.cross_entropy(z, t.labels_a, reduction="none", label_smoothing=eps, ignore_index=ignore_index)
    lb = F.cross_entropy(z, t.labels_b, reduction="none", label_smoothing=eps, ignore_index=ignore_index)
    on = (t.labels_a != ignore_index) & (t.labels_b != ignore_index)
    rows = torch.where(on, t.lam.to(z.dtype) * la + (1 - t.lam.to(z.dtype)) * lb, torch.zeros_like(la))
    return rows if reduction == "none" else rows.sum() if reduction == "sum" else rows.sum() / on.sum()


def check_module(dev):
    """shared with tests/test_gpu_xent_mix.py"""
    import distributed_training_amd as D
    from distributed_training_amd import loss as LS

    gen = torch.Generator().manual_seed(3)
    x = torch.randn(12, 6, generator=gen)
    a = torch.randint(0, 10, (12,), generator=gen)
    b = torch.randint(0, 10, (12,), generator=gen)
    lam = torch.rand(12, generator=gen)
    lam[2], b[3], a[4] = 1.0, a[3], -100
    t = D.MixedTarget(a.to(dev), b.to(dev), lam.to(dev))
    t64 = D.MixedTarget(a, b, lam.double())
    lin64 = torch.nn.Linear(6, 10).double()
    for dtype in (torch.float32, BF16):
        for reduction in ALL:
            lin = torch.nn.Linear(6, 10).to(dev)
            with torch.no_grad():
                lin.weight.copy_(lin64.weight)
                lin.bias.copy_(lin64.bias)
            z = lin(x.to(dev)).to(dtype)
            z.retain_grad()
            loss = D.CrossEntropyLoss(reduction=reduction, label_smoothing=0.1)(z, t)
            assert LS.last_path == "fused" and loss.dtype == torch.float32
            assert loss.shape == ((12,) if reduction == "none" else ())
            loss.sum().backward()
            # the torch composition in fp64 on the same (rounded) logits, through the same linear model
            z64 = z.detach().double().cpu().requires_grad_()
            want = composition(z64, t64, 0.1, reduction)
            want.sum().backward()
            ref = M.xent_mix_ref(z64.detach().numpy(), a.numpy(), b.numpy(), lam.numpy(), 0.1, dtype)
            g = np.float64(1.0) if reduction != "none" else np.ones(12)
            _, bound = ref["grad"](reduction, g)
            de = abs(float(np.float32(0.1)) - 0.1)
            X._close(z.grad.double().cpu().numpy(), z64.grad.numpy(), bound + 2 * de, "d loss / d logits")
            lb = ref["loss_bound"] + de * 40  # |smooth - nll| is far below 40 for these logits
            if reduction == "none":
                X._close(loss.detach().double().cpu().numpy(), want.detach().numpy(), lb, "loss")
            else:
                n = 1 if reduction == "sum" else ref["counted"]
                w = float(want.detach())
                X._close([float(loss.detach())], [w], [(lb[ref["on"]].sum() + M.U32 * abs(w) * n) / n], "loss")
            # the parameters' gradients are the chain rule's on the logits' gradient
            zg = z.grad.float()
            assert torch.allclose(lin.weight.grad, zg.t() @ x.to(dev), rtol=1e-5, atol=1e-6)
            assert torch.allclose(lin.bias.grad, zg.sum(0), rtol=1e-5, atol=1e-6)
    z = torch.randn(12, 10, generator=gen).to(dev).requires_grad_()
    old = os.environ.get("GSYNC_FUSED_LOSS")
    os.environ["GSYNC_FUSED_LOSS"] = "0"
    try:
        for reduction in ALL:
            got = D.cross_entropy(z, t, reduction=reduction, label_smoothing=0.1)
            assert LS.last_path == "torch" and torch.equal(got, composition(z, t, 0.1, reduction))
        m, ref = D.Metrics(topk=(1,), device=dev), D.Metrics(topk=(1,), device=dev)
        D.CrossEntropyLoss(metrics=m)(z, t)
        dominant = torch.where(t.lam >= 0.5, t.labels_a, t.labels_b)
        ref.update(z.detach(), torch.where(t.labels_a == -100, t.labels_a, dominant))
        assert LS.last_path == "torch" and m.compute() == ref.compute() and m.compute()["n"] == 11
    finally:
        if old is None:
            del os.environ["GSYNC_FUSED_LOSS"]
        else:
            os.environ["GSYNC_FUSED_LOSS"] = old
    # anything that is not fusable is the torch composition too
    w = torch.rand(10, generator=gen).to(dev)
    D.cross_entropy(z, t, weight=w)
    assert LS.last_path == "torch"
    D.cross_entropy(z, D.MixedTarget(t.labels_a, t.labels_b, t.lam.double()))
    assert LS.last_path == "torch"
    # metrics on the fused path: the dominant labels' counts
    m, ref = D.Metrics(topk=(1, 5), device=dev), D.Metrics(topk=(1, 5), device=dev)
    crit = D.CrossEntropyLoss(label_smoothing=0.1, metrics=m)
    crit(z, t)
    assert LS.last_path == "fused"
    ref.update(z.detach(), torch.where(t.labels_a == -100, t.labels_a, dominant))
    got, want = m.compute(), ref.compute()
    assert (got["n"], got["correct1"], got["correct5"]) == (want["n"], want["correct1"], want["correct5"]) and got["n"] == 11
    # with every row a one-label row the criterion is bit for bit the one-label criterion
    ones = D.MixedTarget(t.labels_a, t.labels_b, torch.ones_like(t.lam))
    assert M.same_bits(D.cross_entropy(z, ones, label_smoothing=0.1).detach(),
                       D.cross_entropy(z, t.labels_a, label_smoothing=0.1).detach())


def test_module():
    check_module(torch.device("cpu"))


def test_example_trainer_with_mixing():
    """examples/ddp_train.py --mixup / --cutmix: the loader's MixedTarget reaches the criterion on two gloo ranks"""
    import subprocess
    import sys

    from tests._dist_util import free_port

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_PORT=str(free_port()), OMP_NUM_THREADS="1")
    cmd = [sys.executable, os.path.join(repo, "examples", "ddp_train.py"), "--device", "cpu", "--world-size", "2",
           "--fused-loss", "--label-smoothing", "0.1", "--mixup", "0.4", "--cutmix", "1.0", "--mix-prob", "0.9",
           "--max-steps", "1", "--epochs", "1", "--batch-size", "4"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("epoch 1/1")]
    assert len(line) == 1, out.stdout
    words = line[0].split()
    n, loss, top1 = int(words[words.index("n") + 1]), float(words[words.index("loss") + 1]), float(words[-1])
    assert n == 2 * 1 * 4 and math.isfinite(loss) and loss > 0 and 0.0 <= top1 <= 1.0
