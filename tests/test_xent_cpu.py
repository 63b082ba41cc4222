"""The training criterion without a GPU: gs_xent_fwd / gs_xent_bwd on the host backend against a numpy fp64
restatement and against ``F.cross_entropy`` in fp64, the argument checks, and the ``loss`` module (paths,
dtypes, metrics, gloo, the example trainer).

The bounds (u = 2^-24, L = ceil(log2 K); tests/_xent_ref.py computes them).

The unsmoothed loss nll = (m - z_y) + logf(S): test_eval_cpu.py derives
  |nll - truth| <= (L + 10) u (1 + |m - z_y| + |log S|) = b_nll,
and from the same steps the error of logS alone is at most (L + 4) u from S, 2 u |log S| + u from logf:
  |logS - truth| <= (L + 5) u + 2 u |log S|.

The smoothed loss = (1 - eps) * nll + eps * smooth, smooth = (m + logS) - T / (float)K:
  * m + logS: the error of logS and one rounding, u |m + log S|;
  * T = sum z_j on the balanced tree: at most L roundings on a path, each relative u of a partial sum whose
    magnitude is at most sum |z_j|: L u sum |z_j|; the division rounds once more (K <= 2^24 converts exactly):
    T / K is off by at most (L + 1) u sum |z_j| / K; the subtraction rounds once, u |smooth|;
  so |smooth - truth| <= u ((L + 5) + 3 |log S| + |m + log S| + (L + 2) sum |z_j| / K + |smooth|) = b_smooth
  (one |log S| and one sum |z_j| / K of slack for the second-order terms);
  * 1 - eps rounds once (u |nll| after the product), each product once and the final add once, each relative u
    of a value no larger than (1 - eps) |nll| + eps |smooth|;
  |loss - truth| <= (1 - eps) b_nll + eps b_smooth + 4 u ((1 - eps) |nll| + eps |smooth|).
eps is the fp32 value the library receives, in the restatement too; against torch, which keeps the double,
the loss may move by |eps32 - eps| |smooth - nll| and a gradient element by 2 |eps32 - eps| |c|.
A loss that is +inf (a -inf logit under label smoothing) or NaN must be exactly that.
The reduced loss is the fp64 sum of the fp32 losses (exact to 2^-53 relative, ignored) rounded once to fp32:
  |loss_sum - sum truth| <= sum of the rows' bounds + u |sum|, and the mean likewise after the division.

A gradient element dz_j = c * (p_j - q_j), p_j = expf((z_j - m) - logS):
  * the argument: the error of logS, the rounding of z_j - m and of the second subtraction; expf adds 2 ulp.
    The term is p_j (L + 8 + 2 |log S| + |z_j - m|) u: (L + 5) + 2 |log S| from logS, 2 from expf, 1 for the
    second-order terms, and |z_j - m| for the two subtractions.  (Counting both subtractions at their worst
    at once would give 3 |log S| + 2 |z_j - m|; the expression used here is the tighter one, so it asks more
    of the library, not less.)  p_j = 0 (a -inf logit) is exact.
  * q_off = eps / K rounds once, q_on = (1 - eps) + q_off three times: at most 3 u q_j;
  * c = g / (float)counted rounds once, the subtraction once, the product once: 3 u |c| |p_j - q_j|;
  * the one rounding to the logits' dtype: u_out (|dz_j| + the error so far), u_out = 2^-24, 2^-8 (bf16) or
    2^-11 (fp16, plus 2^-25 absolute below its normal range).
  |dz_j - truth| <= |c| (p_j (L + 8 + 2 |log S| + |z_j - m|) u + 3 u q_j + 3 u |p_j - q_j|) + the rounding.
In exact arithmetic a counted row's gradient sums to c (1 - sum q_j) = 0, so the sum of the computed row is at
most the sum of its elements' bounds.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from tests import _eval_ref as E
from tests import _xent_ref as X
from tests._dist_util import free_port, init_pg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    from distributed_training_amd import _lib as L

    return L.lib()


# ---- the two entries on the host backend -----------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [1, 2, 7, 8, 65, 1000])
@pytest.mark.parametrize("Bn", [1, 3, 64, 257])
def test_loss_and_gradient(lib, Bn, K, dtype, eps):
    logits, labels = X.xent_case(Bn, K, dtype, seed=Bn * 1009 + K)
    assert logits.stride(0) > K
    out = X.run_xent(lib, logits, labels, eps, ("none", "mean", "sum"))
    X.check_xent(logits, labels, eps, out)


# row strides that are multiples of 16 bytes: no padding, a tail after the last whole vector, a row shorter than a
# vector, a row of more than one 2048-element chunk (with and without an aligned stride)
LAYOUTS = [(64, 1000, BF16, 0), (3, 8, BF16, 0), (3, 8, torch.float32, 0), (5, 65, BF16, 7), (5, 65, torch.float32, 7),
           (3, 7, BF16, 1), (3, 2500, BF16, 4), (3, 2500, torch.float32, 3), (2, 33, torch.float16, 7)]


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("case", LAYOUTS, ids=lambda c: f"{c[0]}x{c[1]}-{str(c[2])[6:]}-pad{c[3]}")
def test_layouts(lib, case, eps):
    Bn, K, dtype, pad = case
    logits, labels = X.xent_case(Bn, K, dtype, seed=K + pad, pad=pad)
    out = X.run_xent(lib, logits, labels, eps, ("none", "mean", "sum"))
    X.check_xent(logits, labels, eps, out)


def test_fp16_logits(lib):
    logits, labels = X.xent_case(9, 33, torch.float16, seed=9)
    out = X.run_xent(lib, logits, labels, 0.1, ("none", "mean", "sum"))
    X.check_xent(logits, labels, 0.1, out)


def masked_case():
    logits, labels = X.xent_case(5, 7, torch.float32, seed=21, specials=False)
    labels[3] = 2
    logits[3, 5] = -math.inf
    return logits, labels


def test_masked_class(lib):
    logits, labels = masked_case()
    out = X.run_xent(lib, logits, labels, 0.0, ("none", "mean", "sum"))
    X.check_xent(logits, labels, 0.0, out)
    assert math.isfinite(float(out["rows"][3, 0])) and math.isfinite(out["red"][1])
    for dz in out["dz"].values():
        assert float(dz[3, 5]) == 0.0
    # with label smoothing the masked class is a target: the loss is +inf, as torch's
    out = X.run_xent(lib, logits, labels, 0.1, ("none", "mean", "sum"))
    X.check_xent(logits, labels, 0.1, out, against_torch=False)
    want = F.cross_entropy(logits.double(), labels, reduction="none", label_smoothing=0.1)
    assert float(want[3]) == math.inf == float(out["rows"][3, 0])
    assert out["red"][0] == math.inf and out["red"][1] == math.inf


def test_nan_row(lib):
    logits, labels = X.xent_case(8, 10, torch.float32, seed=5, specials=False)
    logits[3, 7] = math.nan
    for eps in (0.0, 0.1):
        out = X.run_xent(lib, logits, labels, eps, ("none", "mean", "sum"))
        X.check_xent(logits, labels, eps, out)  # the other rows within their bounds
        assert int(out["code"][3]) == 2 ** 31 - 1 and out["rows"][3, :3].isnan().all()
        assert math.isnan(out["red"][0]) and math.isnan(out["red"][1]) and out["red"][2:] == (8, 0)
        for dz in out["dz"].values():
            assert dz[3, :10].isnan().all() and not dz[[0, 1, 2, 4, 5, 6, 7], :10].isnan().any()


def test_bad_label(lib):
    logits, labels = X.xent_case(6, 10, torch.float32, seed=6, specials=False)
    labels[2] = 10
    labels[4] = -3
    acc = torch.zeros(8, dtype=torch.int64)
    out = X.run_xent(lib, logits, labels, 0.1, ("none", "mean", "sum"), topk=(1, 5), acc=acc)
    X.check_xent(logits, labels, 0.1, out)
    assert out["red"][2:] == (4, 2) and math.isnan(out["red"][0]) and math.isnan(out["red"][1])
    assert E.acc_words(acc)[:2] == [4, 2]
    assert out["code"][[2, 4]].tolist() == [-2, -2]
    for dz in out["dz"].values():
        assert not dz[[2, 4], :10].any()


def test_all_rows_ignored(lib):
    logits, labels = X.xent_case(5, 9, BF16, seed=7)
    labels[:] = -100
    out = X.run_xent(lib, logits, labels, 0.1, ("none", "mean", "sum"))
    X.check_xent(logits, labels, 0.1, out)
    assert out["red"][0] == 0.0 and math.isnan(out["red"][1]) and out["red"][2:] == (0, 0)
    for dz in out["dz"].values():
        assert not dz[:, :9].any()


def test_one_class(lib):
    for dtype in (torch.float32, BF16):
        logits, labels = X.xent_case(4, 1, dtype, seed=8, specials=False)
        for eps in (0.0, 0.1):
            out = X.run_xent(lib, logits, labels, eps, ("none", "mean", "sum"))
            assert not out["rows"][:, 0].any() and out["red"] == (0.0, 0.0, 4, 0)
            for dz in out["dz"].values():
                assert not dz[:, :1].any()


def test_empty_batch(lib):
    from distributed_training_amd import _lib as L

    red = torch.full((4,), 7.0)
    acc = torch.full((8,), 3, dtype=torch.int64)
    rc = lib.gs_xent_fwd(L.GS_DEV_HOST, None, L.GS_F32, None, 0, 10, 10, -100, 0.1, None, red.data_ptr(),
                         L.i32_array((1,)), 1, acc.data_ptr(), None)
    assert rc == 0, lib.gs_last_error()
    assert float(red[0]) == 0.0 and math.isnan(float(red[1])) and red.view(torch.int32)[2:].tolist() == [0, 0]
    assert acc.tolist() == [3] * 8
    assert lib.gs_xent_bwd(L.GS_DEV_HOST, None, L.GS_F32, None, 0, 10, 10, -100, 0.1, 1, None, None, None, None, 10,
                           None) == 0


def test_twice_gives_identical_bits(lib):
    logits, labels = X.xent_case(64, 65, BF16, seed=12)
    a = X.run_xent(lib, logits, labels, 0.1, ("none", "mean", "sum"))
    b = X.run_xent(lib, logits, labels, 0.1, ("none", "mean", "sum"))
    assert torch.equal(a["rows"].view(torch.int32), b["rows"].view(torch.int32))
    assert str(a["red"]) == str(b["red"])
    for k in a["dz"]:
        assert torch.equal(a["dz"][k].view(torch.int16), b["dz"][k].view(torch.int16))


def check_accumulator(lib, device=None):
    """with acc, the accumulator equals gs_eval_accumulate's on the same batch (host backend): counts exactly, the
    fp64 sum of the unsmoothed losses within the sum of the rows' bounds (both sides are within them of fp64)"""
    dev = torch.device("cpu") if device is None else device
    for eps in (0.0, 0.1):
        acc = torch.zeros(8, dtype=torch.int64, device=dev)
        want = torch.zeros(8, dtype=torch.int64)
        bound = 0.0
        for Bn, K in ((64, 10), (5, 65), (257, 7)):
            logits, labels = X.xent_case(Bn, K, BF16, seed=Bn + K)
            X.run_xent(lib, logits, labels, eps, (), device=device, topk=E.TOPK, acc=acc)
            E.run_accumulate(lib, logits, labels, Bn, acc=want)
            ref = X.xent_ref(E.values64(logits), labels.numpy(), eps, BF16)
            bound += float(ref["nll_bound"][ref["on"]].sum())
        got, w = E.acc_words(acc), E.acc_words(want)
        assert got[:2] == w[:2] and got[3:] == w[3:]
        assert abs(got[2] - w[2]) <= 2 * bound
        if device is None:
            assert got[2] == w[2]  # the host backend forms the same expression on the same tree


def test_accumulator_equals_eval_accumulate(lib):
    check_accumulator(lib)


A = 0x7F0000001000  # made-up addresses, never dereferenced


def _einval(lib, rc):
    from distributed_training_amd import _lib as L

    assert rc == L.GS_EINVAL, rc
    assert lib.gs_last_error()


FWD_BAD = [dict(kind=7), dict(dtype=4), dict(B=-1), dict(K=0), dict(K=2 ** 30 + 1), dict(stride=9), dict(eps=-0.1),
           dict(eps=1.5), dict(eps=math.nan), dict(n_topk=5), dict(topk=(0, 1)), dict(logits=None), dict(labels=None),
           dict(rows=None), dict(red=None), dict(red=A + 8), dict(rows=A + 8), dict(acc=A + 4), dict(logits=A + 2),
           dict(labels=A + 4)]


@pytest.mark.parametrize("bad", FWD_BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_fwd_rejects(lib, bad):
    from distributed_training_amd import _lib as L

    a = dict(kind=L.GS_DEV_HOST, logits=A, dtype=L.GS_F32, labels=A + 0x10000, B=4, K=10, stride=10, ign=-100, eps=0.1,
             rows=A + 0x20000, red=A + 0x28000, topk=(1, 5), n_topk=None, acc=A + 0x30000)
    a.update(bad)
    n_topk = len(a["topk"]) if a["n_topk"] is None else a["n_topk"]
    _einval(lib, lib.gs_xent_fwd(a["kind"], a["logits"], a["dtype"], a["labels"], a["B"], a["K"], a["stride"], a["ign"],
                                 a["eps"], a["rows"], a["red"], L.i32_array(a["topk"]), n_topk, a["acc"], None))


BWD_BAD = [dict(kind=7), dict(dtype=4), dict(B=-1), dict(K=0), dict(K=2 ** 30 + 1), dict(stride=9), dict(dstride=9),
           dict(eps=-0.1), dict(eps=1.5), dict(reduction=3), dict(reduction=-1), dict(logits=None), dict(labels=None),
           dict(rows=None), dict(red=None), dict(g=None), dict(dz=None), dict(red=A + 8), dict(rows=A + 8),
           dict(logits=A + 2), dict(dz=A + 0x40002), dict(g=A + 0x50002), dict(dz=A), dict(dz=A + 40),
           dict(dz=A - 40)]


@pytest.mark.parametrize("bad", BWD_BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bwd_rejects(lib, bad):
    from distributed_training_amd import _lib as L

    a = dict(kind=L.GS_DEV_HOST, logits=A, dtype=L.GS_F32, labels=A + 0x10000, B=4, K=10, stride=10, ign=-100, eps=0.1,
             reduction=1, rows=A + 0x20000, red=A + 0x28000, g=A + 0x50000, dz=A + 0x40000, dstride=10)
    a.update(bad)
    _einval(lib, lib.gs_xent_bwd(a["kind"], a["logits"], a["dtype"], a["labels"], a["B"], a["K"], a["stride"], a["ign"],
                                 a["eps"], a["reduction"], a["rows"], a["red"], a["g"], a["dz"], a["dstride"], None))


# ---- the module -------------------------------------------------------------------------------------------
def check_module(dev):
    """the module's contract on ``dev``; shared with tests/test_gpu_xent.py"""
    import distributed_training_amd as D
    from distributed_training_amd import loss as LS

    gen = torch.Generator().manual_seed(3)
    z32 = (torch.randn(12, 10, generator=gen) * 3)
    y = torch.randint(0, 10, (12,), generator=gen)
    y[4] = -100
    yd = y.to(dev)
    for dtype in (torch.float32, BF16, torch.float16):
        for reduction in ("none", "mean", "sum"):
            z = z32.to(dtype).to(dev).clone().requires_grad_()
            crit = D.CrossEntropyLoss(reduction=reduction, label_smoothing=0.1)
            loss = crit(z, yd)
            assert LS.last_path == "fused"
            assert loss.dtype == torch.float32 and loss.shape == ((12,) if reduction == "none" else ())
            loss.sum().backward()
            assert z.grad.dtype == dtype and z.grad.shape == z.shape
            want = F.cross_entropy(z.detach().double().cpu(), y, reduction=reduction, label_smoothing=0.1)
            assert torch.allclose(loss.detach().double().cpu(), want, rtol=1e-5, atol=1e-5)
    # each fallback computes exactly what F.cross_entropy does
    z = z32.to(dev).clone().requires_grad_()
    w = torch.rand(10, generator=gen).to(dev)
    soft = torch.softmax(torch.randn(12, 10, generator=gen), 1).to(dev)
    z4 = torch.randn(2, 10, 3, 3, generator=gen).to(dev)
    y4 = torch.randint(0, 10, (2, 3, 3), generator=gen).to(dev)
    for kw, args in ((dict(weight=w), (z, yd)), (dict(), (z, soft)), (dict(), (z4, y4)),
                     (dict(size_average=False), (z, yd)), (dict(reduce=False), (z, yd)),
                     (dict(label_smoothing=0.1), (z.double(), yd))):
        got = D.CrossEntropyLoss(**kw)(*args)
        assert LS.last_path == "torch", kw
        assert torch.equal(got, torch.nn.CrossEntropyLoss(**kw)(*args))
        assert torch.equal(D.cross_entropy(*args, **kw), F.cross_entropy(*args, **kw))
    old = os.environ.get("GSYNC_FUSED_LOSS")
    os.environ["GSYNC_FUSED_LOSS"] = "0"
    try:
        got = D.CrossEntropyLoss(label_smoothing=0.1)(z, yd)
        assert LS.last_path == "torch" and torch.equal(got, F.cross_entropy(z, yd, label_smoothing=0.1))
    finally:
        if old is None:
            del os.environ["GSYNC_FUSED_LOSS"]
        else:
            os.environ["GSYNC_FUSED_LOSS"] = old
    D.CrossEntropyLoss()(z, yd)
    assert LS.last_path == "fused"
    # without grad mode nothing is saved
    packed = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: packed.append(1) or t, lambda t: t):
        with torch.no_grad():
            loss = D.CrossEntropyLoss()(z, yd)
        assert not packed and not loss.requires_grad and loss.grad_fn is None
        loss = D.CrossEntropyLoss()(z.detach(), yd)
        assert not packed and not loss.requires_grad
        loss = D.CrossEntropyLoss()(z, yd)
        assert packed and loss.requires_grad
    # a loss scaled by 2^5 (the ColossalAI shim's initial loss scale): fp32 gradients are bitwise 32x
    for reduction in ("mean", "sum", "none"):
        grads = []
        for scale in (1.0, 32.0):
            zz = z32.to(dev).clone().requires_grad_()
            (D.cross_entropy(zz, yd, reduction=reduction, label_smoothing=0.1).sum() * scale).backward()
            grads.append(zz.grad)
        assert torch.equal((grads[0] * 32).view(torch.int32), grads[1].view(torch.int32))
    # metrics: three batches through the criterion in training mode == Metrics.update on the same batches
    for eps in (0.0, 0.1):
        m, ref = D.Metrics(topk=(1, 5), device=dev), D.Metrics(topk=(1, 5), device=dev)
        crit = D.CrossEntropyLoss(label_smoothing=eps, metrics=m)
        for b in range(3):
            zb = (torch.randn(12, 10, generator=gen) * 3).to(BF16).to(dev)
            crit(zb, yd)
            ref.update(zb, yd)
        assert LS.last_path == "fused"
        got, want = m.compute(), ref.compute()
        assert got["n"] == want["n"] == 33 and got["correct1"] == want["correct1"] and got["correct5"] == want["correct5"]
        assert got["loss_sum"] == want["loss_sum"]  # the same expression on the same tree, the same fold
        crit.eval()
        crit(zb, yd)
        assert m.compute()["n"] == 33  # not advanced outside training mode
    # ... and on the fallback path
    m, ref = D.Metrics(topk=(1,), device=dev), D.Metrics(topk=(1,), device=dev)
    D.CrossEntropyLoss(weight=w, metrics=m)(z, yd)
    ref.update(z.detach(), yd)
    assert LS.last_path == "torch" and m.compute() == ref.compute()
    with pytest.raises(ValueError, match="ignore_index"):
        D.CrossEntropyLoss(ignore_index=-1, metrics=m)
    # a view with a row stride above K is read in place; any other layout is copied
    wide = torch.randn(12, 16, generator=gen).to(dev)
    for view in (wide[:, :10], wide.t()[:10].t(), wide[:, ::2]):
        a = D.cross_entropy(view, yd % 8, label_smoothing=0.1)  # labels in [0, 8): the narrowest view has 8 classes
        b = D.cross_entropy(view.contiguous(), yd % 8, label_smoothing=0.1)
        assert torch.equal(a, b) and bool(torch.isfinite(a))


@pytest.mark.filterwarnings("ignore:size_average and reduce args")
def test_module():
    check_module(torch.device("cpu"))


def _gloo_worker(rank, ws, port, q):
    import distributed_training_amd as D

    try:
        init_pg("gloo", rank, ws, port)
        gen = torch.Generator().manual_seed(rank)
        m = D.Metrics(topk=(1,))
        crit = D.CrossEntropyLoss(label_smoothing=0.1, metrics=m)
        n = 0
        for b in range(2 + rank):  # the ranks see different numbers of samples
            z = torch.randn(5 + b, 10, generator=gen, requires_grad=True)
            crit(z, torch.randint(0, 10, (5 + b,), generator=gen)).backward()
            n += 5 + b
        local = m.compute()
        m.reduce()
        q.put((rank, n, local, m.compute()))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:
        import traceback

        q.put((rank, f"rank {rank}: {e!r}\n{traceback.format_exc()}"))
        raise


def test_metrics_reduce_over_two_gloo_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(90)
    for p in procs:
        if p.is_alive():
            p.terminate()
    got = []
    while not q.empty():
        got.append(q.get())
    errs = [g[1] for g in got if len(g) == 2]
    assert not errs, "\n".join(errs)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert len(got) == 2
    total = sum(g[1] for g in got)
    assert total == (5 + 6) + (5 + 6 + 7)
    for rank, n, local, reduced in got:
        assert local["n"] == n and reduced["n"] == total
        assert reduced["correct1"] == sum(g[2]["correct1"] for g in got)
        assert reduced["loss_sum"] == pytest.approx(sum(g[2]["loss_sum"] for g in got), rel=1e-12)


def test_example_trainer_with_the_fused_loss():
    env = dict(os.environ, MASTER_PORT=str(free_port()), OMP_NUM_THREADS="1")
    cmd = [sys.executable, os.path.join(REPO, "examples", "ddp_train.py"), "--device", "cpu", "--world-size", "2",
           "--fused-loss", "--label-smoothing", "0.1", "--max-steps", "2", "--epochs", "1", "--batch-size", "8"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("epoch 1/1")]
    assert len(line) == 1, out.stdout
    words = line[0].split()
    n, loss, top1 = int(words[words.index("n") + 1]), float(words[words.index("loss") + 1]), float(words[-1])
    assert n == 2 * 2 * 8 and math.isfinite(loss) and loss > 0 and 0.0 <= top1 <= 1.0
