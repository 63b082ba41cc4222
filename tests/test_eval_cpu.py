"""Evaluation without a GPU: gs_eval_accumulate on the host backend against a numpy restatement,
``evaluate`` over gloo, the model-state guarantees, the argument checks of the inference BatchNorm
entries and the exactness of the grid the GPU tests compare bit for bit.

The loss bound.  For a counted row with maximum m, S = sum_j exp(z_j - m) and label logit z_y the
library forms loss = (m - z_y) + logf(S) in fp32 (u = 2^-24):
  * z_j - m is one subtraction (relative error u, absolute u |z_j - m|); expf adds at most 2 ulp; a
    term's relative error is at most (3 + |z_j - m|) u, and |z_j - m| exp(z_j - m) <= 1/e, so the terms'
    errors move S by at most 4 u S;
  * S is a balanced tree of depth ceil(log2 K): at most ceil(log2 K) roundings on a path, each
    relative u of a partial sum <= S, so the sum moves S by at most ceil(log2 K) u S;
  * a relative error d of S moves log S by d; logf adds 2 ulp of |log S| (2 u |log S|) and,
    near S = 1, an absolute error below u;
  * m - z_y: one rounding, u |m - z_y|; the final add: one rounding, u |loss| <= u (|m - z_y| + |log S|).
Together |loss - truth| <= (ceil(log2 K) + 4 + 1) u + 3 u |log S| + 2 u |m - z_y|
                        <= (ceil(log2 K) + 10) u (1 + |m - z_y| + |log S|).
"""
import copy
import math

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _bn_ref as B
from tests import _eval_ref as E
from tests._dist_util import free_port, init_pg
from tests._eval_ref import BATCH, N_SAMPLES, TOPK, check_against_ref, run_accumulate
from tests._eval_ref import eval_dataset as _dataset
from tests._eval_ref import eval_model as _model


@pytest.fixture(scope="module")
def lib():
    from distributed_training_amd import _lib as L

    return L.lib()


# ---- gs_eval_accumulate on the host ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [1, 2, 10, 65, 1000])
@pytest.mark.parametrize("Bn", [1, 3, 64, 257])
def test_counts_and_loss(lib, Bn, K, dtype):
    logits, labels = E.metric_case(Bn, K, dtype, seed=Bn * 1009 + K)
    assert logits.stride(0) > K
    for n_valid in sorted({0, 1, Bn - 1, Bn}):
        acc, ws = run_accumulate(lib, logits, labels, n_valid)
        check_against_ref(logits, labels, n_valid, acc, ws)


def test_all_equal_logits_rank_is_the_label(lib):
    K = 10
    logits = torch.full((K, K), 1.5)
    labels = torch.arange(K)
    acc, _ = run_accumulate(lib, logits, labels, K, topk=(1, 3, 10))
    assert E.acc_words(acc)[:6] == [K, 0, pytest.approx(K * math.log(K), abs=1e-5), 1, 3, 10]


def test_nan_row_is_incorrect_and_poisons_the_loss(lib):
    logits, labels = E.metric_case(8, 10, torch.float32, seed=5, specials=False)
    logits[3, 7] = math.nan
    labels[3] = 7
    acc, _ = run_accumulate(lib, logits, labels, 8, topk=(1, 10))
    want, _ = E.metric_ref(E.values64(logits), labels.numpy(), 8, (1, 10))
    got = E.acc_words(acc)
    assert got[0] == 8 and got[3:5] == want[3:5] and got[4] == 7  # top-10 of 10 classes: every row but the NaN one
    assert math.isnan(got[2])


def test_bad_label_is_counted_apart_and_compute_raises(lib):
    from distributed_training_amd import Metrics

    logits, labels = E.metric_case(6, 10, torch.float32, seed=6, specials=False)
    labels[2] = 10
    labels[4] = -3
    acc, ws = run_accumulate(lib, logits, labels, 6)
    check_against_ref(logits, labels, 6, acc, ws)
    assert E.acc_words(acc)[:2] == [4, 2]
    m = Metrics(topk=(1,), device="cpu")
    m.update(logits.contiguous(), labels)
    with pytest.raises(ValueError, match="outside"):
        m.compute()
    m.reset()
    labels[2], labels[4] = 1, -100
    m.update(logits, labels)
    assert m.compute()["n"] == 5


def test_three_calls_accumulate_the_concatenation(lib):
    parts = [E.metric_case(b, 17, torch.float32, seed=40 + b) for b in (5, 9, 2)]
    acc = torch.zeros(8, dtype=torch.int64)
    for z, y in parts:
        run_accumulate(lib, z, y, z.shape[0], acc=acc)
    z = torch.cat([p[0] for p in parts])
    y = torch.cat([p[1] for p in parts])
    want, rows = E.metric_ref(E.values64(z), y.numpy(), z.shape[0], TOPK)
    got = E.acc_words(acc)
    assert got[:2] == want[:2] and got[3:7] == want[3:]
    assert abs(got[2] - want[2]) <= sum(b for _, _, b in rows)
    # the same calls again give the same bits
    acc2 = torch.zeros(8, dtype=torch.int64)
    for zz, yy in parts:
        run_accumulate(lib, zz, yy, zz.shape[0], acc=acc2)
    assert torch.equal(acc, acc2)


def test_fp16_logits(lib):
    logits, labels = E.metric_case(9, 33, torch.float16, seed=9)
    acc, ws = run_accumulate(lib, logits, labels, 9)
    check_against_ref(logits, labels, 9, acc, ws)


A = 0x7F0000001000  # made-up addresses, never dereferenced


def _einval(lib, rc):
    from distributed_training_amd import _lib as L

    assert rc == L.GS_EINVAL, rc
    assert lib.gs_last_error()


@pytest.mark.parametrize("bad", [dict(kind=7), dict(dtype=4), dict(B=-1), dict(K=0), dict(K=2 ** 30 + 1),
                                 dict(stride=9), dict(n_valid=5), dict(n_valid=-1), dict(n_topk=5), dict(topk=(0, 1)),
                                 dict(logits=None), dict(labels=None), dict(ws=None), dict(acc=None), dict(acc=A + 4),
                                 dict(ws=A + 4), dict(logits=A + 2)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_accumulate_rejects(lib, bad):
    from distributed_training_amd import _lib as L

    a = dict(kind=L.GS_DEV_HOST, logits=A, dtype=L.GS_F32, labels=A + 0x10000, B=4, K=10, stride=10, n_valid=4,
             topk=(1, 5), n_topk=None, ign=-100, ws=A + 0x20000, acc=A + 0x30000)
    a.update(bad)
    n_topk = len(a["topk"]) if a["n_topk"] is None else a["n_topk"]
    _einval(lib, lib.gs_eval_accumulate(a["kind"], a["logits"], a["dtype"], a["labels"], a["B"], a["K"], a["stride"],
                                        a["n_valid"], L.i32_array(a["topk"]), n_topk, a["ign"], a["ws"], a["acc"],
                                        None))


# ---- the padding rule against torch's sampler --------------------------------------------------------
@pytest.mark.parametrize("shuffle", [False, True])
def test_real_sample_rule_matches_the_samplers(shuffle):
    from distributed_training_amd import data as D
    from distributed_training_amd.evaluation import _real_samples

    class Loader:
        pass

    for N in (1, 5, 7, 10, 13):
        ds = list(range(N))
        for ws in (1, 2, 3, 4, 8):
            seen = []
            for rank in range(ws):
                for cls in (torch.utils.data.distributed.DistributedSampler, D.DistributedSampler):
                    s = cls(ds, num_replicas=ws, rank=rank, shuffle=shuffle, seed=3, drop_last=False)
                    ld = Loader()
                    ld.sampler = s
                    real = _real_samples(ld)
                    assert real == max(0, math.ceil((N - rank) / ws))
                    idx = list(iter(s))
                    assert len(idx) == math.ceil(N / ws)
                    if cls is D.DistributedSampler:
                        seen += idx[:real]
            assert sorted(seen) == ds  # the real samples of all ranks are the dataset, each once
    ld = Loader()
    ld.sampler = D.DistributedSampler(list(range(7)), num_replicas=2, rank=0, drop_last=True)
    assert _real_samples(ld) is None


# ---- evaluate over gloo ---------------------------------------------------------------------------------
def _single_process():
    import distributed_training_amd as D

    ds = _dataset()
    return D.evaluate(_model(), torch.utils.data.DataLoader(ds, batch_size=BATCH), topk=(1, 5))


def _gloo_worker(rank, ws, port, q):
    import distributed_training_amd as D
    from distributed_training_amd import data as gdata
    from distributed_training_amd import fused_bn

    try:
        init_pg("gloo", rank, ws, port)
        ds = _dataset()
        out = {}
        for name, cls in (("torch", torch.utils.data.distributed.DistributedSampler),
                          ("ours", gdata.DistributedSampler)):
            sampler = cls(ds, num_replicas=ws, rank=rank, shuffle=False, drop_last=False)
            loader = torch.utils.data.DataLoader(ds, batch_size=BATCH, sampler=sampler)
            out[name] = D.evaluate(_model(), loader, topk=(1, 5))
            out[name + "_padded"] = D.evaluate(_model(), loader, topk=(1, 5), dedup_padding=False)
        out["last_path"] = fused_bn.last_path
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:
        import traceback

        q.put((rank, f"rank {rank}: {e!r}\n{traceback.format_exc()}"))
        raise


@pytest.mark.parametrize("ws", [2, 3])
def test_evaluate_over_gloo_counts_every_sample_once(ws):
    want = _single_process()
    assert want["n"] == N_SAMPLES
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, ws, port, q)) for r in range(ws)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(90)
    for p in procs:
        if p.is_alive():
            p.terminate()
    got = {}
    while not q.empty():  # the workers have ended: nothing here waits
        rank, out = q.get()
        got[rank] = out
    errs = [v for v in got.values() if isinstance(v, str)]
    assert not errs, "\n".join(errs)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    padded_n = math.ceil(N_SAMPLES / ws) * ws
    assert padded_n == {2: 14, 3: 15}[ws]
    for rank in range(ws):
        out = got[rank]
        assert out["last_path"] == "stock"
        for name in ("torch", "ours"):
            r = out[name]
            assert r["n"] == N_SAMPLES
            assert r["correct1"] == want["correct1"] and r["correct5"] == want["correct5"]
            assert r["top1"] == want["top1"] and r["top5"] == want["top5"]
            assert r["loss"] == pytest.approx(want["loss"], rel=1e-6)  # per-row fp32 losses, another batch split
            assert out[name + "_padded"]["n"] == padded_n


# ---- model state ---------------------------------------------------------------------------------------
def test_evaluate_leaves_the_model_as_it_was():
    import distributed_training_amd as D

    model = _model()
    model.train()
    model.layer2.eval()
    model.layer3[0].bn1.eval()
    ds = _dataset()
    # grads to preserve
    torch.nn.functional.cross_entropy(model(ds.tensors[0][:4]), ds.tensors[1][:4]).backward()
    flags = {n: m.training for n, m in model.named_modules()}
    assert len(set(flags.values())) == 2
    state = {k: v.clone() for k, v in model.state_dict().items()}
    grads = {n: p.grad.clone() for n, p in model.named_parameters()}
    out = D.evaluate(model, torch.utils.data.DataLoader(ds, batch_size=BATCH), max_batches=2)
    assert out["n"] == 2 * BATCH
    assert {n: m.training for n, m in model.named_modules()} == flags
    now = model.state_dict()
    assert list(now) == list(state)
    for k in state:
        assert torch.equal(B.bits(now[k]) if now[k].is_floating_point() else now[k],
                           B.bits(state[k]) if state[k].is_floating_point() else state[k]), k
    assert any(k.endswith("num_batches_tracked") for k in state)
    for n, p in model.named_parameters():
        assert torch.equal(B.bits(p.grad), B.bits(grads[n])), n
    # an exception inside the loop restores the flags too
    with pytest.raises(ValueError):
        D.evaluate(model, [(ds.tensors[0][:4], ds.tensors[1][:3])])
    assert {n: m.training for n, m in model.named_modules()} == flags


def test_fused_eval_flag_is_off_by_default_and_restored():
    from distributed_training_amd import fused_bn

    assert fused_bn._fused_eval is False
    with fused_bn.fused_eval():
        assert fused_bn._fused_eval is True
        with fused_bn.fused_eval(False):
            assert fused_bn._fused_eval is False
        assert fused_bn._fused_eval is True
    assert fused_bn._fused_eval is False
    with pytest.raises(RuntimeError):
        with fused_bn.fused_eval():
            raise RuntimeError("x")
    assert fused_bn._fused_eval is False
    # a CPU call inside the context is the stock path
    bn = torch.nn.BatchNorm2d(8).eval()
    x = torch.randn(2, 8, 3, 3)
    with fused_bn.fused_eval(), torch.no_grad():
        y = fused_bn.bn_act(bn, x)
    assert fused_bn.last_path == "stock" and torch.equal(y, torch.relu(bn(x)))


# ---- argument checks of the inference BatchNorm entries, all before any launch ---------------------------
R0, C0 = 777, 24


def _act_args(**kw):
    a = dict(x=A, res=A + 0x100000, mean=A + 0x400000, var=A + 0x410000, w=A + 0x420000, b=A + 0x430000, eps=1e-5,
             relu=1, y=A + 0x200000, R=R0, C=C0)
    a.update(kw)
    return [a[k] for k in ("x", "res", "mean", "var", "w", "b", "eps", "relu", "y", "R", "C")] + [None]


ACT_BAD = ([{k: None} for k in ("x", "mean", "var", "w", "b", "y")]
           + [{k: A + 0x700008} for k in ("x", "res", "mean", "var", "w", "b", "y")]
           + [dict(C=12), dict(C=0), dict(R=0), dict(R=-5), dict(eps=-1.0), dict(eps=math.nan), dict(R=2 ** 60),
              dict(y=A + 0x10), dict(y=A + 0x100000), dict(y=A + 0x100000 + 16)])


@pytest.mark.parametrize("bad", ACT_BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_infer_act_rejects(lib, bad):
    _einval(lib, lib.gs_bn_infer_act(*_act_args(**bad)))


def _pool_args(**kw):
    a = dict(x=A, mean=A + 0x400000, var=A + 0x410000, w=A + 0x420000, b=A + 0x430000, eps=1e-5, out=A + 0x200000,
             N=2, H=9, W=7, C=16)
    a.update(kw)
    return [a[k] for k in ("x", "mean", "var", "w", "b", "eps", "out", "N", "H", "W", "C")] + [None]


POOL_BAD = ([{k: None} for k in ("x", "mean", "var", "w", "b", "out")]
            + [{k: A + 0x700008} for k in ("x", "mean", "var", "w", "b", "out")]
            + [dict(C=12), dict(C=0), dict(N=0), dict(H=0), dict(W=-1), dict(eps=-1.0), dict(N=2 ** 60),
               dict(out=A), dict(out=A + 0x10)])


@pytest.mark.parametrize("bad", POOL_BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_infer_relu_maxpool_rejects(lib, bad):
    _einval(lib, lib.gs_bn_infer_relu_maxpool(*_pool_args(**bad)))


# ---- the exact grid is exact ------------------------------------------------------------------------------
def test_exact_variances():
    for k in range(-2, 3):
        var = np.float32(4.0 ** k - E.EPS)
        assert np.float32(var + np.float32(E.EPS)) == np.float32(4.0 ** k)


@pytest.mark.parametrize("shape", E.INFER_SHAPES, ids=B.shape_id)
def test_infer_exact_grid_is_exact(shape):
    R, C = shape
    inp = E.infer_exact_inputs(R, C)
    assert inp["x"].dtype == torch.bfloat16 and inp["res"].dtype == torch.bfloat16
    assert bool((inp["x"].double() * 4 == (inp["x"].double() * 4).round()).all())  # the bf16 conversion kept the grid
    assert bool((inp["res"].double() * 8 == (inp["res"].double() * 8).round()).all())
    rounded = 0
    for residual, relu in E.INFER_VARIANTS:
        st = E.infer_steps(inp, residual, relu)
        # fl32(var + eps32) is a power of four: the fp32 sum of the two fp32 values rounds to it
        half_log = torch.log2(st["d"]) / 2
        assert bool((half_log == half_log.round()).all()) and float(half_log.abs().max()) == 2
        for name, v in st.items():
            assert bool(B.is_f32(v).all()), (residual, relu, name)
        y = E.round_bf16(st["v"])
        rounded += int((y.double() != st["v"]).sum())
    assert R * C < 64 or rounded > 0  # the one rounding to bf16 is exercised
