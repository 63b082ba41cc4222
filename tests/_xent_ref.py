"""References and fixtures for the training criterion's tests (tests/test_xent_cpu.py, tests/test_gpu_xent.py).
Written from the contracts of gs_xent_fwd / gs_xent_bwd in include/gsync.h; the references do not call the
library (``run_xent`` is the tests' shared call of it, on the host backend or a device).

* ``xent_ref``: both entries restated in numpy fp64: codes, per-row losses, the reduced loss, the gradient,
  and the bounds test_xent_cpu.py derives.
* ``torch_ref``: ``F.cross_entropy`` on the fp64 copy of the logits and its autograd gradient.
* ``xent_case``: ``_eval_ref.metric_case`` logits (row stride above K, NaN-filled padding, the special rows).
* ``check_xent``: the comparison both test files make.
"""
import math

import numpy as np
import torch

from tests._eval_ref import U32, metric_case, values64

SENTINEL = 1536.0  # prefill of the gradient buffer; exact in every dtype
REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}
# the unit roundoff of the gradient's dtype
U_OUT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
CONST_P = 8  # the constant of the softmax term (test_xent_cpu.py derives it)


def levels(K):
    return math.ceil(math.log2(K)) if K > 1 else 0


def xent_ref(z, labels, eps, dtype, ignore_index=-100):
    """z: float64 [B, K] holding the logits' values exactly; labels int64 [B]; eps: the python float handed to
    the library (the arithmetic uses its fp32 value, as the library does).  Returns a dict:
    code [B] (rank, INT32_MAX, -1, -2), loss / loss_bound / nll / nll_bound [B] (0 where not counted),
    counted, bad, total (fp64 sum of the counted losses, ascending), total_bound, and
    ``grad(reduction, g) -> (dz64 [B, K], bound [B, K])``."""
    Bn, K = z.shape
    e32 = float(np.float32(eps))
    L = levels(K)
    code = np.zeros(Bn, dtype=np.int64)
    loss, lb, nll, nb = (np.zeros(Bn) for _ in range(4))
    m_, logS_ = np.zeros(Bn), np.zeros(Bn)
    for r in range(Bn):
        y = int(labels[r])
        if y == ignore_index:
            code[r] = -1
            continue
        if y < 0 or y >= K:
            code[r] = -2
            continue
        zr = z[r]
        if np.isnan(zr).any():
            code[r] = 2 ** 31 - 1
            loss[r] = lb[r] = nll[r] = nb[r] = m_[r] = logS_[r] = math.nan
            continue
        zy = zr[y]
        code[r] = int((zr > zy).sum()) + int((zr[:y] == zy).sum())
        m = zr.max()
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            logS = math.log(np.exp(zr - m).sum())
            nll[r] = (m - zy) + logS
            nb[r] = (L + 10) * U32 * (1 + abs(m - zy) + abs(logS))
            if e32 == 0.0:
                loss[r], lb[r] = nll[r], nb[r]
            else:
                smooth = (m + logS) - zr.sum() / K
                sb = U32 * ((L + 5) + 3 * abs(logS) + abs(m + logS) + (L + 2) * np.abs(zr).sum() / K + abs(smooth))
                loss[r] = (1 - e32) * nll[r] + e32 * smooth
                lb[r] = (1 - e32) * nb[r] + e32 * sb + 4 * U32 * ((1 - e32) * abs(nll[r]) + e32 * abs(smooth))
        m_[r], logS_[r] = m, logS
    on = code >= 0
    total = 0.0
    for r in range(Bn):
        if on[r]:
            total += loss[r]
    counted, bad = int(on.sum()), int((code == -2).sum())

    def grad(reduction, g):
        """g: fp64 scalar (mean, sum) or [B] (none)"""
        u_out = U_OUT[dtype]
        dz = np.zeros((Bn, K))
        bound = np.zeros((Bn, K))
        q_off = e32 / K
        for r in range(Bn):
            if not on[r]:
                continue
            if code[r] == 2 ** 31 - 1:
                dz[r] = bound[r] = math.nan
                continue
            c = {"mean": lambda: g / counted, "sum": lambda: g, "none": lambda: g[r]}[reduction]()
            with np.errstate(invalid="ignore", over="ignore"):
                d = z[r] - m_[r]
                p = np.exp(d - logS_[r])
                q = np.full(K, q_off)
                q[int(labels[r])] = (1 - e32) + q_off
                dz[r] = c * (p - q)
                ep = np.where(p > 0, p * (L + CONST_P + 2 * abs(logS_[r]) + np.where(p > 0, np.abs(d), 0.0)) * U32, 0.0)
                e = abs(c) * (ep + 3 * U32 * q + 3 * U32 * np.abs(p - q))
                bound[r] = e + u_out * (np.abs(dz[r]) + e) + (2.0 ** -25 if dtype == torch.float16 else 0.0)
        return dz, bound

    return dict(code=code, loss=loss, loss_bound=lb, nll=nll, nll_bound=nb, counted=counted, bad=bad, total=total,
                total_bound=float(np.nansum(lb[on])) if counted else 0.0, grad=grad, on=on)


def torch_ref(logits, labels, eps, reduction, g):
    """F.cross_entropy on the fp64 CPU copy and the gradient autograd gives for grad_output g"""
    z = logits.detach().cpu().to(torch.float64).clone().requires_grad_()
    out = torch.nn.functional.cross_entropy(z, labels.cpu(), reduction=reduction, label_smoothing=eps)
    out.backward(torch.as_tensor(g, dtype=torch.float64).reshape(out.shape))
    return out.detach().numpy(), z.grad.numpy()


def xent_case(Bn, K, dtype, seed, pad=3, specials=True):
    return metric_case(Bn, K, dtype, seed, pad=pad, specials=specials)


def grad_out_for(reduction, Bn, seed=0):
    """a fixed upstream gradient: 0.75 for the reduced losses, values in [-1, 1] per row for ``none``"""
    if reduction != "none":
        return np.float64(0.75)
    gen = torch.Generator().manual_seed(1000 + seed)
    return (torch.rand(Bn, generator=gen) * 2 - 1).to(torch.float32).double().numpy()


def run_xent(lib, logits, labels, eps, reductions=("mean",), device=None, topk=(), acc=None, ignore_index=-100,
             grad_outs=None):
    """gs_xent_fwd, then gs_xent_bwd once per reduction, on the host backend (device None) or on ``device``.
    logits: a [B, K] view of a buffer whose padding is NaN; the copy handed to the library keeps that layout,
    and the gradient buffer has the same row stride, prefilled with SENTINEL.  Returns CPU tensors:
    rows [B, 4] fp32, code [B] int32, red (loss_sum, loss_mean, counted, bad), dz {reduction: [B, stride]}."""
    from distributed_training_amd import _lib as L

    Bn, K = logits.shape
    stride = logits.stride(0) if Bn > 1 else max(K, logits.stride(0))
    dev = torch.device("cpu") if device is None else device
    kind = L.GS_DEV_HOST if device is None else L.GS_DEV_HIP
    zl = torch.full((Bn, stride), math.nan, dtype=logits.dtype, device=dev)
    zl[:, :K] = logits.to(dev)
    yl = labels.to(dev)
    rows = torch.zeros(max(1, Bn) * 4, dtype=torch.float32, device=dev)
    red = torch.zeros(4, dtype=torch.float32, device=dev)
    stream = L.stream_ptr(dev)
    rc = lib.gs_xent_fwd(kind, zl.data_ptr(), L.gs_dtype(zl.dtype), yl.data_ptr(), Bn, K, stride, ignore_index, eps,
                         rows.data_ptr(), red.data_ptr(), L.i32_array(topk) if topk else None, len(topk),
                         None if acc is None else acc.data_ptr(), stream)
    assert rc == 0, lib.gs_last_error()
    dz = {}
    for red_name in reductions:
        g = grad_out_for(red_name, Bn) if grad_outs is None else grad_outs[red_name]
        gt = torch.as_tensor(g, dtype=torch.float32).reshape(-1).to(dev)
        d = torch.full((Bn, stride), SENTINEL, dtype=logits.dtype, device=dev)
        rc = lib.gs_xent_bwd(kind, zl.data_ptr(), L.gs_dtype(zl.dtype), yl.data_ptr(), Bn, K, stride, ignore_index, eps,
                             REDUCTIONS[red_name], rows.data_ptr(), red.data_ptr(), gt.data_ptr(), d.data_ptr(), stride,
                             stream)
        assert rc == 0, lib.gs_last_error()
        dz[red_name] = d
    if device is not None:
        torch.cuda.synchronize()
    rows = rows.cpu()
    r4 = rows[:4 * Bn].view(Bn, 4)
    redc = red.cpu()
    return dict(rows=r4, code=rows.view(torch.int32)[:4 * Bn].view(Bn, 4)[:, 3].clone(),
                red=(float(redc[0]), float(redc[1]), int(redc.view(torch.int32)[2]), int(redc.view(torch.int32)[3])),
                dz={k: v.cpu() for k, v in dz.items()}, K=K)


def _close(got, want, bound, what):
    """|got - want| <= bound elementwise; NaN and +-inf must match exactly.  -> the worst error / bound"""
    got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want), np.asarray(bound)
    special = ~np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), what
    err = np.abs(got[~special] - want[~special])
    b = bound[~special]
    bad = err > b
    assert not bad.any(), (what, float(err[bad].max()), float((err / np.maximum(b, 1e-300)).max()))
    return float((err / np.maximum(b, 1e-300)).max()) if err.size else 0.0


def check_xent(logits, labels, eps, out, reductions=("none", "mean", "sum"), against_torch=True):
    """``out`` (run_xent's) against the numpy restatement and against torch in fp64: codes and counts exactly,
    every loss and gradient element within its bound, padding untouched, gradient rows summing to zero.
    -> the worst error / bound seen."""
    Bn, K = logits.shape
    z = values64(logits)
    ref = xent_ref(z, labels.numpy(), eps, logits.dtype)
    assert np.array_equal(out["code"].numpy().astype(np.int64), ref["code"])
    loss_sum, loss_mean, counted, bad = out["red"]
    assert (counted, bad) == (ref["counted"], ref["bad"])
    rows = out["rows"].double().numpy()
    on = ref["on"]
    assert not rows[~on, :3].any()  # {0, 0, 0} for a row that is not counted
    worst = _close(rows[on, 0], ref["loss"][on], ref["loss_bound"][on], "row loss")
    # the reduced loss: the fp64 sum of the fp32 losses, rounded once
    if bad:
        assert math.isnan(loss_sum) and math.isnan(loss_mean)
    else:
        tb = ref["total_bound"]
        worst = max(worst, _close([loss_sum], [ref["total"]], [tb + U32 * abs(ref["total"])], "loss_sum"))
        if counted:
            mean = ref["total"] / counted
            worst = max(worst, _close([loss_mean], [mean], [tb / counted + U32 * abs(mean)], "loss_mean"))
        else:
            assert loss_sum == 0.0 and math.isnan(loss_mean)
    de = abs(float(np.float32(eps)) - eps)  # torch uses the double eps
    for name in reductions:
        g = grad_out_for(name, Bn)
        full = out["dz"][name].double().numpy()
        got = full[:, :K]
        assert (full[:, K:] == SENTINEL).all(), "gradient padding written"
        want, bound = ref["grad"](name, g)
        assert not got[~on].any()
        worst = max(worst, _close(got[on], want[on], bound[on], f"gradient ({name})"))
        fin = on & np.isfinite(want).all(axis=1)
        assert (np.abs(got[fin].sum(axis=1)) <= bound[fin].sum(axis=1)).all(), "a gradient row does not sum to 0"
        if against_torch and not bad and not np.isnan(z[on]).any():
            tl, tg = torch_ref(logits, labels, eps, name, g)
            gmax = np.abs(g).max()
            _close(got[on], tg[on], bound[on] + 2 * de * gmax, f"gradient vs torch ({name})")
            with np.errstate(invalid="ignore"):  # d loss / d eps = smooth - nll = (loss - nll) / eps
                slack = de * np.abs(ref["loss"] - ref["nll"]) / eps if eps else np.zeros(Bn)
            if name == "none":
                _close(rows[:, 0], tl, ref["loss_bound"] + slack, "loss vs torch (none)")
            elif name == "sum":
                _close([loss_sum], [tl], [tb + U32 * abs(tl) + np.nansum(slack[on])], "loss vs torch (sum)")
            elif counted:
                _close([loss_mean], [tl], [tb / counted + U32 * abs(tl) + np.nansum(slack[on]) / counted],
                       "loss vs torch (mean)")
    return worst
