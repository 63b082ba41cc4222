"""References and fixtures for the evaluation tests (tests/test_eval_cpu.py, tests/test_gpu_bn_infer.py,
tests/test_gpu_eval.py).  Written from the contracts in include/gsync.h; the references do not call the library
(``run_accumulate`` is the tests' shared call of the host backend).

* ``metric_ref``: gs_eval_accumulate restated in numpy: exact counts, the per-row loss in fp64 and the
  per-row bound of the fp32 loss.
* ``metric_case``: logits (with a row stride above K) and labels with every special row the rules name.
* ``infer_exact_inputs`` / ``infer_steps``: gs_bn_infer_act's inputs on a grid where every step of the fixed
  arithmetic is exact in fp32, and those steps in fp64.
* ``infer_random_inputs`` / ``infer_truth``: random data and the fp64 truth with the derived bound.
"""
import math

import numpy as np
import torch

from tests import _bn_ref as B

U32 = 2.0 ** -24
EPS = 1e-5
EPS32 = float(np.float32(EPS))  # the kernel adds (float)eps


# ---- metrics -------------------------------------------------------------------------------------
def metric_ref(z, labels, n_valid, topk, ignore_index=-100):
    """z: float64 array [B, K] holding the logits' values exactly; labels: int64 [B].
    Returns (acc, rows): acc = [counted, bad, loss_sum, correct@k...] with exact integers and the fp64
    loss sum in ascending row order; rows = [(row, loss64, bound)] of the counted rows, bound being
    (ceil(log2 K) + 10) * 2^-24 * (1 + |m - z_y| + |log S|) (test_eval_cpu.py derives it)."""
    Bn, K = z.shape
    counted = bad = 0
    correct = [0] * len(topk)
    total = 0.0
    rows = []
    for r in range(Bn):
        y = int(labels[r])
        if r >= n_valid or y == ignore_index:
            continue
        if y < 0 or y >= K:
            bad += 1
            continue
        counted += 1
        zr = z[r]
        if np.isnan(zr).any():
            total += math.nan
            rows.append((r, math.nan, math.nan))
            continue
        zy = zr[y]
        rank = int((zr > zy).sum()) + int((zr[:y] == zy).sum())
        for i, k in enumerate(topk):
            correct[i] += rank < k
        m = zr.max()
        with np.errstate(invalid="ignore", over="ignore"):
            S = np.exp(zr - m).sum()
            loss = (m - zy) + math.log(S)
            bound = (math.ceil(math.log2(K)) + 10 if K > 1 else 10) * U32 * (1 + abs(m - zy) + abs(math.log(S)))
        total += loss
        rows.append((r, float(loss), float(bound)))
    return [counted, bad, total] + correct, rows


def metric_case(Bn, K, dtype, seed, pad=3, specials=True):
    """logits: a [Bn, K] view with row stride K + pad of a NaN-filled buffer; labels int64 [Bn].
    With ``specials`` (and room for them): row 0 all-equal logits, row 1 label ignore_index (-100),
    row 2 a tie between the label and a lower and a higher index, the last row duplicates of the maximum."""
    gen = torch.Generator().manual_seed(seed)
    buf = torch.full((Bn, K + pad), math.nan, dtype=dtype)
    z = (torch.randn(Bn, K, generator=gen) * 3).to(dtype)
    labels = torch.randint(0, K, (Bn,), generator=gen)
    if specials:
        z[0] = 0.25
        if Bn > 1:
            labels[1] = -100
        if Bn > 2 and K >= 3:
            y = int(labels[2].clamp(1, K - 2))
            labels[2] = y
            z[2, y - 1] = z[2, y]
            z[2, y + 1] = z[2, y]
        if Bn > 3:
            z[Bn - 1, : max(1, K // 2)] = z[Bn - 1].max()
    buf[:, :K] = z
    return buf[:, :K], labels


def values64(t):
    return t.to(torch.float64).numpy()


def acc_words(acc):
    """the accumulator tensor (int64[8]) -> [counted, bad, loss_sum, c0, c1, c2, c3]"""
    a = acc.cpu()
    return [int(a[0]), int(a[1]), float(a[2:3].view(torch.float64)[0])] + [int(v) for v in a[4:8]]


# ---- inference BatchNorm: the exact grid ----------------------------------------------------------
INFER_SHAPES = [(1, 8), (5, 8), (63, 16), (64, 64), (1025, 72), (4099, 256), (257, 2048)]
INFER_VARIANTS = [(False, False), (False, True), (True, False), (True, True)]  # (residual, relu)
W_CYCLE = (0.5, -1.0, 2.0, 1.0, -0.5, -2.0, 1.0)


def infer_exact_inputs(R, C, seed=None):
    """running_var = fl32(4^k - eps), k = (c mod 5) - 2, so fl32(var + (float)eps) == 4^k and
    1 / sqrt(.) == 2^-k; weights +-2^j; means multiples of 1/2 in [-4, 4]; biases multiples of 1/4 in
    [-2, 2]; x multiples of 1/4 in [-4, 4] (bf16); residuals multiples of 1/8 in [-2, 2] (bf16).
    Cycle lengths 5, 7, 17, 9 are coprime with 8 and 64: channels swapped inside a vector or a tile show."""
    gen = torch.Generator().manual_seed(B.exact_seed(R, C) if seed is None else seed)
    c = torch.arange(C)
    k = (c % 5) - 2
    var = (torch.ldexp(torch.ones(C, dtype=torch.float64), 2 * k) - EPS).to(torch.float32)
    weight = torch.tensor(W_CYCLE, dtype=torch.float32)[c % 7]
    mean = (((5 * c) % 17) - 8).to(torch.float32) * 0.5
    bias = (((2 * c) % 9) - 4).to(torch.float32) * 0.5
    x = ((torch.randint(0, 33, (R, C), generator=gen) - 16).to(torch.float32) * 0.25).to(torch.bfloat16)
    res = ((torch.randint(0, 33, (R, C), generator=gen) - 16).to(torch.float32) * 0.125).to(torch.bfloat16)
    return dict(x=x, res=res, mean=mean, var=var, weight=weight, bias=bias)


def infer_steps(inp, residual, relu, eps32=EPS32):
    """every step of the fixed arithmetic: var + (float)eps as the fp32 sum it is (on the exact grid it
    rounds to 4^k by construction), the steps after it in fp64: a dict of the intermediates and ``v``, the
    value before the one rounding to bf16.  On the exact grid each of them is an fp32 value."""
    w = inp["weight"].double()
    d = (inp["var"] + torch.tensor(eps32, dtype=torch.float32)).double()
    root = torch.sqrt(d)
    inv = 1.0 / root
    s = w * inv
    t = (-inp["mean"].double()) * s + inp["bias"].double()
    v = inp["x"].double() * s + t
    steps = dict(d=d, root=root, inv=inv, s=s, t=t, fma=v)
    if residual:
        v = v + inp["res"].double()
        steps["add"] = v
    if relu:
        v = torch.where(v > 0, v, torch.where(torch.isnan(v), v, torch.zeros_like(v)))
    steps["v"] = v
    return steps


def round_bf16(v):
    """fp64 values that are fp32 values -> bf16, round to nearest even (torch's conversion; NaN -> 0x7FC0)"""
    return v.to(torch.float32).to(torch.bfloat16)


# ---- inference BatchNorm: random data ---------------------------------------------------------------
def infer_random_inputs(R, C, seed):
    """means over [-8, 8], standard deviations over [0.25, 4] (var = sd^2), a zero variance in channel 2,
    weights in [0.5, 1.5] with a negative and a zero one, x ~ N(mean, sd), residual ~ N(0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    mean = torch.linspace(-8.0, 8.0, C)
    sd = torch.logspace(math.log10(0.25), math.log10(4.0), C).flip(0)
    var = (sd * sd).to(torch.float32)
    var[2 % C] = 0.0
    weight = torch.empty(C).uniform_(0.5, 1.5, generator=gen)
    weight[0], weight[1] = -0.75, 0.0
    bias = torch.empty(C).uniform_(-1.0, 1.0, generator=gen)
    x = (torch.randn(R, C, generator=gen) * sd + mean).to(torch.bfloat16)
    res = torch.randn(R, C, generator=gen).to(torch.bfloat16)
    return dict(x=x, res=res, mean=mean, var=var, weight=weight, bias=bias)


def infer_truth(inp, residual, relu):
    """(truth, bound): the fp64 result and ulp_bf16(truth) / 2 + 8 * 2^-24 * (|x s| + |mean s| + |bias| + |r|)"""
    s = inp["weight"].double() / torch.sqrt(inp["var"].double() + EPS32)
    xs = inp["x"].double() * s
    ms = inp["mean"].double() * s
    v = xs - ms + inp["bias"].double()
    mag = xs.abs() + ms.abs() + inp["bias"].double().abs()
    if residual:
        v = v + inp["res"].double()
        mag = mag + inp["res"].double().abs()
    if relu:
        v = torch.clamp(v, min=0.0)
    return v, B.ulp_bf16(v) / 2 + 8 * U32 * mag


# ---- shared by the CPU and the GPU tests ------------------------------------------------------------------
TOPK = (1, 2, 5, 9)


def run_accumulate(lib, logits, labels, n_valid, topk=TOPK, acc=None, ignore_index=-100):
    from distributed_training_amd import _lib as L

    Bn, K = logits.shape
    acc = torch.zeros(8, dtype=torch.int64) if acc is None else acc
    ws = torch.empty(max(1, Bn), dtype=torch.int64)
    rc = lib.gs_eval_accumulate(L.GS_DEV_HOST, logits.data_ptr(), L.gs_dtype(logits.dtype), labels.data_ptr(), Bn, K,
                                logits.stride(0), n_valid, L.i32_array(topk), len(topk), ignore_index, ws.data_ptr(),
                                acc.data_ptr(), None)
    assert rc == 0, lib.gs_last_error()
    return acc, ws


def row_losses(ws):
    """the scratch words -> the fp32 loss of each row (the low half of each 8-byte word)"""
    return ws.view(torch.float32)[0::2].double().tolist()


def check_against_ref(logits, labels, n_valid, acc, ws, topk=TOPK):
    """counts exact, every counted row's fp32 loss within its bound (a NaN row: NaN), the fp64 sum within
    the sum of the bounds; -> the worst error / bound"""
    want, rows = metric_ref(values64(logits), labels.numpy(), n_valid, topk)
    got = acc_words(acc)
    assert got[:2] == want[:2], (got, want)
    assert got[3:3 + len(topk)] == want[3:], (got, want)
    loss = row_losses(ws)
    worst = 0.0
    for r, l64, bound in rows:
        if math.isnan(l64):
            assert math.isnan(loss[r]), r
            continue
        err = abs(loss[r] - l64)
        worst = max(worst, err / bound)
        assert err <= bound, (r, loss[r], l64, bound)
    if math.isnan(want[2]):
        assert math.isnan(got[2])
    else:
        assert abs(got[2] - want[2]) <= sum(b for _, _, b in rows) + 1e-12
    return worst


N_SAMPLES, BATCH = 13, 4


def eval_dataset(dtype=torch.float32):
    g = torch.Generator().manual_seed(11)
    x = torch.rand(N_SAMPLES, 3, 32, 32, generator=g).to(dtype)
    y = torch.randint(0, 10, (N_SAMPLES,), generator=g)
    return torch.utils.data.TensorDataset(x, y)


def eval_model():
    from distributed_training_amd.resnet import micro_resnet

    torch.manual_seed(0)
    m = micro_resnet()
    g = torch.Generator().manual_seed(1)
    for mod in m.modules():  # running statistics that are not the initial 0 / 1
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    return m
