"""gs_bn_bwd_reduce_fork called directly (include/gsync.h): the BatchNorm backward's first pass fed
the two halves of a fork's gradient.

A. on the exact grid of tests/_bn_ref.py (dy_a and dy_b multiples of 0.25 in [-2, 2], so their sum is a
   bf16 and every sum of the pass is exact in fp32 in any order): g_out equals ATen's
   threshold_backward(dy_a + dy_b, y, 0) computed on the device bit for bit (without y: dy_a + dy_b),
   the workspace's sums equal the fp64 reference bit for bit and every partial was written;
B. special values in dy_a / dy_b (ties at a bf16 midpoint of both parities, overflow to Inf on rounding,
   Inf - Inf, NaN, signed zeros, subnormals), each against y in {+x, -x, +0, -0, NaN}, against the
   same two ATen kernels;
C. dy_b absent: the entry is gs_bn_bwd_reduce, bit for bit.

Every buffer is a _bn_ref.guarded view; the workspace is exactly P * C * 2 floats prefilled with NaN;
after the launch the guards are intact and the inputs bitwise unchanged.
"""
import pytest
import torch

from tests import _bn_ref as B

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32

# (R, C): one row; fewer rows than a step; ragged channel tiles below and above one tile; tx = 8 with
# several unrolled iterations; P > 1 with a ragged tile and tail; 2 * ty * unroll + 3 rows at tx = 2
# (ty = 128, 4 rows in flight): unrolled iterations plus a tail
FORK_SHAPES = [(1, 8), (7, 8), (33, 40), (257, 72), (1024, 64), (4099, 520), (2 * 128 * 4 + 3, 16)]


def _L():
    from distributed_training_amd import _lib as L

    return L


def _put(t, dev):
    v = B.guarded(t.numel(), t.dtype, dev, 0)
    v.copy_(t.reshape(-1))
    return v


def _fork_inputs(R, C):
    inp = B.exact_inputs(R, C)
    inp["dy_b"] = B.exact_inputs(R, C, seed=B.exact_seed(R, C) + 104729)["dy"]
    return inp


def _launch(inp, dev, with_y, fork=True, entry="fork"):
    """one launch on guarded buffers -> dict of device views (x, dy, dy_b, y as [R, C]; ws as [P, C, 2]; g)"""
    L = _L()
    lib, stream = L.lib(), L.stream_ptr(dev)
    R, C = inp["x"].shape
    P = L.check(lib.gs_bn_bwd_partials(R, C), "gs_bn_bwd_partials")
    names = ["x", "dy"] + (["dy_b"] if fork else []) + (["y"] if with_y else [])
    d = {k: _put(inp[k], dev) for k in names}
    d["mean"] = _put(inp["mean"], dev)
    ws = B.guarded(P * C * 2, F32, dev)
    ws.fill_(float("nan"))
    g = B.guarded(R * C, BF16, dev)
    snap = {k: B.bits(v).clone() for k, v in d.items()}
    yp = d["y"].data_ptr() if with_y else None
    if entry == "fork":
        bp = d["dy_b"].data_ptr() if fork else None
        rc = lib.gs_bn_bwd_reduce_fork(d["x"].data_ptr(), d["dy"].data_ptr(), bp, yp, g.data_ptr(), d["mean"].data_ptr(),
                                       ws.data_ptr(), ws.numel(), R, C, stream)
    else:
        rc = lib.gs_bn_bwd_reduce(d["x"].data_ptr(), d["dy"].data_ptr(), yp, g.data_ptr(), d["mean"].data_ptr(),
                                  ws.data_ptr(), ws.numel(), R, C, stream)
    L.check(rc, "gs_bn_bwd_reduce_fork")
    torch.cuda.synchronize()
    for k, v in list(d.items()) + [("ws", ws), ("g", g)]:
        assert B.guards_intact(v), f"the launch wrote outside {k}"
    for k, v in d.items():
        assert torch.equal(B.bits(v), snap[k]), f"the launch changed its input {k}"
    out = {k: (v.view(R, C) if k != "mean" else v) for k, v in d.items()}
    out.update(ws=ws.view(P, C, 2), g=g.view(R, C), P=P)
    return out


# ---- A. the exact grid ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FORK_SHAPES, ids=B.shape_id)
@pytest.mark.parametrize("with_y", [True, False], ids=["relu", "plain"])
def test_exact_fork_reduce(cuda_device, with_y, shape):
    inp = _fork_inputs(*shape)
    run = _launch(inp, cuda_device, with_y)
    dy = run["dy"] + run["dy_b"]  # ATen's bf16 add on the device
    assert torch.equal(dy.double(), run["dy"].double() + run["dy_b"].double())  # the grid: the sum is a bf16
    want = torch.ops.aten.threshold_backward(dy, run["y"], 0) if with_y else dy
    bad = torch.nonzero(B.bits(run["g"]) != B.bits(want))
    assert bad.numel() == 0, (bad.shape[0], bad[:4].tolist())
    ws = run["ws"]
    assert not bool(torch.isnan(ws).any()), "a partial of the workspace was never written"
    zeros = torch.zeros_like(run["mean"])
    g, sum_g, sum_gx, _, _, _ = B.bn_bwd_ref(run["x"], dy, run["y"] if with_y else None, run["mean"], zeros, zeros)
    # exactness of the grid for these inputs: multiples of 1/8 whose magnitudes sum below 2^24 / 8
    xc = run["x"].double() - run["mean"].double()
    assert float(g.abs().sum(0).max()) * 8 < 2 ** 24 and float((g * xc).abs().sum(0).max()) * 8 < 2 ** 24
    assert torch.equal(B.bits(run["g"]), B.bf16_bits(g))
    got = ws.double().sum(0)
    assert torch.equal(got[:, 0], sum_g), torch.nonzero(got[:, 0] != sum_g).flatten()[:8]
    assert torch.equal(got[:, 1], sum_gx), torch.nonzero(got[:, 1] != sum_gx).flatten()[:8]


# ---- B. special values ------------------------------------------------------------------------------
# (dy_a, dy_b) as bf16 patterns
SUM_PAIRS = [
    (0x3F80, 0x3B80),  # 1 + 2^-8: a tie, to even 1.0
    (0x3F81, 0x3B80),  # 1.0078125 + 2^-8: a tie, to even 1.015625 (odd parity: rounds up)
    (0xBF80, 0xBB80),  # the negative ties
    (0xBF81, 0xBB80),
    (0x4000, 0xBB80),  # 2 - 2^-8: a tie from a negative operand
    (0x7F61, 0x7F61),  # 3e38 + 3e38: the fp32 sum is Inf
    (0x7F7F, 0x7B00),  # max bf16 + half its ulp: finite in fp32, rounds to Inf
    (0xFF7F, 0xFB00),  # the same, negative
    (0x7F80, 0xFF80),  # Inf - Inf
    (0x7F80, 0x3F80),  # Inf + 1
    (0x7FC0, 0x3F80),  # NaN + 1
    (0x3F80, 0xFFC1),  # 1 + a NaN with a payload and a sign
    (0x0000, 0x0000),  # +0 + +0
    (0x8000, 0x8000),  # -0 + -0
    (0x0000, 0x8000),  # +0 + -0
    (0x3FC0, 0xBFC0),  # x + (-x)
    (0x0001, 0x0001),  # the smallest subnormals
    (0x0040, 0x0020),  # 2^-127 + 2^-128: a subnormal sum
    (0x8040, 0x8020),
    (0x0080, 0x8040),  # 2^-126 - 2^-127: normal operands, subnormal sum
    (0x3FC0, 0x4010),  # 1.5 + 2.25
    (0xC040, 0x3F80),  # -3 + 1
]
Y_VALUES = [0x3F80, 0xBF80, 0x0000, 0x8000, 0x7FC0]


@pytest.mark.parametrize("with_y", [True, False], ids=["relu", "plain"])
def test_fork_special_values_equal_aten(cuda_device, with_y):
    cases = [(a, b, y) for y in Y_VALUES for a, b in SUM_PAIRS]
    C = 8
    R = -(-len(cases) // C)
    cases += [(0x3F80, 0x3F80, 0x3F80)] * (R * C - len(cases))
    inp = dict(x=torch.zeros(R, C, dtype=BF16), mean=torch.zeros(C),
               dy=B.from_bits([c[0] for c in cases]).view(R, C), dy_b=B.from_bits([c[1] for c in cases]).view(R, C),
               y=B.from_bits([c[2] for c in cases]).view(R, C))
    run = _launch(inp, cuda_device, with_y)
    dy = run["dy"] + run["dy_b"]
    want = torch.ops.aten.threshold_backward(dy, run["y"], 0) if with_y else dy
    got, ref = B.bits(run["g"]).flatten().tolist(), B.bits(want).flatten().tolist()
    bad = [tuple(hex(v & 0xFFFF) for v in c + (a, b)) for c, a, b in zip(cases, got, ref) if a != b]
    assert not bad, f"(dy_a, dy_b, y, kernel, ATen): {bad}"
    # and in the contract's own words for a few of them
    by = {c: a & 0xFFFF for c, a in zip(cases, got)}
    pos = 0x3F80 if with_y else 0xBF80  # without y the mask is absent: any y gives the sum
    assert by[(0x3F80, 0x3B80, pos)] == 0x3F80 and by[(0x3F81, 0x3B80, pos)] == 0x3F82
    assert by[(0x7F7F, 0x7B00, pos)] == 0x7F80 and by[(0xFF7F, 0xFB00, pos)] == 0xFF80
    assert (by[(0x7F80, 0xFF80, pos)] & 0x7FFF) == 0x7FC0 and by[(0x0040, 0x0020, pos)] == 0x0060
    if with_y:
        assert by[(0x7FC0, 0x3F80, 0xBF80)] == 0 and by[(0x7FC0, 0x3F80, 0x8000)] == 0  # masked, NaN or not
        assert by[(0x3FC0, 0x4010, 0x7FC0)] == 0x4070  # a NaN y passes the sum


# ---- C. one gradient ---------------------------------------------------------------------------------
def test_without_dy_b_it_is_the_existing_entry(cuda_device):
    inp = _fork_inputs(257, 72)
    a = _launch(inp, cuda_device, True, fork=False, entry="fork")
    b = _launch(inp, cuda_device, True, fork=False, entry="plain")
    assert torch.equal(B.bits(a["ws"]), B.bits(b["ws"])) and torch.equal(B.bits(a["g"]), B.bits(b["g"]))
    assert not bool(torch.isnan(a["ws"]).any())
