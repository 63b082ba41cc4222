"""The channel tile of the BatchNorm backward passes (csrc/gs_bn_kernels.hip, bn_geom): tx = min(32,
pow2ceil(C / 8)) vectors, ty = max(32, 256 / tx) rows per step, tx * ty threads (512 at C = 128, 1024
from C = 256 on).  All six entries, called directly, against the fp64 reference of tests/_bn_ref.py on its
exact grid, where every sum the kernels form is exact in fp32 in any order: a row, vector, partial or
group of the LDS fold that is dropped, doubled or taken from the wrong place changes a bit.

    gs_bn_bwd_reduce (no y; y; y and g_out), gs_bn_bwd_reduce_bits (without and with g_out),
    gs_bn_bwd_reduce_fork, gs_bn_bwd_reduce_fork_bits, gs_bn_bwd_dx (no y; y; fed g), gs_bn_bwd_dx_bits

* the workspace's partials add up to the reference's sums bit for bit and every partial was written (the
  workspace is exactly P * C * 2 floats, prefilled with NaN); g_out is the reference's g;
* grad_weight, grad_bias bitwise; dx is the truncated reference bitwise where R is a power of two, and
  for every R the three ways to the same dx (y, bits, g) agree bitwise;
* every buffer is a guarded view: guards intact and inputs bitwise unchanged after each launch;
* two runs are bitwise equal.

Shapes: C = 128 (a 16-vector tile, 512 threads), 248 (31 of 32 vectors), 256 (exactly one tile), 264 (a
second tile with one live vector), 520 (three tiles, the last with one live vector); R = 1, 31, 32, 33 (one
step of rows less one, exactly, plus one) and 4 * 32 * 2 + 3 = 259; 4096 x 256 (45 row-blocks: the dx
pass's fold of the partials wraps its 8 groups); 33000 x 264 (128 row-blocks of 258 rows: two unrolled
iterations and a ragged tail step in every thread); 8192 x 512 (64 row-blocks of 128 rows: with two
32-vector tiles the grid would have 128 workgroups, fewer than the chip has CUs, so bn_geom halves the tile
to four 16-vector tiles in 512-thread workgroups, as it does at 50176 x 256 and 12544 x 512 of ResNet-50).
tests/test_bn_tile_cpu.py asserts that the grid is exact at each of them.
"""
import functools

import pytest
import torch

from tests import _bn_ref as B

pytestmark = pytest.mark.gpu

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
TILE_C = [128, 248, 256, 264, 520]
TILE_R = [1, 31, 32, 33, 4 * 32 * 2 + 3]
TILE_SHAPES = [(R, C) for C in TILE_C for R in TILE_R] + [(4096, 256), (33000, 264), (8192, 512)]
GUARD = 0xA5


def tile_inputs(R, C):
    """exact_inputs plus the second half of a fork's gradient (same grid: the bf16 sum of the halves is
    exact, a multiple of 0.25 in [-4, 4]) and the mask bytes of y (bit j of byte i = !(y[8 i + j] <= 0))"""
    inp = B.exact_inputs(R, C)
    inp["dy_b"] = B.exact_inputs(R, C, seed=B.exact_seed(R, C) + 1)["dy"]
    keep = ~(inp["y"].float().reshape(-1, 8) <= 0)
    inp["mask"] = (keep.to(torch.int32) << torch.arange(8, dtype=torch.int32)).sum(1).to(U8)
    return inp


def _L():
    from distributed_training_amd import _lib as L

    return L


def _put(t, dev):
    v = B.guarded(t.numel(), t.dtype, dev, 0)
    v.copy_(t.reshape(-1))
    return v


def _bytes(t, dev):
    """the bytes of t between two 4 KiB guards of 0xA5, at an odd address (the mask needs no alignment)"""
    n = t.numel()
    raw = torch.full((B.GUARD_BYTES + B.LINE_BYTES + 1 + n + B.GUARD_BYTES,), GUARD, dtype=U8, device=dev)
    start = B.GUARD_BYTES
    while (raw.data_ptr() + start) % B.LINE_BYTES:
        start += 1
    start += 1
    view = raw[start:start + n]
    view.copy_(t)
    view._guard = (raw, start, n)
    return view


def _intact(v):
    if v.dtype != U8:
        return B.guards_intact(v)
    raw, start, n = v._guard
    return bool((raw[:start] == GUARD).all()) and bool((raw[start + n:] == GUARD).all())


def _raw(v):
    return v if v.dtype == U8 else B.bits(v)


def _run_all(shape, dev):
    """every entry once on the shape's inputs -> {name: output tensors}; guards and inputs checked per launch"""
    L = _L()
    lib, stream = L.lib(), L.stream_ptr(dev)
    R, C = shape
    inp = tile_inputs(R, C)
    P = L.check(lib.gs_bn_bwd_partials(R, C), "gs_bn_bwd_partials")
    d = {k: _put(inp[k], dev) for k in ("x", "dy", "dy_b", "y", "mean", "invstd", "weight")}
    d["mask"] = _bytes(inp["mask"], dev)
    snap = {k: _raw(v).clone() for k, v in d.items()}
    p = {k: v.data_ptr() for k, v in d.items()}
    outs = {}

    def verify(what, frozen=()):
        torch.cuda.synchronize()
        for k, v in list(d.items()) + [(f"{n}.{k}", v) for n, o in outs.items() for k, v in o.items()]:
            assert _intact(v), f"{what} wrote outside {k}"
        for k, v in d.items():
            assert torch.equal(_raw(v), snap[k]), f"{what} changed its input {k}"
        for n, k in frozen:
            assert torch.equal(B.bits(outs[n][k]), snap[(n, k)]), f"{what} changed {n}.{k}"

    def reduce(name, fn, *args, g):
        o = dict(ws=B.guarded(P * C * 2, F32, dev))
        o["ws"].fill_(float("nan"))
        if g:
            o["g"] = B.guarded(R * C, BF16, dev)
        outs[name] = o
        gp = o["g"].data_ptr() if g else None
        L.check(getattr(lib, fn)(p["x"], *args, gp, p["mean"], o["ws"].data_ptr(), o["ws"].numel(), R, C, stream), fn)
        verify(f"{fn} ({name})")
        for k, v in o.items():
            snap[(name, k)] = B.bits(v).clone()

    reduce("r_plain", "gs_bn_bwd_reduce", p["dy"], None, g=False)
    reduce("r_y", "gs_bn_bwd_reduce", p["dy"], p["y"], g=False)
    reduce("r_y_g", "gs_bn_bwd_reduce", p["dy"], p["y"], g=True)
    reduce("r_bits", "gs_bn_bwd_reduce_bits", p["dy"], p["mask"], g=False)
    reduce("r_bits_g", "gs_bn_bwd_reduce_bits", p["dy"], p["mask"], g=True)
    reduce("r_fork", "gs_bn_bwd_reduce_fork", p["dy"], p["dy_b"], p["y"], g=True)
    reduce("r_fork_bits", "gs_bn_bwd_reduce_fork_bits", p["dy"], p["dy_b"], p["mask"], g=True)

    def dx(name, fn, src, dyp, mp):
        o = dict(dx=B.guarded(R * C, BF16, dev), gw=B.guarded(C, F32, dev), gb=B.guarded(C, F32, dev))
        outs[name] = o
        ws = outs[src]["ws"]
        L.check(getattr(lib, fn)(p["x"], dyp, mp, p["mean"], p["invstd"], p["weight"], ws.data_ptr(), ws.numel(),
                                 o["dx"].data_ptr(), o["gw"].data_ptr(), o["gb"].data_ptr(), R, C, stream), fn)
        verify(f"{fn} ({name})", frozen=[(src, k) for k in outs[src]])  # neither the workspace nor g changes

    dx("d_plain", "gs_bn_bwd_dx", "r_plain", p["dy"], None)
    dx("d_y", "gs_bn_bwd_dx", "r_y", p["dy"], p["y"])
    dx("d_bits", "gs_bn_bwd_dx_bits", "r_bits", p["dy"], p["mask"])
    dx("d_g", "gs_bn_bwd_dx", "r_y_g", outs["r_y_g"]["g"].data_ptr(), None)
    return dict(P=P, d=d, outs=outs)


@functools.lru_cache(maxsize=None)
def _case(shape, dev):
    """the shape's run and its three references (fp64 on the device): no mask, the mask, the fork's sum + mask"""
    run = _run_all(shape, dev)
    R, C = shape
    t = {k: (v.view(R, C) if k in ("x", "dy", "dy_b", "y") else v) for k, v in run["d"].items()}
    fork_dy = (t["dy"].float() + t["dy_b"].float()).to(BF16)  # ATen's bf16 add: fp32, rounded once
    assert torch.equal(fork_dy.double(), t["dy"].double() + t["dy_b"].double())  # exact on this grid
    ref = {"plain": B.bn_bwd_ref(t["x"], t["dy"], None, t["mean"], t["invstd"], t["weight"]),
           "relu": B.bn_bwd_ref(t["x"], t["dy"], t["y"], t["mean"], t["invstd"], t["weight"]),
           "fork": B.bn_bwd_ref(t["x"], fork_dy, t["y"], t["mean"], t["invstd"], t["weight"])}
    return run, ref


REDUCES = [("r_plain", "plain"), ("r_y", "relu"), ("r_y_g", "relu"), ("r_bits", "relu"), ("r_bits_g", "relu"),
           ("r_fork", "fork"), ("r_fork_bits", "fork")]
DXS = [("d_plain", "plain"), ("d_y", "relu"), ("d_bits", "relu"), ("d_g", "relu")]


@pytest.mark.parametrize("shape", TILE_SHAPES, ids=B.shape_id)
def test_reduce_sums_and_g_bitwise(cuda_device, shape):
    run, ref = _case(shape, cuda_device)
    R, C = shape
    for name, variant in REDUCES:
        g, sum_g, sum_gx, _, _, _ = ref[variant]
        o = run["outs"][name]
        ws = o["ws"].view(run["P"], C, 2)
        assert not bool(torch.isnan(ws).any()), f"{name}: a partial of the workspace was never written"
        got = ws.double().sum(0)
        assert torch.equal(got[:, 0], sum_g), (name, torch.nonzero(got[:, 0] != sum_g).flatten()[:8].tolist())
        assert torch.equal(got[:, 1], sum_gx), (name, torch.nonzero(got[:, 1] != sum_gx).flatten()[:8].tolist())
        if "g" in o:
            bad = torch.nonzero(B.bits(o["g"].view(R, C)) != B.bf16_bits(g))
            assert bad.numel() == 0, (name, bad.shape[0], bad[:4].tolist())


@pytest.mark.parametrize("shape", TILE_SHAPES, ids=B.shape_id)
def test_dx_and_parameter_gradients_bitwise(cuda_device, shape):
    run, ref = _case(shape, cuda_device)
    R, C = shape
    for name, variant in DXS:
        _, sum_g, _, gw, _, dx = ref[variant]
        o = run["outs"][name]
        assert torch.equal(B.bits(o["gb"]), B.bits(sum_g.float())), (name, "grad_bias")
        assert torch.equal(B.bits(o["gw"]), B.bits(gw.float())), (name, "grad_weight")
        got = o["dx"].view(R, C)
        assert not bool((B.bits(got) == 0x7FC1).any()), f"{name}: an element of dx was never written"
        if R & (R - 1) == 0:
            bad = torch.nonzero(B.bits(got) != B.bits(B.trunc_bf16(dx)))
            assert bad.numel() == 0, (name, bad.shape[0], bad[:4].tolist())
    for name in ("d_bits", "d_g"):  # the same sums and the same g by another way: the same arithmetic
        assert torch.equal(B.bits(run["outs"][name]["dx"]), B.bits(run["outs"]["d_y"]["dx"])), name


@pytest.mark.parametrize("shape", [(259, 128), (259, 264), (4096, 256)], ids=B.shape_id)
def test_two_runs_are_bitwise_equal(cuda_device, shape):
    a, _ = _case(shape, cuda_device)
    b = _run_all(shape, cuda_device)
    for name, o in a["outs"].items():
        for k, v in o.items():
            assert torch.equal(B.bits(v), B.bits(b["outs"][name][k])), (name, k)
