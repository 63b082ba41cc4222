"""The ReLU mask as bits, through the C entry points (include/gsync.h).

The mask of n bf16 elements is n / 8 bytes: byte i belongs to the 16-byte vector i, bit j is set iff
!(v[8 i + j] <= 0).  Every buffer sits between guards; the mask buffer is exactly n / 8 bytes at an odd
address (it needs no alignment) and every case runs with the mask prefilled with 0x00 and with 0xFF, so a
byte that is never written shows.

A. gs_relu_mask_fwd / gs_add_relu_mask_fwd: the output is bitwise torch.relu_ / gs_add_relu_fwd on the same
   input, the mask equals the bits packed on the host from ~(out <= 0); sizes around one workgroup's
   kBlock * kBnUnroll vectors, and every pair of special values;
B. gs_relu_maxpool_mask_fwd: pooled and idx are bitwise gs_relu_maxpool_fwd's, the mask is the packed
   ~(y <= 0) of the un-ReLU'd input, odd heights and widths included;
C. gs_bn_bwd_reduce_bits (without and with g), gs_bn_bwd_reduce_fork_bits and gs_bn_bwd_dx_bits fed the mask
   packed from y on the host: the workspace, g, dx, grad_weight and grad_bias are bitwise what the
   y-taking entries write on the same inputs (tests/test_gpu_bn_kernels.py and test_gpu_bn_fork.py pin those
   to fp64); inputs and mask come back unchanged.
"""
import functools

import pytest
import torch

from tests import _bn_ref as B

pytestmark = pytest.mark.gpu

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
WG_VECS = 256 * 4  # kBlock * kBnUnroll: the vectors of one workgroup of the flat grid
GUARD = 0xA5
PREFILLS = [0x00, 0xFF]


def _L():
    from distributed_training_amd import _lib as L

    return L


def _put(t, dev):
    v = B.guarded(t.numel(), t.dtype, dev, 0)
    v.copy_(t.reshape(-1))
    return v


def _bytes(n, dev, fill, offset=0):
    """n bytes between two 4 KiB guards of 0xA5, starting `offset` bytes past a 128-byte line"""
    raw = torch.full((B.GUARD_BYTES + B.LINE_BYTES + offset + n + B.GUARD_BYTES,), GUARD, dtype=U8, device=dev)
    start = B.GUARD_BYTES
    while (raw.data_ptr() + start) % B.LINE_BYTES:
        start += 1
    start += offset
    view = raw[start:start + n]
    view.fill_(fill)
    view._guard = (raw, start, n)
    return view


def _bytes_intact(view):
    raw, start, n = view._guard
    return bool((raw[:start] == GUARD).all()) and bool((raw[start + n:] == GUARD).all())


def pack_mask(v):
    """the mask bytes of a bf16 tensor, packed on the host: bit j of byte i = !(v[8 i + j] <= 0)"""
    keep = ~(v.detach().cpu().float().reshape(-1, 8) <= 0)
    return (keep.to(torch.int32) << torch.arange(8, dtype=torch.int32)).sum(1).to(U8)


def test_pack_mask_in_the_contract_s_words():
    v = B.from_bits([0x3F80, 0xBF80, 0x0000, 0x8000, 0x7FC0, 0xFFC1, 0x0001, 0x8001])  # 1 -1 +0 -0 NaN -NaN sub -sub
    assert pack_mask(v).tolist() == [0b01110001]


# ---- A. relu + mask, add + relu + mask -----------------------------------------------------------------
def _tail(kind, t_cpu, id_cpu, dev, prefill):
    """the mask-writing tail and its sibling on the same input -> (out, want, mask) on the host"""
    L = _L()
    lib, stream = L.lib(), L.stream_ptr(dev)
    n = t_cpu.numel()
    t, ref = _put(t_cpu, dev), _put(t_cpu, dev)
    mask = _bytes(n // 8, dev, prefill, offset=3)
    if kind == "relu":
        L.check(lib.gs_relu_mask_fwd(t.data_ptr(), mask.data_ptr(), n, stream), "gs_relu_mask_fwd")
        torch.relu_(ref)
        ins = []
    else:
        idn = _put(id_cpu, dev)
        snap = B.bits(idn).clone()
        L.check(lib.gs_add_relu_mask_fwd(t.data_ptr(), idn.data_ptr(), mask.data_ptr(), n, stream),
                "gs_add_relu_mask_fwd")
        L.check(lib.gs_add_relu_fwd(ref.data_ptr(), idn.data_ptr(), n, stream), "gs_add_relu_fwd")
        ins = [(idn, snap)]
    torch.cuda.synchronize()
    assert B.guards_intact(t) and B.guards_intact(ref) and _bytes_intact(mask), "a store outside a buffer"
    for v, snap in ins:
        assert B.guards_intact(v) and torch.equal(B.bits(v), snap), "the identity changed"
    return t.cpu(), ref.cpu(), mask.cpu()


def _check_tail(out, want, mask):
    bad = torch.nonzero(B.bits(out) != B.bits(want)).flatten()
    assert bad.numel() == 0, (bad.numel(), bad[:8].tolist())
    ref = pack_mask(out)
    bad = torch.nonzero(mask != ref).flatten()
    assert bad.numel() == 0, (bad.numel(), [(int(i), int(mask[i]), int(ref[i])) for i in bad[:8]])


@pytest.mark.parametrize("prefill", PREFILLS, ids=["zeros", "ones"])
@pytest.mark.parametrize("nvec", [1, WG_VECS - 1, WG_VECS, WG_VECS + 1, 3 * WG_VECS + 5])
@pytest.mark.parametrize("kind", ["relu", "add_relu"])
def test_tail_output_and_mask(cuda_device, kind, nvec, prefill):
    gen = torch.Generator().manual_seed(1000 + nvec)
    t = torch.randn(nvec * 8, generator=gen).to(BF16)
    idn = torch.randn(nvec * 8, generator=gen).to(BF16)
    t[torch.rand(nvec * 8, generator=gen) < 0.1] = 0.0
    if kind == "add_relu":
        idn[::7] = -t[::7]  # sums that are exactly zero
    out, want, mask = _tail(kind, t, idn, cuda_device, prefill)
    _check_tail(out, want, mask)
    assert 0 < int(pack_mask(out).to(torch.int32).sum()) < 255 * nvec  # neither all clear nor all set


# +0, -0, +Inf, -Inf, NaN, the smallest positive / negative subnormal and normal, and two ordinary values
SPECIALS = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x0001, 0x8001, 0x0080, 0x8080, 0x3FC0, 0xBFC0]


@pytest.mark.parametrize("prefill", PREFILLS, ids=["zeros", "ones"])
@pytest.mark.parametrize("kind", ["relu", "add_relu"])
def test_tail_special_values(cuda_device, kind, prefill):
    pairs = [(a, b) for a in SPECIALS for b in SPECIALS]
    pairs += [(0x3F80, 0x3F80)] * (-len(pairs) % 8)
    t, idn = B.from_bits([p[0] for p in pairs]), B.from_bits([p[1] for p in pairs])
    out, want, mask = _tail(kind, t, idn, cuda_device, prefill)
    _check_tail(out, want, mask)
    got = {p: (int(o) & 0xFFFF, (int(mask[i // 8]) >> (i % 8)) & 1) for i, (p, o) in enumerate(zip(pairs, B.bits(out)))}
    if kind == "relu":  # the second value of the pair plays no part
        assert got[(0x8000, 0x0000)] == (0x0000, 0) and got[(0xFF80, 0x0000)] == (0x0000, 0)  # -0 -> +0, -Inf -> +0
        assert got[(0x7FC0, 0x0000)] == (0x7FC0, 1) and got[(0x7F80, 0x0000)] == (0x7F80, 1)  # NaN stays, bit set
        assert got[(0x0001, 0x0000)] == (0x0001, 1) and got[(0x8001, 0x0000)] == (0x0000, 0)
    else:
        assert got[(0x7F80, 0xFF80)][1] == 1 and (got[(0x7F80, 0xFF80)][0] & 0x7FC0) == 0x7FC0  # Inf - Inf: NaN
        assert got[(0x3FC0, 0xBFC0)] == (0x0000, 0) and got[(0x0001, 0x8001)] == (0x0000, 0)  # sums to +0
        assert got[(0x8000, 0x8000)][1] == 0 and got[(0x0000, 0x8000)] == (0x0000, 0)  # -0 + -0 = -0: bit clear
        assert got[(0x0001, 0x0001)] == (0x0002, 1) and got[(0x8080, 0x0001)][1] == 0


# ---- B. the stem ------------------------------------------------------------------------------------------
STEM_SHAPES = [(1, 1, 1, 8), (2, 5, 3, 8), (1, 7, 7, 16), (2, 8, 8, 64), (1, 9, 4, 64)]  # (N, H, W, C)


@pytest.mark.parametrize("prefill", PREFILLS, ids=["zeros", "ones"])
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_pool_and_mask(cuda_device, shape, prefill):
    L = _L()
    lib, stream, dev = L.lib(), L.stream_ptr(cuda_device), cuda_device
    N, H, W, C = shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    n, on = N * H * W * C, N * OH * OW * C
    gen = torch.Generator().manual_seed(2000 + n)
    y_cpu = torch.randn(n, generator=gen).to(BF16)
    y_cpu[torch.rand(n, generator=gen) < 0.1] = 0.0
    y_cpu[torch.rand(n, generator=gen) < 0.05] = -0.0
    y_cpu[torch.rand(n, generator=gen) < 0.05] = float("nan")
    y = _put(y_cpu, dev)
    snap = B.bits(y).clone()
    pooled, pooled_ref = B.guarded(on, BF16, dev), B.guarded(on, BF16, dev)
    idx, idx_ref = _bytes(on, dev, 0xEE), _bytes(on, dev, 0xEE)
    mask = _bytes(n // 8, dev, prefill, offset=5)
    L.check(lib.gs_relu_maxpool_mask_fwd(y.data_ptr(), pooled.data_ptr(), idx.data_ptr(), mask.data_ptr(), N, H, W, C,
                                         stream), "gs_relu_maxpool_mask_fwd")
    L.check(lib.gs_relu_maxpool_fwd(y.data_ptr(), pooled_ref.data_ptr(), idx_ref.data_ptr(), N, H, W, C, stream),
            "gs_relu_maxpool_fwd")
    torch.cuda.synchronize()
    for k, v in (("y", y), ("pooled", pooled), ("pooled_ref", pooled_ref)):
        assert B.guards_intact(v), f"a store outside {k}"
    for k, v in (("idx", idx), ("idx_ref", idx_ref), ("mask", mask)):
        assert _bytes_intact(v), f"a store outside {k}"
    assert torch.equal(B.bits(y), snap), "the input changed"
    assert torch.equal(B.bits(pooled), B.bits(pooled_ref)) and torch.equal(idx, idx_ref)
    assert int(idx.max()) <= 8
    got, ref = mask.cpu(), pack_mask(y_cpu)
    bad = torch.nonzero(got != ref).flatten()
    assert bad.numel() == 0, (bad.numel(), [(int(i), int(got[i]), int(ref[i])) for i in bad[:8]])


# ---- C. the backward from bits ------------------------------------------------------------------------------
# one row; tx = 1 (C = 8), 4 (24), 8 with dead vectors (40), two tiles with a ragged one (72), nine tiles (520);
# a ragged last row-block; tail steps of the unrolled loop; P past the fold's 64 groups (12544 x 64: P = 79);
# many tiles with few rows (196 x 2048)
BWD_SHAPES = [(1, 8), (2, 8), (147, 8), (30, 24), (37, 40), (300, 72), (513, 520), (4099, 64), (6272, 64),
              (12544, 64), (196, 2048)]
# tx = 2 is C = 16: test_gpu_bn_fork.py's shape with unrolled iterations plus a tail at ty = 128
BWD_SHAPES_ALL = BWD_SHAPES + [(2 * 128 * 4 + 3, 16)]


@functools.lru_cache(maxsize=None)
def _inputs(R, C):
    """random_inputs with NaN and signed zeros of y in known positions, a second gradient, the packed mask"""
    inp = B.random_inputs(R, C, seed=31 * R + C)
    y = inp["y"].reshape(-1)
    n = y.numel()
    y[0] = float("nan")
    y[n - 1] = -0.0
    y[n // 2] = 0.0
    y[(n // 3) | 1] = -float("nan")
    y[5 % n] = -0.0
    inp["dy_b"] = B.random_inputs(R, C, seed=31 * R + C + 7)["dy"]
    inp["mask"] = pack_mask(inp["y"])
    return inp


def _upload(inp, dev, names):
    d = {k: _put(inp[k], dev) for k in names}
    R, C = inp["x"].shape
    d["mask"] = _bytes(R * C // 8, dev, 0, offset=1)
    d["mask"].copy_(inp["mask"])
    snap = {k: (v.clone() if v.dtype == U8 else B.bits(v).clone()) for k, v in d.items()}
    return d, snap


def _after(d, snap, outs):
    torch.cuda.synchronize()
    for k, v in list(d.items()) + list(outs.items()):
        ok = _bytes_intact(v) if v.dtype == U8 else B.guards_intact(v)
        assert ok, f"the launch wrote outside {k}"
    for k, v in d.items():
        assert torch.equal(v if v.dtype == U8 else B.bits(v), snap[k]), f"the launch changed its input {k}"


def _same(a, b, what):
    bad = torch.nonzero(B.bits(a) != B.bits(b)).flatten()
    assert bad.numel() == 0, (what, bad.numel(), bad[:8].tolist())


@pytest.mark.parametrize("shape", BWD_SHAPES_ALL, ids=B.shape_id)
@pytest.mark.parametrize("form", ["sums", "with_g", "fork"])
def test_reduce_from_bits_equals_reduce_from_y(cuda_device, form, shape):
    L = _L()
    lib, stream, dev = L.lib(), L.stream_ptr(cuda_device), cuda_device
    R, C = shape
    inp = _inputs(R, C)
    P = L.check(lib.gs_bn_bwd_partials(R, C), "gs_bn_bwd_partials")
    d, snap = _upload(inp, dev, ["x", "dy", "y", "mean"] + (["dy_b"] if form == "fork" else []))
    ws = {k: B.guarded(P * C * 2, F32, dev) for k in ("y", "bits")}
    g = {k: (B.guarded(R * C, BF16, dev) if form != "sums" else None) for k in ("y", "bits")}
    for v in ws.values():
        v.fill_(float("nan"))
    gp = {k: (v.data_ptr() if v is not None else None) for k, v in g.items()}
    x, dy, mean = d["x"].data_ptr(), d["dy"].data_ptr(), d["mean"].data_ptr()
    if form == "fork":
        dyb = d["dy_b"].data_ptr()
        L.check(lib.gs_bn_bwd_reduce_fork(x, dy, dyb, d["y"].data_ptr(), gp["y"], mean, ws["y"].data_ptr(),
                                          ws["y"].numel(), R, C, stream), "gs_bn_bwd_reduce_fork")
        L.check(lib.gs_bn_bwd_reduce_fork_bits(x, dy, dyb, d["mask"].data_ptr(), gp["bits"], mean,
                                               ws["bits"].data_ptr(), ws["bits"].numel(), R, C, stream),
                "gs_bn_bwd_reduce_fork_bits")
    else:
        L.check(lib.gs_bn_bwd_reduce(x, dy, d["y"].data_ptr(), gp["y"], mean, ws["y"].data_ptr(), ws["y"].numel(), R,
                                     C, stream), "gs_bn_bwd_reduce")
        L.check(lib.gs_bn_bwd_reduce_bits(x, dy, d["mask"].data_ptr(), gp["bits"], mean, ws["bits"].data_ptr(),
                                          ws["bits"].numel(), R, C, stream), "gs_bn_bwd_reduce_bits")
    outs = {f"ws_{k}": v for k, v in ws.items()}
    outs.update({f"g_{k}": v for k, v in g.items() if v is not None})
    _after(d, snap, outs)
    assert not bool(torch.isnan(ws["y"]).any()), "a partial of the workspace was never written"
    _same(ws["bits"], ws["y"], "workspace")
    if form != "sums":
        _same(g["bits"], g["y"], "g")


@pytest.mark.parametrize("shape", BWD_SHAPES_ALL, ids=B.shape_id)
def test_dx_from_bits_equals_dx_from_y(cuda_device, shape):
    L = _L()
    lib, stream, dev = L.lib(), L.stream_ptr(cuda_device), cuda_device
    R, C = shape
    inp = _inputs(R, C)
    P = L.check(lib.gs_bn_bwd_partials(R, C), "gs_bn_bwd_partials")
    d, snap = _upload(inp, dev, ["x", "dy", "y", "mean", "invstd", "weight"])
    ws = B.guarded(P * C * 2, F32, dev)
    x, dy, mean = d["x"].data_ptr(), d["dy"].data_ptr(), d["mean"].data_ptr()
    L.check(lib.gs_bn_bwd_reduce(x, dy, d["y"].data_ptr(), None, mean, ws.data_ptr(), ws.numel(), R, C, stream),
            "gs_bn_bwd_reduce")
    torch.cuda.synchronize()
    d["ws"], snap["ws"] = ws, B.bits(ws).clone()
    out = {k: dict(dx=B.guarded(R * C, BF16, dev), gw=B.guarded(C, F32, dev), gb=B.guarded(C, F32, dev))
           for k in ("y", "bits")}
    for fn, key, m in (("gs_bn_bwd_dx", "y", d["y"]), ("gs_bn_bwd_dx_bits", "bits", d["mask"])):
        o = out[key]
        L.check(getattr(lib, fn)(x, dy, m.data_ptr(), mean, d["invstd"].data_ptr(), d["weight"].data_ptr(),
                                 ws.data_ptr(), ws.numel(), o["dx"].data_ptr(), o["gw"].data_ptr(),
                                 o["gb"].data_ptr(), R, C, stream), fn)
    _after(d, snap, {f"{n}_{k}": v for k, o in out.items() for n, v in o.items()})
    for n in ("dx", "gw", "gb"):
        _same(out["bits"][n], out["y"][n], n)
    assert not bool((B.bits(out["y"]["dx"]) == 0x7FC1).all()), "dx was never written"
