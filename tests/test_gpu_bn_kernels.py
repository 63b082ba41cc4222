"""gs_bn_bwd_reduce / gs_bn_bwd_dx / gs_add_relu_fwd called directly (include/gsync.h), against the
fp64 reference of tests/_bn_ref.py.  The caller chooses mean, invstd and weight, so:

A. on the exact grid (_bn_ref.exact_inputs: every sum exact in fp32 in any order) the workspace's
   sums, grad_weight, grad_bias and g_out equal the reference bit for bit, and so does the truncated
   dx where R is a power of two; a dropped or doubled row, tail step or partial, a channel taken from
   the wrong place in mean / invstd / weight, cannot hide behind rounding noise;
B. on random data every element of dx, and grad_weight / grad_bias per channel, stay within bounds
   derived from the kernels' operation count (below), and |dx| never exceeds |truth| + E: truncation;
C. special values: the mask against ATen's threshold_backward, gs_add_relu_fwd against add_ + relu_
   (ties, signed zeros, overflow, Inf - Inf, NaN, subnormals), a NaN / Inf confined to its channel,
   and run-to-run determinism.

Every buffer is a _bn_ref.guarded view (4 KiB of a NaN pattern on each side, outputs prefilled with
it, the workspace with NaN and exactly P * C * 2 floats); after each launch the guards are intact and
the inputs bitwise unchanged.

Bounds of tier B, u = 2^-24, L = ceil(ceil(R / P) / ty) the longest fp32 chain of one thread (the
folds across threads and partials run in fp64):
    |gb - sum g| <= (L + 3) u sum|g|,   |gw - invstd sum g (x - mean)| <= (L + 3) u invstd sum|g (x - mean)|
    E = 8u |a| (|g| + |m1| + |x - mean| |k2|) + |a| (dm1 + |x - mean| dk2),   a = w invstd,
        dm1 = (L + 3) u sum|g| / R,  dk2 = invstd^2 (L + 3) u sum|g (x - mean)| / R
    |dx - t| <= E + ulp_bf16(|t| + E)   and   |dx| <= |t| + E
(8u: the product a, the two casts of m1 and k2, mean - x, the fma, g - m1 and the last multiply.)

Measured on an MI355X, worst error / bound per case over the 15 cases of tier B (5 shapes x 3 variants):
    |dx - t| / (E + ulp)  0.40 - 0.50 at R = 2, 1.000 (passing: below 1 by less than 5e-4) on the 12 cases
                          with R >= 196: a truncated value uses the whole ulp
    (|dx| - |t|) / E      0.000 - 0.088
    grad_weight           0.003 - 0.210        grad_bias  0.000 - 0.052
Tier A: all 60 (shape, variant) cases bitwise, the 33 sum-bitwise ones with dx inside the bound as well.
With round-to-nearest dx (-DGS_BN_DX_RNE=1) the same file fails exactly where it should: every bitwise
dx case with a value to truncate (all but R = 1 and R = 2), and (|dx| - |t|) / E = 1.02 - 7338 on 14 of
the 15 random cases and 2581 - 7242 on the sum-bitwise shapes; the reduce pass, grad_weight / grad_bias
and all of C pass.  Three arithmetic mutants were caught too: the dx fold started at p = grp + G4 (every
exact dx, every random case, the channel isolation), each thread's last tail step of the reduce dropped
(every exact reduce and dx case: the unwritten partials and g rows show as NaN), `y < 0` in the mask
(every exact case with y, 8 of the 10 random ones, and the special-value table).

gs_add_relu_fwd ends with fmaxf(s, 0) where ATen's relu_ is clamp_min_: for a sum of -0 both return
+0 on the device (as do a negative subnormal sum and relu / clamp_min out of place), so the header's
"bit-identical" holds for signed zeros too.  ATen flushes no bf16 subnormal in add_, relu_ or
threshold_backward, and neither do the kernels.
"""
import functools
import math

import pytest
import torch

from tests import _bn_ref as B

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


def _L():
    from distributed_training_amd import _lib as L

    return L


def _put(t, dev, off):
    v = B.guarded(t.numel(), t.dtype, dev, off)
    v.copy_(t.reshape(-1))
    return v


def _pattern_only(v):
    return bool((B.bits(v) == v._bn_guard[3]).all())


def _run(inp, variant, dev, place=False):
    """reduce, then dx, as fused_bn calls them; checks guards, inputs and the workspace after each launch.
    add_relu is the residual block's order: reduce with y and g_out, dx fed g_out without y."""
    L = _L()
    lib, stream = L.lib(), L.stream_ptr(dev)
    R, C = inp["x"].shape
    P = L.check(lib.gs_bn_bwd_partials(R, C), "gs_bn_bwd_partials")
    ob, of = (8, 4) if place else (0, 0)  # 16 bytes past a 128-byte line: 16-byte aligned only
    names = ("x", "dy") + (() if variant == "plain" else ("y",))
    d = {k: _put(inp[k], dev, ob) for k in names}
    d.update({k: _put(inp[k], dev, of) for k in ("mean", "invstd", "weight")})
    ws = B.guarded(P * C * 2, F32, dev, of)
    ws.fill_(float("nan"))
    out = dict(dx=B.guarded(R * C, BF16, dev, ob), gw=B.guarded(C, F32, dev, of), gb=B.guarded(C, F32, dev, of))
    if variant == "add_relu":
        out["g"] = B.guarded(R * C, BF16, dev, ob)
    snap = {k: B.bits(v).clone() for k, v in d.items()}

    def verify(what):
        torch.cuda.synchronize()
        for k, v in list(d.items()) + list(out.items()) + [("ws", ws)]:
            assert B.guards_intact(v), f"{what} wrote outside {k}"
        for k, v in d.items():
            assert torch.equal(B.bits(v), snap[k]), f"{what} changed its input {k}"

    yp = None if variant == "plain" else d["y"].data_ptr()
    gp = out["g"].data_ptr() if variant == "add_relu" else None
    L.check(lib.gs_bn_bwd_reduce(d["x"].data_ptr(), d["dy"].data_ptr(), yp, gp, d["mean"].data_ptr(), ws.data_ptr(),
                                 ws.numel(), R, C, stream), "gs_bn_bwd_reduce")
    verify("gs_bn_bwd_reduce")
    for k in ("dx", "gw", "gb"):
        assert _pattern_only(out[k]), f"gs_bn_bwd_reduce wrote {k}"
    ws_reduce = ws.clone()
    dyp = d["dy"].data_ptr()
    if variant == "add_relu":
        snap["g"] = B.bits(out["g"]).clone()
        dyp, yp = out["g"].data_ptr(), None
    L.check(lib.gs_bn_bwd_dx(d["x"].data_ptr(), dyp, yp, d["mean"].data_ptr(), d["invstd"].data_ptr(),
                             d["weight"].data_ptr(), ws.data_ptr(), ws.numel(), out["dx"].data_ptr(),
                             out["gw"].data_ptr(), out["gb"].data_ptr(), R, C, stream), "gs_bn_bwd_dx")
    verify("gs_bn_bwd_dx")
    assert torch.equal(B.bits(ws), B.bits(ws_reduce)), "gs_bn_bwd_dx changed the workspace"
    if variant == "add_relu":
        assert torch.equal(B.bits(out["g"]), snap["g"]), "gs_bn_bwd_dx changed g"
    res = dict(P=P, R=R, C=C, line_offsets={k: v.data_ptr() % 128 for k, v in list(d.items()) + list(out.items())
                                            + [("ws", ws)]}, ws=ws_reduce.view(P, C, 2), dx=out["dx"].view(R, C), gw=out["gw"], gb=out["gb"],
               g=out["g"].view(R, C) if variant == "add_relu" else None)
    res.update({k: (v.view(R, C) if k in ("x", "dy", "y") else v) for k, v in d.items()})
    res.setdefault("y", None)
    return res


def _ref(run):
    return B.bn_bwd_ref(run["x"], run["dy"], run["y"], run["mean"], run["invstd"], run["weight"])


@functools.lru_cache(maxsize=None)
def _exact_case(shape, variant, dev):
    run = _run(B.exact_inputs(*shape), variant, dev)
    return run, _ref(run)


def _pow2ceil(n):
    return 1 << (n - 1).bit_length()


def _bounds(run, ref):
    """the derived bounds of the module docstring -> (gb bound, gw bound, E), fp64 on the device"""
    g, sum_g, sum_gx, _, _, _ = ref
    R, C, P = run["R"], run["C"], run["P"]
    ty = 256 // min(8, _pow2ceil(C // 8))
    chain = math.ceil(math.ceil(R / P) / ty)
    k = (chain + 3) * B.U32
    s = run["invstd"].double()
    a = (run["weight"].double() * s).abs()
    xc = (run["x"].double() - run["mean"].double()).abs()
    Sg, Sgx = g.abs().sum(0), (g.abs() * xc).sum(0)
    m1, k2 = (sum_g / R).abs(), (s * s * sum_gx / R).abs()
    dm1, dk2 = k * Sg / R, s * s * k * Sgx / R
    E = 8 * B.U32 * a * (g.abs() + m1 + xc * k2) + a * (dm1 + xc * dk2)
    return k * Sg, k * s * Sgx, E


def _check_dx_bound(run, ref, tag):
    """|dx - t| <= E + ulp_bf16(|t| + E) and |dx| <= |t| + E, per element -> the worst ratios"""
    _, _, E = _bounds(run, ref)
    t = ref[5]
    dx = run["dx"].double()
    assert bool(torch.isfinite(dx).all()), tag
    err = (dx - t).abs()
    bound = E + B.ulp_bf16(t.abs() + E)
    r_err = float((err / bound).max())
    over = dx.abs() - t.abs()  # truncation never increases the magnitude: at most E above |t|
    r_mag = float(torch.where(E > 0, over / E, torch.where(over > 0, math.inf, 0.0)).max())
    print(f"[bn_kernels] {tag} dx: worst |dx - t| / bound {r_err:.3f}, worst (|dx| - |t|) / E {r_mag:.3f}")
    assert bool((err <= bound).all()), (tag, r_err)
    assert bool((over <= E).all()), (tag, r_mag)
    return r_err, r_mag


# ---- A. the exact grid, bitwise ----------------------------------------------------------------
@pytest.mark.parametrize("shape", B.EXACT_SHAPES, ids=B.shape_id)
@pytest.mark.parametrize("variant", B.VARIANTS)
def test_exact_reduce(cuda_device, variant, shape):
    """A1: the partials add up to the reference's sums exactly, every partial was written, g_out is
    the reference's g and ATen's threshold_backward bit for bit"""
    run, (g, sum_g, sum_gx, _, _, _) = _exact_case(shape, variant, cuda_device)
    ws = run["ws"]
    assert not bool(torch.isnan(ws).any()), "a partial of the workspace was never written"
    got = ws.double().sum(0)
    assert torch.equal(got[:, 0], sum_g), torch.nonzero(got[:, 0] != sum_g).flatten()[:8]
    assert torch.equal(got[:, 1], sum_gx), torch.nonzero(got[:, 1] != sum_gx).flatten()[:8]
    if variant == "add_relu":
        assert torch.equal(B.bits(run["g"]), B.bf16_bits(g))
        aten = torch.ops.aten.threshold_backward(run["dy"], run["y"], 0)
        assert torch.equal(B.bits(run["g"]), B.bits(aten))


@pytest.mark.parametrize("shape", B.EXACT_SHAPES, ids=B.shape_id)
@pytest.mark.parametrize("variant", B.VARIANTS)
def test_exact_dx(cuda_device, variant, shape):
    """A2: grad_bias = float32(sum g) and grad_weight = float32(invstd * sum g (x - mean)) bitwise; dx is
    the truncated reference bitwise where R is a power of two, within the derived bound elsewhere"""
    run, ref = _exact_case(shape, variant, cuda_device)
    _, sum_g, sum_gx, gw, _, dx = ref
    assert torch.equal(B.bits(run["gb"]), B.bits(sum_g.float())), torch.nonzero(run["gb"] != sum_g.float()).flatten()[:8]
    assert torch.equal(B.bits(run["gw"]), B.bits(gw.float())), torch.nonzero(run["gw"] != gw.float()).flatten()[:8]
    if shape in B.BITWISE_DX_SHAPES:
        want = B.trunc_bf16(dx)
        bad = torch.nonzero(B.bits(run["dx"]) != B.bits(want))
        assert bad.numel() == 0, (bad.shape[0], bad[:4].tolist(), run["dx"][tuple(bad[0])], want[tuple(bad[0])])
    else:
        _check_dx_bound(run, ref, f"exact {variant} {shape}")


@pytest.mark.parametrize("variant", B.VARIANTS)
def test_placement_16_byte_aligned_only(cuda_device, variant):
    """A3: every bf16 buffer 8 elements, the workspace and the fp32 vectors 4 floats past a 128-byte line"""
    shape = (777, 24)
    base, _ = _exact_case(shape, variant, cuda_device)
    moved = _run(B.exact_inputs(*shape), variant, cuda_device, place=True)
    assert set(moved["line_offsets"].values()) == {16} and set(base["line_offsets"].values()) == {0}
    for k in ("ws", "dx", "gw", "gb") + (("g",) if variant == "add_relu" else ()):
        assert torch.equal(B.bits(moved[k]), B.bits(base[k])), k


# ---- B. random data, derived bounds ---------------------------------------------------------------
RANDOM_SHAPES = [(2, 8), (777, 24), (8191, 64), (20000, 256), (196, 2048)]


@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=B.shape_id)
@pytest.mark.parametrize("variant", B.VARIANTS)
def test_random_within_derived_bounds(cuda_device, variant, shape):
    R, C = shape
    inp = B.random_inputs(R, C, seed=4321 + R + 13 * C)
    run = _run(inp, variant, cuda_device)
    ref = _ref(run)
    g, sum_g, _, gw, _, _ = ref
    if variant != "plain" and R * C >= 1000:
        assert 0.3 < float((g == 0).double().mean()) < 0.7  # the mask is exercised both ways
        assert bool((run["y"] == 0).any())
    b_gb, b_gw, _ = _bounds(run, ref)
    tag = f"random {variant} {shape}"
    e_gb, e_gw = (run["gb"].double() - sum_g).abs(), (run["gw"].double() - gw).abs()
    one = torch.ones_like(b_gb)
    r_gb = float((e_gb / torch.where(b_gb > 0, b_gb, one)).max())
    r_gw = float((e_gw / torch.where(b_gw > 0, b_gw, one)).max())
    print(f"[bn_kernels] {tag} worst error / bound: gb {r_gb:.3f}  gw {r_gw:.3f}")
    assert bool((e_gb <= b_gb).all()), (tag, "gb", r_gb)
    assert bool((e_gw <= b_gw).all()), (tag, "gw", r_gw)
    if variant == "add_relu":
        assert torch.equal(B.bits(run["g"]), B.bits(torch.ops.aten.threshold_backward(run["dy"], run["y"], 0)))
    _check_dx_bound(run, ref, tag)


# ---- C. special values ----------------------------------------------------------------------------
def test_mask_special_values_equal_threshold_backward(cuda_device):
    """C1: every pair of (y, dy) from +-0, NaN, +-Inf, the smallest subnormals and ordinary values"""
    L = _L()
    ys = [0x0000, 0x8000, 0x7FC0, 0x7F80, 0xFF80, 0x0001, 0x8001, 0x3F80, 0xBF80]
    dys = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x0001, 0x8001, 0x0040, 0x3FC0, 0xC000]
    pairs = [(a, b) for a in ys for b in dys]
    C = 8
    R = -(-len(pairs) // C)
    pairs += [(0x3F80, 0x3F80)] * (R * C - len(pairs))
    dev = cuda_device
    y = _put(B.from_bits([p[0] for p in pairs]), dev, 0)
    dy = _put(B.from_bits([p[1] for p in pairs]), dev, 0)
    x = _put(torch.zeros(R * C, dtype=BF16), dev, 0)
    mean = _put(torch.zeros(C), dev, 0)
    P = L.check(L.lib().gs_bn_bwd_partials(R, C))
    ws = B.guarded(P * C * 2, F32, dev)
    g = B.guarded(R * C, BF16, dev)
    snap = [B.bits(t).clone() for t in (x, dy, y)]
    L.check(L.lib().gs_bn_bwd_reduce(x.data_ptr(), dy.data_ptr(), y.data_ptr(), g.data_ptr(), mean.data_ptr(),
                                     ws.data_ptr(), ws.numel(), R, C, L.stream_ptr(dev)), "gs_bn_bwd_reduce")
    torch.cuda.synchronize()
    for t in (x, dy, y, mean, ws, g):
        assert B.guards_intact(t)
    for t, s in zip((x, dy, y), snap):
        assert torch.equal(B.bits(t), s)
    aten = torch.ops.aten.threshold_backward(dy, y, 0)
    got, want = B.bits(g).tolist(), B.bits(aten).tolist()
    bad = [(hex(p[0]), hex(p[1]), hex(a & 0xFFFF), hex(b & 0xFFFF)) for p, a, b in zip(pairs, got, want) if a != b]
    assert not bad, f"(y, dy, kernel, ATen): {bad}"
    # and the contract in its own words: y <= 0 ? +0 : dy, a NaN y passes dy
    own = [0 if (a in (0x0000, 0x8000, 0xFF80, 0x8001, 0xBF80)) else b for a, b in pairs]
    assert [v & 0xFFFF for v in got] == own


def test_nan_and_inf_stay_in_their_channel(cuda_device):
    """C2: one NaN in x (channel 5) and one +Inf in dy (channel 17); every other channel is bitwise the
    clean run's.  The Inf sits where y > 0 (the mask passes it) and x = mean (Inf * 0: the second sum of
    channel 17 is NaN, so all of its dx is, not only the rows that meet Inf - Inf)."""
    shape = (777, 24)
    clean, _ = _exact_case(shape, "relu", cuda_device)
    inp = B.exact_inputs(*shape)
    inp["x"][100, 5] = float("nan")
    inp["dy"][300, 17] = float("inf")
    inp["y"][300, 17] = 1.0
    inp["x"][300, 17] = inp["mean"][17]
    run = _run(inp, "relu", cuda_device)
    others = [c for c in range(shape[1]) if c not in (5, 17)]
    for k in ("dx", "gw", "gb", "ws"):
        a, b = (run[k][:, others], clean[k][:, others]) if k in ("dx", "ws") else (run[k][others], clean[k][others])
        assert torch.equal(B.bits(a), B.bits(b)), k
    assert bool(torch.isnan(run["gw"][5])) and bool(torch.isnan(run["dx"][:, 5]).all())
    assert torch.equal(B.bits(run["gb"][5:6]), B.bits(clean["gb"][5:6]))  # sum g never meets x
    assert float(run["gb"][17]) == math.inf and bool(torch.isnan(run["dx"][:, 17]).all())


# (t, identity) as bf16 patterns
ADD_PAIRS = [
    (0x3F80, 0x3B80),  # 1 + 2^-8: a tie, to even 1.0
    (0x3F81, 0x3B80),  # 1.0078125 + 2^-8: a tie, to even 1.015625
    (0xBF80, 0xBB80),  # a negative tie
    (0x4000, 0xBB80),  # 2 - 2^-8: a tie from a negative operand, to even 2.0
    (0x8000, 0x8000),  # -0 + -0
    (0x0000, 0x8000),  # +0 + -0
    (0x3FC0, 0xBFC0),  # x + (-x)
    (0x7F61, 0x7F61),  # 3e38 + 3e38: overflows to Inf
    (0x7F80, 0xFF80),  # Inf + (-Inf)
    (0x7FC0, 0x3F80),  # NaN + 1
    (0x0040, 0x0020),  # 2^-127 + 2^-128: a subnormal sum
    (0x8040, 0x8020),  # the same, negative
    (0x0080, 0x8040),  # 2^-126 - 2^-127: normal operands, subnormal sum
    (0x8080, 0x0040),  # the same, negative
    (0x3FC0, 0x4010),  # 1.5 + 2.25
    (0xC040, 0x3F80),  # -3 + 1
]


@pytest.mark.parametrize("nvec", [1, 255, 256, 1023, 1024, 1025, 4097])
def test_add_relu_fwd_equals_aten(cuda_device, nvec):
    """C3: bitwise t.add_(identity).relu_(); a workgroup covers 1024 vectors of 8"""
    L = _L()
    n = nvec * 8
    gen = torch.Generator().manual_seed(nvec)
    t0 = torch.randn(n, generator=gen).to(BF16)
    i0 = torch.randn(n, generator=gen).to(BF16)
    ta, ia = B.from_bits([p[0] for p in ADD_PAIRS]), B.from_bits([p[1] for p in ADD_PAIRS])
    planted = []
    for j, v in enumerate(sorted({0, 1023, 1024, nvec - 1} & set(range(nvec)))):
        h = (j % 2) * 8
        t0[v * 8:v * 8 + 8], i0[v * 8:v * 8 + 8] = ta[h:h + 8], ia[h:h + 8]
        planted.append(v)
    t, idn = _put(t0, cuda_device, 0), _put(i0, cuda_device, 0)
    want = t.clone().add_(idn).relu_()
    snap = B.bits(idn).clone()
    L.check(L.lib().gs_add_relu_fwd(t.data_ptr(), idn.data_ptr(), n, L.stream_ptr(cuda_device)), "gs_add_relu_fwd")
    torch.cuda.synchronize()
    assert B.guards_intact(t) and B.guards_intact(idn)
    assert torch.equal(B.bits(idn), snap)
    bad = torch.nonzero(B.bits(t) != B.bits(want)).flatten()
    detail = [(int(i), hex(B.bits(t0)[i].item() & 0xFFFF), hex(B.bits(i0)[i].item() & 0xFFFF),
               hex(B.bits(t)[i].item() & 0xFFFF), hex(B.bits(want)[i].item() & 0xFFFF)) for i in bad[:16].tolist()]
    assert bad.numel() == 0, f"planted vectors {planted}; (index, t, identity, kernel, ATen): {detail}"


def test_two_runs_are_bitwise_equal(cuda_device):
    """C4"""
    shape = (20000, 256)
    a, _ = _exact_case(shape, "add_relu", cuda_device)
    b = _run(B.exact_inputs(*shape), "add_relu", cuda_device)
    for k in ("ws", "g", "dx", "gw", "gb"):
        assert torch.equal(B.bits(a[k]), B.bits(b[k])), k
