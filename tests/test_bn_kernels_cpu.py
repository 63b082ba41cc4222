"""The NHWC BatchNorm backward entry points without a GPU (include/gsync.h, csrc/gs_bn_kernels.hip).

1. the fp64 reference of tests/_bn_ref.py equals autograd's batch_norm + relu in double;
2. the exact grid is exact: for every shape the GPU tests compare bitwise, the fp64 sums are
   fp32-representable in any order and (R a power of two) so is every step of the dx chain;
3. gs_bn_bwd_partials: bounds, stability, argument errors;
4. the argument checks of gs_bn_bwd_reduce / gs_bn_bwd_dx / gs_add_relu_fwd, all of which sit
   before any launch (the pointers are made-up values that are never dereferenced).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _bn_ref as B


@pytest.fixture(scope="module")
def lib():
    from distributed_training_amd import _lib as L

    return L.lib()


# ---- 1. the reference checks itself ---------------------------------------------------------
@pytest.mark.parametrize("R", [5, 64])
def test_reference_equals_autograd_in_double(R):
    C = 16
    gen = torch.Generator().manual_seed(R)
    x = (torch.randn(R, C, generator=gen, dtype=torch.float64) * 1.5 + 0.7).requires_grad_()
    w = torch.randn(C, generator=gen, dtype=torch.float64).requires_grad_()
    b = torch.randn(C, generator=gen, dtype=torch.float64).requires_grad_()
    dy = torch.randn(R, C, generator=gen, dtype=torch.float64)
    eps = 1e-5
    y = F.relu(F.batch_norm(x, None, None, w, b, True, 0.1, eps))
    y.backward(dy)
    xd = x.detach()
    mean = xd.mean(0)
    invstd = 1.0 / torch.sqrt(((xd - mean) ** 2).mean(0) + eps)
    g, sum_g, sum_gx, gw, gb, dx = B.bn_bwd_ref(xd, dy, y.detach(), mean, invstd, w.detach())
    assert 0.2 < float((y == 0).double().mean()) < 0.8  # the mask is exercised both ways
    for name, got, want in (("dx", dx, x.grad), ("gw", gw, w.grad), ("gb", gb, b.grad)):
        err = float((got - want).abs().max())
        assert err <= 1e-12 * float(want.abs().max()), (name, err)
    # without y the reference is the plain BatchNorm backward
    x.grad = w.grad = b.grad = None
    F.batch_norm(x, None, None, w, b, True, 0.1, eps).backward(dy)
    _, _, _, gw, gb, dx = B.bn_bwd_ref(xd, dy, None, mean, invstd, w.detach())
    for name, got, want in (("dx", dx, x.grad), ("gw", gw, w.grad), ("gb", gb, b.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), name


def test_bf16_helpers():
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 2.0 ** -7 + 2.0 ** -9), 3.0, -0.0, 2.0 ** -130],
                     dtype=torch.float64)
    t = B.trunc_bf16(v)
    assert t.dtype == torch.bfloat16
    assert t.double().tolist()[:3] == [1.0, -(1.0 + 2.0 ** -7), 3.0]
    assert B.bf16_bits(t).tolist()[3] == -32768  # -0 keeps its sign
    assert t.double().tolist()[4] == 2.0 ** -130
    u = B.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, -8.0, 0.0, 2.0 ** -127], dtype=torch.float64))
    assert u.tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -4, 2.0 ** -133, 2.0 ** -133]
    assert B.from_bits([0x3F80, 0x8000, 0x7F80]).double().tolist() == [1.0, -0.0, math.inf]


def test_guarded_buffers():
    for dtype, off in ((torch.bfloat16, 0), (torch.bfloat16, 8), (torch.float32, 0), (torch.float32, 4)):
        v = B.guarded(24, dtype, "cpu", off)
        size = v.element_size()
        assert v.numel() == 24 and v.data_ptr() % 128 == off * size and v.data_ptr() % 16 == 0
        raw, start, n, _ = v._bn_guard
        assert start * size >= 4096 and (raw.numel() - start - n) * size >= 4096
        assert bool(torch.isnan(v).all())  # the view starts out holding the pattern, a NaN
        v.zero_()
        assert B.guards_intact(v)
        raw[start - 1] = 0
        assert not B.guards_intact(v)
        raw[start - 1] = raw[0]
        raw[start + n] = 0
        assert not B.guards_intact(v)


# ---- 2. the exact grid is exact --------------------------------------------------------------
@pytest.mark.parametrize("shape", B.EXACT_SHAPES, ids=B.shape_id)
def test_exact_grid_is_exact(shape):
    R, C = shape
    inp = B.exact_inputs(R, C)
    for k in ("x", "dy", "y"):
        assert inp[k].dtype == torch.bfloat16 and inp[k].shape == (R, C)
    # the generator's fp32 values survived the bf16 conversion
    assert bool(((inp["x"].double() - inp["mean"].double()) * 2 == ((inp["x"].double() - inp["mean"].double()) * 2)
                 .round()).all())
    for variant in B.VARIANTS:
        y = None if variant == "plain" else inp["y"]
        g, sum_g, sum_gx, gw, gb, dx = B.bn_bwd_ref(inp["x"], inp["dy"], y, inp["mean"], inp["invstd"],
                                                    inp["weight"])
        xc = inp["x"].double() - inp["mean"].double()
        # every term is a multiple of 1/8 and the sums of magnitudes stay below 2^24 / 8: any partial
        # sum in any order is an integer multiple of 1/8 below 2^24 / 8, hence exact in fp32
        assert bool(((g * 8) == (g * 8).round()).all()) and bool((((g * xc) * 8) == ((g * xc) * 8).round()).all())
        assert float(g.abs().sum(0).max()) * 8 < 2 ** 24, variant
        assert float((g * xc).abs().sum(0).max()) * 8 < 2 ** 24, variant
        for name, v in (("sum_g", sum_g), ("sum_gx", sum_gx), ("gw", gw)):
            assert bool(B.is_f32(v).all()), (variant, name)
        if shape in B.BITWISE_DX_SHAPES:
            # the kernel's chain: a = w * invstd, m1 = sum_g / R, k2 = invstd^2 * sum_gx / R (fp64, then
            # cast), g - m1, fma(mean - x, k2, g - m1), a * (.)
            s, w = inp["invstd"].double(), inp["weight"].double()
            m1, k2 = sum_g / R, s * s * sum_gx / R
            d = g - m1
            t = (-xc) * k2 + d
            for name, v in (("a", w * s), ("m1", m1), ("k2", k2), ("g - m1", d), ("fma", t), ("a * fma", w * s * t)):
                assert bool(B.is_f32(v).all()), (variant, name)
            assert bool((w * s * t == dx).all())  # fp64 carries the chain exactly: it is the reference's dx


# ---- 3. gs_bn_bwd_partials --------------------------------------------------------------------
PART_R = [1, 2, 3, 255, 256, 257, 6272, 802816, 2 ** 31 + 5]
PART_C = [8, 16, 24, 64, 72, 256, 2048]


@pytest.mark.parametrize("C", PART_C)
@pytest.mark.parametrize("R", PART_R)
def test_partials_bounds(lib, R, C):
    P = lib.gs_bn_bwd_partials(R, C)
    assert 1 <= P <= 512, P
    assert P <= max(1, math.isqrt(R // 2)), P  # floor(sqrt(R / 2)): the fold stays below the stream
    assert lib.gs_bn_bwd_partials(R, C) == P


@pytest.mark.parametrize("R,C", [(64, 12), (64, 0), (0, 64), (2 ** 60, 8), (64, -8), (-1, 8)])
def test_partials_rejects(lib, R, C):
    from distributed_training_amd import _lib as L

    lib.gs_bn_bwd_partials(64, 64)
    assert lib.gs_bn_bwd_partials(R, C) == L.GS_EINVAL
    assert lib.gs_last_error()


# ---- 4. argument checks, all before any launch -------------------------------------------------
A = 0x7F0000001000  # made-up addresses, 16-byte aligned, never dereferenced
R0, C0 = 777, 24


def _reduce_args(lib, **kw):
    P = lib.gs_bn_bwd_partials(R0, C0)
    a = dict(x=A, dy=A + 0x100000, y=A + 0x200000, g_out=A + 0x300000, mean=A + 0x400000, ws=A + 0x500000,
             ws_floats=P * C0 * 2, R=R0, C=C0)
    a.update(kw)
    return [a[k] for k in ("x", "dy", "y", "g_out", "mean", "ws", "ws_floats", "R", "C")] + [None]


def _dx_args(lib, **kw):
    P = lib.gs_bn_bwd_partials(R0, C0)
    a = dict(x=A, dy=A + 0x100000, y=A + 0x200000, mean=A + 0x400000, invstd=A + 0x410000, weight=A + 0x420000,
             ws=A + 0x500000, ws_floats=P * C0 * 2, dx=A + 0x600000, gw=A + 0x430000, gb=A + 0x440000, R=R0, C=C0)
    a.update(kw)
    return [a[k] for k in ("x", "dy", "y", "mean", "invstd", "weight", "ws", "ws_floats", "dx", "gw", "gb", "R",
                           "C")] + [None]


def _einval(lib, rc):
    from distributed_training_amd import _lib as L

    assert rc == L.GS_EINVAL, rc
    assert lib.gs_last_error()


REDUCE_BAD = (
    [{k: None} for k in ("x", "dy", "mean", "ws")]
    + [{k: A + 0x700008} for k in ("x", "dy", "y", "g_out", "ws")]
    + [dict(y=None), dict(ws_floats=-1), dict(C=12), dict(C=0), dict(R=0)]
)


@pytest.mark.parametrize("bad", REDUCE_BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_reduce_rejects(lib, bad):
    if bad == dict(ws_floats=-1):
        bad = dict(ws_floats=lib.gs_bn_bwd_partials(R0, C0) * C0 * 2 - 1)
    _einval(lib, lib.gs_bn_bwd_reduce(*_reduce_args(lib, **bad)))


DX_BAD = (
    [{k: None} for k in ("x", "dy", "mean", "invstd", "weight", "ws", "dx", "gw", "gb")]
    + [{k: A + 0x700008} for k in ("x", "dy", "y", "dx", "ws")]
    + [dict(ws_floats=-1), dict(C=12), dict(C=0), dict(R=0)]
)


@pytest.mark.parametrize("bad", DX_BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_dx_rejects(lib, bad):
    if bad == dict(ws_floats=-1):
        bad = dict(ws_floats=lib.gs_bn_bwd_partials(R0, C0) * C0 * 2 - 1)
    _einval(lib, lib.gs_bn_bwd_dx(*_dx_args(lib, **bad)))


@pytest.mark.parametrize("t,idn,n", [(None, A, 64), (A, None, 64), (A, A + 0x1000, 0), (A, A + 0x1000, 12),
                                     (A, A + 0x1000, -8), (A + 8, A + 0x1000, 64), (A, A + 0x1008, 64)])
def test_add_relu_rejects(lib, t, idn, n):
    _einval(lib, lib.gs_add_relu_fwd(t, idn, n, None))
