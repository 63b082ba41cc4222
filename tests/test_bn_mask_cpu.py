"""The entry points of the ReLU mask as bits without a GPU (include/gsync.h).

1. the argument checks of gs_relu_mask_fwd, gs_add_relu_mask_fwd, gs_relu_maxpool_mask_fwd,
   gs_bn_bwd_reduce_bits, gs_bn_bwd_reduce_fork_bits and gs_bn_bwd_dx_bits, all of which sit before any launch
   (the pointers are made-up values that are never dereferenced): GS_EINVAL and a message in gs_last_error();
   the mask pointer of every valid argument list here is odd (it needs no alignment: the GPU tests launch so);
2. the symbols are registered in _lib.py with their argument types;
3. GSYNC_BN_MASK is read per call and defaults to on.
"""
import pytest

from distributed_training_amd import fused_bn

A = 0x7F0000001000  # made-up addresses, 16-byte aligned, never dereferenced
R0, C0 = 777, 24
BYTES = R0 * C0 * 2
MBYTES = R0 * C0 // 8
_ids = lambda d: "-".join(f"{k}={v}" for k, v in d.items())  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    from distributed_training_amd import _lib as L

    return L.lib()


def _rejected(lib, fn, args, word=""):
    from distributed_training_amd import _lib as L

    lib.gs_bn_bwd_partials(64, 64)
    assert getattr(lib, fn)(*args) == L.GS_EINVAL
    msg = lib.gs_last_error()
    msg = msg.decode() if isinstance(msg, bytes) else msg
    assert msg and word in msg, msg


# ---- the backward consumers ---------------------------------------------------------------------
def _reduce_args(lib, fork, **kw):
    P = lib.gs_bn_bwd_partials(R0, C0)
    a = dict(x=A, dy=A + 0x100000, dy_b=A + 0x200000, mask=A + 0x300003, g_out=A + 0x400000, mean=A + 0x500000,
             ws=A + 0x600000, ws_floats=P * C0 * 2, R=R0, C=C0)
    a.update(kw)
    if a["ws_floats"] == "short":
        a["ws_floats"] = P * C0 * 2 - 1
    names = ("x", "dy") + (("dy_b",) if fork else ()) + ("mask", "g_out", "mean", "ws", "ws_floats", "R", "C")
    return [a[k] for k in names] + [None]


REDUCE_BAD = (
    [{k: None} for k in ("x", "dy", "mask", "mean", "ws")]
    + [{k: A + 0x700008} for k in ("x", "dy", "g_out", "ws")]
    + [dict(ws_floats="short"), dict(C=12), dict(C=0), dict(R=0), dict(R=2 ** 60)]
)
FORK_BAD = REDUCE_BAD + [dict(g_out=None), dict(dy_b=A + 0x700008)] + [dict(g_out=A + d) for d in (0, 0x100000, 0x200000)]


# g_out (16-byte aligned) over the whole mask, over its last byte, over its first byte
assert MBYTES == 2331 and BYTES % 16 == 0
G_OUT_ON_MASK = [dict(g_out=A + 0x300000), dict(g_out=A + 0x300000 + 2320), dict(g_out=A + 0x300000 - BYTES + 16)]


@pytest.mark.parametrize("bad", G_OUT_ON_MASK, ids=_ids)
@pytest.mark.parametrize("fork", [False, True], ids=["reduce", "fork"])
def test_g_out_must_not_overlap_the_mask(lib, fork, bad):
    _rejected(lib, "gs_bn_bwd_reduce_fork_bits" if fork else "gs_bn_bwd_reduce_bits", _reduce_args(lib, fork, **bad),
              "g_out overlaps the mask")


@pytest.mark.parametrize("bad", REDUCE_BAD, ids=_ids)
def test_reduce_bits_rejects(lib, bad):
    _rejected(lib, "gs_bn_bwd_reduce_bits", _reduce_args(lib, False, **bad))


@pytest.mark.parametrize("bad", FORK_BAD, ids=_ids)
def test_reduce_fork_bits_rejects(lib, bad):
    _rejected(lib, "gs_bn_bwd_reduce_fork_bits", _reduce_args(lib, True, **bad))


def _dx_args(lib, **kw):
    P = lib.gs_bn_bwd_partials(R0, C0)
    a = dict(x=A, dy=A + 0x100000, mask=A + 0x300003, mean=A + 0x500000, invstd=A + 0x510000, weight=A + 0x520000,
             ws=A + 0x600000, ws_floats=P * C0 * 2, dx=A + 0x400000, gw=A + 0x530000, gb=A + 0x540000, R=R0, C=C0)
    a.update(kw)
    if a["ws_floats"] == "short":
        a["ws_floats"] = P * C0 * 2 - 1
    return [a[k] for k in ("x", "dy", "mask", "mean", "invstd", "weight", "ws", "ws_floats", "dx", "gw", "gb", "R",
                           "C")] + [None]


DX_BAD = (
    [{k: None} for k in ("x", "dy", "mask", "mean", "invstd", "weight", "ws", "dx", "gw", "gb")]
    + [{k: A + 0x700008} for k in ("x", "dy", "dx", "ws")]
    + [dict(dx=A + 0x300000), dict(dx=A + 0x300000 + 2320)]  # dx over the mask's first / last byte
    + [dict(ws_floats="short"), dict(C=12), dict(R=0), dict(R=2 ** 60)]
)


@pytest.mark.parametrize("bad", DX_BAD, ids=_ids)
def test_dx_bits_rejects(lib, bad):
    _rejected(lib, "gs_bn_bwd_dx_bits", _dx_args(lib, **bad))


# ---- the forward producers ------------------------------------------------------------------------
N0 = 4096  # elements: 8192 bytes of activation, 512 bytes of mask


def _tail_args(add, **kw):
    a = dict(t=A, identity=A + 0x10000, mask=A + 0x20001, n=N0)
    a.update(kw)
    return [a[k] for k in (("t", "identity", "mask", "n") if add else ("t", "mask", "n"))] + [None]


TAIL_BAD = ([{k: None} for k in ("t", "mask")] + [dict(t=A + 8), dict(n=0), dict(n=-8), dict(n=12), dict(n=2 ** 62)]
            + [dict(mask=A + 2 * N0 - 1), dict(mask=A - N0 // 8 + 1), dict(mask=A + 100)])  # the mask inside / across t
ADD_BAD = TAIL_BAD + [dict(identity=None), dict(identity=A + 0x10008), dict(mask=A + 0x10000 + 2 * N0 - 1)]


@pytest.mark.parametrize("bad", TAIL_BAD, ids=_ids)
def test_relu_mask_fwd_rejects(lib, bad):
    _rejected(lib, "gs_relu_mask_fwd", _tail_args(False, **bad))


@pytest.mark.parametrize("bad", ADD_BAD, ids=_ids)
def test_add_relu_mask_fwd_rejects(lib, bad):
    _rejected(lib, "gs_add_relu_mask_fwd", _tail_args(True, **bad))


PN, PH, PW, PC = 2, 7, 6, 16  # in 2688 bytes, out 2 * 4 * 3 * 16 * 2 = 768 bytes, idx 384, mask 168


def _pool_args(**kw):
    a = dict(y=A, pooled=A + 0x10000, idx=A + 0x20000, mask=A + 0x30005, N=PN, H=PH, W=PW, C=PC)
    a.update(kw)
    return [a[k] for k in ("y", "pooled", "idx", "mask", "N", "H", "W", "C")] + [None]


POOL_BAD = (
    [{k: None} for k in ("y", "pooled", "idx", "mask")] + [{k: A + 0x70008} for k in ("y", "pooled", "idx")]
    + [dict(pooled=A + 2688 - 16), dict(idx=A + 16), dict(idx=A + 0x10000 + 768 - 16)]  # the stem buffers overlap
    + [dict(mask=A + 2688 - 1), dict(mask=A - 168 + 1), dict(mask=A + 0x10000 + 768 - 1), dict(mask=A + 0x20000 + 5)]
    + [dict(N=0), dict(H=0), dict(W=-1), dict(C=12), dict(C=0), dict(N=2 ** 58)]
)


@pytest.mark.parametrize("bad", POOL_BAD, ids=_ids)
def test_relu_maxpool_mask_fwd_rejects(lib, bad):
    _rejected(lib, "gs_relu_maxpool_mask_fwd", _pool_args(**bad))


# ---- registration, the switch ------------------------------------------------------------------------
NEW = ["gs_relu_mask_fwd", "gs_add_relu_mask_fwd", "gs_relu_maxpool_mask_fwd", "gs_bn_bwd_reduce_bits",
       "gs_bn_bwd_reduce_fork_bits", "gs_bn_bwd_dx_bits"]
SIBLING = {"gs_bn_bwd_reduce_bits": "gs_bn_bwd_reduce", "gs_bn_bwd_reduce_fork_bits": "gs_bn_bwd_reduce_fork",
           "gs_bn_bwd_dx_bits": "gs_bn_bwd_dx"}


@pytest.mark.parametrize("name", NEW)
def test_symbols_are_registered(lib, name):
    fn = getattr(lib, name)
    assert fn.argtypes is not None and fn.restype is not None
    if name in SIBLING:  # the mask takes y's place in the argument list
        assert list(fn.argtypes) == list(getattr(lib, SIBLING[name]).argtypes)


def test_the_switch_is_read_per_call(monkeypatch):
    monkeypatch.delenv("GSYNC_BN_MASK", raising=False)
    assert fused_bn._mask_bits()
    monkeypatch.setenv("GSYNC_BN_MASK", "0")
    assert not fused_bn._mask_bits()
    monkeypatch.setenv("GSYNC_BN_MASK", "1")
    assert fused_bn._mask_bits()
