"""gs_relu_maxpool_fwd / gs_maxpool_bwd called directly (include/gsync.h) against ATen on the device.

Forward: the pooled output equals F.max_pool2d(F.relu(y), 3, 2, 1) bit for bit; the index byte equals a
pure-torch reference written here (pool_ref: the scan in the header's words; test_bn_fork_pool_cpu.py
holds it against ATen's CPU indices) and names the element ATen's device indices name; y is unchanged.
Backward: dx equals max_pool2d_with_indices_backward(dA + dB, ...) with ATen's bf16 add and ATen's own
indices, bit for bit; with one gradient, the same without the add.

Data: random values; all negative (every window a tie at 0 after the ReLU: the first element must
win); blocks of equal positive values; NaN, +-Inf and -0 at corners, on edges and inside.  Gradients
carry -0, +-Inf, NaN, ties of the bf16 sum and values whose fp32 sum over four windows rounds.
Every buffer is a _bn_ref.guarded view, outputs prefilled with the guard pattern.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import _bn_ref as B

BF16 = torch.bfloat16
POOL_SHAPES = [(1, 1, 1, 8), (2, 2, 3, 8), (2, 7, 7, 16), (1, 8, 9, 72), (3, 13, 12, 64), (2, 32, 32, 8)]
DATA = ["random", "negative", "blocks", "special"]


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def pool_ref(y):
    """y [N, H, W, C] (any float dtype, CPU or device) -> (pooled fp32 of relu(y), code uint8 [N, OH, OW, C]).
    Windows clipped at the border, rows outer, columns inner; a later value wins only if it is > the
    current one or is NaN.  code = 3 * kh + kw in the unclipped window."""
    N, H, W, C = y.shape
    OH, OW = out_hw(H, W)
    v = y.float()
    v = torch.where(v > 0, v, torch.where(torch.isnan(v), v, torch.zeros_like(v)))  # relu: NaN stays, -0 -> +0
    vp = torch.zeros(N, H + 3, W + 3, C, dtype=torch.float32, device=y.device)
    ok = torch.zeros(N, H + 3, W + 3, 1, dtype=torch.bool, device=y.device)
    vp[:, 1:H + 1, 1:W + 1] = v
    ok[:, 1:H + 1, 1:W + 1] = True
    best = torch.full((N, OH, OW, C), float("-inf"), device=y.device)
    code = torch.zeros((N, OH, OW, C), dtype=torch.uint8, device=y.device)
    for kh in range(3):
        for kw in range(3):
            cand = vp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2]
            take = ok[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] & ((cand > best) | torch.isnan(cand))
            best = torch.where(take, cand, best)
            code = torch.where(take, torch.full_like(code, 3 * kh + kw), code)
    return best, code


def code_to_flat_index(code, H, W):
    """the index ATen keeps (ih * W + iw, int64 [N, OH, OW, C]) from the window position"""
    N, OH, OW, C = code.shape
    oh = torch.arange(OH, device=code.device).view(1, OH, 1, 1)
    ow = torch.arange(OW, device=code.device).view(1, 1, OW, 1)
    c = code.long()
    return (2 * oh - 1 + c // 3) * W + (2 * ow - 1 + c % 3)


def make_y(shape, kind, seed=0):
    N, H, W, C = shape
    gen = torch.Generator().manual_seed(seed + 97 * H + W)
    y = torch.randn(shape, generator=gen)
    if kind == "negative":
        y = -y.abs() - 0.5
    elif kind == "blocks":
        # 2 x 3 blocks of one positive value: ties inside a window, rows and columns
        hh, ww = torch.arange(H).view(1, H, 1, 1) // 2, torch.arange(W).view(1, 1, W, 1) // 3
        y = ((hh * 5 + ww * 3 + torch.arange(C).view(1, 1, 1, C)) % 4).float() * 0.5 + 0.0 * y
    y = y.to(BF16)
    if kind == "special":
        sp = B.from_bits([0x7FC0, 0x7F80, 0xFF80, 0x8000, 0x0000, 0x7FC0, 0x3F80, 0x7F80])
        spots = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H // 2, W // 2),
                 (H - 1, W // 2), (min(1, H - 1), min(1, W - 1)), (min(2, H - 1), min(1, W - 1))}
        for k, (h, w) in enumerate(sorted(spots)):
            y[:, h, w, :] = sp.roll(k)[:8].repeat(C // 8)
        if H > 2 and W > 2:  # two NaNs in one window: the last one wins
            y[0, 1, 1, 0] = float("nan")
            y[0, 2, 2, 0] = float("nan")
    return y


def make_grads(shape, seed=1):
    N, H, W, C = shape
    OH, OW = out_hw(H, W)
    gen = torch.Generator().manual_seed(seed + 13 * H + W)
    dA = torch.randn(N, OH, OW, C, generator=gen).to(BF16)
    dB = torch.randn(N, OH, OW, C, generator=gen).to(BF16)
    sp_a = B.from_bits([0x8000, 0x0000, 0x3F80, 0x3F81, 0x7F61, 0x7F80, 0x7FC0, 0x0040])
    sp_b = B.from_bits([0x8000, 0x8000, 0x3B80, 0x3B80, 0x7F61, 0xFF80, 0x3F80, 0x0020])
    n = min(8, dA.numel())
    dA.view(-1)[:n], dB.view(-1)[:n] = sp_a[:n], sp_b[:n]  # -0 + -0, +0 + -0, ties, overflow, Inf - Inf, NaN, subnormal
    dA.view(-1)[-n:], dB.view(-1)[-n:] = sp_a[:n], sp_b[:n]
    return dA, dB


def _put(t, dev):
    v = B.guarded(t.numel(), t.dtype, dev, 0)
    v.copy_(t.reshape(-1))
    return v


def _as_nchw(t, shape):
    """a flat NHWC buffer as the channels_last [N, C, H, W] tensor ATen takes"""
    N, H, W, C = shape
    return t.view(N, H, W, C).permute(0, 3, 1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", DATA)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_forward_and_backward_equal_aten(cuda_device, shape, kind):
    from distributed_training_amd import _lib as L

    dev = cuda_device
    lib, stream = L.lib(), L.stream_ptr(dev)
    N, H, W, C = shape
    OH, OW = out_hw(H, W)
    oshape = (N, OH, OW, C)
    y0 = make_y(shape, kind)
    y = _put(y0, dev)
    n_out = N * OH * OW * C
    pooled = B.guarded(n_out, BF16, dev)
    idx_buf = B.guarded(n_out // 2, BF16, dev)  # n_out bytes
    idx = idx_buf.view(torch.uint8)
    assert idx.numel() == n_out and idx.data_ptr() == idx_buf.data_ptr()
    snap_y = B.bits(y).clone()
    L.check(lib.gs_relu_maxpool_fwd(y.data_ptr(), pooled.data_ptr(), idx.data_ptr(), N, H, W, C, stream),
            "gs_relu_maxpool_fwd")
    torch.cuda.synchronize()
    for k, v in (("y", y), ("pooled", pooled), ("idx", idx_buf)):
        assert B.guards_intact(v), f"gs_relu_maxpool_fwd wrote outside {k}"
    assert torch.equal(B.bits(y), snap_y), "gs_relu_maxpool_fwd changed y"

    relu_y = F.relu(_as_nchw(y, shape))
    want, aten_idx = F.max_pool2d(relu_y, 3, 2, 1, return_indices=True)
    assert want.is_contiguous(memory_format=torch.channels_last) or want.numel() == want.shape[1] * N
    want_nhwc, aten_idx = want.permute(0, 2, 3, 1).contiguous(), aten_idx.permute(0, 2, 3, 1).contiguous()
    got = pooled.view(oshape)
    bad = torch.nonzero(B.bits(got) != B.bits(want_nhwc))
    assert bad.numel() == 0, (bad.shape[0], bad[:4].tolist())
    ref_best, ref_code = pool_ref(y0.view(shape))
    code = idx.view(oshape)
    assert int(code.max()) <= 8
    bad = torch.nonzero(code.cpu() != ref_code)
    assert bad.numel() == 0, (bad.shape[0], bad[:4].tolist())
    assert torch.equal(code_to_flat_index(code, H, W), aten_idx), "the byte names another element than ATen's index"
    if kind == "negative":
        # the window's first valid element: row 1 of the window at the top border, column 1 at the left one
        first = torch.tensor([[4 if (oh == 0 and ow == 0) else 3 if oh == 0 else 1 if ow == 0 else 0
                               for ow in range(OW)] for oh in range(OH)], dtype=torch.uint8)
        assert torch.equal(code.cpu(), first.view(1, OH, OW, 1).expand(oshape))  # a tie at 0: the first valid element

    # ---- backward: two gradients, then one ----
    dA0, dB0 = make_grads(shape)
    dA, dB = _put(dA0, dev), _put(dB0, dev)
    snaps = [B.bits(t).clone() for t in (dA, dB, idx_buf)]
    for two in (True, False):
        dx = B.guarded(N * H * W * C, BF16, dev)
        L.check(lib.gs_maxpool_bwd(dA.data_ptr(), dB.data_ptr() if two else None, idx.data_ptr(), dx.data_ptr(),
                                   N, H, W, C, stream), "gs_maxpool_bwd")
        torch.cuda.synchronize()
        for k, v in (("dA", dA), ("dB", dB), ("idx", idx_buf), ("dx", dx)):
            assert B.guards_intact(v), f"gs_maxpool_bwd wrote outside {k}"
        for t, s in zip((dA, dB, idx_buf), snaps):
            assert torch.equal(B.bits(t), s), "gs_maxpool_bwd changed an input"
        grad = (dA + dB) if two else dA  # ATen's bf16 add
        grad = _as_nchw(grad, oshape)
        want_dx = torch.ops.aten.max_pool2d_with_indices_backward(
            grad, relu_y, [3, 3], [2, 2], [1, 1], [1, 1], False, aten_idx.permute(0, 3, 1, 2))
        want_dx = want_dx.permute(0, 2, 3, 1).contiguous()
        bad = torch.nonzero(B.bits(dx.view(shape)) != B.bits(want_dx))
        assert bad.numel() == 0, (two, bad.shape[0], bad[:4].tolist(),
                                  [hex(int(B.bits(dx.view(shape))[tuple(b)]) & 0xFFFF) for b in bad[:4]],
                                  [hex(int(B.bits(want_dx)[tuple(b)]) & 0xFFFF) for b in bad[:4]])
