"""References and fixtures for the resize-based input step (tests/test_resample_cpu.py, tests/test_gpu_resample.py).
Written from the contract of gs_image_resample in include/gsync.h and from the docstring of
data.RandomResizedCropFlip; the references do not call the new entry (``run_resample`` is the tests' shared call).

``resample_ref`` is the contract in numpy: every operation is one numpy float32 operation (one rounding each, no
fma), the taps are ``float32(u8) / float32(255)``.  It is compared bit for bit.  ``device=True`` applies what the
HIP backend documents for records it cannot reject: an index outside the set gives zeros and label 0, a box is
clamped into the image.

``draw_records_scalar`` restates the record draw sample by sample: the same three array draws from PCG64 seeded
``[seed, rank]``, then torchvision's ``get_params`` per sample in numpy float64 scalar operations.
"""
import functools

import numpy as np
import torch

F32 = np.float32
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---- records ---------------------------------------------------------------------------------------------------
def record(index, flip, top, left, h, w):
    return [index, flip, np.uint32(top | (left << 16)).view(np.int32), np.uint32(h | (w << 16)).view(np.int32)]


def decode(row):
    tl, hw = int(np.int32(row[2]).view(np.uint32)), int(np.int32(row[3]).view(np.uint32))
    return int(row[0]), int(row[1]), tl & 0xFFFF, tl >> 16, hw & 0xFFFF, hw >> 16


def random_records(B, n, H, W, seed):
    """valid records: random non-empty boxes inside the image, every second sample flipped"""
    g = np.random.default_rng(seed)
    rec = []
    for i in range(B):
        h, w = int(g.integers(1, H + 1)), int(g.integers(1, W + 1))
        rec.append(record(int(g.integers(n)), (i + seed) % 2, int(g.integers(H - h + 1)), int(g.integers(W - w + 1)), h, w))
    return np.asarray(rec, dtype=np.int32)


def draw_records_scalar(idx, H, W, scale, ratio, flip, seed, rank, skip=()):
    """the records data.RandomResizedCropFlip(size, scale, ratio, flip, seed=seed, rank=rank) draws for the batch
    ``idx``, after batches of the sizes in ``skip``; one sample at a time"""
    rng = np.random.Generator(np.random.PCG64([seed, rank]))
    for B in tuple(skip) + (len(idx),):
        u = rng.random((B, 10, 2))
        f = rng.random(B)
        pos = rng.random((B, 2))
    rec = []
    for i in range(len(idx)):
        box = None
        for k in range(10):
            area = H * W * (scale[0] + u[i, k, 0] * (scale[1] - scale[0]))
            r = np.exp(np.log(ratio[0]) + u[i, k, 1] * (np.log(ratio[1]) - np.log(ratio[0])))
            w, h = int(np.rint(np.sqrt(area * r))), int(np.rint(np.sqrt(area / r)))
            if 0 < w <= W and 0 < h <= H:
                box = (int(np.floor(pos[i, 0] * (H - h + 1))), int(np.floor(pos[i, 1] * (W - w + 1))), h, w)
                break
        if box is None:
            in_ratio = float(W) / float(H)
            if in_ratio < min(ratio):
                w, h = W, int(round(W / min(ratio)))
            elif in_ratio > max(ratio):
                h, w = H, int(round(H * max(ratio)))
            else:
                w, h = W, H
            h, w = min(max(h, 1), H), min(max(w, 1), W)
            box = ((H - h) // 2, (W - w) // 2, h, w)
        rec.append(record(int(idx[i]), int(flip and f[i] < 0.5), *box))
    return np.asarray(rec, dtype=np.int32)


# ---- the contract in numpy -------------------------------------------------------------------------------------
def taps(d, n, V):
    """(i0, i1, l0, l1) of the output coordinates ``d`` along an axis with box extent n and virtual extent V"""
    scale = F32(n) / F32(V)
    s = (d.astype(F32) + F32(0.5)) * scale - F32(0.5)
    s = np.maximum(s, F32(0))
    i0 = np.minimum(s.astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = s - i0.astype(F32)
    l0 = F32(1) - l1
    assert s.dtype == l0.dtype == l1.dtype == F32
    return i0, i1, l0, l1


def resample_ref(imgs, labels, rec, out_hw, frame, mean=None, std=None, device=False):
    """-> (fp32 NCHW numpy [B, C, oh, ow], labels int64 numpy).  imgs: uint8 numpy [N, H, W, C]."""
    N, H, W, C = imgs.shape
    oh, ow = out_hw
    vh, vw, oy, ox = frame
    out = np.zeros((len(rec), C, oh, ow), dtype=F32)
    lab = np.zeros(len(rec), dtype=np.int64)
    for b, row in enumerate(rec):
        idx, flip, top, left, h, w = decode(row)
        if device:
            if not 0 <= idx < N:
                continue
            top, left = min(top, H - 1), min(left, W - 1)
            h, w = max(1, min(h, H - top)), max(1, min(w, W - left))
        assert 0 <= idx < N and h > 0 and w > 0 and top + h <= H and left + w <= W
        lab[b] = labels[idx]
        p = imgs[idx, top:top + h, left:left + w].astype(F32) / F32(255)
        y0, y1, wy0, wy1 = taps(np.arange(oh) + oy, h, vh)
        xs = np.arange(ow)
        x0, x1, wx0, wx1 = taps((ow - 1 - xs if flip else xs) + ox, w, vw)
        wx0, wx1, wy0, wy1 = wx0[None, :, None], wx1[None, :, None], wy0[:, None, None], wy1[:, None, None]
        t = p[y0][:, x0] * wx0 + p[y0][:, x1] * wx1
        u = p[y1][:, x0] * wx0 + p[y1][:, x1] * wx1
        o = t * wy0 + u * wy1
        if mean is not None:
            o = (o - np.asarray(mean, dtype=F32)) / np.asarray(std, dtype=F32)
        assert o.dtype == F32
        out[b] = o.transpose(2, 0, 1)
    return out, lab


def torch_ref(imgs, rec, out_hw, frame, mean=None, std=None):
    """torch's own fp32 CPU result on the same boxes: F.interpolate of x / 255 (the whole virtual frame, then the
    slice at the offset) -> flip -> normalise.  -> fp32 NCHW tensor"""
    oh, ow = out_hw
    vh, vw, oy, ox = frame
    x = torch.from_numpy(imgs).permute(0, 3, 1, 2).to(torch.float32) / 255
    out = []
    for row in rec:
        idx, flip, top, left, h, w = decode(row)
        o = torch.nn.functional.interpolate(x[idx:idx + 1, :, top:top + h, left:left + w], size=(vh, vw), mode="bilinear",
                                            align_corners=False, antialias=False)[0]
        if flip:  # x' = ow - 1 - x, then d_x = x' + off_x: slice, then flip
            o = o[:, oy:oy + oh, ox:ox + ow].flip(-1)
        else:
            o = o[:, oy:oy + oh, ox:ox + ow]
        if mean is not None:
            o = (o - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None]
        out.append(o)
    return torch.stack(out)


def torch_atol(rec, std):
    """Both sides form the source coordinate in fp32, so they differ by a few ulp of the coordinate (at most the box
    extent) times a tap difference <= 1, plus the roundings of the blend: (4 ulp32(max(h, w)) + 16 * 2^-24) / min(std)
    over the batch's largest box.  A wrong tap or weight is off by O(0.1)."""
    ext = max(max(decode(r)[4:]) for r in rec)
    return (4 * float(np.spacing(F32(ext))) + 16 * 2.0 ** -24) / (min(std) if std is not None else 1.0)


# ---- the cases -------------------------------------------------------------------------------------------------
def _images(n, H, W, C, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (n, H, W, C), dtype=np.uint8), g.integers(0, 10, n)


def _case(n, H, W, C, out_hw, rec, frame=None, seed=0):
    imgs, labels = _images(n, H, W, C, seed)
    frame = frame if frame is not None else (out_hw[0], out_hw[1], 0, 0)
    return dict(imgs=imgs, labels=labels, rec=np.asarray(rec, dtype=np.int32), out_hw=out_hw, frame=frame)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> dict(imgs, labels, rec, out_hw, frame); built once and never modified"""
    if name in ("40x48-b1", "40x48-b3", "40x48-b100"):
        B = int(name.split("b")[1])
        return _case(23, 40, 48, 3, (32, 32), random_records(B, 23, 40, 48, seed=B), seed=1)
    if name == "33x47":  # C * oh * ow = 1479: not a multiple of 4
        return _case(11, 33, 47, 3, (17, 29), random_records(3, 11, 33, 47, seed=5), seed=2)
    if name == "upscale":  # every clamp is active: 1x1, 1xw, hx1 and 2x3 boxes
        rec = [record(0, 0, 7, 9, 1, 1), record(1, 1, 39, 47, 1, 1), record(2, 0, 3, 0, 1, 48), record(3, 1, 0, 5, 40, 1),
               record(4, 0, 11, 13, 2, 3), record(5, 1, 38, 45, 2, 3)]
        return _case(7, 40, 48, 3, (32, 32), rec, seed=3)
    if name == "edges":  # a box on each image edge, each corner, and the whole image, both flips
        rec = [record(0, 0, 0, 5, 17, 20), record(1, 1, 23, 5, 17, 20), record(2, 0, 9, 0, 20, 13), record(3, 1, 9, 35, 20, 13),
               record(4, 0, 0, 0, 40, 48), record(5, 1, 0, 0, 40, 48), record(6, 0, 0, 0, 13, 11), record(6, 1, 27, 37, 13, 11)]
        return _case(7, 40, 48, 3, (32, 32), rec, seed=4)
    if name in ("c1", "c4"):
        C = int(name[1])
        return _case(9, 40, 48, C, (32, 32), random_records(3, 9, 40, 48, seed=6 + C), seed=5)
    if name == "500x375":  # extreme downscale
        rec = [record(0, 0, 0, 0, 500, 375), record(1, 1, 3, 7, 480, 360), record(2, 1, 100, 50, 333, 250)]
        return _case(3, 500, 375, 3, (8, 8), rec, seed=6)
    if name == "256to224":  # several bands per sample
        rec = [record(0, 0, 0, 0, 256, 256), record(1, 1, 5, 9, 240, 200), record(2, 0, 100, 60, 150, 190),
               record(3, 1, 30, 20, 90, 120)]
        return _case(4, 256, 256, 3, (224, 224), rec, seed=7)
    if name == "256to224-b8":
        rec = np.concatenate([case("256to224")["rec"], random_records(4, 4, 256, 256, seed=8)])
        return _case(4, 256, 256, 3, (224, 224), rec, seed=7)
    if name == "eval36-32":  # ResizeCenterCrop(36, 32) on 40x48: the whole image resized to 36x43, cropped at (2, 6)
        rec = [record(i, 0, 0, 0, 40, 48) for i in range(5)]
        return _case(5, 40, 48, 3, (32, 32), rec, frame=(36, 43, 2, 6), seed=8)
    if name == "tall":  # 80 output rows: three bands per sample at a small size, upscaled and flipped
        return _case(5, 40, 48, 3, (80, 36), random_records(4, 5, 40, 48, seed=9), seed=9)
    raise KeyError(name)


CASES = ("40x48-b1", "40x48-b3", "40x48-b100", "33x47", "upscale", "edges", "c1", "c4", "500x375", "256to224", "eval36-32",
         "tall")


def norm_of(name, normalise):
    """the mean / std a case is normalised with: ImageNet's for 3 channels"""
    if not normalise:
        return None, None
    C = case(name)["imgs"].shape[3]
    return ((0.485, 0.456, 0.406, 0.5)[:C], (0.229, 0.224, 0.225, 0.25)[:C]) if C != 1 else ((0.45,), (0.225,))


@functools.lru_cache(maxsize=None)
def reference(name, normalise):
    """resample_ref of a case, computed once: (fp32 NCHW tensor, labels tensor)"""
    c = case(name)
    mean, std = norm_of(name, normalise)
    out, lab = resample_ref(c["imgs"], c["labels"], c["rec"], c["out_hw"], c["frame"], mean, std)
    return torch.from_numpy(out), torch.from_numpy(lab)


# ---- the shared call -------------------------------------------------------------------------------------------
SENTINEL = 7.0


def run_resample(lib, c, dtype, channels_last, mean=None, std=None, device=None, guard=0, rec=None, frame=None,
                 shift=0):
    """gs_image_resample on the host backend (device None) or on ``device`` for the case dict ``c``.  -> (rc, images
    as a logical NCHW CPU tensor, labels, the image buffer's guard region, the label buffer's guard region):
    ``guard`` sentinel elements follow the images and the labels; ``shift`` elements precede the images, so that
    ``out`` is not 16-byte aligned."""
    import ctypes

    from distributed_training_amd import _lib as L

    imgs, labels = torch.from_numpy(c["imgs"]), torch.from_numpy(c["labels"])
    rec = torch.as_tensor(c["rec"] if rec is None else rec, dtype=torch.int32).contiguous()
    N, H, W, C = imgs.shape
    oh, ow = c["out_hw"]
    vh, vw, oy, ox = c["frame"] if frame is None else frame
    B = rec.shape[0]
    dev = torch.device("cpu") if device is None else device
    kind = L.GS_DEV_HOST if device is None else L.GS_DEV_HIP
    n_out = B * C * oh * ow
    buf = torch.full((shift + n_out + guard,), SENTINEL, dtype=dtype, device=dev)
    lab = torch.full((B + guard,), -7, dtype=torch.int64, device=dev)
    di, dl, dr = imgs.to(dev), labels.to(dev), rec.to(dev)
    cm = None if mean is None else (ctypes.c_float * len(mean))(*mean)
    cs = None if std is None else (ctypes.c_float * len(std))(*std)
    rc = lib.gs_image_resample(kind, dev.index or 0, di.data_ptr(), dl.data_ptr(), N, H, W, C, oh, ow, vh, vw, oy, ox,
                               dr.data_ptr(), B, cm, cs, buf.data_ptr() + shift * buf.element_size(), L.gs_dtype(dtype),
                               L.GS_LAYOUT_NHWC if channels_last else L.GS_LAYOUT_NCHW, lab.data_ptr(),
                               L.stream_ptr(dev))
    if device is not None:
        torch.cuda.synchronize()
    flat = buf.cpu()
    assert bool((flat[:shift] == SENTINEL).all())
    img = flat[shift:shift + n_out]
    img = img.view(B, oh, ow, C).permute(0, 3, 1, 2) if channels_last else img.view(B, C, oh, ow)
    lab = lab.cpu()
    return rc, img, lab[:B], flat[shift + n_out:], lab[B:]


def same_bits(a, b):
    """bitwise equality of two tensors of one floating dtype (-0 differs from +0)"""
    view = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


COMBOS = [(cl, dt, nm) for cl in (False, True) for dt in (torch.float32, torch.bfloat16) for nm in (False, True)]


def combo_id(combo):
    cl, dt, nm = combo
    return f"{'nhwc' if cl else 'nchw'}-{'f32' if dt == torch.float32 else 'bf16'}-{'norm' if nm else 'plain'}"
