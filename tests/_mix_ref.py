"""References and fixtures for the MixUp / CutMix tests (tests/test_mix_cpu.py, tests/test_xent_mix_cpu.py,
tests/test_gpu_mix.py, tests/test_gpu_xent_mix.py).  Written from the contracts of gs_image_augment_mix,
gs_xent_mix_fwd and gs_xent_mix_bwd in include/gsync.h; the references do not call the new entries
(``run_augment_mix`` and ``run_xent_mix`` are the tests' shared calls of them).

Images.  ``mix_images_ref`` is the contract in numpy fp32 on top of the unmixed batch of the existing host path
(``unmixed_batch``: gs_image_augment, itself pinned to the reference pipeline by tests/test_data_cpu.py): paste
inside a non-empty box, else ``a * lam + b * (1.f - lam)`` with every operation an fp32 numpy operation (one
rounding each), else the sample alone.  Everything is compared bit for bit.

Criterion.  ``xent_mix_ref`` builds on ``tests._xent_ref.xent_ref`` (u = 2^-24; its bounds are derived in
tests/test_xent_cpu.py).  With ref_a and ref_b the one-label references for the labels a and b of every row:

* a skipped, bad or one-label row (lam == 1 or a == b) takes ref_a's values and bounds unchanged;
* a mixed row's truth is lam * loss_a + (1 - lam) * loss_b with lam the fp32 value the library reads.  The
  library forms lam1 = fl(1 - lam) (one rounding: at most u, relative to lam1 <= 1), two products and one add.
  With b_a, b_b the one-label bounds of the computed loss_a, loss_b:
    |loss - truth| <= lam b_a + (1 - lam) b_b                      the errors the two losses arrive with
                      + u (|loss_b| + b_b)                         lam1's rounding, times the computed loss_b
                      + u (lam (|loss_a| + b_a) + (1 - lam + u) (|loss_b| + b_b))      the two products
                      + u (lam (|loss_a| + b_a) + (1 - lam + u) (|loss_b| + b_b)) (1 + 2 u)   the add
  which ``xent_mix_ref`` evaluates as written (the (1 + 2 u) covers the products' own roundings inside the sum);
* a mixed row's target is q_mix = lam q(a) + (1 - lam) q(b), q(y) the one-label target, so the true gradient is
  lam dz_a + (1 - lam) dz_b for the same c.  One-label bounds are |c| (e_p + 3 u q + 3 u |p - q|) plus the
  output rounding, all terms convex in q, so lam bound_a + (1 - lam) bound_b bounds the same count of roundings
  at q_mix (|p - q_mix| <= lam |p - q(a)| + (1 - lam) |p - q(b)|).  The mixed targets take more roundings than
  q_on's three: (1 - eps), the product with lam, q_off and the add are four at a; lam1 makes five at b.  Hence
    |dz_j - truth| <= lam bound_a + (1 - lam) bound_b + 2 u |c| q_mix_j (1 + u_out)    (the last term at a and b).
  c = g / counted uses the mixed batch's count: the one-label gradients are asked for per row (``none``) with
  that c.
* code: ref_a's for a one-label row, else the dominant label's (a if lam >= 0.5 else b).
"""
import math

import numpy as np
import torch

from tests import _xent_ref as X
from tests._eval_ref import U32, values64

ONE_BITS = int(np.float32(1.0).view(np.int32))


# ---- records ---------------------------------------------------------------------------------------------------
def bits(lam):
    return int(np.float32(lam).view(np.int32))


def record(partner, lam, box=None):
    y0, y1, x0, x1 = box if box is not None else (0, 0, 0, 0)
    return [partner, bits(lam), np.uint32(y0 | (y1 << 16)).view(np.int32), np.uint32(x0 | (x1 << 16)).view(np.int32)]


def box_lam(box, oh, ow):
    y0, y1, x0, x1 = box
    return np.float32(1.0 - (y1 - y0) * (x1 - x0) / float(oh * ow))


def handmade_records(oh, ow):
    """lam in {0, 2^-24, 0.3, 0.5, 1}, a full-image box, a one-pixel box, a box at each corner, partner == i, and
    a cycle of partners 0 -> 1 -> ... -> 11 -> 0"""
    h2, w2 = oh // 2, ow // 3
    boxes = [(0, oh, 0, ow), (5, 6, 7, 8), (0, h2, 0, w2), (0, h2, ow - w2, ow), (oh - h2, oh, 0, w2),
             (oh - h2, oh, ow - w2, ow)]
    rec = [record(1, 0.0), record(2, 2.0 ** -24), record(3, 0.3), record(4, 0.5), record(5, 1.0)]
    rec += [record(6 + k, box_lam(b, oh, ow), b) for k, b in enumerate(boxes)]
    rec += [record(0, 0.7), record(12, 0.3), record(13, 0.25, (2, 9, 3, 11))]  # 11 closes the cycle; 12, 13: partner == i
    return np.asarray(rec, dtype=np.int32)


def random_records(B, oh, ow, seed):
    """valid records: a third blends, a third pastes, the rest identity or their own partner"""
    g = np.random.default_rng(seed)
    rec = []
    for i in range(B):
        kind = i % 3 if B > 1 else int(g.integers(3))
        partner = int(g.integers(B))
        if kind == 0:
            rec.append(record(partner, g.random(dtype=np.float32)))
        elif kind == 1:
            y0, x0 = int(g.integers(oh)), int(g.integers(ow))
            b = (y0, int(g.integers(y0 + 1, oh + 1)), x0, int(g.integers(x0 + 1, ow + 1)))
            rec.append(record(partner, box_lam(b, oh, ow), b))
        else:
            rec.append(record(i, 1.0) if g.random() < 0.5 else record(i, 0.4))
    return np.asarray(rec, dtype=np.int32)


def decode(rec_row):
    partner = int(rec_row[0])
    lam = np.int32(rec_row[1]).view(np.float32)
    ys, xs = int(np.int32(rec_row[2]).view(np.uint32)), int(np.int32(rec_row[3]).view(np.uint32))
    return partner, lam, (ys & 0xFFFF, ys >> 16, xs & 0xFFFF, xs >> 16)


# ---- images ----------------------------------------------------------------------------------------------------
GEOMETRIES = {  # name: (H, W, pad, crop)
    "cifar": (32, 32, 4, 32),  # the LDS kernel
    "30x30": (30, 30, 2, 30),  # 2,700 bytes per image, not a multiple of 16: the global-gather kernel
    "96x96": (96, 96, 4, 96),  # two images are 55,296 bytes, above the LDS budget: the global-gather kernel
}


def image_case(geometry, B, seed, n=23):
    """a uint8 image set, labels and a valid [B, 4] params table (index, flip, top, left)"""
    H, W, pad, crop = GEOMETRIES[geometry]
    g = np.random.default_rng(seed)
    imgs = torch.from_numpy(g.integers(0, 256, (n, H, W, 3), dtype=np.uint8))
    labels = torch.from_numpy(g.integers(0, 10, n))
    params = np.stack([g.integers(0, n, B), g.integers(0, 2, B), g.integers(0, H + 2 * pad - crop + 1, B),
                       g.integers(0, W + 2 * pad - crop + 1, B)], axis=1).astype(np.int32)
    return imgs, labels, torch.from_numpy(params)


def unmixed_batch(lib, imgs, labels, params, geometry):
    """the existing host path: gs_image_augment, fp32 NCHW, and the gathered labels"""
    from distributed_training_amd import _lib as L

    H, W, pad, crop = GEOMETRIES[geometry]
    B = params.shape[0]
    out = torch.empty(B, 3, crop, crop)
    lab = torch.empty(B, dtype=torch.int64)
    rc = lib.gs_image_augment(L.GS_DEV_HOST, 0, imgs.data_ptr(), labels.data_ptr(), imgs.shape[0], H, W, 3, pad, crop,
                              crop, params.data_ptr(), B, out.data_ptr(), L.GS_F32, L.GS_LAYOUT_NCHW, lab.data_ptr(),
                              None)
    assert rc == 0, lib.gs_last_error()
    return out, lab


def mix_images_ref(base, lab, rec, dtype):
    """the contract on the unmixed fp32 NCHW batch ``base``: -> (images in ``dtype``, labels_b, lam)"""
    a = base.numpy()
    out = a.copy()
    B = a.shape[0]
    lab_b = lab.clone()
    lam_out = np.ones(B, dtype=np.float32)
    for i in range(B):
        partner, lam, (y0, y1, x0, x1) = decode(rec[i])
        lab_b[i] = lab[partner]
        lam_out[i] = lam
        box = y0 < y1 and x0 < x1
        if partner == i or (not box and lam == np.float32(1.0)):
            continue
        if box:
            out[i, :, y0:y1, x0:x1] = a[partner, :, y0:y1, x0:x1]
        else:
            lam1 = np.float32(1.0) - lam
            out[i] = a[i] * lam + a[partner] * lam1  # fp32 arrays and scalars: every operation rounds once
    assert out.dtype == np.float32
    return torch.from_numpy(out).to(dtype), lab_b, torch.from_numpy(lam_out)


def run_augment_mix(lib, imgs, labels, params, rec, geometry, dtype, channels_last, device=None, guard=0):
    """gs_image_augment_mix on the host backend (device None) or on ``device``.  -> (rc, images as a logical
    NCHW CPU tensor, labels_a, labels_b, lam, guard region): ``guard`` sentinel elements follow the images."""
    from distributed_training_amd import _lib as L

    H, W, pad, crop = GEOMETRIES[geometry]
    B = params.shape[0]
    dev = torch.device("cpu") if device is None else device
    kind = L.GS_DEV_HOST if device is None else L.GS_DEV_HIP
    n_out = B * 3 * crop * crop
    buf = torch.full((n_out + guard,), 7.0, dtype=dtype, device=dev)
    la = torch.full((B,), -7, dtype=torch.int64, device=dev)
    lb = torch.full((B,), -7, dtype=torch.int64, device=dev)
    lam = torch.full((B,), -7.0, dtype=torch.float32, device=dev)
    di, dl, dp = imgs.to(dev), labels.to(dev), params.to(dev)
    dr = torch.as_tensor(rec, dtype=torch.int32).contiguous().to(dev)
    rc = lib.gs_image_augment_mix(kind, dev.index or 0, di.data_ptr(), dl.data_ptr(), imgs.shape[0], H, W, 3, pad, crop,
                                  crop, dp.data_ptr(), dr.data_ptr(), B, buf.data_ptr(), L.gs_dtype(dtype),
                                  L.GS_LAYOUT_NHWC if channels_last else L.GS_LAYOUT_NCHW, la.data_ptr(), lb.data_ptr(),
                                  lam.data_ptr(), L.stream_ptr(dev))
    if device is not None:
        torch.cuda.synchronize()
    flat = buf.cpu()
    img = flat[:n_out]
    img = img.view(B, crop, crop, 3).permute(0, 3, 1, 2) if channels_last else img.view(B, 3, crop, crop)
    return rc, img, la.cpu(), lb.cpu(), lam.cpu(), flat[n_out:]


def same_bits(a, b):
    """bitwise equality of two tensors of one floating dtype (a NaN equals the same NaN, -0 differs from +0)"""
    view = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


# ---- criterion -------------------------------------------------------------------------------------------------
def mix_case(Bn, K, dtype, seed, specials=True):
    """``X.xent_case`` logits and labels a, with labels b and lam [B] fp32.  With ``specials`` (and room): row 3
    lam == 1, row 4 a == b, row 5 lam == 0, row 6 lam == 0.5 (the dominant label is a), row 7 lam == 2^-24."""
    logits, a = X.xent_case(Bn, K, dtype, seed)
    gen = torch.Generator().manual_seed(seed + 77)
    b = torch.randint(0, K, (Bn,), generator=gen)
    lam = torch.rand(Bn, generator=gen)
    if specials:
        for row, v in ((3, 1.0), (5, 0.0), (6, 0.5), (7, 2.0 ** -24)):
            if Bn > row:
                lam[row] = v
        if Bn > 4:
            b[4] = a[4]
    return logits, a, b, lam


def xent_mix_ref(z, a, b, lam, eps, dtype, ignore_index=-100):
    """see the module's docstring.  z fp64 [B, K]; a, b int64 numpy; lam fp32 numpy.  -> a dict as ``xent_ref``'s:
    code, loss, loss_bound, on, counted, bad, total, total_bound, kind ('skip', 'bad', 'one', 'mix') and
    grad(reduction, g) -> (dz64, bound)."""
    Bn, K = z.shape
    ra = X.xent_ref(z, a, eps, dtype, ignore_index)
    rb = X.xent_ref(z, b, eps, dtype, ignore_index)
    lam64 = lam.astype(np.float64)
    kind = []
    code = np.zeros(Bn, dtype=np.int64)
    loss, lb = np.zeros(Bn), np.zeros(Bn)
    for r in range(Bn):
        ya, yb, lm = int(a[r]), int(b[r]), lam64[r]
        if ya == ignore_index or yb == ignore_index:
            kind.append("skip")
            code[r] = -1
        elif not (0 <= ya < K and 0 <= yb < K) or not (0.0 <= lm <= 1.0):
            kind.append("bad")
            code[r] = -2
        elif lm == 1.0 or ya == yb:
            kind.append("one")
            code[r], loss[r], lb[r] = ra["code"][r], ra["loss"][r], ra["loss_bound"][r]
        else:
            kind.append("mix")
            code[r] = (ra if lm >= 0.5 else rb)["code"][r]
            la_, lb_ = ra["loss"][r], rb["loss"][r]
            ba, bb = ra["loss_bound"][r], rb["loss_bound"][r]
            if lm == 0.0 and not math.isfinite(la_):
                loss[r] = lb[r] = math.nan  # 0 * inf in the library too
                continue
            with np.errstate(invalid="ignore"):
                loss[r] = lm * la_ + (1 - lm) * lb_
                pa, pb = lm * (abs(la_) + ba), (1 - lm + U32) * (abs(lb_) + bb)
                lb[r] = lm * ba + (1 - lm) * bb + U32 * (abs(lb_) + bb) + U32 * (pa + pb) + U32 * (pa + pb) * (1 + 2 * U32)
    kind = np.asarray(kind)
    on = code >= 0
    total = 0.0
    for r in range(Bn):
        if on[r]:
            total += loss[r]
    counted, bad = int(on.sum()), int((code == -2).sum())

    def grad(reduction, g):
        c = {"mean": lambda: np.full(Bn, g / max(counted, 1)), "sum": lambda: np.full(Bn, float(g)),
             "none": lambda: np.asarray(g, dtype=np.float64)}[reduction]()
        # the library rounds c = g / (float)counted once; xent_ref's "mean" counts that rounding in its 3 u |c|
        # term and "none" counts none, so nothing is lost by asking for the rows one by one with this c
        # (a rounding that is not made is bounded too)
        a_ok = np.where(on, a, 0)
        b_ok = np.where(on, b, 0)
        ga, bda = X.xent_ref(z, a_ok, eps, dtype, ignore_index)["grad"]("none", c)
        gb, bdb = X.xent_ref(z, b_ok, eps, dtype, ignore_index)["grad"]("none", c)
        dz, bound = np.zeros((Bn, K)), np.zeros((Bn, K))
        e32 = float(np.float32(eps))
        u_out = X.U_OUT[dtype]
        for r in range(Bn):
            if kind[r] == "one":
                dz[r], bound[r] = ga[r], bda[r]
            elif kind[r] == "mix":
                lm = lam64[r]
                dz[r] = lm * ga[r] + (1 - lm) * gb[r]
                bound[r] = lm * bda[r] + (1 - lm) * bdb[r]
                for y, w in ((int(a[r]), lm), (int(b[r]), 1 - lm)):
                    bound[r, y] += 2 * U32 * abs(c[r]) * ((1 - e32) * w + e32 / K) * (1 + u_out)
        return dz, bound

    return dict(code=code, loss=loss, loss_bound=lb, on=on, counted=counted, bad=bad, total=total, kind=kind,
                total_bound=float(np.nansum(lb[on])) if counted else 0.0, grad=grad)


def torch_mix_ref(logits, a, b, lam, eps, reduction, g, counted_rows):
    """the torch composition in fp64 on the CPU and its autograd gradient for grad_output g"""
    z = logits.detach().cpu().to(torch.float64).clone().requires_grad_()
    lm = lam.double()
    ce = torch.nn.functional.cross_entropy
    rows = lm * ce(z, a, reduction="none", label_smoothing=eps) + (1 - lm) * ce(z, b, reduction="none",
                                                                                   label_smoothing=eps)
    rows = torch.where(torch.as_tensor(counted_rows), rows, torch.zeros_like(rows))
    out = rows if reduction == "none" else rows.sum() if reduction == "sum" else rows.sum() / int(counted_rows.sum())
    out.backward(torch.as_tensor(g, dtype=torch.float64).reshape(out.shape))
    return out.detach().numpy(), z.grad.numpy()


def run_xent_mix(lib, logits, a, b, lam, eps, reductions=("mean",), device=None, topk=(), acc=None, ignore_index=-100):
    """``X.run_xent`` for gs_xent_mix_fwd / gs_xent_mix_bwd: the same layout (NaN padding, SENTINEL-filled gradient
    buffer with the logits' row stride) and the same result dict"""
    from distributed_training_amd import _lib as L

    Bn, K = logits.shape
    stride = logits.stride(0) if Bn > 1 else max(K, logits.stride(0))
    dev = torch.device("cpu") if device is None else device
    kind = L.GS_DEV_HOST if device is None else L.GS_DEV_HIP
    zl = torch.full((Bn, stride), math.nan, dtype=logits.dtype, device=dev)
    zl[:, :K] = logits.to(dev)
    ya, yb, lm = a.to(dev), b.to(dev), lam.to(torch.float32).to(dev)
    rows = torch.zeros(max(1, Bn) * 4, dtype=torch.float32, device=dev)
    red = torch.zeros(4, dtype=torch.float32, device=dev)
    stream = L.stream_ptr(dev)
    rc = lib.gs_xent_mix_fwd(kind, zl.data_ptr(), L.gs_dtype(zl.dtype), ya.data_ptr(), yb.data_ptr(), lm.data_ptr(), Bn,
                             K, stride, ignore_index, eps, rows.data_ptr(), red.data_ptr(),
                             L.i32_array(topk) if topk else None, len(topk), None if acc is None else acc.data_ptr(),
                             stream)
    assert rc == 0, lib.gs_last_error()
    dz = {}
    for name in reductions:
        gt = torch.as_tensor(X.grad_out_for(name, Bn), dtype=torch.float32).reshape(-1).to(dev)
        d = torch.full((Bn, stride), X.SENTINEL, dtype=logits.dtype, device=dev)
        rc = lib.gs_xent_mix_bwd(kind, zl.data_ptr(), L.gs_dtype(zl.dtype), ya.data_ptr(), yb.data_ptr(), lm.data_ptr(),
                                 Bn, K, stride, ignore_index, eps, X.REDUCTIONS[name], rows.data_ptr(), red.data_ptr(),
                                 gt.data_ptr(), d.data_ptr(), stride, stream)
        assert rc == 0, lib.gs_last_error()
        dz[name] = d
    if device is not None:
        torch.cuda.synchronize()
    rows = rows.cpu()
    redc = red.cpu()
    return dict(rows=rows[:4 * Bn].view(Bn, 4), code=rows.view(torch.int32)[:4 * Bn].view(Bn, 4)[:, 3].clone(),
                red=(float(redc[0]), float(redc[1]), int(redc.view(torch.int32)[2]), int(redc.view(torch.int32)[3])),
                dz={k: v.cpu() for k, v in dz.items()}, K=K)


def check_xent_mix(logits, a, b, lam, eps, out, reductions=("none", "mean", "sum"), against_torch=True):
    """``out`` (run_xent_mix's) against ``xent_mix_ref`` and against the torch composition in fp64, as
    ``X.check_xent`` does for the one-label entries.  -> the worst error / bound seen."""
    Bn, K = logits.shape
    z = values64(logits)
    lam32 = lam.to(torch.float32)
    ref = xent_mix_ref(z, a.numpy(), b.numpy(), lam32.numpy(), eps, logits.dtype)
    assert np.array_equal(out["code"].numpy().astype(np.int64), ref["code"])
    loss_sum, loss_mean, counted, bad = out["red"]
    assert (counted, bad) == (ref["counted"], ref["bad"])
    rows = out["rows"].double().numpy()
    on = ref["on"]
    assert not rows[~on, :3].any()
    worst = X._close(rows[on, 0], ref["loss"][on], ref["loss_bound"][on], "row loss")
    tb = ref["total_bound"]
    if bad:
        assert math.isnan(loss_sum) and math.isnan(loss_mean)
    else:
        worst = max(worst, X._close([loss_sum], [ref["total"]], [tb + U32 * abs(ref["total"])], "loss_sum"))
        if counted:
            mean = ref["total"] / counted
            worst = max(worst, X._close([loss_mean], [mean], [tb / counted + U32 * abs(mean)], "loss_mean"))
        else:
            assert loss_sum == 0.0 and math.isnan(loss_mean)
    de = abs(float(np.float32(eps)) - eps)
    nll = xent_mix_ref(z, a.numpy(), b.numpy(), lam32.numpy(), 0.0, logits.dtype)["loss"] if eps else ref["loss"]
    for name in reductions:
        g = X.grad_out_for(name, Bn)
        full = out["dz"][name].double().numpy()
        got = full[:, :K]
        assert (full[:, K:] == X.SENTINEL).all(), "gradient padding written"
        want, bound = ref["grad"](name, g)
        assert not got[~on].any()
        worst = max(worst, X._close(got[on], want[on], bound[on], f"gradient ({name})"))
        fin = on & np.isfinite(want).all(axis=1)
        assert (np.abs(got[fin].sum(axis=1)) <= bound[fin].sum(axis=1)).all(), "a gradient row does not sum to 0"
        if against_torch and not bad and counted and not np.isnan(z[on]).any() and np.isfinite(ref["loss"][on]).all():
            tl, tg = torch_mix_ref(logits, torch.where(torch.as_tensor(on), a, torch.zeros_like(a)),
                                   torch.where(torch.as_tensor(on), b, torch.zeros_like(b)), lam32, eps, name, g, on)
            gmax = np.abs(g).max()
            X._close(got[on], tg[on], bound[on] + 2 * de * gmax, f"gradient vs torch ({name})")
            slack = de * np.abs(ref["loss"] - nll) / eps if eps else np.zeros(Bn)
            if name == "none":
                X._close(rows[:, 0], tl, ref["loss_bound"] + slack, "loss vs torch (none)")
            elif name == "sum":
                X._close([loss_sum], [tl], [tb + U32 * abs(tl) + np.nansum(slack[on])], "loss vs torch (sum)")
            else:
                X._close([loss_mean], [tl], [tb / counted + U32 * abs(tl) + np.nansum(slack[on]) / counted],
                         "loss vs torch (mean)")
    return worst
