"""Roofline microbenchmark of the grad-sync kernels at BASELINE sizes, beside
the reference's GPU path for the same work (torch ops on the same device).

For ResNet-50 / ResNet-152 parameter sets (real per-tensor shapes) it times,
with HIP events on the stream each kernel is launched on (libgsync rows: the
plan launch timer, events recorded by the library around each kernel; every
row also `batched_*`: the same launches back to back between one event pair):

  libgsync                         reference GPU path (torch 2.10 on ROCm)
  pack fp32 (x 1/ws)   8 B/param    per-param  torch.mul(grad, 1/ws, out=bucket_view)  (Reducer mark_variable_ready_dense)
  pack fp32->bf16      6 B/param    per-param  bucket_view.copy_(grad.mul(1/ws))
  unpack fp32          8 B/param    per-param  grad.copy_(bucket_view)                 (copy_bucket_to_grad)
  SGD momentum+wd     20 B/param    torch.optim.SGD foreach=True  step
  Adam                28 B/param    torch.optim.Adam foreach=True step
  sq-norm              4 B/param    torch._foreach_norm + stack/norm (clip_grad_norm_)
  LARS norms           8 B/param    torch._foreach_norm(params), torch._foreach_norm(grads)
  LARS update         20 B/param    (timed in-step, right behind its norms pass)
  LARS step           28 B/param    the two norms + trust ratios + foreach add / mul_ / add_ / mul / add_
  LAMB moments        24 B/param    (p, g, m, v read; m, v written; per-tensor sums of p^2, u^2)
  LAMB update         16 B/param    (timed in-step, right behind its moments pass)
  LAMB step           40 B/param    foreach lerp_ / mul_ / addcmul_ / sqrt / div / add + the two norms + ratios + add_
  EMA fp32            12 B/param    torch._foreach_lerp_ (AveragedModel.update_parameters)
  EMA + bf16 copy     14 B/param    (fp32 shadow of a bf16 model, the copy written in the same pass)
  EMA bf16 source     10 B/param

Working sets are replicated `--replicas` times so the timed data exceeds the
256 MiB Infinity Cache (true HBM rates).  Prints one JSON object per kernel.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK = 8000.0


_LAST = {}


def timeit_plan(plan, fn, iters=20, warmup=3, kind=None, per=1):
    """libgsync launches: the plan launch timer (HIP events recorded by the
    library right around each kernel on its stream).  `fn` makes `per` timed
    launches; `kind` keeps the records of one GS_OP_* kind."""
    _LAST["fn"] = fn
    for _ in range(warmup):
        fn()
    plan.timer_enable(iters * per)
    for _ in range(iters):
        fn()
    ts = sorted(plan.timer_read(kind=kind))
    plan.timer_enable(0)
    return ts[len(ts) // 2], sum(ts) / len(ts)


def timeit_batched(fn, iters=20):
    """`iters` back-to-back launches between ONE pair of HIP events on the
    current stream (launch gaps included, no per-launch event cost)."""
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(iters):
        fn()
    b.record(s)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def timeit(fn, iters=20, warmup=3):
    for _ in range(warmup):
        fn()
    _LAST["fn"] = fn
    s = torch.cuda.current_stream()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record(s)
        fn()
        b.record(s)
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return ts[len(ts) // 2], sum(ts) / len(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--replicas", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated row-name prefixes to run (default: all rows)")
    ap.add_argument("--tag", default=os.environ.get("GSYNC_LIB", "libgsync").split("/")[-1])
    args = ap.parse_args()
    from distributed_training_amd.multi_tensor import TensorListPlan
    from distributed_training_amd.resnet import MODELS

    dev = torch.device("cuda", 0)
    shapes = [p.shape for p in MODELS[args.model]().parameters()] * args.replicas
    n = sum(torch.Size(s).numel() for s in shapes)
    g = torch.Generator(device=dev).manual_seed(0)
    mk = lambda scale=1.0: [torch.randn(s, device=dev, generator=g) * scale for s in shapes]  # noqa: E731
    params, grads, bufs = mk(), mk(0.01), mk(0.01)
    ms, vs = mk(0.01), [x.abs() for x in mk(1e-4)]
    plan = TensorListPlan([torch.Size(s).numel() for s in shapes], dev, align=64)
    flat = torch.zeros(plan.flat_numel, device=dev)
    flat16 = torch.zeros(plan.flat_numel, device=dev, dtype=torch.bfloat16)
    offs = plan.offsets
    views = [flat[o:o + torch.Size(s).numel()].view(s) for o, s in zip(offs, shapes)]
    views16 = [flat16[o:o + torch.Size(s).numel()].view(s) for o, s in zip(offs, shapes)]
    out = []
    only = [o for o in args.only.split(",") if o]

    def want(*names):
        return not only or any(nm.startswith(o) for nm in names for o in only)

    last_fn = _LAST

    def rec(name, nbytes, ms_med, ms_avg, impl, **extra):
        gbs = nbytes / (ms_avg * 1e-3) / 1e9
        row = {"kernel": name, "impl": impl, "model": args.model, "replicas": args.replicas, "params": n,
               "tag": args.tag, "task_units": plan.task_units, "n_tasks": plan.n_tasks,
               "alg_bytes": nbytes, "median_ms": ms_med, "avg_ms": ms_avg, "GBps": gbs, "frac_of_8TBps": gbs / HBM_PEAK}
        row.update(extra)
        if "fn" in last_fn:  # the same launches, batched between one event pair
            bms = timeit_batched(last_fn.pop("fn"), args.iters)
            bgbs = nbytes / (bms * 1e-3) / 1e9
            row.update({"batched_avg_ms": bms, "batched_GBps": bgbs, "batched_frac_of_8TBps": bgbs / HBM_PEAK})
        out.append(row)
        print(json.dumps(row), flush=True)

    plan.set_ptrs(1, grads)
    plan.set_ptrs(2, grads)
    if want("pack", "unpack_f32"):
        rec("pack_f32", 8 * n, *timeit_plan(plan, lambda: plan.pack(1, torch.float32, flat, 0.125, 1), args.iters), "libgsync")
        rec("pack_f32_to_bf16", 6 * n, *timeit_plan(plan, lambda: plan.pack(1, torch.float32, flat16, 0.125, 1), args.iters), "libgsync")
        rec("unpack_f32", 8 * n, *timeit_plan(plan, lambda: plan.unpack(flat, 2, torch.float32), args.iters), "libgsync")
    sq = torch.zeros(1, device=dev)
    if want("unpack_f32+sqnorm"):
        rec("unpack_f32+sqnorm", 8 * n, *timeit_plan(plan, lambda: plan.unpack(flat, 2, torch.float32, sqnorm=sq), args.iters), "libgsync")
    if want("sqnorm"):
        rec("sqnorm_f32", 4 * n, *timeit_plan(plan, lambda: plan.sqnorm(1, torch.float32, sq), args.iters), "libgsync")
    # the update kernels run on an update plan, as FusedSGD / FusedAdam build it
    from distributed_training_amd.multi_tensor import update_task_units

    plan = TensorListPlan([torch.Size(s).numel() for s in shapes], dev, task_units=update_task_units(dev))
    plan.set_ptrs(0, params)
    plan.set_ptrs(1, grads)
    plan.set_ptrs(2, bufs)
    if want("sgd"):
        rec("sgd_momentum_wd", 20 * n, *timeit_plan(
            plan, lambda: plan.sgd(torch.float32, 1e-6, 0.9, 0.0, 1e-4, False, False, False), args.iters), "libgsync")
    # LARS (FusedLARS's two launches; 1-D tensors unadapted, as its default): the norms
    # alone, the update as it runs in a step (right behind the norms pass that read the
    # same p and g), and the pair
    from distributed_training_amd import _lib as L

    plan.set_adapt([len(s) > 1 for s in shapes])
    nrm = torch.zeros(2 * len(shapes), device=dev)
    lars_args = (torch.float32, 1e-6, 0.9, 1e-4, 1e-3, 1e-8, nrm)

    def lars_step():
        plan.lars_norms(torch.float32, nrm)
        plan.lars(*lars_args)

    if want("lars"):
        rec("lars_norms", 8 * n, *timeit_plan(plan, lambda: plan.lars_norms(torch.float32, nrm), args.iters), "libgsync")
        upd = timeit_plan(plan, lars_step, args.iters, kind=L.GS_OP_LARS, per=2)
        _LAST.pop("fn")  # the update is not launched alone: no batched figure for it
        rec("lars_update", 20 * n, *upd, "libgsync")
        # the same update writing a bf16 copy of the new p (slot 3, gs_lars_step_lowp: ZeRO's
        # 16-bit model), timed the same way, then the plain update once more: the two plain
        # figures are this run's own spread (`plain_again_ms`)
        lowp = [torch.zeros(s, device=dev, dtype=torch.bfloat16) for s in shapes]  # kept: slot 3 / 4 point at it
        plan.set_ptrs(3, lowp)

        def lars_step_lowp():
            plan.lars_norms(torch.float32, nrm)
            plan.lars(*lars_args, lowp_dtype=torch.bfloat16)

        upd16 = timeit_plan(plan, lars_step_lowp, args.iters, kind=L.GS_OP_LARS, per=2)
        again = timeit_plan(plan, lars_step, args.iters, kind=L.GS_OP_LARS, per=2)
        _LAST.pop("fn")
        rec("lars_update+bf16", 22 * n, *upd16, "libgsync", plain_ms=upd[0], plain_again_ms=again[0],
            ratio_to_plain=upd16[0] / upd[0], byte_ratio=22 / 20)
        both = timeit(lars_step, args.iters)  # one event pair around the two launches
        rec("lars_step", 28 * n, *both, "libgsync")
    plan.set_ptrs(2, ms)
    plan.set_ptrs(3, vs)
    if want("adam"):
        rec("adam", 28 * n, *timeit_plan(
            plan, lambda: plan.adam(torch.float32, 1e-6, 0.9, 0.999, 1e-8, 0.0, False, False, -1e-6, 0.5), args.iters),
            "libgsync")
    # LAMB (FusedLAMB's two launches on the same four streams; 1-D tensors unadapted, as its
    # default): the moments pass alone, the update as it runs in a step (right behind the
    # moments pass that wrote m, v and read p), and the pair
    lamb_hp = (1e-6, 0.01, 0.1, 0.0316)  # eps, wd, bc1, bc2s

    def lamb_moments():
        plan.lamb_moments(torch.float32, 0.9, 0.999, *lamb_hp, nrm)

    def lamb_step():
        lamb_moments()
        plan.lamb(1e-6, *lamb_hp, nrm)

    if want("lamb"):
        rec("lamb_moments", 24 * n, *timeit_plan(plan, lamb_moments, args.iters), "libgsync")
        upd = timeit_plan(plan, lamb_step, args.iters, kind=L.GS_OP_LAMB, per=2)
        _LAST.pop("fn")  # the update is not launched alone: no batched figure for it
        rec("lamb_update", 16 * n, *upd, "libgsync")
        # ... and with the bf16 copy of the new p (slot 4, gs_lamb_step_lowp), as lars_update+bf16
        lowp16 = [torch.zeros(s, device=dev, dtype=torch.bfloat16) for s in shapes]  # kept, as above
        plan.set_ptrs(4, lowp16)

        def lamb_step_lowp():
            lamb_moments()
            plan.lamb(1e-6, *lamb_hp, nrm, lowp_dtype=torch.bfloat16)

        upd16 = timeit_plan(plan, lamb_step_lowp, args.iters, kind=L.GS_OP_LAMB, per=2)
        again = timeit_plan(plan, lamb_step, args.iters, kind=L.GS_OP_LAMB, per=2)
        _LAST.pop("fn")
        rec("lamb_update+bf16", 18 * n, *upd16, "libgsync", plain_ms=upd[0], plain_again_ms=again[0],
            ratio_to_plain=upd16[0] / upd[0], byte_ratio=18 / 16)
        both = timeit(lamb_step, args.iters)  # one event pair around the two launches
        rec("lamb_step", 40 * n, *both, "libgsync")
    # EMA / SWA weight averaging (gs_ema_step, as AveragedModel launches it): the average against
    # the fp32 parameters, the same with the bf16 copy of the new average, and a bf16 source;
    # torch's path for the same work is _foreach_lerp_
    if want("ema"):
        numels = [torch.Size(s).numel() for s in shapes]
        eplan = TensorListPlan(numels, dev, task_units=update_task_units(dev))
        avg = [p.clone() for p in params]
        src16 = [p.bfloat16() for p in params]
        avg16 = [torch.zeros(s, device=dev, dtype=torch.bfloat16) for s in shapes]
        eplan.set_ptrs(0, avg)
        eplan.set_ptrs(1, params)
        eplan.set_ptrs(2, avg16)
        rec("ema_f32", 12 * n, *timeit_plan(eplan, lambda: eplan.ema(torch.float32, 1e-4), args.iters,
                                            kind=L.GS_OP_EMA), "libgsync")
        rec("ema_f32_copy_bf16", 14 * n, *timeit_plan(
            eplan, lambda: eplan.ema(torch.float32, 1e-4, lowp_dtype=torch.bfloat16), args.iters, kind=L.GS_OP_EMA),
            "libgsync")
        eplan.set_ptrs(1, src16)
        rec("ema_bf16src", 10 * n, *timeit_plan(eplan, lambda: eplan.ema(torch.bfloat16, 1e-4), args.iters,
                                                kind=L.GS_OP_EMA), "libgsync")
        if not args.skip_torch:
            tavg = [p.clone() for p in params]
            rec("ema_f32", 12 * n, *timeit(lambda: torch._foreach_lerp_(tavg, params, 1e-4), args.iters),
                "torch _foreach_lerp_")
            del tavg
        eplan.close()
        del avg, src16, avg16
    # the training criterion (gs_xent_fwd + gs_xent_bwd through loss.cross_entropy): forward plus backward
    # with label smoothing, beside torch's path on the same tensors as autocast runs it (the logits cast to
    # fp32 first), both from this run.  Latency-bound: the row's point is the time and the launch count.
    if want("xent"):
        import torch.nn.functional as F

        from distributed_training_amd.loss import cross_entropy

        def launches(fn):
            """device kernels (and memsets / copies) one call of fn enqueues, or None without a profiler"""
            try:
                from torch.profiler import ProfilerActivity, profile

                fn()
                torch.cuda.synchronize()
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    fn()
                    torch.cuda.synchronize()
                return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
            except Exception:  # noqa: BLE001
                return None

        for Bx, Kx, dt in ((256, 1000, torch.bfloat16), (100, 10, torch.float32)):
            zx = (torch.randn(Bx, Kx, device=dev, generator=g) * 3).to(dt).requires_grad_()
            yx = torch.randint(0, Kx, (Bx,), device=dev, generator=g)

            def fused_step():
                zx.grad = None
                cross_entropy(zx, yx, label_smoothing=0.1).backward()

            def torch_step():
                zx.grad = None
                F.cross_entropy(zx.float(), yx, label_smoothing=0.1).backward()

            t_ms = timeit(torch_step, args.iters)
            t_batched = timeit_batched(torch_step, args.iters)
            t_n = launches(torch_step)
            f_n = launches(fused_step)
            f_ms = timeit(fused_step, args.iters)
            rec("xent_step", 3 * Bx * Kx * zx.element_size(), *f_ms, "libgsync", B=Bx, K=Kx, dtype=str(dt)[6:],
                label_smoothing=0.1, launches=f_n, torch_median_ms=t_ms[0], torch_avg_ms=t_ms[1],
                torch_batched_avg_ms=t_batched, torch_launches=t_n, ratio_to_torch=f_ms[0] / t_ms[0])
    # the pair-target criterion (gs_xent_mix_fwd + gs_xent_mix_bwd through loss.cross_entropy with a MixedTarget)
    # beside the one-label criterion and the torch two-call composition on the same logits, all from this run
    if want("xent_mix"):
        import torch.nn.functional as F

        from distributed_training_amd.data import MixedTarget
        from distributed_training_amd.loss import cross_entropy

        Bx, Kx, dt = 256, 1000, torch.bfloat16
        zx = (torch.randn(Bx, Kx, device=dev, generator=g) * 3).to(dt).requires_grad_()
        tx = MixedTarget(torch.randint(0, Kx, (Bx,), device=dev, generator=g),
                         torch.randint(0, Kx, (Bx,), device=dev, generator=g),
                         torch.rand(Bx, device=dev, generator=g))

        def mix_step():
            zx.grad = None
            cross_entropy(zx, tx, label_smoothing=0.1).backward()

        def one_step():
            zx.grad = None
            cross_entropy(zx, tx.labels_a, label_smoothing=0.1).backward()

        def torch_mix_step():
            zx.grad = None
            z32 = zx.float()
            (tx.lam * F.cross_entropy(z32, tx.labels_a, reduction="none", label_smoothing=0.1)
             + (1 - tx.lam) * F.cross_entropy(z32, tx.labels_b, reduction="none", label_smoothing=0.1)).mean().backward()

        o_ms, t_ms = timeit(one_step, args.iters), timeit(torch_mix_step, args.iters)
        t_batched = timeit_batched(torch_mix_step, args.iters)
        o_batched = timeit_batched(one_step, args.iters)
        f_ms = timeit(mix_step, args.iters)
        rec("xent_mix_step", 3 * Bx * Kx * zx.element_size(), *f_ms, "libgsync", B=Bx, K=Kx, dtype=str(dt)[6:],
            label_smoothing=0.1, xent_median_ms=o_ms[0], xent_avg_ms=o_ms[1], xent_batched_avg_ms=o_batched,
            torch_median_ms=t_ms[0], torch_avg_ms=t_ms[1], torch_batched_avg_ms=t_batched,
            ratio_to_torch=f_ms[0] / t_ms[0], ratio_to_xent=f_ms[0] / o_ms[0])
    # the mixed input step (gs_image_augment_mix) at CIFAR geometry, half the records blends and half pastes,
    # beside the unmixed gs_image_augment and gs_image_augment followed by the torch composition of the same mix
    # (a gather, two multiplies, an add, a masked select), all from this run
    if want("augment_mix"):
        import numpy as np

        from distributed_training_amd import data as D

        ds = D.ImageDataset.synthetic(50000, device=dev, seed=0)
        for Ba in (256, 4096):
            rng = np.random.default_rng(Ba)
            prm = np.stack([rng.integers(0, ds.n, Ba), rng.integers(0, 2, Ba), rng.integers(0, 9, Ba),
                            rng.integers(0, 9, Ba)], axis=1).astype(np.int32)
            recs = np.zeros((Ba, 4), dtype=np.int32)
            recs[:, 0] = rng.permutation(Ba)
            lam_np = rng.random(Ba, dtype=np.float32)
            paste = np.arange(Ba) % 2 == 1
            lam_np[paste] = np.float32(1.0 - 16 * 16 / 1024.0)
            recs[:, 1] = lam_np.view(np.int32)
            recs[paste, 2] = 8 | (24 << 16)
            recs[paste, 3] = 8 | (24 << 16)
            dprm, drec = torch.from_numpy(prm).to(dev), torch.from_numpy(recs).to(dev)
            xa = torch.empty(Ba, 3, 32, 32, device=dev)
            la, lb_ = torch.empty(Ba, dtype=torch.int64, device=dev), torch.empty(Ba, dtype=torch.int64, device=dev)
            lm = torch.empty(Ba, device=dev)
            perm = torch.from_numpy(recs[:, 0].astype(np.int64)).to(dev)
            lam_t = torch.from_numpy(lam_np).to(dev).view(Ba, 1, 1, 1)
            box = torch.zeros(Ba, 1, 32, 32, dtype=torch.bool, device=dev)
            box[torch.from_numpy(paste).to(dev), :, 8:24, 8:24] = True
            blend = torch.from_numpy(~paste).to(dev).view(Ba, 1, 1, 1)
            st = torch.cuda.current_stream().cuda_stream

            def plain():
                L.check(L.lib().gs_image_augment(L.GS_DEV_HIP, 0, ds.images.data_ptr(), ds.labels.data_ptr(), ds.n, 32,
                                                 32, 3, 4, 32, 32, dprm.data_ptr(), Ba, xa.data_ptr(), L.GS_F32,
                                                 L.GS_LAYOUT_NCHW, la.data_ptr(), st))

            def fused():
                L.check(L.lib().gs_image_augment_mix(L.GS_DEV_HIP, 0, ds.images.data_ptr(), ds.labels.data_ptr(), ds.n,
                                                     32, 32, 3, 4, 32, 32, dprm.data_ptr(), drec.data_ptr(), Ba,
                                                     xa.data_ptr(), L.GS_F32, L.GS_LAYOUT_NCHW, la.data_ptr(),
                                                     lb_.data_ptr(), lm.data_ptr(), st))

            def composed():
                plain()
                xb = xa[perm]
                return torch.where(box, xb, torch.where(blend, xa * lam_t + xb * (1 - lam_t), xa)), la[perm]

            p_ms, c_ms = timeit(plain, args.iters), timeit(composed, args.iters)
            p_batched, c_batched = timeit_batched(plain, args.iters), timeit_batched(composed, args.iters)
            f_ms = timeit(fused, args.iters)
            rec("augment_mix", Ba * (2 * 3072 + 4 * 3072), *f_ms, "libgsync", B=Ba, geometry="32x32x3 pad 4 crop 32",
                out="f32 nchw", augment_median_ms=p_ms[0], augment_avg_ms=p_ms[1], augment_batched_avg_ms=p_batched,
                augment_plus_torch_median_ms=c_ms[0], augment_plus_torch_avg_ms=c_ms[1],
                augment_plus_torch_batched_avg_ms=c_batched, ratio_to_augment=f_ms[0] / p_ms[0],
                ratio_to_augment_plus_torch=f_ms[0] / c_ms[0])
        del ds
    # the resize-based input step (gs_image_resample: RandomResizedCrop + flip + ToTensor + Normalize + bf16 NHWC in one
    # launch) at B = 256, beside the torch composition on the same records (per-sample slice + F.interpolate + flip into
    # an fp32 batch, then one normalise + cast) and a plain device copy that moves the same number of bytes
    if want("resample"):
        import ctypes

        import numpy as np

        from distributed_training_amd import data as D

        Br = 256
        st = torch.cuda.current_stream().cuda_stream
        for (Hs, n_img, osz) in ((256, 1024, 224), (64, 8192, 56)):
            ds = D.ImageDataset.synthetic(n_img, H=Hs, W=Hs, device=dev, seed=0)
            tf = D.RandomResizedCropFlip(osz, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), seed=0, rank=0)
            recs = tf.records(np.random.default_rng(Hs).integers(0, n_img, Br), Hs, Hs)
            drec = torch.from_numpy(recs).to(dev)
            box = [(int(r[0]), int(r[1]), int(r[2]) & 0xFFFF, (int(r[2]) >> 16) & 0xFFFF, int(r[3]) & 0xFFFF,
                    (int(r[3]) >> 16) & 0xFFFF) for r in recs]
            xr = torch.empty((Br, 3, osz, osz), dtype=torch.bfloat16, device=dev, memory_format=torch.channels_last)
            lr_ = torch.empty(Br, dtype=torch.int64, device=dev)
            c_mean, c_std = (ctypes.c_float * 3)(*tf.mean), (ctypes.c_float * 3)(*tf.std)
            t_mean = torch.tensor(tf.mean, device=dev).view(1, 3, 1, 1) * 255
            t_std = torch.tensor(tf.std, device=dev).view(1, 3, 1, 1) * 255
            tmp = torch.empty((Br, 3, osz, osz), device=dev)
            alg = sum(b[4] * b[5] * 3 for b in box) + Br * 3 * osz * osz * 2
            ca, cb = (torch.empty(alg // 2, dtype=torch.uint8, device=dev) for _ in range(2))

            def fused():
                L.check(L.lib().gs_image_resample(L.GS_DEV_HIP, 0, ds.images.data_ptr(), ds.labels.data_ptr(), ds.n, Hs, Hs,
                                                  3, osz, osz, osz, osz, 0, 0, drec.data_ptr(), Br, c_mean, c_std,
                                                  xr.data_ptr(), L.GS_BF16, L.GS_LAYOUT_NHWC, lr_.data_ptr(), st))

            def composed():
                for i, (idx, flip, top, left, h, w) in enumerate(box):
                    o = torch.nn.functional.interpolate(
                        ds.images[idx, top:top + h, left:left + w].permute(2, 0, 1)[None].float(), size=(osz, osz),
                        mode="bilinear", align_corners=False, antialias=False)
                    tmp[i] = o[0].flip(-1) if flip else o[0]
                return ((tmp - t_mean) / t_std).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

            c_ms = timeit(composed, 5, warmup=1)
            k_ms = timeit(lambda: cb.copy_(ca), 50)
            f_ms = timeit(fused, 50)  # HIP events around each launch, the median of 50; timed last: rec() batches it
            rec("resample", alg, *f_ms, "libgsync", B=Br, geometry=f"{Hs}x{Hs}x3 -> {osz}x{osz}", out="bf16 nhwc normalised",
                copy_median_ms=k_ms[0], copy_avg_ms=k_ms[1], copy_GBps=alg / (k_ms[0] * 1e-3) / 1e9,
                median_GBps=alg / (f_ms[0] * 1e-3) / 1e9, frac_of_copy=k_ms[0] / f_ms[0],
                torch_median_ms=c_ms[0], torch_avg_ms=c_ms[1], ratio_to_torch=f_ms[0] / c_ms[0])
            del ds, ca, cb, tmp
    if not args.skip_torch and want("lamb"):
        # a LAMB step of the same arithmetic as torch foreach ops, everything on the device
        bp, bm, bv = [p.clone() for p in params], [x.clone() for x in ms], [x.clone() for x in vs]
        b_adapt = torch.tensor([len(s) > 1 for s in shapes], device=dev)
        b_wds = (b_adapt * 0.01).unbind()

        def t_lamb():
            torch._foreach_lerp_(bm, grads, 0.1)
            torch._foreach_mul_(bv, 0.999)
            torch._foreach_addcmul_(bv, grads, grads, value=0.001)
            den = torch._foreach_sqrt(bv)
            torch._foreach_div_(den, 0.0316)
            torch._foreach_add_(den, 1e-6)
            u = torch._foreach_div(bm, 0.1)
            torch._foreach_div_(u, den)
            torch._foreach_add_(u, torch._foreach_mul(bp, b_wds))
            wn, un = torch.stack(torch._foreach_norm(bp)), torch.stack(torch._foreach_norm(u))
            ratio = torch.where(b_adapt & (wn > 0) & (un > 0), wn / un, 1.0)
            torch._foreach_add_(bp, torch._foreach_mul(u, (ratio * -1e-6).unbind()))

        rec("lamb_step", 40 * n, *timeit(t_lamb, args.iters), "torch foreach composition")
    if not args.skip_torch and (not only or want("pack", "unpack_f32", "sqnorm", "lars", "sgd", "adam")):
        inv = 1.0 / 8

        def t_pack():
            for gr, v in zip(grads, views):
                torch.mul(gr, inv, out=v)

        def t_pack16():
            for gr, v in zip(grads, views16):
                v.copy_(gr.mul(inv))

        def t_unpack():
            for gr, v in zip(grads, views):
                gr.copy_(v)

        rec("pack_f32", 8 * n, *timeit(t_pack, args.iters), "torch per-param (Reducer)")
        rec("pack_f32_to_bf16", 6 * n, *timeit(t_pack16, args.iters), "torch per-param (Reducer)")
        rec("unpack_f32", 8 * n, *timeit(t_unpack, args.iters), "torch per-param (Reducer)")
        rec("sqnorm_f32", 4 * n, *timeit(lambda: torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads))),
                                         args.iters), "torch _foreach_norm")
        # a LARS step as torch foreach ops, everything on the device (no host sync)
        lp, lb = [p.clone() for p in params], [b.clone() for b in bufs]
        l_adapt = torch.tensor([len(s) > 1 for s in shapes], device=dev)

        def t_lars_norms():
            return torch._foreach_norm(lp), torch._foreach_norm(grads)

        def t_lars():
            wn, gn = (torch.stack(x) for x in t_lars_norms())
            ratio = torch.where(l_adapt & (wn > 0) & (gn > 0), 1e-3 * wn / (gn + 1e-4 * wn + 1e-8), 1.0)
            wds = (l_adapt * 1e-4).unbind()
            g2 = torch._foreach_add(grads, torch._foreach_mul(lp, wds))
            torch._foreach_mul_(lb, 0.9)
            torch._foreach_add_(lb, g2)
            torch._foreach_add_(lp, torch._foreach_mul(lb, (ratio * -1e-6).unbind()))

        rec("lars_norms", 8 * n, *timeit(t_lars_norms, args.iters), "torch _foreach_norm x2")
        rec("lars_step", 28 * n, *timeit(t_lars, args.iters), "torch foreach composition")
        ps = [torch.nn.Parameter(p.clone()) for p in params]
        for p, gr in zip(ps, grads):
            p.grad = gr
        sgd = torch.optim.SGD(ps, lr=1e-6, momentum=0.9, weight_decay=1e-4, foreach=True)
        rec("sgd_momentum_wd", 20 * n, *timeit(sgd.step, args.iters), "torch.optim.SGD foreach")
        adam = torch.optim.Adam(ps, lr=1e-6, foreach=True)
        rec("adam", 28 * n, *timeit(adam.step, args.iters), "torch.optim.Adam foreach")
        fadam = torch.optim.Adam(ps, lr=1e-6, fused=True)
        rec("adam", 28 * n, *timeit(fadam.step, args.iters), "torch.optim.Adam fused")


if __name__ == "__main__":
    main()
