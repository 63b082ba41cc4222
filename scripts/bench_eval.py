"""The evaluation forward: ResNet-50 x 256, bf16 autocast, channels_last, eval mode, plus Metrics.update.

    python scripts/bench_eval.py --fused 0|1 [--kernels 1]
    GSYNC_LIB=.../libgsync_NAME.so python scripts/bench_eval.py --kernels 2     # the kernel rates alone

5 warm-up and 20 timed iterations between device events; one JSON line.  ``--fused 1`` runs the forward
inside ``fused_bn.fused_eval()`` (gs_bn_infer_act / gs_bn_infer_relu_maxpool), ``--fused 0`` the stock
modules.  ``--kernels 1`` also times gs_bn_infer_act (residual + ReLU: two reads, one write) next to
gs_add_relu_fwd (the same traffic) at the ResNet-50 block shapes, against the 6.29 TB/s copy ceiling.
Run each setting in a fresh process (DESIGN §3c has the protocol)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_training_amd import Metrics, fused_bn  # noqa: E402
from distributed_training_amd import _lib as L  # noqa: E402
from distributed_training_amd.resnet import MODELS  # noqa: E402

COPY_CEILING_TBS = 6.29
BLOCK_SHAPES = [(256 * 56 * 56, 256), (256 * 28 * 28, 512), (256 * 14 * 14, 1024), (256 * 7 * 7, 2048)]


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def kernel_rates(dev, warmup, iters):
    lib, rows = L.lib(), []
    for R, C in BLOCK_SHAPES:
        x = torch.randn(R, C, device=dev).to(torch.bfloat16)
        r = torch.randn(R, C, device=dev).to(torch.bfloat16)
        y = torch.empty_like(x)
        mean, var = torch.randn(C, device=dev), torch.rand(C, device=dev) + 0.5
        w, b = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
        s = L.stream_ptr(dev)
        t_bn = timed(lambda: L.check(lib.gs_bn_infer_act(x.data_ptr(), r.data_ptr(), mean.data_ptr(), var.data_ptr(),
                                                         w.data_ptr(), b.data_ptr(), 1e-5, 1, y.data_ptr(), R, C, s)),
                     warmup, iters)
        # in place (y = x), as gs_add_relu_fwd works: two buffers instead of three
        t_ip = timed(lambda: L.check(lib.gs_bn_infer_act(y.data_ptr(), r.data_ptr(), mean.data_ptr(), var.data_ptr(),
                                                         w.data_ptr(), b.data_ptr(), 1e-5, 1, y.data_ptr(), R, C, s)),
                     warmup, iters)
        t_ar = timed(lambda: L.check(lib.gs_add_relu_fwd(y.data_ptr(), r.data_ptr(), R * C, s)), warmup, iters)
        tb = 3 * R * C * 2 / 1e12
        rows.append({"R": R, "C": C, "bn_infer_act_us": round(t_bn * 1e3, 2), "add_relu_fwd_us": round(t_ar * 1e3, 2),
                     "bn_infer_act_inplace_us": round(t_ip * 1e3, 2),
                     "bn_infer_act_inplace_of_ceiling": round(tb / (t_ip * 1e-3) / COPY_CEILING_TBS, 3),
                     "bn_infer_act_tbs": round(tb / (t_bn * 1e-3), 3), "add_relu_fwd_tbs": round(tb / (t_ar * 1e-3), 3),
                     "bn_infer_act_of_ceiling": round(tb / (t_bn * 1e-3) / COPY_CEILING_TBS, 3),
                     "add_relu_fwd_of_ceiling": round(tb / (t_ar * 1e-3) / COPY_CEILING_TBS, 3)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fused", type=int, default=1)
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernels", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.kernels == 2:  # the kernel rates alone (GSYNC_LIB selects a library variant)
        print(json.dumps({"bench": "eval_kernels", "lib": os.path.basename(L.LIB_PATH),
                          "kernels": kernel_rates(dev, args.warmup, args.iters)}))
        return
    torch.manual_seed(0)
    model = MODELS[args.model](num_classes=1000).to(dev).to(memory_format=torch.channels_last).eval()
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(args.batch, 3, 224, 224, device=dev, generator=g).to(memory_format=torch.channels_last)
    x = x.to(torch.bfloat16)
    y = torch.randint(0, 1000, (args.batch,), device=dev, generator=g)
    metrics = Metrics(topk=(1, 5), device=dev)

    def step():
        metrics.update(model(x), y)

    with torch.no_grad(), fused_bn.fused_eval(bool(args.fused)), torch.autocast("cuda", dtype=torch.bfloat16):
        ms = timed(step, args.warmup, args.iters)
        path = fused_bn.last_path
    out = metrics.compute()
    res = {"bench": "eval_forward", "model": args.model, "batch": args.batch, "fused": args.fused, "bn_path": path,
           "warmup": args.warmup, "iters": args.iters, "ms_per_iter": round(ms, 4),
           "images_per_s": round(args.batch / ms * 1e3, 1), "n": out["n"], "loss": round(out["loss"], 5)}
    if args.kernels:
        res["kernels"] = kernel_rates(dev, args.warmup, args.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
