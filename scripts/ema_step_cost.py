"""Per-step cost of ``AveragedModel.update_parameters`` on ResNet-50: torch.optim.swa_utils
against the fused drop-in (distributed_training_amd/ema.py), same ``multi_avg_fn``.

Each variant is timed as wall time of ``--iters`` back-to-back updates ending in a device
synchronise (what a training loop pays per step: host work and launches included), after
``--warmup`` updates.  The variants alternate, ``--rounds`` times, so drift on a shared host
shows up as spread between a variant's own rounds, not as a difference between variants:

  torch_cpu_counter   torch, device=None: its n_averaged stays on the CPU (an H2D copy per call)
  torch_dev_counter   torch, device=cuda: n_averaged on the device (two host reads per call)
  fused               ours, eager
  fused_graph         ours inside CapturedStep (one hipGraph replay per update)

for use_buffers False and True, EMA 0.999.  Launches per update are counted with the torch
profiler where it is available (null otherwise).  One JSON record per (variant, use_buffers)
goes to ``--out`` (default profiles/ema/step_cost.jsonl).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def count_launches(fn):
    """device-side events (kernels, copies, memsets) of one update, by the torch profiler"""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA) or None
    except Exception:  # the profiler is optional here
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--out", default=os.path.join("profiles", "ema", "step_cost.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_step_cost.py measures on the GPU: no HIP device")
    import torch.optim.swa_utils as S

    import distributed_training_amd as D
    from distributed_training_amd.resnet import MODELS

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = MODELS[args.model]().to(dev)
    n_params = sum(p.numel() for p in model.parameters())
    n_bufs = len(list(model.buffers()))
    rows = []
    for use_buffers in (False, True):
        variants = {}
        t_cpu = S.AveragedModel(model, multi_avg_fn=S.get_ema_multi_avg_fn(args.decay), use_buffers=use_buffers)
        variants["torch_cpu_counter"] = lambda m=t_cpu: m.update_parameters(model)
        t_dev = S.AveragedModel(model, device=dev, multi_avg_fn=S.get_ema_multi_avg_fn(args.decay),
                                use_buffers=use_buffers)
        variants["torch_dev_counter"] = lambda m=t_dev: m.update_parameters(model)
        fused = D.AveragedModel(model, multi_avg_fn=D.get_ema_multi_avg_fn(args.decay), use_buffers=use_buffers)
        variants["fused"] = lambda m=fused: m.update_parameters(model)
        graphed = D.AveragedModel(model, multi_avg_fn=D.get_ema_multi_avg_fn(args.decay), use_buffers=use_buffers)
        step = D.CapturedStep(lambda m=graphed: m.update_parameters(model))
        variants["fused_graph"] = step
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        assert fused.last_path == "fused" and graphed.last_path == "fused" and step.replays > 0
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.iters * 1e6)
        for name, ts in times.items():
            rows.append({"script": "ema_step_cost", "model": args.model, "params": n_params, "buffers": n_bufs,
                         "variant": name, "use_buffers": use_buffers, "decay": args.decay, "iters": args.iters,
                         "rounds": args.rounds, "us_per_update_median": statistics.median(ts),
                         "us_per_update_min": min(ts), "us_per_update_max": max(ts),
                         "launches_per_update": None if name == "fused_graph" else count_launches(variants[name])})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
