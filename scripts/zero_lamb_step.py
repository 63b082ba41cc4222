"""ZeroDataParallel.step() on ResNet-50's parameters, bf16 model, stage 2, ws = 1 over RCCL:
optimizer="adamw" (unchanged by the sharded LAMB work: the baseline) against "lamb", in one
process, with and without gradient_clipping.  5 warm-up + 20 timed steps each; a step is
timed by a HIP event pair on the step's stream (device time of everything step() enqueues:
kernels, the small all-reduces, the parameter all-gather) and by the host clock around the
call (what step() costs the Python thread).  Grads come from the synthetic loss
Σ <p_i, r_i> through the real hooks, as tests/test_zero_ds_step.py drives the engine.

    python scripts/zero_lamb_step.py [--out profiles/zero_lamb/step_resnet50.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(free_port()))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    from distributed_training_amd.resnet import MODELS
    from distributed_training_amd.zero import ZeroDataParallel

    out = open(args.out, "a") if args.out else None
    for clip in (1.0, 0.0):
        for kind in ("adamw", "lamb", "adamw", "lamb"):  # each twice: the second pass shows the run's spread
            torch.manual_seed(0)
            model = MODELS[args.model](num_classes=1000).to(dev).to(torch.bfloat16)
            params = list(model.parameters())
            z = ZeroDataParallel(model, stage=2, optimizer=kind, lr=1e-3, betas=(0.9, 0.999), eps=1e-6,
                                 weight_decay=0.01, reduce_bucket_size=int(5e7), gradient_clipping=clip)
            assert z._comm is not None, "the library's RCCL communicator is not in use"
            rs = [torch.randn(p.shape, device=dev) * 1e-3 for p in params]
            dev_ms, host_ms = [], []
            for it in range(args.warmup + args.steps):
                z.prepare_backward()
                sum((p.float() * r).sum() for p, r in zip(params, rs)).backward()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                z.step()
                b.record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    dev_ms.append(a.elapsed_time(b))
                    host_ms.append((t1 - t0) * 1e3)
            row = {"model": args.model, "dtype": "bf16", "stage": 2, "ws": 1, "optimizer": kind,
                   "gradient_clipping": clip, "steps": args.steps, "params": sum(p.numel() for p in params),
                   "buckets": len(z.buckets), "step_device_ms_median": statistics.median(dev_ms),
                   "step_device_ms_min": min(dev_ms), "step_device_ms_max": max(dev_ms),
                   "step_host_ms_median": statistics.median(host_ms)}
            print(json.dumps(row), flush=True)
            if out:
                out.write(json.dumps(row) + "\n")
                out.flush()
            z.close()
            del z, model, params, rs
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
