"""The BatchNorm backward entries alone, at every (R, C) ResNet-50 x 256 launches them with.

    python scripts/bench_bn_bwd.py --libs PATH_A,PATH_B --rounds 3 --out FILE.jsonl
    GSYNC_LIB=.../libgsync_NAME.so python scripts/bench_bn_bwd.py          # one library, one JSON line

3 warm-up and 20 timed launches per (entry, shape) between device events.  Beside each row: gs_add_relu_fwd
on the same element count (two reads and one write of R * C bf16, on a flat grid: what a kernel without a
channel tile reaches there; the mask-reading entries move 2.125 streams, the fork 4.125).  ``launches`` is
the entry's launches per training step at that shape, ``step_ms`` the launch-weighted sum.

With ``--libs`` the libraries alternate, ``--rounds`` times, each run in a fresh child process under its
own time limit (``--limit`` seconds); the first child that fails or runs out of time ends the script.
Library variants: ``make -C distributed_training_amd/csrc variant NAME=tile8 DEFS=-DGS_BN_TILE_VECS=8``
(DESIGN §3e has the protocol and the results)."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N = 256
S112, S56, S28, S14, S7 = (N * s * s for s in (112, 56, 28, 14, 7))
# BatchNorm + ReLU inside the blocks and the stem: reduce and dx from the mask bits, no g
PLAIN = [(S112, 64, 1), (S56, 64, 6), (S56, 128, 1), (S28, 128, 7), (S28, 256, 1), (S14, 256, 11), (S14, 512, 1),
         (S7, 512, 5)]
# block outputs: (R, C, blocks whose output forks, blocks)
BLOCKS = [(S56, 256, 3, 3), (S28, 512, 4, 4), (S14, 1024, 6, 6), (S7, 2048, 2, 3)]


def cases():
    """(entry, R, C, launches per step)"""
    out = [("reduce_bits", R, C, n) for R, C, n in PLAIN] + [("dx_bits", R, C, n) for R, C, n in PLAIN]
    for R, C, forks, blocks in BLOCKS:
        out.append(("reduce_fork_bits", R, C, forks))
        if blocks > forks:
            out.append(("reduce_bits_g", R, C, blocks - forks))
        out.append(("reduce_plain", R, C, 1))    # the downsample BatchNorm, fed g
        out.append(("dx_g", R, C, blocks + 1))   # the block's last BatchNorm and the downsample's
    return out


def one(warmup, iters):
    import torch

    sys.path.insert(0, REPO)
    from distributed_training_amd import _lib as L

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib, s = L.lib(), L.stream_ptr(dev)

    def timed(fn):
        for _ in range(warmup):
            fn()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / iters * 1e3  # microseconds

    rows, bufs, flat = [], {}, {}
    for entry, R, C, launches in sorted(cases(), key=lambda c: (-c[1] * c[2], c[2])):  # shape by shape
        if (R, C) not in bufs:
            bufs.clear()  # one shape's buffers at a time
            g = torch.Generator(device=dev).manual_seed(R + C)
            t = {k: torch.randn(R, C, device=dev, generator=g).to(torch.bfloat16) for k in ("x", "dy", "dy_b")}
            t["out"] = torch.empty_like(t["x"])
            t["mask"] = torch.randint(0, 256, (R * C // 8,), device=dev, generator=g, dtype=torch.uint8)
            t["mean"], t["invstd"] = torch.randn(C, device=dev), torch.rand(C, device=dev) + 0.5
            t["weight"], t["gw"], t["gb"] = torch.rand(C, device=dev) + 0.5, torch.empty(C, device=dev), torch.empty(
                C, device=dev)
            P = L.check(lib.gs_bn_bwd_partials(R, C), "gs_bn_bwd_partials")
            t["ws"] = torch.zeros(P * C * 2, device=dev)
            bufs[(R, C)] = t
            a, b = torch.randn(R * C, device=dev).to(torch.bfloat16), torch.randn(R * C, device=dev).to(torch.bfloat16)
            flat[(R, C)] = timed(lambda: L.check(lib.gs_add_relu_fwd(a.data_ptr(), b.data_ptr(), R * C, s)))
            del a, b
        t = bufs[(R, C)]
        p = {k: v.data_ptr() for k, v in t.items()}
        n = t["ws"].numel()
        fn = {
            "reduce_bits": lambda: lib.gs_bn_bwd_reduce_bits(p["x"], p["dy"], p["mask"], None, p["mean"], p["ws"], n,
                                                             R, C, s),
            "reduce_bits_g": lambda: lib.gs_bn_bwd_reduce_bits(p["x"], p["dy"], p["mask"], p["out"], p["mean"],
                                                               p["ws"], n, R, C, s),
            "reduce_fork_bits": lambda: lib.gs_bn_bwd_reduce_fork_bits(p["x"], p["dy"], p["dy_b"], p["mask"],
                                                                       p["out"], p["mean"], p["ws"], n, R, C, s),
            "reduce_plain": lambda: lib.gs_bn_bwd_reduce(p["x"], p["dy"], None, None, p["mean"], p["ws"], n, R, C, s),
            "dx_bits": lambda: lib.gs_bn_bwd_dx_bits(p["x"], p["dy"], p["mask"], p["mean"], p["invstd"], p["weight"],
                                                     p["ws"], n, p["out"], p["gw"], p["gb"], R, C, s),
            "dx_g": lambda: lib.gs_bn_bwd_dx(p["x"], p["dy"], None, p["mean"], p["invstd"], p["weight"], p["ws"], n,
                                             p["out"], p["gw"], p["gb"], R, C, s),
        }[entry]
        us = timed(lambda: L.check(fn(), entry))
        rows.append({"entry": entry, "R": R, "C": C, "launches": launches, "us": round(us, 2),
                     "add_relu_fwd_us": round(flat[(R, C)], 2)})
    step_ms = sum(r["us"] * r["launches"] for r in rows) / 1e3
    print(json.dumps({"bench": "bn_bwd_kernels", "lib": os.path.basename(L.LIB_PATH), "warmup": warmup, "iters": iters,
                      "step_ms": round(step_ms, 4), "rows": rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="", help="comma-separated library paths: alternate them in child processes")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=180.0, help="seconds per child process")
    ap.add_argument("--out", default="", help="append the children's JSON lines to this file")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not args.libs:
        one(args.warmup, args.iters)
        return 0
    for rnd in range(args.rounds):
        for path in args.libs.split(","):
            env = dict(os.environ, GSYNC_LIB=os.path.abspath(path))
            cmd = [sys.executable, os.path.abspath(__file__), "--warmup", str(args.warmup), "--iters", str(args.iters)]
            try:
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print(f"round {rnd} {path}: no result within {args.limit} s; stopping", file=sys.stderr)
                return 1
            if r.returncode != 0:
                print(f"round {rnd} {path}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                return 1
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            rec = dict(json.loads(line), round=rnd)
            print(json.dumps({k: rec[k] for k in ("lib", "round", "step_ms")}), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
