"""How many 1 Ki-element chunks of the sharded LAMB / LARS piece plan take the update
engine's unaligned path (a stream that does not start on a 16-byte boundary), counted on
the CPU from ZeroDataParallel's own layout: gloo ranks with host plans, no GPU.

    python scripts/zero_piece_alignment.py [--model resnet50] [--ws 1,2,8] [--out file.jsonl]

Per world size: the pieces of every rank, the chunks they cover, and the chunks of pieces
whose master (fp32) or model-copy (bf16) stream starts off a 16-byte boundary.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def worker(rank, ws, port, model, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    from distributed_training_amd.resnet import MODELS
    from distributed_training_amd.zero import ZeroDataParallel

    torch.manual_seed(0)
    z = ZeroDataParallel(MODELS[model](num_classes=1000).to(torch.bfloat16), stage=2, optimizer="lamb",
                         reduce_bucket_size=int(5e7), broadcast_params=False)
    if rank == 0:
        pieces = chunks = off_chunks = empty = split = 0
        held = [0] * len(z.params)
        for r in range(ws):
            for i, (b, off, n) in enumerate(z.shard_pieces(r)):
                if n == 0:
                    empty += 1
                    continue
                pieces += 1
                held[i] += 1
                c = (n + 1023) // 1024
                chunks += c
                # shard buffers are allocations of their own (256-byte aligned): a stream is
                # 16-byte aligned iff its element offset is a multiple of 4 (fp32) / 8 (bf16)
                if off % 8:
                    off_chunks += c
        row = {"model": model, "ws": ws, "tensors": len(z.params), "buckets": len(z.buckets), "pieces": pieces,
               "empty_entries": empty, "tensors_split_over_ranks": sum(h > 1 for h in held), "chunks": chunks,
               "chunks_on_the_unaligned_path": off_chunks,
               "share": off_chunks / max(1, chunks)}
        print(json.dumps(row), flush=True)
        if out:
            with open(out, "a") as f:
                f.write(json.dumps(row) + "\n")
    z.close()
    dist.barrier()
    dist.destroy_process_group()


def free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--ws", default="1,2,8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for ws in (int(x) for x in args.ws.split(",")):
        mp.spawn(worker, args=(ws, free_port(), args.model, args.out), nprocs=ws)


if __name__ == "__main__":
    main()
