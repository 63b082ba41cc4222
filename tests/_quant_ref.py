"""The quantization hook tests' planted input, torch's own fp32 functions as the reference, and the hook harness."""
import functools

import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch.ao.quantization import MinMaxObserver, PerChannelMinMaxObserver
from torch.distributed.algorithms.ddp_comm_hooks import quantization_hooks as TQ

from distributed_training_amd.multi_tensor import QuantPlan
from tests._dist_util import free_port, init_pg

NS = [1, 3, 511, 512, 513, 4 * 512 + 5, 70001]


@functools.lru_cache(maxsize=None)
def planted(n, bs, seed=0):
    """seeded randn, the channels' scales spread over six decades; channels 1..6 (those that exist): zeros,
    positive, negative, constant, a range below 255 eps, and min 0 / max 255 / values k + 0.5 (scale exactly 1)"""
    g, C, eps = torch.Generator().manual_seed(seed + n), -(-n // bs), torch.finfo(torch.float32).eps
    x = (torch.randn(C, bs, generator=g) * 10.0 ** (torch.rand(C, 1, generator=g) * 6 - 4))
    half = torch.cat([torch.tensor([0.0, 255.0]), torch.arange(2, bs) % 255 + 0.5])
    plants = [torch.zeros(bs), x[0].abs() + 1, -x[0].abs() - 1, torch.full((bs,), 0.37),
              torch.rand(bs, generator=g) * 100 * eps - 50 * eps, half]
    for c, p in enumerate(plants[:C - 1]):
        x[c + 1] = p
    return x.flatten()[:n].clone()


def ref_quant(x, bs):
    """(bytes [n], scales [C], zero points [C] as float) by torch's observers and quantize; bs 0: per tensor"""
    t = torch.nn.functional.pad(x, (0, -x.numel() % bs)).view(-1, bs) if bs else x
    obs = PerChannelMinMaxObserver() if bs else MinMaxObserver()
    obs(t)
    s, z = obs.calculate_qparams()
    if bs:
        return TQ._quantize_per_channel_backend(t, s, z.float()).flatten()[:x.numel()], s, z.float()
    sz = torch.FloatTensor([s, z])  # as torch's hook ships them
    return TQ._quantize_per_tensor_backend(x, sz[0], sz[1]), sz[:1], sz[1:]


def ref_mean(parts, n, bs):  # torch's dequantize loop over the ranks' (bytes, scales, zps) in rank order, then / ws
    agg = torch.zeros(n)
    for q, s, z in parts:
        agg += TQ._dequantize_per_tensor_backend(q, s[0], z[0]) if not bs else TQ._dequantize_per_channel_backend(
            torch.nn.functional.pad(q, (0, -n % bs)).view(-1, bs), s, z).flatten()[:n]
    return agg / len(parts)


def _geometry(n, bs):  # channels, bytes of quantized values
    C = -(-n // bs) if bs else 1
    return C, -(-(C * bs if bs else n) // 16) * 16


def split(payload, n, bs):
    (C, Q), p = _geometry(n, bs), payload.cpu()
    return p[:n], p[Q:Q + 4 * C].view(torch.float32), p[Q + 4 * C:Q + 8 * C].view(torch.int32).float()


def join(q, s, z, n, bs):
    body = torch.zeros(_geometry(n, bs)[1], dtype=torch.uint8)
    body[:n] = q
    return torch.cat([body, s.float().view(torch.uint8), z.to(torch.int32).view(torch.uint8)])


def quantize(dev, x, bs):
    plan = QuantPlan(dev)
    payload = torch.zeros(plan.payload_bytes(x.numel(), bs), dtype=torch.uint8, device=dev)
    plan.quant_perchannel(x, payload, bs) if bs else plan.quant_pertensor(x, payload)
    return plan, payload


def check_quant(dev, n, bs, misaligned=False):  # misaligned: the bucket is base[1:], 4-byte aligned only
    x = planted(n, bs or 512)
    xd = torch.cat([x.new_zeros(1), x]).to(dev)[1:] if misaligned else x.to(dev)
    got, want = split(quantize(dev, xd, bs)[1], n, bs), ref_quant(x, bs)
    for name, a, b in zip(("bytes", "scales", "zero points"), got, want):
        assert torch.equal(a, b), (name, n, bs, (a != b).nonzero()[:4].flatten().tolist())


def check_dequant_mean(dev, ws, n=4 * 512 + 5):
    g = torch.Generator().manual_seed(ws)
    for bs in (0, 16, 512, 272):  # 272: a wave's 256 elements straddle channels
        C = _geometry(n, bs)[0]
        parts = [(torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8),
                  torch.rand(C, generator=g) * 10.0 ** torch.randint(-6, 3, (C,), generator=g),
                  torch.randint(0, 256, (C,), generator=g).float()) for _ in range(ws)]
        gathered = torch.cat([join(*p, n, bs) for p in parts]).to(dev)
        o = int(ws == 3)  # one case writes a bucket that is only 4-byte aligned
        out = torch.full((n + 2,), 7.0, device=dev)
        QuantPlan(dev).dequant_mean(gathered, ws, out[o:o + n], bs)
        assert torch.equal(out[o:o + n].cpu(), ref_mean(parts, n, bs)) and out[o + n] == out[0 if o else -1] == 7.0, \
            (ws, bs)  # and nothing is stored outside the bucket


def check_nonfinite(dev, n=8 * 512 + 5, bs=512):  # NaN: exactly the inf's and the NaN's channel; per tensor: all
    clean, x = planted(n, bs), planted(n, bs).clone()
    x[2 * bs + 7], x[5 * bs + 300] = float("inf"), float("nan")
    bad = torch.zeros(n, dtype=torch.bool)
    bad[2 * bs:3 * bs] = bad[5 * bs:6 * bs] = True
    for b in (bs, 0):
        plan, payload = quantize(dev, x.to(dev), b)
        out = torch.empty(n, device=dev)
        plan.dequant_mean(payload, 1, out, b)
        out = out.cpu()
        assert out[bad].isnan().all() and (torch.equal(out[~bad], ref_mean([ref_quant(clean, b)], n, b)[~bad]) if b
                                           else out.isnan().all())


def run_hooks(rank, ws, dev, steps=2):
    """micro_resnet under DDP, each hook: every rank's grads against the reference from all ranks' raw buckets"""
    import distributed_training_amd as D
    from distributed_training_amd.resnet import micro_resnet

    for hook, bs in ((D.quantization_pertensor_hook, 0), (D.quantization_perchannel_hook, 512),
                     (functools.partial(D.quantization_perchannel_hook, bucket_size=128), 128)):
        torch.manual_seed(0)
        ddp = D.DistributedDataParallel(micro_resnet().to(dev))
        seen = []

        def wrapped(pg, bucket, hook=hook):
            seen.append((bucket.buffer().cpu(), bucket))
            return hook(pg, bucket)

        ddp.register_comm_hook(None, wrapped)
        g = torch.Generator(device=dev).manual_seed(50 + rank)
        for it in range(steps):
            seen.clear()
            x = torch.rand(6, 3, 32, 32, device=dev, generator=g)
            y = torch.randint(0, 10, (6,), device=dev, generator=g)
            torch.nn.functional.cross_entropy(ddp(x), y).backward()
            assert seen
            for raw, bucket in seen:
                raws = [torch.empty_like(raw) for _ in range(ws)] if ws > 1 else [raw]
                if ws > 1:
                    dist.all_gather(raws, raw)
                want = ref_mean([ref_quant(r, bs) for r in raws], raw.numel(), bs)
                for p, gv in zip(bucket.parameters(), bucket.gradients()):
                    off = (gv.data_ptr() - bucket.buffer().data_ptr()) // 4
                    assert torch.equal(p.grad.cpu(), want.as_strided(p.size(), p.stride(), off)), (it, bs)
            ddp.zero_grad(set_to_none=True)
        ddp.close()


def _child(rank, ws, port, body, dev):
    init_pg("gloo", rank, ws, port)
    body(rank, ws, dev)
    dist.barrier()
    dist.destroy_process_group()


def spawn_ws2(body, dev):
    mp.spawn(_child, args=(2, free_port(), body, dev), nprocs=2)
