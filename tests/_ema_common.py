"""Shared pieces of the weight-averaging tests (tests/test_ema_cpu.py, tests/test_gpu_ema.py).

The yardstick is torch itself: ``torch.lerp`` / ``torch.optim.swa_utils.AveragedModel`` on
the CPU (the contract of gs_ema_step is that kernel's arithmetic, for both backends)."""
import torch

# 0-element tensors, tails on both sides of the 1 Ki chunk and of the 4 Ki group alignment,
# 5 full chunks (a last group shorter than the group size)
LIST_A = [0, 1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 5 * 4096]
# 200 tensors of 1-7 elements: a mixed chunk whose span exceeds 64 tensors
LIST_B = [1 + (i * 5) % 7 for i in range(200)]


def rand_lists(numels, seed, src_dtype=torch.float32):
    """(a, s): fp32 averages and sources of ``src_dtype`` on the CPU, a few decades of magnitude"""
    g = torch.Generator().manual_seed(seed)
    a = [torch.randn(n, generator=g) * 10 ** float(torch.randint(-3, 3, (1,), generator=g)) for n in numels]
    s = [(torch.randn(n, generator=g) * 10 ** float(torch.randint(-3, 3, (1,), generator=g))).to(src_dtype)
         for n in numels]
    return a, s


def lerp_ref(a, s, w, copy=False):
    """torch's CPU result for one update: the first update's copy_, else torch.lerp on fp32"""
    if copy:
        return [y.float().clone() for y in s]
    return [torch.lerp(x, y.float(), w) for x, y in zip(a, s)]


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(bits(x.cpu()), bits(y.cpu()))


def perturb(model, seed, scale=0.01):
    """a training step's worth of change in every parameter and buffer"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.add_((torch.randn(p.shape, generator=g) * scale).to(p.device, p.dtype))
        for b in model.buffers():
            if b.is_floating_point():
                b.add_((torch.rand(b.shape, generator=g) * scale).to(b.device, b.dtype))
            else:
                b.add_(3)
