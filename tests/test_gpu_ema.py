"""Fused EMA / SWA weight averaging on the GPU: EmaOp on the chunk-map engine, gs_ema_hyper,
the AveragedModel drop-in (no host synchronisation, graph capture) and the ZeRO-sharded average.

The contract of gs_ema_step is one arithmetic for both backends — torch.lerp's CPU kernel — so
every kernel result here must equal torch's CPU result bit for bit; torch's device kernel
(``torch._foreach_lerp_`` on the GPU) is compared as a second yardstick."""
import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn
import torch.optim.swa_utils as S

from tests._dist_util import free_port, init_pg
from tests._ema_common import LIST_A, LIST_B, bits, lerp_ref, perturb, rand_lists, same_bits

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
GUARD_BYTES, LINE = 4096, 128
PATTERN = {F32: (torch.int32, 0x7FC00001), BF16: (torch.int16, 0x7FC1), F16: (torch.int16, 0x7E01)}  # NaNs


class Guarded:
    """n elements inside a larger buffer: 4 KiB of a NaN pattern on each side, the view starting
    ``off`` elements past a 128-byte line"""

    def __init__(self, n, dtype, dev, off=0):
        itype, self.pat = PATTERN[dtype]
        size = torch.empty(0, dtype=dtype).element_size()
        g = GUARD_BYTES // size
        self.raw = torch.full((g + LINE // size + off + n + g,), self.pat, dtype=itype, device=dev)
        start = g
        while (self.raw.data_ptr() + start * size) % LINE:
            start += 1
        self.start, self.n = start + off, n
        self.view = self.raw.view(dtype)[self.start:self.start + n]

    def intact(self):
        return bool((self.raw[:self.start] == self.pat).all()) and bool((self.raw[self.start + self.n:] == self.pat).all())


def _run_lists(dev, numels, sd, ld, cases, seed, offs=(0, 0, 0)):
    """gs_ema_step on guarded device copies of random lists, for every (w, copy) of ``cases``:
    the average, the copy, the untouched source and the guards against torch on the CPU"""
    from distributed_training_amd.multi_tensor import TensorListPlan, update_task_units

    a0, s0 = rand_lists(numels, seed, sd)
    ga = [Guarded(n, F32, dev, offs[0]) for n in numels]
    gs = [Guarded(n, sd, dev, offs[1]) for n in numels]
    gl = [Guarded(n, ld, dev, offs[2]) for n in numels] if ld is not None else None
    plan = TensorListPlan(numels, dev, task_units=update_task_units(dev))
    plan.set_ptrs(0, [g.view for g in ga])
    plan.set_ptrs(1, [g.view for g in gs])
    if gl is not None:
        plan.set_ptrs(2, [g.view for g in gl])
    for g, t in zip(gs, s0):
        g.view.copy_(t)
    for w, copy in cases:
        for g, t in zip(ga, a0):
            g.view.copy_(t)
        if gl is not None:
            for g in gl:
                g.view.zero_()
        plan.ema(sd, w, copy=copy, lowp_dtype=ld)
        torch.cuda.synchronize()
        want = lerp_ref(a0, s0, w, copy)
        for i, n in enumerate(numels):
            assert same_bits(ga[i].view, want[i]), (sd, ld, w, copy, n)
            assert same_bits(gs[i].view, s0[i]), ("source", sd, ld, w, copy, n)
            if gl is not None:
                assert same_bits(gl[i].view, want[i].to(ld)), ("copy", sd, ld, w, copy, n)
        assert all(g.intact() for g in ga + gs + (gl or [])), (sd, ld, w, copy)
    plan.close()


CASES = [(1e-4, False), (0.5, False), (0.7, False), (1.0, False), (0.3, True)]


@pytest.mark.parametrize("ld", [None, BF16, F16], ids=["none", "bf16", "f16"])
@pytest.mark.parametrize("sd", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_kernel_list_a(cuda_device, sd, ld):
    _run_lists(cuda_device, LIST_A, sd, ld, CASES, seed=11)


@pytest.mark.parametrize("sd,ld", [(F32, None), (BF16, BF16)], ids=["f32-none", "bf16-bf16"])
def test_kernel_many_tiny_tensors(cuda_device, sd, ld):
    _run_lists(cuda_device, LIST_B, sd, ld, [(1e-4, False), (0.7, False), (0.3, True)], seed=12)


@pytest.mark.parametrize("numels", [[3 * 1024], [5 * 1024 + 1], [1024]], ids=["3Ki", "5Ki+1", "1Ki"])
def test_kernel_last_group_shorter_than_the_group_size(cuda_device, numels):
    """an odd number of chunks: the last workgroup iteration holds one chunk, aligned (the fast path)"""
    _run_lists(cuda_device, numels, F32, BF16, [(1e-4, False), (0.7, False), (0.3, True)], seed=14)


@pytest.mark.parametrize("slot", [0, 1, 2])
def test_kernel_checked_path_one_element_off_alignment(cuda_device, slot):
    offs = [0, 0, 0]
    offs[slot] = 1
    _run_lists(cuda_device, [4099], F32, BF16, [(1e-4, False), (0.7, False), (0.3, True)], seed=13, offs=tuple(offs))


@pytest.mark.parametrize("ld", [F16, BF16], ids=["f16", "bf16"])
def test_lowp_copy_rounds_the_stored_value(cuda_device, ld):
    """2^20 random elements (the size at which fp32 results land on fp16 ties): the copy is the
    cast of the STORED fp32 average, not a single rounding of the exact fma"""
    from distributed_training_amd.multi_tensor import TensorListPlan

    dev = cuda_device
    n = 1 << 20
    g = torch.Generator(device=dev).manual_seed(9)
    for w in (0.3, 0.7):
        a = torch.randn(n, device=dev, generator=g)
        s = torch.randn(n, device=dev, generator=g)
        a_cpu, s_cpu = a.cpu(), s.cpu()
        lo = torch.zeros(n, device=dev, dtype=ld)
        plan = TensorListPlan([n], dev)
        plan.set_ptrs(0, [a])
        plan.set_ptrs(1, [s])
        plan.set_ptrs(2, [lo])
        plan.ema(F32, w, lowp_dtype=ld)
        torch.cuda.synchronize()
        assert same_bits(a, torch.lerp(a_cpu, s_cpu, w))
        assert torch.equal(bits(lo), bits(a.to(ld)))
        plan.close()


def test_nt_source_loads_change_no_bits(cuda_device):
    """Above the Infinity Cache the source takes non-temporal loads (the engine's size rule).
    The kernel tests of this file again with GS_NT_READ_ONCE=1, which takes that path at every
    size (a child process: the policy is read once per process)."""
    import os
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(repo, "tests", "test_gpu_ema.py"), "-m", "gpu", "-q",
                        "-p", "no:cacheprovider", "-k", "test_kernel_ or test_lowp_copy"],
                       env={**os.environ, "GS_NT_READ_ONCE": "1"}, cwd=repo, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_copy_mode_moves_every_word(cuda_device):
    """an int64 tensor whose halves are quiet / signalling NaN patterns, +-0, subnormals"""
    from distributed_training_amd.multi_tensor import TensorListPlan

    words = [0x7FC00001, 0x7F800001, 0xFFC12345, 0xFF800001, 0x00000000, 0x80000000, 0x00000001, 0x807FFFFF,
             0x7FFFFFFF, 0x7F800000]
    pairs = [(lo_, hi) for lo_ in words for hi in words]
    src = torch.from_numpy(np.array([lo_ | (hi << 32) for lo_, hi in pairs], dtype=np.uint64).view(np.int64)).to(cuda_device)
    dst = torch.zeros_like(src)
    plan = TensorListPlan([2 * src.numel()], cuda_device)
    plan.set_ptrs(0, [dst.data_ptr()])
    plan.set_ptrs(1, [src.data_ptr()])
    plan.ema(F32, copy=True)
    torch.cuda.synchronize()
    assert torch.equal(dst, src)
    plan.close()


def _device_lerp_diff(dev, w):
    """(number of elements where torch._foreach_lerp_ on the device differs from the kernel,
    the largest difference in ulps of the kernel's result, elements)"""
    from distributed_training_amd.multi_tensor import TensorListPlan

    a0, s0 = rand_lists(LIST_A + [1 << 20], 21)
    a = [t.to(dev) for t in a0]
    s = [t.to(dev) for t in s0]
    b = [t.clone() for t in a]
    plan = TensorListPlan([t.numel() for t in a], dev)
    plan.set_ptrs(0, a)
    plan.set_ptrs(1, s)
    plan.ema(F32, w)
    torch._foreach_lerp_(b, s, w)
    torch.cuda.synchronize()
    plan.close()
    assert all(same_bits(x, y) for x, y in zip(a, lerp_ref(a0, s0, w)))  # the contract: torch's CPU kernel
    ka, kb = torch.cat(a), torch.cat(b)
    differ = int((bits(ka) != bits(kb)).sum())
    ulps = int((bits(ka).long() - bits(kb).long()).abs().max())
    print(f"device _foreach_lerp_ vs gs_ema_step at w={w}: {differ} of {ka.numel()} elements differ, max {ulps} ulp")
    return differ, ulps, ka.numel()


def test_device_torch_low_branch(cuda_device):
    """w = 1e-4: torch's device kernel and ours agree bit for bit (AdamOp's exp_avg.lerp_ relies on it)"""
    differ, _, _ = _device_lerp_diff(cuda_device, 1e-4)
    assert differ == 0


def test_device_torch_high_branch(cuda_device):
    """w = 0.7: the branch anchored on the source"""
    differ, _, _ = _device_lerp_diff(cuda_device, 0.7)
    assert differ == 0


def test_hyper_source_equals_arguments(cuda_device):
    from distributed_training_amd import _lib as L
    from distributed_training_amd.multi_tensor import TensorListPlan, ema_hyper

    dev = cuda_device
    a0, s0 = rand_lists(LIST_A, 31)
    s = [t.to(dev) for t in s0]
    n = torch.tensor(0, dtype=torch.int64, device=dev)
    hyper = torch.zeros(4, device=dev)
    a = [t.to(dev) for t in a0]
    b = [t.to(dev) for t in a0]
    pa = TensorListPlan(LIST_A, dev)
    pa.set_ptrs(0, a)
    pa.set_ptrs(1, s)
    pa.set_hyper_source(hyper)
    pb = TensorListPlan(LIST_A, dev)
    pb.set_ptrs(0, b)
    pb.set_ptrs(1, s)
    for it, (mode, decay) in enumerate([(L.GS_EMA_EMA, 0.3), (L.GS_EMA_SWA, 0.0), (L.GS_EMA_SWA, 0.0),
                                        (L.GS_EMA_WARMUP, 0.9999), (L.GS_EMA_EMA, 0.9999)]):
        ema_hyper(n, mode, decay, hyper)
        pa.ema(F32, 0.123)  # ignored: the kernel reads hyper
        w, copy = hyper.cpu().tolist()[:2]
        pb.ema(F32, w, copy=bool(copy))
        torch.cuda.synchronize()
        assert bool(copy) == (it == 0) and int(n) == it + 1
        assert all(same_bits(x, y) for x, y in zip(a, b)), (it, mode)
        for t in s:
            t.mul_(1.25)
    pa.close()
    pb.close()


# ------------------------------------------------------------------ the drop-in
def test_update_parameters_never_synchronises(cuda_device):
    import distributed_training_amd as D
    from distributed_training_amd.resnet import micro_resnet

    torch.manual_seed(0)
    model = micro_resnet().to(cuda_device)
    ours = D.AveragedModel(model, multi_avg_fn=D.get_ema_multi_avg_fn(0.999))
    # torch with its counter on the device too (device=None leaves torch's n_averaged on the CPU)
    theirs = S.AveragedModel(model, device=cuda_device, multi_avg_fn=S.get_ema_multi_avg_fn(0.999))
    assert ours.n_averaged.device == cuda_device and theirs.n_averaged.device == cuda_device
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            ours.update_parameters(model)
            assert ours.last_path == "fused"
        with pytest.raises(RuntimeError):  # the yardstick reads n_averaged on the host
            theirs.update_parameters(model)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(ours.n_averaged) == 3


def test_update_parameters_in_a_graph(cuda_device):
    """SWA: the weight 1 / (n + 1) changes on every replay, so a weight baked into the graph fails"""
    import distributed_training_amd as D
    from distributed_training_amd.resnet import micro_resnet

    torch.manual_seed(0)
    model = micro_resnet().to(cuda_device)
    captured = D.AveragedModel(model, use_buffers=False)
    eager = D.AveragedModel(model, use_buffers=False)
    perturb(model, 0)
    captured.update_parameters(model)  # the first update (copy), outside the graph: plans are built here
    eager.update_parameters(model)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.update_parameters(model)
    assert captured.last_path == "fused"
    for it in range(1, 5):
        perturb(model, it)
        graph.replay()
        eager.update_parameters(model)
    torch.cuda.synchronize()
    assert int(captured.n_averaged) == 5 and int(eager.n_averaged) == 5
    a, b = captured.state_dict(), eager.state_dict()
    assert list(a) == list(b) and all(same_bits(a[k], b[k]) for k in a)
    # ... and the eager updates are torch's: SWA restated on the CPU over the same sequence
    torch.manual_seed(0)
    model2 = micro_resnet()
    ref = None
    for it in range(5):
        perturb(model2, it)
        cur = [p.detach().clone() for p in model2.parameters()]
        ref = cur if ref is None else [torch.lerp(x, y, float(1 / (torch.tensor(it) + 1))) for x, y in zip(ref, cur)]
    for p, r in zip(eager.module.parameters(), ref):
        assert same_bits(p.detach(), r)


@pytest.fixture(scope="module")
def rccl_pg(cuda_device):
    if dist.is_initialized():  # another module's group is still up
        yield
        return
    init_pg("nccl", 0, 1, free_port())
    yield
    from distributed_training_amd.comm import destroy_communicators

    destroy_communicators()
    dist.destroy_process_group()


def test_end_to_end_ddp_fused_sgd_ema(cuda_device, rccl_pg):
    import distributed_training_amd as D
    from distributed_training_amd.resnet import micro_resnet

    dev = cuda_device
    torch.manual_seed(0)
    model = micro_resnet().to(dev)
    ddp = D.DistributedDataParallel(model)
    opt = D.FusedSGD(ddp.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
    ours = D.AveragedModel(model, multi_avg_fn=D.get_ema_multi_avg_fn(0.999))
    theirs = S.AveragedModel(model, multi_avg_fn=S.get_ema_multi_avg_fn(0.999))
    g = torch.Generator(device=dev).manual_seed(3)
    for _ in range(3):
        x = torch.rand(4, 3, 32, 32, device=dev, generator=g)
        y = torch.randint(0, 10, (4,), device=dev, generator=g)
        opt.zero_grad()
        nn.functional.cross_entropy(ddp(x), y).backward()
        opt.step()
        ours.update_parameters(model)
        theirs.update_parameters(model)
        assert ours.last_path == "fused"
    torch.cuda.synchronize()
    a, b = ours.module.state_dict(), theirs.module.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert same_bits(a[k], b[k]), k
    assert int(ours.n_averaged) == 3
    ddp.close()


# ------------------------------------------------------------------ ZeRO
def _zero_bf16_case(dev, rank):
    import distributed_training_amd as D
    from distributed_training_amd.resnet import BasicBlock, ResNet
    from distributed_training_amd.zero import ZeroDataParallel

    torch.manual_seed(0)
    model = ResNet(BasicBlock, [1, 1, 1, 1], num_classes=10, width=8).to(dev).to(BF16)
    z = ZeroDataParallel(model, stage=2, optimizer="adamw", lr=1e-2, reduce_bucket_size=30000)
    decay = 0.9
    avg = D.ShardedAveragedModel(z, multi_avg_fn=D.get_ema_multi_avg_fn(decay))
    pkeys = {n for n, _ in model.named_parameters()}
    g = torch.Generator(device=dev).manual_seed(5 + rank)
    ref = None
    for it in range(2):
        x = torch.rand(4, 3, 32, 32, device=dev, generator=g).to(BF16)
        y = torch.randint(0, 10, (4,), device=dev, generator=g)
        z.prepare_backward()
        nn.functional.cross_entropy(model(x).float(), y).backward()
        z.step()
        avg.update_parameters()
        full = z.consolidated_state_dict()  # CPU tensors: the restatement below is torch's CPU lerp
        ref = ({k: v.clone() for k, v in full.items()} if ref is None else
               {k: (torch.lerp(ref[k], v, 1 - decay) if k in pkeys else v.clone()) for k, v in full.items()})
    got = avg.consolidated_state_dict()
    assert list(got) == list(ref)
    for k in ref:
        assert same_bits(got[k], ref[k]), k
    assert int(avg.n_averaged) == 2
    avg.close()
    z.close()


def test_sharded_average_ws1_rccl(cuda_device, rccl_pg):
    _zero_bf16_case(cuda_device, 0)


def _ws2_worker(rank, ws, port, errq):
    try:
        init_pg("gloo", rank, ws, port)
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        _zero_bf16_case(dev, rank)
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:
        import traceback

        errq.put(f"rank {rank}: {e!r}\n{traceback.format_exc()}")
        raise


def test_sharded_average_ws2_one_gpu(cuda_device):
    ctx = mp.get_context("spawn")
    errq = ctx.SimpleQueue()
    port = free_port()
    procs = [ctx.Process(target=_ws2_worker, args=(r, 2, port, errq)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, "\n".join(errs)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
