"""Evaluation on the GPU: gs_eval_accumulate's HIP kernels against the host backend and the numpy
restatement (counts exact, every row's loss within the bound test_eval_cpu.py derives), ``Metrics.update``
inside a hipGraph, and ``evaluate`` at ws = 1 over the RCCL communicator and with two gloo ranks on one GPU."""
import math

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _eval_ref as E
from tests._dist_util import free_port, init_pg
from tests._eval_ref import BATCH, N_SAMPLES, TOPK, check_against_ref, run_accumulate
from tests._eval_ref import eval_dataset as _dataset
from tests._eval_ref import eval_model as _model

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _hip_accumulate(lib, dev, logits, labels, n_valid, topk=TOPK, acc=None):
    from distributed_training_amd import _lib as L

    Bn, K = logits.shape
    stride = logits.stride(0)
    dl = torch.full((Bn, stride), math.nan, dtype=logits.dtype, device=dev)
    dl[:, :K] = logits.to(dev)
    dy = labels.to(dev)
    acc = torch.zeros(8, dtype=torch.int64, device=dev) if acc is None else acc
    ws = torch.empty(Bn, dtype=torch.int64, device=dev)
    rc = lib.gs_eval_accumulate(L.GS_DEV_HIP, dl.data_ptr(), L.gs_dtype(logits.dtype), dy.data_ptr(), Bn, K, stride,
                                n_valid, L.i32_array(topk), len(topk), -100, ws.data_ptr(), acc.data_ptr(),
                                L.stream_ptr(dev))
    assert rc == 0, lib.gs_last_error()
    torch.cuda.synchronize()
    return acc, ws


@pytest.fixture(scope="module")
def lib(cuda_device):
    from distributed_training_amd import _lib as L

    return L.lib()


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [1, 2, 10, 65, 1000])
@pytest.mark.parametrize("Bn", [1, 3, 64, 257])
def test_hip_equals_host(cuda_device, lib, Bn, K, dtype):
    logits, labels = E.metric_case(Bn, K, dtype, seed=Bn * 1009 + K)
    if Bn > 4:
        logits[4, K // 2] = math.nan  # a NaN row
    for n_valid in sorted({0, 1, Bn - 1, Bn}):
        hacc, hws = run_accumulate(lib, logits, labels, n_valid)
        dacc, dws = _hip_accumulate(lib, cuda_device, logits, labels, n_valid)
        check_against_ref(logits, labels, n_valid, dacc.cpu(), dws.cpu())
        h, d = E.acc_words(hacc), E.acc_words(dacc)
        assert h[:2] == d[:2] and h[3:] == d[3:]
        assert (math.isnan(h[2]) and math.isnan(d[2])) or abs(h[2] - d[2]) <= 2e-5 * max(1.0, abs(h[2]))
        # the ranks and the reasons of the uncounted rows agree row by row
        assert torch.equal(hws.view(torch.int32)[1::2], dws.cpu().view(torch.int32)[1::2])
        # bitwise repeatable
        dacc2, _ = _hip_accumulate(lib, cuda_device, logits, labels, n_valid)
        assert torch.equal(dacc, dacc2)


def test_hip_bad_label_and_fp16(cuda_device, lib):
    logits, labels = E.metric_case(9, 33, torch.float16, seed=9)
    labels[5] = 33
    dacc, dws = _hip_accumulate(lib, cuda_device, logits, labels, 9)
    check_against_ref(logits, labels, 9, dacc.cpu(), dws.cpu())
    assert E.acc_words(dacc)[1] == 1


def test_update_in_a_graph_replayed_three_times(cuda_device):
    from distributed_training_amd import Metrics

    dev = cuda_device
    logits, labels = E.metric_case(64, 100, BF16, seed=3, pad=0)
    logits, labels = logits.to(dev).contiguous(), labels.to(dev)
    m = Metrics(topk=(1, 5), device=dev)
    m.update(logits, labels, 60)  # sizes the scratch outside the capture
    once = m.compute()
    m.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        m.update(logits, labels, 60)
    m.reset()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    got = m.compute()
    assert got["n"] == 3 * once["n"] == 3 * 59  # 60 valid rows, one of them ignore_index
    assert got["correct1"] == 3 * once["correct1"] and got["correct5"] == 3 * once["correct5"]
    assert got["loss_sum"] == pytest.approx(3 * once["loss_sum"], rel=1e-12)


# ---- evaluate -------------------------------------------------------------------------------------------
def _bf16_model(dev):
    m = _model().to(dev)
    for mod in m.modules():  # bf16 convolutions and classifier, fp32 BatchNorm
        if not isinstance(mod, torch.nn.BatchNorm2d):
            for p in mod.parameters(recurse=False):
                p.data = p.data.to(BF16)
    return m.to(memory_format=torch.channels_last)


def _evaluate_all(dev, ws, rank):
    """the assertions of the CPU test for the bf16 model on the GPU"""
    import distributed_training_amd as D
    from distributed_training_amd import data as gdata
    from distributed_training_amd import fused_bn

    ds = _dataset()
    model = _bf16_model(dev)
    want = D.evaluate(model, torch.utils.data.DataLoader(ds, batch_size=BATCH), process_group=None) \
        if ws == 1 else None
    out = {}
    for name, cls in (("torch", torch.utils.data.distributed.DistributedSampler), ("ours", gdata.DistributedSampler)):
        sampler = cls(ds, num_replicas=ws, rank=rank, shuffle=False, drop_last=False)
        loader = torch.utils.data.DataLoader(ds, batch_size=BATCH, sampler=sampler)
        out[name] = D.evaluate(model, loader)
        assert fused_bn.last_path == "fused_eval"
        out[name + "_padded"] = D.evaluate(model, loader, dedup_padding=False)
    # a single-process pass over the whole set on this rank: every count must equal it exactly
    single = Metrics_single(model, ds, dev)
    padded_n = math.ceil(N_SAMPLES / ws) * ws
    for name in ("torch", "ours"):
        r = out[name]
        assert r["n"] == N_SAMPLES
        assert r["correct1"] == single["correct1"] and r["correct5"] == single["correct5"]
        # bf16 logits: a batch of another composition may move a logit by a bf16 ulp (2^-8 relative)
        assert r["loss"] == pytest.approx(single["loss"], rel=2.0 ** -6)
        assert out[name + "_padded"]["n"] == padded_n
    if want is not None:
        assert want["n"] == N_SAMPLES and want["correct1"] == single["correct1"]
    return out


def Metrics_single(model, ds, dev):
    """one batch-of-4 pass over the whole dataset with no sampler and no reduction"""
    import distributed_training_amd as D
    from distributed_training_amd import fused_bn

    m = D.Metrics(device=dev)
    model.eval()
    with torch.no_grad(), fused_bn.fused_eval():
        for i in range(0, N_SAMPLES, BATCH):
            x = ds.tensors[0][i:i + BATCH].to(dev).to(BF16).contiguous(memory_format=torch.channels_last)
            m.update(model(x), ds.tensors[1][i:i + BATCH].to(dev))
    return m.compute()


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


def test_evaluate_ws1_over_rccl(cuda_device, rccl_pg):
    _evaluate_all(cuda_device, 1, 0)


def test_evaluate_device_loader(cuda_device, rccl_pg):
    """DeviceDataLoader + data.DistributedSampler, as build_dataloader makes the test loader"""
    import distributed_training_amd as D
    from distributed_training_amd import data as gdata

    dev = cuda_device
    ds = gdata.ImageDataset.synthetic(n=N_SAMPLES, seed=2, device=dev)
    loader = gdata.DeviceDataLoader(ds, batch_size=BATCH, sampler=gdata.DistributedSampler(ds, 1, 0, shuffle=False),
                                    out_dtype=BF16, memory_format=torch.channels_last)
    out = D.evaluate(_bf16_model(dev), loader)
    assert out["n"] == N_SAMPLES and 0 <= out["correct1"] <= out["correct5"] <= N_SAMPLES


def _ws2_worker(rank, ws, port, errq):
    try:
        init_pg("gloo", rank, ws, port)
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        _evaluate_all(dev, ws, rank)
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:
        import traceback

        errq.put(f"rank {rank}: {e!r}\n{traceback.format_exc()}")
        raise


def test_evaluate_ws2_gloo_one_gpu(cuda_device):
    ctx = mp.get_context("spawn")
    errq = ctx.SimpleQueue()
    port = free_port()
    procs = [ctx.Process(target=_ws2_worker, args=(r, 2, port, errq)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
    for p in procs:
        if p.is_alive():
            p.terminate()
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, "\n".join(errs)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
