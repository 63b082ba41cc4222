"""The training criterion on the GPU: gs_xent_fwd / gs_xent_bwd's HIP kernels against the numpy fp64
restatement and torch in fp64 (the bounds test_xent_cpu.py derives), their agreement with the host backend
(codes and counts identical), the ``loss`` module on the device, under bf16 autocast and inside a hipGraph."""
import math

import pytest
import torch

from tests import _eval_ref as E
from tests import _xent_ref as X
from tests.test_xent_cpu import LAYOUTS, check_accumulator, check_module, masked_case

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
ALL = ("none", "mean", "sum")


@pytest.fixture(scope="module")
def lib(cuda_device):
    from distributed_training_amd import _lib as L

    return L.lib()


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [1, 2, 7, 8, 65, 1000])
@pytest.mark.parametrize("Bn", [1, 3, 64, 257])
def test_hip_loss_and_gradient(cuda_device, lib, Bn, K, dtype, eps):
    logits, labels = X.xent_case(Bn, K, dtype, seed=Bn * 1009 + K)
    if Bn > 4:
        logits[4, K // 2] = math.nan  # a NaN row
    out = X.run_xent(lib, logits, labels, eps, ALL, device=cuda_device)
    X.check_xent(logits, labels, eps, out)
    host = X.run_xent(lib, logits, labels, eps, ())
    assert torch.equal(out["code"], host["code"]) and out["red"][2:] == host["red"][2:]


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("case", LAYOUTS, ids=lambda c: f"{c[0]}x{c[1]}-{str(c[2])[6:]}-pad{c[3]}")
def test_hip_layouts(cuda_device, lib, case, eps):
    """the 16-byte path (whole vectors, a tail, a row shorter than a vector, two chunks) and the scalar one"""
    Bn, K, dtype, pad = case
    logits, labels = X.xent_case(Bn, K, dtype, seed=K + pad, pad=pad)
    out = X.run_xent(lib, logits, labels, eps, ALL, device=cuda_device)
    X.check_xent(logits, labels, eps, out)


def test_hip_fp16_masked_class_and_one_class(cuda_device, lib):
    logits, labels = X.xent_case(9, 33, torch.float16, seed=9)
    X.check_xent(logits, labels, 0.1, X.run_xent(lib, logits, labels, 0.1, ALL, device=cuda_device))
    logits, labels = masked_case()
    out = X.run_xent(lib, logits, labels, 0.0, ALL, device=cuda_device)
    X.check_xent(logits, labels, 0.0, out)
    assert math.isfinite(float(out["rows"][3, 0])) and all(float(dz[3, 5]) == 0.0 for dz in out["dz"].values())
    out = X.run_xent(lib, logits, labels, 0.1, ALL, device=cuda_device)
    X.check_xent(logits, labels, 0.1, out, against_torch=False)
    assert float(out["rows"][3, 0]) == math.inf == out["red"][0] == out["red"][1]
    logits, labels = X.xent_case(4, 1, BF16, seed=8, specials=False)
    for eps in (0.0, 0.1):
        out = X.run_xent(lib, logits, labels, eps, ALL, device=cuda_device)
        assert not out["rows"][:, 0].any() and out["red"] == (0.0, 0.0, 4, 0)
        assert not any(dz[:, :1].any() for dz in out["dz"].values())


def test_hip_bad_label_and_all_ignored(cuda_device, lib):
    logits, labels = X.xent_case(6, 10, torch.float32, seed=6, specials=False)
    labels[2] = 10
    labels[4] = -3
    acc = torch.zeros(8, dtype=torch.int64, device=cuda_device)
    out = X.run_xent(lib, logits, labels, 0.1, ALL, device=cuda_device, topk=(1, 5), acc=acc)
    X.check_xent(logits, labels, 0.1, out)
    assert out["red"][2:] == (4, 2) and math.isnan(out["red"][0]) and math.isnan(out["red"][1])
    assert E.acc_words(acc)[:2] == [4, 2]
    assert not any(dz[[2, 4], :10].any() for dz in out["dz"].values())
    labels[:] = -100
    out = X.run_xent(lib, logits, labels, 0.1, ALL, device=cuda_device)
    X.check_xent(logits, labels, 0.1, out)
    assert out["red"][0] == 0.0 and math.isnan(out["red"][1]) and out["red"][2:] == (0, 0)
    # an empty batch writes the reduced result and nothing else
    from distributed_training_amd import _lib as L

    red = torch.full((4,), 7.0, device=cuda_device)
    acc.fill_(3)
    rc = lib.gs_xent_fwd(L.GS_DEV_HIP, None, L.GS_F32, None, 0, 10, 10, -100, 0.1, None, red.data_ptr(),
                         L.i32_array((1,)), 1, acc.data_ptr(), L.stream_ptr(cuda_device))
    assert rc == 0, lib.gs_last_error()
    red = red.cpu()
    assert float(red[0]) == 0.0 and math.isnan(float(red[1])) and red.view(torch.int32)[2:].tolist() == [0, 0]
    assert acc.tolist() == [3] * 8


def test_hip_twice_gives_identical_bits(cuda_device, lib):
    logits, labels = X.xent_case(257, 1000, BF16, seed=12)
    a = X.run_xent(lib, logits, labels, 0.1, ALL, device=cuda_device)
    b = X.run_xent(lib, logits, labels, 0.1, ALL, device=cuda_device)
    assert torch.equal(a["rows"].view(torch.int32), b["rows"].view(torch.int32)) and str(a["red"]) == str(b["red"])
    for k in ALL:
        assert torch.equal(a["dz"][k].view(torch.int16), b["dz"][k].view(torch.int16))


def test_hip_accumulator_equals_eval_accumulate(cuda_device, lib):
    check_accumulator(lib, cuda_device)


@pytest.mark.filterwarnings("ignore:size_average and reduce args")
def test_module_on_the_device(cuda_device):
    check_module(cuda_device)


def test_micro_resnet_under_bf16_autocast(cuda_device):
    import distributed_training_amd as D
    from distributed_training_amd import loss as LS
    from distributed_training_amd.resnet import micro_resnet

    dev = cuda_device
    torch.manual_seed(0)
    model = micro_resnet().to(dev)
    x = torch.rand(8, 3, 32, 32, device=dev)
    y = torch.randint(0, 10, (8,), device=dev)
    m = D.Metrics(topk=(1,), device=dev)
    crit = D.CrossEntropyLoss(label_smoothing=0.1, metrics=m)
    with torch.autocast("cuda", dtype=BF16):
        logits = model(x)
        loss = crit(logits, y)
    assert logits.dtype == BF16 and LS.last_path == "fused" and loss.dtype == torch.float32
    loss.backward()
    assert math.isfinite(float(loss.detach()))
    grads = [p.grad for p in model.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(bool(g.any()) for g in grads)
    want = torch.nn.functional.cross_entropy(logits.detach().double(), y, label_smoothing=0.1)
    assert float(loss.detach()) == pytest.approx(float(want), rel=1e-5)
    assert m.compute()["n"] == 8


def test_criterion_in_a_graph_replayed_three_times(cuda_device):
    import distributed_training_amd as D

    dev = cuda_device
    logits, labels = E.metric_case(64, 100, BF16, seed=3, pad=0)
    z = logits.contiguous().to(dev).requires_grad_()
    y = labels.to(dev)
    m = D.Metrics(topk=(1, 5), device=dev)
    crit = D.CrossEntropyLoss(label_smoothing=0.1, metrics=m)
    crit(z, y).backward()  # the warm-up call, and the eager result
    eager = z.grad.clone()
    once = m.compute()
    z.grad = None
    m.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        crit(z, y).backward()
    m.reset()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(z.grad.view(torch.int16), eager.view(torch.int16)) and bool(eager.any())
    got = m.compute()
    assert got["n"] == 3 * once["n"] == 3 * 63  # one row is ignore_index
    assert got["correct1"] == 3 * once["correct1"] and got["correct5"] == 3 * once["correct5"]
    assert got["loss_sum"] == pytest.approx(3 * once["loss_sum"], rel=1e-12)
