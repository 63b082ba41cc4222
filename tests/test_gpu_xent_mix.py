"""The pair-target criterion on the GPU: gs_xent_mix_fwd / gs_xent_mix_bwd's HIP kernels against the fp64
restatement and the torch composition (the bounds tests/_mix_ref.py derives), their bit identity with the
one-label kernels, the ``loss`` module on the device, under bf16 autocast, and inside a hipGraph whose targets
change between replays."""
import math

import pytest
import torch

from tests import _mix_ref as M
from tests.test_xent_mix_cpu import (ALL, DTYPES, SHAPES, check_metrics, check_module, check_one_label_identity,
                                     check_shape, check_special_rows)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def lib(cuda_device):
    from distributed_training_amd import _lib as L

    return L.lib()


@pytest.mark.parametrize("eps", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hip_loss_and_gradient(cuda_device, lib, shape, dtype, eps):
    logits, a, b, lam, out = check_shape(lib, *shape, dtype, eps, device=cuda_device)
    host = M.run_xent_mix(lib, logits, a, b, lam, eps, ())
    assert torch.equal(out["code"], host["code"]) and out["red"][2:] == host["red"][2:]


def test_hip_aligned_rows_take_the_vector_path(cuda_device, lib):
    """row strides that are multiples of 16 bytes (the 16-byte loads and stores of the backward), with a tail"""
    for Bn, K, dtype, pad in ((64, 1000, BF16, 0), (3, 2500, BF16, 4), (3, 2500, torch.float32, 3), (5, 65, BF16, 7)):
        logits, a, b, lam = M.mix_case(Bn, K, dtype, seed=K + pad)
        buf = torch.full((Bn, K + pad), math.nan, dtype=dtype)
        buf[:, :K] = logits
        view = buf[:, :K]
        for eps in (0.0, 0.1):
            out = M.run_xent_mix(lib, view, a, b, lam, eps, ALL, device=cuda_device)
            M.check_xent_mix(view, a, b, lam, eps, out)


def test_hip_one_label_rows_are_the_one_label_kernels_bits(cuda_device, lib):
    check_one_label_identity(lib, cuda_device)


def test_hip_special_rows(cuda_device, lib):
    check_special_rows(lib, cuda_device)


def test_hip_metrics(cuda_device, lib):
    check_metrics(lib, cuda_device)


def test_hip_twice_gives_identical_bits(cuda_device, lib):
    logits, a, b, lam = M.mix_case(257, 1000, BF16, seed=12)
    x = M.run_xent_mix(lib, logits, a, b, lam, 0.1, ALL, device=cuda_device)
    y = M.run_xent_mix(lib, logits, a, b, lam, 0.1, ALL, device=cuda_device)
    assert torch.equal(x["rows"].view(torch.int32), y["rows"].view(torch.int32)) and str(x["red"]) == str(y["red"])
    assert all(M.same_bits(x["dz"][k], y["dz"][k]) for k in ALL)


def test_module_on_the_device(cuda_device):
    check_module(cuda_device)


class _Micro(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.body = torch.nn.Sequential(torch.nn.Linear(48, 64), torch.nn.ReLU(), torch.nn.Linear(64, 1000))

    def forward(self, x):
        return self.body(x)


def test_micro_model_under_bf16_autocast(cuda_device):
    import distributed_training_amd as D
    from distributed_training_amd import loss as LS

    dev = cuda_device
    torch.manual_seed(0)
    model = _Micro().to(dev)
    x = torch.randn(64, 48, device=dev)
    gen = torch.Generator().manual_seed(1)
    t = D.MixedTarget(torch.randint(0, 1000, (64,), generator=gen).to(dev),
                      torch.randint(0, 1000, (64,), generator=gen).to(dev), torch.rand(64, generator=gen).to(dev))
    m = D.Metrics(topk=(1, 5), device=dev)
    crit = D.CrossEntropyLoss(label_smoothing=0.1, metrics=m)
    with torch.autocast("cuda", dtype=BF16):
        logits = model(x)
        loss = crit(logits, t)
    assert logits.dtype == BF16 and logits.shape == (64, 1000) and LS.last_path == "fused" and loss.dtype == torch.float32
    loss.backward()
    grads = [p.grad for p in model.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(bool(g.any()) for g in grads)
    z64 = logits.detach().double()
    ce = torch.nn.functional.cross_entropy
    want = (t.lam.double() * ce(z64, t.labels_a, reduction="none", label_smoothing=0.1)
            + (1 - t.lam.double()) * ce(z64, t.labels_b, reduction="none", label_smoothing=0.1)).mean()
    assert float(loss.detach()) == pytest.approx(float(want), rel=1e-5)
    assert m.compute()["n"] == 64


def test_criterion_in_a_graph_replayed_with_new_targets(cuda_device):
    import distributed_training_amd as D

    dev = cuda_device
    logits, a, b, lam = M.mix_case(64, 100, BF16, seed=3)
    z = logits.contiguous().to(dev).requires_grad_()
    gen = torch.Generator().manual_seed(9)
    targets = []
    for k in range(3):
        ak = torch.randint(0, 100, (64,), generator=gen)
        bk = torch.randint(0, 100, (64,), generator=gen)
        lk = torch.rand(64, generator=gen)
        ak[k], lk[k + 3], bk[k + 6] = -100, 1.0, ak[k + 6]  # a skipped row and both kinds of one-label row
        targets.append((ak.to(dev), bk.to(dev), lk.to(dev)))
    crit = D.CrossEntropyLoss(label_smoothing=0.1)

    def eager_step(target):
        # in a function of its own: no loss, hence no autograd graph, outlives the step.  A graph left alive would keep
        # z's AccumulateGrad node, which runs on the stream it was made on, and drag that stream into the recording
        z.grad = None
        loss = crit(z, target)
        loss.backward()
        return loss.detach().clone(), z.grad.clone()

    eager = [eager_step(D.MixedTarget(ak, bk, lk)) for ak, bk, lk in targets]
    static = D.MixedTarget(a.to(dev), b.to(dev), lam.to(dev))
    z.grad = None
    crit(z, static).backward()  # the warm-up call
    z.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        out = crit(z, static)
        out.backward()
    for (ak, bk, lk), (want_loss, want_grad) in zip(targets, eager):
        static.labels_a.copy_(ak)
        static.labels_b.copy_(bk)
        static.lam.copy_(lk)
        graph.replay()
        torch.cuda.synchronize()
        assert M.same_bits(out.detach().reshape(1), want_loss.reshape(1))
        assert M.same_bits(z.grad, want_grad) and bool(want_grad.any())
    assert not M.same_bits(eager[0][1], eager[1][1])
