"""The inference BatchNorm kernels on the GPU (include/gsync.h: gs_bn_infer_act, gs_bn_infer_relu_maxpool)
and the ``fused_eval`` path of fused_bn.py through the ResNets.

1. gs_bn_infer_act bit for bit on the exact grid of tests/_eval_ref.py (test_eval_cpu.py shows the grid is
   exact), all four residual x relu variants and in place, inside guarded buffers;
2. on random data within ulp_bf16(truth) / 2 + 8 * 2^-24 * (|x s| + |mean s| + |bias| + |r|): the 8 counts the
   roundings of the fixed arithmetic (three in s, one in t plus s's error carried through mean, one fma,
   one add, rounded up);
3. special values against the restated rules, a NaN confined to its channel;
4. the stem: gs_bn_infer_relu_maxpool == max_pool2d(gs_bn_infer_act(x, relu)) bit for bit;
5. modules: ``"fused_eval"`` inside the context, the stock bits outside, training untouched, and the
   fused logits no further from the fp32 model than twice the stock path's.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _bn_ref as B
from tests import _eval_ref as E

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _put(t, dev, offset=0):
    v = B.guarded(t.numel(), t.dtype, dev, offset)
    v.copy_(t.reshape(-1).to(dev))
    return v


def _run_act(lib, dev, inp, residual, relu, in_place=False, eps=E.EPS):
    """-> (y as a CPU [R, C] tensor, the buffers); asserts guards and untouched inputs"""
    from distributed_training_amd import _lib as L

    R, C = inp["x"].shape
    bufs = {k: _put(inp[k], dev) for k in ("x", "res", "mean", "var", "weight", "bias")}
    y = bufs["x"] if in_place else B.guarded(R * C, BF16, dev)
    rc = lib.gs_bn_infer_act(bufs["x"].data_ptr(), bufs["res"].data_ptr() if residual else None,
                             bufs["mean"].data_ptr(), bufs["var"].data_ptr(), bufs["weight"].data_ptr(),
                             bufs["bias"].data_ptr(), eps, int(relu), y.data_ptr(), R, C, L.stream_ptr(dev))
    assert rc == 0, lib.gs_last_error()
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert B.guards_intact(v), k
        if not (in_place and k == "x"):
            assert torch.equal(B.bits(v.cpu()), B.bits(inp[k].reshape(-1))), f"{k} was written"
    assert B.guards_intact(y)
    return y.cpu().view(R, C)


@pytest.fixture(scope="module")
def lib(cuda_device):
    from distributed_training_amd import _lib as L

    return L.lib()


# ---- 1. the exact grid ------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("variant", E.INFER_VARIANTS, ids=lambda v: f"res{int(v[0])}relu{int(v[1])}")
@pytest.mark.parametrize("shape", E.INFER_SHAPES, ids=B.shape_id)
def test_infer_act_exact_grid_bitwise(cuda_device, lib, shape, variant, in_place):
    residual, relu = variant
    inp = E.infer_exact_inputs(*shape)
    want = E.round_bf16(E.infer_steps(inp, residual, relu)["v"])
    got = _run_act(lib, cuda_device, inp, residual, relu, in_place)
    bad = B.bits(got) != B.bits(want)
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:4].tolist())


# ---- 2. random data ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", E.INFER_VARIANTS, ids=lambda v: f"res{int(v[0])}relu{int(v[1])}")
@pytest.mark.parametrize("shape", [(1025, 72), (4099, 256)], ids=B.shape_id)
def test_infer_act_random_within_bound(cuda_device, lib, shape, variant):
    residual, relu = variant
    inp = E.infer_random_inputs(*shape, seed=shape[0] + 7)
    assert float(inp["var"].min()) == 0.0 and float(inp["weight"].min()) < 0
    truth, bound = E.infer_truth(inp, residual, relu)
    got = _run_act(lib, cuda_device, inp, residual, relu).double()
    err = (got - truth).abs()
    ratio = float((err / bound).max())
    print(f"infer_act random {shape} res={residual} relu={relu}: max err / bound = {ratio:.3f}")
    assert bool((err <= bound).all()), ratio


# ---- 3. special values ------------------------------------------------------------------------------
def _restated(x, r, mean, var, w, b, relu):
    """the rules in fp32 on the CPU, for s a power of two: x * s is then exact, so the fp32 add that
    follows rounds once, as the kernel's fma does; NaN and infinities follow IEEE in both"""
    s = w * (1.0 / torch.sqrt(var + torch.tensor(E.EPS32)))
    t = (-mean) * s + b  # exact on this test's parameters
    v = x.float() * s + t
    if r is not None:
        v = v + r.float()
    if relu:
        v = torch.where(v > 0, v, torch.where(torch.isnan(v), v, torch.zeros_like(v)))
    y = v.to(BF16)
    y[torch.isnan(v)] = B.from_bits([0x7FC0])[0]  # the contract's NaN; torch's conversion keeps sign and payload
    return y


@pytest.mark.parametrize("variant", E.INFER_VARIANTS, ids=lambda v: f"res{int(v[0])}relu{int(v[1])}")
def test_infer_act_special_values(cuda_device, lib, variant):
    residual, relu = variant
    C = 16
    # NaN, +-Inf, +-0, the smallest and largest subnormal, the smallest normal, ordinary values
    pats = [0x7FC0, 0xFFC1, 0x7F80, 0xFF80, 0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x807F, 0x0080, 0x3F80, 0xBF80,
            0x4049, 0xC2C8, 0x7F7F]
    vals = B.from_bits(pats)
    R = len(pats) * len(pats)
    x = vals.repeat_interleave(len(pats)).unsqueeze(1).expand(R, C).contiguous()
    res = vals.repeat(len(pats)).unsqueeze(1).expand(R, C).contiguous()
    c = torch.arange(C)
    var = (torch.ldexp(torch.ones(C, dtype=torch.float64), 2 * ((c % 3) - 1)) - E.EPS).to(torch.float32)
    weight = torch.tensor([1.0, -1.0, 2.0, 0.5])[c % 4]
    mean = torch.tensor([0.0, 1.0, -2.0])[c % 3]
    mean[5] = 0.0
    bias = torch.tensor([0.0, 0.5, -1.0, 0.0, 2.0])[c % 5]
    bias[5] = 0.0  # channel 5: t = 0, so -0 inputs and subnormals reach the output unchanged in sign and size
    inp = dict(x=x, res=res, mean=mean, var=var, weight=weight, bias=bias)
    want = _restated(x, res if residual else None, mean, var, weight, bias, relu)
    got = _run_act(lib, cuda_device, inp, residual, relu)
    bad = B.bits(got) != B.bits(want)
    assert not bool(bad.any()), [(i, j, hex(int(B.bits(got)[i, j]) & 0xFFFF), hex(int(B.bits(want)[i, j]) & 0xFFFF))
                                 for i, j in bad.nonzero()[:6].tolist()]
    if relu:
        assert not bool((B.bits(got) == -32768).any())  # no -0 leaves the ReLU


def test_infer_act_nan_stays_in_its_channel(cuda_device, lib):
    inp = E.infer_exact_inputs(70, 72)
    inp["x"][3, 17] = math.nan     # one element
    inp["mean"][40] = math.nan     # one channel's statistics
    inp["res"][9, 65] = math.inf   # with x finite: +Inf
    got = _run_act(lib, cuda_device, inp, True, True).float()
    nan = torch.isnan(got)
    want = torch.zeros_like(nan)
    want[3, 17] = True
    want[:, 40] = True
    assert torch.equal(nan, want)
    assert float(got[9, 65]) == math.inf


# ---- 4. the stem --------------------------------------------------------------------------------------
STEM = [(1, 1, 1, 8), (1, 2, 3, 8), (2, 5, 7, 16), (1, 8, 8, 64), (3, 9, 4, 72)]


STEM_CASES = [(s, False) for s in STEM] + [((2, 5, 7, 16), True)]  # one case with NaNs


@pytest.mark.parametrize("shape,nans", STEM_CASES,
                         ids=["x".join(map(str, s)) + ("-nans" if n else "") for s, n in STEM_CASES])
def test_infer_relu_maxpool_equals_pool_of_infer_act(cuda_device, lib, shape, nans):
    from distributed_training_amd import _lib as L

    N, H, W, C = shape
    dev = cuda_device
    inp = E.infer_random_inputs(N * H * W, C, seed=sum(shape))
    if nans:
        g = torch.Generator().manual_seed(3)
        inp["x"][torch.rand(N * H * W, C, generator=g) < 0.15] = math.nan
    act = _run_act(lib, dev, inp, False, True)  # [N*H*W, C] = NHWC
    want = F.max_pool2d(act.view(N, H, W, C).permute(0, 3, 1, 2).to(dev), 3, 2, 1)  # channels_last strides
    want = want.permute(0, 2, 3, 1).contiguous().cpu()
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    bufs = {k: _put(inp[k], dev) for k in ("x", "mean", "var", "weight", "bias")}
    out = B.guarded(N * OH * OW * C, BF16, dev)
    rc = lib.gs_bn_infer_relu_maxpool(bufs["x"].data_ptr(), bufs["mean"].data_ptr(), bufs["var"].data_ptr(),
                                      bufs["weight"].data_ptr(), bufs["bias"].data_ptr(), E.EPS, out.data_ptr(), N, H,
                                      W, C, L.stream_ptr(dev))
    assert rc == 0, lib.gs_last_error()
    torch.cuda.synchronize()
    assert B.guards_intact(out) and all(B.guards_intact(v) for v in bufs.values())
    assert torch.equal(B.bits(bufs["x"].cpu()), B.bits(inp["x"].reshape(-1)))
    got = out.cpu().view(N, OH, OW, C)
    if nans:
        assert bool(torch.isnan(got.float()).any())
    assert torch.equal(B.bits(got), B.bits(want))


# ---- 5. modules ---------------------------------------------------------------------------------------
def _models(dev, name):
    from distributed_training_amd.resnet import micro_resnet, resnet50

    torch.manual_seed(0)
    m32 = (micro_resnet(width=8) if name == "micro" else resnet50(num_classes=10, width=8)).to(dev)
    g = torch.Generator().manual_seed(1)
    for mod in m32.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            n = mod.num_features
            mod.running_mean.copy_(torch.randn(n, generator=g) * 0.2)
            mod.running_var.copy_(torch.rand(n, generator=g) + 0.5)
            mod.weight.data.copy_(torch.rand(n, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(n, generator=g) * 0.1)
    import copy

    m16 = copy.deepcopy(m32)
    for mod in m16.modules():  # bf16 convolutions and classifier, fp32 BatchNorm: the benchmark's recipe
        if not isinstance(mod, torch.nn.BatchNorm2d):
            for p in mod.parameters(recurse=False):
                p.data = p.data.to(BF16)
    m16 = m16.to(memory_format=torch.channels_last)
    return m32.eval(), m16.eval()


def _check_calls(monkeypatch):
    """Wraps the two entry points the ResNets call: every call's path is recorded and, where it reports
    "stock", its output is compared bit for bit with the stock modules applied to the same input.  The whole
    model's logits are not compared between two runs: MIOpen's convolutions are not bitwise repeatable from
    call to call on every shape (seen here on resnet50(width=8), stock against stock), so only a per-call
    comparison says that the code outside the context is the stock code."""
    from distributed_training_amd import fused_bn, resnet

    paths = []
    act, pool_ = resnet.bn_act, resnet.bn_relu_pool

    def bn_act(bn, x, relu=True, residual=None, fork=False):
        want = bn(x)
        if residual is not None:
            want = want + residual
        if relu:
            want = F.relu(want)
        out = act(bn, x, relu=relu, residual=residual, fork=fork)
        paths.append(fused_bn.last_path)
        if paths[-1] == "stock":
            assert torch.equal(B.bits(out[0] if fork else out), B.bits(want))
        return out

    def bn_relu_pool(bn, x, pool, fork=True):
        want = pool(F.relu(bn(x)))
        out = pool_(bn, x, pool, fork=fork)
        paths.append(fused_bn.last_path)
        if paths[-1] == "stock":
            assert torch.equal(B.bits(out[0] if fork else out), B.bits(want))
        return out

    monkeypatch.setattr(resnet, "bn_act", bn_act)
    monkeypatch.setattr(resnet, "bn_relu_pool", bn_relu_pool)
    return paths


@pytest.mark.parametrize("name", ["micro", "resnet50"])
def test_modules_fused_eval(cuda_device, monkeypatch, name):
    from distributed_training_amd import fused_bn

    dev = cuda_device
    m32, m16 = _models(dev, name)
    n_bn = sum(isinstance(m, torch.nn.BatchNorm2d) for m in m16.modules())
    g = torch.Generator().manual_seed(2)
    x32 = torch.rand(4, 3, 64, 64, generator=g).to(dev)
    x = x32.to(BF16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        ref = m32(x.float()).double()
        paths = _check_calls(monkeypatch)
        stock = m16(x)
        assert paths == ["stock"] * n_bn  # every BatchNorm, each bit for bit the stock modules' (checked per call)
        del paths[:]
        with fused_bn.fused_eval():
            fused = m16(x)
        assert paths == ["fused_eval"] * n_bn
        del paths[:]
        m16(x)  # after the context: the stock path again, bit for bit per call
        with fused_bn.fused_eval(False):
            m16(x)
        assert paths == ["stock"] * (2 * n_bn)
        del paths[:]
    e_stock = float((stock.double() - ref).abs().max())
    e_fused = float((fused.double() - ref).abs().max())
    print(f"{name}: max logit error against fp32: stock {e_stock:.6f}, fused_eval {e_fused:.6f} "
          f"(|logit| max {float(ref.abs().max()):.3f})")
    assert e_stock > 0
    assert e_fused <= 2 * e_stock, (e_fused, e_stock)
    # grad mode on but nothing requires grad: still the inference kernels; an input that requires grad: stock
    for p in m16.parameters():
        p.requires_grad_(False)
    with fused_bn.fused_eval():
        out = m16(x)
        assert paths == ["fused_eval"] * n_bn and not out.requires_grad
        del paths[:]
        m16(x.clone().requires_grad_())
        assert paths == ["stock"] * n_bn


def test_training_inside_the_context_is_untouched(cuda_device):
    from distributed_training_amd import fused_bn

    dev = cuda_device
    _, m16 = _models(dev, "micro")
    m16.train()
    g = torch.Generator().manual_seed(4)
    x = torch.rand(4, 3, 32, 32, generator=g).to(dev).to(BF16).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (4,), generator=g).to(dev)

    def step():
        for p in m16.parameters():
            p.grad = None
        F.cross_entropy(m16(x).float(), y).backward()
        return [p.grad.clone() for p in m16.parameters()]

    with fused_bn.fused_eval():
        inside = step()
        assert fused_bn.last_path == "fused"
    assert all(bool(torch.isfinite(g_).all()) for g_ in inside)
    tracked = [int(m.num_batches_tracked) for m in m16.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert set(tracked) == {1}  # the training bookkeeping ran
