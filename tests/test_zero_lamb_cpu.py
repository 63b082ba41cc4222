"""LAMB and LARS under ZeRO-1/2 and 16-bit on the host backend (CPU tensors, gloo): the
update kernels' low-precision copy (gs_lars_step_lowp / gs_lamb_step_lowp), the sharded
step of ZeroDataParallel(optimizer="lamb" | "lars") against the numpy float32
restatements (tests/_zero_lamb_common.py), the fp16 overflow skip, the checkpoints and
the DeepSpeed / ColossalAI surfaces."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import _zero_lamb_common as Z
from tests.test_ddp_cpu import _run

CPU = torch.device("cpu")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIMS = os.path.join(REPO, "distributed_training_amd", "compat", "shims")


# ---- 1. the update kernels with the copy
@pytest.mark.parametrize("placement", Z.PLACEMENTS)
@pytest.mark.parametrize("ldt", [torch.bfloat16, torch.float16])
def test_lamb_step_lowp(ldt, placement):
    Z.run_lamb_lowp(CPU, ldt, placement)


@pytest.mark.parametrize("placement", Z.PLACEMENTS)
@pytest.mark.parametrize("mom", [0.9, 0.0])
@pytest.mark.parametrize("ldt", [torch.bfloat16, torch.float16])
def test_lars_step_lowp(ldt, mom, placement):
    Z.run_lars_lowp(CPU, ldt, mom, placement)


@pytest.mark.parametrize("ldt", [torch.bfloat16, torch.float16])
def test_pieces_off_a_4_element_boundary(ldt):
    Z.run_unaligned_pieces(CPU, ldt)


def test_lowp_argument_errors():
    from distributed_training_amd import _lib as L
    from tests import _lamb_common as CL

    p, g, m, v = CL.make_tensors(CPU, torch.float32, False, seed=1)
    plan = CL.make_plan(CPU, p, g, m, v)
    norms = CL.new_norms(CPU)
    with pytest.raises(RuntimeError, match="slot 4 of tensor 0 is not bound"):
        plan.lamb(0.1, 1e-6, 0.0, 1.0, 1.0, norms, lowp_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="slot 3 of tensor 0 is not bound"):
        plan.set_ptrs(3, [0] * len(Z.SIZES))
        plan.lars(torch.float32, 0.1, 0.0, 0.0, 1e-3, 1e-8, norms, lowp_dtype=torch.float16)
    lib = L.lib()
    assert lib.gs_lamb_step_lowp(plan.handle, L.GS_F32, 0.1, 1e-6, 0.0, 1.0, 1.0, 0.0, 1.0, norms.data_ptr(),
                                 None, None) == L.GS_EINVAL
    # a clip set on the plan stays GS_ESTATE
    sq = torch.ones(1)
    plan.set_clip(1.0, 1e-6, sq)
    assert lib.gs_lamb_step_lowp(plan.handle, -1, 0.1, 1e-6, 0.0, 1.0, 1.0, 0.0, 1.0, norms.data_ptr(),
                                 None, None) == L.GS_ESTATE
    assert lib.gs_lars_step_lowp(plan.handle, L.GS_F32, -1, 0.1, 0.0, 0.0, 1e-3, 1e-8, norms.data_ptr(),
                                 None, None, None) == L.GS_ESTATE
    plan.close()


# ---- 2. / 3. the sharded step
def _bucket_worker(rank, ws):
    for dtype in (torch.float32, torch.bfloat16):
        z = Z.make_engine(Z.model_of("micro").to(dtype), "lamb", 2)
        Z.assert_piece_preconditions(z)
        split, empty, _ = Z.piece_cases(z)
        assert split >= 1 and empty >= 1
        z.close()


@pytest.mark.parametrize("ws", [2, 3])
def test_bucket_size_gives_the_piece_cases(ws):
    _run(_bucket_worker, ws)


def _lamb_worker(rank, ws, stage, dtype):
    Z.sharded_step_vs_restatement(rank, ws, CPU, "lamb", stage, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("ws", [1, 2, 3])
def test_sharded_lamb_step(ws, stage, dtype):
    """Fails on the parent commit: there optimizer="lamb" ran the Adam branch (and had
    neither a piece plan nor sq_norms())."""
    _run(_lamb_worker, ws, stage, dtype)


def _lamb_clamp_worker(rank, ws):
    Z.sharded_step_vs_restatement(rank, ws, CPU, "lamb", 2, torch.bfloat16, clamp=Z.CLAMP)


def test_sharded_lamb_step_applies_the_trust_clamp_ws2():
    _run(_lamb_clamp_worker, 2)


def _lars_worker(rank, ws):
    Z.sharded_step_vs_restatement(rank, ws, CPU, "lars", 2, torch.bfloat16)


def test_sharded_lars_step_bf16_stage2_ws2():
    _run(_lars_worker, 2)


# ---- 4. fp16 overflow
def _overflow_worker(rank, ws, kind):
    Z.overflow_skips_the_step(rank, ws, CPU, kind)


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_fp16_overflow_skips_the_step_ws2(kind):
    _run(_overflow_worker, 2, kind)


# ---- 6. checkpoints
def _checkpoint_worker(rank, ws, kind):
    Z.checkpoint_round_trips(rank, ws, CPU, kind)


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_checkpoint_round_trips_ws2(kind):
    _run(_checkpoint_worker, 2, kind)


# ---- 7. the compat surfaces
def _ds_worker(rank, ws):
    sys.path.insert(0, SHIMS)
    import deepspeed

    from distributed_training_amd.zero import ZeroDataParallel
    from tests._lamb_common import small_model

    cfg = {"train_batch_size": 4 * ws, "bf16": {"enabled": True}, "zero_optimization": {"stage": 2},
           "gradient_clipping": 1.0,
           "optimizer": {"type": "Lamb", "params": {"lr": 0.01, "max_coeff": 0.3, "min_coeff": 0.05,
                                                    "weight_decay": 0.01}}}
    # without the key: today's refusal, with a hint naming the key
    with pytest.raises(NotImplementedError, match="span ranks") as e:
        deepspeed.initialize(args=None, model=small_model(CPU), config=cfg)
    assert "zero_allow_untested_optimizer" in str(e.value)
    cfg["zero_allow_untested_optimizer"] = True
    model = small_model(CPU)
    engine, opt, _, _ = deepspeed.initialize(args=None, model=model, model_parameters=model.parameters(), config=cfg)
    assert isinstance(opt, ZeroDataParallel) and opt.kind == "lamb" and opt.stage == 2 and opt.dtype == torch.bfloat16
    assert opt.adapt == [True] * len(opt.params)  # DeepSpeed's FusedLamb adapts every tensor
    assert (opt.min_trust, opt.max_trust, opt.bias_correction, opt.clip) == (0.05, 0.3, True, 1.0)
    dev = engine.device
    crit = nn.CrossEntropyLoss()
    gen = torch.Generator().manual_seed(3 + rank)
    before = [p.detach().clone() for p in opt.params]
    for _ in range(2):
        x = torch.randn(4, 3, 8, 8, generator=gen).to(dev).to(torch.bfloat16)
        y = torch.randint(0, 10, (4,), generator=gen).to(dev)
        engine.backward(crit(engine(x).float(), y))
        engine.step()
    assert engine.global_steps == 2 and opt.step_count == 2
    assert all(not torch.equal(a, b) for a, b in zip(before, opt.params))
    # min_coeff / max_coeff in force: some free ratio of the last step lies outside the clamp
    from tests._lamb_common import ref_ratios

    free = np.array(ref_ratios(opt.sq_norms()[1].cpu().numpy(), opt.adapt))
    assert (free < 0.05).any() or (free > 0.3).any()
    # the other spellings, and 16-bit at stage 0, take the same engine
    for key, extra in (("FusedLamb", {"zero_optimization": {"stage": 1}}), ("LAMB", {"zero_optimization": {"stage": 0}})):
        cfg2 = dict(cfg, **extra)
        cfg2["optimizer"] = dict(cfg["optimizer"], type=key)
        _, o2, _, _ = deepspeed.initialize(args=None, model=small_model(CPU), config=cfg2)
        assert isinstance(o2, ZeroDataParallel) and o2.kind == "lamb" and o2.stage == 1
        o2.close()
    opt.close()


def test_deepspeed_lamb_bf16_stage2_with_the_key():
    _run(_ds_worker, 2)


def _ds_reference_config_worker(rank, ws, stage, dtype):
    """The reference trainer's DeepSpeed config (tests/golden/make_ds_golden.py::ds_config, its
    values unchanged) with "type": "Lamb" and the key, through the harness loop of
    tests/test_ds_harness_cpu.py: builds, trains three steps, replicas stay identical."""
    sys.path.insert(0, SHIMS)
    import deepspeed
    import torch.distributed as dist

    from tests.golden.make_ds_golden import dataset, ds_config, micro

    torch.set_num_threads(2)
    cfg = ds_config(stage, dtype)
    cfg["optimizer"] = dict(cfg["optimizer"], type="Lamb")
    cfg["zero_allow_untested_optimizer"] = True
    torch.manual_seed(0)
    model = micro()
    engine, opt, loader, _ = deepspeed.initialize(args=None, model=model,
                                                  model_parameters=filter(lambda p: p.requires_grad, model.parameters()),
                                                  training_data=dataset(), config=cfg)
    assert opt.kind == "lamb" and opt.dtype == torch.bfloat16 and opt.clip == 1.0 and opt.hp["betas"] == (0.8, 0.999)
    crit = nn.CrossEntropyLoss()
    before = [p.detach().clone() for p in model.parameters()]
    n = 0
    for images, labels in loader:
        loss = crit(model(images.to(torch.bfloat16)), labels)
        assert torch.isfinite(loss.float()).item()
        engine.backward(loss)
        engine.step()
        n += 1
    # WarmupLR leaves lr 0 for the first step: two of the three steps move the weights
    assert n == 3 and engine.global_steps == 3
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    w = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()])
    allw = [torch.zeros_like(w) for _ in range(ws)]
    dist.all_gather(allw, w)
    assert torch.equal(allw[0], allw[1]), "replicas diverged"
    opt.close()


@pytest.mark.parametrize("stage", [0, 1, 2])
def test_reference_deepspeed_config_with_lamb_default_bf16(stage):
    _run(_ds_reference_config_worker, 2, stage, "bf16")


def _colossal_worker(rank, ws):
    import distributed_training_amd as D
    from distributed_training_amd.compat import colossalai as CA
    from distributed_training_amd.zero import ZeroDataParallel
    from tests._lamb_common import small_model

    model = small_model(CPU)
    opt = CA.DistributedLamb(model.parameters(), lr=0.01, weight_decay=0.01)
    assert isinstance(opt, D.FusedLAMB) and opt.param_groups[0]["adapt"] is True
    with pytest.raises(TypeError, match="nvme_offload"):  # an upstream keyword it does not support
        CA.DistributedLamb(model.parameters(), nvme_offload=True)
    wrapped, wopt = CA.LowLevelZeroPlugin(stage=2, precision="bf16", max_norm=1.0).configure(model, opt, None)
    z = wopt.zero
    assert isinstance(z, ZeroDataParallel) and z.kind == "lamb" and z.dtype == torch.bfloat16 and z.clip == 1.0
    assert z.adapt == [True] * len(z.params) and z.hp["eps"] == 1e-6
    before = [p.detach().clone() for p in z.params]
    x, y = torch.randn(4, 3, 8, 8), torch.randint(0, 10, (4,))
    wopt.backward(nn.functional.cross_entropy(wrapped(x), y))
    assert wopt.step() is True
    assert all(not torch.equal(a, b) for a, b in zip(before, z.params))
    z.close()
    # fp16 brings the dynamic scaler; fp32 none
    m2 = small_model(CPU)
    _, w2 = CA.LowLevelZeroPlugin(stage=1, precision="fp16", initial_scale=2 ** 5).configure(
        m2, CA.DistributedLamb(m2.parameters()), None)
    assert w2.zero.scaler is not None and w2.zero.scaler.scale == 32.0 and w2.zero.kind == "lamb"
    w2.zero.close()
    m3 = small_model(CPU)
    _, w3 = CA.LowLevelZeroPlugin(stage=1, precision="fp32").configure(m3, CA.DistributedLamb(m3.parameters()), None)
    assert w3.zero.scaler is None and w3.zero.dtype == torch.float32
    w3.zero.close()
    # under TorchDDPPlugin it is plain FusedLAMB
    m4 = small_model(CPU)
    o4 = CA.DistributedLamb(m4.parameters(), lr=0.01)
    _, w4 = CA.TorchDDPPlugin().configure(m4, o4, None)
    assert w4.optim is o4


def test_colossalai_distributed_lamb():
    code = ("import sys; sys.path.insert(0, sys.argv[1]);"
            "from colossalai.nn.optimizer import DistributedLamb;"
            "import distributed_training_amd as D;"
            "assert issubclass(DistributedLamb, D.FusedLAMB);"
            "assert 'shims' in sys.modules['colossalai'].__file__")
    subprocess.run([sys.executable, "-c", code, SHIMS], check=True, cwd=REPO)
    _run(_colossal_worker, 2)


def _ctor_worker(rank, ws):
    from distributed_training_amd.zero import ZeroDataParallel

    with pytest.raises(ValueError, match="nope"):
        ZeroDataParallel(Z.model_of("micro"), optimizer="nope")
    for kind in ("lamb", "lars"):
        with pytest.raises(NotImplementedError, match="capture"):
            ZeroDataParallel(Z.model_of("micro"), optimizer=kind, capturable=True)
    with pytest.raises(ValueError, match="adapt"):
        ZeroDataParallel(Z.model_of("micro"), optimizer="lamb", adapt=[True, False])
    z = ZeroDataParallel(Z.model_of("micro"), optimizer="adamw")
    assert z.piece_plan is None
    with pytest.raises(RuntimeError, match="sq_norms"):
        z.sq_norms()
    z.close()


def test_constructor_errors():
    _run(_ctor_worker, 1)
