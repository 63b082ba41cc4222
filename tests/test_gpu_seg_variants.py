"""Every LARS and LAMB kernel variant of the chunk engine on the GPU — seg_sum_kernel with LarsLanes
and LambLanes through seg_full, seg_mixed, seg_load and seg_store (gs_update_kernels.hip),
lars_norm_finish, LarsOp and LambOp (gs_engine.h) — bit for bit against the numpy fp32
restatements of tests/_lars_common.py and tests/_lamb_common.py, on guarded tensors.
tests/test_seg_variants_cpu.py holds the same cases for the host backend.

No tolerance appears here; tests/_seg_common.py says why none is needed (element-wise results
against the restatement fed the published sums; sums on exact-sum inputs only) and which path
stays unreached (the grid-stride loop of seg_sum_kernel, above 2^28 elements).

What is launched:
  * LarsLanes<f32 | bf16 | f16>: test_lars_norms_exact (every list, four alignments of p and g).
  * LambLanes<f32 | bf16 | f16>: test_lamb_moments_exact and test_lamb_moments_random (every list;
    no slot, or one of the four, off 16 bytes).
  * LarsOp: test_lars_every_pair_both_grad_loads runs the (gdt, ldt) product, 3 x 3, and each case
    launches both grad-load arms — NTG = false right behind this plan's gs_lars_norms, NTG = true
    on a fresh plan handed another plan's sums — all 18 instantiations.
  * LambOp<none | bf16 | f16>: test_lamb_every_lowp, all 3 instantiations, with slot 1 (the
    grads) unbound for the update pass, which the library allows.
  * lars_norm_finish beyond one pass of its loop: test_fold_depth_* and
    test_repeatable_at_fold_depth (255 to 2049 partial slots per tensor)."""
import math

import pytest

from tests import _seg_common as S
from tests._seg_common import BF16, DT_IDS, DTYPES, F16, F32, LIST_B, LOWP_IDS, LOWPS

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev(cuda_device):
    return cuda_device


LIST_IDS = list(S.LISTS)
ALIGN = {"aligned": (0, 0), "p-off": (1, 0), "g-off": (0, 1), "both-off": (1, 1)}
PAIRS2 = [(F32, None), (BF16, BF16)]
PAIR2_IDS = ["f32-none", "bf16-bf16"]
GSCALES = [None, 0.37]
GSCALE_IDS = ["noscale", "scale0.37"]


# ------------------------------------------------------- A. gs_lars_norms
@pytest.mark.parametrize("align", list(ALIGN))
@pytest.mark.parametrize("name", LIST_IDS)
@pytest.mark.parametrize("gdt", DTYPES, ids=DT_IDS)
def test_lars_norms_exact(dev, gdt, name, align):
    S.assert_span_layout()
    S.run_lars_norms(dev, S.LISTS[name], gdt, *ALIGN[align])


# ----------------------------------------------------- B. gs_lamb_moments
@pytest.mark.parametrize("grad_scale", [None, 0.5], ids=["noscale", "scale0.5"])
@pytest.mark.parametrize("name", LIST_IDS)
@pytest.mark.parametrize("gdt", DTYPES, ids=DT_IDS)
def test_lamb_moments_exact(dev, gdt, name, grad_scale):
    S.assert_span_layout()
    S.run_lamb_exact(dev, S.LISTS[name], gdt, grad_scale=grad_scale)


@pytest.mark.parametrize("slot", [0, 1, 2, 3])
@pytest.mark.parametrize("name", LIST_IDS + ["off"])
def test_lamb_moments_exact_one_slot_off_alignment(dev, name, slot):
    S.run_lamb_exact(dev, S.OFF_NUMELS if name == "off" else S.LISTS[name], BF16, off_slot=slot,
                     grad_scale=0.5 if slot % 2 else None)


@pytest.mark.parametrize("slot", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("name", LIST_IDS + ["off"])
@pytest.mark.parametrize("gdt", DTYPES, ids=DT_IDS)
def test_lamb_moments_random(dev, gdt, name, slot):
    S.run_lamb(dev, S.OFF_NUMELS if name == "off" else S.LISTS[name], gdt, off_slot=slot, grad_scale=0.37,
               do_step=False)


@pytest.mark.parametrize("slot", [None, 1, 3])
@pytest.mark.parametrize("gdt", DTYPES, ids=DT_IDS)
def test_lamb_found_inf_changes_nothing(dev, gdt, slot):
    S.run_lamb_found_inf(dev, S.LIST_C if slot is None else S.OFF_NUMELS, gdt, F16, off_slot=slot)


# -------------------------------------- C. gs_lars_step / gs_lars_step_lowp
@pytest.mark.parametrize("name", ["listC", "listB"])
@pytest.mark.parametrize("ldt", LOWPS, ids=LOWP_IDS)
@pytest.mark.parametrize("gdt", DTYPES, ids=DT_IDS)
def test_lars_every_pair_both_grad_loads(dev, gdt, ldt, name):
    if name == "listC":
        S.run_lars(dev, S.LIST_C, gdt, ldt, adapt=S.ADAPT_C, zero_p=[S.C_ZERO_P], zero_g=[S.C_ZERO_G])
    else:
        S.run_lars(dev, LIST_B, gdt, ldt)


@pytest.mark.parametrize("mom", [0.9, 0.0], ids=["momentum", "momentum0"])
@pytest.mark.parametrize("wd", [1e-4, 0.0], ids=["wd", "wd0"])
@pytest.mark.parametrize("grad_scale", GSCALES, ids=GSCALE_IDS)
@pytest.mark.parametrize("gdt,ldt", PAIRS2, ids=PAIR2_IDS)
def test_lars_momentum_decay_scale(dev, gdt, ldt, grad_scale, wd, mom):
    S.run_lars(dev, S.LIST_C, gdt, ldt, mom=mom, wd=wd, grad_scale=grad_scale, adapt=S.ADAPT_C,
               zero_p=[S.C_ZERO_P], zero_g=[S.C_ZERO_G])


@pytest.mark.parametrize("mom", [0.9, 0.0], ids=["momentum", "momentum0"])
@pytest.mark.parametrize("slot", [0, 1, 2, 3])
@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
def test_lars_one_slot_off_alignment(dev, gdt, slot, mom):
    S.run_lars(dev, S.OFF_NUMELS, gdt, BF16, off_slot=slot, mom=mom)


@pytest.mark.parametrize("mom", [0.9, 0.0], ids=["momentum", "momentum0"])
def test_lars_found_inf_changes_nothing(dev, mom):
    S.run_lars(dev, S.LIST_C, BF16, F16, mom=mom, grad_scale=0.37, found_inf=1.0, adapt=S.ADAPT_C)


@pytest.mark.parametrize("name", LIST_IDS)
@pytest.mark.parametrize("gdt,ldt", PAIRS2, ids=PAIR2_IDS)
def test_lars_exact_step(dev, gdt, ldt, name):
    S.run_lars(dev, S.LISTS[name], gdt, ldt, exact=True)


# -------------------------------------- D. gs_lamb_step / gs_lamb_step_lowp
@pytest.mark.parametrize("wd", [0.01, 0.0], ids=["wd", "wd0"])
@pytest.mark.parametrize("name", ["listC", "listB"])
@pytest.mark.parametrize("ldt", LOWPS, ids=LOWP_IDS)
def test_lamb_every_lowp(dev, ldt, name, wd):
    hp = dict(S.RANDOM_HP, wd=wd)
    if name == "listC":
        S.run_lamb(dev, S.LIST_C, BF16, ldt, hp=hp, adapt=S.ADAPT_C, zero_p=[S.C_ZERO_P], zero_g=[S.C_ZERO_G])
    else:
        S.run_lamb(dev, LIST_B, F32, ldt, hp=hp)


@pytest.mark.parametrize("slot", [0, 2, 3, 4])
@pytest.mark.parametrize("ldt", [BF16, F16], ids=["bf16", "f16"])
def test_lamb_one_slot_off_alignment(dev, ldt, slot):
    S.run_lamb(dev, S.OFF_NUMELS, F32, ldt, off_slot=slot)


@pytest.mark.parametrize("side,lo,hi", [("lo", 50.0, math.inf), ("hi", 0.0, 1e-3), ("lo", 1.0, 1.0)],
                         ids=["below", "above", "pinned"])
def test_lamb_clamp(dev, side, lo, hi):
    S.run_lamb(dev, S.LIST_C, F32, BF16, adapt=S.ADAPT_C, zero_p=[S.C_ZERO_P], zero_g=[S.C_ZERO_G], lo=lo, hi=hi,
               clamped=side)


@pytest.mark.parametrize("name", LIST_IDS)
@pytest.mark.parametrize("ldt", [None, F16], ids=["none", "f16"])
def test_lamb_exact_step(dev, ldt, name):
    S.run_lamb_exact(dev, S.LISTS[name], F16, ldt=ldt, do_step=True)


# ------------------------------------------------------ E. special values
@pytest.mark.parametrize("mom", [0.9, 0.0], ids=["momentum", "momentum0"])
@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])  # fp16 holds neither 1e-40 nor 3e38
def test_lars_special_values(dev, gdt, mom):
    S.run_lars(dev, S.SPECIAL_NUMELS, gdt, BF16, mom=mom, special=True)


@pytest.mark.parametrize("eps", [0.0, 1e-6], ids=["eps0", "eps1e-6"])
@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])  # fp16 holds neither 1e-40 nor 3e38
def test_lamb_special_values(dev, gdt, eps):
    S.run_lamb(dev, S.SPECIAL_NUMELS, gdt, BF16, hp=dict(S.RANDOM_HP, eps=eps),
               inputs=S.lamb_special_inputs(tuple(S.SPECIAL_NUMELS), gdt))


# ---------------------------------------------------------- G. fold depth
@pytest.mark.parametrize("sparse", [False, True], ids=["grid", "one-per-chunk"])
def test_fold_depth_lars(dev, sparse):
    S.run_fold_lars(dev, BF16, sparse)


@pytest.mark.parametrize("sparse", [False, True], ids=["grid", "one-per-chunk"])
def test_fold_depth_lamb(dev, sparse):
    S.run_fold_lamb(dev, F32, sparse)


# ----------------------------------------------------- H. degenerate plans
@pytest.mark.parametrize("numels", [[], [0, 0], [1], [4096], [4097]],
                         ids=["no-tensors", "empty-tensors", "one-element", "one-group", "one-group+1"])
def test_degenerate_plans(dev, numels):
    S.run_degenerate(dev, numels)


# ------------------------------------------------- I. hyper source, eager
@pytest.mark.parametrize("gdt,ldt", PAIRS2, ids=PAIR2_IDS)
def test_lars_hyper_source(dev, gdt, ldt):
    S.run_lars_hyper(dev, S.LIST_C, gdt, ldt)


@pytest.mark.parametrize("gdt,ldt", PAIRS2, ids=PAIR2_IDS)
def test_lamb_hyper_source(dev, gdt, ldt):
    S.run_lamb_hyper(dev, S.LIST_C, gdt, ldt)


# ------------------------------------------------ J. repeatability at depth
def test_repeatable_at_fold_depth(dev):
    S.run_repeat_at_depth(dev)
