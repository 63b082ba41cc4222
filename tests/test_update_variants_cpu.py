"""Every SGD, Adam, scale, sum and unscale variant of the host backend (gs_host.cpp: host_sgd,
host_adam, host_scale, host_sum, host_unscale_check), bit for bit against a plain reference, on
guarded tensors.  The cases are those of tests/test_gpu_update_variants.py, which runs them on the
HIP kernels; this file runs anywhere, and keeps the two backends on one contract.

No tolerance appears here or in tests/_update_common.py, which says why none is needed: the oracle
restates the backends' fp32 expression without contraction, every 16-bit store is one
round-to-nearest-even cast of the stored fp32 value, and gs_sum's integer inputs are bounded so
that the sum is exact in any order.

``cached=True`` (a Σg² pass before the update) only chooses between two load instructions on the
GPU; here it checks that the pass leaves the grads and the update alone."""
import pytest

from tests import _update_common as U
from tests._update_common import BF16, DT_IDS, DTYPES, F16, F32, LIST_A, LIST_B, LOWP_IDS, LOWPS

LISTS = [LIST_A, LIST_B]
LIST_IDS = ["listA", "listB"]
PAIRS2 = [(F32, None), (BF16, BF16)]
PAIR2_IDS = ["f32-none", "bf16-bf16"]
GSCALES = [None, 0.37]
GSCALE_IDS = ["noscale", "scale0.37"]
ADAM_KINDS = {"adamw": dict(), "l2": dict(adamw=False, wd=3e-7)}
SGD_KINDS = {"momentum": dict(), "nesterov": dict(nesterov=True), "first": dict(first=True),
             "momentum0": dict(momentum=0.0)}


@pytest.fixture
def dev():
    import torch

    return torch.device("cpu")


# -------------------------------------------------------------------- Adam
@pytest.mark.parametrize("numels", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("ldt", LOWPS, ids=LOWP_IDS)
@pytest.mark.parametrize("gdt", DTYPES, ids=DT_IDS)
def test_adam_every_pair(dev, gdt, ldt, numels):
    U.run_adam(dev, numels, gdt, ldt)


@pytest.mark.parametrize("ldt", LOWPS, ids=LOWP_IDS)
@pytest.mark.parametrize("gdt", DTYPES, ids=DT_IDS)
def test_adam_cached_grad_loads(dev, gdt, ldt):
    U.run_adam(dev, LIST_A, gdt, ldt, cached=True)


@pytest.mark.parametrize("numels", U.GROUPS_ADAM, ids=U.GROUP_IDS[:3])
@pytest.mark.parametrize("gdt,ldt", PAIRS2, ids=PAIR2_IDS)
def test_adam_last_group_shorter(dev, gdt, ldt, numels):
    U.run_adam(dev, numels, gdt, ldt)


@pytest.mark.parametrize("slot", [0, 1, 2, 3, 4])
def test_adam_one_slot_off_alignment(dev, slot):
    U.run_adam(dev, U.OFF_SLOT_NUMELS, F32, BF16, off_slot=slot)


@pytest.mark.parametrize("kind", list(ADAM_KINDS))
@pytest.mark.parametrize("grad_scale", GSCALES, ids=GSCALE_IDS)
@pytest.mark.parametrize("gdt", DTYPES, ids=DT_IDS)
def test_adam_maximize(dev, gdt, grad_scale, kind):
    U.run_adam(dev, LIST_A, gdt, BF16, maximize=True, grad_scale=grad_scale, **ADAM_KINDS[kind])


def test_adam_found_inf_changes_nothing(dev):
    U.run_adam(dev, LIST_A, BF16, F16, found_inf=1.0)


@pytest.mark.parametrize("gdt,ldt", PAIRS2, ids=PAIR2_IDS)
def test_adam_hyper_source(dev, gdt, ldt):
    U.run_adam(dev, LIST_A, gdt, ldt, hyper=True)


@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
def test_adam_special_values(dev, gdt):
    U.run_adam(dev, U.SPECIAL_NUMELS, gdt, BF16, special=True)


# --------------------------------------------------------------------- SGD
@pytest.mark.parametrize("numels", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("ldt", LOWPS, ids=LOWP_IDS)
@pytest.mark.parametrize("gdt", DTYPES, ids=DT_IDS)
def test_sgd_every_pair(dev, gdt, ldt, numels):
    U.run_sgd(dev, numels, gdt, ldt)


@pytest.mark.parametrize("ldt", LOWPS, ids=LOWP_IDS)
@pytest.mark.parametrize("gdt", DTYPES, ids=DT_IDS)
def test_sgd_cached_grad_loads(dev, gdt, ldt):
    U.run_sgd(dev, LIST_A, gdt, ldt, cached=True)


@pytest.mark.parametrize("numels", U.GROUPS_SGD, ids=U.GROUP_IDS)
@pytest.mark.parametrize("gdt,ldt", PAIRS2, ids=PAIR2_IDS)
def test_sgd_last_group_shorter(dev, gdt, ldt, numels):
    U.run_sgd(dev, numels, gdt, ldt)


@pytest.mark.parametrize("slot", [0, 1, 2, 3])
def test_sgd_one_slot_off_alignment(dev, slot):
    U.run_sgd(dev, U.OFF_SLOT_NUMELS, F32, BF16, off_slot=slot)


@pytest.mark.parametrize("kind", list(SGD_KINDS))
@pytest.mark.parametrize("grad_scale", GSCALES, ids=GSCALE_IDS)
@pytest.mark.parametrize("gdt", DTYPES, ids=DT_IDS)
def test_sgd_maximize(dev, gdt, grad_scale, kind):
    U.run_sgd(dev, LIST_A, gdt, BF16, maximize=True, grad_scale=grad_scale, **SGD_KINDS[kind])


def test_sgd_found_inf_changes_nothing(dev):
    U.run_sgd(dev, LIST_A, BF16, F16, found_inf=1.0)


@pytest.mark.parametrize("gdt,ldt", PAIRS2, ids=PAIR2_IDS)
def test_sgd_hyper_source(dev, gdt, ldt):
    U.run_sgd(dev, LIST_A, gdt, ldt, hyper=True)


@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
def test_sgd_special_values(dev, gdt):
    U.run_sgd(dev, U.SPECIAL_NUMELS, gdt, BF16, special=True)


# ------------------------------------------------------------------- scale
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("numels", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("mode,s", U.SCALES, ids=U.SCALE_IDS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_scale(dev, dt, mode, s, numels, off):
    U.run_scale(dev, numels, dt, mode, s, off)


# --------------------------------------------------------------------- sum
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("numels", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_sum(dev, dt, numels, off):
    U.run_sum(dev, numels, dt, off)


@pytest.mark.parametrize("numels", [[], [0, 0]], ids=["no-tensors", "empty-tensors"])
def test_sum_empty_plan(dev, numels):
    U.run_sum_empty(dev, numels)


# ----------------------------------------------------------------- unscale
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("numels", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_unscale_clean_and_flag_accumulates(dev, dt, numels, off):
    U.run_unscale(dev, numels, dt, off)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("numels", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_unscale_nonfinite_at_tensor_edges(dev, dt, numels, off):
    U.run_unscale(dev, numels, dt, off, nonfinite=True)


@pytest.mark.parametrize("inv", [None, 1.0], ids=["no-inv", "inv1"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_unscale_writes_nothing(dev, dt, off, inv):
    U.run_unscale_no_write(dev, dt, off, inv)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
def test_unscale_f16_overflow_is_not_an_inf_grad(dev, off):
    U.run_unscale_f16_overflow(dev, off)
