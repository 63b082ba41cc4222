"""Every pack, unpack, sq-norm and clip-scale kernel variant of the chunk engine (gs_engine.h: PackOp,
UnpackOp with its fused Σg² and its fused non-finite check, SqnormOp, ClipScaleOp) on the GPU, bit for
bit against a plain reference, on guarded tensors and a guarded bucket.
tests/test_pack_variants_cpu.py holds the same cases for the host backend.

No tolerance appears here or in tests/_pack_common.py, which says why none is needed.

What the shapes are for: plan alignment 0 leaves most bucket offsets off the 4-element boundary
(the checked path), 64 takes the vector path; a source, destination or bucket pointer one element
off 16 bytes takes the checked path on full chunks too; the group lists end in a group shorter than
the op's (2, 8 or 4 chunks) and let a group straddle two tensors; the large plan has more than 4096
chunks (the one-chunk fp32 pack, the group-sums form of gs_sqnorm_partial_out, the grid-capped
reductions).  The last test repeats a short list of the cases in child processes under the
environment switches that select the non-temporal loads, the combine launch and a grid-stride
reduction."""
import os
import subprocess
import sys

import pytest

from tests import _pack_common as P
from tests._pack_common import BF16, DT_IDS, DTYPES, F16, F32, LIST_A, LIST_B, MODES, PAIR_IDS, PAIRS

pytestmark = pytest.mark.gpu

LISTS = [LIST_A, LIST_B]
LIST_IDS = ["listA", "listB"]
ALIGNS = [0, 64]
ALIGN_IDS = ["align0", "align64"]
OFFS = [0, 1]
OFF_IDS = ["aligned", "off1"]
TRIPLES3 = [(F32, F32, "mul"), (F32, BF16, "div"), (BF16, BF16, "none")]
TRIPLE3_IDS = ["f32-f32-mul", "f32-bf16-div", "bf16-bf16-none"]
# groups of 2 (fp32 bucket, small plan), 8 (fp32 -> 16-bit) and 4 (16-bit -> 16-bit) chunks: a last
# group shorter, and groups that straddle tensors (the virtual space aligns large tensors to 4 Ki)
GROUP_LISTS = [[1024], [3 * 1024], [8 * 1024], [8 * 1024 + 1], [9 * 1024], [4096, 4096, 8192, 12289],
               [4096, 5, 4096, 4095, 8192]]
GROUP_IDS = ["1Ki", "3Ki", "8Ki", "8Ki+1", "9Ki", "straddle", "straddle-tails"]
GROUP_TRIPLES = [(F32, F32, "mul"), (F32, BF16, "div"), (BF16, BF16, "none"), (F16, F16, "mul")]
GROUP_TRIPLE_IDS = ["f32-f32-mul", "f32-bf16-div", "bf16-bf16-none", "f16-f16-mul"]


@pytest.fixture
def dev(cuda_device):
    return cuda_device


# -------------------------------------------------------------------- pack
@pytest.mark.parametrize("align", ALIGNS, ids=ALIGN_IDS)
@pytest.mark.parametrize("numels", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sd,fd", PAIRS, ids=PAIR_IDS)
def test_pack_every_triple(dev, sd, fd, mode, numels, align):
    P.run_pack(dev, numels, sd, fd, mode, align=align)


@pytest.mark.parametrize("numels", [P.OFF_SLOT_NUMELS, LIST_A], ids=["4099", "listA"])
@pytest.mark.parametrize("src_off,flat_off", [(1, 0), (0, 1), (1, 1)], ids=["src-off1", "bucket-off1", "both-off1"])
@pytest.mark.parametrize("sd,fd,mode", TRIPLES3, ids=TRIPLE3_IDS)
def test_pack_off_alignment(dev, sd, fd, mode, src_off, flat_off, numels):
    P.run_pack(dev, numels, sd, fd, mode, align=64, src_off=src_off, flat_off=flat_off)


@pytest.mark.parametrize("align", ALIGNS, ids=ALIGN_IDS)
@pytest.mark.parametrize("numels", GROUP_LISTS, ids=GROUP_IDS)
@pytest.mark.parametrize("sd,fd,mode", GROUP_TRIPLES, ids=GROUP_TRIPLE_IDS)
def test_pack_groups(dev, sd, fd, mode, numels, align):
    P.run_pack(dev, numels, sd, fd, mode, align=align)


@pytest.mark.parametrize("sd,fd,mode", [(F32, F32, "mul"), (BF16, F32, "none")], ids=["f32-f32-mul", "bf16-f32-none"])
def test_pack_large_plan_one_chunk_groups(dev, sd, fd, mode):
    """more than kPackG2MaxChunks chunks (asserted from the numels beside P.LARGE): an fp32 bucket
    takes the GS_G_PACK = 1 instantiation"""
    P.run_pack(dev, P.LARGE, sd, fd, mode, align=64)


@pytest.mark.parametrize("align", ALIGNS, ids=ALIGN_IDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sd,fd", PAIRS, ids=PAIR_IDS)
def test_pack_special_values(dev, sd, fd, mode, align):
    P.run_pack(dev, P.SPECIAL_NUMELS, sd, fd, mode, align=align)


# ------------------------------------------------------------------ unpack
@pytest.mark.parametrize("sqnorm", [False, True], ids=["random", "sqnorm-ints"])
@pytest.mark.parametrize("align", ALIGNS, ids=ALIGN_IDS)
@pytest.mark.parametrize("numels", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("fd,dd", PAIRS, ids=PAIR_IDS)
def test_unpack_every_pair(dev, fd, dd, numels, align, sqnorm):
    P.run_unpack(dev, numels, fd, dd, align=align, sqnorm=sqnorm)


@pytest.mark.parametrize("numels", [P.OFF_SLOT_NUMELS, LIST_A], ids=["4099", "listA"])
@pytest.mark.parametrize("dst_off,flat_off", [(1, 0), (0, 1), (1, 1)], ids=["dst-off1", "bucket-off1", "both-off1"])
@pytest.mark.parametrize("fd", [F32, BF16], ids=["f32", "bf16"])
def test_unpack_off_alignment(dev, fd, dst_off, flat_off, numels):
    P.run_unpack(dev, numels, fd, F32, align=64, dst_off=dst_off, flat_off=flat_off, sqnorm=True)


@pytest.mark.parametrize("align", ALIGNS, ids=ALIGN_IDS)
@pytest.mark.parametrize("fd,dd", PAIRS, ids=PAIR_IDS)
def test_unpack_special_values(dev, fd, dd, align):
    P.run_unpack(dev, P.SPECIAL_NUMELS, fd, dd, align=align)


def test_unpack_large_plan_exact_sqnorm(dev):
    P.run_unpack(dev, P.LARGE, F32, F32, align=64, sqnorm=True, vmax=1)


# ------------------------------------------------------------ unpack check
@pytest.mark.parametrize("align", ALIGNS, ids=ALIGN_IDS)
@pytest.mark.parametrize("numels", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("fd,dd", PAIRS, ids=PAIR_IDS)
def test_unpack_check_clean_and_nan_padding(dev, fd, dd, numels, align):
    P.run_unpack_check(dev, numels, fd, dd, align=align)


@pytest.mark.parametrize("align", ALIGNS, ids=ALIGN_IDS)
@pytest.mark.parametrize("numels", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("fd,dd", PAIRS, ids=PAIR_IDS)
def test_unpack_check_nonfinite_at_tensor_edges(dev, fd, dd, numels, align):
    P.run_unpack_check(dev, numels, fd, dd, align=align, nonfinite=True)


@pytest.mark.parametrize("fd", [F32, BF16], ids=["f32", "bf16"])
def test_unpack_check_f16_overflow_sets_the_flag(dev, fd):
    P.run_unpack_check_f16_overflow(dev, fd)


# ------------------------------------------------------------------ sqnorm
@pytest.mark.parametrize("numels", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("off", OFFS, ids=OFF_IDS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_sqnorm_exact(dev, dt, off, numels):
    """both lists are small plans: gs_sqnorm_partial_out takes the raw form, one partial per
    workgroup, and LIST_A has chunks enough for several"""
    n = P.run_sqnorm_exact(dev, numels, dt, off)
    assert numels is not LIST_A or n > 1, n


@pytest.mark.parametrize("numels", [[], [0, 0]], ids=["no-tensors", "empty-tensors"])
def test_sqnorm_exact_empty_plan(dev, numels):
    P.run_sqnorm_empty(dev, numels)


def test_sqnorm_large_plan_group_sums(dev):
    """more than 4096 chunks: gs_sqnorm_partial_out returns the fused reduction's group sums"""
    from distributed_training_amd import _lib as L

    n = P.run_sqnorm_exact(dev, P.LARGE, F32, 0, vmax=1)
    assert n <= L.GS_RED_GROUPS, n  # the raw form would return one partial per workgroup


# -------------------------------------------------------------- clip-scale
@pytest.mark.parametrize("sq", [P.SQ_CLIPS, P.SQ_COEF_ONE], ids=["clip", "coef1"])
@pytest.mark.parametrize("off", OFFS, ids=OFF_IDS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_clip_scale(dev, dt, off, sq):
    P.run_clip_scale(dev, LIST_A, dt, off, sq)


@pytest.mark.parametrize("sq", [P.SQ_CLIPS, P.SQ_COEF_ONE], ids=["clip", "coef1"])
@pytest.mark.parametrize("off", OFFS, ids=OFF_IDS)
def test_clip_scale_tiny_tensors(dev, off, sq):
    P.run_clip_scale(dev, LIST_B, F32, off, sq)


# -------------------------------------------------------------- NULL slots
@pytest.mark.parametrize("align", ALIGNS, ids=ALIGN_IDS)
@pytest.mark.parametrize("case", ["pack-mul", "pack-div", "unpack-sqnorm", "unpack-check"])
def test_null_slots(dev, case, align):
    if case.startswith("pack"):
        P.run_pack(dev, LIST_A, F32, BF16, case[5:], align=align, null=P.NULL_A)
    elif case == "unpack-sqnorm":
        P.run_unpack(dev, LIST_A, BF16, F32, align=align, sqnorm=True, null=P.NULL_A)
    else:
        P.run_unpack_check(dev, LIST_A, BF16, F32, align=align, null=P.NULL_A)


# ------------------------------------------------- the environment switches
_POLICY_CHILD = r"""
import sys, torch
sys.path.insert(0, {repo!r})
from tests import _pack_common as P
P.run_policy_suite(torch.device("cuda", 0))
print("OK")
"""
POLICIES = [{"GS_NT_READ_ONCE": "1", "GS_NT_SQNORM": "1"}, {"GS_RED_FUSE": "0"}, {"GS_RED_GRID": "3"}]


@pytest.mark.parametrize("env", POLICIES, ids=["non-temporal", "combine-launch", "grid3"])
def test_policy_children(env):
    """The load policy and the reduction form are read from the environment once per process, so
    each setting gets a fresh child, which runs P.run_policy_suite on cuda:0 and prints OK.
    GS_NT_READ_ONCE = GS_NT_SQNORM = 1 selects every non-temporal instantiation of pack, unpack,
    sq-norm and clip-scale at these small sizes; GS_RED_FUSE = 0 the combine launch behind the
    unpack's reductions and gs_sqnorm; GS_RED_GRID = 3 grid-stride reductions over three partials.
    Which instantiation a setting selects rests on nt_read_once() and launch() as written
    (gs_engine.h): the test cannot observe it, only that no setting changes a bit."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _POLICY_CHILD.format(repo=repo)], env={**os.environ, **env},
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
