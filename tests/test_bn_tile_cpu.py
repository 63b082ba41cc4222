"""The geometry of the wide channel tile of the BatchNorm backward passes, without a GPU
(csrc/gs_bn_kernels.hip, bn_geom; tests/test_gpu_bn_tile.py runs the kernels).

1. gs_bn_bwd_partials at every BatchNorm of ResNet-50 x 256 returns what the 8-vector tile returned (the
   values are the parent library's): the workspace, the dx pass's fold and the rows per thread did not move;
2. its bounds at the channel counts of the tile tests;
3. the shapes of tests/test_gpu_bn_tile.py reach the paths they are named for;
4. the exact grid is exact at those shapes, the fork's summed gradient included: any partial sum in any
   order is exact in fp32 and, for R a power of two, so is every step of the dx chain.
"""
import math

import pytest
import torch

from tests import _bn_ref as B
from tests.test_gpu_bn_tile import TILE_C, TILE_SHAPES, tile_inputs


@pytest.fixture(scope="module")
def lib():
    from distributed_training_amd import _lib as L

    return L.lib()


# (R, C) -> P of the parent library: the stem, then layer1 .. layer4 (block outputs: C = 256 .. 2048)
RESNET50_X256_PARTIALS = {
    (256 * 112 * 112, 64): 512,
    (256 * 56 * 56, 64): 512, (256 * 56 * 56, 256): 256,
    (256 * 56 * 56, 128): 512, (256 * 28 * 28, 128): 256, (256 * 28 * 28, 512): 128,
    (256 * 28 * 28, 256): 256, (256 * 14 * 14, 256): 128, (256 * 14 * 14, 1024): 64,
    (256 * 14 * 14, 512): 128, (256 * 7 * 7, 512): 64, (256 * 7 * 7, 2048): 32,
}


@pytest.mark.parametrize("shape", list(RESNET50_X256_PARTIALS), ids=B.shape_id)
def test_partials_at_the_resnet_shapes_are_the_parent_s(lib, shape):
    assert lib.gs_bn_bwd_partials(*shape) == RESNET50_X256_PARTIALS[shape]


@pytest.mark.parametrize("C", TILE_C + [1024, 4096])
@pytest.mark.parametrize("R", [1, 2, 31, 32, 33, 259, 4096, 50176, 802816, 2 ** 31 + 5])
def test_partials_bounds(lib, R, C):
    P = lib.gs_bn_bwd_partials(R, C)
    assert 1 <= P <= 512, P
    assert P <= max(1, math.isqrt(R // 2)), P
    assert P <= -(-R // 32), P  # a row-block has at least one step of ty >= 32 rows
    assert lib.gs_bn_bwd_partials(R, C) == P


def test_shapes_reach_the_paths_they_are_named_for(lib):
    assert lib.gs_bn_bwd_partials(4096, 256) > 8  # more partials than the dx fold has groups (ty / 4 = 8)
    P = lib.gs_bn_bwd_partials(33000, 264)
    rpb = -(-33000 // P)
    assert 2 * 4 * 32 < rpb < 3 * 4 * 32 and rpb % 32  # two unrolled iterations, then a ragged tail step
    for C in TILE_C:
        assert lib.gs_bn_bwd_partials(32, C) == 1 and lib.gs_bn_bwd_partials(259, C) > 1
    # 64 row-blocks of 128 rows (an unrolled step per thread) times two 32-vector tiles: under 256 workgroups
    assert lib.gs_bn_bwd_partials(8192, 512) == 64


@pytest.mark.parametrize("shape", TILE_SHAPES, ids=B.shape_id)
def test_exact_grid_is_exact(shape):
    R, C = shape
    inp = tile_inputs(R, C)
    fork = inp["dy"].double() + inp["dy_b"].double()
    assert torch.equal(fork.to(torch.bfloat16).double(), fork)  # the bf16 sum of the halves is exact
    xc = inp["x"].double() - inp["mean"].double()
    for variant, dy, y in (("plain", inp["dy"], None), ("relu", inp["dy"], inp["y"]),
                           ("fork", fork.to(torch.bfloat16), inp["y"])):
        g, sum_g, sum_gx, gw, _, dx = B.bn_bwd_ref(inp["x"], dy, y, inp["mean"], inp["invstd"], inp["weight"])
        # every term is a multiple of 1/8 and the sums of magnitudes stay below 2^24 / 8
        assert bool(((g * 8) == (g * 8).round()).all()) and bool((((g * xc) * 8) == ((g * xc) * 8).round()).all())
        assert float(g.abs().sum(0).max()) * 8 < 2 ** 24, variant
        assert float((g * xc).abs().sum(0).max()) * 8 < 2 ** 24, variant
        for name, v in (("sum_g", sum_g), ("sum_gx", sum_gx), ("gw", gw)):
            assert bool(B.is_f32(v).all()), (variant, name)
        if R & (R - 1) == 0 and variant != "fork":  # the dx pass is compared bitwise (the fork has none of its own)
            s, w = inp["invstd"].double(), inp["weight"].double()
            m1, k2 = sum_g / R, s * s * sum_gx / R
            d = g - m1
            t = (-xc) * k2 + d
            for name, v in (("a", w * s), ("m1", m1), ("k2", k2), ("g - m1", d), ("fma", t), ("a * fma", w * s * t)):
                assert bool(B.is_f32(v).all()), (variant, name)
            assert bool((w * s * t == dx).all())
