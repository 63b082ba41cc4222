"""MixUp / CutMix in the input step without a GPU: ``MixUpCutMix``'s draws against a restatement of the order its
docstring states, the box invariants, gs_image_augment_mix on the host backend bit for bit against the numpy
restatement of its contract (tests/_mix_ref.py), the loader with mixing off, and the argument checks."""
import numpy as np
import pytest
import torch

from distributed_training_amd import _lib as L
from distributed_training_amd import data as D
from oracle import input_pipeline as R
from tests import _mix_ref as M

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    return L.lib()


# ---- the draws -------------------------------------------------------------------------------------------------
def restated_records(rng, B, oh, ow, mixup_alpha, cutmix_alpha, prob, switch_prob, mode):
    """MixUpCutMix.records restated from the class's docstring, sample by sample"""
    ident = [M.record(i, 1.0) for i in range(B)]

    def choose_cut(u):
        return u < switch_prob if (mixup_alpha > 0 and cutmix_alpha > 0) else cutmix_alpha > 0

    def one(i, partner, cut, lam, cy, cx):
        if not cut:
            return M.record(partner, np.float32(lam))
        r = np.sqrt(1.0 - lam)
        ch, cw = int(oh * r), int(ow * r)
        y0, y1 = int(np.clip(cy - ch // 2, 0, oh)), int(np.clip(cy + ch // 2, 0, oh))
        x0, x1 = int(np.clip(cx - cw // 2, 0, ow)), int(np.clip(cx + cw // 2, 0, ow))
        if (y1 - y0) * (x1 - x0) == 0:
            return ident[i]
        return M.record(partner, np.float32(1.0 - (y1 - y0) * (x1 - x0) / (oh * ow)), (y0, y1, x0, x1))

    if mode == "batch":
        u_apply = rng.random()
        u_switch = rng.random()
        if u_apply >= prob:
            return np.asarray(ident, dtype=np.int32).reshape(B, 4)
        cut = choose_cut(u_switch)
        alpha = cutmix_alpha if cut else mixup_alpha
        lam = rng.beta(alpha, alpha)
        cy = cx = None
        if cut:
            cy = rng.integers(oh)
            cx = rng.integers(ow)
        perm = rng.permutation(B)
        rec = [one(i, int(perm[i]), cut, lam, cy, cx) for i in range(B)]
    else:
        u_apply = rng.random(B)
        u_switch = rng.random(B)
        apply = u_apply < prob
        cut = [bool(apply[i] and choose_cut(u_switch[i])) for i in range(B)]
        alpha = np.asarray([1.0 if not apply[i] else cutmix_alpha if cut[i] else mixup_alpha for i in range(B)])
        lam = rng.beta(alpha, alpha)
        cy = cx = np.zeros(B, dtype=np.int64)
        if cutmix_alpha > 0:
            cy = rng.integers(oh, size=B)
            cx = rng.integers(ow, size=B)
        perm = rng.permutation(B)
        rec = [one(i, int(perm[i]), cut[i], lam[i], cy[i], cx[i]) if apply[i] else ident[i] for i in range(B)]
    return np.asarray(rec, dtype=np.int32).reshape(B, 4)


@pytest.mark.parametrize("mode", ["batch", "elem"])
@pytest.mark.parametrize("alphas", [(0.8, 0.0), (0.0, 1.0), (0.4, 1.0)], ids=["mixup", "cutmix", "both"])
@pytest.mark.parametrize("prob", [0.0, 0.5, 1.0])
def test_draw_order(mode, alphas, prob):
    for B in (1, 3, 100):
        mix = D.MixUpCutMix(*alphas, prob=prob, switch_prob=0.4, mode=mode, seed=5, rank=2)
        rng = np.random.Generator(np.random.PCG64([5, 2]))
        kinds = set()
        for _ in range(20):
            got = mix.records(B, 32, 28)
            want = restated_records(rng, B, 32, 28, *alphas, prob, 0.4, mode)
            assert got.dtype == np.int32 and got.shape == (B, 4)
            assert np.array_equal(got, want)
            for row in got:
                _, lam, (y0, y1, x0, x1) = M.decode(row)
                kinds.add("box" if y1 > y0 else "blend" if lam != 1 else "identity")
        if prob == 0.0:
            assert kinds == {"identity"}
        elif prob == 1.0 and B == 100:
            assert ("blend" in kinds) == (alphas[0] > 0) and ("box" in kinds) == (alphas[1] > 0)


def test_box_invariants():
    for mode in ("batch", "elem"):
        mix = D.MixUpCutMix(0.0, 1.0, mode=mode, seed=1)
        n_box = 0
        for oh, ow in ((32, 32), (7, 50), (1, 1)):
            for _ in range(30):
                for i, row in enumerate(mix.records(16, oh, ow)):
                    partner, lam, (y0, y1, x0, x1) = M.decode(row)
                    assert 0 <= partner < 16 and 0 <= y0 <= y1 <= oh and 0 <= x0 <= x1 <= ow
                    if y1 > y0:
                        assert x1 > x0
                        assert lam == np.float32(1.0 - (y1 - y0) * (x1 - x0) / (oh * ow)) and 0.0 <= lam < 1.0
                        n_box += 1
                    else:
                        assert (partner, lam, x0, x1) == (i, 1.0, 0, 0)
        assert n_box > 100


def test_state_dict_round_trip_and_rank_streams():
    a = D.MixUpCutMix(0.4, 1.0, mode="elem", seed=9, rank=0)
    for _ in range(3):
        a.records(8, 32, 32)
    state = a.state_dict()
    want = [a.records(8, 32, 32) for _ in range(4)]
    b = D.MixUpCutMix(0.4, 1.0, mode="elem", seed=123, rank=5)
    b.load_state_dict(state)
    assert all(np.array_equal(b.records(8, 32, 32), w) for w in want)
    r0, r1 = D.MixUpCutMix(0.4, seed=9, rank=0), D.MixUpCutMix(0.4, seed=9, rank=1)
    assert not np.array_equal(r0.records(64, 32, 32), r1.records(64, 32, 32))
    assert D.MixUpCutMix(0.4, seed=9).rank == 0  # no process group: rank 0
    with pytest.raises(ValueError):
        D.MixUpCutMix()
    with pytest.raises(ValueError):
        D.MixUpCutMix(0.0, 0.0, prob=0.5)


# ---- the images, bit for bit -----------------------------------------------------------------------------------
_BASE = {}


def base_case(lib, geometry, records):
    """(imgs, labels, params, rec, unmixed fp32 batch, its labels), computed once per case and left unchanged"""
    key = (geometry, records)
    if key not in _BASE:
        H, W, pad, crop = M.GEOMETRIES[geometry]
        if records == "handmade":
            rec = M.handmade_records(crop, crop)
        else:
            rec = M.random_records(int(records), crop, crop, seed=int(records))
        imgs, labels, params = M.image_case(geometry, rec.shape[0], seed=len(geometry) + rec.shape[0])
        base, lab = M.unmixed_batch(lib, imgs, labels, params, geometry)
        _BASE[key] = (imgs, labels, params, rec, base, lab)
    return _BASE[key]


def check_images(lib, geometry, records, dtype, channels_last, device=None):
    imgs, labels, params, rec, base, lab = base_case(lib, geometry, records)
    want, want_b, want_lam = M.mix_images_ref(base, lab, rec, dtype)
    rc, got, la, lb, lam, _ = M.run_augment_mix(lib, imgs, labels, params, rec, geometry, dtype, channels_last, device)
    assert rc == 0, lib.gs_last_error()
    assert M.same_bits(got, want)
    assert torch.equal(la, lab) and torch.equal(lb, want_b) and M.same_bits(lam, want_lam)
    return got


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("geometry", list(M.GEOMETRIES))
def test_images_bit_for_bit(lib, geometry, dtype, channels_last):
    got = check_images(lib, geometry, "handmade", dtype, channels_last)
    base = base_case(lib, geometry, "handmade")[4]
    # the records did something: the blends and pastes differ from the unmixed batch, the identities do not
    changed = [not torch.equal(got[i], base[i].to(dtype)) for i in range(got.shape[0])]
    assert changed == [True] * 4 + [False] + [True] * 7 + [False, False]
    assert torch.equal(got[5], base[6].to(dtype))  # the full-image box is the partner's image
    check_images(lib, geometry, "3", dtype, channels_last)


# ---- off means off ---------------------------------------------------------------------------------------------
def _images(n=103, seed=0):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8), g.integers(0, 10, n)


def test_prob_zero_equals_no_mix_and_leaves_torch_rng_alone():
    imgs, labels = _images()
    ds = D.ImageDataset(imgs, labels, "cpu")
    runs = []
    for mix in (None, D.MixUpCutMix(0.4, 1.0, prob=0.0)):
        ld = D.DeviceDataLoader(ds, batch_size=10, drop_last=True, transform=D.TRAIN_TRANSFORM, mix=mix,
                                sampler=D.DistributedSampler(ds, num_replicas=2, rank=1))
        torch.manual_seed(31)
        runs.append(([(x.clone(), t) for x, t in ld], torch.get_rng_state()))
    (plain, st_plain), (mixed, st_mixed) = runs
    assert torch.equal(st_plain, st_mixed)
    assert len(plain) == len(mixed) == 5
    for (px, py), (mx, mt) in zip(plain, mixed):
        assert isinstance(mt, D.MixedTarget) and not isinstance(py, D.MixedTarget)
        assert M.same_bits(px, mx) and torch.equal(py, mt.labels_a) and torch.equal(py, mt.labels_b)
        assert mt.lam.dtype == torch.float32 and bool((mt.lam == 1).all())


def test_no_mix_loader_equals_reference_pipeline():
    imgs, labels = _images()
    ref = R.reference_loader(imgs, labels, 10, 2, 1, train=True, drop_last=True)
    ds = D.ImageDataset(imgs, labels, "cpu")
    mine = D.DeviceDataLoader(ds, batch_size=10, shuffle=False, drop_last=True, mix=None,
                              sampler=D.DistributedSampler(ds, num_replicas=2, rank=1), transform=D.TRAIN_TRANSFORM)
    torch.manual_seed(100)
    want = [(x.clone(), y.clone()) for x, y in ref]
    st_ref = torch.get_rng_state()
    torch.manual_seed(100)
    got = [(x.clone(), y.clone()) for x, y in mine]
    assert torch.equal(torch.get_rng_state(), st_ref) and len(got) == len(want) == 5
    for (gx, gy), (wx, wy) in zip(got, want):
        assert torch.equal(gx, wx) and torch.equal(gy, wy)


def test_mixing_loader_applies_its_records():
    """one epoch with mixing on: every batch is the numpy restatement applied to the unmixed loader's batch with the
    records a second generator in the same state draws"""
    imgs, labels = _images(64, seed=2)
    ds = D.ImageDataset(imgs, labels, "cpu")
    kw = dict(batch_size=16, drop_last=True, transform=D.TRAIN_TRANSFORM)
    twin = D.MixUpCutMix(0.4, 1.0, mode="elem", seed=4)
    torch.manual_seed(8)
    plain = [(x.clone(), y.clone()) for x, y in D.DeviceDataLoader(ds, **kw)]
    torch.manual_seed(8)
    mixed = list(D.DeviceDataLoader(ds, mix=D.MixUpCutMix(0.4, 1.0, mode="elem", seed=4), **kw))
    differs = 0
    for (px, py), (mx, mt) in zip(plain, mixed):
        want, want_b, want_lam = M.mix_images_ref(px, py, twin.records(16, 32, 32), torch.float32)
        assert M.same_bits(mx, want) and torch.equal(mt.labels_a, py) and torch.equal(mt.labels_b, want_b)
        assert M.same_bits(mt.lam, want_lam)
        differs += not torch.equal(mx, px)
    assert differs == len(plain) == 4


# ---- the argument checks ---------------------------------------------------------------------------------------
BAD_RECORDS = {
    "partner-high": M.record(3, 0.5), "partner-negative": M.record(-1, 0.5), "lam-above-1": M.record(1, 1.5),
    "lam-negative": M.record(1, -0.25), "lam-nan": M.record(1, np.nan), "box-past-bottom": M.record(1, 0.5, (0, 33, 0, 4)),
    "box-past-right": M.record(1, 0.5, (0, 4, 30, 33)), "box-reversed": M.record(1, 0.5, (9, 4, 0, 4)),
}


@pytest.mark.parametrize("name", list(BAD_RECORDS))
def test_host_backend_rejects_a_bad_record(lib, name):
    imgs, labels, params = M.image_case("cifar", 3, seed=1)
    rec = np.asarray([M.record(1, 0.5), BAD_RECORDS[name], M.record(0, 0.25)], dtype=np.int32)
    rc, got, la, lb, lam, _ = M.run_augment_mix(lib, imgs, labels, params, rec, "cifar", torch.float32, False)
    assert rc == L.GS_EINVAL and lib.gs_last_error()
    # rejected before anything was written
    assert bool((got == 7.0).all()) and la.tolist() == lb.tolist() == [-7] * 3 and lam.tolist() == [-7.0] * 3


def test_host_backend_rejects_what_the_unmixed_entry_rejects(lib):
    imgs, labels, params = M.image_case("cifar", 2, seed=1)
    rec = np.asarray([M.record(1, 0.5), M.record(0, 0.5)], dtype=np.int32)
    bad = params.clone()
    bad[1, 0] = imgs.shape[0]
    rc = M.run_augment_mix(lib, imgs, labels, bad, rec, "cifar", torch.float32, False)[0]
    assert rc == L.GS_EINVAL and b"index out of range" in lib.gs_last_error()
    bad = params.clone()
    bad[0, 2] = 9
    rc = M.run_augment_mix(lib, imgs, labels, bad, rec, "cifar", torch.float32, False)[0]
    assert rc == L.GS_EINVAL and b"crop offset" in lib.gs_last_error()
    out = torch.empty(2, 3, 32, 32)
    rc = lib.gs_image_augment_mix(L.GS_DEV_HOST, 0, imgs.data_ptr(), labels.data_ptr(), imgs.shape[0], 32, 32, 3, 4, 32,
                                  32, params.data_ptr(), None, 2, out.data_ptr(), L.GS_F32, L.GS_LAYOUT_NCHW, None, None,
                                  None, None)
    assert rc == L.GS_EINVAL
    assert lib.gs_image_augment_mix(L.GS_DEV_HOST, 0, None, None, 0, 32, 32, 3, 4, 32, 32, None, None, 0, None, L.GS_F32,
                                    L.GS_LAYOUT_NCHW, None, None, None, None) == 0  # an empty batch
