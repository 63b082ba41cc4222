"""The resize-based input step on the host backend: gs_image_resample against the numpy restatement of its contract
bit for bit, against torch's own bilinear resize within the fp32 coordinate's error, the record draw of
data.RandomResizedCropFlip against a per-sample restatement, the two transforms through DeviceDataLoader, and what the
host backend rejects."""
import numpy as np
import pytest
import torch

from distributed_training_amd import _lib as L
from distributed_training_amd import data as D
from tests import _resample_ref as R

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    return L.lib()


# ---- images: bit for bit against the restatement ---------------------------------------------------------------
@pytest.mark.parametrize("combo", R.COMBOS, ids=R.combo_id)
@pytest.mark.parametrize("name", R.CASES)
def test_host_equals_the_restatement(lib, name, combo):
    channels_last, dtype, normalise = combo
    c = R.case(name)
    mean, std = R.norm_of(name, normalise)
    want, want_lab = R.reference(name, normalise)
    rc, got, lab, guard, lab_guard = R.run_resample(lib, c, dtype, channels_last, mean, std, guard=64)
    assert rc == 0, lib.gs_last_error()
    assert R.same_bits(got, want.to(dtype))
    assert torch.equal(lab, want_lab)
    assert bool((guard == R.SENTINEL).all()) and bool((lab_guard == -7).all())


def test_the_cases_cover_both_flips_and_every_clamp():
    flips = {int(r[1]) for n in R.CASES for r in R.case(n)["rec"]}
    assert flips == {0, 1}
    boxes = {R.decode(r)[4:] for r in R.case("upscale")["rec"]}
    assert {(1, 1), (1, 48), (40, 1), (2, 3)} <= boxes
    c = R.case("33x47")
    assert (c["imgs"].shape[3] * c["out_hw"][0] * c["out_hw"][1]) % 4 != 0


def test_identity_transform_is_totensor_normalize(lib):
    """resize=None, crop=None, mean = std = 0.5: the DeepSpeed reference's ToTensor + Normalize, computed by torch"""
    ds = D.ImageDataset.synthetic(n=37, H=40, W=48, seed=3)
    t = D.ResizeCenterCrop(mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))
    want = (ds.images.permute(0, 3, 1, 2).to(torch.float32) / 255 - 0.5) / 0.5
    got = torch.cat([x for x, _ in D.DeviceDataLoader(ds, batch_size=10, transform=t)])
    assert R.same_bits(got, want)
    plain = torch.cat([x for x, _ in D.DeviceDataLoader(ds, batch_size=10, transform=D.ResizeCenterCrop())])
    assert R.same_bits(plain, ds.images.permute(0, 3, 1, 2).to(torch.float32) / 255)


# ---- images: against torch itself ------------------------------------------------------------------------------
@pytest.mark.parametrize("normalise", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("name", R.CASES)
def test_host_is_close_to_torch(lib, name, normalise):
    c = R.case(name)
    mean, std = R.norm_of(name, normalise)
    rc, got, _, _, _ = R.run_resample(lib, c, torch.float32, False, mean, std)
    assert rc == 0, lib.gs_last_error()
    want = R.torch_ref(c["imgs"], c["rec"], c["out_hw"], c["frame"], mean, std)
    atol = R.torch_atol(c["rec"], std)
    worst = float((got - want).abs().max())
    print(f"{name}: worst |host - torch| = {worst:.3e}, bound {atol:.3e}")
    assert worst <= atol


def test_eval_transform_is_torch_resize_then_crop():
    ds = D.ImageDataset.synthetic(n=12, H=40, W=48, seed=4)
    t = D.ResizeCenterCrop(36, 32, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD)
    assert t.frame(40, 48) == (36, 43, 2, 6, (32, 32)) and t.out_hw(40, 48) == (32, 32)
    assert D.ResizeCenterCrop(36, 32).frame(48, 40) == (43, 36, 6, 2, (32, 32))  # the shorter side is the width
    assert D.ResizeCenterCrop((36, 50), (30, 31)).frame(40, 48) == (36, 50, 3, 10, (30, 31))
    got, lab = next(iter(D.DeviceDataLoader(ds, batch_size=12, transform=t)))
    x = ds.images.permute(0, 3, 1, 2).to(torch.float32) / 255
    want = torch.nn.functional.interpolate(x, size=(36, 43), mode="bilinear", align_corners=False, antialias=False)
    want = (want[:, :, 2:34, 6:38] - torch.tensor(R.IMAGENET_MEAN)[:, None, None]) / torch.tensor(R.IMAGENET_STD)[:, None, None]
    rec = [R.record(i, 0, 0, 0, 40, 48) for i in range(12)]
    assert float((got - want).abs().max()) <= R.torch_atol(rec, R.IMAGENET_STD)
    assert torch.equal(lab, ds.labels)
    with pytest.raises(ValueError):
        D.ResizeCenterCrop(36, 40).frame(40, 48)


# ---- records ---------------------------------------------------------------------------------------------------
GEOMS = {"32x32": (32, 32, (0.08, 1.0), (3 / 4, 4 / 3)), "500x375": (500, 375, (0.08, 1.0), (3 / 4, 4 / 3)),
         "fallback-wide": (40, 48, (4.0, 5.0), (3.0, 4.0)),  # every try is larger than the image; in_ratio < min(ratio)
         "fallback-tall": (40, 48, (4.0, 5.0), (0.25, 0.5)),  # in_ratio > max(ratio)
         "fallback-whole": (40, 48, (4.0, 5.0), (1.0, 1.5))}


@pytest.mark.parametrize("B", [1, 3, 257])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_the_vectorised_draw_equals_the_scalar_restatement(geom, B):
    H, W, scale, ratio = GEOMS[geom]
    t = D.RandomResizedCropFlip(24, scale=scale, ratio=ratio, seed=5, rank=2)
    idx = np.random.default_rng(B).integers(0, 1000, B)
    first = t.records(idx, H, W)
    second = t.records(idx[::-1].copy(), H, W)  # the stream goes on: the second batch differs
    assert first.dtype == np.int32 and first.shape == (B, 4)
    assert np.array_equal(first, R.draw_records_scalar(idx, H, W, scale, ratio, True, 5, 2))
    assert np.array_equal(second, R.draw_records_scalar(idx[::-1], H, W, scale, ratio, True, 5, 2, skip=(B,)))
    for row in np.concatenate([first, second]):
        _, flip, top, left, h, w = R.decode(row)
        assert flip in (0, 1) and h >= 1 and w >= 1 and 0 <= top and top + h <= H and 0 <= left and left + w <= W
    if geom.startswith("fallback"):
        want = {"fallback-wide": (16, 48), "fallback-tall": (40, 20), "fallback-whole": (40, 48)}[geom]
        assert all(R.decode(r)[4:] == want and R.decode(r)[2:4] == ((H - want[0]) // 2, (W - want[1]) // 2) for r in first)
    elif B == 257:
        assert len({tuple(r[2:]) for r in first}) > 200 and 60 < int(first[:, 1].sum()) < 200


def test_flip_off_rank_and_state_dict():
    a = D.RandomResizedCropFlip(24, flip=False, seed=1, rank=0)
    b = D.RandomResizedCropFlip(24, flip=True, seed=1, rank=0)
    idx = np.arange(50)
    ra, rb = a.records(idx, 64, 64), b.records(idx, 64, 64)
    assert not ra[:, 1].any() and rb[:, 1].any() and np.array_equal(ra[:, 2:], rb[:, 2:])  # f is drawn all the same
    other = D.RandomResizedCropFlip(24, seed=1, rank=1).records(idx, 64, 64)
    assert not np.array_equal(other[:, 2:], rb[:, 2:])
    state = b.state_dict()
    nxt = b.records(idx, 64, 64)
    fresh = D.RandomResizedCropFlip(24, seed=9, rank=3)
    fresh.load_state_dict(state)
    assert np.array_equal(fresh.records(idx, 64, 64), nxt)


def test_a_loader_epoch_leaves_torch_rng_alone_and_matches_the_records(lib):
    ds = D.ImageDataset.synthetic(n=50, H=40, W=48, seed=6)
    kw = dict(scale=(0.25, 1.0), mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD, seed=7, rank=0)
    ld = D.DeviceDataLoader(ds, batch_size=16, transform=D.RandomResizedCropFlip(32, **kw),
                            sampler=D.DistributedSampler(ds, num_replicas=1, rank=0), out_dtype=BF16,
                            memory_format=torch.channels_last)
    torch.manual_seed(11)
    before = torch.get_rng_state()
    batches = list(ld)
    assert torch.equal(torch.get_rng_state(), before)
    assert [x.shape[0] for x, _ in batches] == [16, 16, 16, 2]
    order = ld.sampler.indices()
    twin = D.RandomResizedCropFlip(32, **kw)
    c = dict(imgs=ds.images.numpy(), labels=ds.labels.numpy())
    for k, (x, y) in enumerate(batches):
        assert x.dtype == BF16 and x.is_contiguous(memory_format=torch.channels_last)
        rec = twin.records(order[16 * k:16 * k + 16], 40, 48)
        want, lab = R.resample_ref(c["imgs"], c["labels"], rec, (32, 32), (32, 32, 0, 0), R.IMAGENET_MEAN, R.IMAGENET_STD)
        assert R.same_bits(x.contiguous(), torch.from_numpy(want).to(BF16)) and torch.equal(y, torch.from_numpy(lab))


# ---- what is rejected ------------------------------------------------------------------------------------------
BAD = {
    "index": dict(rec=[R.record(0, 0, 0, 0, 40, 48), R.record(23, 0, 0, 0, 40, 48)]),
    "negative-index": dict(rec=[R.record(-1, 0, 0, 0, 40, 48)]),
    "empty-h": dict(rec=[R.record(0, 0, 3, 3, 0, 5)]),
    "empty-w": dict(rec=[R.record(0, 0, 3, 3, 5, 0)]),
    "box-below": dict(rec=[R.record(0, 0, 30, 0, 11, 48)]),
    "box-right": dict(rec=[R.record(0, 0, 0, 40, 40, 9)]),
    "std-zero": dict(mean=(0.5, 0.5, 0.5), std=(0.5, 0.0, 0.5)),
    "mean-alone": dict(mean=(0.5, 0.5, 0.5)),
    "frame-offset": dict(frame=(36, 43, 5, 6)),  # 5 + 32 > 36
    "frame-negative": dict(frame=(36, 43, -1, 6)),
    "frame-small": dict(frame=(31, 43, 0, 0)),
}


@pytest.mark.parametrize("what", list(BAD))
def test_host_rejects_before_writing(lib, what):
    kw = dict(BAD[what])
    if "rec" in kw:
        kw["rec"] = np.asarray(kw["rec"], dtype=np.int32)
    rc, img, lab, _, _ = R.run_resample(lib, R.case("40x48-b3"), torch.float32, False, **kw)
    assert rc == L.GS_EINVAL
    assert bool((img == R.SENTINEL).all()) and bool((lab == -7).all())


def test_mix_with_a_resize_transform_raises():
    ds = D.ImageDataset.synthetic(n=8, H=40, W=48)
    for t in (D.RandomResizedCropFlip(32), D.ResizeCenterCrop(36, 32)):
        with pytest.raises(NotImplementedError, match="mix"):
            D.DeviceDataLoader(ds, batch_size=4, transform=t, mix=D.MixUpCutMix(0.2))
    with pytest.raises(ValueError):
        D.DeviceDataLoader(ds, batch_size=4, transform=D.ResizeCenterCrop(mean=(0.5,), std=(0.5,)))


def test_the_package_exports_the_transforms():
    import distributed_training_amd as P

    assert P.RandomResizedCropFlip is D.RandomResizedCropFlip and P.ResizeCenterCrop is D.ResizeCenterCrop
