"""The resize-based input step on the GPU: gs_image_resample's two gfx950 kernels against the host backend (itself
pinned to the numpy restatement in tests/test_resample_cpu.py), bit for bit, in both layouts and dtypes with and
without Normalize; records the device must handle defensively; and one loader epoch per transform on the device
against the CPU.

The band kernel (LDS-staged source rows) takes the 4-aligned geometries up to a 2x downscale; 33x47 -> 17x29
(C * oh * ow is odd), 500x375 -> 8x8 (the taps skip most rows) and an ``out`` that is not 16-byte aligned take the
global-gather kernel.  "tall" and 256 -> 224 run several bands per sample."""
import numpy as np
import pytest
import torch

from distributed_training_amd import _lib as L
from distributed_training_amd import data as D
from tests import _resample_ref as R

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def lib(cuda_device):
    return L.lib()


@pytest.mark.parametrize("name", R.CASES)
def test_hip_equals_the_host_backend(cuda_device, lib, name):
    c = R.case(name)
    for combo in R.COMBOS:  # one launch per (layout, dtype, normalise)
        channels_last, dtype, normalise = combo
        mean, std = R.norm_of(name, normalise)
        host = R.run_resample(lib, c, dtype, channels_last, mean, std)
        got = R.run_resample(lib, c, dtype, channels_last, mean, std, device=cuda_device, guard=4096)
        assert host[0] == got[0] == 0, lib.gs_last_error()
        assert R.same_bits(got[1], host[1]), R.combo_id(combo)
        assert R.same_bits(got[1], R.reference(name, normalise)[0].to(dtype)), R.combo_id(combo)
        assert torch.equal(got[2], host[2])
        assert bool((got[3] == R.SENTINEL).all()) and bool((got[4] == -7).all())


def test_many_bands_per_sample_bf16_nhwc(cuda_device, lib):
    """256x256 -> 224x224, B = 8, bf16 NHWC with Normalize: the flagship geometry, seven bands per sample"""
    c = R.case("256to224-b8")
    host = R.run_resample(lib, c, BF16, True, R.IMAGENET_MEAN, R.IMAGENET_STD)
    got = R.run_resample(lib, c, BF16, True, R.IMAGENET_MEAN, R.IMAGENET_STD, device=cuda_device, guard=4096)
    assert host[0] == got[0] == 0, lib.gs_last_error()
    assert R.same_bits(got[1], host[1]) and torch.equal(got[2], host[2])
    assert bool((got[3] == R.SENTINEL).all()) and bool((got[4] == -7).all())


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["40x48-b3", "tall"])
def test_an_unaligned_out_takes_the_gather_kernel(cuda_device, lib, name, dtype):
    """``out`` one element past a 16-byte boundary: scalar stores, the same bits, the element before it untouched"""
    c = R.case(name)
    host = R.run_resample(lib, c, dtype, True, R.IMAGENET_MEAN, R.IMAGENET_STD)
    got = R.run_resample(lib, c, dtype, True, R.IMAGENET_MEAN, R.IMAGENET_STD, device=cuda_device, guard=4096, shift=1)
    assert host[0] == got[0] == 0, lib.gs_last_error()
    assert R.same_bits(got[1], host[1]) and torch.equal(got[2], host[2])
    assert bool((got[3] == R.SENTINEL).all()) and bool((got[4] == -7).all())


@pytest.mark.parametrize("name", ["40x48-b3", "33x47"], ids=["band", "gather"])
def test_records_the_device_cannot_reject(cuda_device, lib, name):
    """an ordinary in-bounds launch: sample 1's index is outside the set (zeros and label 0), sample 3's box reaches
    past the image and is clamped into it, sample 4's is empty and becomes one pixel.  Neighbours exact, the guard
    regions behind ``out`` and behind the labels untouched."""
    c = R.case(name)
    N, H, W, _ = c["imgs"].shape
    rec = R.random_records(6, N, H, W, seed=21)
    rec[1] = R.record(N + 5, 1, 2, 3, 10, 10)
    rec[3] = R.record(2, 1, H - 7, W - 9, 30, 40)
    rec[4] = R.record(3, 0, H + 20, W + 20, 0, 0)
    want, want_lab = R.resample_ref(c["imgs"], c["labels"], rec, c["out_hw"], c["frame"], R.IMAGENET_MEAN, R.IMAGENET_STD,
                                    device=True)
    valid = rec.copy()  # what the device makes of them, as records the host backend accepts
    valid[1] = R.record(0, 0, 0, 0, 1, 1)
    valid[3] = R.record(2, 1, H - 7, W - 9, 7, 9)
    valid[4] = R.record(3, 0, H - 1, W - 1, 1, 1)
    host = R.run_resample(lib, c, torch.float32, False, R.IMAGENET_MEAN, R.IMAGENET_STD, rec=valid)
    assert host[0] == 0, lib.gs_last_error()
    for channels_last, dtype in ((False, torch.float32), (True, BF16)):
        rc, got, lab, guard, lab_guard = R.run_resample(lib, c, dtype, channels_last, R.IMAGENET_MEAN, R.IMAGENET_STD,
                                                        device=cuda_device, guard=4096, rec=rec)
        assert rc == 0, lib.gs_last_error()
        assert R.same_bits(got, torch.from_numpy(want).to(dtype))
        assert not got[1].any() and int(lab[1]) == 0
        keep = [0, 2, 3, 4, 5]
        assert R.same_bits(got[keep], host[1][keep].to(dtype))
        assert torch.equal(lab, torch.from_numpy(want_lab)) and torch.equal(lab[keep], host[2][keep])
        assert guard.numel() == 4096 and bool((guard == R.SENTINEL).all()) and bool((lab_guard == -7).all())


def _epoch(ds, transform, **kw):
    ld = D.DeviceDataLoader(ds, batch_size=64, transform=transform, sampler=D.DistributedSampler(ds, num_replicas=1, rank=0),
                            **kw)
    out = []
    for x, y in ld:
        assert x.device == y.device == ds.device
        out.append((x.cpu(), y.cpu()))
    return out


def test_one_random_resized_crop_epoch_equals_the_cpu(cuda_device):
    cpu = D.ImageDataset.synthetic(n=300, H=40, W=48, seed=2)
    dev = D.ImageDataset(cpu.images, cpu.labels, cuda_device)
    kw = dict(mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD, seed=3, rank=0)
    torch.manual_seed(5)
    before = torch.get_rng_state()
    a = _epoch(cpu, D.RandomResizedCropFlip(32, **kw), out_dtype=BF16, memory_format=torch.channels_last, drop_last=True)
    b = _epoch(dev, D.RandomResizedCropFlip(32, **kw), out_dtype=BF16, memory_format=torch.channels_last, drop_last=True)
    assert torch.equal(torch.get_rng_state(), before)
    assert len(a) == len(b) == 4
    for (xa, ya), (xb, yb) in zip(a, b):
        assert xb.is_contiguous(memory_format=torch.channels_last)
        assert R.same_bits(xa, xb) and torch.equal(ya, yb)
    assert len({int(x[0].float().sum() * 1000) for x, _ in a}) == 4  # the batches differ


def test_one_resize_center_crop_epoch_equals_the_cpu(cuda_device):
    cpu = D.ImageDataset.synthetic(n=300, H=40, W=48, seed=2)
    dev = D.ImageDataset(cpu.images, cpu.labels, cuda_device)
    t = D.ResizeCenterCrop(36, 32, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD)
    a, b = _epoch(cpu, t), _epoch(dev, t)
    assert [x.shape[0] for x, _ in b] == [64, 64, 64, 64, 44]
    for (xa, ya), (xb, yb) in zip(a, b):
        assert R.same_bits(xa, xb) and torch.equal(ya, yb)
