"""MixUp / CutMix in the input step on the GPU: gs_image_augment_mix's two gfx950 kernels against the host backend
(itself pinned to the numpy restatement in tests/test_mix_cpu.py), bit for bit, in both layouts and dtypes;
a record the device must neutralise; and one loader epoch on the device against the CPU."""
import pytest
import torch

from distributed_training_amd import _lib as L
from distributed_training_amd import data as D
from tests import _mix_ref as M
from tests.test_mix_cpu import base_case, check_images

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def lib(cuda_device):
    return L.lib()


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("geometry", list(M.GEOMETRIES))  # cifar: the LDS kernel; the other two: the gather kernel
def test_hip_images_equal_the_host_backend(cuda_device, lib, geometry, dtype, channels_last):
    for records in ("handmade", "1", "3", "100"):
        imgs, labels, params, rec, _, _ = base_case(lib, geometry, records)
        host = M.run_augment_mix(lib, imgs, labels, params, rec, geometry, dtype, channels_last)
        check_images(lib, geometry, records, dtype, channels_last, device=cuda_device)  # against the restatement
        got = M.run_augment_mix(lib, imgs, labels, params, rec, geometry, dtype, channels_last, device=cuda_device)
        assert host[0] == got[0] == 0
        assert M.same_bits(got[1], host[1])
        assert torch.equal(got[2], host[2]) and torch.equal(got[3], host[3]) and M.same_bits(got[4], host[4])


@pytest.mark.parametrize("geometry", ["cifar", "30x30"], ids=["lds", "gather"])
def test_a_bad_record_on_the_device_is_neutralised(cuda_device, lib, geometry):
    """an ordinary in-bounds launch: sample 2's partner is outside the batch and its box larger than the output;
    sample 4's partner is fine and its box oversized, so it is clamped.  Neighbours exact, guard untouched."""
    crop = M.GEOMETRIES[geometry][3]
    imgs, labels, params = M.image_case(geometry, 6, seed=11)
    rec = M.random_records(6, crop, crop, seed=6)
    rec[2] = M.record(6, 0.25, (3, crop + 40, 2, crop + 9))
    rec[4] = M.record(1, 0.25, (3, crop + 40, 2, crop + 9))
    base, lab = M.unmixed_batch(lib, imgs, labels, params, geometry)
    valid = rec.copy()
    valid[2] = M.record(2, 1.0)  # what the device makes of it: the sample alone
    valid[4] = M.record(1, 0.25, (3, crop, 2, crop))  # the box clamped to the output
    want, want_b, want_lam = M.mix_images_ref(base, lab, valid, torch.float32)
    rc, got, la, lb, lam, guard = M.run_augment_mix(lib, imgs, labels, params, rec, geometry, torch.float32, False,
                                                    device=cuda_device, guard=4096)
    assert rc == 0, lib.gs_last_error()
    assert M.same_bits(got, want) and M.same_bits(got[2], base[2])
    assert torch.equal(la, lab) and torch.equal(lb, want_b) and M.same_bits(lam, want_lam)
    assert int(lb[2]) == int(la[2]) and float(lam[2]) == 1.0
    assert guard.numel() == 4096 and bool((guard == 7.0).all())


def test_one_loader_epoch_equals_the_cpu(cuda_device):
    cpu = D.ImageDataset.synthetic(n=1000)
    dev = D.ImageDataset(cpu.images, cpu.labels, cuda_device)
    out = {}
    for name, ds in (("cpu", cpu), ("hip", dev)):
        ld = D.DeviceDataLoader(ds, batch_size=100, drop_last=True, transform=D.TRAIN_TRANSFORM,
                                mix=D.MixUpCutMix(0.4, 1.0, mode="elem", seed=2),
                                sampler=D.DistributedSampler(ds, num_replicas=1, rank=0))
        torch.manual_seed(3)
        out[name] = []
        for x, t in ld:
            assert x.device == t.labels_a.device == t.labels_b.device == t.lam.device == ds.device
            out[name].append((x.cpu(), t.labels_a.cpu(), t.labels_b.cpu(), t.lam.cpu()))
    assert len(out["cpu"]) == len(out["hip"]) == 10
    mixed = 0
    for c, h in zip(out["cpu"], out["hip"]):
        assert M.same_bits(c[0], h[0]) and torch.equal(c[1], h[1]) and torch.equal(c[2], h[2]) and M.same_bits(c[3], h[3])
        mixed += int((c[3] != 1).sum())
    assert mixed > 500
