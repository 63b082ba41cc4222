"""Input step of the CIFAR configuration on libgsync.

The reference builds its batches with torchvision + a torch DataLoader
(R:resnet/pytorch_ddp/ddp_train.py:25-48):

    transform_train = Compose([Pad(4), RandomHorizontalFlip(), RandomCrop(32), ToTensor()])
    DataLoader(CIFAR10(...), batch_size, shuffle=False, drop_last=True,
               sampler=DistributedSampler(train_dataset))
    ... images.to(device)                                           (:62)

Here the uint8 image set is resident on the device (HBM: CIFAR-10's 50,000
train images are 153.6 MB) and every batch is ONE libgsync kernel that
gathers the sampled images, pads, flips, crops and converts to float
(x / 255) straight into the training tensor, labels gathered alongside —
no per-sample PIL work, no collate, no H2D of pixels.  Only the per-sample
(index, flip, top, left) table (16 B/sample) crosses PCIe.

Parity with the reference pipeline is exact, not statistical:

* :class:`DistributedSampler` yields torch's indices (randperm(n) under
  ``manual_seed(seed + epoch)``, head-repeat padding, ``[rank::ws]`` stride;
  T:utils/data/distributed.py:107-138), computed by libgsync's C++ restatement
  of torch's MT19937 / randperm.
* the per-sample random flip / crop offsets consume torch's *global* CPU
  generator in torchvision 0.15.2's order (flip draw, then the crop's two
  draws, per sample in sampler order, after the DataLoader iterator's one
  int64 base-seed draw), so a script that seeds torch gets the same
  augmentations as with the reference's DataLoader, and the generator is left
  in the same state.

Image sets of another shape (pre-resized 256x256, downsampled ImageNet 64x64)
take the resize-based transforms :class:`RandomResizedCropFlip` and
:class:`ResizeCenterCrop` (+ ``Normalize``): one ``gs_image_resample`` launch
per batch, boxes drawn from the transform's own numpy generator.

There is no dataset download (no network): :meth:`ImageDataset.cifar10_bin`
reads the CIFAR-10 *binary* distribution from disk when present;
:meth:`ImageDataset.synthetic` makes a seeded stand-in of the same shape.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Iterator, NamedTuple, Sequence

import numpy as np
import torch
import torch.distributed as dist

from . import _lib as L


def _sampler_indices(n, num_replicas, rank, shuffle, seed, epoch, drop_last) -> np.ndarray:
    lib = L.lib()
    count = ctypes.c_int64()
    L.check(lib.gs_distributed_sampler_indices(n, num_replicas, rank, int(bool(shuffle)), int(seed), int(epoch),
                                               int(bool(drop_last)), None, 0, ctypes.byref(count)),
            "gs_distributed_sampler_indices")
    out = np.empty(max(1, count.value), dtype=np.int64)
    L.check(lib.gs_distributed_sampler_indices(n, num_replicas, rank, int(bool(shuffle)), int(seed), int(epoch),
                                               int(bool(drop_last)), out.ctypes.data, out.size,
                                               ctypes.byref(count)),
            "gs_distributed_sampler_indices")
    return out[: count.value]


def randperm(n: int, seed: int) -> np.ndarray:
    """torch.randperm(n, generator=torch.Generator().manual_seed(seed)), in C++."""
    out = np.empty(max(1, n), dtype=np.int64)
    L.check(L.lib().gs_randperm(int(seed), int(n), out.ctypes.data), "gs_randperm")
    return out[:n]


class DistributedSampler(torch.utils.data.Sampler):
    """Drop-in for torch.utils.data.DistributedSampler (same arguments, errors,
    ``set_epoch``, ``__len__``), indices from libgsync."""

    def __init__(self, dataset, num_replicas: int | None = None, rank: int | None = None, shuffle: bool = True,
                 seed: int = 0, drop_last: bool = False):
        if num_replicas is None:
            if not dist.is_available():
                raise RuntimeError("Requires distributed package to be available")
            num_replicas = dist.get_world_size()
        if rank is None:
            if not dist.is_available():
                raise RuntimeError("Requires distributed package to be available")
            rank = dist.get_rank()
        if rank >= num_replicas or rank < 0:
            raise ValueError(f"Invalid rank {rank}, rank should be in the interval [0, {num_replicas - 1}]")
        self.dataset = dataset
        self.num_replicas = num_replicas
        self.rank = rank
        self.epoch = 0
        self.drop_last = drop_last
        n = len(dataset)
        if self.drop_last and n % self.num_replicas != 0:
            self.num_samples = math.ceil((n - self.num_replicas) / self.num_replicas)
        else:
            self.num_samples = math.ceil(n / self.num_replicas)
        self.total_size = self.num_samples * self.num_replicas
        self.shuffle = shuffle
        self.seed = seed

    def indices(self) -> np.ndarray:
        return _sampler_indices(len(self.dataset), self.num_replicas, self.rank, self.shuffle, self.seed,
                                self.epoch, self.drop_last)

    def __iter__(self) -> Iterator[int]:
        return iter(self.indices().tolist())

    def __len__(self) -> int:
        return self.num_samples

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch


class ImageDataset:
    """A uint8 image set ``[N, H, W, C]`` (HWC, as CIFAR10.data) + int64 labels,
    resident on one device (HBM for a HIP device)."""

    def __init__(self, images, labels, device="cpu"):
        images = torch.as_tensor(images)
        labels = torch.as_tensor(labels)
        if images.dtype != torch.uint8 or images.dim() != 4:
            raise ValueError("images must be uint8 [N, H, W, C]")
        if labels.dim() != 1 or labels.numel() != images.shape[0]:
            raise ValueError("labels must be [N]")
        self.device = torch.device(device)
        self.images = images.contiguous().to(self.device)
        self.labels = labels.to(torch.int64).contiguous().to(self.device)
        self.n, self.H, self.W, self.C = (int(x) for x in images.shape)

    def __len__(self) -> int:
        return self.n

    @classmethod
    def synthetic(cls, n=50000, H=32, W=32, C=3, classes=10, seed=0, device="cpu"):
        g = torch.Generator().manual_seed(seed)
        imgs = torch.randint(0, 256, (n, H, W, C), dtype=torch.uint8, generator=g)
        labels = torch.randint(0, classes, (n,), generator=g)
        return cls(imgs, labels, device)

    @classmethod
    def cifar10_bin(cls, root, train=True, device="cpu"):
        """CIFAR-10 binary version (cifar-10-batches-bin/{data_batch_1..5,test_batch}.bin:
        records of 1 label byte + 3,072 bytes R|G|B planes of 32x32, row-major)."""
        d = os.path.join(root, "cifar-10-batches-bin") if not os.path.exists(os.path.join(root, "test_batch.bin")) else root
        names = [f"data_batch_{i}.bin" for i in range(1, 6)] if train else ["test_batch.bin"]
        recs = []
        for nm in names:
            path = os.path.join(d, nm)
            if not os.path.exists(path):
                raise FileNotFoundError(f"{path} (CIFAR-10 binary version; there is no download here)")
            raw = np.fromfile(path, dtype=np.uint8)
            if raw.size % 3073:
                raise ValueError(f"{path}: size is not a multiple of 3073-byte records")
            recs.append(raw.reshape(-1, 3073))
        rec = np.concatenate(recs)
        labels = rec[:, 0].astype(np.int64)
        imgs = rec[:, 1:].reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1).copy()
        return cls(imgs, labels, device)


class PadFlipCrop:
    """Compose([Pad(pad), RandomHorizontalFlip(), RandomCrop(crop), ToTensor()])
    (R:resnet/pytorch_ddp/ddp_train.py:27-31); pad=0, flip=False, crop=None is
    the test transform ToTensor() (:32)."""

    def __init__(self, pad=4, flip=True, crop=32):
        self.pad, self.flip, self.crop = int(pad), bool(flip), crop

    def out_hw(self, H, W):
        if self.crop is None:
            return H + 2 * self.pad, W + 2 * self.pad
        c = self.crop
        return (c, c) if isinstance(c, int) else (int(c[0]), int(c[1]))


TRAIN_TRANSFORM = PadFlipCrop(4, True, 32)
TEST_TRANSFORM = PadFlipCrop(0, False, None)


class MixedTarget(NamedTuple):
    """The target of a mixed batch: row ``i`` is ``labels_a[i]`` with weight ``lam[i]`` and
    ``labels_b[i]`` with weight ``1 - lam[i]``.  int64 ``[B]``, int64 ``[B]``, float32 ``[B]``, on the
    batch's device.  ``loss.cross_entropy`` and ``CrossEntropyLoss`` take it in place of the labels."""
    labels_a: torch.Tensor
    labels_b: torch.Tensor
    lam: torch.Tensor


_LAM_ONE = int(np.float32(1.0).view(np.int32))


class MixUpCutMix:
    """MixUp (Zhang et al., 2018) and CutMix (Yun et al., 2019) for :class:`DeviceDataLoader`: it draws, per
    batch, the ``[B, 4]`` int32 records ``gs_image_augment_mix`` (include/gsync.h) applies inside the input
    kernel: ``(partner, lam as fp32 bits, y0 | y1 << 16, x0 | x1 << 16)``.

    ``mixup_alpha`` / ``cutmix_alpha``: the Beta(alpha, alpha) parameter of each; 0 turns that one off, both
    0 is an error.  ``prob``: the chance that a batch (``mode="batch"``) or a sample (``mode="elem"``) is
    mixed at all.  ``switch_prob``: with both on, the chance of CutMix.

    The draws come from this object's own ``numpy.random.Generator`` (PCG64 seeded ``[seed, rank]``;
    ``rank=None``: the process group's rank if one is initialised, else 0), never from torch's generators.
    ``state_dict()`` / ``load_state_dict()`` carry the bit generator's state.

    Draw order per batch of ``B`` samples with output extent ``oh x ow``, ``mode="batch"``:

    1. ``u_apply = rng.random()``
    2. ``u_switch = rng.random()`` (both always drawn)
    3. ``u_apply >= prob``: identity records, nothing else is drawn
    4. CutMix if both alphas are positive and ``u_switch < switch_prob``, or if only ``cutmix_alpha`` is
       positive; else MixUp; ``a`` is the chosen one's alpha
    5. ``lam = rng.beta(a, a)``
    6. CutMix only: ``cy = rng.integers(oh)``, then ``cx = rng.integers(ow)``
    7. ``perm = rng.permutation(B)``: sample ``i``'s partner is batch position ``perm[i]``

    ``mode="elem"`` makes the same draws as length-``B`` vectors in the same order and never stops early:
    ``u_apply = rng.random(B)``, ``u_switch = rng.random(B)``, ``lam = rng.beta(a, a)`` with ``a`` the
    vector of each sample's chosen alpha (1.0 for a sample with ``u_apply >= prob``, whose draws are then
    unused), then, if ``cutmix_alpha`` is positive, ``cy = rng.integers(oh, size=B)`` and
    ``cx = rng.integers(ow, size=B)``, then one ``perm = rng.permutation(B)``.

    MixUp's record is ``(perm[i], fp32(lam), 0, 0)``.  CutMix's box is the paper's ``rand_bbox`` on the output
    extent: ``r = sqrt(1 - lam)``, ``ch = int(oh * r)``, ``cw = int(ow * r)``, ``y0, y1 = clip(cy -/+ ch // 2,
    0, oh)``, ``x0, x1`` likewise, and the weight is corrected to the box, ``lam = 1 - (y1 - y0) * (x1 - x0) /
    (oh * ow)`` in double, rounded to fp32.  An empty box, and a sample that is not mixed, is the identity
    record ``(i, fp32(1), 0, 0)``."""

    def __init__(self, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, prob: float = 1.0,
                 switch_prob: float = 0.5, mode: str = "batch", seed: int = 0, rank: int | None = None):
        if mixup_alpha < 0 or cutmix_alpha < 0 or not (mixup_alpha > 0 or cutmix_alpha > 0):
            raise ValueError("MixUpCutMix: mixup_alpha and cutmix_alpha must be >= 0 and not both 0")
        if mode not in ("batch", "elem"):
            raise ValueError("MixUpCutMix: mode must be 'batch' or 'elem'")
        if not (0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0):
            raise ValueError("MixUpCutMix: prob and switch_prob must be in [0, 1]")
        if rank is None:
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.mode = float(prob), float(switch_prob), mode
        self.seed, self.rank = int(seed), int(rank)
        self.rng = np.random.Generator(np.random.PCG64([self.seed, self.rank]))

    def state_dict(self) -> dict:
        return {"bit_generator": self.rng.bit_generator.state}

    def load_state_dict(self, state: dict) -> None:
        self.rng.bit_generator.state = state["bit_generator"]

    def _cutmix(self, u_switch):
        """CutMix (True) or MixUp (False) for the draw(s) ``u_switch``"""
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            return u_switch < self.switch_prob
        return np.full(np.shape(u_switch), self.cutmix_alpha > 0)

    def records(self, B: int, oh: int, ow: int) -> np.ndarray:
        """the next batch's ``[B, 4]`` int32 records (see the class's docstring for the draws)"""
        rng = self.rng
        rec = np.zeros((B, 4), dtype=np.int32)
        rec[:, 0] = np.arange(B)
        rec[:, 1] = _LAM_ONE
        if self.mode == "batch":
            u_apply, u_switch = rng.random(), rng.random()
            if u_apply >= self.prob:
                return rec
            is_cut = bool(self._cutmix(u_switch))
            a = self.cutmix_alpha if is_cut else self.mixup_alpha
            cut = np.full(B, is_cut)
            lam = np.full(B, rng.beta(a, a))
            cy = cx = None
            if is_cut:
                cy = np.full(B, rng.integers(oh))
                cx = np.full(B, rng.integers(ow))
            apply = np.ones(B, dtype=bool)
        else:
            u_apply, u_switch = rng.random(B), rng.random(B)
            apply = u_apply < self.prob
            cut = np.asarray(self._cutmix(u_switch), dtype=bool) & apply
            a = np.where(apply, np.where(cut, self.cutmix_alpha, self.mixup_alpha), 1.0)
            lam = rng.beta(a, a)
            cy = cx = None
            if self.cutmix_alpha > 0:
                cy, cx = rng.integers(oh, size=B), rng.integers(ow, size=B)
        perm = rng.permutation(B)
        lam32 = lam.astype(np.float32)
        ys = np.zeros(B, dtype=np.int64)
        xs = np.zeros(B, dtype=np.int64)
        if cy is not None:
            r = np.sqrt(1.0 - lam)
            ch, cw = (oh * r).astype(np.int64), (ow * r).astype(np.int64)
            y0, y1 = np.clip(cy - ch // 2, 0, oh), np.clip(cy + ch // 2, 0, oh)
            x0, x1 = np.clip(cx - cw // 2, 0, ow), np.clip(cx + cw // 2, 0, ow)
            area = (y1 - y0) * (x1 - x0)
            boxed = cut & (area > 0)
            apply = apply & (boxed | ~cut)  # an empty box is the identity
            lam32 = np.where(cut, (1.0 - area / float(oh * ow)).astype(np.float32), lam32)
            ys = np.where(boxed, y0 | (y1 << 16), 0)
            xs = np.where(boxed, x0 | (x1 << 16), 0)
        rec[:, 0] = np.where(apply, perm, rec[:, 0])
        rec[:, 1] = np.where(apply, lam32.view(np.int32), _LAM_ONE)
        rec[:, 2] = ys.astype(np.uint32).view(np.int32)
        rec[:, 3] = xs.astype(np.uint32).view(np.int32)
        return rec


def _pair(v):
    return (int(v), int(v)) if isinstance(v, (int, np.integer)) else (int(v[0]), int(v[1]))


def _mean_std(mean, std, what):
    if (mean is None) != (std is None):
        raise ValueError(f"{what}: mean and std go together")
    if mean is None:
        return None, None
    mean, std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
    if len(mean) != len(std) or not 1 <= len(mean) <= 4:
        raise ValueError(f"{what}: mean and std must have the same length, at most 4")
    if any(np.float32(s) == 0 for s in std):
        raise ValueError(f"{what}: std must not be 0")
    return mean, std


def _pack_records(idx, flip, top, left, h, w) -> np.ndarray:
    """the ``[B, 4]`` int32 records of ``gs_image_resample``: (index, flip, top | left << 16, h | w << 16)"""
    rec = np.empty((len(idx), 4), dtype=np.int32)
    rec[:, 0] = idx
    rec[:, 1] = flip
    rec[:, 2] = (np.asarray(top, dtype=np.int64) | (np.asarray(left, dtype=np.int64) << 16)).astype(np.uint32).view(np.int32)
    rec[:, 3] = (np.asarray(h, dtype=np.int64) | (np.asarray(w, dtype=np.int64) << 16)).astype(np.uint32).view(np.int32)
    return rec


class RandomResizedCropFlip:
    """Compose([RandomResizedCrop(size, scale, ratio, antialias=False), RandomHorizontalFlip(), ToTensor(),
    Normalize(mean, std)]) of torchvision's tensor path for :class:`DeviceDataLoader`: it draws, per batch, the
    ``[B, 4]`` int32 records ``gs_image_resample`` (include/gsync.h) applies in one launch:
    ``(index, flip, top | left << 16, h | w << 16)``.  ``flip=False`` leaves every image unflipped;
    ``mean=None, std=None`` leaves out ``Normalize``.

    The draws come from this object's own ``numpy.random.Generator`` (PCG64 seeded ``[seed, rank]``;
    ``rank=None``: the process group's rank if one is initialised, else 0), never from torch's generators.
    ``state_dict()`` / ``load_state_dict()`` carry the bit generator's state.

    Draw order per batch of ``B`` samples of ``H x W`` images; the count is fixed, so the stream's state does not
    depend on the data:

    1. ``u = rng.random((B, 10, 2))``: ten tries per sample
    2. ``f = rng.random(B)``
    3. ``pos = rng.random((B, 2))``

    Try ``k`` of a sample follows torchvision's ``get_params`` in numpy float64 operations:
    ``area = H * W * (s0 + u[k, 0] * (s1 - s0))``,
    ``r = np.exp(np.log(r0) + u[k, 1] * (np.log(r1) - np.log(r0)))``, ``w = np.rint(np.sqrt(area * r))``,
    ``h = np.rint(np.sqrt(area / r))``; the try is valid when ``0 < w <= W`` and ``0 < h <= H``, and the first
    valid try wins.  Then ``top = floor(pos[0] * (H - h + 1))`` and ``left = floor(pos[1] * (W - w + 1))``.
    A sample with no valid try takes torchvision's ratio-clamped central crop and ignores ``pos``: with
    ``in_ratio = W / H``, ``w = W, h = int(round(W / min(ratio)))`` if ``in_ratio < min(ratio)``;
    ``h = H, w = int(round(H * max(ratio)))`` if ``in_ratio > max(ratio)``; else the whole image; h and w are
    kept in ``[1, H]`` and ``[1, W]``; ``top = (H - h) // 2``, ``left = (W - w) // 2``.
    ``flip = f < 0.5`` (0 when ``flip=False``; ``f`` is drawn all the same)."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip: bool = True, mean=None, std=None,
                 seed: int = 0, rank: int | None = None):
        self.size = _pair(size)
        if min(self.size) <= 0 or max(self.size) > 65535:
            raise ValueError("RandomResizedCropFlip: size must be in [1, 65535]")
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        if not (0 < self.scale[0] <= self.scale[1]) or not (0 < self.ratio[0] <= self.ratio[1]):
            raise ValueError("RandomResizedCropFlip: scale and ratio must be positive (min, max) pairs")
        self.flip = bool(flip)
        self.mean, self.std = _mean_std(mean, std, "RandomResizedCropFlip")
        if rank is None:
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.seed, self.rank = int(seed), int(rank)
        self.rng = np.random.Generator(np.random.PCG64([self.seed, self.rank]))

    def state_dict(self) -> dict:
        return {"bit_generator": self.rng.bit_generator.state}

    def load_state_dict(self, state: dict) -> None:
        self.rng.bit_generator.state = state["bit_generator"]

    def out_hw(self, H, W):
        return self.size

    def frame(self, H, W):
        """(virt_h, virt_w, off_y, off_x): the output is the whole resized box"""
        return self.size[0], self.size[1], 0, 0

    def records(self, idx: np.ndarray, H: int, W: int) -> np.ndarray:
        """the next batch's ``[B, 4]`` int32 records (see the class's docstring for the draws)"""
        rng = self.rng
        B = len(idx)
        u = rng.random((B, 10, 2))
        f = rng.random(B)
        pos = rng.random((B, 2))
        (s0, s1), (r0, r1) = self.scale, self.ratio
        area = (H * W) * (s0 + u[:, :, 0] * (s1 - s0))
        lr0, lr1 = np.log(r0), np.log(r1)
        r = np.exp(lr0 + u[:, :, 1] * (lr1 - lr0))
        w = np.rint(np.sqrt(area * r))
        h = np.rint(np.sqrt(area / r))
        valid = (w > 0) & (w <= W) & (h > 0) & (h <= H)
        any_valid = valid.any(axis=1)
        first = np.argmax(valid, axis=1)
        rows = np.arange(B)
        w = w[rows, first].astype(np.int64)
        h = h[rows, first].astype(np.int64)
        top = np.floor(pos[:, 0] * (H - h + 1)).astype(np.int64)
        left = np.floor(pos[:, 1] * (W - w + 1)).astype(np.int64)
        if not any_valid.all():
            in_ratio = float(W) / float(H)
            if in_ratio < min(self.ratio):
                fw, fh = W, int(round(W / min(self.ratio)))
            elif in_ratio > max(self.ratio):
                fh, fw = H, int(round(H * max(self.ratio)))
            else:
                fw, fh = W, H
            fh, fw = min(max(fh, 1), H), min(max(fw, 1), W)
            h, w = np.where(any_valid, h, fh), np.where(any_valid, w, fw)
            top, left = np.where(any_valid, top, (H - fh) // 2), np.where(any_valid, left, (W - fw) // 2)
        flip = (f < 0.5) if self.flip else np.zeros(B, dtype=bool)
        return _pack_records(idx, flip, top, left, h, w)


class ResizeCenterCrop:
    """Compose([Resize(resize, antialias=False), CenterCrop(crop), ToTensor(), Normalize(mean, std)]) of
    torchvision's tensor path for :class:`DeviceDataLoader`; deterministic.  An int ``resize`` makes the image's
    shorter side ``resize`` and the longer one ``int(resize * long / short)``; a pair is ``(h, w)``; ``None``
    keeps the image's extent.  ``crop`` (an int or ``(h, w)``; ``None``: the whole resized image) is taken at
    ``int(round((V - c) / 2.0))`` of the resized extent ``V`` on each axis and must fit inside it.

    The kernel never forms the resized image: the record's box is the whole image, and the launch's virtual
    output frame is the resized extent with the crop's offset, which equals resizing and then slicing exactly.
    ``resize=None, crop=None`` is ``ToTensor()`` (+ ``Normalize``) alone, bit-identical to ``(x / 255 - mean) / std``
    (every second weight is 0): with ``mean = std = (0.5, 0.5, 0.5)`` the DeepSpeed reference's transform
    (R:resnet/deepspeed/deepspeed_train.py:227-230)."""

    def __init__(self, resize=None, crop=None, mean=None, std=None):
        self.resize = None if resize is None else (int(resize) if isinstance(resize, (int, np.integer)) else _pair(resize))
        self.crop = None if crop is None else _pair(crop)
        self.mean, self.std = _mean_std(mean, std, "ResizeCenterCrop")

    def _virt(self, H, W):
        if self.resize is None:
            return H, W
        if isinstance(self.resize, int):
            s = self.resize
            return (s, int(s * W / H)) if H <= W else (int(s * H / W), s)
        return self.resize

    def out_hw(self, H, W):
        return self.frame(H, W)[4]

    def frame(self, H, W):
        """(virt_h, virt_w, off_y, off_x, (out_h, out_w))"""
        vh, vw = self._virt(H, W)
        ch, cw = self.crop if self.crop is not None else (vh, vw)
        if not (0 < ch <= vh <= 65535 and 0 < cw <= vw <= 65535):
            raise ValueError(f"ResizeCenterCrop: crop {ch}x{cw} does not fit the resized image {vh}x{vw}")
        return vh, vw, int(round((vh - ch) / 2.0)), int(round((vw - cw) / 2.0)), (ch, cw)

    def records(self, idx: np.ndarray, H: int, W: int) -> np.ndarray:
        z = np.zeros(len(idx), dtype=np.int64)
        return _pack_records(idx, z, z, z, z + H, z + W)


class DeviceDataLoader:
    """``DataLoader(dataset, batch_size, shuffle=False, sampler=..., drop_last=...)``
    over an :class:`ImageDataset`, yielding ``(images, labels)`` on the
    dataset's device: images float32 (or ``out_dtype``) ``[B, C, h, w]`` in
    ``memory_format``, labels int64 ``[B]``.

    ``mix``: a :class:`MixUpCutMix`; the batch is then mixed inside the same kernel
    (``gs_image_augment_mix``) and the loader yields ``(images, MixedTarget)``.

    ``transform``: a :class:`PadFlipCrop` (``gs_image_augment``), or a :class:`RandomResizedCropFlip` or
    :class:`ResizeCenterCrop` (``gs_image_resample``: resized crop, flip, ToTensor and Normalize in one launch).
    The latter two draw nothing from torch's generators and cannot be combined with ``mix`` yet."""

    def __init__(self, dataset: ImageDataset, batch_size: int = 1, shuffle: bool = False, sampler=None,
                 drop_last: bool = False, transform=TEST_TRANSFORM,
                 out_dtype: torch.dtype = torch.float32, memory_format=torch.contiguous_format,
                 generator: torch.Generator | None = None, mix: MixUpCutMix | None = None):
        if shuffle and sampler is not None:
            raise ValueError("sampler option is mutually exclusive with shuffle")
        if shuffle:
            raise NotImplementedError("shuffle=True (RandomSampler) is not on the reference path; "
                                      "pass sampler=DistributedSampler(...)")
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("out_dtype must be float32 or bfloat16")
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.sampler = sampler
        self.drop_last = drop_last
        self.transform = transform
        self.out_dtype = out_dtype
        self.memory_format = memory_format
        self.generator = generator
        self.mix = mix
        self.device = dataset.device
        self._kind = L.GS_DEV_HIP if self.device.type == "cuda" else L.GS_DEV_HOST
        if self._kind == L.GS_DEV_HIP and not L.available():
            raise L.GsyncUnavailable(L._load_error)
        self._resample = isinstance(transform, (RandomResizedCropFlip, ResizeCenterCrop))
        if self._resample and mix is not None:
            raise NotImplementedError("mix= with RandomResizedCropFlip / ResizeCenterCrop: mixing two resized crops "
                                      "in one launch is not implemented; use a PadFlipCrop transform with mix=")
        if self._resample and max(dataset.H, dataset.W) > 65535:
            raise ValueError("gs_image_resample takes images of at most 65535 x 65535")
        if self._resample and transform.mean is not None and len(transform.mean) != dataset.C:
            raise ValueError(f"transform has {len(transform.mean)} mean / std values for {dataset.C} channels")
        self.oh, self.ow = transform.out_hw(dataset.H, dataset.W)

    def _indices(self) -> list:
        if self.sampler is None:
            return list(range(len(self.dataset)))
        if hasattr(self.sampler, "indices"):
            return self.sampler.indices().tolist()
        return list(iter(self.sampler))

    def __len__(self) -> int:
        n = len(self.sampler) if self.sampler is not None else len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _rng_get(self):
        if self.generator is not None:
            return self.generator.get_state()
        return torch.get_rng_state()

    def _rng_set(self, st):
        if self.generator is not None:
            self.generator.set_state(st)
        else:
            torch.set_rng_state(st)

    def _draw_params(self, idx: np.ndarray) -> torch.Tensor:
        B = idx.size
        t = self.transform
        # a fresh pinned block per batch: torch's host caching allocator keeps it
        # from reuse until the non_blocking H2D copy that reads it has run
        params = torch.empty((B, 4), dtype=torch.int32, pin_memory=self._kind == L.GS_DEV_HIP)
        st = self._rng_get()
        nbytes = st.numel()
        L.check(L.lib().gs_crop_flip_params(idx.ctypes.data, B, self.dataset.H, self.dataset.W, t.pad, self.oh,
                                            self.ow, int(t.flip), st.data_ptr(), nbytes, params.data_ptr()),
                "gs_crop_flip_params")
        self._rng_set(st)
        return params

    def _iter_resample(self, order: np.ndarray):
        """the batches of a RandomResizedCropFlip / ResizeCenterCrop loader: one gs_image_resample each"""
        t, ds, bs = self.transform, self.dataset, self.batch_size
        vh, vw, oy, ox = t.frame(ds.H, ds.W)[:4]
        hip = self._kind == L.GS_DEV_HIP
        mean = std = None
        if t.mean is not None:
            mean, std = (ctypes.c_float * ds.C)(*t.mean), (ctypes.c_float * ds.C)(*t.std)
        for k in range(len(self)):
            idx = order[k * bs:(k + 1) * bs]
            B = idx.size
            # the records travel as PadFlipCrop's params do: a pinned block per batch, a non-blocking copy
            rec = torch.empty((B, 4), dtype=torch.int32, pin_memory=hip)
            rec.numpy()[...] = t.records(idx, ds.H, ds.W)
            drec = rec.to(self.device, non_blocking=True) if hip else rec
            out = torch.empty((B, ds.C, self.oh, self.ow), dtype=self.out_dtype, device=self.device,
                              memory_format=self.memory_format)
            layout = L.GS_LAYOUT_NHWC if (self.memory_format == torch.channels_last and B > 0) else L.GS_LAYOUT_NCHW
            labels = torch.empty(B, dtype=torch.int64, device=self.device)
            L.check(L.lib().gs_image_resample(self._kind, self.device.index or 0, ds.images.data_ptr(),
                                               ds.labels.data_ptr(), ds.n, ds.H, ds.W, ds.C, self.oh, self.ow, vh, vw,
                                               oy, ox, drec.data_ptr(), B, mean, std, out.data_ptr(),
                                               L.gs_dtype(self.out_dtype), layout, labels.data_ptr(),
                                               L.stream_ptr(self.device)),
                    "gs_image_resample")
            yield out, labels

    def __iter__(self):
        order = np.asarray(self._indices(), dtype=np.int64)
        if order.size and (order.min() < 0 or order.max() >= len(self.dataset)):
            raise IndexError("sampler produced an index outside the dataset")
        if self._resample:
            yield from self._iter_resample(order)
            return
        # _BaseDataLoaderIter.__init__: one int64 draw for the workers' base seed
        torch.empty((), dtype=torch.int64).random_(generator=self.generator)
        bs = self.batch_size
        nb = len(self)
        ds = self.dataset
        for k in range(nb):
            idx = np.ascontiguousarray(order[k * bs:(k + 1) * bs])
            B = idx.size
            params = self._draw_params(idx)
            if self._kind == L.GS_DEV_HIP:
                dparams = params.to(self.device, non_blocking=True)
                stream = L.stream_ptr(self.device)
            else:
                dparams, stream = params, None
            out = torch.empty((B, ds.C, self.oh, self.ow), dtype=self.out_dtype, device=self.device,
                              memory_format=self.memory_format)
            layout = L.GS_LAYOUT_NHWC if (self.memory_format == torch.channels_last and B > 0) else L.GS_LAYOUT_NCHW
            labels = torch.empty(B, dtype=torch.int64, device=self.device)
            if self.mix is not None:
                # the records travel as params does: a pinned block per batch, a non-blocking copy
                rec = torch.empty((B, 4), dtype=torch.int32, pin_memory=self._kind == L.GS_DEV_HIP)
                rec.numpy()[...] = self.mix.records(B, self.oh, self.ow)
                drec = rec.to(self.device, non_blocking=True) if self._kind == L.GS_DEV_HIP else rec
                labels_b = torch.empty(B, dtype=torch.int64, device=self.device)
                lam = torch.empty(B, dtype=torch.float32, device=self.device)
                L.check(L.lib().gs_image_augment_mix(self._kind, self.device.index or 0, ds.images.data_ptr(),
                                                      ds.labels.data_ptr(), ds.n, ds.H, ds.W, ds.C,
                                                      self.transform.pad, self.oh, self.ow, dparams.data_ptr(),
                                                      drec.data_ptr(), B, out.data_ptr(),
                                                      L.gs_dtype(self.out_dtype), layout, labels.data_ptr(),
                                                      labels_b.data_ptr(), lam.data_ptr(), stream),
                        "gs_image_augment_mix")
                yield out, MixedTarget(labels, labels_b, lam)
                continue
            L.check(L.lib().gs_image_augment(self._kind, self.device.index or 0, ds.images.data_ptr(),
                                              ds.labels.data_ptr(), ds.n, ds.H, ds.W, ds.C, self.transform.pad,
                                              self.oh, self.ow, dparams.data_ptr(), B, out.data_ptr(),
                                              L.gs_dtype(self.out_dtype), layout, labels.data_ptr(), stream),
                    "gs_image_augment")
            yield out, labels


def build_dataloader(batch_size: int, dataset_train: ImageDataset, dataset_test: ImageDataset | None = None,
                     **kw):
    """build_dataloader of R:resnet/pytorch_ddp/ddp_train.py:25-48 on device-resident data."""
    train = DeviceDataLoader(dataset_train, batch_size=batch_size, shuffle=False, drop_last=True,
                             sampler=DistributedSampler(dataset_train), transform=TRAIN_TRANSFORM, **kw)
    test = None
    if dataset_test is not None:
        test = DeviceDataLoader(dataset_test, batch_size=batch_size, shuffle=False, drop_last=False,
                                sampler=DistributedSampler(dataset_test), transform=TEST_TRANSFORM, **kw)
    return train, test
