"""distributed_training_amd — MI355X-native data-parallel gradient-synchronisation
engine (libgsync) behind the reference's DDP / DeepSpeed / ColossalAI wrappers.

Public surface:
  DistributedDataParallel   drop-in for torch.nn.parallel.DistributedDataParallel
  FusedSGD / FusedAdam / FusedAdamW / FusedLARS / FusedLAMB / clip_grad_norm_
  Communicator              libgsync-owned RCCL communicator
  CapturedStep              the whole training step recorded into one hipGraph
  AveragedModel / ShardedAveragedModel / get_ema_multi_avg_fn / get_swa_multi_avg_fn
                            fused EMA / SWA weight averaging (torch.optim.swa_utils drop-ins)
  Metrics / evaluate        distributed evaluation: exact metrics kept on the device, every dataset
                            sample counted once, the fused inference BatchNorm forward
  CrossEntropyLoss / cross_entropy  the fused training criterion (label smoothing, fp32 loss, gradient
                            in the logits' dtype), optionally advancing a Metrics on the device
  MixUpCutMix / MixedTarget  MixUp and CutMix inside the device input kernel (data.DeviceDataLoader(mix=...))
                            and the pair targets the criterion takes in place of labels
  RandomResizedCropFlip / ResizeCenterCrop  the resize-based input transforms (RandomResizedCrop + flip, or
                            Resize + CenterCrop, + ToTensor + Normalize) as one launch per batch
                            (data.DeviceDataLoader(transform=...))
  compat.deepspeed / compat.colossalai  API shims for the other two trainers
"""
from . import _lib  # noqa: F401
from .comm import Communicator, destroy_communicators, get_communicator  # noqa: F401
from .ddp import DDP, DistributedDataParallel, GradBucket, compute_bucket_assignment_by_size  # noqa: F401
from .graphs import CapturedStep  # noqa: F401
from .ema import AveragedModel, ShardedAveragedModel, get_ema_multi_avg_fn, get_swa_multi_avg_fn  # noqa: F401
from .data import MixedTarget, MixUpCutMix, RandomResizedCropFlip, ResizeCenterCrop  # noqa: F401
from .evaluation import Metrics, evaluate  # noqa: F401
from .loss import CrossEntropyLoss, cross_entropy  # noqa: F401
from .flatten import copy_flat_to, flatten_dense_tensors, unflatten_dense_tensors  # noqa: F401
from .multi_tensor import TensorListPlan  # noqa: F401
from .optim import FusedAdam, FusedAdamW, FusedLAMB, FusedLARS, FusedSGD, clip_grad_norm_  # noqa: F401

__version__ = "0.1.0"
