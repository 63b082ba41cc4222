from distributed_training_amd.compat.colossalai import DistributedLamb, FusedLAMB, HybridAdam, Lamb  # noqa: F401
