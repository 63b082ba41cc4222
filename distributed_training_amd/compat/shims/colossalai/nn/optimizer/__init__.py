from distributed_training_amd.compat.colossalai import FusedLAMB, HybridAdam, Lamb  # noqa: F401
