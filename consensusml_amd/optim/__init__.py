"""Fused optimizers over flat buffers (one HIP launch per parameter group and dtype)."""
from .fused import FusedAdam, FusedAdamW, FusedLAMB, FusedLARS, FusedSGD, build_optimizer

__all__ = ["FusedSGD", "FusedAdam", "FusedAdamW", "FusedLARS", "FusedLAMB",
           "build_optimizer"]
