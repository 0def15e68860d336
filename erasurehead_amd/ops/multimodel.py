"""Several models of one scalar loss per pass over X: the worker-gradient plan of an (alpha, lr) sweep
(csrc/kernels/grad_multimodel.hip).

The M models of a sweep differ only in their update coefficients, so at every round their gradients differ only
through beta.  On the device, and in every message, the model is model-major ``[M][ld_x]``: a blocked model whose
blocks are the models (ops/blockplan.py has the layout, the tables and the encoding).
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

from .._ext import native
from ..models.losses import LEAST_SQUARES, LOGISTIC, LOGISTIC_W, SQUARED_HINGE, SQUARED_HINGE_W, is_weighted
from .blockplan import MAX_LD, SUBS, BlockGradPlan  # noqa: F401 (the plan's limits)
from .grad import _residual_torch
from .precision import Precision

MIN_MODELS, MAX_MODELS = 2, 8  # csrc/kernels/launchers.h kMinBlocks / kMaxBlocks
PRECISIONS = ("fp64", "fp32", "fp32x64")
LOSSES = (LOGISTIC, LEAST_SQUARES, SQUARED_HINGE, LOGISTIC_W, SQUARED_HINGE_W)  # the weighted codes: CPU tensors only

# csrc/kernels/grad_multimodel.hip instantiates the three unweighted losses only
NO_WEIGHTED_KERNEL = ("multi-model: --class-weight / --sample-weights in a sweep (--alphas / --lrs / --l1s) run on CPU "
                      "tensors only: the multi-model GPU kernel has no weighted instance")


class MultiModelGradPlan(BlockGradPlan):
    """Gradient of every local message for M models at once over dense partitions.

    partitions: {partition_index: (X [rows, ld_x] storage dtype, y [rows] acc dtype)}
    messages:   sequence of segments [(partition_index, coef), ...]
    beta / every message row: [M * ld_x], model k in block k.
    """

    who = "multi-model"

    @staticmethod
    def check_supported(prec: Precision, loss: int, models: int, sparse: bool = False, ld_x: int = 0,
                        gpu: bool = False) -> None:
        """The limits that do not depend on the data; each a ValueError that names the limit (also raised by
        the trainer before it loads anything)."""
        if not MIN_MODELS <= int(models) <= MAX_MODELS:
            raise ValueError(f"multi-model: models must be in {MIN_MODELS}..{MAX_MODELS}, got {models}")
        if is_weighted(loss) and gpu:
            raise ValueError(NO_WEIGHTED_KERNEL)
        if loss not in LOSSES:
            raise ValueError("multi-model: the loss must be logistic, least squares or squared hinge "
                             "(softmax has its own plan)")
        if prec.name not in PRECISIONS:
            raise ValueError(f"multi-model: {prec.name} storage is not supported (fp64, fp32 or fp32x64)")
        if sparse:
            raise ValueError("multi-model: sparse data sources are not supported (dense partitions only)")
        if gpu:
            MultiModelGradPlan.check_ld(ld_x)

    def __init__(self, messages: Sequence[Sequence[Tuple[int, float]]],
                 partitions: Dict[int, Tuple[torch.Tensor, torch.Tensor]], prec: Precision, loss: int, models: int,
                 d: int):
        self.check_supported(prec, int(loss), models)
        if is_weighted(int(loss)) and any(X.is_cuda for X, _ in partitions.values()):
            raise ValueError(NO_WEIGHTED_KERNEL)
        self.loss = int(loss)
        self.models = int(models)
        super().__init__(messages, partitions, prec, models, d)

    def _make_launcher(self):
        return native().GradLauncher.multimodel(self.prec.code, self.loss, self.models, self.segs, self.tasks,
                                                self.slab, self.part_task_begin, self.d_x, self.ld_x)

    def _grad_torch(self, X: torch.Tensor, y: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
        one = torch.tensor(1.0, dtype=B.dtype)  # the scalar-loss gradient of the dense plan's torch path, per model
        return torch.stack([X.t() @ _residual_torch(self.loss, X @ B[k], y, one) for k in range(self.models)])
