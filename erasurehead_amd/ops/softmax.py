"""Multi-class softmax regression: the worker-gradient plan (csrc/kernels/grad_softmax.hip).

The model is B [C, d_x]; on the device, and in every message, it is class-major ``[C][ld_x]``: a blocked model
whose blocks are the classes (ops/blockplan.py has the layout, the tables and the encoding).  Labels are class
indices held as floats.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

from .._ext import native
from ..models.losses import MAX_CLASSES, MIN_CLASSES, SOFTMAX
from .blockplan import MAX_LD, MIN_ROWS_PER_TASK, SUBS, TASKS_PER_CU, BlockGradPlan  # noqa: F401 (the plan's limits)
from .precision import Precision


def softmax_grad_torch(X: torch.Tensor, y: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """[C, ld]: sum_rows (softmax(x B^T) - onehot(y)) x, coefficient 1, in B's dtype."""
    Z = X @ B.t()
    R = torch.softmax(Z, dim=1)
    R[torch.arange(X.shape[0]), y.long()] -= 1.0
    return R.t() @ X


class SoftmaxGradPlan(BlockGradPlan):
    """Softmax gradient of every local message over dense partitions.

    partitions: {partition_index: (X [rows, ld_x] storage dtype, y [rows] class indices, acc dtype)}
    messages:   sequence of segments [(partition_index, coef), ...]
    """

    who = "softmax"
    loss = SOFTMAX

    @staticmethod
    def check_supported(prec: Precision, classes: int, sparse: bool = False) -> None:
        """The limits that do not depend on the data; each a ValueError that names the limit (also raised
        by the trainer before it loads anything)."""
        if not MIN_CLASSES <= int(classes) <= MAX_CLASSES:
            raise ValueError(f"softmax: classes must be in {MIN_CLASSES}..{MAX_CLASSES}, got {classes}")
        if prec.name == "bf16":
            raise ValueError("softmax: bf16 storage is not supported (fp64 or fp32)")
        if prec.name == "fp32x64":  # the multi-class kernel has no fp32-storage, fp64-accumulator instance yet
            raise ValueError("softmax: fp32x64 (fp32 storage, fp64 arithmetic) is not supported (fp64 or fp32)")
        if sparse:
            raise ValueError("softmax: sparse data sources are not supported (dense partitions only)")

    def __init__(self, messages: Sequence[Sequence[Tuple[int, float]]],
                 partitions: Dict[int, Tuple[torch.Tensor, torch.Tensor]], prec: Precision, classes: int, d: int):
        self.check_supported(prec, classes)
        self.classes = int(classes)
        super().__init__(messages, partitions, prec, classes, d)

    def _check_labels(self, p: int, y: torch.Tensor) -> None:
        if y.numel() and not bool(((y >= 0) & (y < self.classes) & (y == torch.floor(y))).all()):
            raise ValueError(f"softmax: partition {p} has labels that are not integers in [0, {self.classes})")

    def _make_launcher(self):
        return native().GradLauncher.softmax(self.prec.code, self.classes, self.segs, self.tasks, self.slab,
                                             self.part_task_begin, self.d_x, self.ld_x)

    def _grad_torch(self, X: torch.Tensor, y: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
        return softmax_grad_torch(X, y, B)
