"""One-vs-rest multi-class training: the worker-gradient plan (csrc/kernels/grad_ovr.hip).

The model is B [C, d_x]: C binary classifiers of one scalar loss (logistic or squared hinge), model k "class k
against the rest".  On the device, and in every message, it is class-major ``[C][ld_x]``: a blocked model whose
blocks are the classes (ops/blockplan.py has the layout, the tables and the encoding).  Labels are class indices held
as floats, as for softmax; model k sees ``+1`` where the label is k and ``-1`` elsewhere, formed in the kernel from
the one copy of the labels, so all C gradients come from one pass over X.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

from .._ext import native
from ..models.losses import LEAST_SQUARES, LOGISTIC, SOFTMAX, SQUARED_HINGE, is_weighted
from .blockplan import MAX_LD, SUBS, BlockGradPlan  # noqa: F401 (the plan's limits)
from .grad import _residual_torch
from .precision import Precision

MIN_CLASSES, MAX_CLASSES = 2, 8  # csrc/kernels/launchers.h kMinBlocks / kMaxBlocks
PRECISIONS = ("fp64", "fp32", "fp32x64")
LOSSES = (LOGISTIC, SQUARED_HINGE)


class OvrGradPlan(BlockGradPlan):
    """One-vs-rest gradient of every local message over dense partitions.

    partitions: {partition_index: (X [rows, ld_x] storage dtype, y [rows] class indices, acc dtype)}
    messages:   sequence of segments [(partition_index, coef), ...]
    beta / every message row: [C * ld_x], the classifier of class k in block k.
    """

    who = "one-vs-rest"

    @staticmethod
    def check_supported(prec: Precision, loss: int, classes: int, sparse: bool = False, ld_x: int = 0,
                        gpu: bool = False) -> None:
        """The limits that do not depend on the data; each a ValueError that names the limit (also raised by
        the trainer before it loads anything)."""
        if not MIN_CLASSES <= int(classes) <= MAX_CLASSES:
            raise ValueError(f"one-vs-rest: classes must be in {MIN_CLASSES}..{MAX_CLASSES}, got {classes}")
        if loss == LEAST_SQUARES:
            raise ValueError("one-vs-rest: the least squares loss is not supported (logistic or squared hinge)")
        if loss == SOFTMAX:
            raise ValueError("one-vs-rest: the softmax loss is not supported (it has its own plan; logistic or "
                             "squared hinge)")
        if is_weighted(loss):
            raise ValueError("one-vs-rest: class / sample weights are not supported (the labels are class indices "
                             "and cannot carry a weight)")
        if loss not in LOSSES:
            raise ValueError(f"one-vs-rest: unknown loss kind {loss} (logistic or squared hinge)")
        if prec.name == "bf16":
            raise ValueError("one-vs-rest: bf16 storage is not supported (fp64, fp32 or fp32x64)")
        if prec.name not in PRECISIONS:
            raise ValueError(f"one-vs-rest: {prec.name} storage is not supported (fp64, fp32 or fp32x64)")
        if sparse:
            raise ValueError("one-vs-rest: sparse data sources are not supported (dense partitions only)")
        if gpu:
            OvrGradPlan.check_ld(ld_x)

    def __init__(self, messages: Sequence[Sequence[Tuple[int, float]]],
                 partitions: Dict[int, Tuple[torch.Tensor, torch.Tensor]], prec: Precision, loss: int, classes: int,
                 d: int):
        self.check_supported(prec, int(loss), classes)
        self.loss = int(loss)
        self.classes = int(classes)
        super().__init__(messages, partitions, prec, classes, d)

    def _check_labels(self, p: int, y: torch.Tensor) -> None:
        if y.numel() and not bool(((y >= 0) & (y < self.classes) & (y == torch.floor(y))).all()):
            raise ValueError(f"one-vs-rest: partition {p} has labels that are not integers in [0, {self.classes})")

    def _make_launcher(self):
        return native().GradLauncher.ovr(self.prec.code, self.loss, self.classes, self.segs, self.tasks, self.slab,
                                         self.part_task_begin, self.d_x, self.ld_x)

    def _grad_torch(self, X: torch.Tensor, y: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
        one = torch.tensor(1.0, dtype=B.dtype)  # the scalar-loss gradient of the dense plan's torch path, per class
        pos, neg = torch.ones_like(y), -torch.ones_like(y)
        return torch.stack([X.t() @ _residual_torch(self.loss, X @ B[k], torch.where(y == k, pos, neg), one)
                            for k in range(self.classes)])
