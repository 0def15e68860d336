"""Jacobi-preconditioned (diagonal-Newton) training: the worker-gradient plan (csrc/kernels/grad_curv.hip).

A ``--precondition diag`` run trains ONE model of a scalar loss, and every worker message carries, next to the
gradient ``g = sum r_i x_i``, the diagonal of the loss Hessian ``h = sum l''(z_i) x_i^2`` from the same pass over X.
Both are linear in the partitions, so every gradient code encodes and decodes them with the same coefficients.  On the
device, and in every message, the vector is ``[2][ld_x]``: a blocked model (ops/blockplan.py has the layout, the tables
and the encoding) whose block 0 is the gradient and block 1 the curvature diagonal.  The model travels in the same
shape, block 0 beta and block 1 exact zeros; the kernel reads block 0 only.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

from .._ext import native
from ..models.losses import LEAST_SQUARES, LOGISTIC, SOFTMAX, SQUARED_HINGE, is_weighted
from .blockplan import MAX_LD, SUBS, BlockGradPlan  # noqa: F401 (the plan's limits)
from .grad import _residual_torch
from .precision import Precision

PRECISIONS = ("fp64", "fp32", "fp32x64")
LOSSES = (LOGISTIC, LEAST_SQUARES, SQUARED_HINGE)


def _curvature_torch(loss: int, z: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """l''(z) per row in z's dtype (models/losses.py curvature)."""
    if loss == LOGISTIC:
        s = torch.sigmoid(-(y * z))
        return s * (1.0 - s)
    if loss == SQUARED_HINGE:
        return torch.where(1.0 - y * z > 0, torch.full_like(z, 2.0), torch.zeros_like(z))
    return torch.full_like(z, 2.0)


class PrecondGradPlan(BlockGradPlan):
    """Gradient and Hessian diagonal of every local message for one model over dense partitions.

    partitions: {partition_index: (X [rows, ld_x] storage dtype, y [rows] acc dtype)}
    messages:   sequence of segments [(partition_index, coef), ...]
    beta: [2 * ld_x], the model in block 0 (block 1 is not read); every message row: [2 * ld_x], block 0 the
    gradient and block 1 the curvature diagonal.
    """

    who = "preconditioned"  # the prefix of the plan's own errors, as GradLauncher.precond's; the limits name the flag

    @staticmethod
    def check_supported(prec: Precision, loss: int, sparse: bool = False, ld_x: int = 0, gpu: bool = False) -> None:
        """The limits that do not depend on the data; each a ValueError that names the flag (also raised by
        the trainer before it loads anything)."""
        if loss == SOFTMAX:
            raise ValueError("--precondition: the softmax loss is not supported (logistic, least squares or "
                             "squared hinge)")
        if is_weighted(loss):
            raise ValueError("--precondition: class / sample weights are not supported")
        if loss not in LOSSES:
            raise ValueError(f"--precondition: unknown loss kind {loss} (logistic, least squares or squared hinge)")
        if prec.name == "bf16":
            raise ValueError("--precondition: bf16 storage is not supported (fp64, fp32 or fp32x64)")
        if prec.name not in PRECISIONS:
            raise ValueError(f"--precondition: {prec.name} storage is not supported (fp64, fp32 or fp32x64)")
        if sparse:
            raise ValueError("--precondition: sparse data sources are not supported (dense partitions only)")
        if gpu and ld_x > MAX_LD:
            raise ValueError(f"--precondition: rows of {ld_x} columns exceed the kernel's limit of {MAX_LD}")

    def __init__(self, messages: Sequence[Sequence[Tuple[int, float]]],
                 partitions: Dict[int, Tuple[torch.Tensor, torch.Tensor]], prec: Precision, loss: int, d: int):
        self.check_supported(prec, int(loss))
        self.loss = int(loss)
        super().__init__(messages, partitions, prec, 2, d)

    def _make_launcher(self):
        return native().GradLauncher.precond(self.prec.code, self.loss, self.segs, self.tasks, self.slab,
                                             self.part_task_begin, self.d_x, self.ld_x)

    def _grad_torch(self, X: torch.Tensor, y: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
        one = torch.tensor(1.0, dtype=B.dtype)
        z = X @ B[0]  # only block 0 of the model is beta
        return torch.stack([X.t() @ _residual_torch(self.loss, z, y, one), (X * X).t() @ _curvature_torch(self.loss, z, y)])
