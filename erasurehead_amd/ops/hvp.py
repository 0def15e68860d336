"""Truncated Newton (Newton-CG) training: the worker-gradient plan (csrc/kernels/grad_hvp.hip).

A ``--newton-cg J`` run trains ONE model of a scalar loss, and every worker message carries, next to the gradient
``g = sum r_i x_i``, the loss Hessian applied to the master's conjugate-gradient direction,
``u = sum l''(z_i) (x_i . v) x_i``, from the same pass over X.  Both are linear in the partitions, so every gradient
code encodes and decodes them with the same coefficients.  On the device, and in every message, the vector is
``[2][ld_x]``: a blocked model (ops/blockplan.py has the layout, the tables and the encoding) whose block 0 is the
gradient and block 1 the product.  The model travels in the same shape, block 0 beta and block 1 the direction v
(exact zeros in a gradient round, which then returns exact zeros in block 1).
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

from .._ext import native
from ..models.losses import LEAST_SQUARES, LOGISTIC, SOFTMAX, SQUARED_HINGE, is_weighted
from .blockplan import MAX_LD, BlockGradPlan
from .grad import _residual_torch
from .precision import Precision
from .precond import _curvature_torch

PRECISIONS = ("fp64", "fp32", "fp32x64")
LOSSES = (LOGISTIC, LEAST_SQUARES, SQUARED_HINGE)


class HvpGradPlan(BlockGradPlan):
    """Gradient and Hessian-vector product of every local message for one model over dense partitions.

    partitions: {partition_index: (X [rows, ld_x] storage dtype, y [rows] acc dtype)}
    messages:   sequence of segments [(partition_index, coef), ...]
    beta: [2 * ld_x], the model in block 0 and the direction v in block 1; every message row: [2 * ld_x], block 0 the
    gradient and block 1 the loss Hessian applied to v.
    """

    who = "newton-cg"  # the prefix of the plan's own errors, as GradLauncher.hvp's; the limits name the flag

    @staticmethod
    def check_supported(prec: Precision, loss: int, sparse: bool = False, ld_x: int = 0, gpu: bool = False) -> None:
        """The limits that do not depend on the data; each a ValueError that names the flag (also raised by
        the trainer before it loads anything)."""
        if loss == SOFTMAX:
            raise ValueError("--newton-cg: the softmax loss is not supported (logistic, least squares or "
                             "squared hinge)")
        if is_weighted(loss):
            raise ValueError("--newton-cg: class / sample weights are not supported")
        if loss not in LOSSES:
            raise ValueError(f"--newton-cg: unknown loss kind {loss} (logistic, least squares or squared hinge)")
        if prec.name not in PRECISIONS:
            raise ValueError(f"--newton-cg: {prec.name} storage is not supported (fp64, fp32 or fp32x64)")
        if sparse:
            raise ValueError("--newton-cg: sparse data sources are not supported (dense partitions only)")
        if gpu and ld_x > MAX_LD:
            raise ValueError(f"--newton-cg: rows of {ld_x} columns exceed the kernel's limit of {MAX_LD}")

    def __init__(self, messages: Sequence[Sequence[Tuple[int, float]]],
                 partitions: Dict[int, Tuple[torch.Tensor, torch.Tensor]], prec: Precision, loss: int, d: int):
        self.check_supported(prec, int(loss))
        self.loss = int(loss)
        super().__init__(messages, partitions, prec, 2, d)

    def _make_launcher(self):
        return native().GradLauncher.hvp(self.prec.code, self.loss, self.segs, self.tasks, self.slab,
                                         self.part_task_begin, self.d_x, self.ld_x)

    def _grad_torch(self, X: torch.Tensor, y: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
        one = torch.tensor(1.0, dtype=B.dtype)
        z = X @ B[0]
        return torch.stack([X.t() @ _residual_torch(self.loss, z, y, one),
                            X.t() @ (_curvature_torch(self.loss, z, y) * (X @ B[1]))])
