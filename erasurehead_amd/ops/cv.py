"""K-fold cross-validation: the worker-gradient plan (csrc/kernels/grad_folds.hip).

The K fold models of a ``--cv K`` run are K models of one scalar loss that share one (alpha, lr, l1); they differ from a
sweep's models in one respect: model k does not see the rows of fold k.  Row i of a partition (its position in the
partition, from 0) belongs to fold ``i mod K`` -- the task, the stage and the rank never enter, so every replica of a
partition holds out the same rows on every worker, which a coded scheme's decode needs.  On the device, and in every
message, the model is model-major ``[K][ld_x]``: a blocked model whose blocks are the fold models (ops/blockplan.py
has the layout, the tables and the encoding).
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch

from .._ext import native
from ..models.losses import LEAST_SQUARES, LOGISTIC, SOFTMAX, SQUARED_HINGE, is_weighted
from .blockplan import MAX_LD, SUBS, BlockGradPlan  # noqa: F401 (the plan's limits)
from .grad import _residual_torch
from .precision import Precision

MIN_FOLDS, MAX_FOLDS = 2, 8  # csrc/kernels/launchers.h kMinBlocks / kMaxBlocks
PRECISIONS = ("fp64", "fp32", "fp32x64")
LOSSES = (LOGISTIC, LEAST_SQUARES, SQUARED_HINGE)


class CvGradPlan(BlockGradPlan):
    """Gradient of every local message for the K fold models at once over dense partitions.

    partitions: {partition_index: (X [rows, ld_x] storage dtype, y [rows] acc dtype)}
    messages:   sequence of segments [(partition_index, coef), ...]
    beta / every message row: [K * ld_x], fold model k in block k; block k of a message sums over the rows whose fold
    is not k.
    """

    who = "--cv"

    @staticmethod
    def fold_rows(n_p: int, K: int) -> List[int]:
        """[ceil((n_p - k) / K) for k in 0..K-1]: the rows of a partition of n_p rows that belong to fold k."""
        n_p, K = int(n_p), int(K)
        return [max(0, -(-(n_p - k) // K)) for k in range(K)]

    @staticmethod
    def check_supported(prec: Precision, loss: int, folds: int, sparse: bool = False, ld_x: int = 0,
                        gpu: bool = False) -> None:
        """The limits that do not depend on the data; each a ValueError that names the limit (also raised by
        the trainer before it loads anything)."""
        if not MIN_FOLDS <= int(folds) <= MAX_FOLDS:
            raise ValueError(f"--cv: folds must be in {MIN_FOLDS}..{MAX_FOLDS}, got {folds}")
        if loss == SOFTMAX:
            raise ValueError("--cv: the softmax loss is not supported (logistic, least squares or "
                             "squared hinge)")
        if is_weighted(loss):
            raise ValueError("--cv: class / sample weights are not supported")
        if loss not in LOSSES:
            raise ValueError(f"--cv: unknown loss kind {loss} (logistic, least squares or squared hinge)")
        if prec.name == "bf16":
            raise ValueError("--cv: bf16 storage is not supported (fp64, fp32 or fp32x64)")
        if prec.name not in PRECISIONS:
            raise ValueError(f"--cv: {prec.name} storage is not supported (fp64, fp32 or fp32x64)")
        if sparse:
            raise ValueError("--cv: sparse data sources are not supported (dense partitions only)")
        if gpu:
            CvGradPlan.check_ld(ld_x)

    def __init__(self, messages: Sequence[Sequence[Tuple[int, float]]],
                 partitions: Dict[int, Tuple[torch.Tensor, torch.Tensor]], prec: Precision, loss: int, folds: int,
                 d: int):
        self.check_supported(prec, int(loss), folds)
        self.loss = int(loss)
        self.folds = int(folds)
        super().__init__(messages, partitions, prec, folds, d)

    def _make_launcher(self):
        return native().GradLauncher.folds(self.prec.code, self.loss, self.folds, self.segs, self.tasks, self.slab,
                                           self.part_task_begin, self.d_x, self.ld_x)

    def _grad_torch(self, X: torch.Tensor, y: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
        one = torch.tensor(1.0, dtype=B.dtype)  # the scalar-loss gradient of the dense plan's torch path, per fold model
        fold = torch.arange(X.shape[0]) % self.folds
        out = []
        for k in range(self.folds):
            keep = fold != k  # the held-out rows are left out, not zeroed: a non-finite held-out row cannot enter
            Xk = X[keep]
            out.append(Xk.t() @ _residual_torch(self.loss, Xk @ B[k], y[keep], one))
        return torch.stack(out)
