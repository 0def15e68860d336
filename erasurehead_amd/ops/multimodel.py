"""Several models of one scalar loss per pass over X: the worker-gradient plan of an (alpha, lr) sweep
(csrc/kernels/grad_multimodel.hip).

The M models of a sweep differ only in their update coefficients, so at every round their gradients
differ only through beta.  On the device, and in every message, the model is model-major ``[M][ld_x]``
with ``ld_x = prec.ld(d_x)``, flattened to ``D = M * ld_x`` elements -- the layout, and the rules, of
softmax's ``[C][ld_x]`` (ops/softmax.py): padding columns of every block are zero in beta_0 and in every
gradient, so they stay zero, and the rest of the engine sees one vector of length D.

Like the softmax plan, the kernel computes every DISTINCT local partition's gradient once with
coefficient 1 into ``Gb [nparts][D]`` (one pass over X whatever M is) and the device encoding forms the
messages; a plan whose messages are exactly the partitions with coefficient 1 (naive) writes G directly.
On CPU tensors the same math runs in torch, at any width.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

from .._ext import native
from ..models.losses import LEAST_SQUARES, LOGISTIC, SQUARED_HINGE
from .grad import _residual_torch
from .precision import Precision
from .softmax import SoftmaxGradPlan

MIN_MODELS, MAX_MODELS = 2, 8  # csrc/kernels/launchers.h kModelsMin / kModelsMax
MAX_LD = 1024  # kModelsMaxLd: 16 columns per lane
SUBS = 4  # kModelsSubs: slab rows (waves) per task
PRECISIONS = ("fp64", "fp32", "fp32x64")
LOSSES = (LOGISTIC, LEAST_SQUARES, SQUARED_HINGE)


class MultiModelGradPlan:
    """Gradient of every local message for M models at once over dense partitions.

    partitions: {partition_index: (X [rows, ld_x] storage dtype, y [rows] acc dtype)}
    messages:   sequence of segments [(partition_index, coef), ...]
    beta / every message row: [M * ld_x], model k in block k.
    """

    @staticmethod
    def check_supported(prec: Precision, loss: int, models: int, sparse: bool = False, ld_x: int = 0,
                        gpu: bool = False) -> None:
        """The limits that do not depend on the data; each a ValueError that names the limit (also raised by
        the trainer before it loads anything)."""
        if not MIN_MODELS <= int(models) <= MAX_MODELS:
            raise ValueError(f"multi-model: models must be in {MIN_MODELS}..{MAX_MODELS}, got {models}")
        if loss not in LOSSES:
            raise ValueError("multi-model: the loss must be logistic, least squares or squared hinge "
                             "(softmax has its own plan)")
        if prec.name not in PRECISIONS:
            raise ValueError(f"multi-model: {prec.name} storage is not supported (fp64, fp32 or fp32x64)")
        if sparse:
            raise ValueError("multi-model: sparse data sources are not supported (dense partitions only)")
        if gpu and ld_x > MAX_LD:
            raise ValueError(f"multi-model: rows of {ld_x} columns exceed the kernel's limit of {MAX_LD}")

    def __init__(self, messages: Sequence[Sequence[Tuple[int, float]]],
                 partitions: Dict[int, Tuple[torch.Tensor, torch.Tensor]], prec: Precision, loss: int, models: int,
                 d: int):
        self.prec = prec
        self.loss = int(loss)
        self.models = int(models)
        self.d_x = int(d)
        self.ld_x = prec.ld(self.d_x)
        self.d = self.ld = self.models * self.ld_x  # the flattened model, as the engine sees it
        self.messages = [list(m) for m in messages]
        self.nslots = len(self.messages)
        self.partitions = partitions
        for p, (X, y) in partitions.items():
            if not isinstance(X, torch.Tensor) or X.layout != torch.strided:
                raise ValueError(f"multi-model: partition {p} is sparse; only dense partitions are supported")
        any_t = next(iter(partitions.values()))[0] if partitions else torch.empty(0)
        self.device = any_t.device
        self.check_supported(prec, self.loss, self.models, False, self.ld_x, self.device.type == "cuda")
        self.basis = sorted({p for m in self.messages for p, _ in m})
        for p in self.basis:
            X, y = partitions[p]
            if X.dim() != 2 or X.shape[1] != self.ld_x or X.dtype != prec.storage or not X.is_contiguous():
                raise ValueError(f"partition {p}: X must be contiguous [rows, {self.ld_x}] {prec.storage}")
            if y.shape[0] != X.shape[0] or y.dtype != prec.acc or not y.is_contiguous():
                raise ValueError(f"partition {p}: y must be contiguous [{X.shape[0]}] {prec.acc}")
        pos = {p: j for j, p in enumerate(self.basis)}
        self.total_rows = sum(partitions[p][0].shape[0] for m in self.messages for p, _ in m)
        # identity: the messages are the distinct partitions with coefficient 1 -> no encode launch
        self.identity = all(len(m) == 1 and m[0][1] == 1.0 and pos[m[0][0]] == s
                            for s, m in enumerate(self.messages)) and self.nslots == len(self.basis)
        ptr, idx, coef = [0], [], []
        for m in self.messages:
            for p, c in m:
                idx.append(pos[p])
                coef.append(float(c))
            ptr.append(len(idx))
        self.E = torch.zeros((self.nslots, len(self.basis)), dtype=torch.float64)
        for s in range(self.nslots):
            for k in range(ptr[s], ptr[s + 1]):
                self.E[s, idx[k]] += coef[k]
        self._launcher = None
        if self.device.type == "cuda":
            dev = self.device
            self.enc_ptr = torch.tensor(ptr, dtype=torch.int32, device=dev)
            self.enc_idx = torch.tensor(idx or [0], dtype=torch.int32, device=dev)[: len(idx)]
            self.enc_coef = torch.tensor(coef or [0.0], dtype=torch.float64, device=dev)[: len(coef)]
            self.Gb = torch.zeros((len(self.basis), self.ld), dtype=prec.acc, device=dev)
            # one segment per distinct partition, row tasks of about two per CU, part_task_begin, the slab
            # [ntasks][4][D]: the softmax plan's tables, built by its code (it reads basis / partitions / ld)
            SoftmaxGradPlan._build_tables(self)

    def out_buffer(self, n: int = 1) -> torch.Tensor:
        """Message buffer(s) [n, nslots, D] in the accumulator dtype."""
        return torch.zeros((n, self.nslots, self.ld), dtype=self.prec.acc, device=self.device)

    def native_launcher(self):
        """C++ GradLauncher (csrc/runtime/grad_launcher.h, kind 4) for the native round executors."""
        if self.device.type != "cuda":
            raise RuntimeError("native launchers need GPU tensors")
        if self._launcher is None:
            L = native().GradLauncher.multimodel(self.prec.code, self.loss, self.models, self.segs, self.tasks,
                                                 self.slab, self.part_task_begin, self.d_x, self.ld_x)
            if not self.identity:
                L.set_encode(self.enc_ptr, self.enc_idx, self.enc_coef, self.Gb)
            self._launcher = L
        return self._launcher

    def run(self, beta: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
        """G[slot] block k = gradient of message slot at beta block k (beta: [D] acc dtype, model-major)."""
        if G.shape != (self.nslots, self.ld):
            raise ValueError(f"G must be [{self.nslots}, {self.ld}]")
        if self.device.type == "cuda":
            self.native_launcher().launch(beta, G)  # the gradient into Gb, then encode_messages (identity: into G)
            return G
        acc = self.prec.acc
        B = beta.to(acc).reshape(self.models, self.ld_x)
        one = torch.tensor(1.0, dtype=acc)
        Gb = torch.zeros((len(self.basis), self.models, self.ld_x), dtype=acc)
        for j, p in enumerate(self.basis):
            X, y = self.partitions[p]
            Xa = X.to(acc)
            for k in range(self.models):  # the scalar-loss gradient of the dense plan's torch path, per model
                Gb[j, k] = Xa.t() @ _residual_torch(self.loss, Xa @ B[k], y, one)
        G.copy_((self.E.to(acc) @ Gb.reshape(len(self.basis), self.ld)).to(G.dtype))
        return G

    @property
    def bytes_per_round(self) -> int:
        """Bytes of X the messages cover per round (replicas counted each time; once for all M models)."""
        return int(self.total_rows) * self.ld_x * self.prec.storage_bytes

    @property
    def distinct_bytes(self) -> int:
        """Bytes of the distinct partitions: what the kernel streams from HBM per round."""
        rows = sum(self.partitions[p][0].shape[0] for p in self.basis)
        return int(rows) * self.ld_x * self.prec.storage_bytes
