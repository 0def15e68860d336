"""The worker-gradient plan of a blocked model: what the softmax plan (blocks = classes, ops/softmax.py) and the
multi-model plan (blocks = models of an (alpha, lr) sweep, ops/multimodel.py) share.

On the device, and in every message, the model is block-major ``[blocks][ld_x]`` with ``ld_x = prec.ld(d_x)``,
flattened to ``D = blocks * ld_x`` elements.  The padding columns of every block are zero in beta_0 and in every
gradient, so they stay zero, and the rest of the engine (transport, integrity tags, collector, combine + update,
checkpoints) sees one vector of length D.

Like the sparse plan, the kernel computes every DISTINCT local partition's gradient once with coefficient 1 into
``Gb [nparts][D]`` (one pass over X whatever the number of blocks) and the device encoding forms the messages,
``G[slot] = sum coef * Gb[idx]``; a plan whose messages are exactly the partitions with coefficient 1 (naive) writes
G directly.  On CPU tensors the same math runs in torch, at any width.

A subclass names itself in ``who`` (the prefix of its error texts) and gives ``_make_launcher`` (its native
GradLauncher) and ``_grad_torch`` (one partition's gradient in torch); ``_check_labels`` is its to refine.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from .grad import _SEG, N_CUS
from .precision import Precision

MAX_LD = 1024  # csrc/kernels/launchers.h kBlockMaxLd: 16 columns per lane
SUBS = 4  # kBlockSubs: slab rows (waves) per task
TASKS_PER_CU = 2  # workgroups of 4 waves and <= 67 KiB of LDS: two per CU
MIN_ROWS_PER_TASK = 64


def stage_rows(rowbytes: int) -> int:
    """Rows per LDS stage: a mirror of csrc/kernels/grad_blocks.h blocks_stage_rows (about 32 KiB, 4..32 rows)."""
    return min(32, max(4, 32768 // int(rowbytes)))


def waves_per_group(blocks: int) -> int:
    """Waves that share one pair of blocks and split a stage's rows: a mirror of grad_blocks.h blocks_wpg
    (2 blocks -> 4, 3 or 4 -> 2, 5..8 -> 1)."""
    return SUBS // ((int(blocks) + 1) // 2)


class BlockGradPlan:
    """Gradient of every local message for a model of ``blocks`` blocks over dense partitions.

    partitions: {partition_index: (X [rows, ld_x] storage dtype, y [rows] acc dtype)}
    messages:   sequence of segments [(partition_index, coef), ...]
    beta / every message row: [blocks * ld_x], block k at [k * ld_x, (k + 1) * ld_x).
    """

    who = "blocked model"

    @classmethod
    def check_ld(cls, ld_x: int) -> None:
        if ld_x > MAX_LD:
            raise ValueError(f"{cls.who}: rows of {ld_x} columns exceed the kernel's limit of {MAX_LD}")

    def __init__(self, messages: Sequence[Sequence[Tuple[int, float]]],
                 partitions: Dict[int, Tuple[torch.Tensor, torch.Tensor]], prec: Precision, blocks: int, d: int):
        self.prec = prec
        self.blocks = int(blocks)
        self.d_x = int(d)
        self.ld_x = prec.ld(self.d_x)
        self.d = self.ld = self.blocks * self.ld_x  # the flattened model, as the engine sees it
        self.messages = [list(m) for m in messages]
        self.nslots = len(self.messages)
        self.partitions = partitions
        for p, (X, y) in partitions.items():
            if not isinstance(X, torch.Tensor) or X.layout != torch.strided:
                raise ValueError(f"{self.who}: partition {p} is sparse; only dense partitions are supported")
        any_t = next(iter(partitions.values()))[0] if partitions else torch.empty(0)
        self.device = any_t.device
        if self.device.type == "cuda":
            self.check_ld(self.ld_x)
        self.basis = sorted({p for m in self.messages for p, _ in m})
        for p in self.basis:  # the kernels read X and y with raw LDS-DMA: both contiguous
            X, y = partitions[p]
            if X.dim() != 2 or X.shape[1] != self.ld_x or X.dtype != prec.storage or not X.is_contiguous():
                raise ValueError(f"partition {p}: X must be contiguous [rows, {self.ld_x}] {prec.storage}")
            if y.shape[0] != X.shape[0] or y.dtype != prec.acc or not y.is_contiguous():
                raise ValueError(f"partition {p}: y must be contiguous [{X.shape[0]}] {prec.acc}")
            self._check_labels(p, y)
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
            self._build_tables()

    def _check_labels(self, p: int, y: torch.Tensor) -> None:
        """What a subclass requires of partition p's labels (a ValueError naming the partition)."""

    def _make_launcher(self):
        """The plan's C++ GradLauncher (csrc/runtime/grad_launcher.cpp make_blocked), without the encoding."""
        raise NotImplementedError

    def _grad_torch(self, X: torch.Tensor, y: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
        """[blocks, ld_x]: one partition's gradient with coefficient 1 at B [blocks, ld_x], X in B's dtype."""
        raise NotImplementedError

    def _build_tables(self):
        """One segment per distinct partition; its rows split into tasks (one workgroup each, about two
        per CU over the whole plan), tasks of a partition contiguous: part_task_begin."""
        rows = sum(self.partitions[p][0].shape[0] for p in self.basis)
        per_task = max(MIN_ROWS_PER_TASK, -(-rows // (TASKS_PER_CU * N_CUS)))
        segs = bytearray()
        tasks: List[Tuple[int, int, int, int, int]] = []
        begin = [0]
        for j, p in enumerate(self.basis):
            X, y = self.partitions[p]
            n = X.shape[0]
            segs += _SEG.pack(X.data_ptr(), y.data_ptr(), 1.0, n)
            bounds = (list(range(0, n, per_task)) or [0]) + [n]
            for r0, r1 in zip(bounds[:-1], bounds[1:]):
                tasks.append((j, j, r0, r1, len(tasks)))
            begin.append(len(tasks))
        dev = self.device
        self.segs = torch.tensor(list(bytes(segs) or b"\0" * 32), dtype=torch.uint8).to(dev)
        self.ntasks = len(tasks)
        self.tasks = torch.from_numpy(np.asarray(tasks, dtype=np.int32).reshape(-1, 5)).to(dev)
        self.part_task_begin = torch.tensor(begin, dtype=torch.int32, device=dev)
        self.slab = torch.empty((max(1, self.ntasks), SUBS, self.ld), dtype=self.prec.acc, device=dev)

    def out_buffer(self, n: int = 1) -> torch.Tensor:
        """Message buffer(s) [n, nslots, D] in the accumulator dtype."""
        return torch.zeros((n, self.nslots, self.ld), dtype=self.prec.acc, device=self.device)

    def native_launcher(self):
        """C++ GradLauncher (csrc/runtime/grad_launcher.h) for the native round executors."""
        if self.device.type != "cuda":
            raise RuntimeError("native launchers need GPU tensors")
        if self._launcher is None:
            L = self._make_launcher()
            if not self.identity:
                L.set_encode(self.enc_ptr, self.enc_idx, self.enc_coef, self.Gb)
            self._launcher = L
        return self._launcher

    def run(self, beta: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
        """G[slot] block k = gradient of message slot at beta block k (beta: [D] acc dtype, block-major)."""
        if G.shape != (self.nslots, self.ld):
            raise ValueError(f"G must be [{self.nslots}, {self.ld}]")
        if self.device.type == "cuda":
            self.native_launcher().launch(beta, G)  # the gradient into Gb, then encode_messages (identity: into G)
            return G
        acc = self.prec.acc
        B = beta.to(acc).reshape(self.blocks, self.ld_x)
        Gb = torch.zeros((len(self.basis), self.ld), dtype=acc)
        for j, p in enumerate(self.basis):
            X, y = self.partitions[p]
            Gb[j] = self._grad_torch(X.to(acc), y, B).reshape(-1)
        G.copy_((self.E.to(acc) @ Gb).to(G.dtype))
        return G

    @property
    def bytes_per_round(self) -> int:
        """Bytes of X the messages cover per round (replicas counted each time; once for all blocks)."""
        return int(self.total_rows) * self.ld_x * self.prec.storage_bytes

    @property
    def distinct_bytes(self) -> int:
        """Bytes of the distinct partitions: what the kernel streams from HBM per round."""
        rows = sum(self.partitions[p][0].shape[0] for p in self.basis)
        return int(rows) * self.ld_x * self.prec.storage_bytes
