"""Data sources: where worker partitions and the evaluation sets come from.

* :class:`FileSource`      — the reference on-disk layout (text ``.dat`` / CSR ``.npz``);
* :class:`SyntheticSource` — the reference GMM model drawn directly on the device;
* :class:`ArraySource`     — in-memory arrays (tests, notebooks);
* :class:`WeightedSource`  — any of them with class / sample weights carried by the labels.

Every source hands out partitions by 0-based index, already in the worker layout:
dense X as a contiguous ``[rows, ld]`` tensor in the storage precision (zero-padded
columns), labels in the accumulator precision; sparse X as ``scipy.sparse.csr_matrix``.
Labels of partition p are rows ``[p*rpw, (p+1)*rpw)`` of the full label vector, exactly
like the reference's slicing (ref src/replication.py:52).
"""
from __future__ import annotations

import hashlib
import os
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..ops.precision import Precision
from . import io as dio
from .synthetic import DeviceGMM


def _pad_dense(X, prec: Precision, device, rounding: Optional[List[float]] = None) -> torch.Tensor:
    """rounding: a one-element list holding the largest |x - fl(x)| / |x| so far of the fp64 originals rounded
    to the storage precision; updated with this array's (DataSource.storage_max_rel_rounding)."""
    if not isinstance(X, torch.Tensor):  # memory-mapped .npy twins are read-only: copy those
        X = torch.from_numpy(np.require(np.asarray(X, dtype=np.float64), requirements=["W", "C"]))
    if X.dim() == 1:
        X = X[None, :]
    n, d = X.shape
    ld = prec.ld(d)
    out = torch.zeros((n, ld), dtype=prec.storage, device=device)
    X64 = X.to(device=device, dtype=torch.float64)
    out[:, :d] = X64.to(prec.storage)
    if rounding is not None and prec.storage != torch.float64 and X64.numel():
        err = (X64 - out[:, :d].double()).abs() / X64.abs()  # 0 / 0 (an exact zero) is no rounding
        rounding[0] = max(rounding[0], float(torch.nan_to_num(err, nan=0.0, posinf=float("inf")).max()))
    return out


class DataSource:
    is_sparse = False
    d: int
    # largest |x - fl(x)| / |x| over the dense training rows handed out by partition() so far, for sources that
    # hold fp64 originals (0.0: the storage precision holds them exactly); None: drawn directly in the storage
    # precision, or sparse (kept in the accumulator precision)
    storage_max_rel_rounding: Optional[float] = None

    def _padded_partition(self, X, prec: Precision, device) -> torch.Tensor:
        r = [self.storage_max_rel_rounding or 0.0]
        out = _pad_dense(X, prec, device, r)
        self.storage_max_rel_rounding = r[0]
        return out

    def partition(self, p: int, prec: Precision, device):
        raise NotImplementedError

    def train_eval_chunks(self, parts: Sequence[int], prec: Precision, device) -> Iterator[Tuple[object, torch.Tensor]]:
        """(X, y) of the given partitions, in order, labels taken from the *prefix* of label.dat."""
        raise NotImplementedError

    def test(self, prec: Precision, device) -> Tuple[object, torch.Tensor]:
        raise NotImplementedError


class FileSource(DataSource):
    def __init__(self, data_dir: str, is_real: int, rows_per_partition: int, n_cols: int):
        self.data_dir = data_dir
        self.is_real = int(is_real)
        self.is_sparse = bool(is_real)
        self.rpw = int(rows_per_partition)
        self.d = int(n_cols)
        self._labels: Optional[np.ndarray] = None

    def labels(self) -> np.ndarray:
        if self._labels is None:
            self._labels = dio.load_labels(self.data_dir)
        return self._labels

    def train_labels(self, p: int) -> np.ndarray:
        return np.asarray(self.labels()[p * self.rpw:(p + 1) * self.rpw], dtype=np.float64)

    def partition(self, p: int, prec: Precision, device):
        X = dio.load_partition(self.data_dir, p, self.is_real)
        y = self.labels()[p * self.rpw:(p + 1) * self.rpw]
        if X.shape[0] != len(y):
            raise ValueError(f"partition {p + 1}: {X.shape[0]} rows but {len(y)} labels; check n_rows")
        if self.is_sparse:
            return X, np.asarray(y, dtype=np.float64)
        return self._padded_partition(X, prec, device), torch.tensor(np.asarray(y), dtype=prec.acc, device=device)

    def train_eval_chunks(self, parts, prec, device):
        y = self.labels()
        off = 0
        for p in parts:
            X = dio.load_partition(self.data_dir, p, self.is_real)
            n = X.shape[0]
            yy = torch.tensor(np.asarray(y[off:off + n]), dtype=torch.float64, device=device)
            off += n
            yield (X if self.is_sparse else _pad_dense(X, prec, device)), yy

    def test(self, prec, device):
        X = dio.load_test(self.data_dir, self.is_real)
        y = torch.tensor(np.asarray(dio.load_labels(self.data_dir, test=True)), dtype=torch.float64, device=device)
        return (X if self.is_sparse else _pad_dense(X, prec, device)), y


class SyntheticSource(DataSource):
    """Partitions of the reference synthetic model generated on the device (no files)."""

    def __init__(self, n_rows: int, n_cols: int, n_partitions: int, seed: int = 0, classes: Optional[int] = None):
        self.gen = DeviceGMM(n_rows, n_cols, n_partitions, seed, classes=classes)
        self.d = n_cols

    def partition(self, p, prec, device):
        self.gen.ld = prec.ld(self.d)
        X, y = self.gen.partition(p, device=device, dtype=prec.storage)
        return X.contiguous(), y.to(prec.acc)

    def train_labels(self, p: int, device="cpu") -> np.ndarray:
        """Partition p's labels (the generator draws the rows with them: used once, for balanced class weights)."""
        return self.gen.partition(p, device=device)[1].double().cpu().numpy()

    def train_eval_chunks(self, parts, prec, device):
        self.gen.ld = prec.ld(self.d)
        for p in parts:
            X, y = self.gen.partition(p, device=device, dtype=prec.storage)
            yield X.contiguous(), y

    def test(self, prec, device):
        self.gen.ld = prec.ld(self.d)
        X, y = self.gen.test(device=device, dtype=prec.storage)
        return X.contiguous(), y


class ArraySource(DataSource):
    """parts: list of (X, y) numpy arrays or scipy CSR; test: (X, y).  weights: optionally one vector of sample
    weights per partition (the in-memory form of --sample-weights; the trainer then wraps the source in a
    :class:`WeightedSource`, the labels handed out here stay the plain ones)."""

    def __init__(self, parts: List[Tuple[object, np.ndarray]], test: Tuple[object, np.ndarray], sparse: bool = False,
                 weights: Optional[Sequence[np.ndarray]] = None):
        self.parts = parts
        self._test = test
        self.is_sparse = sparse
        self.d = parts[0][0].shape[1]
        self.weights = None
        if weights is not None:
            if len(weights) != len(parts):
                raise ValueError(f"sample weights: {len(weights)} vectors for {len(parts)} partitions")
            self.weights = [check_weights(w, len(y), f"sample weights of partition {p}")
                            for p, (w, (_, y)) in enumerate(zip(weights, parts))]

    def train_labels(self, p: int) -> np.ndarray:
        return np.asarray(self.parts[p][1], dtype=np.float64)

    def partition(self, p, prec, device):
        X, y = self.parts[p]
        if self.is_sparse:
            return X, np.asarray(y, dtype=np.float64)
        return self._padded_partition(X, prec, device), torch.tensor(np.asarray(y), dtype=prec.acc, device=device)

    def train_eval_chunks(self, parts, prec, device):
        ys = np.concatenate([np.asarray(y) for _, y in self.parts])
        off = 0
        for p in parts:
            X = self.parts[p][0]
            n = X.shape[0]
            yy = torch.as_tensor(ys[off:off + n], dtype=torch.float64, device=device)
            off += n
            yield (X if self.is_sparse else _pad_dense(X, prec, device)), yy

    def test(self, prec, device):
        X, y = self._test
        yy = torch.as_tensor(np.asarray(y), dtype=torch.float64, device=device)
        return (X if self.is_sparse else _pad_dense(X, prec, device)), yy


# ------------------------------------------------------------------ class / sample weights
def check_weights(w, n: int, what: str) -> np.ndarray:
    """A weight vector as fp64 [n]: finite and >= 0, else a ValueError that names ``what``."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if len(w) != n:
        raise ValueError(f"{what}: {len(w)} weights for {n} labels")
    if not bool(np.all(np.isfinite(w) & (w >= 0))):
        raise ValueError(f"{what}: every weight must be finite and >= 0 (negative, NaN or infinite weight found)")
    return w


def balanced_class_weights(n_pos: int, n_neg: int) -> Tuple[float, float]:
    """(w+, w-) = (n / (2 n+), n / (2 n-)): both classes get the same total weight n / 2."""
    if n_pos <= 0 or n_neg <= 0:
        raise ValueError(f"--class-weight balanced: a class has no training rows ({n_pos} positive, {n_neg} negative)")
    n = n_pos + n_neg
    return n / (2.0 * n_pos), n / (2.0 * n_neg)


class WeightedSource(DataSource):
    """A source whose labels carry the rows' weights: every label handed out is y~ = s * w with s the +-1 label
    of the wrapped source and w = class weight of s times the row's sample weight (csrc/kernels/common.h
    kLogisticW / kSquaredHingeW read the class from the sign bit and the weight from the magnitude, so a zero
    weight keeps its class as +0.0 / -0.0).

    class_weight: (w+, w-) or None.  sample: the full weight vector in label.dat's order (entry i belongs to label i
    wherever that label is used, the label prefix of train_eval_chunks included), or None; an ArraySource brings its
    own per-partition vectors (ArraySource.weights).  Test rows take the class weights only."""

    def __init__(self, inner: DataSource, class_weight: Optional[Tuple[float, float]] = None,
                 sample: Optional[np.ndarray] = None):
        self.inner = inner
        self.is_sparse = inner.is_sparse
        self.d = inner.d
        self.class_weight = None if class_weight is None else (float(class_weight[0]), float(class_weight[1]))
        per_part = getattr(inner, "weights", None)
        if per_part is not None and sample is not None:
            raise ValueError("sample weights: given both with the ArraySource and as a vector")
        self._per_part = per_part
        self._flat = np.concatenate(per_part) if per_part is not None else sample
        self._rpw = getattr(inner, "rpw", None)

    def __getattr__(self, name):  # data_dir, storage_max_rel_rounding, ...: the wrapped source's
        if name == "inner":
            raise AttributeError(name)
        return getattr(self.inner, name)

    def sample_sha256(self) -> Optional[str]:
        """SHA-256 of the sample-weight vector (fp64, label order); None without sample weights."""
        if self._flat is None:
            return None
        return hashlib.sha256(np.ascontiguousarray(self._flat, dtype=np.float64).tobytes()).hexdigest()

    def partition_weights(self, p: int, n: int) -> Optional[np.ndarray]:
        if self._per_part is not None:
            return self._per_part[p]
        if self._flat is None:
            return None
        w = self._flat[p * self._rpw:(p + 1) * self._rpw]
        if len(w) != n:
            raise ValueError(f"--sample-weights: {len(w)} weights for the {n} rows of partition {p + 1}")
        return w

    def weigh(self, y, w: Optional[np.ndarray] = None):
        """y~ = y * class weight * w for labels y in {-1, +1} (torch tensor or ndarray; same type and dtype back)."""
        wp, wn = self.class_weight or (1.0, 1.0)
        if isinstance(y, torch.Tensor):
            if bool(((y != 1) & (y != -1)).any()):
                raise ValueError("--class-weight / --sample-weights need labels in {-1, +1}")
            f64 = dict(dtype=torch.float64, device=y.device)
            t = torch.where(y > 0, torch.tensor(wp, **f64), torch.tensor(wn, **f64))
            if w is not None:
                t = t * torch.as_tensor(w, dtype=torch.float64, device=y.device)
            return (y.double() * t).to(y.dtype)
        y = np.asarray(y, dtype=np.float64)
        if bool(np.any((y != 1) & (y != -1))):
            raise ValueError("--class-weight / --sample-weights need labels in {-1, +1}")
        t = np.where(y > 0, wp, wn)
        return y * (t if w is None else t * w)

    def partition(self, p, prec, device):
        X, y = self.inner.partition(p, prec, device)
        return X, self.weigh(y, self.partition_weights(p, len(y)))

    def train_eval_chunks(self, parts, prec, device):
        off = 0
        for X, y in self.inner.train_eval_chunks(parts, prec, device):
            n = len(y)
            yield X, self.weigh(y, None if self._flat is None else self._flat[off:off + n])
            off += n

    def test(self, prec, device):
        X, y = self.inner.test(prec, device)
        return X, self.weigh(y)
