"""Master epilogue: evaluate every stored beta, print, save (ref src/naive.py:153-209).

Reference quirks reproduced unless ``fix_quirks``:
  * the training set is partitions 1..W-1 — partition W is skipped (ref src/naive.py:161,167
    ``range(2, n_procs-1)``), labels are the matching prefix of label.dat (ref :172);
  * linear-regression runs print but do not write result files (ref src/naive.py:413-417);
  * result names follow each scheme's (colliding) prefixes (codes/schemes.py).
Squared-hinge runs (not in the reference) are scored and printed like logistic ones, and every result
name carries the prefix ``sqhinge_`` so a run in the same data directory keeps the logistic files.
Sweep runs (--alphas / --lrs, M models) are scored per model: the arrays get a trailing model axis [R, M], the
console prints ``>> Model k: alpha = ..., lr = ...`` before model k's usual iteration lines, and model k's
result names carry the prefix ``sweep{k}_`` (before ``sqhinge_`` where that applies).
Softmax runs are scored by cross-entropy and accuracy: the console line carries the accuracy where the
logistic line has the AUC, ``EvalResult.auc`` (and the ``auc`` result file) hold the accuracy, and the
result names carry the prefix ``softmax_``.
One-vs-rest runs (--ovr C) are scored like softmax runs with their own loss: training and test loss are the mean over
rows of sum_k l(y_k z_k) (l the run's binary loss, y_k = +1 for the row's class and -1 for the others), the accuracy
(argmax_k z_k, first on ties) stands where softmax puts it, and the result names carry the prefix ``ovr_`` (before
``sqhinge_`` where that applies).
Runs with an L1 penalty (--l1 / --l1s, some lambda > 0) also report sparsity: ``EvalResult.nnz`` (the non-zero
data columns of every iterate) and ``l1_penalty`` are filled for every run; with some lambda > 0 the console gets
one line ``>> L1: l1 = ..., nnz = k of d`` per model, the ``>> Model k:`` line of a sweep names ``l1``, and an
``nnz`` result file is written next to the ``auc`` file, under the same prefixes.
Weighted runs (--class-weight / --sample-weights): training and test loss are the weighted means (1/n) sum w_i l_i
with n the row count (test rows take the class weights), the AUC is the ordinary unweighted ROC AUC on the classes,
the console gets one line ``>> Weights: class_weight = ..., w+ = ..., w- = ..., sum w / n = ...`` before the usual
ones, and the result names carry the prefix ``weighted_`` (after ``sweep{k}_``, before ``sqhinge_``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from ..data import io as dio
from ..models.losses import LOGISTIC, SQUARED_HINGE, base_kind, is_classification, is_multiclass
from ..ops.eval import auc_columns, loss_sums, predictions, predictions_and_loss, sign_labels
from ..utils import report
from .trainer import TrainResult, Trainer


SQHINGE_PREFIX = "sqhinge_"  # result files of squared-hinge runs (next to the logistic names)
SOFTMAX_PREFIX = "softmax_"
OVR_PREFIX = "ovr_"  # result files of one-vs-rest runs (before sqhinge_)
WEIGHTED_PREFIX = "weighted_"  # result files of runs with class / sample weights
SOFTMAX_P_ELEMS = 1 << 26  # logits held at once by the softmax evaluation (rounds are chunked to fit)


@dataclass
class EvalResult:
    training_loss: np.ndarray
    testing_loss: np.ndarray
    auc: np.ndarray  # softmax runs: the test accuracy of every round
    n_train: int
    n_test: int
    files: Optional[Dict[str, str]] = None  # sweep runs: {"sweep{k}_" + key: path} of every model
    best: Optional[int] = None  # sweep runs (arrays [R, M]): the model with the lowest final test loss
    # non-zero data columns of every iterate: [R], sweep [R, M]; softmax and one-vs-rest: all C blocks
    nnz: Optional[np.ndarray] = None
    l1_penalty: Optional[np.ndarray] = None  # l1 * ||beta||_1 of every iterate, shaped like nnz


def sparsity(trainer: Trainer, betaset: np.ndarray):
    """(nnz, l1_penalty) of every iterate over the data columns: [R], or [R, M] for a sweep run (softmax counts
    and one-vs-rest count over their C class blocks: they are one model with one lambda)."""
    B = np.asarray(betaset, dtype=np.float64)
    R, M = B.shape[0], getattr(trainer, "models", 1)
    if M > 1:
        blocks = B.reshape(R, M, trainer.ld_x)[:, :, : trainer.d_x]
        l1 = np.asarray(trainer.sweep_l1, dtype=np.float64)
        return np.count_nonzero(blocks, axis=2), np.abs(blocks).sum(axis=2) * l1
    if is_multiclass(trainer.loss) or getattr(trainer, "ovr", False):
        B = B.reshape(R, trainer.classes, trainer.ld_x)[:, :, : trainer.d_x].reshape(R, -1)
    else:
        B = B[:, : trainer.d]
    return np.count_nonzero(B, axis=1), np.abs(B).sum(axis=1) * float(trainer.cfg.l1)


def _nnz_line(l1: float, nnz: int, d: int) -> str:
    return ">> L1: l1 = %g, nnz = %d of %d" % (l1, nnz, d)


def _write_nnz(files: Dict[str, str], nnz, key: str = "nnz") -> None:
    """The nnz result file next to the auc file: the same directory and prefixes, ``auc`` -> ``nnz``."""
    auc_key = key[: -len("nnz")] + "auc"
    head, tail = files[auc_key].rsplit("auc", 1)
    files[key] = head + "nnz" + tail
    dio.save_vector(np.asarray(nnz, dtype=np.float64), files[key])


def _weights_line(trainer: Trainer) -> str:
    cw = trainer.cfg.class_weight
    spec = "none" if cw is None else cw if isinstance(cw, str) else "%g:%g" % tuple(cw)
    return ">> Weights: class_weight = %s, w+ = %g, w- = %g, sum w / n = %g" % (
        spec, trainer.class_weight[0], trainer.class_weight[1], trainer.weight_sum_over_n)


def _result_names(trainer: Trainer) -> Dict[str, str]:
    """The scheme's result names under the loss's prefixes: ``weighted_`` first, then ``sqhinge_``."""
    names = trainer.scheme.output_names(trainer.cfg.fix_quirks)
    if base_kind(trainer.loss) == SQUARED_HINGE:
        names = {k: SQHINGE_PREFIX + v for k, v in names.items()}
    if getattr(trainer, "weighted", False):
        names = {k: WEIGHTED_PREFIX + v for k, v in names.items()}
    return names


def eval_partitions(trainer: Trainer):
    W = trainer.cfg.n_workers
    if trainer.cfg.fix_quirks:
        return list(range(trainer.scheme.n_partition_files))
    return list(range(max(1, W - 1)))


def _train_chunks(trainer: Trainer, parts, prec, dev):
    """Training partitions for the evaluation, in order.

    Dense partitions this rank already holds in HBM (all of them on one GPU) are evaluated in
    place instead of being re-read from disk or regenerated.  The reference reloads every file
    (ref src/naive.py:161-172).  Its labels are the prefix of label.dat, which for partitions
    taken in order 0..k is exactly each partition's own labels.
    """
    resident = getattr(trainer, "_parts", None) or {}
    if trainer.source.is_sparse or not all(p in resident for p in parts) or list(parts) != sorted(parts):
        yield from trainer.source.train_eval_chunks(parts, prec, dev)
        return
    for p in parts:
        yield resident[p]


def _softmax_sums(X, y, B, classes: int, d_x: int):
    """(CE sums [R], correct counts [R]) of the rows X, y for the models B [R * classes, ld_x]: logits from
    the prediction GEMM (ops/eval.predictions), rounds chunked so the logits stay bounded."""
    n, R = X.shape[0], B.shape[0] // classes
    ce = torch.zeros(R, dtype=torch.float64)
    hit = torch.zeros(R, dtype=torch.float64)
    step = max(1, SOFTMAX_P_ELEMS // max(1, n * classes))
    yl = y.to(X.device).long()
    for r0 in range(0, R, step):
        r1 = min(R, r0 + step)
        Z = predictions(X, B[r0 * classes: r1 * classes], d_x).double().reshape(n, r1 - r0, classes)
        zy = Z.gather(2, yl[:, None, None].expand(n, r1 - r0, 1))[:, :, 0]
        ce[r0:r1] = (torch.logsumexp(Z, dim=2) - zy).sum(0).cpu()
        hit[r0:r1] = (Z.argmax(dim=2) == yl[:, None]).double().sum(0).cpu()
    return ce.numpy(), hit.numpy()


def _ovr_sums(X, y, B, classes: int, d_x: int, kind: int):
    """(loss sums [R], correct counts [R]) of the rows X, y (class indices) for the one-vs-rest models
    B [R * classes, ld_x]: sum over rows and classes of l(y_k z_k) with l the logistic or the squared-hinge loss;
    scores from the prediction GEMM, rounds chunked like _softmax_sums."""
    n, R = X.shape[0], B.shape[0] // classes
    tot = torch.zeros(R, dtype=torch.float64)
    hit = torch.zeros(R, dtype=torch.float64)
    step = max(1, SOFTMAX_P_ELEMS // max(1, n * classes))
    yl = y.to(X.device).long()
    own = yl[:, None, None] == torch.arange(classes, device=X.device)[None, None, :]
    for r0 in range(0, R, step):
        r1 = min(R, r0 + step)
        Z = predictions(X, B[r0 * classes: r1 * classes], d_x).double().reshape(n, r1 - r0, classes)
        m = torch.where(own, -Z, Z)  # -y_k z_k
        if kind == LOGISTIC:
            v = torch.clamp(m, min=0) + torch.log1p(torch.exp(-m.abs()))
        else:
            v = torch.clamp(1.0 + m, min=0) ** 2
        tot[r0:r1] = v.sum(dim=(0, 2)).cpu()
        hit[r0:r1] = (Z.argmax(dim=2) == yl[:, None]).double().sum(0).cpu()
    return tot.numpy(), hit.numpy()


def _evaluate_softmax(trainer: Trainer, res: TrainResult, log, write: bool) -> EvalResult:
    """Softmax and one-vs-rest runs: a [classes][ld_x] model scored by its loss and the test accuracy."""
    cfg, dev, prec = trainer.cfg, trainer.env.device, trainer.prec
    C, d_x, ld_x = trainer.classes, trainer.d_x, trainer.ld_x
    R = res.betaset.shape[0]
    B = torch.from_numpy(np.ascontiguousarray(res.betaset)).to(dev).reshape(R * C, ld_x)
    parts = eval_partitions(trainer)
    if getattr(trainer, "ovr", False):
        kind = trainer.loss

        def sums(X, y):
            return _ovr_sums(X, y, B, C, d_x, kind)
        prefix = OVR_PREFIX + (SQHINGE_PREFIX if kind == SQUARED_HINGE else "")
    else:
        def sums(X, y):
            return _softmax_sums(X, y, B, C, d_x)
        prefix = SOFTMAX_PREFIX
    if cfg.verbose:
        log(report.total_time_line(res.total_time))
    tr_sum, n_train = np.zeros(R), 0
    for X, y in _train_chunks(trainer, parts, prec, dev):
        s, _ = sums(X, y)
        tr_sum += s
        n_train += X.shape[0]
    Xt, yt = trainer.source.test(prec, dev)
    te_sum, hits = sums(Xt, yt)
    n_test = Xt.shape[0]
    training_loss = tr_sum / max(1, n_train)
    testing_loss = te_sum / max(1, n_test)
    acc = hits / max(1, n_test)
    nnz, pen = sparsity(trainer, res.betaset)
    if cfg.verbose:
        for i in range(R):
            log(report.softmax_line(i, training_loss[i], testing_loss[i], acc[i], res.timeset[i]))
        if trainer.prox and R:
            log(_nnz_line(cfg.l1, nnz[-1], C * d_x))
    files = None
    if write:
        names = {k: prefix + v for k, v in trainer.scheme.output_names(cfg.fix_quirks).items()}
        data_dir = getattr(trainer.source, "data_dir", None) or cfg.input_dir
        files = report.write_results(dio.results_dir(data_dir), names, training_loss, testing_loss, acc,
                                     res.timeset, res.worker_timeset, cfg.full_precision_outputs)
        if trainer.prox:
            _write_nnz(files, nnz)
    if cfg.verbose:
        log(">>> Done")
    return EvalResult(training_loss, testing_loss, acc, n_train, n_test, files, nnz=nnz, l1_penalty=pen)


def sweep_prefix(k: int) -> str:
    return f"sweep{k}_"


def _evaluate_sweep(trainer: Trainer, res: TrainResult, log, write: bool) -> EvalResult:
    """Every model of a sweep run through the single-model evaluation: betaset [R, M * ld_x] as R * M models."""
    cfg, dev, prec = trainer.cfg, trainer.env.device, trainer.prec
    M, d_x, ld_x, kind = trainer.models, trainer.d_x, trainer.ld_x, trainer.loss
    R = res.betaset.shape[0]
    B = torch.from_numpy(np.ascontiguousarray(res.betaset)).to(dev).reshape(R * M, ld_x)
    parts = eval_partitions(trainer)
    weighted = getattr(trainer, "weighted", False)
    if cfg.verbose:
        if weighted:
            log(_weights_line(trainer))
        log(report.total_time_line(res.total_time))
        if trainer.scheme.logs_eval_loading and not trainer.source.is_sparse:
            for p in parts:
                log(">> Loaded %d" % (p + 1))
    sums, n_train = loss_sums(_train_chunks(trainer, parts, prec, dev), B, d_x, kind, acc=prec)
    Xt, yt = trainer.source.test(prec, dev)
    P, tsum = predictions_and_loss(Xt, yt, B, d_x, kind, acc=prec)
    n_test = Xt.shape[0]
    training_loss = (np.asarray(sums) / max(1, n_train)).reshape(R, M)
    testing_loss = (np.asarray(tsum) / max(1, n_test)).reshape(R, M)
    classify = is_classification(kind)
    # weighted runs: the classes behind the weighted labels (an unweighted AUC, comparable across runs)
    auc = (auc_columns(sign_labels(yt) if weighted else yt, P) if classify else np.zeros(R * M)).reshape(R, M)
    nnz, pen = sparsity(trainer, res.betaset)
    files = None
    do_write = write and (classify or cfg.save_linear)
    if do_write:
        files = {}
        data_dir = getattr(trainer.source, "data_dir", None) or cfg.input_dir
    for k in range(M):
        if cfg.verbose:
            log(">> Model %d: alpha = %g, lr = %g" % (k, trainer.sweep_alpha[k], trainer.sweep_lr[k])
                + (", l1 = %g" % trainer.sweep_l1[k] if trainer.prox else ""))
            for i in range(R):
                if classify:
                    log(report.logistic_line(i, training_loss[i, k], testing_loss[i, k], auc[i, k], res.timeset[i]))
                else:
                    log(report.linear_line(i, training_loss[i, k], testing_loss[i, k], res.timeset[i]))
            if trainer.prox and R:
                log(_nnz_line(trainer.sweep_l1[k], nnz[-1, k], d_x))
        if do_write:
            names = {key: sweep_prefix(k) + v for key, v in _result_names(trainer).items()}
            out = report.write_results(dio.results_dir(data_dir), names, training_loss[:, k], testing_loss[:, k],
                                       auc[:, k], res.timeset, res.worker_timeset, cfg.full_precision_outputs)
            files.update({sweep_prefix(k) + key: v for key, v in out.items()})
            if trainer.prox:
                _write_nnz(files, nnz[:, k], sweep_prefix(k) + "nnz")
    final = testing_loss[-1] if R else np.zeros(M)
    best = int(np.argmin(np.where(np.isfinite(final), final, np.inf)))
    if cfg.verbose:
        log(">> Best model: %d (alpha = %g, lr = %g, final test loss %g)"
            % (best, trainer.sweep_alpha[best], trainer.sweep_lr[best], final[best]))
        log(">>> Done")
    return EvalResult(training_loss, testing_loss, auc, n_train, n_test, files, best, nnz=nnz, l1_penalty=pen)


def evaluate(trainer: Trainer, res: TrainResult, log=None, write: bool = True) -> EvalResult:
    log = log or report.log
    if is_multiclass(trainer.loss) or getattr(trainer, "ovr", False):
        return _evaluate_softmax(trainer, res, log, write)
    if getattr(trainer, "models", 1) > 1:
        return _evaluate_sweep(trainer, res, log, write)
    cfg = trainer.cfg
    dev = trainer.env.device
    prec = trainer.prec
    d, ld = trainer.d, trainer.ld
    R = res.betaset.shape[0]
    B = torch.zeros((R, ld), dtype=torch.float64, device=dev)
    B[:, :d] = torch.from_numpy(res.betaset).to(dev)
    kind = trainer.loss
    parts = eval_partitions(trainer)
    weighted = getattr(trainer, "weighted", False)
    if cfg.verbose:
        if weighted:
            log(_weights_line(trainer))
        log(report.total_time_line(res.total_time))
        if trainer.scheme.logs_eval_loading and not trainer.source.is_sparse:
            for p in parts:
                log(">> Loaded %d" % (p + 1))
    sums, n_train = loss_sums(_train_chunks(trainer, parts, prec, dev), B, d, kind, acc=prec)
    Xt, yt = trainer.source.test(prec, dev)
    P, tsum = predictions_and_loss(Xt, yt, B, d, kind, acc=prec)
    n_test = Xt.shape[0]
    training_loss = sums / max(1, n_train)
    testing_loss = tsum / max(1, n_test)
    classify = is_classification(kind)
    # weighted runs: the classes behind the weighted labels (an unweighted AUC, comparable across runs)
    auc = auc_columns(sign_labels(yt) if weighted else yt, P) if classify else np.zeros(R)
    nnz, pen = sparsity(trainer, res.betaset)
    if cfg.verbose:
        for i in range(R):
            if classify:
                log(report.logistic_line(i, training_loss[i], testing_loss[i], auc[i], res.timeset[i]))
            else:
                log(report.linear_line(i, training_loss[i], testing_loss[i], res.timeset[i]))
        if trainer.prox and R:
            log(_nnz_line(cfg.l1, nnz[-1], d))
    files = None
    if write and (classify or cfg.save_linear):
        names = _result_names(trainer)
        data_dir = getattr(trainer.source, "data_dir", None) or cfg.input_dir
        files = report.write_results(dio.results_dir(data_dir), names, training_loss, testing_loss, auc,
                                     res.timeset, res.worker_timeset, cfg.full_precision_outputs)
        if trainer.prox:
            _write_nnz(files, nnz)
    if cfg.verbose:
        log(">>> Done")
    return EvalResult(training_loss, testing_loss, auc, n_train, n_test, files, nnz=nnz, l1_penalty=pen)
