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
Cross-validation runs (--cv K, K fold models) are scored per fold model the same way, and by the held-out loss: the
evaluation cuts every training partition it walks into the folds the kernel used (row i of a partition: fold i mod K),
model k's loss over the rows of fold k is its held-out loss and its loss over the other rows its training loss;
``EvalResult.cv_loss_folds`` [R, K] is the mean held-out loss of every fold, ``cv_loss`` [R] their mean over the folds
and ``cv_std`` [R] their standard deviation (ddof = 1).  The console prints ``>> Fold k: held-out rows = n_k of n``
(the objective's counts) before fold model k's usual lines and closes with ``>> CV: K folds, held-out loss = ... +- ...
(final round)``; fold model k's result names carry the prefix ``cv{k}_`` (before ``sqhinge_``) and one more file, named
like the training-loss file with ``cv_loss`` in its place and no fold prefix, holds ``cv_loss``.
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

import os
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from ..data import io as dio
from ..models.losses import LOGISTIC
from ..ops.eval import auc_columns, loss_sums, predictions, predictions_and_loss, sign_labels
from ..utils import report
from .trainer import TrainResult, Trainer

SOFTMAX_P_ELEMS = 1 << 26  # logits held at once by the class evaluation (rounds are chunked to fit)


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
    # cross-validation runs (the other arrays [R, K], one column per fold model): the mean held-out loss of every
    # fold [R, K], its mean over the folds [R] and its standard deviation over the folds (ddof = 1) [R]
    cv_loss_folds: Optional[np.ndarray] = None
    cv_loss: Optional[np.ndarray] = None
    cv_std: Optional[np.ndarray] = None


def _nnz_line(l1: float, nnz: int, d: int) -> str:
    return ">> L1: l1 = %g, nnz = %d of %d" % (l1, nnz, d)


def _write_nnz(files: Dict[str, str], nnz, key: str = "nnz") -> None:
    """The nnz result file next to the auc file: the same directory and prefixes, ``auc`` -> ``nnz``."""
    auc_key = key[: -len("nnz")] + "auc"
    head, tail = files[auc_key].rsplit("auc", 1)
    files[key] = head + "nnz" + tail
    dio.save_vector(np.asarray(nnz, dtype=np.float64), files[key])


def _write_cv_loss(files: Dict[str, str], prefix: str, cv_loss) -> None:
    """The cv_loss result file next to fold model 0's training-loss file (written under ``prefix``): the same
    directory and prefixes without the fold's own, ``training_loss`` -> ``cv_loss``; a training-loss name that does
    not say ``training_loss`` gets ``cv_loss_`` in front instead."""
    folder, name = os.path.split(files[prefix + "training_loss"])
    name = name[len(prefix):] if name.startswith(prefix) else name
    head, sep, tail = name.rpartition("training_loss")
    files["cv_loss"] = os.path.join(folder, head + "cv_loss" + tail if sep else "cv_loss_" + name)
    dio.save_vector(np.asarray(cv_loss, dtype=np.float64), files["cv_loss"])


def _cv_sums(chunks, B, d_x: int, kind: int, K: int, prec):
    """A cross-validation run's loss sums over whole training partitions: (training sums [R, K], held-out sums
    [R, K], training rows [K], held-out rows [K]).  Every partition is cut into its folds X[k::K] (the rows the
    kernel held out of model k: a row's fold is its index in the partition mod K), each as a contiguous copy for the
    evaluation GEMM; model k's sum over fold k is its held-out sum, the other models' sums add to their training sums."""
    RK = B.shape[0]
    train, held = np.zeros((RK // K, K)), np.zeros((RK // K, K))
    n_held, n = np.zeros(K, dtype=np.int64), 0
    for X, y in chunks:
        n += X.shape[0]
        for k in range(K):
            Xk, yk = X[k::K].contiguous(), y[k::K].contiguous()
            if Xk.shape[0] == 0:
                continue
            s, m = loss_sums([(Xk, yk)], B, d_x, kind, acc=prec)
            s = np.asarray(s).reshape(RK // K, K)
            held[:, k] += s[:, k]
            s[:, k] = 0.0
            train += s
            n_held[k] += m
    return train, held, n - n_held, n_held


def _weights_line(trainer: Trainer) -> str:
    cw = trainer.cfg.class_weight
    spec = "none" if cw is None else cw if isinstance(cw, str) else "%g:%g" % tuple(cw)
    return ">> Weights: class_weight = %s, w+ = %g, w- = %g, sum w / n = %g" % (
        spec, trainer.class_weight[0], trainer.class_weight[1], trainer.weight_sum_over_n)


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


def _class_sums(X, y, B, classes: int, d_x: int, row_loss):
    """(loss sums [R], correct counts [R]) of the rows X, y (class indices) for the models B [R * classes, ld_x]:
    scores from the prediction GEMM (ops/eval.predictions), rounds chunked so the scores held at once stay bounded;
    row_loss(Z [n, r, classes], y [n]) gives a chunk's loss sums [r]."""
    n, R = X.shape[0], B.shape[0] // classes
    tot = torch.zeros(R, dtype=torch.float64)
    hit = torch.zeros(R, dtype=torch.float64)
    step = max(1, SOFTMAX_P_ELEMS // max(1, n * classes))
    yl = y.to(X.device).long()
    for r0 in range(0, R, step):
        r1 = min(R, r0 + step)
        Z = predictions(X, B[r0 * classes: r1 * classes], d_x).double().reshape(n, r1 - r0, classes)
        tot[r0:r1] = row_loss(Z, yl).cpu()
        hit[r0:r1] = (Z.argmax(dim=2) == yl[:, None]).double().sum(0).cpu()
    return tot.numpy(), hit.numpy()


def _softmax_sums(X, y, B, spec):
    """Cross-entropy logsumexp(z) - z_y."""
    def ce(Z, yl):
        zy = Z.gather(2, yl[:, None, None].expand(Z.shape[0], Z.shape[1], 1))[:, :, 0]
        return (torch.logsumexp(Z, dim=2) - zy).sum(0)
    return _class_sums(X, y, B, spec.classes, spec.d_x, ce)


def _ovr_sums(X, y, B, spec):
    """Sum over classes of l(y_k z_k), l the run's logistic or squared-hinge loss."""
    def loss(Z, yl):
        own = yl[:, None, None] == torch.arange(spec.classes, device=Z.device)[None, None, :]
        m = torch.where(own, -Z, Z)  # -y_k z_k
        if spec.loss == LOGISTIC:
            v = torch.clamp(m, min=0) + torch.log1p(torch.exp(-m.abs()))
        else:
            v = torch.clamp(1.0 + m, min=0) ** 2
        return v.sum(dim=(0, 2))
    return _class_sums(X, y, B, spec.classes, spec.d_x, loss)


_CLASS_SUMS = {"softmax": _softmax_sums, "ovr": _ovr_sums}


def _evaluate_classes(trainer: Trainer, res: TrainResult, log, write: bool) -> EvalResult:
    """Softmax and one-vs-rest runs: a [classes][ld_x] model scored by its loss and the test accuracy."""
    cfg, dev, prec, spec = trainer.cfg, trainer.env.device, trainer.prec, trainer.model
    R = res.betaset.shape[0]
    B = torch.from_numpy(spec.rows(res.betaset)).to(dev)
    parts = eval_partitions(trainer)
    sums = _CLASS_SUMS[spec.kind]
    if cfg.verbose:
        log(report.total_time_line(res.total_time))
    tr_sum, n_train = np.zeros(R), 0
    for X, y in _train_chunks(trainer, parts, prec, dev):
        s, _ = sums(X, y, B, spec)
        tr_sum += s
        n_train += X.shape[0]
    Xt, yt = trainer.source.test(prec, dev)
    te_sum, hits = sums(Xt, yt, B, spec)
    n_test = Xt.shape[0]
    training_loss = tr_sum / max(1, n_train)
    testing_loss = te_sum / max(1, n_test)
    acc = hits / max(1, n_test)
    nnz, pen = spec.sparsity(res.betaset)
    if cfg.verbose:
        for i in range(R):
            log(report.softmax_line(i, training_loss[i], testing_loss[i], acc[i], res.timeset[i]))
        if spec.prox and R:
            log(_nnz_line(spec.l1, nnz[-1], spec.classes * spec.d_x))
    files = None
    if write:
        names = spec.result_names(trainer.scheme.output_names(cfg.fix_quirks))
        data_dir = getattr(trainer.source, "data_dir", None) or cfg.input_dir
        files = report.write_results(dio.results_dir(data_dir), names, training_loss, testing_loss, acc,
                                     res.timeset, res.worker_timeset, cfg.full_precision_outputs)
        if spec.prox:
            _write_nnz(files, nnz)
    if cfg.verbose:
        log(">>> Done")
    return EvalResult(training_loss, testing_loss, acc, n_train, n_test, files, nnz=nnz, l1_penalty=pen)


def _evaluate_scalar(trainer: Trainer, res: TrainResult, log, write: bool) -> EvalResult:
    """Runs of a scalar loss, M >= 1 models through one evaluation: betaset as R * M rows of the model matrix.  A
    single model is M = 1 without a model axis, per-model header or prefix."""
    cfg, dev, prec, spec = trainer.cfg, trainer.env.device, trainer.prec, trainer.model
    M, d_x, kind = spec.models, spec.d_x, spec.loss
    R = res.betaset.shape[0]
    B = torch.from_numpy(spec.rows(res.betaset)).to(dev)
    parts = eval_partitions(trainer)
    if cfg.verbose:
        if spec.weighted:
            log(_weights_line(trainer))
        log(report.total_time_line(res.total_time))
        if trainer.scheme.logs_eval_loading and not trainer.source.is_sparse:
            for p in parts:
                log(">> Loaded %d" % (p + 1))
    cv = spec.kind == "cv"
    if cv:  # every fold model's training rows are the partitions' rows outside its fold
        sums, held, rows_k, held_k = _cv_sums(_train_chunks(trainer, parts, prec, dev), B, d_x, kind, M, prec)
        n_train = int(rows_k[0] + held_k[0])
        training_loss = sums / np.maximum(1, rows_k)[None, :]
    else:
        sums, n_train = loss_sums(_train_chunks(trainer, parts, prec, dev), B, d_x, kind, acc=prec)
        training_loss = (np.asarray(sums) / max(1, n_train)).reshape(R, M)
    Xt, yt = trainer.source.test(prec, dev)
    P, tsum = predictions_and_loss(Xt, yt, B, d_x, kind, acc=prec)
    n_test = Xt.shape[0]
    testing_loss = (np.asarray(tsum) / max(1, n_test)).reshape(R, M)
    classify = spec.scoring == "auc"
    # weighted runs: the classes behind the weighted labels (an unweighted AUC, comparable across runs)
    auc = (auc_columns(sign_labels(yt) if spec.weighted else yt, P) if classify else np.zeros(R * M)).reshape(R, M)
    nnz, pen = spec.sparsity(res.betaset)
    nnz_k = nnz.reshape(R, M)
    files = None
    if write and (classify or cfg.save_linear):
        files = {}
        data_dir = getattr(trainer.source, "data_dir", None) or cfg.input_dir
    for k, (header, prefix, l1) in enumerate(spec.scalar_models()):
        if cfg.verbose:
            if header:
                log(header)
            for i in range(R):
                if classify:
                    log(report.logistic_line(i, training_loss[i, k], testing_loss[i, k], auc[i, k], res.timeset[i]))
                else:
                    log(report.linear_line(i, training_loss[i, k], testing_loss[i, k], res.timeset[i]))
            if spec.prox and R:
                log(_nnz_line(l1, nnz_k[-1, k], d_x))
        if files is not None:
            names = spec.result_names(trainer.scheme.output_names(cfg.fix_quirks), prefix)
            out = report.write_results(dio.results_dir(data_dir), names, training_loss[:, k], testing_loss[:, k],
                                       auc[:, k], res.timeset, res.worker_timeset, cfg.full_precision_outputs)
            files.update({prefix + key: v for key, v in out.items()})
            if spec.prox:
                _write_nnz(files, nnz_k[:, k], prefix + "nnz")
    final = testing_loss[-1] if R else np.zeros(M)
    best = spec.best(final)
    cv_folds = cv_loss = cv_std = None
    if cv:
        cv_folds = held / np.maximum(1, held_k)[None, :]
        cv_loss, cv_std = cv_folds.mean(axis=1), cv_folds.std(axis=1, ddof=1)
        if files is not None:
            _write_cv_loss(files, spec.scalar_models()[0][1], cv_loss)
        if cfg.verbose and R:
            log(">> CV: %d folds, held-out loss = %g +- %g (final round)" % (M, cv_loss[-1], cv_std[-1]))
    if cfg.verbose:
        if best is not None:
            log(">> Best model: %d (alpha = %g, lr = %g, final test loss %g)"
                % (best, spec.sweep_alpha[best], spec.sweep_lr[best], final[best]))
        log(">>> Done")
    return EvalResult(spec.per_model(training_loss), spec.per_model(testing_loss), spec.per_model(auc), n_train,
                      n_test, files, best, nnz=nnz, l1_penalty=pen, cv_loss_folds=cv_folds, cv_loss=cv_loss,
                      cv_std=cv_std)


def evaluate(trainer: Trainer, res: TrainResult, log=None, write: bool = True) -> EvalResult:
    log = log or report.log
    if trainer.model.scoring == "accuracy":
        return _evaluate_classes(trainer, res, log, write)
    return _evaluate_scalar(trainer, res, log, write)
