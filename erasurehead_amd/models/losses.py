"""Model math: logistic regression (L2), least squares and the squared-hinge L2-SVM — fp64 NumPy oracles.

These are the reference formulas verbatim (SURVEY §2.2 "Math spec"), kept independent
of the device path so the HIP kernels can be checked against them:

  logistic worker gradient   g = -X^T( y_mod / (exp(y * (X beta)) + 1) )   ref src/naive.py:137-139
  least-squares gradient     g = -2 X^T (y - X beta)                        ref src/naive.py:345-346
  squared-hinge gradient     g = -2 X^T( y_mod * max(0, 1 - y * (X beta)) )  (L2-SVM; not in the reference)
  GD                         beta <- (1 - 2 alpha eta) beta - (eta/n) g      ref src/naive.py:112-115
  AGD (theta = 2/(i+2))      y = (1-theta) beta + theta u
                             beta' = y - (eta/n) g - 2 alpha eta beta
                             u = beta + (beta' - beta)/theta                 ref src/naive.py:116-122
  training loss              (1/n) sum log(1 + exp(-y * p))                 ref src/util.py:136-137
  MSE                        mean (y - p)^2                                  ref src/util.py:139-141
  squared-hinge loss         mean max(0, 1 - y * p)^2
  AUC                        area under ROC of scores p vs labels in {-1,1}  ref src/naive.py:196-197

Multi-class softmax regression (not in the reference): labels are class indices 0..C-1, the model is
B [C, d] and travels flattened class-major (on the device [C][ld_x], padding columns zero):
  logits / probabilities     z_c = x . B_c,  p = softmax(z)  (max_c z_c subtracted before exp)
  worker gradient            G_c = sum_rows coef (p_c - [y = c]) x    (the scale of logistic_grad: C = 2 with
                             B_0 = 0, B_1 = beta gives G_1 = logistic_grad(X, 2y - 1, beta), G_0 = -G_1)
  cross-entropy              CE = logsumexp(z) - z_y  (never -log p_y)
  step size                  the CE Hessian is bounded by XtX / 2 (logistic: XtX / 4): lr 5 where logistic uses 10

One-vs-rest (not in the reference): the same labels and [C, d] layout, C binary models of the logistic or the
squared-hinge loss, model k with the labels y_k = +1 where y = k and -1 elsewhere:
  objective                  (1/n) sum_rows sum_k l(y_k * x . B_k)
  worker gradient            G_k = the scalar-loss gradient at (B_k, y_k)
  prediction                 argmax_k x . B_k (first on ties)
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

LOGISTIC = 0
LEAST_SQUARES = 1
SQUARED_HINGE = 2
SOFTMAX = 3
# weighted logistic / squared hinge (csrc/kernels/common.h kLogisticW / kSquaredHingeW): the label carries the row's
# weight, y~ = s * w with the class s the sign BIT of y~ and w = |y~| >= 0.  The engine selects them when a run has
# class or sample weights (engine/model.py); no --loss name maps to them.
LOGISTIC_W = 4
SQUARED_HINGE_W = 5
_WEIGHTED = {LOGISTIC: LOGISTIC_W, SQUARED_HINGE: SQUARED_HINGE_W}
LOSS_NAMES = {"logistic": LOGISTIC, "least_squares": LEAST_SQUARES, "squared_hinge": SQUARED_HINGE}
# every loss a run can name (--loss): the per-row scalar losses above plus the multi-class model
LOSS_CHOICES = {**LOSS_NAMES, "softmax": SOFTMAX}
MIN_CLASSES, MAX_CLASSES = 2, 8  # csrc/kernels/launchers.h kMinBlocks / kMaxBlocks


def is_multiclass(kind: int) -> bool:
    """Losses over class-index labels with a [C, d] model: scored by accuracy."""
    return kind == SOFTMAX


def check_classes(classes: int) -> int:
    if not MIN_CLASSES <= int(classes) <= MAX_CLASSES:
        raise ValueError(f"classes must be in {MIN_CLASSES}..{MAX_CLASSES}, got {classes}")
    return int(classes)


def is_classification(kind: int) -> bool:
    """Losses over labels in {-1, +1}: their runs are scored by ROC AUC and write result files."""
    return kind in (LOGISTIC, SQUARED_HINGE, LOGISTIC_W, SQUARED_HINGE_W)


def weighted_kind(kind: int) -> int:
    """The weighted code of a +-1-label loss: logistic -> LOGISTIC_W, squared hinge -> SQUARED_HINGE_W."""
    if kind not in _WEIGHTED:
        raise ValueError(f"loss kind {kind} has no weighted form (logistic and squared hinge only)")
    return _WEIGHTED[kind]


def base_kind(kind: int) -> int:
    """The unweighted loss of a weighted code; every other code is its own base."""
    return {w: k for k, w in _WEIGHTED.items()}.get(kind, kind)


def is_weighted(kind: int) -> bool:
    return kind in (LOGISTIC_W, SQUARED_HINGE_W)


def split_weighted(y) -> Tuple[np.ndarray, np.ndarray]:
    """(s, w) of weighted labels y~ = s * w: s = -1 where the sign bit is set (so at -0.0 too), else +1; w = |y~|."""
    y = np.asarray(y, dtype=np.float64)
    return np.where(np.signbit(y), -1.0, 1.0), np.abs(y)


def _sigmoid_neg(t: np.ndarray) -> np.ndarray:
    """1 / (exp(t) + 1) without overflow warnings."""
    out = np.empty_like(t, dtype=np.float64)
    pos = t > 0
    e = np.exp(-t[pos])
    out[pos] = e / (1.0 + e)
    out[~pos] = 1.0 / (1.0 + np.exp(t[~pos]))
    return out


def logistic_grad(X, y: np.ndarray, beta: np.ndarray, coef=None) -> np.ndarray:
    """-X^T (coef*y / (exp(y * X beta) + 1)); X dense ndarray or scipy sparse."""
    z = X.dot(beta)
    ymod = y if coef is None else coef * y
    r = -ymod * _sigmoid_neg(y * z)
    return np.asarray(X.T.dot(r)).ravel()


def least_squares_grad(X, y: np.ndarray, beta: np.ndarray, coef=None) -> np.ndarray:
    z = X.dot(beta)
    c = 1.0 if coef is None else coef
    r = -2.0 * c * (y - z)
    return np.asarray(X.T.dot(r)).ravel()


def squared_hinge_grad(X, y: np.ndarray, beta: np.ndarray, coef=None) -> np.ndarray:
    """-2 X^T (coef*y * max(0, 1 - y * X beta)); X dense ndarray or scipy sparse."""
    z = X.dot(beta)
    ymod = y if coef is None else coef * y
    r = -2.0 * ymod * np.maximum(0.0, 1.0 - y * z)
    return np.asarray(X.T.dot(r)).ravel()


def logistic_w_grad(X, y: np.ndarray, beta: np.ndarray, coef=None) -> np.ndarray:
    """-X^T (coef*y~ / (exp(s * X beta) + 1)) with y~ = s * w."""
    s, _ = split_weighted(y)
    z = X.dot(beta)
    ymod = y if coef is None else coef * y
    r = -ymod * _sigmoid_neg(s * z)
    return np.asarray(X.T.dot(r)).ravel()


def squared_hinge_w_grad(X, y: np.ndarray, beta: np.ndarray, coef=None) -> np.ndarray:
    """-2 X^T (coef*y~ * max(0, 1 - s * X beta)) with y~ = s * w."""
    s, _ = split_weighted(y)
    z = X.dot(beta)
    ymod = y if coef is None else coef * y
    r = -2.0 * ymod * np.maximum(0.0, 1.0 - s * z)
    return np.asarray(X.T.dot(r)).ravel()


def _logits(X, B: np.ndarray) -> np.ndarray:
    return np.asarray(X.dot(np.asarray(B, dtype=np.float64).T))


def softmax_grad(X, y: np.ndarray, B: np.ndarray, coef=None) -> np.ndarray:
    """[C, d]: G_c = X^T (coef * (softmax(X B^T)_c - [y = c])); y holds class indices."""
    Z = _logits(X, B)
    E = np.exp(Z - Z.max(axis=1, keepdims=True))
    R = E / E.sum(axis=1, keepdims=True)
    R[np.arange(len(y)), np.asarray(y).astype(np.int64)] -= 1.0
    if coef is not None:
        R = R * coef
    return np.asarray(X.T.dot(R)).T


def softmax_ce(y: np.ndarray, Z: np.ndarray) -> np.ndarray:
    """Per-row cross-entropy logsumexp(z) - z_y from logits Z [n, C]."""
    Z = np.asarray(Z, dtype=np.float64)
    m = Z.max(axis=1)
    lse = m + np.log(np.exp(Z - m[:, None]).sum(axis=1))
    return lse - Z[np.arange(len(y)), np.asarray(y).astype(np.int64)]


def softmax_loss(y: np.ndarray, Z: np.ndarray, n: Optional[int] = None) -> float:
    """(1/n) sum CE over logits Z [n, C]."""
    return float(softmax_ce(y, Z).sum() / (len(y) if n is None else n))


def accuracy(y: np.ndarray, Z: np.ndarray) -> float:
    """Share of rows whose largest logit (first on ties) is their label."""
    return float(np.mean(np.argmax(np.asarray(Z), axis=1) == np.asarray(y).astype(np.int64)))


def softmax_unpack(betaset: np.ndarray, classes: int, d_x: int) -> np.ndarray:
    """[R, C * ld_x] flattened class-major models (as the engine stores them) -> [R, C, d_x]."""
    b = np.asarray(betaset)
    b = b.reshape(1, -1) if b.ndim == 1 else b
    if b.shape[1] % classes or b.shape[1] // classes < d_x:
        raise ValueError(f"model length {b.shape[1]} is not {classes} class blocks of >= {d_x} columns")
    return b.reshape(b.shape[0], classes, b.shape[1] // classes)[:, :, :d_x]


def softmax_pack(B: np.ndarray, ld_x: int) -> np.ndarray:
    """[C, d_x] -> flattened class-major [C * ld_x] with zero padding columns."""
    B = np.asarray(B, dtype=np.float64)
    out = np.zeros((B.shape[0], ld_x))
    out[:, : B.shape[1]] = B
    return out.ravel()


def ovr_labels(y: np.ndarray, classes: int) -> np.ndarray:
    """[n, C] of +-1: column k is +1 where the class index y is k, -1 elsewhere (the labels model k of a
    one-vs-rest run sees)."""
    y = np.asarray(y)
    return np.where(y[:, None] == np.arange(int(classes))[None, :], 1.0, -1.0)


def ovr_grad(kind: int, X, y: np.ndarray, B: np.ndarray, coef=None) -> np.ndarray:
    """[C, d]: block k is the scalar-loss gradient (logistic or squared hinge) at (B_k, ovr_labels(y)[:, k])."""
    if kind not in (LOGISTIC, SQUARED_HINGE):
        raise ValueError(f"one-vs-rest: loss kind {kind} is not logistic or squared hinge")
    B = np.asarray(B, dtype=np.float64)
    Y = ovr_labels(y, B.shape[0])
    return np.stack([_GRADS[kind](X, Y[:, k], B[k], coef) for k in range(B.shape[0])])


def ovr_row_loss(kind: int, y: np.ndarray, Z: np.ndarray) -> np.ndarray:
    """Per-row one-vs-rest loss sum_k l(y_k z_k) from scores Z [n, C]."""
    if kind not in (LOGISTIC, SQUARED_HINGE):
        raise ValueError(f"one-vs-rest: loss kind {kind} is not logistic or squared hinge")
    Z = np.asarray(Z, dtype=np.float64)
    m = -ovr_labels(y, Z.shape[1]) * Z
    if kind == LOGISTIC:
        v = np.maximum(m, 0.0) + np.log1p(np.exp(-np.abs(m)))
    else:
        v = np.maximum(0.0, 1.0 + m) ** 2
    return v.sum(axis=1)


def ovr_loss(kind: int, y: np.ndarray, Z: np.ndarray, n: Optional[int] = None) -> float:
    """(1/n) sum_rows sum_k l(y_k z_k) over scores Z [n, C]."""
    return float(ovr_row_loss(kind, y, Z).sum() / (len(y) if n is None else n))


def sweep_unpack(betaset: np.ndarray, models: int, d_x: int) -> np.ndarray:
    """[R, M * ld_x] flattened model-major models of a sweep run (as the engine stores them) -> [R, M, d_x]."""
    b = np.asarray(betaset)
    b = b.reshape(1, -1) if b.ndim == 1 else b
    if b.shape[1] % models or b.shape[1] // models < d_x:
        raise ValueError(f"model length {b.shape[1]} is not {models} model blocks of >= {d_x} columns")
    return b.reshape(b.shape[0], models, b.shape[1] // models)[:, :, :d_x]


def sweep_pack(B: np.ndarray, ld_x: int) -> np.ndarray:
    """[R, M, d_x] (or [M, d_x]) -> flattened model-major [R, M * ld_x] ([M * ld_x]) with zero padding columns."""
    B = np.asarray(B, dtype=np.float64)
    if B.shape[-1] > ld_x:
        raise ValueError(f"{B.shape[-1]} columns do not fit blocks of {ld_x}")
    out = np.zeros(B.shape[:-1] + (ld_x,))
    out[..., : B.shape[-1]] = B
    return out.reshape(B.shape[:-2] + (B.shape[-2] * ld_x,))


_GRADS = {LOGISTIC: logistic_grad, LEAST_SQUARES: least_squares_grad, SQUARED_HINGE: squared_hinge_grad,
          LOGISTIC_W: logistic_w_grad, SQUARED_HINGE_W: squared_hinge_w_grad}


def cv_fold_mask(n: int, folds: int) -> np.ndarray:
    """[n, K] bool: entry (i, k) is True where row i of a partition trains fold model k, that is where its fold
    i mod K is not k (the rows model k of a cross-validation run sees)."""
    return (np.arange(int(n)) % int(folds))[:, None] != np.arange(int(folds))[None, :]


def cv_grad(kind: int, X, y: np.ndarray, B: np.ndarray, coef=None) -> np.ndarray:
    """[K, d]: block k is the scalar-loss gradient at B_k over the rows of the partition (X, y) whose fold is not k."""
    if kind not in (LOGISTIC, LEAST_SQUARES, SQUARED_HINGE):
        raise ValueError(f"cross-validation: loss kind {kind} is not logistic, least squares or squared hinge")
    B = np.asarray(B, dtype=np.float64)
    keep = cv_fold_mask(X.shape[0], B.shape[0])
    y = np.asarray(y)
    return np.stack([_GRADS[kind](X[keep[:, k]], y[keep[:, k]], B[k], coef) for k in range(B.shape[0])])


def worker_grad(kind: int, X, y, beta, coef=None) -> np.ndarray:
    if kind == SOFTMAX:  # beta: the flattened [C, X.shape[1]] model; returns the gradient flattened alike
        d = X.shape[1]
        return softmax_grad(X, y, np.asarray(beta).reshape(np.size(beta) // d, d), coef).ravel()
    if kind not in _GRADS:
        raise ValueError(f"unknown loss kind {kind}")
    return _GRADS[kind](X, y, beta, coef)


def logistic_loss(y: np.ndarray, p: np.ndarray, n: Optional[int] = None) -> float:
    """(1/n) sum log(1 + exp(-y p)) in a stable form (identical where the reference is finite)."""
    m = -np.asarray(y) * np.asarray(p)
    v = np.maximum(m, 0.0) + np.log1p(np.exp(-np.abs(m)))
    return float(v.sum() / (len(y) if n is None else n))


def squared_hinge_loss(y: np.ndarray, p: np.ndarray, n: Optional[int] = None) -> float:
    """(1/n) sum max(0, 1 - y p)^2."""
    m = np.maximum(0.0, 1.0 - np.asarray(y, dtype=np.float64) * np.asarray(p, dtype=np.float64))
    return float((m * m).sum() / (len(m) if n is None else n))


def logistic_w_loss(y: np.ndarray, p: np.ndarray, n: Optional[int] = None) -> float:
    """(1/n) sum w log(1 + exp(-s p)) over weighted labels y~ = s * w; n is the row count, not sum w."""
    s, w = split_weighted(y)
    m = -s * np.asarray(p, dtype=np.float64)
    v = w * (np.maximum(m, 0.0) + np.log1p(np.exp(-np.abs(m))))
    return float(v.sum() / (len(s) if n is None else n))


def squared_hinge_w_loss(y: np.ndarray, p: np.ndarray, n: Optional[int] = None) -> float:
    """(1/n) sum w max(0, 1 - s p)^2 over weighted labels y~ = s * w."""
    s, w = split_weighted(y)
    m = np.maximum(0.0, 1.0 - s * np.asarray(p, dtype=np.float64))
    return float((w * m * m).sum() / (len(s) if n is None else n))


def mse(y: np.ndarray, p: np.ndarray) -> float:
    d = np.asarray(y, dtype=np.float64) - np.asarray(p, dtype=np.float64)
    return float(np.mean(d * d))


def roc_auc(y: np.ndarray, scores: np.ndarray, pos_label: float = 1) -> float:
    """ROC AUC with ties counted 1/2 — equal to sklearn roc_curve + auc (trapezoid)."""
    y = np.asarray(y)
    s = np.asarray(scores, dtype=np.float64)
    pos = y == pos_label
    n_pos = int(pos.sum())
    n_neg = len(y) - n_pos
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    order = np.argsort(s, kind="mergesort")
    ss = s[order]
    ranks = np.empty(len(s))
    # average ranks over ties
    i = 0
    n = len(s)
    idx = np.flatnonzero(np.diff(ss)) + 1
    starts = np.concatenate([[0], idx])
    ends = np.concatenate([idx, [n]])
    avg = (starts + ends - 1) / 2.0 + 1.0
    ranks_sorted = np.repeat(avg, ends - starts)
    ranks[order] = ranks_sorted
    u = ranks[pos].sum() - n_pos * (n_pos + 1) / 2.0
    return float(u / (n_pos * n_neg))


def soft_threshold(x, t):
    """S_t(x) = (|x| <= t) ? +0.0 : x - copysign(t, x), the proximal operator of t * |x| (t >= 0, scalar or
    broadcastable).  NaN stays NaN, +-inf stays +-inf, and every |x| <= t (-0.0 at t = 0 included) becomes +0.0:
    the oracle of the soft threshold in combine_update_prox (csrc/kernels/update.hip)."""
    x = np.asarray(x, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    if np.any(~(t >= 0)):
        raise ValueError("soft_threshold: the threshold must be >= 0")
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) <= t, 0.0, x - np.copysign(t, x))


@dataclass
class UpdateRule:
    """GD / AGD with the reference's constants (alpha = 1/n_rows, eta schedule), and optionally the proximal
    step of an L1 penalty l1 * ||beta||_1 (lasso / elastic net) after every update."""

    rule: str  # "GD" | "AGD"
    alpha: float
    n_samples: int
    grad_scale: float = 1.0
    l1: float = 0.0  # L1 strength (lambda); 0 = no proximal step

    def coeffs(self, i: int, eta: float) -> Tuple[float, float, float, float, int]:
        """(decay, grad_multiplier, l2, theta, rule_code) for round i."""
        gm = eta / self.n_samples * self.grad_scale
        decay = 1.0 - 2.0 * self.alpha * eta
        l2 = 2.0 * self.alpha * eta
        theta = 2.0 / (i + 2.0)
        return decay, gm, l2, theta, (0 if self.rule == "GD" else 1)

    def block_coeffs(self, i: int, etas, alphas):
        """Round i of a sweep run: ([decay_k], [gm_k], [l2_k], theta, rule_code) with model k's step etas[k] and L2
        strength alphas[k] -- each exactly what coeffs() gives a single-model run with that alpha."""
        co = [dataclasses.replace(self, alpha=float(a)).coeffs(i, float(e)) for e, a in zip(etas, alphas)]
        return [c[0] for c in co], [c[1] for c in co], [c[2] for c in co], co[0][3], co[0][4]

    def threshold(self, i: int, eta: float) -> float:
        """Round i's soft threshold t_i = eta_i * l1.  grad_scale does not enter: it rescales the gradient
        multiplier only (avoidstragg), and the penalty is not part of the gradient."""
        return float(eta) * float(self.l1)

    def block_thresholds(self, i: int, etas, l1s):
        """Round i of a sweep run: [t_k] with model k's step etas[k] and L1 strength l1s[k]."""
        return [dataclasses.replace(self, l1=float(l)).threshold(i, float(e)) for e, l in zip(etas, l1s)]

    def apply(self, i: int, eta: float, beta: np.ndarray, u: np.ndarray, g: np.ndarray) -> None:
        """In-place host update (oracle of the combine_update kernel; with l1 > 0 of combine_update_prox: the new
        beta is soft-thresholded and the AGD momentum is formed from the thresholded beta)."""
        decay, gm, l2, theta, code = self.coeffs(i, eta)
        prox = self.l1 > 0
        if code == 0:
            np.subtract(decay * beta, gm * g, out=beta)
            if prox:
                beta[:] = soft_threshold(beta, self.threshold(i, eta))
        else:
            ytemp = (1 - theta) * beta + theta * u
            betatemp = ytemp - gm * g - l2 * beta
            if prox:
                betatemp = soft_threshold(betatemp, self.threshold(i, eta))
            u[:] = beta + (betatemp - beta) * (1 / theta)
            beta[:] = betatemp
