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


def curvature(kind: int, z, y) -> np.ndarray:
    """The second derivative l''(z) of the per-row loss whose first derivative is the worker gradient's residual:
    logistic s (1 - s) with s = sigmoid(-y z), least squares 2, squared hinge 2 where y z < 1 and 0 elsewhere."""
    z, y = np.asarray(z, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if kind == LOGISTIC:
        s = _sigmoid_neg(y * z)
        return s * (1.0 - s)
    if kind == LEAST_SQUARES:
        return np.full_like(z, 2.0)
    if kind == SQUARED_HINGE:
        return np.where(1.0 - y * z > 0.0, 2.0, 0.0)
    raise ValueError(f"preconditioned: loss kind {kind} is not logistic, least squares or squared hinge")


def precond_grad(kind: int, X, y: np.ndarray, beta: np.ndarray, coef=None) -> np.ndarray:
    """[2, d]: row 0 the scalar-loss gradient sum r_i x_i at beta, row 1 the diagonal of its Hessian
    sum l''(z_i) x_i^2 (what one partition contributes to a --precondition diag message, times coef)."""
    X = np.asarray(X, dtype=np.float64)
    w = curvature(kind, X.dot(beta), y)
    h = (X * X).T.dot(w)
    return np.stack([_GRADS[kind](X, y, beta, coef), h if coef is None else coef * h])


def precond_unpack(betaset: np.ndarray, d_x: Optional[int] = None) -> np.ndarray:
    """[R, 2 * ld_x] trajectory of a --precondition diag run (as the engine stores it) -> block 0 [R, d_x], the
    model (d_x absent: all ld_x columns); block 1 is the curvature diagonal's place on the wire and stays zero."""
    b = np.asarray(betaset)
    b = b.reshape(1, -1) if b.ndim == 1 else b
    if b.shape[1] % 2 or (d_x is not None and b.shape[1] // 2 < d_x):
        raise ValueError(f"model length {b.shape[1]} is not two blocks of >= {d_x or 1} columns")
    return b[:, : (b.shape[1] // 2 if d_x is None else int(d_x))]


def hvp_grad(kind: int, X, y: np.ndarray, beta: np.ndarray, v: np.ndarray, coef=None) -> np.ndarray:
    """[2, d]: row 0 the scalar-loss gradient sum r_i x_i at beta, row 1 its Hessian applied to v,
    sum l''(z_i) (x_i . v) x_i (what one partition contributes to a --newton-cg message, times coef)."""
    X = np.asarray(X, dtype=np.float64)
    u = X.T.dot(curvature(kind, X.dot(beta), y) * X.dot(v))
    return np.stack([_GRADS[kind](X, y, beta, coef), u if coef is None else coef * u])


def newton_unpack(betaset: np.ndarray, d_x: Optional[int] = None) -> np.ndarray:
    """[R, 2 * ld_x] trajectory of a --newton-cg run (as the engine stores it) -> block 0 [R, d_x], the model (d_x
    absent: all ld_x columns); block 1 is the CG direction's place on the wire and is zero in every stored row."""
    return precond_unpack(betaset, d_x)


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
class LbfgsState:
    """What the oracle UpdateRule.step_lbfgs remembers between rounds (the engines keep ops/update.py lbfgs_state):
    at most `memory` accepted pairs (s, y), oldest first, and the previous round's beta and gradient (None before the
    first round)."""

    memory: int
    pairs: list = dataclasses.field(default_factory=list)
    beta_prev: Optional[np.ndarray] = None
    g_prev: Optional[np.ndarray] = None


@dataclass
class NewtonState:
    """What the oracle UpdateRule.step_newton remembers between rounds (the engines keep ops/update.py newton_state):
    the accumulated step x, the CG residual r, the direction (what the next round's workers apply the Hessian to; zeros
    before a gradient round), the gradient g0 at the outer iterate, rs = r . r, g0norm2 = g0 . g0, and the counters
    phase (0: a gradient round is next, 1: a CG round), inner (CG steps taken in this outer iteration), mode (the last
    round's, NEWTON_MODES) and outer (outer iterations finished)."""

    x: Optional[np.ndarray] = None
    r: Optional[np.ndarray] = None
    direction: Optional[np.ndarray] = None
    g0: Optional[np.ndarray] = None
    rs: float = 0.0
    g0norm2: float = 0.0
    phase: int = 0
    inner: int = 0
    mode: int = 0
    outer: int = 0


# the last round's mode (csrc/kernels/launchers.h NewtonMode)
NEWTON_MODES = ("start", "continue", "step-tolerance", "step-cap", "step-curvature", "gd-curvature", "gd-gradient")


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

    def precond_coeffs(self, i: int, eta: float) -> Tuple[float, float, float, float, int]:
        """(eta, gs, l2c, theta, rule_code) of round i's preconditioned step: gs = gm / eta is the scale coeffs()
        gives the gradient (1 / n, avoidstragg's rescale included) and l2c = 2 alpha the L2 term's curvature."""
        _, _, _, theta, code = self.coeffs(i, eta)
        return float(eta), self.grad_scale / self.n_samples, 2.0 * self.alpha, theta, code

    def step_precond(self, i: int, eta: float, beta: np.ndarray, u: np.ndarray, g: np.ndarray, h: np.ndarray,
                     damping: float) -> None:
        """In-place Jacobi-preconditioned (diagonal-Newton) update from the decoded gradient g and curvature diagonal
        h (oracle of combine_update_precond): P = gs max(h, 0) + 2 alpha + damping, step = eta (gs g + 2 alpha beta) / P,
        GD beta -= step, AGD as apply() with the step in place of gm g + l2 beta."""
        if not (np.isfinite(damping) and damping > 0):
            raise ValueError(f"--precondition-damping must be finite and > 0, got {damping}")
        eta, gs, l2c, theta, code = self.precond_coeffs(i, eta)
        P = gs * np.where(h < 0, 0.0, h) + l2c + damping
        step = eta * (gs * g + l2c * beta) / P
        if code == 0:
            beta -= step
        else:
            betatemp = (1 - theta) * beta + theta * u - step
            u[:] = beta + (betatemp - beta) * (1 / theta)
            beta[:] = betatemp

    def lbfgs_coeffs(self, i: int, eta: float) -> Tuple[float, float, float]:
        """(eta, gs, l2c) of round i's L-BFGS step: the gradient is G = gs g + l2c beta, as precond_coeffs'."""
        if self.rule != "GD":
            raise ValueError("--lbfgs: the update rule must be GD")
        return float(eta), self.grad_scale / self.n_samples, 2.0 * self.alpha

    def step_lbfgs(self, i: int, eta: float, beta: np.ndarray, g: np.ndarray, state: "LbfgsState", tau: float) -> int:
        """In-place limited-memory BFGS update from the decoded message sum g: the textbook two-loop recursion over
        full-length vectors.  An oracle only: the engines, CPU and GPU, step through ops/update.py lbfgs_update, which
        reads the same dot products off a Gram matrix; this second formulation is what replays hold them to.  Returns
        the step's mode: 0 quasi-Newton, 1 GD (no pair held), 2 GD and the ring emptied."""
        eta, gs, l2c = self.lbfgs_coeffs(i, eta)
        b = beta.copy()
        with np.errstate(all="ignore"):
            G = gs * g + l2c * b
            if state.beta_prev is not None:
                s, y = b - state.beta_prev, G - state.g_prev
                sy, ss, yy = s.dot(y), s.dot(s), y.dot(y)
                if np.isfinite([sy, ss, yy]).all() and sy > 1e-8 * np.sqrt(ss * yy):
                    state.pairs = (state.pairs + [(s, y)])[-state.memory:]
            mode, q = 1, G
            if state.pairs:
                q, a = G.copy(), []
                for s, y in reversed(state.pairs):
                    a.append(s.dot(q) / s.dot(y))
                    q -= a[-1] * y
                s, y = state.pairs[-1]
                q *= s.dot(y) / y.dot(y)
                for (s, y), aj in zip(state.pairs, reversed(a)):
                    q += (aj - y.dot(q) / s.dot(y)) * s
                gp = G.dot(q)
                mode = 0 if np.isfinite(gp) and gp > 0 else 2
            if mode == 2:
                state.pairs = []
            beta -= tau * q if mode == 0 else eta * G
        state.beta_prev, state.g_prev = b, G
        return mode

    def newton_coeffs(self, i: int, eta: float) -> Tuple[float, float, float]:
        """(eta, gs, l2c) of round i's Newton-CG step: G = gs g + l2c beta and H v = gs u + l2c v, as lbfgs_coeffs'."""
        if self.rule != "GD":
            raise ValueError("--newton-cg: the update rule must be GD")
        return float(eta), self.grad_scale / self.n_samples, 2.0 * self.alpha

    def step_newton(self, i: int, eta: float, beta: np.ndarray, g: np.ndarray, u: np.ndarray, state: "NewtonState",
                    J: int, xi: float, tau: float) -> int:
        """One round of truncated Newton (Newton-CG) in place, from the decoded message sums g (block 0) and u (block
        1: the loss Hessian applied to state.direction): the plain vector-space recurrences of linear CG on
        H x = -G, one step per round.  beta moves only in the round that ends an outer iteration; state.direction is
        what the next round's workers need in block 1 (zeros after such a round).  Returns the round's mode (an index
        into NEWTON_MODES).  The oracle of csrc/kernels/newton_cg.hip and the step of the Python round loop."""
        eta, gs, l2c = self.newton_coeffs(i, eta)
        s = state
        ok = lambda v: bool(np.isfinite(v) and v > 0)  # noqa: E731
        with np.errstate(all="ignore"):
            if s.phase != 1:
                G = gs * g + l2c * beta
                rs = float(G.dot(G))
                s.g0, s.inner = G, 0
                if ok(rs):
                    s.x, s.r, s.direction = np.zeros_like(G), -G, -G
                    s.rs = s.g0norm2 = rs
                    s.mode = 0
                else:
                    s.mode = 6
            else:
                Hv = gs * u + l2c * s.direction
                kappa = float(s.direction.dot(Hv))
                if not ok(kappa):
                    s.mode = 5 if s.inner == 0 else 4
                else:
                    a = s.rs / kappa
                    s.x = s.x + a * s.direction
                    s.r = s.r - a * Hv
                    rs = float(s.r.dot(s.r))
                    s.inner += 1
                    if not rs > xi * xi * s.g0norm2:
                        s.mode = 2
                    elif s.inner >= J:
                        s.mode = 3
                    else:
                        s.mode = 1
                        s.direction = s.r + (rs / s.rs) * s.direction
                        s.rs = rs
            if s.mode in (0, 1):
                s.phase = 1
            else:
                beta += -eta * s.g0 if s.mode >= 5 else tau * s.x
                s.phase, s.outer = 0, s.outer + 1
                s.direction = np.zeros_like(beta)
        return s.mode

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
