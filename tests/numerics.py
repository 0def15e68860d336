"""Hostile inputs, a long-double oracle and per-column forward-error bounds for the dense kernels.

The older GPU tests draw ``X ~ 0.3 N(0, 1)`` with i.i.d. columns and divide the error by the largest
gradient entry; a column whose gradient is 1e-4 of the largest can then be entirely wrong and pass.
Here the columns of X span four decades of scale, about 5 % of the entries are exact zeros, beta is
scaled so that a large share of the rows saturate (|z| > 30), and every column of a result is held
to its own bound

    bound_j = K u sum_p sum_i (|r_i| + L_p sum_k |x_ik beta_k|) |x_ij|  +  tiny sum_p |c_p| sum_i |x_ij|

with u the accumulator's epsilon (2^-52 fp64, 2^-23 fp32 accumulation of fp32 / bf16 storage), tiny
its smallest normal (a hardware exp2 may flush a denormal sigmoid to zero) and L_p the Lipschitz
constant of the residual in z (|c_p| / 4 logistic, 2 |c_p| least squares and squared hinge).  The
first term is the accumulation error of X^T r, the second the dot product's error carried through
the residual.

K is measured, not chosen: the largest ``err_j / (u sum ...)`` the plain same-precision torch path
(``DenseGradPlan._run_torch`` on CPU tensors) reaches over the grid of tests/test_numerics_cpu.py
(d in {37, 1000, 4097}, n in {1, 65, 257}, three losses, three precisions) is

    MEASURED_CPU_RATIO = 0.72   (0.712: fp64, least squares, d = 37, n = 257; fp32 / bf16 stay below 0.46)

and K = 8 x that, rounded up to a power of two = 8.  The factor 8: the kernels sum lane-strided and
then by tree, not in BLAS order.  K stays orders of magnitude below the worst case (n + d) u.  A
kernel that needs a larger K is a finding to explain, not a reason to raise it; no kernel family has
a K of its own.

The evaluation GEMM uses the same scheme: |dP_ij| <= K u sum_k |x_ik b_jk|, and for the loss sums
sum_i Lip_i dP_ij + K 2^-52 sum_i loss_i (Lip_i = 1 logistic, 2 |y - p| least squares,
2 max(0, 1 - y p) squared hinge; the epilogue sums in fp64 with atomics).

Softmax (C classes, model B [C, d], class blocks of one message): every column of every class block is
held to

    w_ic     = |r_ic| + p_ic + 1/2 max_j sum_k |x_ik B_jk|
    bound_cj = K u sum_p |c_p| sum_i w_ic |x_ij|  +  C tiny sum_p |c_p| sum_i |x_ij|

|r| is the accumulation of X^T r; p: the true class's p - 1 cancels, so its error is absolute in p;
1/2 max: the softmax Jacobian's infinity norm is at most 1/2, applied to the dot products' error;
C tiny: up to C exps flushed to zero per row.  The plain path (SoftmaxGradPlan on CPU tensors, fp64 and
fp32) reaches MEASURED_SOFTMAX_CPU_RATIO = 0.77 over the cases of tests/block_edge_cases.py, which by the
same rule gives K = 8 again (the softmax section below has the case and what sets it).

The oracle computes in ``np.longdouble`` with scipy's overflow-free expit (the softmax oracle: the row's
maximum subtracted before exp) and shares no code with erasurehead_amd.models.losses (only the integer
loss codes are the package's).
"""
import numpy as np
import torch
from scipy.special import expit

LOGISTIC, LEAST_SQUARES, SQUARED_HINGE = 0, 1, 2
LOSSES = (LOGISTIC, LEAST_SQUARES, SQUARED_HINGE)
LOSS_IDS = {LOGISTIC: "logistic", LEAST_SQUARES: "lsq", SQUARED_HINGE: "sqhinge"}

MEASURED_CPU_RATIO = 0.72
K = 8  # 8 x MEASURED_CPU_RATIO, rounded up to a power of two

LD = np.longdouble
SATURATED = 30.0  # |z| beyond which a row counts as saturated


def acc_eps(prec) -> float:
    """Epsilon of the accumulator type."""
    return 2.0 ** -52 if prec.acc == torch.float64 else 2.0 ** -23


def acc_tiny(prec) -> float:
    """Smallest normal of the accumulator type."""
    return float(np.finfo(np.float64 if prec.acc == torch.float64 else np.float32).tiny)


def hostile_partition(rng, n, d, prec):
    """(X [n, ld] storage dtype, y [n] accumulator dtype, fp64 view [n, d] of the stored values).

    N(0, 1) entries scaled per column by 10**U(-3, 1), about 5 % exact zeros, labels +-1, padding
    columns d..ld exactly zero (the engine's contract).  n = 0 gives [0, ld] tensors."""
    scale = 10.0 ** rng.uniform(-3.0, 1.0, d)
    X = rng.randn(n, d) * scale
    X[rng.uniform(size=(n, d)) < 0.05] = 0.0
    y = rng.choice([-1.0, 1.0], n)
    Xp = torch.zeros((n, prec.ld(d)), dtype=torch.float64)
    Xp[:, :d] = torch.from_numpy(X)
    Xs = Xp.to(prec.storage).contiguous()
    return Xs, torch.from_numpy(y).to(prec.acc), Xs[:, :d].double().numpy()


def hostile_beta(rng, d, prec):
    """(beta [ld] accumulator dtype, its fp64 view [d]): randn(d) 10**U(-2, 0.5, d) 30 / sqrt(d), zero
    padding; with hostile_partition's rows a large share of the margins saturate."""
    b = rng.randn(d) * 10.0 ** rng.uniform(-2.0, 0.5, d) * 30.0 / np.sqrt(d)
    beta = torch.zeros(prec.ld(d), dtype=prec.acc)
    beta[:d] = torch.from_numpy(b).to(prec.acc)
    return beta, beta[:d].double().numpy()


def lipschitz(loss, coef):
    """Lipschitz constant of the residual in z."""
    return abs(coef) / 4.0 if loss == LOGISTIC else 2.0 * abs(coef)


def oracle_residual(loss, z, y, coef):
    """r_i in long double: the derivative of coef * loss(y_i, z_i) in z_i."""
    z, y, c = np.asarray(z, LD), np.asarray(y, LD), LD(coef)
    if loss == LOGISTIC:
        return -(c * y) * expit(-(y * z))
    if loss == LEAST_SQUARES:
        return -2 * c * (y - z)
    if loss == SQUARED_HINGE:
        return -2 * c * y * np.maximum(LD(0), 1 - y * z)
    raise ValueError(f"unknown loss {loss}")


def oracle_segment(loss, Xh, yh, bh, coef):
    """One segment: (gradient [d], K-free bound sum [d], sum_i |x_ij| [d], z [n]) in long double."""
    X, b = np.asarray(Xh, LD), np.asarray(bh, LD)
    z = X @ b
    r = oracle_residual(loss, z, yh, coef)
    aX = np.abs(X)
    w = np.abs(r) + LD(lipschitz(loss, coef)) * (aX @ np.abs(b))
    return X.T @ r, aX.T @ w, aX.sum(0), z


def oracle_message(loss, segments, host, bh, prec, k=K):
    """(gradient, per-column bound) of one message; segments = [(partition, coef)], host[p] = (X, y)."""
    d = len(bh)
    g, acc, tiny = np.zeros(d, LD), np.zeros(d, LD), np.zeros(d, LD)
    for p, coef in segments:
        gs, ws, ax, _ = oracle_segment(loss, host[p][0], host[p][1], bh, coef)
        g += gs
        acc += ws
        tiny += abs(coef) * ax
    return g, LD(k * acc_eps(prec)) * acc + LD(acc_tiny(prec)) * tiny


def column_ratio(got, ref, bound):
    """Largest |got_j - ref_j| / bound_j over the columns (0 / 0 counts as 0, x / 0 as inf)."""
    err = np.abs(np.asarray(got, LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, LD(0), err / bound)
    return float(np.max(q)) if q.size else 0.0


def check_columns(got, ref, bound, what="", k=K):
    """Every column within its own bound; the message names the worst column."""
    assert np.all(np.isfinite(np.asarray(got, np.float64))), f"{what}: non-finite entries (unwritten or overflowed)"
    err = np.abs(np.asarray(got, LD) - ref)
    bad = np.nonzero(~(err <= bound))[0]
    if bad.size:
        j = bad[np.argmax((err[bad] / np.maximum(bound[bad], np.finfo(LD).tiny)))]
        raise AssertionError(f"{what}: {bad.size} of {err.size} columns beyond their bound; worst column {j}: "
                             f"got {float(got[j])!r} ref {float(ref[j])!r} err {float(err[j]):.3e} "
                             f"bound {float(bound[j]):.3e} (K = {k})")


# ---- sparse partitions ----------------------------------------------------------------------------
# The sparse kernels (csrc/kernels/grad_sparse.hip, eval_sparse.hip) are held to the same bound formula with a
# constant of their own, measured by the same rule: the plain same-precision scipy path -- CSR ``X.dot(b)``, the
# residual in the accumulator dtype, ``X.T.dot(r)``, in float64 and in float32 -- over every gradient case of
# tests/sparse_edge_cases.py (the loop is tests/test_sparse_edge_cases_cpu.py
# test_measured_sparse_ratio_is_current) reaches at most
#
#     MEASURED_SPARSE_CPU_RATIO   (the case, message and column that set it: MEASURED_SPARSE_CPU_CASE)
#
# and K_SPARSE = 8 x that, rounded up to a power of two.  What sets it: scipy adds a column's entries one after
# the other, and a pattern-only column whose rows hold one or two entries carries the same |r| thousands of times
# (z takes one or two values), so the roundings of the running sum share a sign and the error grows with the
# column's length (41.4 and 21.2 at the 4096-entry column of the multitile cases, 26.0 at the 924-entry one of
# the columns cases, 14.8 at ragged d = 1); valued cases stay below 3.7, every case of 5 or more entries per row
# below 1.9.  The dense constant K above is untouched.
# On an MI355X the kernels (tiles summed by lane, scan and tile) stayed within 0.0025 of the K_SPARSE bound,
# 1.3 u sum ..., on every case (columns-fp32-val-d5000-logistic).
MEASURED_SPARSE_CPU_RATIO = 41.5
MEASURED_SPARSE_CPU_CASE = "multitile-fp64-pat-d37-logistic message 0 column 5 (41.42)"
K_SPARSE = 512


def sparse_k_rule(ratio: float) -> int:
    """8 x the measured ratio, rounded up to a power of two."""
    return int(2 ** int(np.ceil(np.log2(8.0 * ratio))))


def hostile_sparse_partition(rng, n, d, counts, valued, prec):
    """(scipy CSR [n, d], y [n] float64): row i holds a number of non-zeros drawn from ``counts`` (0 allowed; at most
    d), in sorted columns without duplicates.  valued: N(0, 1) entries scaled per column by 10**U(-3, 1) and
    rounded to the accumulator type (what the plan stores); else every entry is exactly 1.0.  Labels +-1."""
    import scipy.sparse as sps

    assert n * d <= 2 ** 24, "a dense [n, d] key matrix is drawn: keep the case small"
    counts = np.minimum(np.asarray(counts, dtype=np.int64), d)
    c = counts[rng.randint(0, len(counts), n)] if n else np.zeros(0, dtype=np.int64)
    order = np.argsort(rng.uniform(size=(n, d)), axis=1)  # a random permutation of the columns per row
    cols = np.sort(np.where(np.arange(d)[None, :] < c[:, None], order, d), axis=1)  # the first c of it, sorted
    cols = cols[cols < d].astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
    if valued:
        scale = 10.0 ** rng.uniform(-3.0, 1.0, d)
        npacc = np.float64 if prec.acc == torch.float64 else np.float32
        data = (rng.randn(cols.size) * scale[cols]).astype(npacc).astype(np.float64)
    else:
        data = np.ones(cols.size)
    y = rng.choice([-1.0, 1.0], n)
    return sps.csr_matrix((data, cols, indptr), shape=(n, d)), y


def hostile_sparse_beta(rng, d, prec, mean_nnz):
    """hostile_beta for rows of ``mean_nnz`` entries on average: randn(d) 10**U(-2, 0.5, d) 30 / sqrt(max(1, mean_nnz)),
    so a large share of the margins saturate whatever the rows' length."""
    b = rng.randn(d) * 10.0 ** rng.uniform(-2.0, 0.5, d) * 30.0 / np.sqrt(max(1.0, mean_nnz))
    beta = torch.zeros(prec.ld(d), dtype=prec.acc)
    beta[:d] = torch.from_numpy(b).to(prec.acc)
    return beta, beta[:d].double().numpy()


def oracle_sparse_segment(loss, A, yh, bh, coef):
    """oracle_segment from the COO triplets of a scipy matrix: (gradient [d], K-free bound sum [d], sum_i |x_ij| [d],
    z [n]) in long double."""
    C = A.tocoo()
    n, d = C.shape
    rows, cols, x = C.row, C.col, np.asarray(C.data, LD)
    b = np.asarray(bh, LD)
    xb = x * b[cols]
    z, az = np.zeros(n, LD), np.zeros(n, LD)
    np.add.at(z, rows, xb)
    np.add.at(az, rows, np.abs(xb))
    r = oracle_residual(loss, z, yh, coef)
    w = np.abs(r) + LD(lipschitz(loss, coef)) * az
    g, acc, ax = np.zeros(d, LD), np.zeros(d, LD), np.zeros(d, LD)
    np.add.at(g, cols, x * r[rows])
    np.add.at(acc, cols, np.abs(x) * w[rows])
    np.add.at(ax, cols, np.abs(x))
    return g, acc, ax, z


def oracle_sparse_terms(loss, segments, host, bh):
    """(gradient, sum_p sum_i (|r_i| + L_p sum_k |x_ik beta_k|) |x_ij|, sum_p |c_p| sum_i |x_ij|) of one message over
    scipy partitions: segments = [(partition, coef)], host[p] = (CSR, y)."""
    d = len(bh)
    g, acc, tiny = np.zeros(d, LD), np.zeros(d, LD), np.zeros(d, LD)
    for p, coef in segments:
        gs, ws, ax, _ = oracle_sparse_segment(loss, host[p][0], host[p][1], bh, coef)
        g += gs
        acc += ws
        tiny += abs(coef) * ax
    return g, acc, tiny


def sparse_bound(acc, tiny, prec, k=None):
    k = K_SPARSE if k is None else k
    return LD(k * acc_eps(prec)) * acc + LD(acc_tiny(prec)) * tiny


def oracle_sparse_message(loss, segments, host, bh, prec, k=None):
    """oracle_message over scipy partitions.  A column no partition of the message has an entry in, and every
    column of a message of coefficient 0, has bound 0: the result must be exactly 0 there."""
    g, acc, tiny = oracle_sparse_terms(loss, segments, host, bh)
    return g, sparse_bound(acc, tiny, prec, k)


# ---- softmax (blocked model: C classes) -------------------------------------------------------------
# The softmax kernel (csrc/kernels/grad_softmax.hip) is held to the bound of the header's softmax paragraph, its
# constant measured by the same rule: the plain same-precision path is SoftmaxGradPlan on CPU tensors
# (softmax_grad_torch), in fp64 and fp32, over every case of tests/block_edge_cases.py softmax_cases() and both
# message sets (the loop is tests/test_block_edge_cases_cpu.py test_measured_softmax_ratio_is_current), and its largest
# err_cj / (u sum_p |coef_p| sum_i w_ic |x_ij| + C tiny ...) is
#
#     MEASURED_SOFTMAX_CPU_RATIO   (the case, message, class and column that set it: MEASURED_SOFTMAX_CPU_CASE)
#
# That is just above the dense MEASURED_CPU_RATIO (0.72), so sparse_k_rule applies: 8 x 0.77 rounded up to a power of
# two is 8 again, K_SOFTMAX = K, and the softmax kernel has no constant of its own.  What sets it: the logits of the
# offset model, in either precision (fp64 reaches 0.751).  |z| is hundreds there, so a logit carries an absolute error
# of about u sum_k |x_ik B_ck| into a softmax whose logits differ by O(1) -- the 1/2 max_j sum_k |x_ik B_jk| term of
# w -- and a 16-row partition has no room to average it out.  The saturated model (residuals of exactly 0 and -1 in
# most rows) stays below 0.28.
# On an MI355X the kernel (lane-strided dot products, DPP softmax, per-wave slab rows) stayed within 0.06 of the
# K_SOFTMAX bound, 0.48 u sum ..., on every case (fp32-d1-C5-offset, naive messages, whole tasks).
MEASURED_SOFTMAX_CPU_RATIO = 0.77
MEASURED_SOFTMAX_CPU_CASE = "fp32-d256-C3-offset naive message 4 class 0 (0.763)"
K_SOFTMAX = 8  # sparse_k_rule(MEASURED_SOFTMAX_CPU_RATIO): the dense K


def hostile_class_labels(rng, n, C, prec):
    """(y [n] accumulator dtype, its float64 NumPy copy): class indices uniform in 0..C-1.  The callers make sure
    that some partition lacks class C - 1 and that the one-row partition exists."""
    y = rng.randint(0, C, n).astype(np.float64)
    return torch.from_numpy(y).to(prec.acc), y


def _class_major(blocks, d, prec):
    ld = prec.ld(d)
    beta = torch.zeros((len(blocks), ld), dtype=prec.acc)
    beta[:, :d] = torch.from_numpy(np.stack(blocks)).to(prec.acc)
    return beta.reshape(-1).contiguous(), beta[:, :d].double().numpy()


def hostile_softmax_models(rng, host, d, C, prec):
    """{"saturated", "offset"}: each (beta [C * ld] accumulator dtype, class-major with zero padding; its fp64 view
    [C, d]).  host[p] = (fp64 view of X, ...) gives the column scales the offset model is built for.

    saturated: C independent hostile_beta draws -- one class takes probability exactly 1.0 in many rows and the other
               exps underflow.
    offset:    B_c = b + delta_c, b one hostile_beta draw (a common logit of hundreds that only the max subtraction
               removes) and delta_c[j] = 1.5 randn / (sqrt(d) rms_j), rms_j the root mean square of column j over all
               partitions (1 where that is 0): the logits differ by O(1) while |z| is large."""
    sat = [hostile_beta(rng, d, prec)[1] for _ in range(C)]
    b = hostile_beta(rng, d, prec)[1]
    rows = sum(X.shape[0] for X, *_ in host.values())
    sq = sum((np.asarray(X, np.float64) ** 2).sum(0) for X, *_ in host.values())
    rms = np.sqrt(sq / max(1, rows))
    rms = np.where(rms == 0, 1.0, rms)
    off = [b + 1.5 * rng.randn(d) / (np.sqrt(d) * rms) for _ in range(C)]
    return {"saturated": _class_major(sat, d, prec), "offset": _class_major(off, d, prec)}


def oracle_softmax_probs(Xh, Bh):
    """(p [n, C], z [n, C]) in long double, the row's maximum subtracted before the exp."""
    Z = np.asarray(Xh, LD) @ np.asarray(Bh, LD).T
    with np.errstate(under="ignore"):
        E = np.exp(Z - Z.max(axis=1, keepdims=True)) if Z.size else Z
    return E / np.maximum(E.sum(axis=1, keepdims=True), LD(1)), Z


def oracle_softmax_segment(Xh, yh, Bh):
    """One segment with coefficient 1: (gradient [C, d], K-free bound sum_i w_ic |x_ij| [C, d], sum_i |x_ij| [d]) in
    long double, w_ic = |r_ic| + p_ic + 1/2 max_j sum_k |x_ik B_jk|."""
    X, B = np.asarray(Xh, LD), np.asarray(Bh, LD)
    P, _ = oracle_softmax_probs(X, B)
    R = P.copy()
    R[np.arange(X.shape[0]), np.asarray(yh).astype(np.int64)] -= LD(1)
    aX = np.abs(X)
    dots = (aX @ np.abs(B).T).max(axis=1, keepdims=True) if X.shape[0] else np.zeros((0, 1), LD)
    W = np.abs(R) + P + LD(0.5) * dots
    return R.T @ X, W.T @ aX, aX.sum(0)


def oracle_softmax_terms(segments, host, Bh):
    """(gradient, sum_p |coef_p| sum_i w_ic |x_ij|, sum_p |coef_p| sum_i |x_ij|), [C, d] each, of one message:
    segments = [(partition, coef)], host[p] = (X, y)."""
    C, d = np.shape(Bh)
    g, acc, tiny = np.zeros((C, d), LD), np.zeros((C, d), LD), np.zeros((C, d), LD)
    for p, coef in segments:
        gs, ws, ax = oracle_softmax_segment(host[p][0], host[p][1], Bh)
        g += LD(coef) * gs
        acc += LD(abs(coef)) * ws
        tiny += LD(abs(coef)) * ax[None, :]
    return g, acc, tiny


def softmax_bound(acc, tiny, C, prec, k=K_SOFTMAX):
    return LD(k * acc_eps(prec)) * acc + LD(C * acc_tiny(prec)) * tiny


def oracle_softmax_message(segments, host, Bh, prec, k=K_SOFTMAX):
    """(gradient [C, d], per-class, per-column bound [C, d]) of one softmax message."""
    g, acc, tiny = oracle_softmax_terms(segments, host, Bh)
    return g, softmax_bound(acc, tiny, np.shape(Bh)[0], prec, k)


# ---- evaluation GEMM ------------------------------------------------------------------------------
def oracle_eval(loss, Xh, yh, Bh, prec, k=K):
    """(P [n, R], bound on P, loss sums [R], bound on the sums) in long double."""
    X, B, y = np.asarray(Xh, LD), np.asarray(Bh, LD), np.asarray(yh, LD)[:, None]
    P = X @ B.T
    dP = LD(k * acc_eps(prec)) * (np.abs(X) @ np.abs(B).T)
    if loss == LOGISTIC:
        m = -y * P
        per = np.maximum(m, 0) + np.log1p(np.exp(-np.abs(m)))
        lip = np.ones_like(P)
    elif loss == LEAST_SQUARES:
        per = (y - P) ** 2
        lip = 2 * np.abs(y - P)
    else:
        h = np.maximum(LD(0), 1 - y * P)
        per = h * h
        lip = 2 * h
    return P, dP, per.sum(0), (lip * dP).sum(0) + LD(k * 2.0 ** -52) * per.sum(0)
