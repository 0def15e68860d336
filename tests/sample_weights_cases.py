"""Oracle, bounds, inputs and case tables of tests/test_sample_weights_cpu.py and tests/test_sample_weights_gpu.py.
A plain module (no GPU, no tests).

The weighted codes read a label y~ = s * w: the class s is the sign BIT of y~ (so -0.0 is a negative row of
weight 0) and the weight w = |y~| >= 0.  The oracle below computes in ``np.longdouble`` from (s, w) and shares no
code with erasurehead_amd.models.losses (only the integer codes are the package's).

The per-column bound is tests/numerics.py's with the row's weight in the Lipschitz constant and the tiny term:

    bound_j = K u sum_i (|r_i| + L_i sum_k |x_ik beta_k|) |x_ij|  +  tiny |c| sum_i w_i |x_ij|

L_i = w_i |c| / 4 for the logistic code, 2 w_i |c| for the hinge code, K = numerics.K = 8, u and tiny the
accumulator's epsilon and smallest normal (numerics.acc_eps / acc_tiny).
"""
import numpy as np
import torch
from scipy.special import expit

import numerics as nx

LOGISTIC_W, SQUARED_HINGE_W = 4, 5
WEIGHTED = (LOGISTIC_W, SQUARED_HINGE_W)
BASE = {LOGISTIC_W: nx.LOGISTIC, SQUARED_HINGE_W: nx.SQUARED_HINGE}  # the unweighted code each one extends
IDS = {LOGISTIC_W: "logistic_w", SQUARED_HINGE_W: "sqhinge_w"}
LD = nx.LD
SIZES = (257, 64, 1, 0)  # rows of the dense partitions: more than one block, a short one, one row, none
EMPTY = 3


# ---- labels and weights ---------------------------------------------------------------------------
def split(yt):
    """(s, w) of weighted labels: the sign bit and the magnitude."""
    yt = np.asarray(yt, dtype=np.float64)
    return np.where(np.signbit(yt), -1.0, 1.0), np.abs(yt)


def hostile_weights(rng, n, zeros=0.05):
    """w = 10**U(-2, 2) with about 5 % exact zeros."""
    w = 10.0 ** rng.uniform(-2.0, 2.0, n)
    w[rng.uniform(size=n) < zeros] = 0.0
    return w


def carry(y, w):
    """y~ = y * w for labels y in {-1, +1}: a zero weight keeps its class as +0.0 / -0.0."""
    return np.asarray(y, dtype=np.float64) * np.asarray(w, dtype=np.float64)


def mixed_zeros(rng, n):
    """n labels of weight 0 with both zero signs (at least one of each from n = 2 on)."""
    z = np.where(rng.uniform(size=n) < 0.5, -0.0, 0.0)
    if n >= 2:
        z[0], z[1] = 0.0, -0.0
    return z


# ---- long-double oracle ---------------------------------------------------------------------------
def lipschitz(loss, coef, w):
    """Per-row Lipschitz constant of the residual in z."""
    w = np.asarray(w, LD)
    return w * LD(abs(coef)) / 4 if loss == LOGISTIC_W else 2 * w * LD(abs(coef))


def residual(loss, z, yt, coef):
    """r_i: the derivative of coef * w_i * loss(s_i, z_i) in z_i."""
    s, w = split(yt)
    z, s, w, c = np.asarray(z, LD), np.asarray(s, LD), np.asarray(w, LD), LD(coef)
    if loss == LOGISTIC_W:
        return -(c * s * w) * expit(-(s * z))
    if loss == SQUARED_HINGE_W:
        return -2 * c * s * w * np.maximum(LD(0), 1 - s * z)
    raise ValueError(f"not a weighted code: {loss}")


def row_loss(loss, yt, p):
    """w_i * loss(s_i, p_i) [n, R] and its Lipschitz constant in p, in long double; p is [n, R]."""
    s, w = split(yt)
    s, w, p = np.asarray(s, LD)[:, None], np.asarray(w, LD)[:, None], np.asarray(p, LD)
    t = s * p
    if loss == LOGISTIC_W:
        return w * (np.maximum(-t, 0) + np.log1p(np.exp(-np.abs(t)))), w * np.ones_like(p)
    h = np.maximum(LD(0), 1 - t)
    return w * h * h, 2 * w * h


def segment(loss, Xh, yt, bh, coef):
    """One segment: (gradient [d], K-free bound sum [d], sum_i w_i |x_ij| [d]) in long double."""
    X, b = np.asarray(Xh, LD), np.asarray(bh, LD)
    z = X @ b
    r = residual(loss, z, yt, coef)
    aX = np.abs(X)
    t = np.abs(r) + lipschitz(loss, coef, split(yt)[1]) * (aX @ np.abs(b))
    return X.T @ r, aX.T @ t, aX.T @ np.asarray(split(yt)[1], LD)


def message(loss, segments, host, bh, prec, k=nx.K):
    """(gradient, per-column bound) of one message; segments = [(partition, coef)], host[p] = (X fp64 [n, d], y~)."""
    d = len(bh)
    g, acc, tiny = np.zeros(d, LD), np.zeros(d, LD), np.zeros(d, LD)
    for p, coef in segments:
        gs, ws, ax = segment(loss, host[p][0], host[p][1], bh, coef)
        g += gs
        acc += ws
        tiny += abs(coef) * ax
    return g, LD(k * nx.acc_eps(prec)) * acc + LD(nx.acc_tiny(prec)) * tiny


def sequential_message(loss, segments, host, bh, dtype):
    """The plain reference of the bound's check: every sum strictly sequential in ``dtype`` (over the columns
    of each row's dot product, then over the rows), the residual through the dtype's own exp."""
    f = np.dtype(dtype).type
    d = len(bh)
    g = np.zeros(d, dtype)
    b = np.asarray(bh, dtype)
    for p, coef in segments:
        X, (s, w) = np.asarray(host[p][0], dtype), split(host[p][1])
        yt = np.asarray(host[p][1], dtype)
        for i in range(X.shape[0]):
            z = f(0)
            for k in range(d):
                z = f(z + X[i, k] * b[k])
            t = f(-z) if s[i] < 0 else z
            if loss == LOGISTIC_W:
                e = np.exp(f(-abs(t)))
                r = f(-(f(coef) * yt[i])) * (f(e / f(f(1) + e)) if t > 0 else f(f(1) / f(f(1) + e)))
            else:
                r = f(f(-2) * f(f(coef) * yt[i])) * max(f(0), f(f(1) - t))
            for j in range(d):
                g[j] = f(g[j] + r * X[i, j])
    return g


def evaluation(loss, Xh, yt, Bh, prec, k=nx.K):
    """(P [n, R], bound on P, weighted loss sums [R], bound on the sums): numerics.oracle_eval's form, the
    per-row Lipschitz factor scaled by w_i."""
    X, B = np.asarray(Xh, LD), np.asarray(Bh, LD)
    P = X @ B.T
    dP = LD(k * nx.acc_eps(prec)) * (np.abs(X) @ np.abs(B).T)
    per, lip = row_loss(loss, yt, P)
    return P, dP, per.sum(0), (lip * dP).sum(0) + LD(k * 2.0 ** -52) * per.sum(0)


# ---- inputs ---------------------------------------------------------------------------------------
def dense_case(prec, d, sizes=SIZES, seed=0, plain_x=False):
    """Hostile partitions (numerics.hostile_partition; plain_x: N(0, 1) rows, which fit the 58-bit window whole)
    with +-1 labels, hostile weights per partition, a hostile beta.  Returns (parts {p: (X, y +-1)}, weights {p: w},
    host {p: X fp64 [n, d]}, beta [ld], bh [d]), all on the CPU."""
    rng = np.random.RandomState((7919 * d + 31 * sum(sizes) + 977 * seed + prec.code) % 2 ** 31)
    parts, weights, host = {}, {}, {}
    for p, n in enumerate(sizes):
        X, y, Xh = nx.hostile_partition(rng, n, d, prec)
        if plain_x:
            X = torch.zeros((n, prec.ld(d)), dtype=torch.float64)
            X[:, :d] = torch.from_numpy(rng.randn(n, d))
            X = X.to(prec.storage).contiguous()
            Xh = X[:, :d].double().numpy()
        parts[p], weights[p], host[p] = (X, y), hostile_weights(rng, n), Xh
    beta, bh = nx.hostile_beta(rng, d, prec)
    return parts, weights, host, beta, bh


def labels(parts, weights, prec, which):
    """{p: y} in the accumulator dtype: "unit" the +-1 labels, "hostile" y * w, "zero" weight 0 with mixed zero signs."""
    out = {}
    for p, (_, y) in parts.items():
        yh = y.double().numpy()
        if which == "hostile":
            yh = carry(yh, weights[p])
        elif which == "zero":
            yh = mixed_zeros(np.random.RandomState(p), len(yh))
        out[p] = torch.from_numpy(np.ascontiguousarray(yh)).to(prec.acc)
    return out


def distinct_messages(empty=True):
    """Every partition in one message: two segments, a negative coefficient, and (``empty``) the empty partition
    next to a non-empty one and a last message of the empty partition alone."""
    if not empty:
        return [[(0, 1.0), (1, -0.7)], [(2, 2.5)]]
    return [[(0, 1.0), (1, -0.7)], [(2, 2.5), (EMPTY, 1.0)], [(EMPTY, 1.0)]]


def replica_messages(R, empty=True):
    """Partition 0 read by R messages, partition 1 by min(R, 2); the rest as distinct_messages."""
    msgs = [[(0, 1.0), (1, -0.7)]]
    for q in range(1, R):
        msgs.append([(0, 0.5 + 0.25 * q)] + ([(1, 2.0)] if q == 1 else []))
    return msgs + distinct_messages(empty)[1:]


def dense_families():
    """[(id, precision, d, replicas, KernelChoice kwargs or None, pack)]: every dense kernel family a plan can
    select, reached with the forced choices of tests/dense_edge_cases.py: fused (one row in flight), pair (the
    interleaved two-row kernel), one-wave bundles of 1 / 2 / 3, LDS-staged bundles of 4, wide rows, two-pass, in
    fp64, fp32 and fp32x64; the packed 58-bit stream (fp64); bf16 MFMA bundles.  d in {37, 1000} where the family
    allows it: wide rows start past 2048 columns, the two-pass path past the widest one-pass row.  pack: the plan is
    built with pack=True over N(0, 1) rows (they fit the 58-bit window whole) and without the empty partition (the
    packer's own tests, tests/test_pack58_gpu.py, pack non-empty partitions only)."""
    from erasurehead_amd.ops import get_precision
    from erasurehead_amd.ops.grad import wide_ept

    out = []
    for pn in ("fp64", "fp32", "fp32x64"):
        twopass_d = 512 * wide_ept(get_precision(pn)) + 1
        for d in (37, 1000):
            out.append((f"{pn}-fused-d{d}", pn, d, 1, dict(kind="fused", rows=1), False))
            out.append((f"{pn}-pair-d{d}", pn, d, 1, dict(kind="fused", rows=2), False))
            for R in (1, 2, 3):
                out.append((f"{pn}-multi-R{R}-d{d}", pn, d, R,
                            dict(kind="multi", replicas=R, bundle_rows=32, fold=True, lane_epi=R > 1), False))
            out.append((f"{pn}-staged-R4-d{d}", pn, d, 4, dict(kind="staged", replicas=4, bundle_rows=32), False))
        out.append((f"{pn}-wide-d3000", pn, 3000, 1, dict(kind="wide"), False))
        out.append((f"{pn}-twopass-d{twopass_d}", pn, twopass_d, 1, dict(kind="twopass"), False))
    out.append(("fp64-p58-R3-d1000", "fp64", 1000, 3,
                dict(kind="multi", replicas=3, bundle_rows=32, fold=True, lane_epi=True), True))
    for d in (37, 1000):
        out.append((f"bf16-mfma-R3-d{d}", "bf16", d, 3, dict(kind="mfma", replicas=3, bundle_rows=32), False))
    return out


# Sparse plans: the shapes at which tests/test_squared_hinge_gpu.py runs every row format (three partitions of
# 400 + 37 p rows, 5 non-zeros per row; their row-count edges are the business of tests/test_sparse_tables.py).
SPARSE_SIZES = (400, 437, 474)
SPARSE_MSGS = [[(0, 1.0), (1, 0.5)], [(2, -1.5)], [(0, 1.0)]]
SPARSE_FAMILIES = [("ell-lds", True, True), ("ell", False, True), ("csr", False, False)]  # id, pattern-only, use_ell


def sparse_case(prec, d, pattern_only, seed=3):
    """{p: (X scipy CSR, y +-1)}, {p: w}: 5 non-zeros per row; valued rows are N(0, 1) scaled per column by
    10**U(-3, 1), stored in the accumulator precision (what the plan keeps)."""
    import scipy.sparse as sps

    rng = np.random.RandomState(seed + d + 7 * int(pattern_only))
    scale = 10.0 ** rng.uniform(-3.0, 1.0, d)
    parts, weights = {}, {}
    for p, n in enumerate(SPARSE_SIZES):
        cols = np.stack([rng.choice(d, 5, replace=False) for _ in range(n)])
        vals = np.ones(cols.size) if pattern_only else rng.randn(cols.size) * scale[cols.ravel()]
        vals = vals.astype(np.float32 if prec.acc == torch.float32 else np.float64).astype(np.float64)
        X = sps.csr_matrix((vals, cols.ravel(), np.arange(0, cols.size + 1, 5)), shape=(n, d))
        parts[p] = (X, rng.choice([-1.0, 1.0], n))
        weights[p] = hostile_weights(rng, n)
    return parts, weights


def sparse_beta(rng, d, prec):
    beta = torch.zeros(prec.ld(d), dtype=prec.acc)
    beta[:d] = torch.from_numpy(rng.randn(d)).to(prec.acc)
    return beta, beta[:d].double().numpy()
