"""Case tables and helpers of tests/test_elastic_net_cpu.py and tests/test_elastic_net_gpu.py (L1 / elastic net).

The engine cases are the seeded schemes of tests/test_multimodel_cpu.py::make (40 rows per partition, d = 33,
8 rounds, labels in {-1, +1}, lr = 1; beta_0 is N(0, 1) or, for the cyclic code, zero).  With L1 = 0.02 every
case and rule ends with a support that is neither empty nor full (1 to 30 of the 33 columns).
"""
import numpy as np

from erasurehead_amd.codes.schemes import Arrival
from erasurehead_amd.models.losses import LOGISTIC, UpdateRule, soft_threshold, worker_grad
from test_multimodel_cpu import CASES, TOL, make  # noqa: F401  (re-exported to the two test modules)

L1 = 0.02  # the single-model cases
ALPHAS = [1e-3, 1e-2, 1e-1]  # the sweep of tests/test_multimodel_cpu.py ...
LRS = [1.0, 1.0, 3.0]
L1S = [0.005, 0.02, 0.01]  # ... with one lambda per model
MARGIN = 1e-9  # no pre-threshold magnitude within this relative distance of its threshold (GPU-against-CPU supports)


def replay(scheme, parts, beta0, arrivals_log, rule, alpha, n_samples, eta, l1, kind=LOGISTIC):
    """tests/oracle.py::replay with an L1 strength: decode the logged arrivals, NumPy worker gradients, then
    ``UpdateRule.apply``.  Returns (betaset [R, d], margin): margin is the smallest | |x| - t | / t over every
    round and column, x the pre-threshold update (the same state through an l1 = 0 rule) and t the threshold."""
    rule = "AGD" if scheme.fixed_agd else rule
    up = UpdateRule(rule, alpha, n_samples, scheme.grad_scale(), l1)
    plain = UpdateRule(rule, alpha, n_samples, scheme.grad_scale())
    beta = np.array(beta0, dtype=np.float64)
    u = np.zeros_like(beta)
    out, margin = [], np.inf
    for i, arr in enumerate(arrivals_log):
        used = scheme.decode([Arrival(w, p, t) for (w, p, t) in arr])
        g = np.zeros_like(beta)
        for (w, part), c in used.items():
            m = [x for x in scheme.messages if x.worker == w and x.part == part][0]
            g += c * sum(worker_grad(kind, parts[p][0], parts[p][1], beta, coef) for p, coef in m.segments)
        x, ux = beta.copy(), u.copy()
        plain.apply(i, eta[i], x, ux, g)
        t = up.threshold(i, eta[i])
        if t > 0:
            margin = min(margin, float(np.min(np.abs(np.abs(x) - t))) / t)
        up.apply(i, eta[i], beta, u, g)
        np.testing.assert_array_equal(beta, soft_threshold(x, t) if t > 0 else x)
        out.append(beta.copy())
    return np.array(out), margin


def lasso_problem():
    """The issue's lasso: n = 240, d = 12, RandomState(0), support {1, 4, 7} = (2, -1.5, 0.75), noise 0.1; four
    partitions of 60 rows for the naive scheme with four workers.  Returns (X, y, parts, lr = 1 / L)."""
    rng = np.random.RandomState(0)
    n, d = 240, 12
    X = rng.randn(n, d)
    bt = np.zeros(d)
    bt[[1, 4, 7]] = [2.0, -1.5, 0.75]
    y = X @ bt + 0.1 * rng.randn(n)
    alpha = 1.0 / n
    L = 2.0 * np.linalg.eigvalsh(X.T @ X / n)[-1] + 2.0 * alpha
    parts = [(X[k * 60: (k + 1) * 60].copy(), y[k * 60: (k + 1) * 60].copy()) for k in range(4)]
    return X, y, parts, 1.0 / L


LASSO_L1 = [0.05, 0.5, 10.0]
LASSO_SUPPORT = {0.05: [1, 4, 7], 0.5: [1, 4, 7], 10.0: []}

# ---- the update kernel (GPU): shapes of the issue.  (d, ld): ld > d where an fp32 / fp64 vector pads the row.
KERNEL_SHAPES = [(1, 4), (37, 40), (255, 256), (256, 256), (257, 260), (1000, 1000)]
KERNEL_NMSG = [1, 8, 9, 17]  # one, a full batch of eight, one past it, two batches and one
KERNEL_BLOCKS = [2, 3, 8]
