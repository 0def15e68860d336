"""What the cross-validation tests share (tests/test_cv_cpu.py, test_cv_gpu.py, mp_cv_run.py): the scheme cases and
shapes of tests/test_multimodel_cpu.py run with ``cv = K``, the same data with one fold's rows deleted (the
single-model run fold model k must equal), and the NumPy replay of a saved multi-rank run."""
import dataclasses

import numpy as np

from erasurehead_amd.data.source import ArraySource
from erasurehead_amd.ops.cv import CvGradPlan
from oracle import replay
from test_multimodel_cpu import CASES, TOL, make as make_binary  # noqa: F401 (re-exported)

ALPHA, LR = 3e-3, 0.7  # explicit: the default alpha is 1 / n_rows, and the two runs compared differ in n_rows
MP_CASE, MP_RULE, MP_K = "agc_uneven", "AGD", 3  # the run of tests/mp_cv_run.py


def fold_of(n: int, K: int) -> np.ndarray:
    """The fold of every row of a partition of n rows: its position in the partition mod K."""
    return np.arange(n) % K


def held_out_rows(parts, K: int, k: int) -> int:
    return int(sum((fold_of(len(y), K) == k).sum() for _, y in parts))


def without_fold(parts, K: int, k: int):
    """The partitions with the rows of fold k deleted."""
    return [(X[fold_of(len(y), K) != k], y[fold_of(len(y), K) != k]) for X, y in parts]


def make(case, rule="GD", K=3, **kw):
    """(cfg, source, scheme, host partitions) of a --cv K run: test_multimodel_cpu.make's data and seeds."""
    kw.setdefault("alpha", ALPHA)
    kw.setdefault("lr", LR)
    return make_binary(case, rule, cv=K, **kw)


def make_without_fold(case, rule, K, k, **kw):
    """The single-model run fold model k must equal: the same data, seeds, alpha and lr, every partition without its
    rows of fold k, and n_rows the rows that are left."""
    kw.setdefault("alpha", ALPHA)
    kw.setdefault("lr", LR)
    cfg, src, sch, parts = make_binary(case, rule, **kw)
    left = without_fold(parts, K, k)
    n_k = held_out_rows(parts, K, k)
    assert n_k == len(parts) * CvGradPlan.fold_rows(len(parts[0][1]), K)[k]
    cfg = dataclasses.replace(cfg, n_rows=cfg.n_rows - n_k)
    return cfg, ArraySource(left, src._test), sch, left


def check_against_replay(z):
    """The saved run of tests/mp_cv_run.py against tests/oracle.py's replay, once per fold model: the single-model
    replay over the partitions without fold k, with n - n_k rows."""
    K = MP_K
    cfg, src, sch, parts = make(CASES[MP_CASE], MP_RULE, K)
    d_x, ld_x = 33, 34
    arrivals = [[tuple(a) for a in rnd] for rnd in z["arrivals"]]
    got = np.asarray(z["betaset"]).reshape(-1, K, ld_x)
    assert np.all(got[:, :, d_x:] == 0.0)
    beta0 = np.asarray(z["beta0"]).reshape(K, ld_x)[:, :d_x]
    for k in range(K):
        ref = replay(sch, without_fold(parts, K, k), beta0[k], arrivals, MP_RULE, cfg.alpha_value,
                     cfg.n_rows - held_out_rows(parts, K, k), cfg.eta())
        np.testing.assert_allclose(got[:, k, :d_x], ref, **TOL)
