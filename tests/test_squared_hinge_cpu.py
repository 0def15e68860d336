"""Squared-hinge (L2-SVM) loss on the CPU: library math against this file's own fp64 oracle and central
finite differences, the engine against the NumPy replay, evaluation, result files, CLI, sparse plan."""
import os

import numpy as np
import pytest
import scipy.sparse as sps
import torch

from erasurehead_amd import cli
from erasurehead_amd.engine import Trainer, evaluate
from erasurehead_amd.models import losses
from erasurehead_amd.models.losses import roc_auc
from erasurehead_amd.ops import SparseGradPlan, get_precision
from erasurehead_amd.parallel.dist import DistEnv
from oracle import replay
from test_engine_cpu import CASES, make


# ---- the test's own oracle (issue: z = X beta, m = max(0, 1 - y z), g = -2 X^T(coef y m), loss = mean m^2)
def _margin(X, y, beta):
    return np.maximum(0.0, 1.0 - y * np.asarray(X.dot(beta)).ravel())


def _grad(X, y, beta, coef=1.0):
    return np.asarray(X.T.dot(-2.0 * coef * y * _margin(X, y, beta))).ravel()


def _loss_sum(X, y, beta):
    return float(np.sum(_margin(X, y, beta) ** 2))


def _active_share(X, y, beta):
    return float(np.mean(y * np.asarray(X.dot(beta)).ravel() < 1.0))


def _dense(seed, n=300, d=37):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, d) * 0.3
    y = rng.choice([-1.0, 1.0], n)
    beta = rng.randn(d) * 10.0 / np.sqrt(d)  # z has std ~3: both sides of the kink
    assert 0.3 < _active_share(X, y, beta) < 0.9
    return X, y, beta


def test_names_and_kinds():
    assert losses.SQUARED_HINGE == 2
    assert losses.LOSS_NAMES == {"logistic": 0, "least_squares": 1, "squared_hinge": 2}
    assert losses.is_classification(losses.LOGISTIC) and losses.is_classification(losses.SQUARED_HINGE)
    assert not losses.is_classification(losses.LEAST_SQUARES)


@pytest.mark.parametrize("coef", [None, 1.0, -0.7])
def test_library_gradient_is_the_oracle(coef):
    X, y, beta = _dense(1)
    got = losses.squared_hinge_grad(X, y, beta, coef)
    np.testing.assert_allclose(got, _grad(X, y, beta, 1.0 if coef is None else coef), rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(losses.worker_grad(losses.SQUARED_HINGE, X, y, beta, coef), got)
    Xs = sps.csr_matrix(X)
    np.testing.assert_allclose(losses.squared_hinge_grad(Xs, y, beta, coef), got, rtol=1e-12, atol=1e-12)


def test_worker_grad_is_three_way():
    X, y, beta = _dense(2)
    np.testing.assert_array_equal(losses.worker_grad(losses.LOGISTIC, X, y, beta, 0.5),
                                  losses.logistic_grad(X, y, beta, 0.5))
    np.testing.assert_array_equal(losses.worker_grad(losses.LEAST_SQUARES, X, y, beta, 0.5),
                                  losses.least_squares_grad(X, y, beta, 0.5))
    g = losses.worker_grad(losses.SQUARED_HINGE, X, y, beta, 0.5)
    assert not np.allclose(g, losses.least_squares_grad(X, y, beta, 0.5))
    with pytest.raises(ValueError):
        losses.worker_grad(7, X, y, beta)


def test_gradient_is_the_derivative_of_the_loss():
    """Central finite differences of sum m^2 (h = 1e-6) against the library's and the oracle's gradient."""
    X, y, beta = _dense(3)
    h = 1e-6
    fd = np.empty_like(beta)
    for j in range(beta.size):
        e = np.zeros_like(beta)
        e[j] = h
        fd[j] = (_loss_sum(X, y, beta + e) - _loss_sum(X, y, beta - e)) / (2 * h)
    for g in (losses.squared_hinge_grad(X, y, beta), _grad(X, y, beta)):
        assert np.max(np.abs(g - fd)) / np.max(np.abs(fd)) < 1e-5


def test_library_loss_is_the_oracle():
    X, y, beta = _dense(4)
    p = X @ beta
    assert losses.squared_hinge_loss(y, p) == pytest.approx(_loss_sum(X, y, beta) / len(y), rel=1e-14)
    assert losses.squared_hinge_loss(y, p, 1) == pytest.approx(_loss_sum(X, y, beta), rel=1e-14)
    assert losses.squared_hinge_loss(np.array([1.0, -1.0]), np.array([2.0, -1.0])) == 0.0  # past the margin


ENGINE_CASES = [CASES[0], CASES[1], CASES[4], CASES[6]]  # naive, cyclic s=2, AGC (7, s=2, k=4), partial replication


@pytest.mark.parametrize("case", ENGINE_CASES)
@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_engine_matches_numpy_replay(case, rule):
    cfg, src, sch, parts = make(case, rule, loss="squared_hinge", lr=1.0)  # (the default 10 exceeds 1/L ~ 3.7)
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    assert tr.loss == losses.SQUARED_HINGE
    res = tr.run()
    ref = replay(sch, parts, tr.beta0, res.arrivals, rule, cfg.alpha_value, cfg.n_rows, cfg.eta(),
                 losses.SQUARED_HINGE)
    np.testing.assert_allclose(res.betaset, ref, rtol=1e-10, atol=1e-12)


def test_training_loss_falls_every_round():
    cfg, src, sch, parts = make(CASES[0], "GD", loss="squared_hinge", lr=1.0)
    res = Trainer(cfg, DistEnv(), src, scheme=sch).run()
    X = np.vstack([p[0] for p in parts])
    y = np.concatenate([p[1] for p in parts])
    ls = [_loss_sum(X, y, b) / len(y) for b in res.betaset]
    assert len(ls) == 6 and all(b < a for a, b in zip(ls, ls[1:])), ls


def test_evaluate_scores_prints_and_writes_next_to_logistic(tmp_path):
    out = {}
    for loss in ("logistic", "squared_hinge"):
        cfg, src, sch, parts = make(CASES[0], "GD", loss=loss, lr=1.0)
        cfg.input_dir = str(tmp_path) + "/"
        tr = Trainer(cfg, DistEnv(), src, scheme=sch)
        res = tr.run()
        cfg.verbose = True
        lines = []
        ev = evaluate(tr, res, log=lines.append, write=True)
        out[loss] = (ev, lines, res, src, parts, cfg)
        if loss == "logistic":
            kept = {p: open(p, "rb").read() for p in ev.files.values()}
    ev, lines, res, src, parts, cfg = out["squared_hinge"]
    Xtr = np.vstack([parts[p][0] for p in range(cfg.n_workers - 1)])  # (partition W is skipped, as for logistic)
    ytr = np.concatenate([parts[p][1] for p in range(cfg.n_workers)])[: Xtr.shape[0]]
    Xte, yte = src._test
    for i, b in enumerate(res.betaset):
        assert ev.training_loss[i] == pytest.approx(_loss_sum(Xtr, ytr, b) / len(ytr), rel=1e-10)
        assert ev.testing_loss[i] == pytest.approx(_loss_sum(Xte, yte, b) / len(yte), rel=1e-10)
        assert ev.auc[i] == pytest.approx(roc_auc(yte, Xte @ b), rel=1e-12)
    it = [l for l in lines if l.startswith("Iteration ")]
    assert len(it) == len(res.betaset) and all("AUC = " in l for l in it)  # the classification console line
    names = {k: os.path.basename(v) for k, v in ev.files.items()}
    logistic_names = {k: os.path.basename(v) for k, v in out["logistic"][0].files.items()}
    assert names == {k: "sqhinge_" + v for k, v in logistic_names.items()}
    assert all(os.path.exists(p) for p in ev.files.values())
    for p, body in kept.items():  # the logistic run's files are still what that run wrote
        assert open(p, "rb").read() == body


def test_cli_accepts_squared_hinge_and_rejects_unknown_names(capsys):
    argv = ["5", "40", "6", "/tmp/eh_cli_sqh/", "0", "x", "0", "0", "0", "0", "0", "0", "GD"]
    cfg, _ = cli.parse(argv + ["--loss", "squared_hinge"])
    assert cfg.loss == "squared_hinge"
    with pytest.raises(SystemExit):
        cli.parse(argv + ["--loss", "hinge"])
    capsys.readouterr()


@pytest.mark.parametrize("pattern_only", [True, False])
def test_sparse_plan_on_cpu_tensors(pattern_only):
    prec = get_precision("fp64")
    rng = np.random.RandomState(3)
    d = 700
    parts = {}
    for p in range(3):
        n = 400 + 37 * p
        nnz = rng.randint(5, 9, n)
        ptr = np.concatenate([[0], np.cumsum(nnz)])
        cols = np.concatenate([np.sort(rng.choice(d, k, replace=False)) for k in nnz])
        vals = np.ones(cols.size) if pattern_only else rng.randn(cols.size)
        parts[p] = (sps.csr_matrix((vals, cols, ptr), shape=(n, d)), rng.choice([-1.0, 1.0], n))
    msgs = [[(0, 1.0), (1, 0.5)], [(2, -1.5)], [(0, 1.0)]]
    plan = SparseGradPlan(msgs, parts, prec, losses.SQUARED_HINGE, d, device="cpu")
    beta = torch.zeros(prec.ld(d), dtype=torch.float64)
    beta[:d] = torch.from_numpy(rng.randn(d) * 1.0)
    bh = beta[:d].numpy()
    for X, y in parts.values():
        assert 0.3 < _active_share(X, y, bh) < 0.9
    G = plan.run(beta, torch.zeros((len(msgs), prec.ld(d)), dtype=torch.float64))
    for s, m in enumerate(msgs):
        ref = sum(_grad(parts[p][0], parts[p][1], bh, c) for p, c in m)
        assert np.max(np.abs(G[s, :d].numpy() - ref)) / np.max(np.abs(ref)) < 1e-11
