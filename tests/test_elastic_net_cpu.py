"""L1 / elastic-net regularisation on the CPU: the soft threshold and the update rule against hand-written values, a
lasso whose solution is held to its KKT conditions (independent of any implementation), trajectories against a NumPy
replay, sweeps over the L1 strength, flags, checkpoints and three gloo ranks."""
import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from elastic_net_cases import (ALPHAS, CASES, L1, L1S, LASSO_L1, LASSO_SUPPORT, LRS, MARGIN, TOL, lasso_problem, make,
                               replay)
from erasurehead_amd import cli
from erasurehead_amd.codes import make_scheme
from erasurehead_amd.config import RunConfig
from erasurehead_amd.data.source import ArraySource
from erasurehead_amd.engine import Trainer, evaluate
from erasurehead_amd.models import losses
from erasurehead_amd.models.losses import UpdateRule, soft_threshold
from erasurehead_amd.ops.update import combine_update, combine_update_blocks, combine_update_prox
from erasurehead_amd.parallel.dist import DistEnv
from test_multimodel_cpu import arrival_sets, run

HERE = os.path.dirname(os.path.abspath(__file__))
ARGV = ["5", "400", "20", "/tmp/eh_en_cli/", "0", "synthetic", "0", "0", "0", "0", "0", "0", "GD"]
BASE = dict(n_procs=5, n_rows=400, n_cols=20, input_dir="/tmp/x")
TINY = 5e-324  # the smallest denormal


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ---- 1. the soft threshold and the update rule against hand-written values
def test_soft_threshold_hand_values():
    x = [3.0, -3.0, 1.0, -1.0, 0.5, -0.5, 0.0, -0.0, 1.25, -1.25]
    assert same_bits(soft_threshold(x, 1.0), [2.0, -2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.25, -0.25])  # +-t -> +0.0
    assert same_bits(soft_threshold(x, 0.0), [3.0, -3.0, 1.0, -1.0, 0.5, -0.5, 0.0, 0.0, 1.25, -1.25])  # -0.0 -> +0.0
    hostile = [np.nan, np.inf, -np.inf]
    assert same_bits(soft_threshold(hostile, 1.0), hostile) and same_bits(soft_threshold(hostile, 0.0), hostile)
    assert same_bits(soft_threshold(hostile, 1e300), hostile)
    den = [TINY, -TINY, 2 * TINY, -2 * TINY, 3 * TINY]
    assert same_bits(soft_threshold(den, 0.0), den)
    assert same_bits(soft_threshold(den, TINY), [0.0, 0.0, TINY, -TINY, 2 * TINY])
    assert same_bits(soft_threshold(den, 1e-300), [0.0] * 5)
    assert same_bits(soft_threshold([1.0, -1.0], TINY), [1.0, -1.0])  # a denormal threshold rounds away
    assert same_bits(soft_threshold([[4.0, -4.0], [4.0, -4.0]], [[1.0], [3.0]]), [[3.0, -3.0], [1.0, -1.0]])  # broadcast
    assert soft_threshold(2.0, 0.5) == 1.5
    for bad in (-1.0, np.nan, [0.0, -1e-300]):
        with pytest.raises(ValueError):
            soft_threshold([1.0, 2.0], bad)


def test_update_rule_l1_field_threshold_and_apply():
    f = dataclasses.fields(UpdateRule)
    assert f[-1].name == "l1" and f[-1].default == 0.0
    assert UpdateRule("GD", 0.1, 10).l1 == 0.0 and UpdateRule("GD", 0.1, 10, 1.0, 0.25).l1 == 0.25
    up = UpdateRule("AGD", 1e-3, 400, 1.5, 0.25)  # grad_scale rescales gm only, never the threshold
    assert up.threshold(3, 2.0) == 0.5 and UpdateRule("AGD", 1e-3, 400, 1.0, 0.25).threshold(0, 2.0) == 0.5
    assert up.coeffs(3, 2.0) == UpdateRule("AGD", 1e-3, 400, 1.5).coeffs(3, 2.0) and len(up.coeffs(3, 2.0)) == 5
    assert up.block_thresholds(3, [0.5, 4.0], [0.0, 0.25]) == [0.0, 1.0]
    co = up.block_coeffs(3, [0.5, 4.0], [1e-3, 1e-1])
    assert len(co) == 5 and [len(c) for c in co[:3]] == [2, 2, 2]
    # GD, alpha = 0 (decay 1), eta = 1, n = 1: x = beta - g, then S_0.5
    beta, u = np.array([1.0, -1.0, 0.1, 2.0, np.nan]), np.zeros(5)
    UpdateRule("GD", 0.0, 1, 1.0, 0.5).apply(0, 1.0, beta, u, np.array([0.0, 0.0, 0.0, 1.5, 0.0]))
    assert same_bits(beta, [0.5, -0.5, 0.0, 0.0, np.nan]) and same_bits(u, np.zeros(5))
    # AGD round 1: theta = 2/3; alpha = 0, g = 0: y = beta/3 + 2u/3, beta' = S_t(y), u' = beta + (beta' - beta) * 1.5
    beta, u = np.array([3.0, -3.0, 0.3]), np.array([0.0, 3.0, 0.0])
    UpdateRule("AGD", 0.0, 1, 1.0, 0.5).apply(1, 1.0, beta, u, np.zeros(3))
    np.testing.assert_allclose(beta, [0.5, 0.5, 0.0], rtol=1e-15)
    np.testing.assert_allclose(u, [3.0 + (0.5 - 3.0) * 1.5, -3.0 + (0.5 + 3.0) * 1.5, 0.3 + (0.0 - 0.3) * 1.5], rtol=1e-15)
    assert beta[2] == 0.0 and not np.signbit(beta[2])
    # l1 = 0 leaves apply exactly as it was (no S_0: a -0.0 stays -0.0)
    beta, u = np.array([-0.0, 1.0]), np.zeros(2)
    UpdateRule("GD", 0.0, 1).apply(0, 1.0, beta, u, np.zeros(2))
    assert same_bits(beta, [-0.0, 1.0])


def test_cpu_operator_is_the_block_update_then_the_threshold():
    rng = np.random.RandomState(3)
    M, bl, dx = 3, 10, 7
    msgs = [torch.from_numpy(rng.randn(M * bl)) for _ in range(9)]
    coefs = list(rng.randn(9))
    decay, gm, l2, thr = [0.9, 0.8, 0.7], [0.1, 0.2, 0.3], [0.01, 0.02, 0.03], [0.0, 0.3, 100.0]
    for rule in (0, 1):
        beta0 = losses.sweep_pack(rng.randn(M, dx), bl)
        u0 = losses.sweep_pack(rng.randn(M, dx), bl)
        beta, u = torch.from_numpy(beta0.copy()), torch.from_numpy(u0.copy())
        hist, bw = torch.zeros(M * bl, dtype=torch.float64), torch.full((M * bl,), 5.0, dtype=torch.float32)
        combine_update_prox(msgs, coefs, beta, u, bl, dx, decay, gm, l2, thr, 0.4, rule, hist=hist, beta_w=bw)
        b2, u2 = torch.from_numpy(beta0.copy()), torch.from_numpy(u0.copy())
        combine_update_blocks(msgs, coefs, b2, u2, bl, dx, decay, gm, l2, 0.4, rule)
        want = soft_threshold(b2.numpy().reshape(M, bl), np.array(thr)[:, None]).ravel()
        assert same_bits(beta.numpy(), want) and same_bits(hist.numpy(), want)
        assert same_bits(bw.numpy().astype(np.float64), want.astype(np.float32).astype(np.float64))
        assert np.all(beta.numpy().reshape(M, bl)[2] == 0.0) and np.all(beta.numpy().reshape(M, bl)[:, dx:] == 0.0)
        if rule == 1:
            np.testing.assert_allclose(u.numpy(), beta0 + (want - beta0) * (1.0 / 0.4), rtol=1e-15, atol=1e-15)
        # one block is the single model
        b1, u1 = torch.from_numpy(beta0[:bl].copy()), torch.from_numpy(u0[:bl].copy())
        combine_update_prox([m[:bl] for m in msgs], coefs, b1, u1, bl, dx, decay[:1], gm[:1], l2[:1], [0.3], 0.4, rule)
        b3, u3 = torch.from_numpy(beta0[:bl].copy()), torch.from_numpy(u0[:bl].copy())
        combine_update([m[:bl] for m in msgs], coefs, b3, u3, dx, decay[0], gm[0], l2[0], 0.4, rule)
        assert same_bits(b1.numpy(), soft_threshold(b3.numpy(), 0.3))
    for bad in ([0.0, -0.1, 0.0], [0.0, float("nan"), 0.0], [0.0, 0.0]):
        with pytest.raises(ValueError):
            combine_update_prox(msgs, coefs, beta, u, bl, dx, decay, gm, l2, bad, 0.4, 0)
    with pytest.raises(ValueError):
        combine_update_prox(msgs, coefs, beta, u, bl, bl + 1, decay, gm, l2, thr, 0.4, 0)


# ---- 2. lasso: the KKT conditions of the solution
@pytest.mark.parametrize("lam", LASSO_L1)
def test_lasso_solution_satisfies_kkt(lam):
    """GD, naive, alpha = 1 / n, lr = 1 / L, 100 rounds: beta_100 is held to the optimality conditions of
    (1/n) sum (y - x beta)^2 + alpha |beta|^2 + lam |beta|_1 with this test's own gradient."""
    X, y, parts, lr = lasso_problem()
    n, d = X.shape
    alpha = 1.0 / n
    src = ArraySource([(Xp, yp) for Xp, yp in parts], (X[:40].copy(), y[:40].copy()))
    cfg = RunConfig(5, n, d, "/tmp/eh_cpu_lasso/", 0, "x", 0, 0, 0, 0, 0, 0, "GD", num_itrs=100, seed=0, verbose=False,
                    loss="least_squares", lr=lr, l1=lam)
    assert cfg.alpha_value == alpha
    tr = Trainer(cfg, DistEnv(), src, scheme=make_scheme("naive", 4, 0, n, 0, 0, rng=np.random.RandomState(7)))
    res = tr.run()
    ev = evaluate(tr, res, write=False)
    beta = res.betaset[-1]
    g = 2.0 * X.T @ (X @ beta - y)  # sum of the per-row gradients of (y - x beta)^2
    on = beta != 0
    resid_on = np.abs(g[on] / n + 2.0 * alpha * beta[on] + lam * np.sign(beta[on]))
    resid_off = np.abs(g[~on] / n) - lam
    print("lambda", lam, "KKT residual on the support", resid_on.max(initial=0.0), "off it", resid_off.max(initial=-lam))
    assert np.all(resid_on <= 1e-12) and np.all(resid_off <= 1e-12)
    assert list(np.flatnonzero(on)) == LASSO_SUPPORT[lam]
    assert ev.nnz.shape == (100,) and ev.nnz[-1] == len(LASSO_SUPPORT[lam])
    np.testing.assert_allclose(ev.l1_penalty[-1], lam * np.abs(beta).sum(), rtol=1e-15)
    if lam == 10.0:
        assert np.all(beta == 0.0) and ev.nnz[-1] == 0
    assert tr.rank_report()["prox"] is True and tr.rank_report()["l1"] == lam


# ---- 3. trajectories against the NumPy replay
@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_engine_matches_the_numpy_replay(name, rule):
    tr, res, ev = run(CASES[name], rule, l1=L1)
    cfg, src, sch, parts = make(CASES[name], rule, l1=L1)
    ref, margin = replay(sch, parts, tr.beta0, res.arrivals, rule, cfg.alpha_value, cfg.n_rows, cfg.eta(), L1)
    assert margin > MARGIN
    np.testing.assert_allclose(res.betaset, ref, **TOL)
    np.testing.assert_array_equal(res.betaset == 0, ref == 0)
    nnz = np.count_nonzero(ref, axis=1)
    np.testing.assert_array_equal(ev.nnz, nnz)
    assert 0 < nnz[-1] < 33  # the threshold zeroes some columns and keeps others
    np.testing.assert_allclose(ev.l1_penalty, L1 * np.abs(ref).sum(axis=1), **TOL)
    plain, _ = replay(sch, parts, tr.beta0, res.arrivals, rule, cfg.alpha_value, cfg.n_rows, cfg.eta(), 0.0)
    assert not np.allclose(ref, plain)  # the penalty does change the trajectory


def test_csr_source_matches_the_replay():
    import scipy.sparse as sps

    cfg, src, sch, parts = make(CASES["agc_uneven"], "AGD", l1=L1)
    sparse = ArraySource([(sps.csr_matrix(X), y) for X, y in parts], (sps.csr_matrix(src._test[0]), src._test[1]),
                         sparse=True)
    tr = Trainer(cfg, DistEnv(), sparse, scheme=sch)
    res = tr.run()
    ev = evaluate(tr, res, write=False)
    assert tr.source.is_sparse and tr.prox
    ref, margin = replay(sch, parts, tr.beta0, res.arrivals, "AGD", cfg.alpha_value, cfg.n_rows, cfg.eta(), L1)
    assert margin > MARGIN
    np.testing.assert_allclose(res.betaset[:, : tr.d_x], ref, **TOL)
    np.testing.assert_array_equal(ev.nnz, np.count_nonzero(ref, axis=1))


@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_softmax_with_l1_matches_the_replay_and_keeps_padding_zero(rule):
    from test_softmax_cpu import CASES as SM_CASES, make as sm_make

    lam = 0.01  # lr = 5: t = 0.05
    cfg, src, sch, parts = sm_make(SM_CASES["cyclic"], rule, l1=lam)
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    res = tr.run()
    ev = evaluate(tr, res, write=False)
    C, d_x, ld_x = tr.classes, tr.d_x, tr.ld_x
    assert (C, d_x, ld_x) == (3, 33, 34) and tr.prox and tr.models == 1
    full = res.betaset.reshape(-1, C, ld_x)
    assert np.all(full[:, :, d_x:] == 0.0) and np.all(tr.beta.reshape(C, ld_x)[:, d_x:].numpy() == 0.0)
    assert np.all(tr.beta_in.reshape(-1, C, ld_x)[:, :, d_x:].numpy() == 0.0)
    b0 = tr.beta0.reshape(C, ld_x)[:, :d_x].ravel()
    ref, margin = replay(sch, parts, b0, res.arrivals, rule, cfg.alpha_value, cfg.n_rows, cfg.eta(), lam,
                         kind=losses.SOFTMAX)
    assert margin > MARGIN
    np.testing.assert_allclose(full[:, :, :d_x].reshape(len(ref), -1), ref, **TOL)
    np.testing.assert_array_equal(ev.nnz, np.count_nonzero(ref, axis=1))  # over all C blocks
    assert 0 < ev.nnz[-1] < C * d_x
    np.testing.assert_allclose(ev.l1_penalty, lam * np.abs(ref).sum(axis=1), **TOL)


# ---- 4. sweeps over the L1 strength
@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_sweep_block_k_is_the_single_model_run(rule):
    tr, res, ev = run(CASES["agc_uneven"], rule, sweep_alpha=ALPHAS, sweep_lr=LRS, sweep_l1=L1S)
    assert tr.models == 3 and tr.prox and tr.sweep_l1 == L1S and ev.nnz.shape == (8, 3)
    got = losses.sweep_unpack(res.betaset, 3, tr.d_x)
    assert np.all(res.betaset.reshape(-1, 3, tr.ld_x)[:, :, tr.d_x:] == 0.0)
    for k in range(3):
        t1, r1, e1 = run(CASES["agc_uneven"], rule, alpha=ALPHAS[k], lr=LRS[k], l1=L1S[k])
        assert arrival_sets(res) == arrival_sets(r1)
        np.testing.assert_allclose(got[:, k], r1.betaset, **TOL)
        np.testing.assert_array_equal(ev.nnz[:, k], e1.nnz)
        np.testing.assert_allclose(ev.l1_penalty[:, k], e1.l1_penalty, **TOL)
        np.testing.assert_allclose(ev.testing_loss[:, k], e1.testing_loss, **TOL)
    assert len({int(x) for x in ev.nnz[-1]}) > 1  # the lambdas select different supports


def test_a_zero_lambda_block_is_the_plain_sweeps_block():
    _, plain, _ = run(CASES["cyclic"], "AGD", sweep_alpha=ALPHAS[:2], sweep_lr=LRS[:2])
    tr, res, _ = run(CASES["cyclic"], "AGD", sweep_alpha=ALPHAS[:2], sweep_lr=LRS[:2], sweep_l1=[0.0, 0.1])
    assert tr.prox and arrival_sets(res) == arrival_sets(plain)
    a, b = losses.sweep_unpack(res.betaset, 2, tr.d_x), losses.sweep_unpack(plain.betaset, 2, tr.d_x)
    np.testing.assert_array_equal(a[:, 0], b[:, 0])
    assert not np.allclose(a[:, 1], b[:, 1])


def test_all_zero_lambdas_take_todays_paths():
    t0, r0, e0 = run(CASES["agc_uneven"], "AGD")
    t1, r1, e1 = run(CASES["agc_uneven"], "AGD", l1=0.0)
    np.testing.assert_array_equal(r0.betaset, r1.betaset)
    rep = t1.rank_report()
    assert rep["prox"] is False and rep["l1"] == 0.0 and not t1.prox
    assert e1.nnz.shape == (8,) and np.all(e1.l1_penalty == 0.0)
    _, s0, _ = run(CASES["agc_uneven"], "AGD", sweep_alpha=ALPHAS, sweep_lr=LRS)
    t2, s1, e2 = run(CASES["agc_uneven"], "AGD", sweep_alpha=ALPHAS, sweep_lr=LRS, sweep_l1=[0.0, 0.0, 0.0])
    np.testing.assert_array_equal(s0.betaset, s1.betaset)
    rep = t2.rank_report()
    assert rep["prox"] is False and rep["l1"] == [0.0, 0.0, 0.0] and e2.nnz.shape == (8, 3)


def test_flags_zip_and_broadcast(capsys):
    cfg, _ = cli.parse(ARGV + ["--l1", "0.25"])
    assert cfg.l1 == 0.25 and cfg.sweep() is None and cfg.sweep_l1s() is None and cfg.sweep_l1 is None
    cfg, _ = cli.parse(ARGV)
    assert cfg.l1 == 0.0 and cfg.sweep_l1s() is None
    cfg, _ = cli.parse(ARGV + ["--l1s", "0,0.1,0.2", "--lr", "7"])  # --l1s alone: alpha and lr broadcast
    assert cfg.sweep() == [(1.0 / 400, 7.0)] * 3 and cfg.sweep_l1s() == [0.0, 0.1, 0.2]
    assert cfg.sweep_etas().shape == (3, cfg.num_itrs)
    cfg, _ = cli.parse(ARGV + ["--alphas", "1e-4,1e-3,1e-2", "--lrs", "1,2,3", "--l1s", "0.3,0.2,0.1"])
    assert cfg.sweep() == [(1e-4, 1.0), (1e-3, 2.0), (1e-2, 3.0)] and cfg.sweep_l1s() == [0.3, 0.2, 0.1]
    cfg, _ = cli.parse(ARGV + ["--alphas", "1e-4,1e-3", "--l1s", "0.5"])  # length 1: broadcast
    assert cfg.sweep() == [(1e-4, 10.0), (1e-3, 10.0)] and cfg.sweep_l1s() == [0.5, 0.5]
    cfg, _ = cli.parse(ARGV + ["--alphas", "0.25", "--l1s", "0.1,0.2"])
    assert cfg.sweep() == [(0.25, 10.0), (0.25, 10.0)] and cfg.sweep_l1s() == [0.1, 0.2]
    cfg, _ = cli.parse(ARGV + ["--lrs", "1,2", "--l1", "0.125"])  # --l1 with a sweep: every model's lambda
    assert cfg.sweep_l1s() == [0.125, 0.125]
    capsys.readouterr()


def test_flag_limits_are_value_errors():
    with pytest.raises(ValueError, match="equal lengths"):
        RunConfig(**BASE, sweep_alpha=[1, 2, 3], sweep_l1=[0.1, 0.2])
    with pytest.raises(ValueError, match="equal lengths"):
        RunConfig(**BASE, sweep_lr=[1, 2], sweep_l1=[0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="2..8"):
        RunConfig(**BASE, sweep_l1=[0.1])  # M = 1
    with pytest.raises(ValueError, match="2..8"):
        RunConfig(**BASE, sweep_l1=[0.1 * k for k in range(9)])
    RunConfig(**BASE, sweep_l1=[0.1 * k for k in range(8)])
    with pytest.raises(ValueError, match="empty"):
        RunConfig(**BASE, sweep_l1=[])
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="l1"):
            RunConfig(**BASE, l1=bad)
        with pytest.raises(ValueError, match="l1s"):
            RunConfig(**BASE, sweep_l1=[0.1, bad])
    with pytest.raises(ValueError, match="--l1"):
        RunConfig(**BASE, l1=0.1, sweep_l1=[0.1, 0.2])
    with pytest.raises(ValueError, match="softmax"):
        RunConfig(**BASE, loss="softmax", sweep_l1=[0.1, 0.2])
    assert RunConfig(**BASE, loss="softmax", l1=0.1).sweep() is None  # softmax with --l1: a single model
    RunConfig(**BASE, sweep_l1=[0.1, 0.2], lr_schedule=[1.0] * 100)  # like --alphas, --l1s keeps an explicit schedule


def test_evaluation_lines_and_files(tmp_path):
    cfg, src, sch, parts = make(CASES["naive"], "GD", sweep_alpha=ALPHAS, sweep_lr=LRS, sweep_l1=L1S)
    cfg.input_dir, cfg.verbose = str(tmp_path) + "/", True
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    lines = []
    res = tr.run(log=lines.append)
    ev = evaluate(tr, res, log=lines.append)
    heads = [ln for ln in lines if ln.startswith(">> Model ")]
    assert heads == [">> Model %d: alpha = %g, lr = %g, l1 = %g" % (k, ALPHAS[k], LRS[k], L1S[k]) for k in range(3)]
    assert [ln for ln in lines if ln.startswith(">> L1: ")] == \
        [">> L1: l1 = %g, nnz = %d of %d" % (L1S[k], ev.nnz[-1, k], 33) for k in range(3)]
    single = dict(tr.scheme.output_names(cfg.fix_quirks))
    single["nnz"] = single["auc"].replace("auc", "nnz")
    assert set(ev.files) == {f"sweep{k}_{key}" for k in range(3) for key in single}
    for k in range(3):
        path = ev.files[f"sweep{k}_nnz"]
        assert os.path.basename(path) == f"sweep{k}_{single['nnz']}"
        np.testing.assert_array_equal(np.loadtxt(path), ev.nnz[:, k])
    assert tr.rank_report()["l1"] == L1S and tr.rank_report()["prox"] is True
    # a single squared-hinge model: its prefix; one L1 line before ">>> Done"
    cfg, src, sch, parts = make(CASES["naive"], "GD", loss="squared_hinge", lr=0.1, l1=0.5)
    cfg.input_dir, cfg.verbose = str(tmp_path) + "/", True
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    lines = []
    ev = evaluate(tr, tr.run(log=lines.append), log=lines.append)
    assert lines[-2:] == [">> L1: l1 = 0.5, nnz = %d of 33" % ev.nnz[-1], ">>> Done"]
    assert os.path.basename(ev.files["nnz"]) == "sqhinge_" + single["nnz"]
    # without a lambda: the lines and files of before
    cfg, src, sch, parts = make(CASES["naive"], "GD")
    cfg.input_dir, cfg.verbose = str(tmp_path) + "/", True
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    lines = []
    ev = evaluate(tr, tr.run(log=lines.append), log=lines.append)
    assert not any("L1" in ln or "l1" in ln for ln in lines) and "nnz" not in ev.files


def test_softmax_evaluation_writes_nnz_under_its_prefix(tmp_path):
    from test_softmax_cpu import CASES as SM_CASES, make as sm_make

    cfg, src, sch, parts = sm_make(SM_CASES["naive"], "GD", l1=0.01)
    cfg.input_dir, cfg.verbose = str(tmp_path) + "/", True
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    lines = []
    ev = evaluate(tr, tr.run(log=lines.append), log=lines.append)
    assert lines[-2] == ">> L1: l1 = 0.01, nnz = %d of 99" % ev.nnz[-1]
    assert os.path.basename(ev.files["nnz"]) == "softmax_" + tr.scheme.output_names()["auc"].replace("auc", "nnz")


def test_cli_runs_an_l1_path_on_synthetic_data(capsys, tmp_path):
    argv = ["5", "160", "6", str(tmp_path) + "/", "0", "x", "0", "0", "0", "0", "0", "0", "GD"]
    rc = cli.main(argv + ["--data", "synthetic", "--device", "cpu", "--num-itrs", "3", "--lr", "1", "--seed", "0",
                          "--l1s", "0,0.05,100"])
    assert rc == 0
    lines = capsys.readouterr().out.splitlines()
    assert [ln.split(",")[-1] for ln in lines if ln.startswith(">> Model ")] == [" l1 = 0", " l1 = 0.05", " l1 = 100"]
    nnz = [ln for ln in lines if ln.startswith(">> L1: ")]
    assert len(nnz) == 3 and nnz[0].endswith("nnz = 6 of 6") and nnz[2] == ">> L1: l1 = 100, nnz = 0 of 6"
    for k in range(3):
        assert os.path.exists(os.path.join(str(tmp_path), "results", f"sweep{k}_naive_acc_nnz.dat"))


def test_checkpoint_round_trip_and_refused_resume(tmp_path):
    ck = str(tmp_path / "ck.pt")
    _, full, _ = run(CASES["cyclic"], "AGD", l1=L1)
    run(CASES["cyclic"], "AGD", l1=L1, rounds=4, checkpoint_every=4, checkpoint_path=ck)
    st = torch.load(ck, weights_only=False)
    assert st["l1"] == L1
    _, resumed, _ = run(CASES["cyclic"], "AGD", l1=L1, resume=ck)
    np.testing.assert_allclose(resumed.betaset, full.betaset, **TOL)
    with pytest.raises(ValueError, match="l1"):
        run(CASES["cyclic"], "AGD", l1=2 * L1, resume=ck)
    with pytest.raises(ValueError, match="l1"):
        run(CASES["cyclic"], "AGD", resume=ck)
    # a checkpoint without the key means 0
    del st["l1"]
    old = str(tmp_path / "old.pt")
    torch.save(st, old)
    with pytest.raises(ValueError, match="l1 = 0"):
        run(CASES["cyclic"], "AGD", l1=L1, resume=old)
    run(CASES["cyclic"], "AGD", resume=old)
    # sweeps store the list
    sw = dict(sweep_alpha=ALPHAS, sweep_lr=LRS)
    cks = str(tmp_path / "sweep.pt")
    _, full, _ = run(CASES["cyclic"], "GD", sweep_l1=L1S, **sw)
    run(CASES["cyclic"], "GD", sweep_l1=L1S, rounds=4, checkpoint_every=4, checkpoint_path=cks, **sw)
    assert torch.load(cks, weights_only=False)["sweep_l1"] == L1S
    _, resumed, _ = run(CASES["cyclic"], "GD", sweep_l1=L1S, resume=cks, **sw)
    np.testing.assert_allclose(resumed.betaset, full.betaset, **TOL)
    with pytest.raises(ValueError, match="sweep_l1"):
        run(CASES["cyclic"], "GD", sweep_l1=[0.005, 0.02, 0.03], resume=cks, **sw)
    with pytest.raises(ValueError, match="sweep_l1"):
        run(CASES["cyclic"], "GD", resume=cks, **sw)


# ---- 5. three gloo ranks
def test_three_gloo_ranks_equal_the_single_process_run(tmp_path):
    out = str(tmp_path / "elastic_gloo.npz")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]),
               EH_ELASTIC_OUT=out, EH_ELASTIC_DEVICE="cpu", EH_ELASTIC_CASE="naive")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr",
           "127.0.0.1", f"--master-port={port}", os.path.join(HERE, "mp_elastic_net_run.py")]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    z = np.load(out, allow_pickle=True)
    assert bool(z["prox"])
    # the naive scheme waits for every worker, so the gradient (and with it the run) does not depend on who came first
    tr, res, _ = run(CASES["naive"], "AGD", l1=L1)
    np.testing.assert_array_equal(z["beta0"], tr.beta0)
    np.testing.assert_allclose(z["betaset"], res.betaset, **TOL)
    np.testing.assert_array_equal(z["betaset"] == 0, res.betaset == 0)
    check_against_replay(z, "naive")


def check_against_replay(z, name):
    """The saved run of tests/mp_elastic_net_run.py against the replay of its logged arrivals."""
    cfg, src, sch, parts = make(CASES[name], "AGD", l1=L1)
    arrivals = [[tuple(a) for a in rnd] for rnd in z["arrivals"]]
    ref, margin = replay(sch, parts, z["beta0"], arrivals, "AGD", cfg.alpha_value, cfg.n_rows, cfg.eta(), L1)
    assert margin > MARGIN
    got = np.asarray(z["betaset"])
    np.testing.assert_allclose(got[:, :33], ref, **TOL)
    assert np.all(got[:, 33:] == 0.0)
