"""K-fold cross-validation runs (--cv K) on the CPU: the fold counts, the plan against the library twin, the contract
(fold model k of a --cv K run is the single-model run on the data without the rows of fold k), the held-out scores
against a NumPy recomputation, console lines and result files, every rejection (before data is loaded), checkpoints,
three gloo ranks, and a run without the flag."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from cv_cases import (ALPHA, CASES, LR, TOL, check_against_replay, fold_of, held_out_rows, make, make_binary,
                      make_without_fold, without_fold)
from erasurehead_amd import cli
from erasurehead_amd.config import RunConfig
from erasurehead_amd.data.source import ArraySource
from erasurehead_amd.engine import Trainer, evaluate
from erasurehead_amd.engine.model import ModelSpec
from erasurehead_amd.models import losses
from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.cv import CvGradPlan
from erasurehead_amd.parallel.dist import DistEnv

HERE = os.path.dirname(os.path.abspath(__file__))
LOSS_OF = {"logistic": losses.LOGISTIC, "least_squares": losses.LEAST_SQUARES, "squared_hinge": losses.SQUARED_HINGE}


def run(case, rule, K, **kw):
    cfg, src, sch, parts = make(case, rule, K, **kw)
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    return tr, tr.run(), parts


def run_without_fold(case, rule, K, k, **kw):
    cfg, src, sch, parts = make_without_fold(case, rule, K, k, **kw)
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    return tr, tr.run()


def arrival_sets(res):
    return [[(w, p) for (w, p, _t) in r] for r in res.arrivals]


# ---- 1. the fold counts and the library twins
@pytest.mark.parametrize("K", range(2, 9))
@pytest.mark.parametrize("n_p", [0, 1, 2, 3, 5, 7, 8, 9, 40, 64, 67, 150])  # n_p < K, n_p = 0, no multiple of K
def test_fold_rows_is_the_brute_force_count(n_p, K):
    want = [sum(1 for i in range(n_p) if i % K == k) for k in range(K)]
    assert CvGradPlan.fold_rows(n_p, K) == want and sum(want) == n_p
    mask = losses.cv_fold_mask(n_p, K)
    assert mask.shape == (n_p, K) and mask.dtype == bool
    assert [int((~mask[:, k]).sum()) for k in range(K)] == want
    if n_p:
        assert np.all((~mask).sum(axis=1) == 1)  # every row is held out of exactly one model


def _grad(kind, X, y, b, coef=1.0):
    """The test's own scalar-loss gradient, from the loss's definition."""
    z = X @ b
    if kind == losses.LOGISTIC:
        r = -y / (1.0 + np.exp(y * z))
    elif kind == losses.LEAST_SQUARES:
        r = -2.0 * (y - z)
    else:
        r = -2.0 * y * np.maximum(0.0, 1.0 - y * z)
    return coef * (r @ X)


@pytest.mark.parametrize("kind", sorted(LOSS_OF.values()))
@pytest.mark.parametrize("K", [2, 3, 5, 8])
def test_library_gradient_leaves_out_the_fold(kind, K):
    rng = np.random.RandomState(K)
    X, y, B = rng.randn(67, 9) * 0.3, rng.choice([-1.0, 1.0], 67), rng.randn(K, 9)
    got = losses.cv_grad(kind, X, y, B, -0.7)
    for k in range(K):
        keep = fold_of(67, K) != k
        np.testing.assert_allclose(got[k], _grad(kind, X[keep], y[keep], B[k], -0.7), rtol=1e-12, atol=1e-13)
    with pytest.raises(ValueError, match="cross-validation"):
        losses.cv_grad(losses.SOFTMAX, X, y, B)


@pytest.mark.parametrize("kind", sorted(LOSS_OF.values()))
def test_cpu_plan_is_the_library_twin(kind):
    prec = get_precision("fp64")
    rng = np.random.RandomState(8)
    K, d = 5, 37
    ld = prec.ld(d)
    raw, parts = {}, {}
    for p, n in enumerate([57, 64, 1, 0, 3]):  # an empty partition, one with fewer rows than folds
        Xp_, yp = rng.randn(n, d) * 0.3, rng.choice([-1.0, 1.0], n)
        raw[p] = (Xp_, yp)
        Xp = np.zeros((n, ld))
        Xp[:, :d] = Xp_
        parts[p] = (torch.from_numpy(Xp), torch.from_numpy(yp))
    Bm = rng.randn(K, d) * 6.0 / np.sqrt(d)
    msgs = [[(0, 1.0), (1, -0.7)], [(2, 2.5), (3, 1.0)], [(1, 1.0), (0, 0.3), (4, 1.0)]]
    plan = CvGradPlan(msgs, parts, prec, kind, K, d)
    assert (plan.nslots, plan.ld, plan.d, plan.folds) == (3, K * ld, K * ld, K)
    G = plan.run(torch.from_numpy(losses.sweep_pack(Bm, ld)), plan.out_buffer()[0])
    for s, m in enumerate(msgs):
        ref = sum(losses.cv_grad(kind, raw[p][0], raw[p][1], Bm, c) for p, c in m)
        got = G[s].numpy().reshape(K, ld)
        assert np.max(np.abs(got[:, :d] - ref)) / np.max(np.abs(ref)) < 1e-12
        assert np.all(got[:, d:] == 0.0)
    # a non-finite held-out row does not enter the CPU plan: the rows are left out, not multiplied by 0
    parts[0][0][0::K] = float("nan")
    G2 = plan.run(torch.from_numpy(losses.sweep_pack(Bm, ld)), plan.out_buffer()[0]).numpy().reshape(3, K, ld)
    assert np.all(np.isfinite(G2[:, 0])) and not np.all(np.isfinite(G2[:, 1]))
    wide = {0: (torch.zeros((4, 2050), dtype=torch.float64), torch.ones(4, dtype=torch.float64))}
    CvGradPlan([[(0, 1.0)]], wide, prec, kind, 2, 2049)  # CPU tensors run at any width


def test_plan_limits():
    prec = get_precision("fp64")
    part = {0: (torch.zeros((4, 6), dtype=torch.float64), torch.ones(4, dtype=torch.float64))}
    for bad in (1, 9):
        with pytest.raises(ValueError, match="--cv.*2..8"):
            CvGradPlan([[(0, 1.0)]], part, prec, losses.LOGISTIC, bad, 6)
    for kind, word in ((losses.SOFTMAX, "softmax"), (losses.LOGISTIC_W, "weights"), (losses.SQUARED_HINGE_W, "weights")):
        with pytest.raises(ValueError, match="--cv.*" + word):
            CvGradPlan([[(0, 1.0)]], part, prec, kind, 3, 6)
    with pytest.raises(ValueError, match="--cv.*bf16"):
        CvGradPlan.check_supported(get_precision("bf16"), losses.LOGISTIC, 3)
    with pytest.raises(ValueError, match="--cv.*sparse"):
        CvGradPlan.check_supported(prec, losses.LOGISTIC, 3, sparse=True)
    with pytest.raises(ValueError, match="--cv.*1024"):
        CvGradPlan.check_supported(prec, losses.LOGISTIC, 3, ld_x=1026, gpu=True)
    CvGradPlan.check_supported(prec, losses.LOGISTIC, 3, ld_x=1026, gpu=False)


# ---- 2. the feature is what it claims: fold model k is the single-model run without the rows of fold k
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_fold_model_k_is_the_run_without_fold_k(name, rule, K):
    tr, res, parts = run(CASES[name], rule, K)
    assert isinstance(tr.plan, CvGradPlan) and tr.cv == K and tr.models == K and tr.classes == 1
    assert res.betaset.shape == (8, K * tr.ld_x)
    got = losses.sweep_unpack(res.betaset, K, tr.d_x)
    n = tr.cfg.n_rows
    assert list(tr.model.fold_rows) == [held_out_rows(parts, K, k) for k in range(K)]
    for k in range(K):
        t1, r1 = run_without_fold(CASES[name], rule, K, k)
        assert not isinstance(t1.plan, CvGradPlan) and t1.cfg.n_rows == n - tr.model.fold_rows[k]
        np.testing.assert_array_equal(tr.beta0.reshape(K, tr.ld_x)[k, : tr.d_x], t1.beta0)  # the same beta_0
        np.testing.assert_allclose(got[:, k], r1.betaset, **TOL)
        assert arrival_sets(res) == arrival_sets(r1)
    assert not np.allclose(got[:, 0], got[:, 1])  # the fold models do differ
    assert np.all(res.betaset.reshape(-1, K, tr.ld_x)[:, :, tr.d_x:] == 0.0)
    rep = tr.rank_report()
    assert rep["cv"] == K and rep["fold_rows"] == list(tr.model.fold_rows)


@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_the_contract_holds_with_l1(rule):
    K = 3
    tr, res, parts = run(CASES["agc_uneven"], rule, K, l1=0.02)
    assert tr.prox
    got = losses.sweep_unpack(res.betaset, K, tr.d_x)
    for k in range(K):
        _, r1 = run_without_fold(CASES["agc_uneven"], rule, K, k, l1=0.02)
        np.testing.assert_allclose(got[:, k], r1.betaset, **TOL)
        np.testing.assert_array_equal(got[:, k] == 0.0, r1.betaset == 0.0)
    assert 0 < np.count_nonzero(got[-1] == 0.0) < got[-1].size  # the threshold bites


@pytest.mark.parametrize("loss", ["least_squares", "squared_hinge"])
def test_the_contract_holds_for_the_other_losses(loss):
    K = 3
    tr, res, parts = run(CASES["cyclic"], "AGD", K, loss=loss, lr=0.1)
    assert tr.loss == LOSS_OF[loss]
    got = losses.sweep_unpack(res.betaset, K, tr.d_x)
    for k in range(K):
        _, r1 = run_without_fold(CASES["cyclic"], "AGD", K, k, loss=loss, lr=0.1)
        np.testing.assert_allclose(got[:, k], r1.betaset, **TOL)


def test_update_schedule_scales_gm_only():
    cfg, src, sch, parts = make(CASES["naive"], "AGD", 3, l1=0.01)
    spec = ModelSpec.resolve(cfg, sch, False, False, get_precision("fp64"), False)
    assert (spec.kind, spec.models, spec.blocks, spec.cv, spec.d, spec.ld) == ("cv", 3, 3, 3, 3 * 34, 3 * 34)
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    sched = tr._update_schedule()
    n, nk = cfg.n_rows, np.array(spec.fold_rows, dtype=np.float64)
    assert list(spec.fold_rows) == [4 * 14, 4 * 13, 4 * 13] and n == 160
    for i in range(cfg.num_itrs):
        decay, gm, l2, theta, code = tr.update.coeffs(i, float(cfg.eta()[i]))
        np.testing.assert_array_equal(sched.decay[i], [decay] * 3)
        np.testing.assert_array_equal(sched.l2[i], [l2] * 3)
        np.testing.assert_array_equal(sched.thr[i], [tr.update.threshold(i, float(cfg.eta()[i]))] * 3)
        np.testing.assert_allclose(sched.gm[i], gm * n / (n - nk), rtol=1e-15)
    assert (sched.block_ld, sched.block_d) == (34, 33)


# ---- 3. evaluation: the held-out scores against a NumPy recomputation from betaset
def _loss_rows(kind, X, y, b):
    z = X @ b
    if kind == losses.LOGISTIC:
        return np.logaddexp(0.0, -y * z)
    if kind == losses.LEAST_SQUARES:
        return (y - z) ** 2
    return np.maximum(0.0, 1.0 - y * z) ** 2


@pytest.mark.parametrize("loss", ["logistic", "squared_hinge"])
@pytest.mark.parametrize("fix_quirks", [False, True])
def test_held_out_scores_are_the_numpy_recomputation(fix_quirks, loss, tmp_path):
    K = 3
    cfg, src, sch, parts = make(CASES["naive"], "GD", K, loss=loss, fix_quirks=fix_quirks, lr=0.3)
    cfg.input_dir = str(tmp_path) + "/"
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    res = tr.run()
    cfg.verbose = True
    lines = []
    ev = evaluate(tr, res, log=lines.append, write=True)
    Bs = losses.sweep_unpack(res.betaset, K, tr.d_x)
    R = len(Bs)
    used = parts if fix_quirks else parts[: cfg.n_workers - 1]  # (partition W is skipped, as for a single model)
    assert len(used) == (4 if fix_quirks else 3)
    Xte, yte = src._test
    folds = np.zeros((R, K))
    for i in range(R):
        for k in range(K):
            held = np.concatenate([_loss_rows(tr.loss, X[k::K], y[k::K], Bs[i, k]) for X, y in used])
            kept = np.concatenate([_loss_rows(tr.loss, X, y, Bs[i, k]) for X, y in without_fold(used, K, k)])
            assert len(held) == held_out_rows(used, K, k) and len(held) + len(kept) == 40 * len(used)
            folds[i, k] = held.mean()
            assert ev.training_loss[i, k] == pytest.approx(kept.mean(), rel=1e-10)
            assert ev.testing_loss[i, k] == pytest.approx(_loss_rows(tr.loss, Xte, yte, Bs[i, k]).mean(), rel=1e-10)
    assert ev.cv_loss_folds.shape == (R, K) and ev.cv_loss.shape == (R,) and ev.cv_std.shape == (R,)
    np.testing.assert_allclose(ev.cv_loss_folds, folds, rtol=1e-10)
    np.testing.assert_allclose(ev.cv_loss, folds.mean(axis=1), rtol=1e-10)
    np.testing.assert_allclose(ev.cv_std, folds.std(axis=1, ddof=1), rtol=1e-8)
    assert ev.best is None and ev.auc.shape == (R, K) and ev.n_train == 40 * len(used)
    assert np.all(folds[-1] < folds[0]) and np.all(ev.cv_std > 0)  # the models learn; the folds differ

    # the console: a fold header before each model's lines, one closing line
    n_k = [held_out_rows(parts, K, k) for k in range(K)]
    heads = [i for i, l in enumerate(lines) if l.startswith(">> Fold ")]
    assert [lines[i] for i in heads] == [">> Fold %d: held-out rows = %d of %d" % (k, n_k[k], cfg.n_rows)
                                         for k in range(K)]
    for h in heads:
        assert all(l.startswith("Iteration ") for l in lines[h + 1: h + 1 + R])
    assert len([l for l in lines if l.startswith("Iteration ")]) == K * R
    closing = [l for l in lines if l.startswith(">> CV: ")]
    assert closing == [">> CV: %d folds, held-out loss = %g +- %g (final round)" % (K, ev.cv_loss[-1], ev.cv_std[-1])]
    assert lines.index(closing[0]) > heads[-1] + R and lines[-1] == ">>> Done"
    assert not any(l.startswith(">> Best model") or l.startswith(">> Model ") for l in lines)

    # the files: cv{k}_ before sqhinge_, and one cv_loss file named like the training-loss file
    sq = "sqhinge_" if loss == "squared_hinge" else ""
    base = sch.output_names(fix_quirks)
    names = {key: os.path.basename(v) for key, v in ev.files.items()}
    want = {"cv%d_%s" % (k, key): "cv%d_%s%s" % (k, sq, v) for k in range(K) for key, v in base.items()}
    want["cv_loss"] = sq + base["training_loss"].replace("training_loss", "cv_loss")
    assert names == want
    assert all(os.path.exists(p) for p in ev.files.values())
    assert os.path.dirname(ev.files["cv_loss"]) == os.path.dirname(ev.files["cv0_training_loss"])
    # (the result files keep the reference's three decimals)
    np.testing.assert_allclose(np.loadtxt(ev.files["cv_loss"]), ev.cv_loss, rtol=0, atol=5.01e-4)
    np.testing.assert_allclose(np.loadtxt(ev.files["cv1_training_loss"]), ev.training_loss[:, 1], rtol=0, atol=5.01e-4)


def test_cv_loss_file_name_follows_the_training_loss_file(tmp_path):
    from erasurehead_amd.engine.evaluate import _write_cv_loss

    d = str(tmp_path)
    files = {"cv0_training_loss": os.path.join(d, "cv0_sqhinge_coded_acc_2_training_loss.dat")}
    _write_cv_loss(files, "cv0_", [1.0, 0.5])
    assert files["cv_loss"] == os.path.join(d, "sqhinge_coded_acc_2_cv_loss.dat") and os.path.exists(files["cv_loss"])
    files = {"cv0_training_loss": os.path.join(d, "cv0_odd_name.dat")}  # a name that does not say training_loss
    _write_cv_loss(files, "cv0_", [1.0, 0.5])
    assert files["cv_loss"] == os.path.join(d, "cv_loss_odd_name.dat") and os.path.exists(files["cv_loss"])


def test_l1_reports_sparsity_per_fold_model(tmp_path):
    K = 2
    cfg, src, sch, parts = make(CASES["naive"], "GD", K, l1=0.02, rounds=3)
    cfg.input_dir = str(tmp_path) + "/"
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    res = tr.run()
    cfg.verbose = True
    lines = []
    ev = evaluate(tr, res, log=lines.append, write=True)
    got = losses.sweep_unpack(res.betaset, K, tr.d_x)
    np.testing.assert_array_equal(ev.nnz, np.count_nonzero(got, axis=2))
    for k in range(K):
        assert ">> L1: l1 = 0.02, nnz = %d of %d" % (ev.nnz[-1, k], tr.d_x) in lines
        assert os.path.basename(ev.files["cv%d_nnz" % k]) == os.path.basename(ev.files["cv%d_auc" % k]).replace("auc", "nnz")


# ---- 4. every rejection names the flag, and is raised before data is loaded
BASE = dict(n_procs=5, n_rows=160, n_cols=6, input_dir="/tmp/x")


@pytest.mark.parametrize("kw,match", [
    (dict(cv=1), "--cv.*2..8"),
    (dict(cv=9), "--cv.*2..8"),
    (dict(cv=0), "--cv.*2..8"),
    (dict(cv=3, loss="softmax"), "--cv.*softmax"),
    (dict(cv=3, loss="softmax", classes=3), "--cv.*softmax"),
    (dict(cv=3, ovr=3), "--cv.*--ovr"),
    (dict(cv=3, classes=3), "--cv.*--classes"),
    (dict(cv=3, sweep_alpha=[1e-3, 1e-2]), "--cv.*--alphas"),
    (dict(cv=3, sweep_lr=[1.0, 2.0]), "--cv.*--lrs"),
    (dict(cv=3, sweep_l1=[0.0, 1e-3]), "--cv.*--l1s"),
    (dict(cv=3, class_weight="balanced"), "--cv.*--class-weight"),
    (dict(cv=3, class_weight="2:1"), "--cv.*--class-weight"),
    (dict(cv=3, sample_weights="/tmp/w.dat"), "--cv.*--sample-weights"),
    (dict(cv=3, precision="bf16"), "--cv.*bf16"),
    (dict(cv=3, is_real=1, dataset="amazon"), "--cv.*sparse"),
])
def test_config_rejections_name_the_flag(kw, match):
    with pytest.raises(ValueError, match=match):
        RunConfig(**BASE, **kw)


def test_config_accepts_what_it_should():
    assert RunConfig(**BASE).cv is None
    for K in (2, 8):
        assert RunConfig(**BASE, cv=K).cv == K
    for loss in ("auto", "logistic", "least_squares", "squared_hinge"):
        assert RunConfig(**BASE, cv=3, loss=loss, l1=1e-3).l1 == 1e-3
    assert RunConfig(**BASE, cv=3, precision="fp32x64").sweep() is None
    assert losses.LOSS_NAMES == {"logistic": 0, "least_squares": 1, "squared_hinge": 2}


def test_trainer_rejections_come_before_any_load(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the trainer loaded data before it rejected the run")

    import scipy.sparse as sps

    cfg, src, sch, parts = make(CASES["naive"])
    sparse = ArraySource([(sps.csr_matrix(X), y) for X, y in parts], (sps.csr_matrix(src._test[0]), src._test[1]),
                         sparse=True)
    monkeypatch.setattr(sparse, "partition", boom)
    with pytest.raises(ValueError, match="--cv.*sparse"):
        Trainer(cfg, DistEnv(), sparse, scheme=sch)

    # a source that brings sample weights of its own makes the run weighted: rejected by name as well
    cfg, src, sch, parts = make(CASES["naive"])
    weighted = ArraySource(parts, src._test, weights=[np.ones(len(y)) for _, y in parts])
    monkeypatch.setattr(weighted, "partition", boom)
    with pytest.raises(ValueError, match="--cv.*weights"):
        Trainer(cfg, DistEnv(), weighted, scheme=sch)

    # ... whatever the loss: with least squares the weights' own rejection must not come first
    cfg, src, sch, parts = make(CASES["naive"], loss="least_squares")
    weighted = ArraySource(parts, src._test, weights=[np.ones(len(y)) for _, y in parts])
    monkeypatch.setattr(weighted, "partition", boom)
    with pytest.raises(ValueError, match="--cv.*weights"):
        Trainer(cfg, DistEnv(), weighted, scheme=sch)

    # the fold counts assume the scheme's equal partitions: an n_rows they do not add up to is refused before a load,
    cfg, src, sch, parts = make(CASES["naive"])
    cfg.n_rows += 2
    sch.n_samples += 2
    monkeypatch.setattr(src, "partition", boom)
    with pytest.raises(ValueError, match="--cv.*multiple of the partition count"):
        Trainer(cfg, DistEnv(), src, scheme=sch)
    monkeypatch.undo()
    # ... and a source whose partitions have other sizes as soon as they are loaded
    cfg, src, sch, parts = make(CASES["naive"])
    uneven = ArraySource([(X[: 40 - p], y[: 40 - p]) for p, (X, y) in enumerate(parts)], src._test)
    with pytest.raises(ValueError, match="--cv: partition 1 has 39 rows.*40"):
        Trainer(cfg, DistEnv(), uneven, scheme=sch)
    cfg.cv = None  # (a run without the flag takes such a source as it always did)
    Trainer(cfg, DistEnv(), uneven, scheme=sch)

    # more than 1024 columns: a limit of the GPU kernel, decided before anything is loaded
    cfg, src, sch, parts = make(CASES["naive"], d=1030, rows=4)
    with pytest.raises(ValueError, match="--cv.*1024"):
        ModelSpec.resolve(cfg, sch, False, False, get_precision("fp64"), True)
    assert ModelSpec.resolve(cfg, sch, False, False, get_precision("fp64"), False).kind == "cv"

    # a fold that holds every row leaves its model nothing to train on
    cfg, src, sch, parts = make(CASES["naive"], rows=1)
    with pytest.raises(ValueError, match="--cv.*every row"):
        ModelSpec.resolve(cfg, sch, False, False, get_precision("fp64"), False)

    # auto means what it means without the flag: least squares for the reference's regression data set
    cfg, src, sch, parts = make_binary(CASES["frc"], "GD", loss="auto", cv=2, alpha=ALPHA, lr=LR)
    cfg.dataset = "kc_house_data"
    assert sch.has_linear and Trainer(cfg, DistEnv(), src, scheme=sch).loss == losses.LEAST_SQUARES
    cfg.dataset = "x"
    assert Trainer(cfg, DistEnv(), src, scheme=sch).loss == losses.LOGISTIC


# ---- 5. the CLI
ARGV = ["5", "160", "6", "/tmp/eh_cli_cv/", "0", "x", "0", "0", "0", "0", "0", "0", "GD"]


def test_cli_parses_and_rejects(capsys):
    cfg, _ = cli.parse(ARGV + ["--cv", "4", "--loss", "squared_hinge", "--l1", "1e-3"])
    assert cfg.cv == 4 and cfg.loss == "squared_hinge" and cfg.l1 == 1e-3
    assert cli.parse(ARGV)[0].cv is None
    for extra, match in ((["--cv", "9"], "2..8"), (["--cv", "1"], "2..8"), (["--cv", "3", "--classes", "3"], "--classes"),
                         (["--cv", "3", "--loss", "softmax"], "softmax"), (["--cv", "3", "--ovr", "3"], "--ovr"),
                         (["--cv", "3", "--alphas", "1e-3,1e-2"], "--alphas"),
                         (["--cv", "3", "--lrs", "1,2"], "--lrs"), (["--cv", "3", "--l1s", "0,1e-3"], "--l1s"),
                         (["--cv", "3", "--class-weight", "balanced"], "--class-weight"),
                         (["--cv", "3", "--sample-weights", "/tmp/w.dat"], "--sample-weights"),
                         (["--cv", "3", "--precision", "bf16"], "bf16")):
        with pytest.raises(ValueError, match="--cv.*" + match):
            cli.parse(ARGV + extra)
    capsys.readouterr()


def test_cli_runs_on_synthetic_data(capsys, tmp_path):
    argv = ARGV[:3] + [str(tmp_path) + "/"] + ARGV[4:]
    rc = cli.main(argv + ["--data", "synthetic", "--cv", "3", "--device", "cpu", "--num-itrs", "3", "--lr", "0.5",
                          "--seed", "0", "--loss", "squared_hinge"])
    assert rc == 0
    out = capsys.readouterr().out.splitlines()
    assert len([l for l in out if l.startswith("Iteration ")]) == 9
    assert [l for l in out if l.startswith(">> Fold ")] == [
        ">> Fold 0: held-out rows = 56 of 160", ">> Fold 1: held-out rows = 52 of 160",
        ">> Fold 2: held-out rows = 52 of 160"]
    assert len([l for l in out if l.startswith(">> CV: 3 folds, held-out loss = ")]) == 1
    res = sorted(os.listdir(os.path.join(str(tmp_path), "results")))
    assert len(res) == 3 * 5 + 1 and sum(f.startswith("sqhinge_") and "cv_loss" in f for f in res) == 1
    assert all(f.startswith("cv%d_sqhinge_" % k) for k in range(3) for f in res[5 * k: 5 * k + 5])


# ---- 6. checkpoints
def test_checkpoint_resumes_and_refuses_another_k(tmp_path):
    ck = str(tmp_path / "ck.pt")
    K = 3
    _, full, _ = run(CASES["cyclic"], "AGD", K)
    cfg, src, sch, parts = make(CASES["cyclic"], "AGD", K, checkpoint_every=4, checkpoint_path=ck, rounds=4)
    Trainer(cfg, DistEnv(), src, scheme=sch).run()
    assert torch.load(ck, weights_only=True)["cv"] == K
    cfg, src, sch2, parts = make(CASES["cyclic"], "AGD", K, resume=ck)
    res = Trainer(cfg, DistEnv(), src, scheme=None).run()  # the scheme's code comes back from the checkpoint
    np.testing.assert_allclose(res.betaset, full.betaset, **TOL)

    # d = 33 at K = 2 and d = 22 at K = 3 give the same flattened length: only the stored cv tells them apart
    cfg, src, sch2, parts = make(CASES["cyclic"], "AGD", 2, resume=ck)
    with pytest.raises(ValueError, match="cv = 3.*cv = 2"):
        Trainer(cfg, DistEnv(), src).run()
    cfg, src, sch2, parts = make_binary(CASES["cyclic"], "AGD", resume=ck, alpha=ALPHA, lr=LR)
    with pytest.raises(ValueError, match="cv = 3.*cv = None"):
        Trainer(cfg, DistEnv(), src).run()


def test_an_old_checkpoint_without_the_key_resumes(tmp_path):
    """A checkpoint of a run without --cv has no ``cv`` key (as every checkpoint written before the flag existed): it
    resumes such a run as before, and a --cv run refuses it."""
    ck = str(tmp_path / "old.pt")
    cfg, src, sch, parts = make_binary(CASES["cyclic"], "AGD", alpha=ALPHA, lr=LR)
    full = Trainer(cfg, DistEnv(), src, scheme=sch).run()
    cfg, src, sch, parts = make_binary(CASES["cyclic"], "AGD", alpha=ALPHA, lr=LR, checkpoint_every=4,
                                       checkpoint_path=ck, rounds=4)
    Trainer(cfg, DistEnv(), src, scheme=sch).run()
    assert "cv" not in torch.load(ck, weights_only=True)
    cfg, src, sch, parts = make_binary(CASES["cyclic"], "AGD", alpha=ALPHA, lr=LR, resume=ck)
    res = Trainer(cfg, DistEnv(), src).run()
    np.testing.assert_allclose(res.betaset, full.betaset, **TOL)
    cfg, src, sch, parts = make(CASES["cyclic"], "AGD", 2, resume=ck)
    with pytest.raises(ValueError, match="cv = None.*cv = 2"):
        Trainer(cfg, DistEnv(), src).run()


# ---- 7. a run without the flag
RANK_REPORT_KEYS = {"rank", "role", "device", "transport", "round_loop", "loop_reason", "drain", "release_form",
                    "replicas", "workers", "messages", "partitions", "l1", "prox", "weighted", "class_weight",
                    "weight_sum_over_n", "grad_kernel", "packed_bundles", "plain_bundles", "x_stream_bytes",
                    "storage_max_rel_rounding"}


def test_a_run_without_cv_is_what_it_was():
    from oracle import replay

    cfg, src, sch, parts = make_binary(CASES["naive"], "AGD", alpha=ALPHA, lr=LR)
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    res = tr.run()
    assert tr.cv == 0 and tr.model.kind == "single" and tr.model.fold_rows is None and tr.model.cv_scale is None
    rep = tr.rank_report()
    assert set(rep) - set(tr.rank_stats) == RANK_REPORT_KEYS and "cv" not in rep and "fold_rows" not in rep
    ref = replay(sch, parts, tr.beta0, res.arrivals, "AGD", ALPHA, cfg.n_rows, cfg.eta())
    np.testing.assert_allclose(res.betaset, ref, **TOL)
    ev = evaluate(tr, res, write=False)
    assert ev.cv_loss is None and ev.cv_loss_folds is None and ev.cv_std is None and ev.training_loss.shape == (8,)


# ---- 8. three gloo ranks
def test_three_gloo_ranks_match_the_replay(tmp_path):
    out = str(tmp_path / "cv_gloo.npz")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]),
               EH_CV_OUT=out, EH_CV_DEVICE="cpu")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr",
           "127.0.0.1", f"--master-port={port}", os.path.join(HERE, "mp_cv_run.py")]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    check_against_replay(np.load(out, allow_pickle=True))
