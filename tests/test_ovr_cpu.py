"""One-vs-rest multi-class training (--ovr C) on the CPU: library math against this file's own fp64 oracle and
central finite differences, the engine against a NumPy replay of the logged arrivals, padding, evaluation, result
files, a planted model, every rejection (before data is loaded), the CLI, --l1, checkpoints and three gloo ranks."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from erasurehead_amd import cli
from erasurehead_amd.codes import make_scheme, scheme_key
from erasurehead_amd.codes.schemes import Arrival
from erasurehead_amd.config import RunConfig
from erasurehead_amd.data.source import ArraySource
from erasurehead_amd.engine import Trainer, evaluate
from erasurehead_amd.models import losses
from erasurehead_amd.ops import get_precision
from erasurehead_amd.parallel.dist import DistEnv
from test_softmax_cpu import CASES

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = dict(rtol=1e-9, atol=1e-11)  # the engine tolerance of tests/test_softmax_cpu.py / test_engine_cpu.py
LOSS_OF = {"logistic": losses.LOGISTIC, "squared_hinge": losses.SQUARED_HINGE}


# ---- the test's own oracle, from the spec: y_k = +1 if y == k else -1, z_k = x . B_k,
# ---- logistic      l = log(1 + exp(-y_k z_k)),     dl/dz = -y_k / (1 + exp(y_k z_k))
# ---- squared hinge l = max(0, 1 - y_k z_k)^2,      dl/dz = -2 y_k max(0, 1 - y_k z_k)
def _signs(y, C):
    Y = -np.ones((len(y), C))
    Y[np.arange(len(y)), y.astype(int)] = 1.0
    return Y


def _row_loss(kind, X, y, B):
    m = _signs(y, B.shape[0]) * (X @ B.T)
    if kind == losses.LOGISTIC:
        return np.logaddexp(0.0, -m).sum(axis=1)
    return (np.maximum(0.0, 1.0 - m) ** 2).sum(axis=1)


def _loss_sum(kind, X, y, B):
    return float(_row_loss(kind, X, y, B).sum())


def _grad(kind, X, y, B, coef=1.0):
    Y = _signs(y, B.shape[0])
    m = Y * (X @ B.T)
    if kind == losses.LOGISTIC:
        R = -Y / (1.0 + np.exp(m))
    else:
        R = -2.0 * Y * np.maximum(0.0, 1.0 - m)
    return (coef * R).T @ X


def _accuracy(X, y, B):
    return float(np.mean(np.argmax(X @ B.T, axis=1) == y.astype(int)))


def _data(seed, n=300, d=37, C=3):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, d) * 0.3
    y = rng.randint(0, C, n).astype(np.float64)
    B = rng.randn(C, d) * 6.0 / np.sqrt(d)
    return X, y, B


def _unpad(flat, C, d_x, ld_x):
    return np.asarray(flat).reshape(C, ld_x)[:, :d_x]


# ---- 1. library math
@pytest.mark.parametrize("kind", sorted(LOSS_OF.values()))
@pytest.mark.parametrize("C", [2, 3, 7, 8])
@pytest.mark.parametrize("coef", [None, -0.7])
def test_library_gradient_and_loss_are_the_oracle(kind, C, coef):
    X, y, B = _data(1, C=C)
    np.testing.assert_array_equal(losses.ovr_labels(y, C), _signs(y, C))
    got = losses.ovr_grad(kind, X, y, B, coef)
    assert got.shape == (C, X.shape[1])
    np.testing.assert_allclose(got, _grad(kind, X, y, B, 1.0 if coef is None else coef), rtol=1e-12, atol=1e-12)
    Z = X @ B.T
    assert losses.ovr_loss(kind, y, Z) == pytest.approx(_loss_sum(kind, X, y, B) / len(y), rel=1e-13)
    assert losses.ovr_loss(kind, y, Z, 1) == pytest.approx(_loss_sum(kind, X, y, B), rel=1e-13)
    np.testing.assert_allclose(losses.ovr_row_loss(kind, y, Z), _row_loss(kind, X, y, B), rtol=1e-13, atol=1e-15)
    for bad in (losses.LEAST_SQUARES, losses.SOFTMAX, losses.LOGISTIC_W):
        with pytest.raises(ValueError, match="one-vs-rest"):
            losses.ovr_grad(bad, X, y, B)


def test_gradient_is_the_derivative_of_the_logistic_loss():
    X, y, B = _data(2)
    h = 1e-6
    fd = np.empty_like(B)
    for c in range(B.shape[0]):
        for j in range(B.shape[1]):
            e = np.zeros_like(B)
            e[c, j] = h
            fd[c, j] = (_loss_sum(losses.LOGISTIC, X, y, B + e) - _loss_sum(losses.LOGISTIC, X, y, B - e)) / (2 * h)
    for g in (losses.ovr_grad(losses.LOGISTIC, X, y, B), _grad(losses.LOGISTIC, X, y, B)):
        assert np.max(np.abs(g - fd)) / np.max(np.abs(fd)) < 1e-5


def test_two_classes_are_two_logistic_gradients():
    X, y, B = _data(3, C=2)
    G = losses.ovr_grad(losses.LOGISTIC, X, y, B)
    np.testing.assert_allclose(G[1], losses.logistic_grad(X, 2.0 * y - 1.0, B[1]), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(G[0], losses.logistic_grad(X, 1.0 - 2.0 * y, B[0]), rtol=1e-12, atol=1e-12)


# ---- 2. the CPU engine against a NumPy replay of the logged arrivals
def make(case, rule="GD", loss="logistic", rows=40, d=33, C=3, rounds=8, seed=0, precision="fp64", planted=False,
         **kw):
    """The shapes of tests/test_softmax_cpu.py::make: class-index labels, a one-vs-rest run of `loss`."""
    is_coded, P, ver, n_procs, s, k = case
    W = n_procs - 1
    key = scheme_key(is_coded, P, ver)
    uneven = key in ("approx", "replication") and W % (s + 1) != 0
    n_parts = make_scheme(key, W, s, rows * W, k, P, allow_uneven=uneven).n_partition_files
    n = rows * n_parts
    rng = np.random.RandomState(seed)
    Bstar = rng.choice([-1.0, 1.0], (C, d)) if planted else None

    def draw(m):
        X = rng.randn(m, d) * 0.3
        if not planted:
            return X, rng.randint(0, C, m).astype(np.float64)
        X = X * (1.0 / 0.3)
        return X, np.argmax(X @ Bstar.T + rng.randn(m, C), axis=1).astype(np.float64)

    parts = [draw(rows) for _ in range(n_parts)]
    src = ArraySource(parts, draw(rows * 2))
    kw.setdefault("lr", 1.0)
    kw.setdefault("ovr", C)
    cfg = RunConfig(n_procs, n, d, "/tmp/eh_cpu_ovr/", 0, "x", is_coded, s, P, ver, k, 0, rule, num_itrs=rounds,
                    seed=0, verbose=False, allow_uneven_groups=uneven, loss=loss, precision=precision, **kw)
    sch = make_scheme(key, W, s, n, k, P, allow_uneven=uneven, rng=np.random.RandomState(7))
    return cfg, src, sch, parts


def replay(kind, scheme, parts, B0, arrivals_log, rule, alpha, n_samples, eta, l1=0.0):
    """betaset [R, C, d_x] from the logged arrivals: decode, per-message oracle gradients, GD / AGD with the L2 term
    on the model (the reference's update rules, written out here) and, with l1 > 0, the soft threshold eta_i * l1."""
    rule = "AGD" if scheme.fixed_agd else rule
    scale = scheme.grad_scale()
    B = np.array(B0, dtype=np.float64)
    U = np.zeros_like(B)
    out = []

    def prox(V, t):
        return V if l1 <= 0 else np.where(np.abs(V) <= t, 0.0, V - np.copysign(t, V))

    for i, arr in enumerate(arrivals_log):
        used = scheme.decode([Arrival(w, p, t) for (w, p, t) in arr])
        g = np.zeros_like(B)
        for (w, part), c in used.items():
            m = [x for x in scheme.messages if x.worker == w and x.part == part][0]
            g += c * sum(_grad(kind, parts[p][0], parts[p][1], B, coef) for p, coef in m.segments)
        gm = eta[i] / n_samples * scale
        if rule == "GD":
            B = prox((1.0 - 2.0 * alpha * eta[i]) * B - gm * g, eta[i] * l1)
        else:
            theta = 2.0 / (i + 2.0)
            yt = (1 - theta) * B + theta * U
            Bn = prox(yt - gm * g - 2.0 * alpha * eta[i] * B, eta[i] * l1)
            U = B + (Bn - B) * (1 / theta)
            B = Bn
        out.append(B.copy())
    return np.array(out)


def _run_and_replay(name, rule, loss="logistic", env=None, **kw):
    cfg, src, sch, parts = make(CASES[name], rule, loss, **kw)
    tr = Trainer(cfg, env or DistEnv(), src, scheme=sch)
    assert tr.loss == LOSS_OF[loss] and tr.ovr is True and tr.classes == cfg.ovr and tr.models == 1
    res = tr.run()
    C, d_x, ld_x = tr.classes, tr.d_x, tr.ld_x
    ref = replay(tr.loss, sch, parts, _unpad(tr.beta0, C, d_x, ld_x), res.arrivals, rule, cfg.alpha_value, cfg.n_rows,
                 cfg.eta(), cfg.l1)
    return tr, res, ref


@pytest.mark.parametrize("loss", sorted(LOSS_OF))
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_engine_matches_numpy_replay(name, rule, loss):
    tr, res, ref = _run_and_replay(name, rule, loss)
    assert res.betaset.shape == (8, tr.classes * tr.ld_x)
    np.testing.assert_allclose(losses.softmax_unpack(res.betaset, tr.classes, tr.d_x), ref, **TOL)
    assert tr.replica_policy in ("encoded", "none")
    rep = tr.rank_report()
    assert rep["ovr"] is True and rep["classes"] == 3


def test_a_run_without_ovr_reports_none_of_it():
    from test_multimodel_cpu import CASES as BIN, make as make_binary

    cfg, src, sch, parts = make_binary(BIN["naive"], "GD")
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    assert tr.ovr is False and tr.classes == 1 and "ovr" not in tr.rank_report()


# ---- 3. padding
def test_padding_stays_zero():
    tr, res, ref = _run_and_replay("cyclic", "AGD", "squared_hinge")
    C, d_x, ld_x = tr.classes, tr.d_x, tr.ld_x
    assert ld_x == 34 and d_x == 33  # one padding column per class block in fp64
    blocks = res.betaset.reshape(-1, C, ld_x)
    assert np.all(blocks[:, :, d_x:] == 0.0)
    assert np.all(np.asarray(tr.beta0).reshape(C, ld_x)[:, d_x:] == 0.0)
    packed = np.stack([losses.softmax_pack(b, ld_x) for b in losses.softmax_unpack(res.betaset, C, d_x)])
    np.testing.assert_array_equal(packed, res.betaset)


# ---- 4. evaluation
@pytest.mark.parametrize("loss", sorted(LOSS_OF))
def test_evaluate_scores_prints_and_writes(loss, tmp_path):
    cfg, src, sch, parts = make(CASES["naive"], "GD", loss)
    cfg.input_dir = str(tmp_path) + "/"
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    res = tr.run()
    cfg.verbose = True
    lines = []
    ev = evaluate(tr, res, log=lines.append, write=True)
    Bs = losses.softmax_unpack(res.betaset, tr.classes, tr.d_x)
    Xtr = np.vstack([parts[p][0] for p in range(cfg.n_workers - 1)])  # (partition W is skipped, as for logistic)
    ytr = np.concatenate([parts[p][1] for p in range(cfg.n_workers)])[: Xtr.shape[0]]
    Xte, yte = src._test
    for i, B in enumerate(Bs):
        assert ev.training_loss[i] == pytest.approx(_loss_sum(tr.loss, Xtr, ytr, B) / len(ytr), rel=1e-10)
        assert ev.testing_loss[i] == pytest.approx(_loss_sum(tr.loss, Xte, yte, B) / len(yte), rel=1e-10)
        assert ev.auc[i] == pytest.approx(_accuracy(Xte, yte, B), abs=1e-12)  # EvalResult.auc holds the accuracy
    it = [l for l in lines if l.startswith("Iteration ")]
    assert len(it) == len(Bs) and all("Accuracy = " in l and "AUC" not in l for l in it)
    assert not any(l.startswith(">> L1") for l in lines)
    prefix = "ovr_" + ("sqhinge_" if loss == "squared_hinge" else "")
    names = {k: os.path.basename(v) for k, v in ev.files.items()}
    assert names == {k: prefix + v for k, v in sch.output_names(cfg.fix_quirks).items()}
    assert all(os.path.exists(p) for p in ev.files.values())
    np.testing.assert_array_equal(ev.nnz, np.count_nonzero(Bs.reshape(len(Bs), -1), axis=1))


def test_ties_predict_the_first_class():
    """A zero model scores every class 0: argmax takes index 0, so the accuracy is the share of class 0."""
    cfg, src, sch, parts = make(CASES["naive"], "GD", rounds=1, lr=0.0, alpha=0.0)
    cfg.seed = None
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    res = tr.run()
    res.betaset[:] = 0.0
    ev = evaluate(tr, res, write=False)
    assert ev.auc[0] == float(np.mean(src._test[1] == 0.0))
    assert ev.testing_loss[0] == pytest.approx(3 * np.log(2.0), rel=1e-12)


# ---- 5. a planted model
@pytest.mark.parametrize("loss", sorted(LOSS_OF))
def test_accuracy_rises_above_chance_on_a_planted_model(loss):
    C = 4
    cfg, src, sch, parts = make(CASES["naive"], "GD", loss, rows=80, C=C, rounds=30, planted=True,
                                lr=1.0 if loss == "logistic" else 0.05)
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    res = tr.run()
    ev = evaluate(tr, res, write=False)
    y = src._test[1]
    majority = np.bincount(y.astype(int), minlength=C).max() / len(y)
    print(f"{loss}: test accuracy {ev.auc[0]:.3f} -> {ev.auc[-1]:.3f}, majority share {majority:.3f}, "
          f"loss {ev.training_loss[0]:.3f} -> {ev.training_loss[-1]:.3f}")
    assert ev.auc[-1] > 2 * majority or ev.auc[-1] > 0.8
    assert ev.auc[-1] > 1.0 / C + 0.25
    assert ev.training_loss[-1] < ev.training_loss[0]


# ---- 6. every rejection names the flag, and is raised before data is loaded
BASE = dict(n_procs=5, n_rows=160, n_cols=6, input_dir="/tmp/x")


@pytest.mark.parametrize("kw,match", [
    (dict(ovr=1), "--ovr.*2..8"),
    (dict(ovr=9), "--ovr.*2..8"),
    (dict(ovr=3, loss="least_squares"), "--ovr.*least_squares"),
    (dict(ovr=3, loss="softmax"), "--ovr.*softmax"),
    (dict(ovr=3, loss="logistic", classes=3), "--ovr.*--classes"),
    (dict(ovr=3, classes=3), "--ovr.*--classes"),
    (dict(ovr=3, sweep_alpha=[1e-3, 1e-2]), "--ovr.*--alphas"),
    (dict(ovr=3, sweep_lr=[1.0, 2.0]), "--ovr.*--lrs"),
    (dict(ovr=3, sweep_l1=[0.0, 1e-3]), "--ovr.*--l1s"),
    (dict(ovr=3, class_weight="balanced"), "--ovr.*--class-weight"),
    (dict(ovr=3, class_weight="2:1"), "--ovr.*--class-weight"),
    (dict(ovr=3, sample_weights="/tmp/w.dat"), "--ovr.*--sample-weights"),
])
def test_config_rejections_name_the_flag(kw, match):
    with pytest.raises(ValueError, match=match):
        RunConfig(**BASE, **kw)


def test_config_accepts_what_it_should():
    assert RunConfig(**BASE).ovr is None
    for C in (2, 8):
        assert RunConfig(**BASE, ovr=C).ovr == C
    assert RunConfig(**BASE, ovr=3, loss="squared_hinge", l1=1e-3).l1 == 1e-3
    assert RunConfig(**BASE, ovr=3, loss="auto").classes is None  # --classes stays softmax's
    with pytest.raises(ValueError, match="softmax"):  # and keeps raising without --ovr
        RunConfig(**BASE, loss="logistic", classes=3)
    assert losses.LOSS_NAMES == {"logistic": 0, "least_squares": 1, "squared_hinge": 2}
    assert losses.LOSS_CHOICES == {**losses.LOSS_NAMES, "softmax": 3}


def test_trainer_rejections_come_before_any_load(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the trainer loaded data before it rejected the run")

    # auto resolving to least squares: the reference's dispatch for its regression data set
    cfg, src, sch, parts = make(CASES["naive"], loss="auto")
    cfg.dataset = "kc_house_data"
    monkeypatch.setattr(src, "partition", boom)
    assert sch.has_linear
    with pytest.raises(ValueError, match="--ovr.*least squares"):
        Trainer(cfg, DistEnv(), src, scheme=sch)
    cfg.dataset = "x"  # auto otherwise means logistic
    monkeypatch.undo()
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    assert tr.loss == losses.LOGISTIC and tr.ovr

    cfg, src, sch, parts = make(CASES["naive"], precision="bf16")
    monkeypatch.setattr(src, "partition", boom)
    with pytest.raises(ValueError, match="one-vs-rest.*bf16"):
        Trainer(cfg, DistEnv(), src, scheme=sch)

    import scipy.sparse as sps

    cfg, src, sch, parts = make(CASES["naive"])
    sparse = ArraySource([(sps.csr_matrix(X), y) for X, y in parts], (sps.csr_matrix(src._test[0]), src._test[1]),
                         sparse=True)
    monkeypatch.setattr(sparse, "partition", boom)
    with pytest.raises(ValueError, match="one-vs-rest.*sparse"):
        Trainer(cfg, DistEnv(), sparse, scheme=sch)

    # a source that brings sample weights of its own makes the run weighted: rejected by name as well
    cfg, src, sch, parts = make(CASES["naive"])
    weighted = ArraySource(parts, src._test, weights=[np.ones(len(y)) for _, y in parts])
    monkeypatch.setattr(weighted, "partition", boom)
    with pytest.raises(ValueError, match="weights"):
        Trainer(cfg, DistEnv(), weighted, scheme=sch)


def test_plan_limits_and_cpu_plan_is_the_oracle():
    from erasurehead_amd.ops.ovr import OvrGradPlan

    prec = get_precision("fp64")
    X, y, B = _data(6, n=20, d=6)
    part = lambda yy: {0: (torch.from_numpy(X.copy()), torch.from_numpy(np.asarray(yy, dtype=np.float64)))}  # noqa: E731
    msgs = [[(0, 1.0)]]
    for bad in (1, 9):
        with pytest.raises(ValueError, match="one-vs-rest.*2..8"):
            OvrGradPlan(msgs, part(y), prec, losses.LOGISTIC, bad, 6)
    with pytest.raises(ValueError, match="partition 0"):
        OvrGradPlan(msgs, part(np.where(np.arange(20) == 3, 3.0, y)), prec, losses.LOGISTIC, 3, 6)  # a label equal to C
    with pytest.raises(ValueError, match="partition 0"):
        OvrGradPlan(msgs, part(np.where(np.arange(20) == 3, 1.5, y)), prec, losses.LOGISTIC, 3, 6)
    for kind, word in ((losses.LEAST_SQUARES, "least squares"), (losses.SOFTMAX, "softmax"),
                       (losses.LOGISTIC_W, "weights"), (losses.SQUARED_HINGE_W, "weights")):
        with pytest.raises(ValueError, match="one-vs-rest.*" + word):
            OvrGradPlan(msgs, part(y), prec, kind, 3, 6)
    with pytest.raises(ValueError, match="one-vs-rest.*bf16"):
        OvrGradPlan(msgs, part(y), get_precision("bf16"), losses.LOGISTIC, 3, 6)
    with pytest.raises(ValueError, match="one-vs-rest.*sparse"):
        OvrGradPlan.check_supported(prec, losses.LOGISTIC, 3, sparse=True)
    with pytest.raises(ValueError, match="one-vs-rest.*1024"):
        OvrGradPlan.check_supported(prec, losses.LOGISTIC, 3, ld_x=1026, gpu=True)
    OvrGradPlan.check_supported(prec, losses.LOGISTIC, 3, ld_x=1026, gpu=False)  # the CPU path has no width limit

    rng = np.random.RandomState(8)
    C, d = 7, 37
    ld = prec.ld(d)
    raw, parts = {}, {}
    for p, n in enumerate([57, 64, 1]):
        Xp_, yp = rng.randn(n, d) * 0.3, rng.randint(0, C, n).astype(np.float64)
        raw[p] = (Xp_, yp)
        Xp = np.zeros((n, ld))
        Xp[:, :d] = Xp_
        parts[p] = (torch.from_numpy(Xp), torch.from_numpy(yp))
    Bm = rng.randn(C, d) * 6.0 / np.sqrt(d)
    msgs = [[(0, 1.0), (1, -0.7)], [(2, 2.5)], [(1, 1.0), (0, 0.3), (2, 1.0)]]
    for kind in sorted(LOSS_OF.values()):
        plan = OvrGradPlan(msgs, parts, prec, kind, C, d)
        assert (plan.nslots, plan.ld, plan.d) == (3, C * ld, C * ld)
        G = plan.run(torch.from_numpy(losses.softmax_pack(Bm, ld)), plan.out_buffer()[0])
        for s, m in enumerate(msgs):
            ref = sum(_grad(kind, raw[p][0], raw[p][1], Bm, c) for p, c in m)
            got = G[s].numpy().reshape(C, ld)
            assert np.max(np.abs(got[:, :d] - ref)) / np.max(np.abs(ref)) < 1e-12
            assert np.all(got[:, d:] == 0.0)


# ---- 7. the CLI
ARGV = ["5", "160", "6", "/tmp/eh_cli_ovr/", "0", "x", "0", "0", "0", "0", "0", "0", "GD"]


@pytest.mark.parametrize("extra", [["--loss", "logistic"], ["--loss", "squared_hinge", "--share-partitions"], []])
def test_cli_runs_on_synthetic_data(extra, capsys, tmp_path):
    argv = ARGV[:3] + [str(tmp_path) + "/"] + ARGV[4:]
    rc = cli.main(argv + ["--data", "synthetic", "--ovr", "3", "--device", "cpu", "--num-itrs", "3", "--lr", "0.5",
                          "--seed", "0"] + extra)
    assert rc == 0
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Iteration ")]
    assert len(lines) == 3 and all("Accuracy = " in l for l in lines)
    res = os.path.join(str(tmp_path), "results")
    assert os.path.isdir(res) and os.listdir(res) and all(f.startswith("ovr_") for f in os.listdir(res))
    assert all(f.startswith("ovr_sqhinge_") for f in os.listdir(res)) == ("squared_hinge" in extra)


def test_cli_parses_and_rejects(capsys):
    cfg, _ = cli.parse(ARGV + ["--ovr", "4", "--loss", "squared_hinge", "--l1", "1e-3"])
    assert cfg.ovr == 4 and cfg.loss == "squared_hinge" and cfg.classes is None and cfg.l1 == 1e-3
    assert cli.parse(ARGV)[0].ovr is None
    for extra, match in ((["--ovr", "9"], "2..8"), (["--ovr", "3", "--classes", "3"], "--classes"),
                         (["--ovr", "3", "--loss", "softmax"], "softmax"),
                         (["--ovr", "3", "--loss", "least_squares"], "least_squares"),
                         (["--ovr", "3", "--alphas", "1e-3,1e-2"], "--alphas"),
                         (["--ovr", "3", "--lrs", "1,2"], "--lrs"), (["--ovr", "3", "--l1s", "0,1e-3"], "--l1s"),
                         (["--ovr", "3", "--class-weight", "balanced"], "--class-weight"),
                         (["--ovr", "3", "--sample-weights", "/tmp/w.dat"], "--sample-weights")):
        with pytest.raises(ValueError, match="--ovr.*" + match):
            cli.parse(ARGV + extra)
    with pytest.raises(ValueError, match="softmax"):
        cli.parse(ARGV + ["--loss", "logistic", "--classes", "3"])
    capsys.readouterr()


# ---- 8. --l1 thresholds the flattened model
@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_l1_thresholds_the_flattened_model(rule):
    tr, res, ref = _run_and_replay("agc_uneven", rule, "logistic", l1=0.02)
    assert tr.prox and tr.models == 1
    got = losses.softmax_unpack(res.betaset, tr.classes, tr.d_x)
    np.testing.assert_allclose(got, ref, **TOL)
    np.testing.assert_array_equal(got == 0.0, ref == 0.0)
    assert 0 < np.count_nonzero(got[-1] == 0.0) < got[-1].size  # the threshold bites, in every class block's data
    tr.cfg.verbose = True
    lines = []
    ev = evaluate(tr, res, log=lines.append, write=False)
    np.testing.assert_array_equal(ev.nnz, np.count_nonzero(got.reshape(len(got), -1), axis=1))
    assert ">> L1: l1 = 0.02, nnz = %d of %d" % (ev.nnz[-1], tr.classes * tr.d_x) in lines


def test_l1_writes_the_nnz_file(tmp_path):
    cfg, src, sch, parts = make(CASES["naive"], "GD", l1=0.02, rounds=3)
    cfg.input_dir = str(tmp_path) + "/"
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    ev = evaluate(tr, tr.run(), write=True)
    assert os.path.basename(ev.files["nnz"]).startswith("ovr_") and os.path.exists(ev.files["nnz"])
    assert os.path.basename(ev.files["nnz"]) == os.path.basename(ev.files["auc"]).replace("auc", "nnz")


# ---- 9. checkpoints
def test_checkpoint_resumes_and_refuses_another_ovr(tmp_path):
    ck = str(tmp_path / "ck.pt")
    full_tr, full, _ = _run_and_replay("cyclic", "AGD")
    cfg, src, sch, parts = make(CASES["cyclic"], "AGD", checkpoint_every=4, checkpoint_path=ck, rounds=4)
    Trainer(cfg, DistEnv(), src, scheme=sch).run()
    assert torch.load(ck, weights_only=True)["ovr"] == 3
    cfg, src, sch2, parts = make(CASES["cyclic"], "AGD", resume=ck)
    res = Trainer(cfg, DistEnv(), src, scheme=None).run()  # the scheme's code comes back from the checkpoint
    np.testing.assert_allclose(res.betaset, full.betaset, **TOL)

    # d = 22 at C = 3 and d = 33 at C = 2 give the same flattened length: only the stored ovr tells them apart
    cfg, src, sch2, parts = make(CASES["cyclic"], "AGD", resume=ck, C=2)
    with pytest.raises(ValueError, match="ovr = 3.*ovr = 2"):
        Trainer(cfg, DistEnv(), src).run()
    from test_multimodel_cpu import CASES as BIN, make as make_binary

    cfg, src, sch2, parts = make_binary(BIN["cyclic"], "AGD", resume=ck)
    with pytest.raises(ValueError, match="ovr = 3.*ovr = None"):
        Trainer(cfg, DistEnv(), src).run()


# ---- 10. three gloo ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def check_against_replay(z, loss="logistic"):
    cfg, src, sch, parts = make(CASES["agc_uneven"], "AGD", loss)
    C, d_x, ld_x = 3, 33, 34
    arrivals = [[tuple(a) for a in rnd] for rnd in z["arrivals"]]
    ref = replay(LOSS_OF[loss], sch, parts, _unpad(z["beta0"], C, d_x, ld_x), arrivals, "AGD", cfg.alpha_value,
                 cfg.n_rows, cfg.eta())
    np.testing.assert_allclose(losses.softmax_unpack(z["betaset"], C, d_x), ref, **TOL)


def test_three_gloo_ranks_match_the_replay(tmp_path):
    out = str(tmp_path / "ovr_gloo.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]),
               EH_OVR_OUT=out, EH_OVR_DEVICE="cpu")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr",
           "127.0.0.1", f"--master-port={_free_port()}", os.path.join(HERE, "mp_ovr_run.py")]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    check_against_replay(np.load(out, allow_pickle=True))
