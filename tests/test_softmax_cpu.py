"""Multi-class softmax regression on the CPU: library math against this file's own fp64 oracle and central
finite differences, the engine against a NumPy replay of the logged arrivals, padding, evaluation, result
files, convergence on a planted model, the CLI and the multi-class synthetic generator."""
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
from erasurehead_amd.data.source import ArraySource, SyntheticSource
from erasurehead_amd.data.synthetic import DeviceGMM
from erasurehead_amd.engine import Trainer, evaluate
from erasurehead_amd.models import losses
from erasurehead_amd.ops import DenseGradPlan, SoftmaxGradPlan, SparseGradPlan, get_precision
from erasurehead_amd.parallel.dist import DistEnv

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the test's own oracle, from the spec: z_c = x.B_c, p = softmax(z), r_c = coef (p_c - [y = c]),
# ---- G_c = sum_rows r_c x, CE = logsumexp(z) - z_y
def _probs(X, B):
    Z = X @ B.T
    E = np.exp(Z - Z.max(axis=1, keepdims=True))
    return E / E.sum(axis=1, keepdims=True)


def _grad(X, y, B, coef=1.0):
    R = _probs(X, B)
    R[np.arange(len(y)), y.astype(int)] -= 1.0
    return (coef * R).T @ X


def _ce_sum(X, y, B):
    Z = X @ B.T
    m = Z.max(axis=1)
    return float(np.sum(m + np.log(np.exp(Z - m[:, None]).sum(axis=1)) - Z[np.arange(len(y)), y.astype(int)]))


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


# ---- 1. library gradient
@pytest.mark.parametrize("C", [2, 3, 7, 8])
@pytest.mark.parametrize("coef", [None, 1.0, -0.7])
def test_library_gradient_is_the_oracle(C, coef):
    X, y, B = _data(1, C=C)
    got = losses.softmax_grad(X, y, B, coef)
    assert got.shape == (C, X.shape[1])
    np.testing.assert_allclose(got, _grad(X, y, B, 1.0 if coef is None else coef), rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(losses.worker_grad(losses.SOFTMAX, X, y, B.ravel(), coef), got.ravel())


def test_gradient_is_the_derivative_of_the_cross_entropy():
    X, y, B = _data(2)
    h = 1e-6
    fd = np.empty_like(B)
    for c in range(B.shape[0]):
        for j in range(B.shape[1]):
            e = np.zeros_like(B)
            e[c, j] = h
            fd[c, j] = (_ce_sum(X, y, B + e) - _ce_sum(X, y, B - e)) / (2 * h)
    for g in (losses.softmax_grad(X, y, B), _grad(X, y, B)):
        assert np.max(np.abs(g - fd)) / np.max(np.abs(fd)) < 1e-5


def test_two_classes_are_the_logistic_gradient():
    X, y, B = _data(3, C=2)
    B[0] = 0.0
    G = losses.softmax_grad(X, y, B)
    ref = losses.logistic_grad(X, 2.0 * y - 1.0, B[1])
    np.testing.assert_allclose(G[1], ref, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(G[0], -ref, rtol=1e-12, atol=1e-12)


def test_library_loss_and_accuracy_are_the_oracle():
    X, y, B = _data(4, C=7)
    Z = X @ B.T
    assert losses.softmax_loss(y, Z) == pytest.approx(_ce_sum(X, y, B) / len(y), rel=1e-14)
    assert losses.softmax_loss(y, Z, 1) == pytest.approx(_ce_sum(X, y, B), rel=1e-14)
    assert losses.accuracy(y, Z) == _accuracy(X, y, B)


# ---- 2. overflow
def test_extreme_logits_stay_finite():
    X, y, B = _data(5)
    B *= 800.0 / np.abs(X @ B.T).max()
    assert np.abs(X @ B.T).max() == pytest.approx(800.0)
    G = losses.softmax_grad(X, y, B)
    ce = losses.softmax_loss(y, X @ B.T)
    assert np.all(np.isfinite(G)) and np.isfinite(ce)
    np.testing.assert_allclose(G, _grad(X, y, B), rtol=1e-13, atol=1e-13)
    assert ce == pytest.approx(_ce_sum(X, y, B) / len(y), rel=1e-14)


# ---- 3. the CPU engine against a NumPy replay of the logged arrivals
CASES = {  # (is_coded, partitions, coded_ver, n_procs, s, num_collect)
    "naive": (0, 0, 0, 5, 0, 0),
    "agc_uneven": (1, 0, 3, 9, 2, 6),
    "cyclic": (1, 0, 0, 7, 2, 0),
}


def make(case, rule="GD", rows=40, d=33, C=3, rounds=8, seed=0, precision="fp64", planted=False, **kw):
    is_coded, P, ver, n_procs, s, k = case
    W = n_procs - 1
    key = scheme_key(is_coded, P, ver)
    uneven = key in ("approx", "replication") and W % (s + 1) != 0
    n_parts = make_scheme(key, W, s, rows * W, k, P, allow_uneven=uneven).n_partition_files
    n = rows * n_parts
    rng = np.random.RandomState(seed)

    def draw(m):
        X = rng.randn(m, d) * 0.3
        if not planted:
            return X, rng.randint(0, C, m).astype(np.float64)
        X = X * (1.0 / 0.3)
        p = _probs(X, Bstar)
        return X, np.array([rng.choice(C, p=q) for q in p], dtype=np.float64)

    Bstar = rng.choice([-1.0, 1.0], (C, d)) if planted else None
    parts = [draw(rows) for _ in range(n_parts)]
    test = draw(rows * 2)
    src = ArraySource(parts, test)
    cfg = RunConfig(n_procs, n, d, "/tmp/eh_cpu_softmax/", 0, "x", is_coded, s, P, ver, k, 0, rule, num_itrs=rounds,
                    seed=0, verbose=False, allow_uneven_groups=uneven, loss="softmax", classes=C, lr=5.0,
                    precision=precision, **kw)
    sch = make_scheme(key, W, s, n, k, P, allow_uneven=uneven, rng=np.random.RandomState(7))
    return cfg, src, sch, parts


def replay(scheme, parts, B0, arrivals_log, rule, alpha, n_samples, eta):
    """betaset [R, C, d_x] from the logged arrivals: decode, per-message oracle gradients, GD / AGD with the
    L2 term on the model (the reference's update rules, written out here)."""
    rule = "AGD" if scheme.fixed_agd else rule
    scale = scheme.grad_scale()
    B = np.array(B0, dtype=np.float64)
    U = np.zeros_like(B)
    out = []
    for i, arr in enumerate(arrivals_log):
        used = scheme.decode([Arrival(w, p, t) for (w, p, t) in arr])
        g = np.zeros_like(B)
        for (w, part), c in used.items():
            m = [x for x in scheme.messages if x.worker == w and x.part == part][0]
            g += c * sum(_grad(parts[p][0], parts[p][1], B, coef) for p, coef in m.segments)
        gm = eta[i] / n_samples * scale
        if rule == "GD":
            B = (1.0 - 2.0 * alpha * eta[i]) * B - gm * g
        else:
            theta = 2.0 / (i + 2.0)
            yt = (1 - theta) * B + theta * U
            Bn = yt - gm * g - 2.0 * alpha * eta[i] * B
            U = B + (Bn - B) * (1 / theta)
            B = Bn
        out.append(B.copy())
    return np.array(out)


def _run_and_replay(name, rule, **kw):
    cfg, src, sch, parts = make(CASES[name], rule, **kw)
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    assert tr.loss == losses.SOFTMAX and tr.classes == cfg.classes
    res = tr.run()
    C, d_x, ld_x = tr.classes, tr.d_x, tr.ld_x
    ref = replay(sch, parts, _unpad(tr.beta0, C, d_x, ld_x), res.arrivals, rule, cfg.alpha_value, cfg.n_rows, cfg.eta())
    return tr, res, ref


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_engine_matches_numpy_replay(name, rule):
    tr, res, ref = _run_and_replay(name, rule)
    assert res.betaset.shape == (8, tr.classes * tr.ld_x)
    got = losses.softmax_unpack(res.betaset, tr.classes, tr.d_x)
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-11)
    assert tr.replica_policy in ("encoded", "none")


# ---- 4. padding
def test_padding_stays_zero_and_unpack_round_trips():
    tr, res, ref = _run_and_replay("cyclic", "AGD")
    C, d_x, ld_x = tr.classes, tr.d_x, tr.ld_x
    assert ld_x == 34 and d_x == 33  # one padding column per class block in fp64
    blocks = res.betaset.reshape(-1, C, ld_x)
    assert np.all(blocks[:, :, d_x:] == 0.0)
    assert np.all(np.asarray(tr.beta0).reshape(C, ld_x)[:, d_x:] == 0.0)
    un = losses.softmax_unpack(res.betaset, C, d_x)
    assert un.shape == (8, C, d_x)
    np.testing.assert_array_equal(un, blocks[:, :, :d_x])
    packed = np.stack([losses.softmax_pack(b, ld_x) for b in un])
    np.testing.assert_array_equal(packed, res.betaset)
    with pytest.raises(ValueError):
        losses.softmax_unpack(res.betaset, C + 1, d_x)


# ---- 5. evaluation
def test_evaluate_scores_prints_and_writes(tmp_path):
    cfg, src, sch, parts = make(CASES["naive"], "GD")
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
        assert ev.training_loss[i] == pytest.approx(_ce_sum(Xtr, ytr, B) / len(ytr), rel=1e-10)
        assert ev.testing_loss[i] == pytest.approx(_ce_sum(Xte, yte, B) / len(yte), rel=1e-10)
        assert ev.auc[i] == pytest.approx(_accuracy(Xte, yte, B), abs=1e-12)  # EvalResult.auc holds the accuracy
    it = [l for l in lines if l.startswith("Iteration ")]
    assert len(it) == len(Bs) and all("Accuracy = " in l and "AUC" not in l for l in it)
    names = {k: os.path.basename(v) for k, v in ev.files.items()}
    assert names == {k: "softmax_" + v for k, v in sch.output_names(cfg.fix_quirks).items()}
    assert all(os.path.exists(p) for p in ev.files.values())


# ---- 6. convergence on a planted model
@pytest.mark.parametrize("C", [3, 7])
def test_converges_on_a_planted_model(C):
    cfg, src, sch, parts = make(CASES["naive"], "GD", rows=80, C=C, rounds=30, planted=True)
    assert cfg.n_rows == 320
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    res = tr.run()
    B = losses.softmax_unpack(res.betaset, C, tr.d_x)[-1]
    X = np.vstack([p[0] for p in parts])
    y = np.concatenate([p[1] for p in parts])
    ce, acc = _ce_sum(X, y, B) / len(y), _accuracy(X, y, B)
    majority = np.bincount(y.astype(int), minlength=C).max() / len(y)
    print(f"C={C}: CE {ce:.3f} (log C {np.log(C):.3f}), accuracy {acc:.3f}, majority share {majority:.3f}")
    assert ce < np.log(C)
    assert acc > 2 * majority


# ---- 7. CLI, configuration and plan limits
ARGV = ["5", "160", "6", "/tmp/eh_cli_softmax/", "0", "x", "0", "0", "0", "0", "0", "0", "GD"]


@pytest.mark.parametrize("extra", [[], ["--share-partitions"]])  # accepted, changes nothing: the plan shares already
def test_cli_runs_softmax_on_synthetic_data(extra, capsys, tmp_path):
    argv = ARGV[:3] + [str(tmp_path) + "/"] + ARGV[4:]
    rc = cli.main(argv + ["--data", "synthetic", "--loss", "softmax", "--classes", "3", "--device", "cpu",
                          "--num-itrs", "3", "--lr", "5", "--seed", "0"] + extra)
    assert rc == 0
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Iteration ")]
    assert len(lines) == 3 and all("Accuracy = " in l for l in lines)
    assert os.path.exists(os.path.join(str(tmp_path), "results"))


def test_cli_and_config_name_their_limits(capsys):
    cfg, _ = cli.parse(ARGV + ["--loss", "softmax", "--classes", "3"])
    assert cfg.loss == "softmax" and cfg.classes == 3
    assert cli.parse(ARGV + ["--loss", "softmax"])[0].classes == 2
    with pytest.raises(ValueError, match="2..8"):
        cli.parse(ARGV + ["--loss", "softmax", "--classes", "9"])
    with pytest.raises(ValueError, match="softmax"):
        cli.parse(ARGV + ["--loss", "logistic", "--classes", "3"])
    assert losses.LOSS_NAMES == {"logistic": 0, "least_squares": 1, "squared_hinge": 2}
    assert losses.LOSS_CHOICES == {**losses.LOSS_NAMES, "softmax": 3} and losses.SOFTMAX == 3
    assert losses.is_multiclass(losses.SOFTMAX) and not losses.is_classification(losses.SOFTMAX)
    assert not any(losses.is_multiclass(k) for k in losses.LOSS_NAMES.values())
    capsys.readouterr()


def test_trainer_rejects_bf16_and_sparse_sources():
    import scipy.sparse as sps

    cfg, src, sch, parts = make(CASES["naive"], precision="bf16")
    with pytest.raises(ValueError, match="bf16"):
        Trainer(cfg, DistEnv(), src, scheme=sch)
    cfg, src, sch, parts = make(CASES["naive"])
    sparse = ArraySource([(sps.csr_matrix(X), y) for X, y in parts], (sps.csr_matrix(src._test[0]), src._test[1]),
                         sparse=True)
    with pytest.raises(ValueError, match="sparse"):
        Trainer(cfg, DistEnv(), sparse, scheme=sch)


def test_plan_constructor_checks():
    prec = get_precision("fp64")
    X, y, B = _data(6, n=20, d=6)
    part = lambda yy: {0: (torch.from_numpy(X.copy()), torch.from_numpy(np.asarray(yy, dtype=np.float64)))}  # noqa: E731
    msgs = [[(0, 1.0)]]
    for bad in (1, 9):
        with pytest.raises(ValueError, match="2..8"):
            SoftmaxGradPlan(msgs, part(y), prec, bad, 6)
    with pytest.raises(ValueError, match="partition 0"):
        SoftmaxGradPlan(msgs, part(np.where(np.arange(20) == 3, 3.0, y)), prec, 3, 6)  # a label equal to C
    with pytest.raises(ValueError, match="partition 0"):
        SoftmaxGradPlan(msgs, part(np.where(np.arange(20) == 3, 1.5, y)), prec, 3, 6)
    with pytest.raises(ValueError, match="bf16"):
        SoftmaxGradPlan(msgs, part(y), get_precision("bf16"), 3, 6)
    with pytest.raises(ValueError, match="softmax"):
        DenseGradPlan(msgs, part(y), prec, losses.SOFTMAX, 6)
    with pytest.raises(ValueError, match="softmax"):
        SparseGradPlan(msgs, {}, prec, losses.SOFTMAX, 6)


def test_blocked_plans_reject_a_non_contiguous_y():
    """Both kernels read y with raw LDS-DMA, so both plans require it contiguous and name the partition."""
    from erasurehead_amd.ops.multimodel import MultiModelGradPlan

    prec = get_precision("fp64")
    X = torch.zeros((10, 6), dtype=torch.float64)
    y = torch.zeros(20, dtype=torch.float64)[::2]  # ten valid labels for either plan, stride 2
    assert not y.is_contiguous()
    msgs, parts = [[(0, 1.0)]], {0: (X, y)}
    with pytest.raises(ValueError, match="partition 0"):
        SoftmaxGradPlan(msgs, parts, prec, 3, 6)
    with pytest.raises(ValueError, match="partition 0"):
        MultiModelGradPlan(msgs, parts, prec, losses.LOGISTIC, 3, 6)
    parts = {0: (X, y.contiguous())}  # the same data, contiguous: both construct
    assert SoftmaxGradPlan(msgs, parts, prec, 3, 6).nslots == 1
    assert MultiModelGradPlan(msgs, parts, prec, losses.LOGISTIC, 3, 6).nslots == 1


def test_plan_on_cpu_tensors_is_the_oracle():
    prec = get_precision("fp64")
    rng = np.random.RandomState(8)
    C, d = 7, 37
    ld = prec.ld(d)
    raw, parts = {}, {}
    for p, n in enumerate([57, 64, 1]):
        X, y = rng.randn(n, d) * 0.3, rng.randint(0, C, n).astype(np.float64)
        raw[p] = (X, y)
        Xp = np.zeros((n, ld))
        Xp[:, :d] = X
        parts[p] = (torch.from_numpy(Xp), torch.from_numpy(y))
    B = rng.randn(C, d) * 6.0 / np.sqrt(d)
    msgs = [[(0, 1.0), (1, -0.7)], [(2, 2.5)], [(1, 1.0), (0, 0.3), (2, 1.0)]]
    plan = SoftmaxGradPlan(msgs, parts, prec, C, d)
    assert (plan.nslots, plan.ld, plan.d) == (3, C * ld, C * ld) and plan.out_buffer(2).shape == (2, 3, C * ld)
    assert plan.distinct_bytes == (57 + 64 + 1) * ld * 8 and plan.bytes_per_round == (57 + 64 + 1 + 64 + 57 + 1) * ld * 8
    G = plan.run(torch.from_numpy(losses.softmax_pack(B, ld)), plan.out_buffer()[0])
    for s, m in enumerate(msgs):
        ref = sum(_grad(raw[p][0], raw[p][1], B, c) for p, c in m)
        got = G[s].numpy().reshape(C, ld)
        assert np.max(np.abs(got[:, :d] - ref)) / np.max(np.abs(ref)) < 1e-12
        assert np.all(got[:, d:] == 0.0)


# ---- 8. synthetic generator
def test_synthetic_generator_keeps_binary_draws_and_draws_classes():
    a = DeviceGMM(120, 9, 4, seed=3)
    b = DeviceGMM(120, 9, 4, seed=3, classes=None)
    for p in range(4):
        (Xa, ya), (Xb, yb) = a.partition(p), b.partition(p)
        assert torch.equal(Xa, Xb) and torch.equal(ya, yb)
    assert torch.equal(a.test()[0], b.test()[0]) and np.array_equal(a.beta_star, b.beta_star)
    g = DeviceGMM(400, 9, 4, seed=3, classes=4)
    ys = torch.cat([g.partition(p)[1] for p in range(4)])
    assert set(ys.tolist()) == {0.0, 1.0, 2.0, 3.0}
    assert g.partition(1)[0].shape == (100, 9) and torch.equal(g.partition(1)[1], g.partition(1)[1])
    src = SyntheticSource(400, 9, 4, 3, classes=4)
    X, y = src.partition(0, get_precision("fp32"), "cpu")
    assert X.shape == (100, 12) and X.dtype == torch.float32 and bool((X[:, 9:] == 0).all())
    assert y.dtype == torch.float32 and bool(((y >= 0) & (y < 4) & (y == y.floor())).all())


# ---- 9. three gloo ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_three_gloo_ranks_match_the_replay(tmp_path):
    out = str(tmp_path / "softmax_gloo.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]),
               EH_SOFTMAX_OUT=out, EH_SOFTMAX_DEVICE="cpu")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr",
           "127.0.0.1", f"--master-port={_free_port()}", os.path.join(HERE, "mp_softmax_run.py")]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    z = np.load(out, allow_pickle=True)
    cfg, src, sch, parts = make(CASES["agc_uneven"], "AGD")
    C, d_x, ld_x = 3, 33, 34
    arrivals = [[tuple(a) for a in rnd] for rnd in z["arrivals"]]
    ref = replay(sch, parts, _unpad(z["beta0"], C, d_x, ld_x), arrivals, "AGD", cfg.alpha_value, cfg.n_rows, cfg.eta())
    np.testing.assert_allclose(losses.softmax_unpack(z["betaset"], C, d_x), ref, rtol=1e-9, atol=1e-11)
