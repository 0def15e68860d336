"""(alpha, lr) sweep runs on the CPU: flags and limits, the packed layout, the contract (block k of a sweep run is
the single-model run with (alpha_k, lr_k) and the same seed), evaluation, rejections, checkpoints and three
gloo ranks against the NumPy replay of tests/oracle.py."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from erasurehead_amd import cli
from erasurehead_amd.codes import make_scheme, scheme_key
from erasurehead_amd.config import RunConfig
from erasurehead_amd.data.source import ArraySource
from erasurehead_amd.engine import Trainer, evaluate
from erasurehead_amd.engine.model import ModelSpec
from erasurehead_amd.models import losses
from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.multimodel import MultiModelGradPlan
from erasurehead_amd.ops.update import combine_update, combine_update_blocks
from erasurehead_amd.parallel.dist import DistEnv
from oracle import replay

HERE = os.path.dirname(os.path.abspath(__file__))
ARGV = ["5", "400", "20", "/tmp/eh_mm_cli/", "0", "synthetic", "0", "0", "0", "0", "0", "0", "GD"]
ALPHAS = [1e-3, 1e-2, 1e-1]  # M = 3: three alphas, two distinct lrs
LRS = [1.0, 1.0, 3.0]
TOL = dict(rtol=1e-9, atol=1e-11)  # the engine tolerance of tests/test_softmax_cpu.py / test_engine_cpu.py

CASES = {  # (is_coded, partitions, coded_ver, n_procs, s, num_collect)
    "naive": (0, 0, 0, 5, 0, 0),
    "frc": (1, 0, 1, 7, 2, 0),
    "agc_uneven": (1, 0, 3, 9, 2, 6),
    "cyclic": (1, 0, 0, 7, 2, 0),
}


def make(case, rule="GD", rows=40, d=33, rounds=8, seed=0, precision="fp64", loss="logistic", **kw):
    """The shapes of tests/test_softmax_cpu.py::make with labels in {-1, +1}."""
    is_coded, P, ver, n_procs, s, k = case
    W = n_procs - 1
    key = scheme_key(is_coded, P, ver)
    uneven = key in ("approx", "replication") and W % (s + 1) != 0
    n_parts = make_scheme(key, W, s, rows * W, k, P, allow_uneven=uneven).n_partition_files
    n = rows * n_parts
    rng = np.random.RandomState(seed)

    def draw(m):
        return rng.randn(m, d) * 0.3, rng.choice([-1.0, 1.0], m)

    parts = [draw(rows) for _ in range(n_parts)]
    src = ArraySource(parts, draw(rows * 2))
    kw.setdefault("lr", 1.0)
    cfg = RunConfig(n_procs, n, d, "/tmp/eh_cpu_multimodel/", 0, "x", is_coded, s, P, ver, k, 0, rule, num_itrs=rounds,
                    seed=0, verbose=False, allow_uneven_groups=uneven, loss=loss, precision=precision, **kw)
    sch = make_scheme(key, W, s, n, k, P, allow_uneven=uneven, rng=np.random.RandomState(7))
    return cfg, src, sch, parts


def run(case, rule, env=None, **kw):
    cfg, src, sch, parts = make(case, rule, **kw)
    tr = Trainer(cfg, env or DistEnv(), src, scheme=sch)
    res = tr.run()
    return tr, res, evaluate(tr, res, write=False)


def arrival_sets(res):
    return [[(w, p) for (w, p, _t) in r] for r in res.arrivals]


# ---- 1. flags and limits
def test_flags_zip_and_broadcast(capsys):
    cfg, _ = cli.parse(ARGV + ["--alphas", "1e-4,1e-3,1e-2", "--lrs", "1,2,3"])
    assert cfg.sweep() == [(1e-4, 1.0), (1e-3, 2.0), (1e-2, 3.0)]
    cfg, _ = cli.parse(ARGV + ["--alphas", "1e-4,1e-3", "--lr", "7"])  # absent lrs: the run's own lr
    assert cfg.sweep() == [(1e-4, 7.0), (1e-3, 7.0)]
    cfg, _ = cli.parse(ARGV + ["--lrs", "1,2", "--alpha", "0.5"])  # absent alphas: the run's own alpha
    assert cfg.sweep() == [(0.5, 1.0), (0.5, 2.0)]
    cfg, _ = cli.parse(ARGV + ["--lrs", "1,2"])
    assert cfg.sweep() == [(1.0 / 400, 1.0), (1.0 / 400, 2.0)]
    cfg, _ = cli.parse(ARGV + ["--alphas", "0.25", "--lrs", "1,2,3"])  # length 1: broadcast
    assert cfg.sweep() == [(0.25, 1.0), (0.25, 2.0), (0.25, 3.0)]
    cfg, _ = cli.parse(ARGV)
    assert cfg.sweep() is None and cfg.sweep_etas() is None and cfg.sweep_alpha is None and cfg.sweep_lr is None
    capsys.readouterr()


def test_flag_limits_are_value_errors():
    base = dict(n_procs=5, n_rows=400, n_cols=20, input_dir="/tmp/x")
    with pytest.raises(ValueError, match="equal lengths"):
        RunConfig(**base, sweep_alpha=[1, 2, 3], sweep_lr=[1, 2])
    with pytest.raises(ValueError, match="2..8"):
        RunConfig(**base, sweep_alpha=[1e-3])  # M = 1
    with pytest.raises(ValueError, match="2..8"):
        RunConfig(**base, sweep_alpha=[1e-3], sweep_lr=[2.0])
    with pytest.raises(ValueError, match="2..8"):
        RunConfig(**base, sweep_lr=[float(k + 1) for k in range(9)])  # M = 9
    RunConfig(**base, sweep_lr=[float(k + 1) for k in range(8)])
    with pytest.raises(ValueError, match="lr_schedule"):
        RunConfig(**base, sweep_lr=[1.0, 2.0], lr_schedule=[1.0] * 100)
    RunConfig(**base, sweep_alpha=[1.0, 2.0], lr_schedule=[1.0] * 100)  # alphas alone keep an explicit schedule
    with pytest.raises(ValueError, match="softmax"):
        RunConfig(**base, loss="softmax", sweep_alpha=[1e-3, 1e-2])


@pytest.mark.parametrize("kind", ["const", "invscaling", "exponential"])
def test_model_schedules_are_eta_with_that_lr(kind):
    base = dict(n_procs=5, n_rows=400, n_cols=20, input_dir="/tmp/x", num_itrs=12, lr_kind=kind)
    se = RunConfig(**base, sweep_lr=[0.5, 4.0]).sweep_etas()
    assert se.shape == (2, 12)
    for k, lr in enumerate([0.5, 4.0]):
        np.testing.assert_array_equal(se[k], RunConfig(**base, lr=lr).eta())


def test_block_coeffs_are_the_single_model_coeffs():
    up = losses.UpdateRule("AGD", 123.0, 400, 1.5)
    decay, gm, l2, theta, code = up.block_coeffs(3, [0.5, 4.0], [1e-3, 1e-1])
    for k, (eta, alpha) in enumerate([(0.5, 1e-3), (4.0, 1e-1)]):
        assert (decay[k], gm[k], l2[k], theta, code) == losses.UpdateRule("AGD", alpha, 400, 1.5).coeffs(3, eta)


# ---- 2. the packed layout
def test_pack_unpack_round_trip():
    rng = np.random.RandomState(0)
    B = rng.randn(5, 3, 33)
    flat = losses.sweep_pack(B, 34)
    assert flat.shape == (5, 3 * 34)
    assert np.all(flat.reshape(5, 3, 34)[:, :, 33:] == 0.0)
    np.testing.assert_array_equal(losses.sweep_unpack(flat, 3, 33), B)
    assert losses.sweep_pack(B[0], 34).shape == (3 * 34,)
    np.testing.assert_array_equal(losses.sweep_unpack(losses.sweep_pack(B[0], 34), 3, 33)[0], B[0])
    with pytest.raises(ValueError):
        losses.sweep_unpack(flat, 4, 33)
    with pytest.raises(ValueError):
        losses.sweep_pack(B, 32)


@pytest.mark.parametrize("kind, kw, blocks", [
    ("single", {}, 1), ("softmax", dict(loss="softmax", classes=3), 3), ("ovr", dict(ovr=3), 3),
    ("sweep", dict(sweep_alpha=ALPHAS, sweep_lr=LRS), 3)])
def test_model_spec_lays_out_every_kind(kind, kw, blocks):
    cfg, _, sch, _ = make(CASES["naive"], **kw)
    prec = get_precision("fp64")
    spec = ModelSpec.resolve(cfg, sch, False, False, prec, False)
    ld = blocks * 34
    assert (spec.kind, spec.d_x, spec.ld_x, spec.d, spec.ld, spec.blocks) == (kind, 33, 34, 33 if kind == "single" else ld,
                                                                             ld, blocks)
    b0 = spec.beta0(False, cfg.seed)
    assert b0.shape == (ld,) and np.all(b0.reshape(blocks, 34)[:, 33:] == 0.0)
    assert np.all(b0.reshape(blocks, 34)[:, :33] != 0.0)
    if kind == "sweep":  # every block is the single-model beta_0 of the same seed
        single = ModelSpec.resolve(make(CASES["naive"])[0], sch, False, False, prec, False).beta0(False, cfg.seed)
        for k in range(3):
            np.testing.assert_array_equal(b0.reshape(3, 34)[k], single)
    if kind in ("softmax", "ovr"):  # classes * d_x values drawn in one call
        np.testing.assert_array_equal(spec.unpack(b0[None])[0].ravel(), np.random.RandomState(cfg.seed + 1).randn(3 * 33))
    np.testing.assert_array_equal(spec.beta0(True, cfg.seed), np.zeros(ld))
    x = np.random.RandomState(1).randn(5, blocks, 33)
    flat = spec.pack(x)
    assert flat.shape == (5, ld) and np.all(flat.reshape(5, blocks, 34)[:, :, 33:] == 0.0)
    np.testing.assert_array_equal(spec.unpack(flat), x)
    np.testing.assert_array_equal(spec.unpack(flat[:, : spec.d]), x)  # a stored trajectory is [R, d]
    np.testing.assert_array_equal(spec.rows(flat[:, : spec.d]), flat.reshape(5 * blocks, 34))


def test_padding_stays_zero_over_a_run():
    tr, res, _ = run(CASES["cyclic"], "AGD", sweep_alpha=ALPHAS, sweep_lr=LRS)
    assert (tr.d_x, tr.ld_x, tr.models, tr.d, tr.ld) == (33, 34, 3, 102, 102)
    full = res.betaset.reshape(8, 3, 34)
    assert np.all(full[:, :, 33:] == 0.0) and np.all(full[:, :, :33] != 0.0)
    assert np.all(tr.beta0.reshape(3, 34)[:, 33:] == 0.0)
    assert np.all(tr.beta.reshape(3, 34)[:, 33:].numpy() == 0.0) and np.all(tr.u.reshape(3, 34)[:, 33:].numpy() == 0.0)
    assert np.all(tr.beta_in.reshape(-1, 3, 34)[:, :, 33:].numpy() == 0.0)


# ---- 3. the contract
@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_block_k_is_the_single_model_run(name, rule):
    tr, res, ev = run(CASES[name], rule, sweep_alpha=ALPHAS, sweep_lr=LRS)
    assert isinstance(tr.plan, MultiModelGradPlan) and res.betaset.shape == (8, 3 * tr.ld_x)
    got = losses.sweep_unpack(res.betaset, 3, tr.d_x)
    for k in range(3):
        t1, r1, e1 = run(CASES[name], rule, alpha=ALPHAS[k], lr=LRS[k])
        assert not isinstance(t1.plan, MultiModelGradPlan)
        np.testing.assert_array_equal(tr.beta0.reshape(3, tr.ld_x)[k, : tr.d_x], t1.beta0)  # the same beta_0
        np.testing.assert_allclose(got[:, k], r1.betaset, **TOL)
        assert arrival_sets(res) == arrival_sets(r1)
        for what in ("training_loss", "testing_loss", "auc"):
            np.testing.assert_allclose(getattr(ev, what)[:, k], getattr(e1, what), **TOL)
    assert not np.allclose(got[:, 0], got[:, 2])  # the models do differ


@pytest.mark.parametrize("loss", ["least_squares", "squared_hinge"])
def test_contract_holds_for_the_other_losses(loss):
    tr, res, ev = run(CASES["agc_uneven"], "AGD", loss=loss, sweep_alpha=ALPHAS, sweep_lr=[0.1, 0.1, 0.3])
    got = losses.sweep_unpack(res.betaset, 3, tr.d_x)
    for k in range(3):
        _, r1, e1 = run(CASES["agc_uneven"], "AGD", loss=loss, alpha=ALPHAS[k], lr=[0.1, 0.1, 0.3][k])
        np.testing.assert_allclose(got[:, k], r1.betaset, **TOL)
        np.testing.assert_allclose(ev.testing_loss[:, k], e1.testing_loss, **TOL)


def test_share_partitions_changes_nothing():
    _, a, _ = run(CASES["agc_uneven"], "GD", sweep_alpha=ALPHAS, sweep_lr=LRS)
    tr, b, _ = run(CASES["agc_uneven"], "GD", sweep_alpha=ALPHAS, sweep_lr=LRS, share_partitions=True)
    assert isinstance(tr.plan, MultiModelGradPlan)
    np.testing.assert_array_equal(a.betaset, b.betaset)


def test_block_update_is_the_single_update_per_block():
    rng = np.random.RandomState(3)
    M, bl, dx = 3, 10, 7
    msgs = [torch.from_numpy(rng.randn(M * bl)) for _ in range(9)]
    coefs = list(rng.randn(9))
    decay, gm, l2 = [0.9, 0.8, 0.7], [0.1, 0.2, 0.3], [0.01, 0.02, 0.03]
    for rule in (0, 1):
        beta0 = losses.sweep_pack(rng.randn(M, dx), bl)
        u0 = losses.sweep_pack(rng.randn(M, dx), bl)
        beta, u = torch.from_numpy(beta0.copy()), torch.from_numpy(u0.copy())
        hist, bw = torch.zeros(M * bl, dtype=torch.float64), torch.full((M * bl,), 5.0, dtype=torch.float32)
        combine_update_blocks(msgs, coefs, beta, u, bl, dx, decay, gm, l2, 0.4, rule, hist=hist, beta_w=bw)
        for k in range(M):
            s = slice(k * bl, (k + 1) * bl)
            b1, u1 = torch.from_numpy(beta0[s].copy()), torch.from_numpy(u0[s].copy())
            combine_update([m[s] for m in msgs], coefs, b1, u1, dx, decay[k], gm[k], l2[k], 0.4, rule)
            assert torch.equal(beta[s], b1) and torch.equal(u[s], u1) and torch.equal(hist[s], b1)
            assert torch.equal(bw[s], b1.float()) and bool((bw[s][dx:] == 0).all()) and bool((beta[s][dx:] == 0).all())


def test_plan_on_cpu_tensors_is_the_library_gradient():
    prec = get_precision("fp64")
    rng = np.random.RandomState(8)
    M, d = 5, 37
    ld = prec.ld(d)
    raw, parts = {}, {}
    for p, n in enumerate([57, 64, 1, 0]):
        X, y = rng.randn(n, d) * 0.3, rng.choice([-1.0, 1.0], n)
        raw[p] = (X, y)
        Xp = np.zeros((n, ld))
        Xp[:, :d] = X
        parts[p] = (torch.from_numpy(Xp), torch.from_numpy(y))
    B = rng.randn(M, d) * 6.0 / np.sqrt(d)
    msgs = [[(0, 1.0), (1, -0.7)], [(2, 2.5), (3, 1.0)], [(1, 1.0), (0, 0.3), (2, 1.0)]]
    for loss in (losses.LOGISTIC, losses.LEAST_SQUARES, losses.SQUARED_HINGE):
        plan = MultiModelGradPlan(msgs, parts, prec, loss, M, d)
        assert (plan.nslots, plan.ld, plan.d, plan.identity) == (3, M * ld, M * ld, False)
        assert plan.distinct_bytes == 122 * ld * 8 and plan.bytes_per_round == (121 + 1 + 122) * ld * 8
        G = plan.run(torch.from_numpy(losses.sweep_pack(B, ld)), plan.out_buffer()[0]).numpy().reshape(3, M, ld)
        for s, m in enumerate(msgs):
            for k in range(M):
                ref = sum(losses.worker_grad(loss, raw[p][0], raw[p][1], B[k], c) for p, c in m)
                # (<=: the one-row message has a zero squared-hinge gradient where its margin is above 1)
                assert np.max(np.abs(G[s, k, :d] - ref)) <= 1e-12 * np.max(np.abs(ref))
        assert np.all(G[:, :, d:] == 0.0)


# ---- 4. evaluation
def test_evaluation_shapes_files_best_and_headers(tmp_path):
    cfg, src, sch, parts = make(CASES["naive"], "GD", sweep_alpha=ALPHAS, sweep_lr=LRS)
    cfg.input_dir, cfg.verbose = str(tmp_path) + "/", True
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    lines = []
    res = tr.run(log=lines.append)
    ev = evaluate(tr, res, log=lines.append)
    for a in (ev.training_loss, ev.testing_loss, ev.auc):
        assert a.shape == (8, 3) and np.all(np.isfinite(a))
    assert ev.best == int(np.argmin(ev.testing_loss[-1]))
    heads = [i for i, ln in enumerate(lines) if ln.startswith(">> Model ")]
    assert [lines[i] for i in heads] == [">> Model %d: alpha = %g, lr = %g" % (k, ALPHAS[k], LRS[k]) for k in range(3)]
    for k, i in enumerate(heads):  # that model's usual iteration lines follow its header
        assert [ln.split(":")[0] for ln in lines[i + 1: i + 9]] == ["Iteration %d" % r for r in range(8)]
        assert ("Test Loss = %5.3f" % ev.testing_loss[0, k]) in lines[i + 1]
    single = tr.scheme.output_names(cfg.fix_quirks)
    assert set(ev.files) == {f"sweep{k}_{key}" for k in range(3) for key in single}
    for k in range(3):
        for key, name in single.items():
            path = ev.files[f"sweep{k}_{key}"]
            assert os.path.basename(path) == f"sweep{k}_{name}" and os.path.exists(path)
    rep = tr.rank_report()
    assert (rep["models"], rep["sweep_alpha"], rep["sweep_lr"]) == (3, ALPHAS, LRS)
    # squared hinge: its prefix comes after the sweep prefix
    cfg, src, sch, parts = make(CASES["naive"], "GD", loss="squared_hinge", sweep_alpha=ALPHAS[:2], lr=0.1)
    cfg.input_dir = str(tmp_path) + "/"
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    ev = evaluate(tr, tr.run())
    assert os.path.basename(ev.files["sweep1_auc"]) == "sweep1_sqhinge_" + single["auc"]
    # a run without the flags reports nothing new
    tr1, _, e1 = run(CASES["naive"], "GD")
    assert "models" not in tr1.rank_report() and e1.best is None and e1.testing_loss.shape == (8,)


# ---- 5. rejections
def test_trainer_rejects_bf16_and_sparse_sources():
    import scipy.sparse as sps

    cfg, src, sch, parts = make(CASES["naive"], precision="bf16", sweep_alpha=ALPHAS)
    with pytest.raises(ValueError, match="bf16"):
        Trainer(cfg, DistEnv(), src, scheme=sch)
    cfg, src, sch, parts = make(CASES["naive"], sweep_alpha=ALPHAS)
    sparse = ArraySource([(sps.csr_matrix(X), y) for X, y in parts], (sps.csr_matrix(src._test[0]), src._test[1]),
                         sparse=True)
    with pytest.raises(ValueError, match="sparse"):
        Trainer(cfg, DistEnv(), sparse, scheme=sch)
    prec = get_precision("fp64")
    with pytest.raises(ValueError, match="1024"):
        MultiModelGradPlan.check_supported(prec, losses.LOGISTIC, 3, False, 1026, gpu=True)
    MultiModelGradPlan.check_supported(prec, losses.LOGISTIC, 3, False, 1026, gpu=False)  # the CPU path: any width
    for bad in (1, 9):
        with pytest.raises(ValueError, match="2..8"):
            MultiModelGradPlan.check_supported(prec, losses.LOGISTIC, bad)
    with pytest.raises(ValueError, match="softmax"):
        MultiModelGradPlan.check_supported(prec, losses.SOFTMAX, 3)


# ---- 6. checkpoint and resume
def test_resume_continues_the_trajectory_and_refuses_other_lists(tmp_path):
    ck = str(tmp_path / "ck.pt")
    _, full, _ = run(CASES["cyclic"], "AGD", sweep_alpha=ALPHAS, sweep_lr=LRS)
    run(CASES["cyclic"], "AGD", sweep_alpha=ALPHAS, sweep_lr=LRS, rounds=4, checkpoint_every=4, checkpoint_path=ck)
    _, resumed, _ = run(CASES["cyclic"], "AGD", sweep_alpha=ALPHAS, sweep_lr=LRS, resume=ck)
    np.testing.assert_allclose(resumed.betaset, full.betaset, **TOL)
    with pytest.raises(ValueError, match="sweep"):
        run(CASES["cyclic"], "AGD", sweep_alpha=ALPHAS, sweep_lr=[1.0, 1.0, 2.0], resume=ck)
    with pytest.raises(ValueError):
        run(CASES["cyclic"], "AGD", resume=ck)  # a single-model run cannot continue a sweep


# ---- 7. three gloo ranks
def test_three_gloo_ranks_match_the_replay(tmp_path):
    out = str(tmp_path / "multimodel_gloo.npz")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]),
               EH_MULTIMODEL_OUT=out, EH_MULTIMODEL_DEVICE="cpu")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr",
           "127.0.0.1", f"--master-port={port}", os.path.join(HERE, "mp_multimodel_run.py")]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    check_against_replay(np.load(out, allow_pickle=True))


def check_against_replay(z):
    """The saved sweep run of tests/mp_multimodel_run.py against tests/oracle.py's replay, once per model."""
    cfg, src, sch, parts = make(CASES["agc_uneven"], "AGD", sweep_alpha=ALPHAS, sweep_lr=LRS)
    d_x, ld_x = 33, 34
    arrivals = [[tuple(a) for a in rnd] for rnd in z["arrivals"]]
    got = np.asarray(z["betaset"]).reshape(-1, 3, ld_x)
    assert np.all(got[:, :, d_x:] == 0.0)
    beta0 = np.asarray(z["beta0"]).reshape(3, ld_x)[:, :d_x]
    etas = cfg.sweep_etas()
    for k in range(3):
        ref = replay(sch, parts, beta0[k], arrivals, "AGD", ALPHAS[k], cfg.n_rows, etas[k])
        np.testing.assert_allclose(got[:, k, :d_x], ref, **TOL)
