"""--newton-cg J on the CPU: the oracle UpdateRule.step_newton on a problem CG solves exactly, the engine (Python round
loop, NumPy twin of newton_cg_update) against a replay through that oracle, the flags' rejections, checkpoint and
resume."""
import numpy as np
import pytest
import torch

from erasurehead_amd import cli
from erasurehead_amd.engine import Trainer
from erasurehead_amd.models import losses
from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.hvp import HvpGradPlan
from erasurehead_amd.parallel.dist import DistEnv
from test_multimodel_cpu import ARGV, CASES, make


def test_least_squares_is_solved_in_one_outer_iteration():
    """CG is exact on a quadratic after d steps: with J >= d = 6 and a tiny tolerance one outer iteration (a gradient
    round and at most 6 CG rounds) reaches the normal-equation solution."""
    rng = np.random.RandomState(0)
    n, d, alpha = 40, 6, 1e-2
    X, y = rng.randn(n, d), rng.randn(n)
    rule, state, beta = losses.UpdateRule("GD", alpha, n), losses.NewtonState(), rng.randn(d)
    rounds = 0
    while state.outer == 0:
        v = state.direction if state.phase == 1 else np.zeros(d)
        g, u = losses.hvp_grad(losses.LEAST_SQUARES, X, y, beta, v)
        rule.step_newton(rounds, 0.1, beta, g, u, state, 8, 1e-12, 1.0)
        rounds += 1
    # (1/n) |y - X b|^2 + alpha |b|^2
    want = np.linalg.solve(X.T @ X / n + alpha * np.eye(d), X.T @ y / n)
    assert rounds <= 1 + d and losses.NEWTON_MODES[state.mode].startswith("step")
    assert np.abs(beta - want).max() <= 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("name,kw", [("naive", {}), ("frc", {}), ("naive", dict(d=5, loss="least_squares"))])
def test_engine_against_a_replay_through_the_oracle(name, kw):
    cfg, src, sch, parts = make(CASES[name], newton_cg=3, newton_tol=1e-3, rounds=12, **dict(dict(lr=2.0), **kw))
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    res = tr.run()
    assert isinstance(tr.plan, HvpGradPlan) and res.betaset.shape == (12, 2 * tr.ld_x)
    rule, eta, state = losses.UpdateRule("GD", cfg.alpha_value, cfg.n_rows), cfg.eta(), losses.NewtonState()
    beta, want, d = tr.model.beta0(sch.init_zero, cfg.seed)[: cfg.n_cols].copy(), [], cfg.n_cols
    for i in range(cfg.num_itrs):
        v = state.direction if state.phase == 1 else np.zeros(d)
        g, u = sum(losses.hvp_grad(tr.model.loss, X, y, beta, v) for X, y in parts)
        rule.step_newton(i, float(eta[i]), beta, g, u, state, cfg.newton_cg, cfg.newton_tol, cfg.newton_step)
        want.append(beta.copy())
    np.testing.assert_allclose(losses.newton_unpack(res.betaset, d), want, rtol=1e-9, atol=1e-11)
    assert np.all(res.betaset[:, tr.ld_x:] == 0)  # block 1 of every stored iterate
    assert state.outer >= 2 and tr.newton_state[2].tolist() == [state.phase, state.inner, state.mode, state.outer]
    rep = tr.rank_report()
    assert (rep["newton_cg"], rep["newton_tol"], rep["newton_step"]) == (3, 1e-3, 1.0)
    assert all(v.startswith("newton_") for v in tr.model.result_names({"a": "x.dat"}).values())


def test_checkpoint_and_resume_continue_the_trajectory(tmp_path):
    """The checkpoint falls inside an outer iteration (round 5 of J = 3: a CG round is next), so the resumed run needs
    the direction on the wire and the CG state."""
    path, kw = str(tmp_path / "ck.pt"), dict(newton_cg=3, newton_tol=1e-6, lr=2.0)
    cfg, src, sch, _ = make(CASES["naive"], rounds=12, **kw)
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    full = tr.run().betaset
    np.testing.assert_array_equal(tr.run().betaset, full)  # a second run starts with a gradient round
    cfg, src, sch, _ = make(CASES["naive"], checkpoint_every=6, checkpoint_path=path, rounds=6, **kw)
    Trainer(cfg, DistEnv(), src, scheme=sch).run()
    st = torch.load(path, weights_only=True)
    assert (st["newton_cg"], st["newton_tol"], st["newton_step"]) == (3, 1e-6, 1.0) and st["newton_phase"][0] == 1
    cfg, src, sch, _ = make(CASES["naive"], rounds=12, resume=path, **kw)
    np.testing.assert_array_equal(Trainer(cfg, DistEnv(), src, scheme=sch).run().betaset, full)
    for other in (dict(newton_cg=4, newton_tol=1e-6), dict(newton_cg=3, newton_tol=1e-6, newton_step=0.5), {}):
        cfg, src, sch, _ = make(CASES["naive"], rounds=12, lr=2.0, resume=path, **other)
        with pytest.raises(ValueError, match="--newton-cg"):
            Trainer(cfg, DistEnv(), src, scheme=sch).run()


@pytest.mark.parametrize("flags", [
    "--newton-cg 33", "--newton-cg -1", "--newton-tol 0 --newton-cg 3", "--newton-tol nan --newton-cg 3",
    "--newton-step 0 --newton-cg 3", "--newton-step inf --newton-cg 3", "--newton-tol 0.5", "--newton-tol 0.1",
    "--newton-step 0.5", "--newton-step 1", "--newton-cg 3 --loss softmax", "--newton-cg 3 --ovr 3", "--newton-cg 3 --cv 2",
    "--newton-cg 3 --alphas 1e-3,1e-2", "--newton-cg 3 --lrs 1,2", "--newton-cg 3 --l1s 0,1e-3", "--newton-cg 3 --l1 1e-3",
    "--newton-cg 3 --precondition diag", "--newton-cg 3 --lbfgs 3", "--newton-cg 3 --class-weight balanced",
    "--newton-cg 3 --sample-weights w.npy"])
def test_rejections_name_the_flag(flags):
    with pytest.raises(ValueError, match=flags.split()[0] + r"\b(?!-)"):
        cli.parse(ARGV + flags.split())


def test_flags_parse_and_agd_bf16_sparse_are_rejected():
    cfg = cli.parse(ARGV + ["--newton-cg", "5", "--newton-tol", "0.01", "--newton-step", "0.5"])[0]
    assert (cfg.newton_cg, cfg.newton_tol, cfg.newton_step) == (5, 0.01, 0.5)
    cfg = cli.parse(ARGV)[0]
    assert (cfg.newton_cg, cfg.newton_tol, cfg.newton_step) == (0, 0.1, 1.0)
    with pytest.raises(ValueError, match="--newton-cg"):
        cli.parse(ARGV[:-1] + ["AGD", "--newton-cg", "3"])
    cfg, src, sch, _ = make((1, 0, 2, 7, 2, 0), newton_cg=3)  # avoidstragg: always AGD
    with pytest.raises(ValueError, match="--newton-cg"):
        Trainer(cfg, DistEnv(), src, scheme=sch)
    cfg, src, sch, _ = make(CASES["naive"], newton_cg=3, precision="bf16")
    with pytest.raises(ValueError, match="--newton-cg.*bf16"):
        Trainer(cfg, DistEnv(), src, scheme=sch)
    with pytest.raises(ValueError, match="--newton-cg.*sparse"):
        HvpGradPlan.check_supported(get_precision("fp64"), losses.LOGISTIC, sparse=True)
