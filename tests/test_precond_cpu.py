"""--precondition diag on the CPU: rejections, the torch plan and the update against the NumPy oracles, engine runs
against a replay of their rounds, and one identity: ONE round solves least squares on orthogonal columns."""
import numpy as np
import pytest
import torch

from erasurehead_amd.codes.schemes import Arrival
from erasurehead_amd.config import RunConfig
from erasurehead_amd.data.source import ArraySource
from erasurehead_amd.engine import Trainer, evaluate
from erasurehead_amd.models import losses
from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.precond import PrecondGradPlan
from erasurehead_amd.ops.update import combine_update_precond
from erasurehead_amd.parallel.dist import DistEnv
from test_multimodel_cpu import CASES, TOL, make

BASE = dict(n_procs=5, n_rows=400, n_cols=20, input_dir="/tmp/x", precondition="diag")
FP64 = get_precision("fp64")


@pytest.mark.parametrize("kwargs,pattern", [
    (dict(loss="softmax"), "--precondition.*softmax"), (dict(ovr=3), "--precondition.*--ovr"),
    (dict(cv=4), "--precondition.*--cv"), (dict(sweep_alpha=[1e-3, 1e-2]), "--precondition.*sweep"),
    (dict(sweep_lr=[1.0, 2.0]), "--precondition.*sweep"), (dict(sweep_l1=[0.0, 0.1]), "--precondition.*sweep"),
    (dict(l1=0.1), "--precondition.*--l1"), (dict(class_weight="balanced"), "--precondition.*--class-weight"),
    (dict(sample_weights="w.dat"), "--precondition.*--sample-w"), (dict(precision="bf16"), "--precondition.*bf16"),
    (dict(is_real=1, dataset="covtype"), "--precondition.*sparse"), (dict(precondition="full"), "--precondition"),
    (dict(precondition_damping=0.0), "--precondition-damping"), (dict(precondition_damping=-1.0), "-damping"),
    (dict(precondition_damping=float("nan")), "-damping"), (dict(precondition_damping=float("inf")), "-damping")])
def test_rejections_name_the_flag(kwargs, pattern):
    with pytest.raises(ValueError, match=pattern):
        RunConfig(**{**BASE, **kwargs})


def test_width_limit_holds_on_a_gpu_only():
    with pytest.raises(ValueError, match="--precondition.*1024"):
        PrecondGradPlan.check_supported(FP64, losses.LOGISTIC, False, 1026, gpu=True)
    PrecondGradPlan.check_supported(FP64, losses.LOGISTIC, False, 1026, gpu=False)  # the CPU path: any width


@pytest.mark.parametrize("loss", [losses.LOGISTIC, losses.LEAST_SQUARES, losses.SQUARED_HINGE])
def test_torch_plan_is_the_numpy_oracle(loss):
    rng = np.random.RandomState(loss)
    d, ld = 33, FP64.ld(33)
    host = {p: (rng.randn(n, d) * 0.3, rng.choice([-1.0, 1.0], n)) for p, n in enumerate([7, 1, 12])}
    parts = {p: (torch.from_numpy(np.pad(X, ((0, 0), (0, ld - d)))), torch.from_numpy(y)) for p, (X, y) in host.items()}
    msgs = [[(0, 1.0), (2, -0.5)], [(1, 2.0)]]
    beta = torch.zeros(2 * ld, dtype=torch.float64)
    beta[:d] = torch.from_numpy(rng.randn(d))
    beta[ld:] = 7.0  # block 1 of the model is not read
    plan = PrecondGradPlan(msgs, parts, FP64, loss, d)
    G = plan.run(beta, plan.out_buffer()[0]).numpy().reshape(2, 2, ld)
    for s, m in enumerate(msgs):
        ref = sum(losses.precond_grad(loss, *host[p], beta[:d].numpy(), c) for p, c in m)
        np.testing.assert_allclose(G[s, :, :d], ref, rtol=1e-12, atol=1e-13)
    assert np.all(G[:, :, d:] == 0.0)


@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_update_is_step_precond_and_clamps_negative_curvature(rule):
    rng = np.random.RandomState(1)
    d, ld = 5, 6
    msgs = [torch.from_numpy(np.pad(np.stack([rng.randn(d), rng.uniform(0.5, 2.0, d)]), ((0, 0), (0, 1))).ravel())
            for _ in range(3)]
    coefs = [1.5, -0.25, 0.75]  # both signs: the decoded curvature of column 0 is made negative below
    msgs[1][ld] = 50.0
    h = sum(c * m[ld: ld + d].numpy() for c, m in zip(coefs, msgs))
    assert h[0] < 0 < h[1:].min()
    up = losses.UpdateRule(rule, 1e-2, 40, 1.25)
    beta, u = torch.zeros(2 * ld, dtype=torch.float64), torch.zeros(2 * ld, dtype=torch.float64)
    beta[:d], u[:d] = torch.from_numpy(rng.randn(d)), torch.from_numpy(rng.randn(d))
    rb, ru = beta[:d].numpy().copy(), u[:d].numpy().copy()
    hist, bw = torch.full((2 * ld,), np.nan, dtype=torch.float64), torch.full((2 * ld,), np.nan, dtype=torch.float32)
    eta, gs, l2c, theta, code = up.precond_coeffs(3, 0.8)
    combine_update_precond(msgs, coefs, beta, u, ld, d, eta, gs, l2c, 1e-3, theta, code, hist=hist, beta_w=bw)
    up.step_precond(3, 0.8, rb, ru, sum(c * m[:d].numpy() for c, m in zip(coefs, msgs)), h, 1e-3)
    np.testing.assert_allclose(torch.stack([beta[:d], u[:d]]).numpy(), np.stack([rb, ru]), rtol=1e-13)
    assert torch.equal(hist[:d], beta[:d]) and torch.all(hist[ld:] == 0) and torch.all(beta[d:] == 0)
    assert torch.equal(bw[:d], beta[:d].float()) and torch.all(bw[d:] == 0)
    with pytest.raises(ValueError, match="damping"):
        combine_update_precond(msgs, coefs, beta, u, ld, d, eta, gs, l2c, 0.0, theta, code)


def replay(sch, parts, beta0, arrivals_log, rule, cfg, loss, damping):
    """The rounds of a run in NumPy: decode, sum the used messages' [g ; h], UpdateRule.step_precond."""
    up = losses.UpdateRule("AGD" if sch.fixed_agd else rule, cfg.alpha_value, cfg.n_rows, sch.grad_scale())
    beta, u, out = np.array(beta0), np.zeros_like(beta0), []
    for i, arr in enumerate(arrivals_log):
        gh = np.zeros((2, len(beta)))
        for (w, part), c in sch.decode([Arrival(*a) for a in arr]).items():
            m = [x for x in sch.messages if x.worker == w and x.part == part][0]
            gh += c * sum(losses.precond_grad(loss, *parts[p], beta, coef) for p, coef in m.segments)
        up.step_precond(i, cfg.eta()[i], beta, u, gh[0], gh[1], damping)
        out.append(beta.copy())
    return np.array(out)


@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("case,loss", [("naive", "logistic"), ("cyclic", "squared_hinge"), ("agc_uneven", "logistic")])
def test_engine_follows_the_replay(case, loss, rule):
    cfg, src, sch, parts = make(CASES[case], rule, loss=loss, precondition="diag", precondition_damping=1e-6, lr=0.7)
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    res, (d, ld) = tr.run(), (33, 34)
    ev = evaluate(tr, res, write=False)
    assert res.betaset.shape == (cfg.num_itrs, 2 * ld) and np.all(res.betaset[:, ld:] == 0.0)
    got = losses.precond_unpack(res.betaset, d)
    ref = replay(sch, parts, tr.beta0[:d], res.arrivals, rule, cfg, losses.LOSS_NAMES[loss], 1e-6)
    np.testing.assert_allclose(got, ref, **TOL)
    assert tr.rank_report()["damping"] == 1e-6 and ev.training_loss.shape == (cfg.num_itrs,)


def test_one_round_solves_least_squares_on_orthogonal_columns():
    """X = Q diag(s), Q orthonormal: the Hessian (2/n) diag(s^2) is diagonal, so with alpha = 0 and lr = 1 one GD round
    lands on beta* = Q^T y / s up to (beta_0 - beta*) delta / P_j and the rounding of the sums; plain GD cannot."""
    n, d, W, delta = 64, 8, 4, 1e-30
    rng = np.random.RandomState(5)
    s = 10.0 ** np.linspace(-3, 3, d)
    Q = np.linalg.qr(rng.randn(n, d))[0]
    X, y = Q * s, rng.randn(n)
    parts = [(X[k::W], y[k::W]) for k in range(W)]

    def run(**kw):
        cfg = RunConfig(W + 1, n, d, "/tmp/eh_cpu_precond/", 0, "x", 0, 0, 0, 0, 0, 0, "GD", num_itrs=1, seed=0,
                        verbose=False, loss="least_squares", alpha=0.0, **kw)
        tr = Trainer(cfg, DistEnv(), ArraySource(parts, parts[0]))
        got = tr.run().betaset[0]
        return tr.beta0[:d], got

    b0, got = run(lr=1.0, precondition="diag", precondition_damping=delta)
    star = Q.T @ y / s
    u = 2.0 ** -52
    r = np.abs(2 * (y - X @ b0)) + 2 * (np.abs(X) @ np.abs(b0))  # |r_i| and the error its dot product carries
    P = 2 * (X * X).sum(0) / n + delta
    err_g = (n + d + 4) * u * (np.abs(X).T @ r) / n  # of gs g_j, summed in any order
    bound = np.abs(b0 - star) * delta / P.min() + err_g / P + (n + 8) * u * (2 * np.abs(b0) + 2 * np.abs(star))
    assert np.all(np.abs(got[:d] - star) <= bound), (np.abs(got[:d] - star) / bound).max()
    _, plain = run(lr=n / (2 * s.max() ** 2))  # the largest column's exact step: the others hardly move
    assert np.abs(plain[:d] - star).max() > 1e6 * bound.max()
