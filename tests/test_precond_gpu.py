"""--precondition diag on the GPU: grad_curv and combine_update_precond against long-double references, the engine
against its CPU run.  Block 0 of a message (the gradient) is held to tests/numerics.py oracle_message with the project's
K.  Block 1 (h_j = sum w_i x_ij^2) is held per column to a bound built the same way,
    K_CURV u sum_p |c_p| sum_i (w_i + L sum_k |x_ik beta_k|) x_ij^2  +  tiny sum_p |c_p| sum_i x_ij^2,
L the curvature's Lipschitz constant in z: 1 / (6 sqrt 3) logistic, 0 least squares; squared hinge is piecewise
constant, and the oracle asserts on the long-double z that no row lies within K u sum_k |x_ik beta_k| of its jump at
y z = 1 (no row is excluded).  K_CURV by the rule at the top of tests/numerics.py: PrecondGradPlan on CPU tensors
reaches at most MEASURED_CURV_CPU_RATIO over GRID and both message sets (least squares has L = 0, so its bound is the
bare accumulation term; the gradient's ratio there is 0.71).  hostile_partition keeps |x| below 50: x^2 is finite."""
import numpy as np
import pytest
import torch
from scipy.special import expit

from erasurehead_amd.engine import Trainer
from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.precond import PrecondGradPlan
from erasurehead_amd.ops.update import combine_update_precond
from erasurehead_amd.parallel.dist import DistEnv
import block_edge_cases as bc
import numerics as nx
from numerics import LD, LEAST_SQUARES, LOGISTIC, LOSS_IDS, LOSSES, SQUARED_HINGE
from test_multimodel_cpu import CASES, TOL, arrival_sets, make

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEASURED_CURV_CPU_RATIO = 3.31  # d = 37, least squares, fp32x64, coded message 0 (3.305)
K_CURV = 32  # 8 x MEASURED_CURV_CPU_RATIO, rounded up to a power of two
WIDTHS = (1, 37, 256, 257, 512, 513, 1000, 1024)
GRID = [(d, l, p) for d in (37, 1000) for l in LOSSES for p in bc.SCALAR_PRECS] + \
       [(d, LOGISTIC, p) for d in WIDTHS if d not in (37, 1000) for p in ("fp64", "fp32")]
_dev_parts = {}


def curv_oracle(loss, segments, host, bh, prec, k=K_CURV):
    """(h [d], per-column bound [d]) of block 1 of one message in long double; asserts the squared-hinge margin."""
    d = len(bh)
    h, acc, tiny = np.zeros(d, LD), np.zeros(d, LD), np.zeros(d, LD)
    for p, coef in segments:
        X, y, b = np.asarray(host[p][0], LD), np.asarray(host[p][1], LD), np.asarray(bh, LD)
        z, az = X @ b, np.abs(X) @ np.abs(b)
        if loss == LOGISTIC:
            s = expit(-(y * z))
            w, lip = s * (1 - s), LD(1) / (6 * np.sqrt(LD(3)))
        else:
            w, lip = (np.full_like(z, 2) if loss == LEAST_SQUARES else np.where(y * z < 1, LD(2), LD(0))), LD(0)
        if loss == SQUARED_HINGE:
            assert np.all(np.abs(1 - y * z) > nx.K * nx.acc_eps(prec) * az), "a row sits on the squared hinge's jump"
        h += LD(coef) * ((X * X).T @ w)
        acc += abs(coef) * ((X * X).T @ (w + lip * az))
        tiny += abs(coef) * (X * X).sum(0)
    return h, LD(k * nx.acc_eps(prec)) * acc + LD(nx.acc_tiny(prec)) * tiny


def check(G, msgs, host, bh, loss, prec, d, what):
    ld = prec.ld(d)
    got = G.double().cpu().numpy().reshape(len(msgs), 2, ld)
    for s, m in enumerate(msgs):
        nx.check_columns(got[s, 0, :d], *nx.oracle_message(loss, m, host, bh, prec), f"{what} message {s} gradient")
        nx.check_columns(got[s, 1, :d], *curv_oracle(loss, m, host, bh, prec), f"{what} message {s} curvature", K_CURV)
    assert np.all(got[:, :, d:] == 0.0), f"{what}: padding columns of both blocks must be exact zeros"


def inputs(d, prec_name):
    sizes, cpu_parts, host, betas = bc.scalar_inputs(d, prec_name, 2)
    if (d, prec_name) not in _dev_parts:
        _dev_parts[(d, prec_name)] = bc.to_device(cpu_parts, DEV)
    return sizes, _dev_parts[(d, prec_name)], host, betas


def model(beta_ld, prec):  # beta in block 0; block 1 is NaN: the kernel must not read it
    return torch.cat([beta_ld, torch.full_like(beta_ld, float("nan"))]).to(DEV)


@pytest.mark.parametrize("d,loss,prec_name", GRID, ids=[f"d{d}-{LOSS_IDS[l]}-{p}" for d, l, p in GRID])
def test_kernel_within_the_column_bounds(d, loss, prec_name, native, monkeypatch):
    prec = get_precision(prec_name)
    sizes, parts, host, betas = inputs(d, prec_name)
    beta, bh = model(betas[0][0], prec), betas[0][1]
    for rows in bc.TASK_ROWS:
        bc.forced_task_rows(monkeypatch, rows)
        for kind in ("naive", "coded"):
            msgs = bc.MESSAGES[kind](len(sizes))
            plan = PrecondGradPlan(msgs, parts, prec, loss, d)
            assert plan.identity == (kind == "naive")
            bc.assert_tasks_reach_the_edges(plan, sizes, bc.geometry(prec, d, 2)[0], rows)
            G = plan.run(beta, plan.out_buffer()[0].fill_(float("nan")))
            G2 = plan.out_buffer()[0].fill_(float("nan"))
            plan.native_launcher().launch(beta, G2)
            torch.cuda.synchronize()
            check(G, msgs, host, bh, loss, prec, d, f"{kind} tasks of {rows}")
            assert torch.equal(G, G2)  # two launches: bitwise identical


def test_least_squares_curvature_ignores_beta_and_logistic_at_zero_is_a_quarter(native):
    prec = get_precision("fp64")
    sizes, parts, host, betas = inputs(37, "fp64")
    msgs, ld = bc.coded_messages(len(sizes)), prec.ld(37)
    plan = PrecondGradPlan(msgs, parts, prec, LEAST_SQUARES, 37)
    Ga = plan.run(model(betas[0][0], prec), plan.out_buffer()[0]).clone()
    Gb = plan.run(model(betas[1][0], prec), plan.out_buffer()[0])
    assert torch.equal(Ga.reshape(-1, 2, ld)[:, 1], Gb.reshape(-1, 2, ld)[:, 1]) and not torch.equal(Ga, Gb)
    plan = PrecondGradPlan(msgs, parts, prec, LOGISTIC, 37)
    G = plan.run(torch.zeros(2 * ld, dtype=prec.acc, device=DEV), plan.out_buffer()[0]).cpu().numpy().reshape(-1, 2, ld)
    for s, m in enumerate(msgs):
        quarter = sum(LD(c) * (np.asarray(host[p][0], LD) ** 2).sum(0) for p, c in m) / 4
        bound = curv_oracle(LOGISTIC, m, host, np.zeros(37), prec)[1]
        nx.check_columns(G[s, 1, :37], quarter, bound, f"message {s}", K_CURV)


@pytest.mark.parametrize("kw", [{}, dict(loss=2), dict(dtype=1, ld_x=40), dict(dtype=3, ld_x=40), dict(d_x=1024, ld_x=1024),
                                dict(ld_x=0, d_x=0), dict(ld_x=1026, d_x=1000), dict(d_x=0), dict(d_x=39), dict(ld_x=37, d_x=37),
                                dict(dtype=1, ld_x=38), dict(dtype=2, ld_x=40), dict(dtype=4), dict(loss=3), dict(loss=4),
                                dict(loss=5), dict(loss=-1)], ids=str)
def test_launcher_validates_its_arguments(kw, native):
    """grad_curv_launch over empty tables: the first five argument sets are valid, every other one is an error (odd
    widths, bf16, unknown storage, softmax and the weighted loss codes), not a launch."""
    i32 = dict(dtype=torch.int32, device=DEV)
    buf, a = torch.zeros(2 * 1024, dtype=torch.float64, device=DEV), dict(dict(dtype=0, loss=0, d_x=37, ld_x=38), **kw)
    args = (a["dtype"], a["loss"], torch.zeros(32, dtype=torch.uint8, device=DEV), torch.zeros((0, 5), **i32),
            torch.zeros(1, **i32), buf, buf, buf, a["d_x"], a["ld_x"])
    if kw in ({}, dict(loss=2), dict(dtype=1, ld_x=40), dict(dtype=3, ld_x=40), dict(d_x=1024, ld_x=1024)):
        native._grad_curv_raw(*args)
    else:
        with pytest.raises(RuntimeError, match="invalid"):
            native._grad_curv_raw(*args)


@pytest.mark.parametrize("mdt", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("rule", [0, 1], ids=["GD", "AGD"])
@pytest.mark.parametrize("nmsg", [1, 2, 8, 9, 128])
def test_update_kernel_against_long_double(nmsg, rule, mdt, native):
    assert native.MAX_MSGS == 128
    rng = np.random.RandomState(nmsg)
    d, ld, eta, gs, l2c, damp, theta = 301, 302, 0.8, 1.25 / 40, 2e-2, 1e-3, 0.4
    M = np.zeros((nmsg, 2, ld))
    M[:, 0, :d], M[:, 1, :d] = rng.randn(nmsg, d), rng.uniform(0.5, 2.0, (nmsg, d))
    coefs = rng.uniform(0.5, 1.5, nmsg) * np.where(np.arange(nmsg) % 3 == 1, -0.05, 1.0)
    M[0, 1, 0] = -1e3  # the decoded curvature of column 0 is negative: the clamp
    msgs = [torch.from_numpy(m.ravel()).to(mdt).to(DEV) for m in M]
    Mh = np.stack([m.double().cpu().numpy() for m in msgs]).reshape(nmsg, 2, ld).astype(LD)
    b0, u0 = np.pad(rng.randn(d), (0, 2 * ld - d)), np.pad(rng.randn(d), (0, 2 * ld - d))
    beta, u = torch.from_numpy(b0).to(DEV), torch.from_numpy(u0).to(DEV)
    hist = torch.full((2 * ld,), float("nan"), dtype=torch.float64, device=DEV)
    bw = torch.full((2 * ld,), float("nan"), dtype=torch.float32, device=DEV)
    combine_update_precond(msgs, coefs, beta, u, ld, d, eta, gs, l2c, damp, theta, rule, hist=hist, beta_w=bw)
    torch.cuda.synchronize()
    c, b, uu = coefs.astype(LD)[:, None], b0[:d].astype(LD), u0[:d].astype(LD)
    g, h = (c * Mh[:, 0, :d]).sum(0), (c * Mh[:, 1, :d]).sum(0)
    assert h[0] < 0 < h[1:].min()
    P = gs * np.maximum(h, 0) + l2c + damp
    step = eta * (gs * g + l2c * b) / P
    nb = b - step if rule == 0 else (1 - theta) * b + theta * uu - step
    # each decoded sum carries (nmsg + 1) u sum |c v| through the step; a few more roundings in the update itself
    e, eps = np.abs(c)[:, :, None] * np.abs(Mh[:, :, :d]), LD(2.0 ** -52)
    err = eps * ((nmsg + 1) * gs * (eta * e[:, 0].sum(0) + np.abs(step) * e[:, 1].sum(0)) / P
                 + 8 * (np.abs(step) + np.abs(b) + np.abs(uu)))
    assert np.all(np.abs(beta.cpu().numpy()[:d] - nb) <= err)
    if rule == 1:
        eu = (err + 4 * eps * (np.abs(nb) + np.abs(b))) / theta
        assert np.all(np.abs(u.cpu().numpy()[:d] - (b + (nb - b) / theta)) <= eu)
    assert torch.equal(hist[:d], beta[:d]) and torch.equal(bw[:d], beta[:d].float())
    assert torch.all(hist[ld:] == 0) and torch.all(bw[d:] == 0) and torch.all(beta[d:] == 0) and torch.all(u[d:] == 0)
    for bad in (0.0, -1.0, float("nan")):  # the launcher's own rejection, past the Python wrapper's
        with pytest.raises(RuntimeError, match="invalid"):
            native.combine_update_precond(msgs, list(coefs), beta, u, hist, bw, ld, d, eta, gs, l2c, bad, theta, rule)


@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", ["naive", "agc_uneven"])
def test_gpu_engine_matches_the_cpu_engine(name, rule, native):
    kw = dict(precondition="diag", precondition_damping=1e-6, lr=0.7)
    cfg, src, sch, _ = make(CASES[name], rule, **kw)
    cfg.device_loop = "stream"
    tg = Trainer(cfg, DistEnv(device=torch.device(DEV)), src, scheme=sch)
    rg = tg.run()
    cfg, src, sch, _ = make(CASES[name], rule, **kw)
    rc = Trainer(cfg, DistEnv(), src, scheme=sch).run()
    np.testing.assert_allclose(rg.betaset, rc.betaset, **TOL)
    assert arrival_sets(rg) == arrival_sets(rc) and isinstance(tg.plan, PrecondGradPlan)
    assert tg.rank_report()["precondition"] == "diag" and tg.rank_report()["round_loop"] == "stream"
