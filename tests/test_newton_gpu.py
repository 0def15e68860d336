"""--newton-cg J on the GPU: grad_hvp against a long-double oracle, newton_cg_update against UpdateRule.step_newton in
fp64 NumPy over a script of rounds that visits every branch, the launchers' rejections, the engine against its CPU run.

Block 0 of a message (the gradient) is held to tests/numerics.py oracle_message with the project's K.  Block 1
(u_j = sum_p c_p sum_i w_i q_i x_ij, q = x . v) is held per column to
    K_HVP u sum_p |c_p| sum_i (|w_i q_i| + w_i sum_k |x_ik v_k| + L |q_i| sum_k |x_ik beta_k|) |x_ij| + tiny sum_p |c_p| sum_i |x_ij|:
the accumulation of X^T (w q), then the error of the dot product q carried through w, then that of z carried through
the curvature (L its Lipschitz constant in z: 1 / (6 sqrt 3) logistic, 0 least squares; squared hinge is piecewise
constant and the oracle asserts that no row lies within K u sum_k |x_ik beta_k| of its jump).  The oracle, hvp_oracle,
lives in tests/newton_edge_cases.py.  K_HVP below was measured on the kernel itself; the stage-edge tests of
tests/test_newton_edges_gpu.py hold block 1 to K_HVP_EDGE, which follows the rule at the top of tests/numerics.py (the
plain torch path on CPU tensors, times 8, rounded up to a power of two)."""
import numpy as np
import pytest
import torch

from erasurehead_amd.engine import Trainer
from erasurehead_amd.models import losses
from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.hvp import HvpGradPlan
from erasurehead_amd.ops.update import newton_cg_update, newton_state
from erasurehead_amd.parallel.dist import DistEnv
import block_edge_cases as bc
import numerics as nx
from newton_edge_cases import hvp_oracle
from numerics import LD, LOSS_IDS, LOSSES
from test_lbfgs_cpu import check_step, rel
from test_multimodel_cpu import arrival_sets, make

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEASURED_HVP_RATIO = 0.53  # d = 300, least squares, fp32x64 (0.521); logistic stays below 0.16
K_HVP = 2  # 2 x MEASURED_HVP_RATIO, rounded up to a power of two
MEASURED_STEP_REL = 39.1  # in 2^-52: the worst max|x - ref| / max|ref| of a vector after a round (ld = 6, one fp64 message)
STEP_REL = 128 * 2.0 ** -52  # 2 x MEASURED_STEP_REL, rounded up to a power of two
SIZES = (1, 5, 70)  # waves without rows, a ragged stage, more than one stage at d = 1000
MESSAGES = {"naive": [[(p, 1.0)] for p in range(3)],
            "coded": [[(0, 1.0), (2, -0.7)], [(1, 2.5)], [(2, 1.5), (0, 0.3), (1, -1.25)]]}
_inputs = {}


def inputs(d, prec_name):
    """Partitions of SIZES rows on the device, their host views, a hostile beta and a v of mixed magnitudes: drawn
    once per (d, precision) and never changed."""
    if (d, prec_name) not in _inputs:
        prec, rng = get_precision(prec_name), np.random.RandomState(7000 + d)
        parts, host = {}, {}
        for p, n in enumerate(SIZES):
            Xs, y, Xh = nx.hostile_partition(rng, n, d, prec)
            parts[p], host[p] = (Xs.to(DEV), y.to(DEV)), (Xh, y.double().numpy())
        beta, bh = nx.hostile_beta(rng, d, prec)
        v = torch.zeros_like(beta)
        v[:d] = torch.from_numpy(rng.randn(d) * 10.0 ** rng.uniform(-3.0, 1.0, d) / np.sqrt(d)).to(prec.acc)
        _inputs[(d, prec_name)] = (parts, host, beta, bh, v, v[:d].double().numpy())
    return _inputs[(d, prec_name)]


@pytest.mark.parametrize("prec_name", bc.SCALAR_PRECS)
@pytest.mark.parametrize("loss", LOSSES, ids=[LOSS_IDS[l] for l in LOSSES])
@pytest.mark.parametrize("d", [37, 300, 1000])
def test_kernel_within_the_column_bounds(d, loss, prec_name, native, monkeypatch):
    prec = get_precision(prec_name)
    parts, host, beta, bh, v, vh = inputs(d, prec_name)
    ld, S = prec.ld(d), native._blocks_geometry(prec.ld(d) * prec.storage_bytes, 2)[0]
    assert S == bc.geometry(prec, d, 2)[0] and (d < 1000 or 70 > 2 * S)
    bc.forced_task_rows(monkeypatch, bc.ODD_TASKS)  # the 70-row partition: a second task that starts at row 37
    worst = 0.0
    for kind, msgs in MESSAGES.items():
        plan = HvpGradPlan(msgs, parts, prec, loss, d)
        assert plan.identity == (kind == "naive") and any(t[1] % 2 for t in bc.task_bounds(plan))
        for direction, dh in ((v, vh), (torch.zeros_like(v), np.zeros(d))):
            model = torch.cat([beta, direction]).to(DEV)
            G = plan.run(model, plan.out_buffer()[0].fill_(float("nan")))
            G2 = plan.out_buffer()[0].fill_(float("nan"))
            plan.native_launcher().launch(model, G2)
            torch.cuda.synchronize()
            assert torch.equal(G, G2)  # two launches: bitwise identical
            got = G.double().cpu().numpy().reshape(len(msgs), 2, ld)
            assert np.all(got[:, :, d:] == 0.0), "padding columns of both blocks must be exact zeros"
            for s, m in enumerate(msgs):
                nx.check_columns(got[s, 0, :d], *nx.oracle_message(loss, m, host, bh, prec), f"{kind} message {s} gradient")
                if not dh.any():
                    assert np.all(got[s, 1] == 0.0), "v = 0 must give u exactly 0"
                    continue
                ref, bound = hvp_oracle(loss, m, host, bh, dh, prec, 1)
                worst = max(worst, nx.column_ratio(got[s, 1, :d], ref, bound))
                nx.check_columns(got[s, 1, :d], ref, K_HVP * bound, f"{kind} message {s} product", K_HVP)
    print(f"grad_hvp d={d} {LOSS_IDS[loss]} {prec_name}: worst err / (u sum) = {worst:.3f}")


@pytest.mark.parametrize("kw", [{}, dict(loss=2), dict(dtype=3, ld_x=40), dict(dtype=2, ld_x=40), dict(dtype=4), dict(loss=3),
                                dict(loss=4), dict(loss=5), dict(ld_x=1026, d_x=1000), dict(d_x=39)], ids=str)
def test_worker_launcher_validates_its_arguments(kw, native):
    """grad_hvp_launch over empty tables: the first three argument sets are valid, every other one (bf16, unknown
    storage, softmax and the weighted loss codes, a width past the limit) is an error, not a launch."""
    i32 = dict(dtype=torch.int32, device=DEV)
    buf, a = torch.zeros(2 * 1024, dtype=torch.float64, device=DEV), dict(dict(dtype=0, loss=0, d_x=37, ld_x=38), **kw)
    args = (a["dtype"], a["loss"], torch.zeros(32, dtype=torch.uint8, device=DEV), torch.zeros((0, 5), **i32),
            torch.zeros(1, **i32), buf, buf, buf, a["d_x"], a["ld_x"])
    if kw in ({}, dict(loss=2), dict(dtype=3, ld_x=40)):
        native._grad_hvp_raw(*args)
    else:
        with pytest.raises(RuntimeError, match="invalid"):
            native._grad_hvp_raw(*args)


# (xi, what is wrong with the round's messages, at which CG step): one outer iteration each
SCRIPT = [(1e-9, None, 0),     # the J cap: start, continue, continue, step-cap
          (0.9, None, 0),      # the tolerance: start, step-tolerance
          (1e-9, "neg", 0),    # kappa <= 0 on the first CG round: the GD step from G0
          (1e-9, "neg", 1),    # kappa <= 0 on a later one: the x held
          (1e-9, "nan", -1)]   # a NaN message in the gradient round: the GD step


@pytest.mark.parametrize("mdt", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("nmsg", [1, 8, 9])
@pytest.mark.parametrize("ld", [6, 257, 1024])
def test_update_kernel_follows_the_oracle_through_every_branch(ld, nmsg, mdt, native):
    """A diagonal quadratic (loss Hessian A in [1, 4], a new linear term every outer iteration, so the gradient stays
    O(1) and no error is measured against a vanishing one); the round's [g ; u] is split over nmsg coded messages."""
    rng = np.random.RandomState(ld + nmsg)
    d, J, tau = ld - 1, 3, 0.9
    A = rng.uniform(1.0, 4.0, d)
    rule = losses.UpdateRule("GD", 0.05, 10)
    want, ostate = rng.randn(d), losses.NewtonState()
    beta = torch.from_numpy(np.pad(want, (0, ld + 1))).to(DEV)
    state, scal, phase = newton_state(ld, DEV)
    hist = torch.full((2 * ld,), float("nan"), dtype=torch.float64, device=DEV)
    bw = torch.full((2 * ld,), float("nan"), dtype=mdt, device=DEV)
    coefs = rng.uniform(0.5, 1.5, nmsg) * np.where(np.arange(nmsg) % 3 == 1, -0.5, 1.0)
    share = rng.uniform(0.5, 1.5, nmsg)
    share /= coefs.dot(share)
    wire_eps = 0.0 if mdt == torch.float64 else 2.0 ** -24
    seen, worst, i = set(), 0.0, 0
    for xi, fault, at in SCRIPT:
        outer, c = ostate.outer, rng.randn(d)
        while ostate.outer == outer:
            v = ostate.direction if ostate.phase == 1 else np.zeros(d)
            sign = -1.0 if fault == "neg" and ostate.phase == 1 and ostate.inner == at else 1.0
            full = np.zeros((2, ld))
            full[0, :d], full[1, :d] = A * want - c, sign * A * v
            msgs = [torch.from_numpy(s * full.ravel()).to(mdt).to(DEV) for s in share]
            if fault == "nan":
                msgs[-1][d // 2] = float("nan")
            eta, gs, l2c = rule.newton_coeffs(i, 0.01)
            newton_cg_update(msgs, coefs, beta, state, scal, phase, ld, d, J, eta, gs, l2c, xi, tau, hist=hist, beta_w=bw)
            g, u = sum(k * m.double().cpu().numpy() for k, m in zip(coefs, msgs)).reshape(2, ld)[:, :d]
            seen.add(rule.step_newton(i, 0.01, want, g, u, ostate, J, xi, tau))
            assert phase.tolist() == [ostate.phase, ostate.inner, ostate.mode, ostate.outer], f"round {i}"
            b, h, w = beta.cpu().numpy(), hist.cpu().numpy(), bw.double().cpu().numpy()
            assert np.all(h[ld:] == 0) and np.all(b[d:] == 0) and np.all(w[d:ld] == 0) and np.all(w[ld + d:] == 0)
            for got, ref, eps in ((b[:d], want, 0.0), (h[:d], want, 0.0), (w[:d], want, wire_eps),
                                  (w[ld:ld + d], ostate.direction, wire_eps)):
                if fault == "nan":
                    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(want).sum() == 1
                    got, ref = np.nan_to_num(got), np.nan_to_num(ref)
                scale = max(np.abs(ref).max(), 1e-300)
                err = np.abs(got - ref).max() / scale
                worst = max(worst, err - eps)
                assert err <= STEP_REL + eps, f"round {i} mode {ostate.mode}: {err:.3e}"
            i += 1
    assert seen == set(range(7))
    print(f"newton_cg_update ld={ld} nmsg={nmsg}: worst relative error {worst / 2.0 ** -52:.2f} x 2^-52")


@pytest.mark.parametrize("kw", [dict(J=0), dict(J=33), dict(J=-1), dict(xi=0.0), dict(xi=float("nan")), dict(xi=float("inf")),
                                dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf"))], ids=str)
def test_update_launcher_rejects_invalid_arguments(kw, native):
    ld, d = 6, 5
    beta = torch.arange(2.0 * ld, dtype=torch.float64, device=DEV)
    t = newton_state(ld, DEV)
    a = dict(dict(J=3, xi=0.1, tau=1.0), **kw)
    with pytest.raises(RuntimeError, match="invalid"):
        native.newton_cg_update([torch.ones(2 * ld, dtype=torch.float64, device=DEV)], [1.0], beta, None, None, *t, ld, d,
                                a["J"], 0.1, 1.0, 0.0, a["xi"], a["tau"], None)
    torch.cuda.synchronize()
    assert torch.equal(beta.cpu(), torch.arange(2.0 * ld, dtype=torch.float64)) and all(not x.any() for x in t)


@pytest.mark.parametrize("name,case", [("naive", (0, 0, 0, 5, 0, 0)), ("agc", (1, 0, 3, 5, 1, 3))])
def test_gpu_engine_follows_the_cpu_engine(name, case, native):
    """Stream = graph, bitwise; within test_lbfgs_gpu.py's engine bound per round of the CPU run (the Python loop)."""
    kw, runs = dict(rows=50, d=20, rounds=12, newton_cg=4, lr=2.0), {}
    for loop in ("stream", "graph"):
        cfg, src, sch, _ = make(case, **kw)
        cfg.device_loop = loop
        tg = Trainer(cfg, DistEnv(device=torch.device(DEV)), src, scheme=sch)
        runs[loop] = tg.run()
        assert tg.rank_report()["round_loop"] == loop and tg.rank_report()["newton_cg"] == 4
        assert isinstance(tg.plan, HvpGradPlan) and int(tg.newton_state[2][3]) >= 2
    np.testing.assert_array_equal(runs["stream"].betaset, runs["graph"].betaset)
    cfg, src, sch, _ = make(case, **kw)
    rc = Trainer(cfg, DistEnv(), src, scheme=sch).run()
    assert arrival_sets(runs["stream"]) == arrival_sets(rc) and cfg.n_rows == 200
    per_round = 2 * check_step(None, 33, 3, 1)[1]
    for i, (got, ref) in enumerate(zip(runs["stream"].betaset, rc.betaset)):
        print(f"newton engine {name} round {i}: {rel(got, ref.astype(LD)):.3e} bound {(i + 1) * per_round:.3e}")
        assert rel(got, ref.astype(LD)) <= (i + 1) * per_round, f"round {i}"
