"""The fp32-storage, fp64-arithmetic precision ``fp32x64`` on the GPU: every dense-gradient family on hostile inputs
at its selector edges against the long-double oracle with the fp64 bound (K = 8, u = 2^-52, tests/numerics.py --
no constant of its own), proof that the accumulators are fp64, the launch equivalences, the evaluation GEMM at its
tile edges, and the engine against the CPU engine and over the IPC mailbox.  Case tables: tests/fp32x64_cases.py."""
import functools
import json

import numpy as np
import pytest
import torch

import dense_edge_cases as ec
import fp32x64_cases as fc
import numerics as nx
from erasurehead_amd.engine import Trainer, evaluate
from erasurehead_amd.ops import DenseGradPlan, get_precision, loss_sums, predictions
from erasurehead_amd.ops.eval import predictions_and_loss
from erasurehead_amd.ops.grad import KernelChoice
from erasurehead_amd.parallel.dist import DistEnv

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAME = "fp32x64"


# ---- 1. kernel conformance on hostile inputs -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_case(d, sizes):
    """Hostile partitions and beta, generated once per (width, row counts) and left unchanged."""
    prec = get_precision(NAME)
    rng = np.random.RandomState((7919 * d + 31 * sum(sizes) + prec.code) % 2 ** 31)
    parts, host = {}, {}
    for p, n in enumerate(sizes):
        X, y, Xh = nx.hostile_partition(rng, n, d, prec)
        assert X.dtype == torch.float32 and y.dtype == torch.float64
        parts[p] = (X, y)
        host[p] = (Xh, y.numpy())
    beta, bh = nx.hostile_beta(rng, d, prec)
    return prec, parts, host, beta, bh


@functools.lru_cache(maxsize=None)
def _oracle(d, sizes, loss, segments):
    prec, parts, host, beta, bh = _host_case(d, sizes)
    return nx.oracle_message(loss, segments, host, bh, prec)


def _run_case(case, native):
    prec, parts, host, beta_h, bh = _host_case(case.d, case.sizes)
    d, ld = case.d, prec.ld(case.d)
    msgs = ec.messages(case.replicas)
    dev = {p: (X.to(DEV), y.to(DEV)) for p, (X, y) in parts.items()}
    plan = DenseGradPlan(msgs, dev, prec, case.loss, d, choice=case.choice)
    if case.choice is not None:
        assert plan.choice == case.choice
    else:
        assert plan.choice == fc.default_choice(d, case.sizes, case.replicas)
    assert plan.cpl == fc.cpl_of(ld)
    beta = beta_h.to(DEV)
    out = []
    for how in ("run", "launcher", "run"):
        G = torch.full((len(msgs), ld), 7.0, dtype=torch.float64, device=DEV)
        if how == "run":
            plan.run(beta, G)
        else:
            plan.native_launcher().launch(beta, G)
        torch.cuda.synchronize()
        out.append(G)
    G = out[0]
    Gh = G.cpu().numpy()
    what = f"{case.id} [{plan.choice.label()}]"
    for s, m in enumerate(msgs):
        ref, bound = _oracle(d, case.sizes, case.loss, tuple(m))
        nx.check_columns(Gh[s, :d], ref, bound, f"{what} message {s}")
    assert torch.all(G[:, d:] == 0), "padding columns must be exactly zero"
    only_empty = [s for s, m in enumerate(msgs) if all(p == ec.EMPTY for p, _ in m)]
    assert only_empty and torch.all(G[only_empty] == 0), "a message of empty partitions must be exactly zero"
    assert torch.equal(out[0], out[1]), "plan.run and the native launcher differ"
    assert torch.equal(out[0], out[2]), "two launches differ"
    return plan


DEFAULT = fc.default_cases()
FORCED = fc.forced_cases()


@pytest.mark.parametrize("case", DEFAULT, ids=[c.id for c in DEFAULT])
def test_default_choice_at_every_width_edge(case, native):
    _run_case(case, native)


@pytest.mark.parametrize("case", FORCED, ids=[c.id for c in FORCED])
def test_forced_choice_at_its_narrowest_and_widest_row(case, native):
    plan = _run_case(case, native)
    if case.choice.kind == "wide" and case.replicas > 1:
        assert plan.cpl in (32, 256) and plan.choice.bundled


# ---- 2. the accumulators really are fp64 -----------------------------------------------------------
@pytest.mark.parametrize("replicas", [1, 3])
def test_the_same_rows_under_fp32_miss_the_fp64_bound(replicas, native):
    """d = 1000, n = 257: the stored fp32 rows run under ``fp32`` (fp32 beta, labels, accumulators, messages) must
    leave the fp64 bound in some column, and under ``fp32x64`` stay inside it in every column.  If the fp32 run
    stays inside, these inputs cannot tell the two apart and the conformance tests above prove nothing."""
    d, sizes = 1000, (257, 33, 16, 17, 15, 0)
    prec, parts, host, beta_h, bh = _host_case(d, sizes)
    p32 = get_precision("fp32")
    msgs = ec.messages(replicas)
    plans = {NAME: DenseGradPlan(msgs, {p: (X.to(DEV), y.to(DEV)) for p, (X, y) in parts.items()}, prec, nx.LOGISTIC, d),
             "fp32": DenseGradPlan(msgs, {p: (X.to(DEV), y.float().to(DEV)) for p, (X, y) in parts.items()}, p32,
                                   nx.LOGISTIC, d)}
    worst = {}
    for name, plan in plans.items():
        acc = plan.prec.acc
        G = torch.full((len(msgs), plan.ld), 7.0, dtype=acc, device=DEV)
        plan.run(beta_h.to(acc).to(DEV), G)
        torch.cuda.synchronize()
        Gh = G.double().cpu().numpy()
        worst[name] = max(nx.column_ratio(Gh[s, :d], *_oracle(d, sizes, nx.LOGISTIC, tuple(m))) for s, m in enumerate(msgs))
    print("largest error / fp64 bound:", worst)
    assert worst[NAME] <= 1.0
    assert worst["fp32"] > 1.0, "the inputs are too tame: fp32 accumulation stays within the fp64 bound"


# ---- 3. closed gate --------------------------------------------------------------------------------
@pytest.mark.parametrize("d,replicas,choice", [
    (1000, 3, None),                                                                  # one-wave bundles
    (1000, 4, KernelChoice("staged", replicas=4, bundle_rows=8, pair=True)),          # LDS-staged, R = 4
    (3000, 3, None),                                                                  # wide-row bundles
], ids=["multi", "staged-R4", "wide"])
def test_closed_gate_leaves_a_prefilled_G_untouched(d, replicas, choice, native):
    prec, parts, host, beta_h, bh = _host_case(d, ec.DEFAULT_SIZES)
    dev = {p: (X.to(DEV), y.to(DEV)) for p, (X, y) in parts.items()}
    plan = DenseGradPlan(ec.messages(replicas), dev, prec, nx.LOGISTIC, d, choice=choice)
    assert plan.choice.kind == ("staged" if choice else "multi" if d == 1000 else "wide")
    launcher = plan.native_launcher()
    beta = beta_h.to(DEV)
    ref = plan.out_buffer()[0]
    launcher.launch(beta, ref)
    gate = torch.ones(1, dtype=torch.int32, device=DEV)
    G = torch.full_like(ref, 7.0)
    launcher.launch(beta, G, gate)
    torch.cuda.synchronize()
    assert torch.all(G == 7.0)
    gate.zero_()
    launcher.launch(beta, G, gate)
    torch.cuda.synchronize()
    assert torch.equal(G, ref)


# ---- 4. the evaluation GEMM at its tile edges ------------------------------------------------------
EVAL_R = (1, 16, 17)


@functools.lru_cache(maxsize=None)
def _eval_case(n, d, R):
    prec = get_precision(NAME)
    rng = np.random.RandomState(100000 + 1009 * n + 31 * d + R + prec.code)
    X, y, Xh = nx.hostile_partition(rng, n, d, prec)
    B = torch.stack([nx.hostile_beta(rng, d, prec)[0] for _ in range(R)])  # [R, ld] fp64
    oracles = {loss: nx.oracle_eval(loss, Xh, y.numpy(), B[:, :d].numpy(), prec) for loss in nx.LOSSES}
    return prec, X, y, B, oracles


def _check(got, ref, bound, what):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    err = np.abs(got.astype(nx.LD) - ref)
    assert np.all(err <= bound), f"{what}: beyond the bound at {np.argwhere(~(err <= bound))[:4].tolist()}"


@pytest.mark.parametrize("d", [1, 31, 32, 33, 1000])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_eval_gemm_at_tile_edges(n, d, native):
    """fp32 X, fp64 y / B / P: the 16-byte-aligned kernel on padded rows and the scalar-staging kernel on rows of
    d columns, through the kernel (NaN-filled P) and through ops/eval.py with the accumulator from the precision."""
    for R in EVAL_R:
        prec, X, y, B, oracles = _eval_case(n, d, R)
        for padded in (True, False):
            Xd = (X if padded else X[:, :d].contiguous()).to(DEV)
            Bd = (B if padded else B[:, :d].contiguous()).to(DEV)
            yd = y.to(DEV)
            for loss in nx.LOSSES:
                what = f"n={n} d={d} R={R} {nx.LOSS_IDS[loss]} padded={padded}"
                Pref, dP, sref, ds = oracles[loss]
                Pn = torch.full((n, R), float("nan"), dtype=torch.float64, device=DEV)
                s = torch.zeros(R, dtype=torch.float64, device=DEV)
                native.eval_gemm_loss(loss, Xd, n, d, yd, Bd, s, Pn)
                _check(Pn.cpu().numpy(), Pref, dP, what + " kernel P")
                _check(s.cpu().numpy(), sref, ds, what + " kernel sums")
                sums, rows = loss_sums([(Xd, yd)], Bd, d, loss, acc=prec)
                assert rows == n
                _check(sums, sref, ds, what + " loss_sums")
                P, s2 = predictions_and_loss(Xd, yd, Bd, d, loss, acc=prec)
                assert P.dtype == torch.float64
                _check(P.cpu().numpy(), Pref, dP, what + " predictions_and_loss P")
                _check(s2, sref, ds, what + " predictions_and_loss sums")
            P = predictions(Xd, Bd, d, acc=prec)
            _check(P.cpu().numpy(), oracles[nx.LOGISTIC][0], oracles[nx.LOGISTIC][1], f"n={n} d={d} R={R} predictions")


# ---- 5. the engine ---------------------------------------------------------------------------------
ENGINE = {"naive": (0, 0, 0, 5, 0, 0), "agc-uneven": (1, 0, 3, 9, 2, 6), "cyclic-s2": (1, 0, 0, 7, 2, 0)}


def _engine(name, rule, device, precision=NAME, source=None, **kw):
    from test_engine_cpu import make

    cfg, src, sch, parts = make(ENGINE[name], rule, precision=precision, **kw)
    tr = Trainer(cfg, DistEnv(device=torch.device(device)), source or src, scheme=sch)
    res = tr.run()
    ev = evaluate(tr, res, write=False)
    return tr, res, ev


@functools.lru_cache(maxsize=None)
def _cpu_engine(name, rule):
    return _engine(name, rule, "cpu")[1:]


def _same_run(res, ev, ref, ref_ev):
    assert [[(w, p) for (w, p, _t) in r] for r in res.arrivals] == [[(w, p) for (w, p, _t) in r] for r in ref.arrivals]
    np.testing.assert_allclose(res.betaset, ref.betaset, rtol=1e-9, atol=1e-11)
    for k in ("training_loss", "testing_loss", "auc"):
        np.testing.assert_allclose(getattr(ev, k), getattr(ref_ev, k), rtol=1e-9, atol=1e-11, err_msg=k)


@pytest.mark.parametrize("device_loop", ["graph", "stream", "off"])
@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", sorted(ENGINE))
def test_gpu_engine_matches_the_cpu_engine(name, rule, device_loop, native):
    tr, res, ev = _engine(name, rule, "cuda", device_loop=device_loop)
    assert tr.prec.name == NAME and tr.device_loop == (None if device_loop == "off" else device_loop)
    assert tr.G.dtype == torch.float64 and all(X.dtype == torch.float32 for X, _ in tr._parts.values())
    _same_run(res, ev, *_cpu_engine(name, rule))


@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", sorted(ENGINE))
def test_gpu_engine_on_fp32_exact_data_matches_gpu_fp64(name, rule, native):
    from test_fp32x64_cpu import exact_source

    a = _engine(name, rule, "cuda", source=exact_source(ENGINE[name]))
    b = _engine(name, rule, "cuda", precision="fp64", source=exact_source(ENGINE[name]))
    assert a[0].rank_report()["storage_max_rel_rounding"] == 0.0
    _same_run(a[1], a[2], b[1], b[2])


def test_three_ranks_over_the_ipc_mailbox(tmp_path, native):
    """AGC over the IPC mailbox, 3 ranks on the one GPU: the workers' fused put carries storage code 3.  Replayed
    with the fp64 NumPy oracle on the rows rounded to fp32."""
    from oracle import replay
    from test_engine_cpu import CASES, make
    from test_multiproc_gpu import _launch

    case_i = 4
    r = _launch(3, case_i, "AGD", str(tmp_path / "x.npz"), EH_TEST_CFG=json.dumps({"precision": NAME}))
    assert str(r["transport"]) == "ipc"
    reports = json.loads(str(r["reports"]))
    assert any(rep.get("fused_put") for rep in reports if rep["role"] == "workers"), reports
    cfg, src, sch, parts = make(CASES[case_i], "AGD")
    rounded = [(X.astype(np.float32).astype(np.float64), y) for X, y in parts]
    arrivals = [[(w, p, 0.0) for (w, p) in a] for a in r["arrivals"]]
    ref = replay(sch, rounded, r["beta0"], arrivals, "AGD", cfg.alpha_value, cfg.n_rows, 10.0 * np.ones(len(arrivals)))
    np.testing.assert_allclose(r["betaset"], ref, rtol=1e-9, atol=1e-11)
