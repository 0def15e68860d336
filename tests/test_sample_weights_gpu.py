"""The weighted loss codes (csrc/kernels/common.h kLogisticW = 4, kSquaredHingeW = 5) on the gfx950 kernels (GPU only).

Every kernel family a plan can select runs three ways: with unit weights, where code 4 / 5 must give the messages of
code 0 / 2 bit for bit; with hostile weights (10**U(-2, 2), about 5 % exact zeros on both classes), where every
column of every message is held to its own bound against the long-double oracle of tests/sample_weights_cases.py
with the project's K = 8; and with weights that are all zero, with both zero signs, where the gradient is exactly
zero.  Then the evaluation kernels, the launch validators (the multi-model kernel has no weighted instance and keeps
rejecting the codes; a weighted sweep runs on CPU tensors only) and the engine (GPU against CPU, the round loops
against each other, a closed gate, three ranks over IPC).  Dense partitions of [257, 64, 1, 0] rows.
"""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import numerics as nx
import sample_weights_cases as sw
from erasurehead_amd.codes import make_scheme, scheme_key
from erasurehead_amd.config import RunConfig
from erasurehead_amd.data.source import ArraySource, balanced_class_weights
from erasurehead_amd.engine import Trainer, evaluate
from erasurehead_amd.models import losses
from erasurehead_amd.ops import DenseGradPlan, SparseGradPlan, get_precision, loss_sums
from erasurehead_amd.ops.eval import auc_columns, predictions_and_loss, sign_labels, sparse_eval_device
from erasurehead_amd.ops.grad import KernelChoice
from erasurehead_amd.ops.multimodel import MultiModelGradPlan
from erasurehead_amd.parallel.dist import DistEnv
from test_multimodel_cpu import CASES
from test_sample_weights_cpu import CW, draw_weights, make_weighted, replay

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
DENSE = sw.dense_families()
ENGINE_TOL = dict(rtol=1e-9, atol=1e-11)  # tests/test_squared_hinge_gpu.py, GPU engine against CPU engine


# ---- dense plans ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_case(pn, d, pack):
    return sw.dense_case(get_precision(pn), d, sizes=sw.SIZES[:3] if pack else sw.SIZES, plain_x=pack)


def _dense_plans(fam, which, codes):
    """{code: plan} of one family over the same partitions with the labels ``which``; also the host view."""
    fid, pn, d, R, kw, pack = fam
    prec = get_precision(pn)
    parts, weights, host, beta, bh = _dense_case(pn, d, pack)
    lab = sw.labels(parts, weights, prec, which)
    dev = {p: (X.to(DEV), lab[p].to(DEV)) for p, (X, _) in parts.items()}
    msgs = sw.distinct_messages(not pack) if R == 1 else sw.replica_messages(R, not pack)
    choice = KernelChoice(**kw)
    extra = {"pack": True} if pack else {}
    plans = {}
    for code in codes:
        plan = DenseGradPlan(msgs, dev, prec, code, d, choice=choice, **extra)
        assert plan.choice == choice, fid
        if pack:
            assert plan.packed and plan.packed_bundles > 0
        plans[code] = plan
    hostw = {p: (host[p], lab[p].double().numpy()) for p in parts}  # the labels as stored (accumulator dtype)
    return prec, plans, msgs, hostw, beta.to(DEV), bh


def _launch(plan, beta, how="launcher"):
    G = torch.full((plan.nslots, plan.ld), float("nan"), dtype=plan.prec.acc, device=DEV)
    if how == "run":
        plan.run(beta, G)
    else:
        plan.native_launcher().launch(beta, G)
    torch.cuda.synchronize()
    return G


@pytest.mark.parametrize("fam", DENSE, ids=[f[0] for f in DENSE])
def test_dense_unit_weights_are_bitwise_the_unweighted_kernel(fam, native):
    prec, plans, msgs, hostw, beta, bh = _dense_plans(fam, "unit", (0, 2, 4, 5))
    for code in sw.WEIGHTED:
        Gw, Gb = _launch(plans[code], beta), _launch(plans[sw.BASE[code]], beta)
        assert torch.isfinite(Gb).all() and bool((Gb != 0).any())
        assert torch.equal(Gw, Gb), f"{fam[0]}: code {code} with unit weights differs from code {sw.BASE[code]}"


@pytest.mark.parametrize("fam", DENSE, ids=[f[0] for f in DENSE])
def test_dense_hostile_weights_stay_within_the_column_bounds(fam, native):
    prec, plans, msgs, hostw, beta, bh = _dense_plans(fam, "hostile", sw.WEIGHTED)
    d = fam[2]
    for code, plan in plans.items():
        G, G2 = _launch(plan, beta, "run"), _launch(plan, beta)
        Gh = G.double().cpu().numpy()
        for s, m in enumerate(msgs):
            ref, bound = sw.message(code, m, hostw, bh, prec)
            nx.check_columns(Gh[s, :d], ref, bound, f"{fam[0]} {sw.IDS[code]} [{plan.choice.label()}] message {s}")
        assert torch.all(G[:, d:] == 0), "padding columns must be exactly zero"
        if msgs[-1] == [(sw.EMPTY, 1.0)]:
            assert torch.all(G[-1] == 0), "a message of the empty partition must be exactly zero"
        assert torch.equal(G, G2), "two launches differ"


@pytest.mark.parametrize("fam", DENSE, ids=[f[0] for f in DENSE])
def test_dense_zero_weights_give_an_exactly_zero_gradient(fam, native):
    prec, plans, msgs, hostw, beta, bh = _dense_plans(fam, "zero", sw.WEIGHTED)
    signs = np.concatenate([np.signbit(y) for _, y in hostw.values()])
    assert signs.any() and not signs.all()  # both zero signs
    for code, plan in plans.items():
        G = _launch(plan, beta)
        assert torch.all(G == 0), f"{fam[0]} {sw.IDS[code]}"


# ---- sparse plans ---------------------------------------------------------------------------------
SPARSE = [(f"{pn}-{fid}-d{d}", pn, d, po, ell) for pn in ("fp64", "fp32") for fid, po, ell in sw.SPARSE_FAMILIES
          for d in (37, 1000)]


def _stored(yt, prec):
    """Weighted labels as the plan stores them: rounded to the accumulator dtype."""
    return np.asarray(yt, np.float32 if prec.acc == torch.float32 else np.float64).astype(np.float64)


def _sparse_run(plan, beta):
    G, G2 = plan.out_buffer()[0], plan.out_buffer()[0]
    plan.run(beta, G)
    plan.native_launcher().launch(beta, G2)
    torch.cuda.synchronize()
    assert torch.equal(G, G2), "two launches differ"
    return G


def _sparse_three_ways(parts, weights, msgs, prec, d, make_plan, what):
    rng = np.random.RandomState(d)
    beta_h, bh = sw.sparse_beta(rng, d, prec)
    beta = beta_h.to(DEV)
    unit = {p: (X, y) for p, (X, y) in parts.items()}
    hostile = {p: (X, _stored(sw.carry(y, weights[p]), prec)) for p, (X, y) in parts.items()}
    zero = {p: (X, sw.mixed_zeros(np.random.RandomState(p), len(y))) for p, (X, y) in parts.items()}
    dense = {p: (np.asarray(X.todense()), hostile[p][1]) for p, (X, _) in parts.items()}
    for code in sw.WEIGHTED:
        Gw, Gb = _sparse_run(make_plan(unit, code), beta), _sparse_run(make_plan(unit, sw.BASE[code]), beta)
        assert bool((Gb != 0).any()) and torch.equal(Gw, Gb), f"{what}: unit weights, code {code}"
        G = _sparse_run(make_plan(hostile, code), beta)
        Gh = G.double().cpu().numpy()
        for s, m in enumerate(msgs):
            ref, bound = sw.message(code, m, dense, bh, prec)
            nx.check_columns(Gh[s, :d], ref, bound, f"{what} {sw.IDS[code]} message {s}")
        assert torch.all(G[:, d:] == 0), "padding columns must be exactly zero"
        assert torch.all(_sparse_run(make_plan(zero, code), beta) == 0), f"{what}: zero weights, code {code}"


@pytest.mark.parametrize("case", SPARSE, ids=[c[0] for c in SPARSE])
def test_sparse_row_formats(case, native):
    """ELL with beta in LDS (pattern-only rows), valued ELL and CSR row passes."""
    cid, pn, d, pattern_only, use_ell = case
    prec = get_precision(pn)
    parts, weights = sw.sparse_case(prec, d, pattern_only)

    def make_plan(p, code):
        plan = SparseGradPlan(sw.SPARSE_MSGS, p, prec, code, d, device=DEV, use_ell=use_ell)
        assert plan.pattern_only == pattern_only and plan.ell == use_ell
        return plan

    _sparse_three_ways(parts, weights, sw.SPARSE_MSGS, prec, d, make_plan, cid)


@pytest.mark.parametrize("pn", ["fp64", "fp32"])
def test_sparse_frc_units(pn, native):
    """FRC groups stacked into units: the column pass of the units plan reads the row passes' weighted residuals."""
    from erasurehead_amd.data.synthetic import onehot_partitions

    prec = get_precision(pn)
    parts_l, _, d = onehot_partitions(4 * 1500, 1800, 9, 4, seed=6)
    parts = dict(enumerate(parts_l))
    rng = np.random.RandomState(8)
    weights = {p: sw.hostile_weights(rng, len(y)) for p, (_, y) in parts.items()}
    msgs = [[(0, 1.0), (1, 1.0)], [(0, 1.0), (1, 1.0)], [(2, 1.0), (3, 1.0)], [(2, 1.0), (3, 1.0)], [(2, 1.0), (3, 1.0)]]

    def make_plan(p, code):
        plan = SparseGradPlan(msgs, p, prec, code, d, device=DEV, use_ell=True)
        assert plan.units == [(0, 1), (2, 3)] and plan.identity
        return plan

    _sparse_three_ways(parts, weights, msgs, prec, d, make_plan, f"{pn} frc units")


# ---- evaluation kernels ---------------------------------------------------------------------------
def _check_sums(s, sref, bound, what):
    s = np.asarray(s, np.float64)
    assert np.all(np.isfinite(s))
    err = np.abs(s.astype(nx.LD) - sref)
    assert np.all(err <= bound), (what, err.astype(float).tolist(), bound.astype(float).tolist())


@pytest.mark.parametrize("pn", ["fp64", "fp32", "bf16"])
@pytest.mark.parametrize("n,d,R", [(257, 37, 5), (129, 65, 113)])
def test_dense_evaluation_against_the_weighted_long_double_loss(n, d, R, pn, native):
    prec = get_precision(pn)
    rng = np.random.RandomState(1009 * n + d + prec.code)
    X, y, Xh = nx.hostile_partition(rng, n, d, prec)
    yt = torch.from_numpy(sw.carry(y.double().numpy(), sw.hostile_weights(rng, n))).to(prec.acc)
    B = torch.stack([nx.hostile_beta(rng, d, prec)[0] for _ in range(R)])
    Bh = B[:, :d].double().numpy()
    Xd, yd, Bd = X.to(DEV), yt.to(DEV), B.to(DEV)
    for code in sw.WEIGHTED:
        Pref, dP, sref, ds = sw.evaluation(code, Xh, yt.double().numpy(), Bh, prec)
        sums, rows = loss_sums([(Xd, yd)], Bd, d, code)
        assert rows == n
        _check_sums(sums, sref, ds, f"{pn} loss_sums {sw.IDS[code]}")
        P, s2 = predictions_and_loss(Xd, yd, Bd, d, code)
        _check_sums(s2, sref, ds, f"{pn} predictions_and_loss {sw.IDS[code]}")
        err = np.abs(P.double().cpu().numpy().astype(nx.LD) - Pref)
        assert np.all(err <= dP)
    # the AUC of a weighted run: on the classes, not on y~
    s = sign_labels(yd)
    Pd = P.double()
    want = [losses.roc_auc(s.cpu().numpy(), Pd[:, j].cpu().numpy()) for j in range(R)]
    np.testing.assert_allclose(auc_columns(s, Pd), want, rtol=1e-12)


@pytest.mark.parametrize("pattern_only", [True, False])
def test_sparse_evaluation_against_the_weighted_long_double_loss(pattern_only, native):
    prec = get_precision("fp64")
    d, R = 1000, 37
    parts, weights = sw.sparse_case(prec, d, pattern_only)
    X, y = parts[2]
    yt = sw.carry(y, weights[2])
    assert np.any(yt == 0) and set(np.signbit(yt[yt == 0])) == {True, False}
    rng = np.random.RandomState(4)
    Bh = rng.randn(R, d)
    B = torch.from_numpy(Bh).to(DEV)
    Xh = np.asarray(X.todense())
    for code in sw.WEIGHTED:
        Pref, dP, sref, ds = sw.evaluation(code, Xh, yt, Bh, prec)
        sums, rows = loss_sums([(X, torch.from_numpy(yt))], B, d, code)
        assert rows == X.shape[0]
        _check_sums(sums, sref, ds, f"sparse loss_sums {sw.IDS[code]}")
        P, s2 = predictions_and_loss(X, torch.from_numpy(yt), B, d, code)
        _check_sums(s2, sref, ds, f"sparse predictions_and_loss {sw.IDS[code]}")
        assert np.all(np.abs(P.double().cpu().numpy().astype(nx.LD) - Pref) <= dP)
        _, s3 = sparse_eval_device(X, torch.from_numpy(yt), B.t().contiguous(), code, False)
        _check_sums(s3.cpu().numpy(), sref, ds, f"sparse kernel {sw.IDS[code]}")
    s = sign_labels(torch.from_numpy(yt))
    want = [losses.roc_auc(s.numpy(), Pref[:, j].astype(np.float64)) for j in range(R)]
    np.testing.assert_allclose(auc_columns(s, P.double()), want, rtol=1e-9)


NAIVE = [[(0, 1.0)], [(1, 1.0)], [(2, 1.0)], [(3, 1.0)]]


# ---- launch validation ----------------------------------------------------------------------------
@pytest.mark.parametrize("code", [3, 6, -1])
def test_launchers_reject_other_loss_codes(code, native):
    prec = get_precision("fp64")
    d = 37
    parts, weights, host, beta_h, bh = _dense_case("fp64", d, False)
    dev = {p: (X.to(DEV), y.to(DEV)) for p, (X, y) in parts.items()}
    beta = beta_h.to(DEV)
    # dense
    plan = DenseGradPlan(sw.distinct_messages(), dev, prec, 4, d)
    G = torch.full((plan.nslots, plan.ld), 123.0, dtype=prec.acc, device=DEV)
    with pytest.raises(RuntimeError, match="invalid"):
        native.GradLauncher.dense(prec.code, code, plan.cpl, plan.segs, plan.tasks, plan.slab, plan.slot_task_begin,
                                  plan.part, plan.ld, choice=plan._native_choice).launch(beta, G)
    torch.cuda.synchronize()
    assert torch.all(G == 123.0)
    plan.run(beta, G)
    torch.cuda.synchronize()
    assert not torch.any(G[:-1, :d] == 123.0)
    # sparse: the plan's own launcher with the code swapped
    sparts, _ = sw.sparse_case(prec, d, False)
    splan = SparseGradPlan(sw.SPARSE_MSGS, sparts, prec, 5, d, device=DEV)
    splan.loss = code
    with pytest.raises(RuntimeError, match="invalid"):
        splan.native_launcher().launch(beta, splan.out_buffer()[0])
    torch.cuda.synchronize()
    # multi-model: no weighted instance, so its launch validator and its launcher keep the range 0..2
    i32 = dict(dtype=torch.int32, device=DEV)
    segs = torch.zeros(32, dtype=torch.uint8, device=DEV)
    tasks, ptb = torch.zeros((0, 5), **i32), torch.zeros(1, **i32)
    buf = torch.zeros(8 * 1024, dtype=torch.float64, device=DEV)
    for ok in (0, 1, 2):
        native._grad_models_raw(0, ok, 3, segs, tasks, ptb, buf, buf, buf, 37, 38)
    for bad in (code, 4, 5):
        with pytest.raises(RuntimeError, match="invalid"):
            native._grad_models_raw(0, bad, 3, segs, tasks, ptb, buf, buf, buf, 37, 38)
        with pytest.raises(ValueError):
            MultiModelGradPlan(NAIVE, dev, prec, bad, 3, d)
    torch.cuda.synchronize()


# ---- the engine -----------------------------------------------------------------------------------
def _both_devices(build):
    """build(dev) -> (cfg, src, sch); runs it on the CPU and on the GPU and returns {dev: (trainer, result, eval)}."""
    out = {}
    for dev in ("cpu", "cuda"):
        cfg, src, sch = build()
        tr = Trainer(cfg, DistEnv(device=torch.device(dev)), src, scheme=sch)
        res = tr.run()
        out[dev] = (tr, res, evaluate(tr, res, write=False))
    return out


def _compare(out):
    (tc, rc, ec), (tg, rg, eg) = out["cpu"], out["cuda"]
    assert tg.weighted and tg.loss == tc.loss and tg.class_weight == tc.class_weight
    assert tg.weight_sum_over_n == pytest.approx(tc.weight_sum_over_n, rel=1e-12)
    np.testing.assert_allclose(rg.betaset, rc.betaset, **ENGINE_TOL)
    for a, b in ((eg.training_loss, ec.training_loss), (eg.testing_loss, ec.testing_loss), (eg.auc, ec.auc)):
        np.testing.assert_allclose(a, b, **ENGINE_TOL)


@pytest.mark.parametrize("loss", ["logistic", "squared_hinge"])
@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", ["naive", "agc_uneven"])
def test_gpu_engine_matches_cpu_on_a_dense_source(name, rule, loss, native):
    out = _both_devices(lambda: make_weighted(CASES[name], rule, loss)[:3])
    _compare(out)
    tg, rg, eg = out["cuda"]
    Xt, yt = tg.source.inner._test
    assert eg.auc[-1] == pytest.approx(losses.roc_auc(yt, Xt @ rg.betaset[-1]), rel=1e-12)


@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("ver,k", [(None, 0), (3, 4)], ids=["naive", "agc"])
def test_gpu_engine_matches_cpu_on_a_one_hot_source(ver, k, rule, native):
    from erasurehead_amd.data.synthetic import onehot_partitions

    W, s = 6, (0 if ver is None else 2)
    parts, test, d = onehot_partitions(6 * 150, 400, 8, W, seed=11)
    n = sum(p[0].shape[0] for p in parts)
    key = scheme_key(0 if ver is None else 1, 0, ver or 0)

    def build():
        src = ArraySource(parts, test, sparse=True, weights=draw_weights(parts))
        cfg = RunConfig(W + 1, n, d, "/tmp/eh_gpu_sw/", 1, "covtype", 0 if ver is None else 1, s, 0, ver or 0, k, 0, rule,
                        num_itrs=6, seed=0, verbose=False, class_weight="balanced")
        return cfg, src, make_scheme(key, W, s, n, k, 0, rng=np.random.RandomState(0))

    out = _both_devices(build)
    _compare(out)
    tg = out["cuda"][0]
    y = np.concatenate([yy for _, yy in parts])
    assert tg.plan.ell and tg.class_weight == balanced_class_weights(int((y > 0).sum()), int((y < 0).sum()))


def test_a_weighted_sweep_on_the_gpu_is_rejected_before_anything_is_loaded(native):
    """The multi-model kernel has no weighted instance: the trainer says so by name (the CPU engine runs it)."""
    cfg, src, sch, parts, wts = make_weighted(CASES["frc"], "GD", sweep_alpha=[1e-3, 1e-2, 1e-1])
    with pytest.raises(ValueError, match="--class-weight / --sample-weights"):
        Trainer(cfg, DistEnv(device=torch.device(DEV)), src, scheme=sch)
    tr = Trainer(cfg, DistEnv(device=torch.device("cpu")), src, scheme=sch)
    assert tr.models == 3 and tr.loss == losses.LOGISTIC_W


def _gpu_run(name, rule, device_loop, loss="logistic"):
    cfg, src, sch, parts, wts = make_weighted(CASES[name], rule, loss)
    cfg.device_loop = device_loop
    tr = Trainer(cfg, DistEnv(device=torch.device(DEV)), src, scheme=sch)
    return tr, tr.run()


@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_stream_loop_and_native_pump_agree_bitwise(rule, native):
    ts, rs = _gpu_run("agc_uneven", rule, "stream")
    to, ro = _gpu_run("agc_uneven", rule, "off")
    assert ts.rank_report()["round_loop"] == "stream" and to.rank_report()["round_loop"] == "native pump"
    np.testing.assert_array_equal(rs.betaset, ro.betaset)


def test_closed_gate_leaves_the_messages_untouched(native):
    closed = torch.ones(1, dtype=torch.int32, device=DEV)
    opened = torch.zeros(1, dtype=torch.int32, device=DEV)
    fam = [f for f in DENSE if f[0] == "fp64-multi-R3-d1000"][0]
    prec, plans, msgs, hostw, beta, bh = _dense_plans(fam, "hostile", sw.WEIGHTED)
    sparts, sweights = sw.sparse_case(prec, 37, True)
    shost = {p: (X, sw.carry(y, sweights[p])) for p, (X, y) in sparts.items()}
    beta37 = nx.hostile_beta(np.random.RandomState(0), 37, prec)[0].to(DEV)
    cases = [(plans[4], beta), (plans[5], beta),
             (SparseGradPlan(sw.SPARSE_MSGS, shost, prec, 5, 37, device=DEV), beta37)]
    for plan, b in cases:
        L = plan.native_launcher()
        G = plan.out_buffer()[0].fill_(12345.0)
        L.launch(b, G, gate=closed)
        torch.cuda.synchronize()
        assert bool((G == 12345.0).all()), type(plan).__name__
        G.zero_()
        L.launch(b, G, gate=opened)
        torch.cuda.synchronize()
        assert bool((G != 0).any()) and not bool((G == 12345.0).any())


def test_three_ranks_over_ipc_match_the_replay(tmp_path, native):
    out = str(tmp_path / "weights_ipc.npz")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", EH_WEIGHTS_OUT=out,
               EH_WEIGHTS_DEVICE="cuda", EH_WEIGHTS_CASE="agc_uneven")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr",
           "127.0.0.1", f"--master-port={port}", os.path.join(HERE, "mp_sample_weights_run.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out, allow_pickle=True)
    assert str(z["transport"]) == "ipc" and bool(z["weighted"])
    check_against_replay(z, "agc_uneven")


def check_against_replay(z, name):
    """The saved run of tests/mp_sample_weights_run.py against the replay of its logged arrivals."""
    cfg, src, sch, parts, wts = make_weighted(CASES[name], "AGD", class_weight="balanced")
    y = np.concatenate([yy for _, yy in parts])
    cw = balanced_class_weights(int((y > 0).sum()), int((y < 0).sum()))
    np.testing.assert_array_equal(z["class_weight"], cw)  # every rank used rank 0's two numbers
    arrivals = [[tuple(a) for a in rnd] for rnd in z["arrivals"]]
    ref = replay("logistic", sch, parts, wts, cw, z["beta0"], arrivals, "AGD", cfg.alpha_value, cfg.n_rows, cfg.eta())
    got = np.asarray(z["betaset"])
    np.testing.assert_allclose(got[:, :33], ref, rtol=1e-9, atol=1e-11)
    assert np.all(got[:, 33:] == 0.0)
