"""The cross-validation gradient kernel (csrc/kernels/grad_folds.hip) and --cv runs of the engine on the GPU (GPU only).

The kernel is held to the long-double oracle and the per-column bounds of tests/numerics.py with the project's
K = 8, on hostile inputs with an independent hostile beta per fold model: block k of every message against
``oracle_message(loss, segments, host_k, beta_k, prec)``, host_k the host data with the rows of fold k zeroed (a zero
row adds nothing to the gradient or to its bound).  Partitions of [150, 1, 67, 0] rows: the 150-row partition is cut
into tasks at rows 64 and 128, which are multiples of neither 3 nor 5, and at d = 1000 its stages of 4 rows start at
rows that are no multiples of the fold count -- the smallest shapes at which a task-local or stage-local fold index,
in place of the partition-local one, gives a wrong answer.  Fold counts 2, 3, 5, 8: 4, 2 and 1 waves per model pair,
an idle fourth wave at 5 and an idle second model of a wave at 3 and 5.  Block k is also bitwise the sweep kernel's
block k on the data with the rows of fold k zeroed: the two kernels are one text.

Held-out rows and non-finite values: a held-out row runs through the dot products and the gradient FMAs with residual
0, so a non-finite LABEL in fold k never reaches model k (the residual is dropped by a select), which is what
test_folds_do_not_leak checks; a non-finite VALUE OF X in a held-out row would reach it as 0 * NaN.  The engine
requires finite data, and the CPU plan leaves the rows out altogether (tests/test_cv_cpu.py).
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import block_edge_cases as bc
from cv_cases import CASES, TOL, check_against_replay, make
from erasurehead_amd.engine import Trainer, evaluate
from erasurehead_amd.models import losses
from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.cv import CvGradPlan
from erasurehead_amd.ops.multimodel import MultiModelGradPlan
from erasurehead_amd.parallel.dist import DistEnv
from numerics import LOSS_IDS, LOSSES, check_columns, hostile_beta, hostile_partition, oracle_message

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [150, 1, 67, 0]
CODED = [[(0, 1.0), (1, -0.7)], [(2, 2.5), (3, 1.0)], [(1, 1.0), (0, 0.3), (2, 1.0)]]  # a cyclic row: the encode path
NAIVE = [[(0, 1.0)], [(1, 1.0)], [(2, 1.0)], [(3, 1.0)]]  # the identity path
FOLDS = [2, 3, 5, 8]
WIDTHS = [37, 300, 1000, 1024]  # 4, 8 and 16 columns per lane; stages of 4 rows at 1000; the full width
PRECS = ["fp64", "fp32", "fp32x64"]
GRID = [(d, loss, p) for d in WIDTHS for loss in LOSSES for p in PRECS]

_inputs = {}


def inputs(d, prec_name):
    """(partitions on the device, host X and labels, 8 hostile betas), drawn once per (d, precision); never changed."""
    key = (d, prec_name)
    if key not in _inputs:
        prec = get_precision(prec_name)
        rng = np.random.RandomState(2000 + d)
        parts, host = {}, {}
        for p, n in enumerate(SIZES):
            Xs, y, Xh = hostile_partition(rng, n, d, prec)
            parts[p] = (Xs.to(DEV).contiguous(), y.to(DEV).contiguous())
            host[p] = (Xh, y.double().numpy())
        _inputs[key] = (parts, host, [hostile_beta(rng, d, prec) for _ in range(8)])
    return _inputs[key]


def zero_fold(host, K, k):
    """The host data as fold model k sees it: the rows of fold k (row i of a partition: fold i mod K) are zero rows."""
    out = {}
    for p, (X, y) in host.items():
        Xk = X.copy()
        Xk[k::K] = 0.0
        out[p] = (Xk, y)
    return out


def model(betas, K):
    """The flattened [K][ld] model on the device and the fp64 view of every block."""
    return torch.cat([b for b, _ in betas[:K]]).to(DEV), [bh for _, bh in betas[:K]]


def check(G, msgs, host, bhs, loss, prec, d, what):
    K, ld = len(bhs), prec.ld(d)
    got = G.double().cpu().numpy().reshape(len(msgs), K, ld)
    for k in range(K):
        host_k = zero_fold(host, K, k)
        for s, m in enumerate(msgs):
            ref, bound = oracle_message(loss, m, host_k, bhs[k], prec)
            check_columns(got[s, k, :d], ref, bound, f"{what} message {s} fold model {k}")
    assert np.all(got[:, :, d:] == 0.0), f"{what}: padding columns must be exact zeros"


# ---- 1. the kernel against the long-double oracle
@pytest.mark.parametrize("K", FOLDS)
@pytest.mark.parametrize("d,loss,prec_name", GRID, ids=[f"d{d}-{LOSS_IDS[l]}-{p}" for d, l, p in GRID])
def test_kernel_within_the_column_bounds(d, loss, prec_name, K, native):
    prec = get_precision(prec_name)
    parts, host, betas = inputs(d, prec_name)
    beta, bhs = model(betas, K)
    for msgs in (NAIVE, CODED):
        plan = CvGradPlan(msgs, parts, prec, loss, K, d)
        assert plan.identity == (msgs is NAIVE) and plan.ld == K * prec.ld(d)
        assert [tuple(t[2:4]) for t in plan.tasks.cpu().tolist()[:3]] == [(0, 64), (64, 128), (128, 150)]
        G = plan.out_buffer()[0].fill_(float("nan"))  # every element, padding included, must be overwritten
        plan.run(beta, G)
        G2 = plan.out_buffer()[0].fill_(float("nan"))
        plan.native_launcher().launch(beta, G2)
        torch.cuda.synchronize()
        check(G, msgs, host, bhs, loss, prec, d, f"{'naive' if msgs is NAIVE else 'coded'} K={K}")
        assert torch.equal(G, G2)  # two launches: bitwise identical


# ---- 1b. stage edges: ragged stages of every row count, ring reuse, tasks that start at odd rows
STAGE_GRID = bc.scalar_grid(LOSSES)
_edge_parts = {}


@pytest.mark.parametrize("K", bc.SCALAR_BLOCKS)
@pytest.mark.parametrize("d,loss,prec_name", STAGE_GRID, ids=[f"d{d}-{LOSS_IDS[l]}-{p}" for d, l, p in STAGE_GRID])
def test_stage_edges_within_the_column_bounds(d, loss, prec_name, K, native, monkeypatch):
    """Partitions of tests/block_edge_cases.py partition_sizes (every ragged stage around a row per wave and the full
    stage, S + 1, 2S, 2S + 1, 3S + 2, empty), once as whole tasks of three and four stages and once cut into tasks of
    37 rows, naive and coded messages; the same oracle, bound and checks as above.  Tasks that start at rows 37 and
    74 are the point here: the fold of a row is its index in the partition mod K, so under tasks of 37 rows block k
    must still be bitwise the sweep kernel's block k on the data with the rows of fold k zeroed."""
    prec = get_precision(prec_name)
    sizes, cpu_parts, host, betas = bc.scalar_inputs(d, prec_name, K)
    if (d, prec_name, K) not in _edge_parts:
        _edge_parts[(d, prec_name, K)] = bc.to_device(cpu_parts, DEV)
    parts = _edge_parts[(d, prec_name, K)]
    beta, bhs = model(betas, K)
    ld = prec.ld(d)
    for rows in bc.TASK_ROWS:
        bc.forced_task_rows(monkeypatch, rows)
        for kind in ("naive", "coded"):
            msgs = bc.MESSAGES[kind](len(sizes))
            plan = CvGradPlan(msgs, parts, prec, loss, K, d)
            assert plan.identity == (kind == "naive")
            bc.assert_tasks_reach_the_edges(plan, sizes, bc.geometry(prec, d, K)[0], rows)
            G = plan.out_buffer()[0].fill_(float("nan"))
            plan.run(beta, G)
            G2 = plan.out_buffer()[0].fill_(float("nan"))
            plan.native_launcher().launch(beta, G2)
            torch.cuda.synchronize()
            check(G, msgs, host, bhs, loss, prec, d, f"{kind} K={K} tasks of {rows}")
            assert torch.equal(G, G2)  # two launches: bitwise identical
        if rows == bc.ODD_TASKS:  # G: the coded messages
            for k in range(K):
                parts_k = {}
                for p, (X, y) in parts.items():
                    Xk = X.clone()
                    Xk[k::K] = 0
                    parts_k[p] = (Xk, y)
                sweep = MultiModelGradPlan(msgs, parts_k, prec, loss, K, d)
                Gk = sweep.run(beta, sweep.out_buffer()[0]).reshape(len(msgs), K, ld)
                torch.cuda.synchronize()
                assert torch.equal(G.reshape(len(msgs), K, ld)[:, k], Gk[:, k]), f"fold model {k}"


# ---- 2. bitwise the sweep kernel on the data with the fold's rows zeroed: the same wave layout, row and FMA order
@pytest.mark.parametrize("K", FOLDS)
@pytest.mark.parametrize("d,prec_name,msgs", [(37, "fp64", CODED), (1000, "fp64", NAIVE), (1000, "fp32", CODED),
                                              (300, "fp32x64", NAIVE), (1024, "fp32x64", CODED)],
                         ids=["d37-fp64-coded", "d1000-fp64-naive", "d1000-fp32-coded", "d300-fp32x64-naive",
                              "d1024-fp32x64-coded"])
def test_block_k_is_bitwise_the_sweep_kernel_on_zeroed_rows(d, prec_name, msgs, K, native):
    """grad_folds adds 0 * x for a held-out row where grad_models adds r * 0 for a zero row; the inputs are finite."""
    prec = get_precision(prec_name)
    parts, host, betas = inputs(d, prec_name)
    beta, _ = model(betas, K)
    ld = prec.ld(d)
    for loss in LOSSES:
        plan = CvGradPlan(msgs, parts, prec, loss, K, d)
        G = plan.run(beta, plan.out_buffer()[0]).reshape(len(msgs), K, ld)
        assert bool(torch.isfinite(G).all())
        for k in range(K):
            parts_k = {}
            for p, (X, y) in parts.items():
                Xk = X.clone()
                Xk[k::K] = 0
                parts_k[p] = (Xk, y)
            sweep = MultiModelGradPlan(msgs, parts_k, prec, loss, K, d)
            Gk = sweep.run(beta, sweep.out_buffer()[0]).reshape(len(msgs), K, ld)
            torch.cuda.synchronize()
            assert torch.equal(G[:, k], Gk[:, k]), f"{LOSS_IDS[loss]} fold model {k}"


# ---- 3. the folds do not leak
@pytest.mark.parametrize("loss,poison", [(losses.LOGISTIC, float("nan")), (losses.LEAST_SQUARES, float("inf"))],
                         ids=["logistic-nan", "lsq-inf"])
@pytest.mark.parametrize("K,d", [(2, 37), (3, 1000), (5, 300), (8, 1024)])
def test_folds_do_not_leak(K, d, loss, poison, native):
    """Fold k's rows set to NaN (their labels: see the module docstring) leave model k's block finite and bitwise what
    it was, while every other model's block changes.  With least squares and a label of +inf the residual -2 (y - z) is
    -inf before the select: the select really stands behind the residual, and nothing of it reaches the FMAs."""
    prec = get_precision("fp64")
    parts, host, betas = inputs(d, "fp64")
    beta, _ = model(betas, K)
    ld = prec.ld(d)
    plan = CvGradPlan(NAIVE, parts, prec, loss, K, d)
    clean = plan.run(beta, plan.out_buffer()[0]).clone().reshape(len(NAIVE), K, ld)
    assert bool(torch.isfinite(clean).all())
    for k in range(K):
        bad = {}
        for p, (X, y) in parts.items():
            yk = y.clone()
            yk[k::K] = poison
            bad[p] = (X, yk)
        plan_k = CvGradPlan(NAIVE, bad, prec, loss, K, d)
        G = plan_k.run(beta, plan_k.out_buffer()[0]).reshape(len(NAIVE), K, ld)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(G[:, k]).all()) and torch.equal(G[:, k], clean[:, k]), f"fold {k}"
        # (the 150-row partition has rows of every fold: the other models do see the changed rows)
        assert all(not torch.equal(G[0, j], clean[0, j]) for j in range(K) if j != k)
        if loss == losses.LEAST_SQUARES:  # ... and there the poison is plain to see: -inf * x in every other model
            assert all(not bool(torch.isfinite(G[0, j, :d]).all()) for j in range(K) if j != k)


@pytest.mark.parametrize("msgs", [CODED, NAIVE], ids=["coded", "naive"])
@pytest.mark.parametrize("K,d,prec_name", [(3, 37, "fp64"), (5, 1000, "fp32x64"), (8, 300, "fp32")])
def test_changed_labels_of_fold_k_change_every_block_but_k(K, d, prec_name, msgs, native):
    """With the labels of fold k flipped the messages are the library twin's (cv_grad, here as the long-double oracle
    over the zeroed rows, whose bound the twin itself meets) on the changed data, and block k is bitwise unchanged."""
    prec = get_precision(prec_name)
    parts, host, betas = inputs(d, prec_name)
    beta, bhs = model(betas, K)
    ld = prec.ld(d)
    plan = CvGradPlan(msgs, parts, prec, losses.SQUARED_HINGE, K, d)
    clean = plan.run(beta, plan.out_buffer()[0]).clone().reshape(len(msgs), K, ld)
    k = K - 1
    flipped, host_f = {}, {}
    for p, (X, y) in parts.items():
        yk = y.clone()
        yk[k::K] = -yk[k::K]
        flipped[p] = (X, yk.contiguous())
        host_f[p] = (host[p][0], yk.double().cpu().numpy())
    plan_f = CvGradPlan(msgs, flipped, prec, losses.SQUARED_HINGE, K, d)
    G = plan_f.run(beta, plan_f.out_buffer()[0])
    torch.cuda.synchronize()
    check(G, msgs, host_f, bhs, losses.SQUARED_HINGE, prec, d, "flipped labels")
    G = G.reshape(len(msgs), K, ld)
    assert torch.equal(G[:, k], clean[:, k])
    assert all(not torch.equal(G[:, j], clean[:, j]) for j in range(K) if j != k)
    # ... and the twin itself: kernel and twin (NumPy, fp64) each meet the oracle's column bound, so they are within
    # twice that bound of each other
    got = G.double().cpu().numpy()
    for s, m in enumerate(msgs):
        twin = sum(losses.cv_grad(losses.SQUARED_HINGE, host_f[p][0], host_f[p][1], np.stack(bhs), c) for p, c in m)
        for j in range(K):
            ref, bound = oracle_message(losses.SQUARED_HINGE, m, zero_fold(host_f, K, j), bhs[j], prec)
            check_columns(twin[j], ref, bound, f"cv_grad message {s} fold model {j}")
            assert np.all(np.abs(got[s, j, :d] - twin[j]) <= 2 * bound), f"message {s} fold model {j}"


# ---- 4. closed gate
@pytest.mark.parametrize("msgs", [CODED, NAIVE], ids=["coded", "naive"])
def test_closed_gate_leaves_the_messages_untouched(msgs, native):
    prec = get_precision("fp64")
    parts, host, betas = inputs(37, "fp64")
    beta, bhs = model(betas, 3)
    plan = CvGradPlan(msgs, parts, prec, losses.LOGISTIC, 3, 37)
    L = plan.native_launcher()
    G = plan.out_buffer()[0].fill_(12345.0)
    L.launch(beta, G, gate=torch.ones(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert bool((G == 12345.0).all())
    L.launch(beta, G, gate=torch.zeros(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    check(G, msgs, host, bhs, losses.LOGISTIC, prec, 37, "open gate")


# ---- 5. launcher validation: an error, not a launch
def test_launcher_rejects_invalid_arguments(native):
    i32 = dict(dtype=torch.int32, device=DEV)
    segs = torch.zeros(32, dtype=torch.uint8, device=DEV)
    tasks, ptb = torch.zeros((0, 5), **i32), torch.zeros(1, **i32)
    buf = torch.zeros(8 * 1024, dtype=torch.float64, device=DEV)

    def call(dtype=0, loss=0, folds=3, d_x=37, ld_x=38):
        native._grad_folds_raw(dtype, loss, folds, segs, tasks, ptb, buf, buf, buf, d_x, ld_x)

    call()
    call(loss=1)
    call(loss=2)
    call(dtype=1, ld_x=40)
    call(dtype=3, ld_x=40)
    call(folds=2)
    call(folds=8, d_x=1024, ld_x=1024)
    bad = [dict(folds=1), dict(folds=9), dict(ld_x=0, d_x=0), dict(ld_x=1026, d_x=1000), dict(d_x=0), dict(d_x=39),
           dict(ld_x=37, d_x=37), dict(dtype=1, ld_x=38), dict(dtype=3, ld_x=38), dict(dtype=2, ld_x=40), dict(dtype=4),
           dict(dtype=-1), dict(loss=3), dict(loss=4), dict(loss=5), dict(loss=-1)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="invalid"):
            call(**kw)
    torch.cuda.synchronize()
    # the plan's limits: ValueErrors from the constructor, before any launch
    prec = get_precision("fp64")
    parts, _, _ = inputs(37, "fp64")
    for K in (1, 9):
        with pytest.raises(ValueError, match="2..8"):
            CvGradPlan(NAIVE, parts, prec, losses.LOGISTIC, K, 37)
    y4 = torch.tensor([1.0, -1.0, 1.0, -1.0], dtype=torch.float64, device=DEV)
    wide = {0: (torch.zeros((4, 1026), dtype=torch.float64, device=DEV), y4)}
    with pytest.raises(ValueError, match="--cv.*1024"):
        CvGradPlan([[(0, 1.0)]], wide, prec, losses.LOGISTIC, 2, 1025)
    with pytest.raises((RuntimeError, ValueError), match="cross-validation"):  # the native plan validator names itself
        native.GradLauncher.folds(0, 3, 3, segs, tasks, buf, ptb, 37, 38)
    with pytest.raises((RuntimeError, ValueError), match="cross-validation"):
        native.GradLauncher.folds(2, 0, 3, segs, tasks, buf, ptb, 37, 38)


# ---- 6. the engine on the GPU against the CPU engine
def _run(dev, case, rule, K=3, device_loop="auto", **kw):
    cfg, src, sch, parts = make(case, rule, K, **kw)
    cfg.device_loop = device_loop
    tr = Trainer(cfg, DistEnv(device=torch.device(dev)) if dev == "cuda" else DistEnv(), src, scheme=sch)
    res = tr.run()
    return tr, res, evaluate(tr, res, write=False)


def _arrival_sets(res):
    return [[(w, p) for (w, p, _t) in r] for r in res.arrivals]


SCORES = ("training_loss", "testing_loss", "auc", "cv_loss_folds", "cv_loss", "cv_std")


@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_engine_matches_cpu_engine(name, rule, native):
    tg, rg, eg = _run("cuda", CASES[name], rule)
    assert tg.native_loop and isinstance(tg.plan, CvGradPlan) and tg.cv == 3
    assert tg.rank_report()["round_loop"] != "arbiter"
    tc, rc, ec = _run("cpu", CASES[name], rule)
    np.testing.assert_allclose(rg.betaset, rc.betaset, **TOL)
    assert _arrival_sets(rg) == _arrival_sets(rc)
    for what in SCORES:
        np.testing.assert_allclose(getattr(eg, what), getattr(ec, what), rtol=1e-9, atol=1e-11, err_msg=what)
    assert np.all(rg.betaset.reshape(-1, 3, tg.ld_x)[:, :, tg.d_x:] == 0.0)


@pytest.mark.parametrize("prec_name", ["fp32", "fp32x64"])
def test_gpu_engine_in_the_fp32_storage_precisions(prec_name, native):
    """fp32x64 keeps the fp64 tolerance against its CPU run (the same stored values, fp64 arithmetic); fp32 is held
    to the project's fp32 engine tolerance, 2e-4 of the largest entry (tests/test_engine_gpu.py)."""
    tg, rg, _ = _run("cuda", CASES["agc_uneven"], "AGD", precision=prec_name)
    tc, rc, _ = _run("cpu", CASES["agc_uneven"], "AGD", precision=prec_name)
    if prec_name == "fp32x64":
        np.testing.assert_allclose(rg.betaset, rc.betaset, **TOL)
    else:
        err = np.max(np.abs(rg.betaset - rc.betaset)) / np.max(np.abs(rc.betaset))
        print("fp32 GPU against CPU: relative to the largest entry", err)
        assert err < 2e-4, err
    assert np.all(rg.betaset.reshape(-1, 3, tg.ld_x)[:, :, tg.d_x:] == 0.0)


@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_gpu_engine_with_l1(rule, native):
    tg, rg, eg = _run("cuda", CASES["cyclic"], rule, l1=0.02)
    tc, rc, ec = _run("cpu", CASES["cyclic"], rule, l1=0.02)
    assert tg.prox
    np.testing.assert_allclose(rg.betaset, rc.betaset, **TOL)
    np.testing.assert_array_equal(eg.nnz, ec.nnz)
    assert 0 < np.count_nonzero(rg.betaset[-1] == 0.0)


@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_device_loops_agree_bitwise(rule, native):
    ts, rs, _ = _run("cuda", CASES["agc_uneven"], rule, 5, "stream", loss="squared_hinge", lr=0.1)
    to, ro, _ = _run("cuda", CASES["agc_uneven"], rule, 5, "off", loss="squared_hinge", lr=0.1)
    assert ts.device_loop == "stream" and to.device_loop is None
    np.testing.assert_array_equal(rs.betaset, ro.betaset)
    tg, rg, _ = _run("cuda", CASES["agc_uneven"], rule, 5, "graph", loss="squared_hinge", lr=0.1)
    assert tg.device_loop == "graph"
    np.testing.assert_array_equal(rg.betaset, ro.betaset)


# ---- 7. three ranks sharing the GPU over the IPC mailbox
def test_three_ranks_over_ipc_match_the_replay(tmp_path, native):
    out = str(tmp_path / "cv_ipc.npz")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", EH_CV_OUT=out, EH_CV_DEVICE="cuda")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr",
           "127.0.0.1", f"--master-port={port}", os.path.join(HERE, "mp_cv_run.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out, allow_pickle=True)
    assert str(z["transport"]) == "ipc"
    check_against_replay(z)
