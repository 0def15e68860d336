"""The one-vs-rest gradient kernel (csrc/kernels/grad_ovr.hip) and --ovr runs of the engine on the GPU (GPU only).

The kernel is held to the long-double oracle and the per-column bounds of tests/numerics.py with the project's
K = 8, on the hostile inputs of tests/test_multimodel_gpu.py with the labels replaced by class indices and an
independent hostile beta per class: block k of every message against ``oracle_message(loss, segments, host_k,
beta_k, prec)``, host_k the host data with the labels relabelled to +-1 for class k.  Partitions of [257, 64, 1, 0]
rows: several stages, a ragged last stage, a one-row task and an empty partition; in the 64-row partition class
C - 1 never occurs, so one model sees only -1 there.  Block k is also bitwise the sweep kernel's block k on the
relabelled data: the two kernels are one text.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from erasurehead_amd.engine import Trainer, evaluate
from erasurehead_amd.models import losses
from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.multimodel import MultiModelGradPlan
from erasurehead_amd.ops.ovr import OvrGradPlan
from erasurehead_amd.parallel.dist import DistEnv
import block_edge_cases as bc
from numerics import LOSS_IDS, check_columns, hostile_beta, hostile_partition, oracle_message
from test_multimodel_cpu import TOL
from test_ovr_cpu import CASES, check_against_replay, make

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [257, 64, 1, 0]
CODED = [[(0, 1.0), (1, -0.7)], [(2, 2.5), (3, 1.0)], [(1, 1.0), (0, 0.3), (2, 1.0)]]  # a cyclic row: the encode path
NAIVE = [[(0, 1.0)], [(1, 1.0)], [(2, 1.0)], [(3, 1.0)]]  # the identity path
CLASSES = [2, 3, 4, 5, 8]  # wpg 4, 2, 2, 1, 1; an idle fourth wave at 5; an inactive second model at odd C
OVR_LOSSES = (losses.LOGISTIC, losses.SQUARED_HINGE)
# the full cross at d = 37 and 1000; the other widths (both CPL edges, the clamped tail read, the full width)
# with logistic fp64 and fp32
GRID = [(d, loss, p) for d in (37, 1000) for loss in OVR_LOSSES for p in ("fp64", "fp32", "fp32x64")] + \
       [(d, losses.LOGISTIC, p) for d in (1, 256, 257, 512, 513, 1024) for p in ("fp64", "fp32")]

_rows, _inputs = {}, {}


def inputs(d, prec_name, C):
    """(partitions on the device with class-index labels, host X and class indices, 8 hostile betas): the rows and
    betas drawn once per (d, precision), the labels once per (d, precision, C); never changed."""
    prec = get_precision(prec_name)
    if (d, prec_name) not in _rows:
        rng = np.random.RandomState(1000 + d)
        rows = [hostile_partition(rng, n, d, prec) for n in SIZES]
        _rows[(d, prec_name)] = ([Xs.to(DEV).contiguous() for Xs, _, _ in rows], [Xh for _, _, Xh in rows],
                                 [hostile_beta(rng, d, prec) for _ in range(8)])
    key = (d, prec_name, C)
    if key not in _inputs:
        Xd, Xh, betas = _rows[(d, prec_name)]
        rng = np.random.RandomState(7000 + 10 * d + C)
        parts, host = {}, {}
        for p, n in enumerate(SIZES):
            y = rng.randint(0, C, n).astype(np.float64)
            if n == 64:
                y[y == C - 1] = 0.0  # class C - 1 is absent here: its model sees only -1
            parts[p] = (Xd[p], torch.from_numpy(y).to(prec.acc).to(DEV).contiguous())
            host[p] = (Xh[p], y)
        _inputs[key] = (parts, host, betas)
    return _inputs[key]


def relabel(host, k):
    """The host data as model k sees it: +1 for class k, -1 for the rest."""
    return {p: (X, np.where(y == k, 1.0, -1.0)) for p, (X, y) in host.items()}


def model(betas, C):
    """The flattened [C][ld] model on the device and the fp64 view of every block."""
    return torch.cat([b for b, _ in betas[:C]]).to(DEV), [bh for _, bh in betas[:C]]


def check(G, msgs, host, bhs, loss, prec, d, what):
    C, ld = len(bhs), prec.ld(d)
    got = G.double().cpu().numpy().reshape(len(msgs), C, ld)
    for k in range(C):
        host_k = relabel(host, k)
        for s, m in enumerate(msgs):
            ref, bound = oracle_message(loss, m, host_k, bhs[k], prec)
            check_columns(got[s, k, :d], ref, bound, f"{what} message {s} class {k}")
    assert np.all(got[:, :, d:] == 0.0), f"{what}: padding columns must be exact zeros"


# ---- 1. the kernel against the long-double oracle
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("d,loss,prec_name", GRID, ids=[f"d{d}-{LOSS_IDS[l]}-{p}" for d, l, p in GRID])
def test_kernel_within_the_column_bounds(d, loss, prec_name, C, native):
    prec = get_precision(prec_name)
    parts, host, betas = inputs(d, prec_name, C)
    assert not bool((parts[1][1] == C - 1).any()) and bool((parts[0][1] == C - 1).any())
    beta, bhs = model(betas, C)
    for msgs in (NAIVE, CODED):
        plan = OvrGradPlan(msgs, parts, prec, loss, C, d)
        assert plan.identity == (msgs is NAIVE) and plan.ld == C * prec.ld(d) and plan.ntasks >= 8
        G = plan.out_buffer()[0].fill_(float("nan"))  # every element, padding included, must be overwritten
        plan.run(beta, G)
        G2 = plan.out_buffer()[0].fill_(float("nan"))
        plan.native_launcher().launch(beta, G2)
        torch.cuda.synchronize()
        check(G, msgs, host, bhs, loss, prec, d, f"{'naive' if msgs is NAIVE else 'coded'} C={C}")
        assert torch.equal(G, G2)  # two launches: bitwise identical


# ---- 1b. stage edges: ragged stages of every row count, ring reuse, tasks that start at odd rows
STAGE_GRID = bc.scalar_grid(OVR_LOSSES)
_edge_inputs = {}


def edge_inputs(d, prec_name, C):
    """The rows and betas of block_edge_cases.scalar_inputs with class-index labels (drawn once, never changed); the
    partition of exactly one full stage has no row of class C - 1."""
    key = (d, prec_name, C)
    if key not in _edge_inputs:
        prec = get_precision(prec_name)
        sizes, cpu_parts, host, betas = bc.scalar_inputs(d, prec_name, C)
        rng = np.random.RandomState(7000 + 10 * d + C)
        lacks = bc.lacking_partition(sizes, bc.geometry(prec, d, C)[0])
        parts, hostc = {}, {}
        for p, n in enumerate(sizes):
            y = rng.randint(0, C, n).astype(np.float64)
            if p == lacks:
                y[y == C - 1] = 0.0
            parts[p] = (cpu_parts[p][0].to(DEV).contiguous(), torch.from_numpy(y).to(prec.acc).to(DEV).contiguous())
            hostc[p] = (host[p][0], y)
        _edge_inputs[key] = (sizes, parts, hostc, betas)
    return _edge_inputs[key]


@pytest.mark.parametrize("C", bc.SCALAR_BLOCKS)
@pytest.mark.parametrize("d,loss,prec_name", STAGE_GRID, ids=[f"d{d}-{LOSS_IDS[l]}-{p}" for d, l, p in STAGE_GRID])
def test_stage_edges_within_the_column_bounds(d, loss, prec_name, C, native, monkeypatch):
    """Partitions of tests/block_edge_cases.py partition_sizes (every ragged stage around a row per wave and the full
    stage, S + 1, 2S, 2S + 1, 3S + 2, empty), once as whole tasks of three and four stages and once cut into tasks of
    37 rows, naive and coded messages; the same oracle, bound and checks as above."""
    prec = get_precision(prec_name)
    sizes, parts, host, betas = edge_inputs(d, prec_name, C)
    beta, bhs = model(betas, C)
    for rows in bc.TASK_ROWS:
        bc.forced_task_rows(monkeypatch, rows)
        for kind in ("naive", "coded"):
            msgs = bc.MESSAGES[kind](len(sizes))
            plan = OvrGradPlan(msgs, parts, prec, loss, C, d)
            assert plan.identity == (kind == "naive")
            bc.assert_tasks_reach_the_edges(plan, sizes, bc.geometry(prec, d, C)[0], rows)
            G = plan.out_buffer()[0].fill_(float("nan"))
            plan.run(beta, G)
            G2 = plan.out_buffer()[0].fill_(float("nan"))
            plan.native_launcher().launch(beta, G2)
            torch.cuda.synchronize()
            check(G, msgs, host, bhs, loss, prec, d, f"{kind} C={C} tasks of {rows}")
            assert torch.equal(G, G2)  # two launches: bitwise identical


# ---- 2. bitwise the sweep kernel on the relabelled data: the same task table, wave layout and FMA order
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("d,prec_name,msgs", [(37, "fp64", CODED), (1000, "fp64", NAIVE), (1000, "fp32", CODED),
                                              (37, "fp32x64", NAIVE), (513, "fp32x64", CODED)],
                         ids=["d37-fp64-coded", "d1000-fp64-naive", "d1000-fp32-coded", "d37-fp32x64-naive",
                              "d513-fp32x64-coded"])
def test_block_k_is_bitwise_the_sweep_kernel_on_relabelled_data(d, prec_name, msgs, C, native):
    prec = get_precision(prec_name)
    parts, host, betas = inputs(d, prec_name, C)
    beta, _ = model(betas, C)
    ld = prec.ld(d)
    for loss in OVR_LOSSES:
        plan = OvrGradPlan(msgs, parts, prec, loss, C, d)
        G = plan.run(beta, plan.out_buffer()[0]).reshape(len(msgs), C, ld)
        one, neg = torch.ones_like(parts[0][1][:1]), -torch.ones_like(parts[0][1][:1])
        for k in range(C):
            parts_k = {p: (X, torch.where(y == k, one, neg).contiguous()) for p, (X, y) in parts.items()}
            sweep = MultiModelGradPlan(msgs, parts_k, prec, loss, C, d)
            Gk = sweep.run(beta, sweep.out_buffer()[0]).reshape(len(msgs), C, ld)
            torch.cuda.synchronize()
            assert torch.equal(G[:, k], Gk[:, k]), f"{LOSS_IDS[loss]} class {k}"


def test_classes_do_not_leak_into_each_other(native):
    """Block k depends on beta block k alone: changing another class's beta leaves it bitwise unchanged."""
    prec = get_precision("fp64")
    parts, host, betas = inputs(37, "fp64", 5)
    plan = OvrGradPlan(CODED, parts, prec, losses.LOGISTIC, 5, 37)
    beta, _ = model(betas, 5)
    G = plan.run(beta, plan.out_buffer()[0]).clone()
    ld = prec.ld(37)
    beta2 = beta.clone()
    beta2[3 * ld: 4 * ld] = betas[7][0].to(DEV)
    G2 = plan.run(beta2, plan.out_buffer()[0])
    torch.cuda.synchronize()
    keep = [k for k in range(5) if k != 3]
    a, b = G.reshape(3, 5, ld), G2.reshape(3, 5, ld)
    assert torch.equal(a[:, keep], b[:, keep]) and not torch.equal(a[:, 3], b[:, 3])


# ---- 3. closed gate
@pytest.mark.parametrize("msgs", [CODED, NAIVE], ids=["coded", "naive"])
def test_closed_gate_leaves_the_messages_untouched(msgs, native):
    prec = get_precision("fp64")
    parts, host, betas = inputs(37, "fp64", 3)
    beta, bhs = model(betas, 3)
    plan = OvrGradPlan(msgs, parts, prec, losses.LOGISTIC, 3, 37)
    L = plan.native_launcher()
    G = plan.out_buffer()[0].fill_(12345.0)
    L.launch(beta, G, gate=torch.ones(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert bool((G == 12345.0).all())
    L.launch(beta, G, gate=torch.zeros(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    check(G, msgs, host, bhs, losses.LOGISTIC, prec, 37, "open gate")


# ---- 4. launcher validation: an error, not a launch
def test_launcher_rejects_invalid_arguments(native):
    i32 = dict(dtype=torch.int32, device=DEV)
    segs = torch.zeros(32, dtype=torch.uint8, device=DEV)
    tasks, ptb = torch.zeros((0, 5), **i32), torch.zeros(1, **i32)
    buf = torch.zeros(8 * 1024, dtype=torch.float64, device=DEV)

    def call(dtype=0, loss=0, classes=3, d_x=37, ld_x=38):
        native._grad_ovr_raw(dtype, loss, classes, segs, tasks, ptb, buf, buf, buf, d_x, ld_x)

    call()
    call(loss=2)
    call(dtype=1, ld_x=40)
    call(dtype=3, ld_x=40)
    call(classes=2)
    call(classes=8, d_x=1024, ld_x=1024)
    bad = [dict(classes=1), dict(classes=9), dict(ld_x=0, d_x=0), dict(ld_x=1026, d_x=1000), dict(d_x=0), dict(d_x=39),
           dict(ld_x=37, d_x=37), dict(dtype=1, ld_x=38), dict(dtype=3, ld_x=38), dict(dtype=2, ld_x=40), dict(dtype=4),
           dict(dtype=-1), dict(loss=1), dict(loss=3), dict(loss=4), dict(loss=5), dict(loss=-1)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="invalid"):
            call(**kw)
    torch.cuda.synchronize()
    # the plan's limits: ValueErrors from the constructor, before any launch
    prec = get_precision("fp64")
    parts, _, _ = inputs(37, "fp64", 3)
    for C in (1, 9):
        with pytest.raises(ValueError, match="2..8"):
            OvrGradPlan(NAIVE, parts, prec, losses.LOGISTIC, C, 37)
    y4 = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64, device=DEV)
    wide = {0: (torch.zeros((4, 1026), dtype=torch.float64, device=DEV), y4)}
    with pytest.raises(ValueError, match="1024"):
        OvrGradPlan([[(0, 1.0)]], wide, prec, losses.LOGISTIC, 2, 1025)
    X6 = torch.zeros((4, 6), dtype=torch.float64, device=DEV)
    for lab in ([0.0, 1.0, 3.0, 2.0], [0.0, 1.5, 1.0, 2.0]):  # a label equal to C; a non-integer label
        yb = torch.tensor(lab, dtype=torch.float64, device=DEV)
        with pytest.raises(ValueError, match="partition 0"):
            OvrGradPlan([[(0, 1.0)]], {0: (X6, yb)}, prec, losses.LOGISTIC, 3, 6)
    with pytest.raises((RuntimeError, ValueError), match="one-vs-rest"):  # the native plan validator names itself
        native.GradLauncher.ovr(0, 1, 3, segs, tasks, buf, ptb, 37, 38)


# ---- 5. the engine on the GPU against the CPU engine
def _run(dev, case, rule, loss, device_loop="auto", **kw):
    cfg, src, sch, parts = make(case, rule, loss, **kw)
    cfg.device_loop = device_loop
    tr = Trainer(cfg, DistEnv(device=torch.device(dev)) if dev == "cuda" else DistEnv(), src, scheme=sch)
    res = tr.run()
    return tr, res, evaluate(tr, res, write=False)


def _arrival_sets(res):
    return [[(w, p) for (w, p, _t) in r] for r in res.arrivals]


@pytest.mark.parametrize("loss", ["logistic", "squared_hinge"])
@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_engine_matches_cpu_engine(name, rule, loss, native):
    tg, rg, eg = _run("cuda", CASES[name], rule, loss)
    assert tg.native_loop and isinstance(tg.plan, OvrGradPlan) and tg.ovr and tg.loss == losses.LOSS_NAMES[loss]
    tc, rc, ec = _run("cpu", CASES[name], rule, loss)
    np.testing.assert_allclose(rg.betaset, rc.betaset, **TOL)
    assert _arrival_sets(rg) == _arrival_sets(rc)
    for what in ("training_loss", "testing_loss", "auc"):  # auc: the accuracy of a one-vs-rest run
        np.testing.assert_allclose(getattr(eg, what), getattr(ec, what), **TOL)
    assert np.all(rg.betaset.reshape(-1, 3, tg.ld_x)[:, :, tg.d_x:] == 0.0)


@pytest.mark.parametrize("prec_name", ["fp32", "fp32x64"])
def test_gpu_engine_in_the_fp32_storage_precisions(prec_name, native):
    """fp32x64 keeps the fp64 tolerance against its CPU run (the same stored values, fp64 arithmetic); fp32 is held
    to the project's fp32 engine tolerance, 2e-4 of the largest entry (tests/test_engine_gpu.py)."""
    tg, rg, _ = _run("cuda", CASES["agc_uneven"], "AGD", "logistic", precision=prec_name)
    tc, rc, _ = _run("cpu", CASES["agc_uneven"], "AGD", "logistic", precision=prec_name)
    if prec_name == "fp32x64":
        np.testing.assert_allclose(rg.betaset, rc.betaset, **TOL)
    else:
        err = np.max(np.abs(rg.betaset - rc.betaset)) / np.max(np.abs(rc.betaset))
        print("fp32 GPU against CPU: relative to the largest entry", err)
        assert err < 2e-4, err
    assert np.all(rg.betaset.reshape(-1, 3, tg.ld_x)[:, :, tg.d_x:] == 0.0)


@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_device_loops_agree_bitwise(rule, native):
    ts, rs, _ = _run("cuda", CASES["agc_uneven"], rule, "squared_hinge", "stream")
    to, ro, _ = _run("cuda", CASES["agc_uneven"], rule, "squared_hinge", "off")
    assert ts.device_loop == "stream" and to.device_loop is None
    np.testing.assert_array_equal(rs.betaset, ro.betaset)
    tg, rg, _ = _run("cuda", CASES["agc_uneven"], rule, "squared_hinge", "graph")
    assert tg.device_loop == "graph"
    np.testing.assert_array_equal(rg.betaset, ro.betaset)


def test_gpu_engine_eight_classes_headline_width(native):
    kw = dict(C=8, d=1000, rounds=3)  # D = 8 * 1000 = 8000
    tg, rg, eg = _run("cuda", CASES["naive"], "GD", "logistic", "graph", **kw)
    tc, rc, ec = _run("cpu", CASES["naive"], "GD", "logistic", **kw)
    assert rg.betaset.shape == (3, 8000)
    np.testing.assert_allclose(rg.betaset, rc.betaset, **TOL)
    for what in ("training_loss", "testing_loss", "auc"):
        np.testing.assert_allclose(getattr(eg, what), getattr(ec, what), **TOL)


# ---- 6. three ranks sharing the GPU over the IPC mailbox
def test_three_ranks_over_ipc_match_the_replay(tmp_path, native):
    out = str(tmp_path / "ovr_ipc.npz")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", EH_OVR_OUT=out, EH_OVR_DEVICE="cuda")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr",
           "127.0.0.1", f"--master-port={port}", os.path.join(HERE, "mp_ovr_run.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out, allow_pickle=True)
    assert str(z["transport"]) == "ipc"
    assert np.all(np.asarray(z["betaset"]).reshape(-1, 3, 34)[:, :, 33:] == 0.0)
    check_against_replay(z)
