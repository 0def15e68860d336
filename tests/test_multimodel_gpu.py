"""The multi-model gradient kernel (csrc/kernels/grad_multimodel.hip), the per-block update
(csrc/kernels/update.hip combine_update_blocks) and sweep runs of the engine on the GPU (GPU only).

The kernel is held to the long-double oracle and the per-column bounds of tests/numerics.py with the project's
K = 8, on hostile inputs with an independent hostile beta per model: block k of every message against
``oracle_message(loss, segments, host, beta_k, prec)``.  Partitions of [257, 64, 1, 0] rows: several stages, a
ragged last stage, a one-row task and an empty partition.
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
from erasurehead_amd.ops.update import combine_update, combine_update_blocks
from erasurehead_amd.parallel.dist import DistEnv
import block_edge_cases as bc
from numerics import LOSS_IDS, LOSSES, check_columns, hostile_beta, hostile_partition, oracle_message
from test_multimodel_cpu import ALPHAS, CASES, LRS, TOL, arrival_sets, check_against_replay, make

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [257, 64, 1, 0]
CODED = [[(0, 1.0), (1, -0.7)], [(2, 2.5), (3, 1.0)], [(1, 1.0), (0, 0.3), (2, 1.0)]]  # a cyclic row: the encode path
NAIVE = [[(0, 1.0)], [(1, 1.0)], [(2, 1.0)], [(3, 1.0)]]  # the identity path
MODELS = [2, 3, 4, 5, 8]  # wpg 4, 2, 2, 1, 1; an idle fourth wave at 5; an inactive second model at odd M
# the full cross at d = 37 and 1000; the other widths (both CPL edges, the clamped tail read, the full width)
# with logistic fp64 and fp32
GRID = [(d, loss, p) for d in (37, 1000) for loss in LOSSES for p in ("fp64", "fp32", "fp32x64")] + \
       [(d, LOSSES[0], p) for d in (1, 256, 257, 512, 513, 1024) for p in ("fp64", "fp32")]

_inputs = {}


def inputs(d, prec_name):
    """(partitions on the device, host copies, 8 hostile betas): drawn once per (d, precision), never changed."""
    key = (d, prec_name)
    if key not in _inputs:
        prec = get_precision(prec_name)
        rng = np.random.RandomState(1000 + d)
        parts, host = {}, {}
        for p, n in enumerate(SIZES):
            Xs, y, Xh = hostile_partition(rng, n, d, prec)
            parts[p] = (Xs.to(DEV).contiguous(), y.to(DEV).contiguous())
            host[p] = (Xh, y.double().numpy())
        betas = [hostile_beta(rng, d, prec) for _ in range(8)]
        _inputs[key] = (parts, host, betas)
    return _inputs[key]


def model(betas, M):
    """The flattened [M][ld] model on the device and the fp64 view of every block."""
    return torch.cat([b for b, _ in betas[:M]]).to(DEV), [bh for _, bh in betas[:M]]


def check(G, msgs, host, bhs, loss, prec, d, what):
    M, ld = len(bhs), prec.ld(d)
    got = G.double().cpu().numpy().reshape(len(msgs), M, ld)
    for s, m in enumerate(msgs):
        for k in range(M):
            ref, bound = oracle_message(loss, m, host, bhs[k], prec)
            check_columns(got[s, k, :d], ref, bound, f"{what} message {s} model {k}")
    assert np.all(got[:, :, d:] == 0.0), f"{what}: padding columns must be exact zeros"


# ---- 1. the kernel against the long-double oracle
@pytest.mark.parametrize("M", MODELS)
@pytest.mark.parametrize("d,loss,prec_name", GRID, ids=[f"d{d}-{LOSS_IDS[l]}-{p}" for d, l, p in GRID])
def test_kernel_within_the_column_bounds(d, loss, prec_name, M, native):
    prec = get_precision(prec_name)
    parts, host, betas = inputs(d, prec_name)
    beta, bhs = model(betas, M)
    for msgs in (NAIVE, CODED):
        plan = MultiModelGradPlan(msgs, parts, prec, loss, M, d)
        assert plan.identity == (msgs is NAIVE) and plan.ld == M * prec.ld(d) and plan.ntasks >= 8
        G = plan.out_buffer()[0].fill_(float("nan"))  # every element, padding included, must be overwritten
        plan.run(beta, G)
        G2 = plan.out_buffer()[0].fill_(float("nan"))
        plan.native_launcher().launch(beta, G2)
        torch.cuda.synchronize()
        check(G, msgs, host, bhs, loss, prec, d, f"{'naive' if msgs is NAIVE else 'coded'} M={M}")
        assert torch.equal(G, G2)  # two launches: bitwise identical


# ---- 1b. stage edges: ragged stages of every row count, ring reuse, tasks that start at odd rows
STAGE_GRID = bc.scalar_grid(LOSSES)
_edge_parts = {}


@pytest.mark.parametrize("M", bc.SCALAR_BLOCKS)
@pytest.mark.parametrize("d,loss,prec_name", STAGE_GRID, ids=[f"d{d}-{LOSS_IDS[l]}-{p}" for d, l, p in STAGE_GRID])
def test_stage_edges_within_the_column_bounds(d, loss, prec_name, M, native, monkeypatch):
    """Partitions of tests/block_edge_cases.py partition_sizes (every ragged stage around a row per wave and the full
    stage, S + 1, 2S, 2S + 1, 3S + 2, empty), once as whole tasks of three and four stages and once cut into tasks of
    37 rows, naive and coded messages; the same oracle, bound and checks as above."""
    prec = get_precision(prec_name)
    sizes, cpu_parts, host, betas = bc.scalar_inputs(d, prec_name, M)
    if (d, prec_name, M) not in _edge_parts:
        _edge_parts[(d, prec_name, M)] = bc.to_device(cpu_parts, DEV)
    parts = _edge_parts[(d, prec_name, M)]
    beta, bhs = model(betas, M)
    for rows in bc.TASK_ROWS:
        bc.forced_task_rows(monkeypatch, rows)
        for kind in ("naive", "coded"):
            msgs = bc.MESSAGES[kind](len(sizes))
            plan = MultiModelGradPlan(msgs, parts, prec, loss, M, d)
            assert plan.identity == (kind == "naive")
            bc.assert_tasks_reach_the_edges(plan, sizes, bc.geometry(prec, d, M)[0], rows)
            G = plan.out_buffer()[0].fill_(float("nan"))
            plan.run(beta, G)
            G2 = plan.out_buffer()[0].fill_(float("nan"))
            plan.native_launcher().launch(beta, G2)
            torch.cuda.synchronize()
            check(G, msgs, host, bhs, loss, prec, d, f"{kind} M={M} tasks of {rows}")
            assert torch.equal(G, G2)  # two launches: bitwise identical


def test_models_do_not_leak_into_each_other(native):
    """Block k depends on beta block k alone: changing another model's beta leaves it bitwise unchanged."""
    prec = get_precision("fp64")
    parts, host, betas = inputs(37, "fp64")
    plan = MultiModelGradPlan(CODED, parts, prec, LOSSES[0], 5, 37)
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


# ---- 2. closed gate
@pytest.mark.parametrize("msgs", [CODED, NAIVE], ids=["coded", "naive"])
def test_closed_gate_leaves_the_messages_untouched(msgs, native):
    prec = get_precision("fp64")
    parts, host, betas = inputs(37, "fp64")
    beta, bhs = model(betas, 3)
    plan = MultiModelGradPlan(msgs, parts, prec, LOSSES[0], 3, 37)
    L = plan.native_launcher()
    G = plan.out_buffer()[0].fill_(12345.0)
    L.launch(beta, G, gate=torch.ones(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert bool((G == 12345.0).all())
    L.launch(beta, G, gate=torch.zeros(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    check(G, msgs, host, bhs, LOSSES[0], prec, 37, "open gate")


# ---- 3. launcher validation: an error, not a launch
def test_launcher_rejects_invalid_arguments(native):
    i32 = dict(dtype=torch.int32, device=DEV)
    segs = torch.zeros(32, dtype=torch.uint8, device=DEV)
    tasks, ptb = torch.zeros((0, 5), **i32), torch.zeros(1, **i32)
    buf = torch.zeros(8 * 1024, dtype=torch.float64, device=DEV)

    def call(dtype=0, loss=0, models=3, d_x=37, ld_x=38):
        native._grad_models_raw(dtype, loss, models, segs, tasks, ptb, buf, buf, buf, d_x, ld_x)

    call()
    call(dtype=1, ld_x=40)
    call(dtype=3, ld_x=40)
    call(models=2)
    call(models=8, d_x=1024, ld_x=1024)
    bad = [dict(models=1), dict(models=9), dict(ld_x=0, d_x=0), dict(ld_x=1026, d_x=1000), dict(d_x=0), dict(d_x=39),
           dict(ld_x=37, d_x=37), dict(dtype=1, ld_x=38), dict(dtype=3, ld_x=38), dict(dtype=2, ld_x=40), dict(dtype=4),
           dict(dtype=-1), dict(loss=3), dict(loss=-1)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="invalid"):
            call(**kw)
    torch.cuda.synchronize()
    # the plan's limits: ValueErrors from the constructor, before any launch
    prec = get_precision("fp64")
    parts, _, _ = inputs(37, "fp64")
    for M in (1, 9):
        with pytest.raises(ValueError, match="2..8"):
            MultiModelGradPlan(NAIVE, parts, prec, LOSSES[0], M, 37)
    wide = {0: (torch.zeros((4, 1026), dtype=torch.float64, device=DEV), torch.ones(4, dtype=torch.float64, device=DEV))}
    with pytest.raises(ValueError, match="1024"):
        MultiModelGradPlan([[(0, 1.0)]], wide, prec, LOSSES[0], 2, 1025)


# ---- 4. the per-block update: bitwise combine_update on every block
@pytest.mark.parametrize("nmsg", [1, 8, 9])  # nine crosses the batch of eight
@pytest.mark.parametrize("w_dtype", [torch.float64, torch.float32], ids=["w64", "w32"])
@pytest.mark.parametrize("m_dtype", [torch.float64, torch.float32], ids=["m64", "m32"])
@pytest.mark.parametrize("rule", [0, 1], ids=["GD", "AGD"])
def test_block_update_is_combine_update_per_block(rule, m_dtype, w_dtype, nmsg, native):
    rng = np.random.RandomState(10 * nmsg + rule)
    M, bl, dx = 5, 72, 67  # d_x < block_ld: padding in every block; blocks that straddle workgroups of 256
    msgs = [torch.from_numpy(losses.sweep_pack(rng.randn(M, dx), bl)).to(m_dtype).to(DEV) for _ in range(nmsg)]
    coefs = list(rng.randn(nmsg))
    decay, gm, l2 = list(1.0 - rng.rand(M) * 0.1), list(rng.rand(M) * 0.1), list(rng.rand(M) * 0.1)
    beta0 = torch.from_numpy(losses.sweep_pack(rng.randn(M, dx), bl)).to(DEV)
    u0 = torch.from_numpy(losses.sweep_pack(rng.randn(M, dx), bl)).to(DEV)
    beta, u = beta0.clone(), u0.clone()
    hist = torch.zeros(M * bl, dtype=torch.float64, device=DEV)
    bw = torch.full((M * bl,), float("nan"), dtype=w_dtype, device=DEV)
    g = torch.zeros(M * bl, dtype=torch.float64, device=DEV)
    combine_update_blocks(msgs, coefs, beta, u, bl, dx, decay, gm, l2, 0.4, rule, hist=hist, beta_w=bw, g_out=g)
    torch.cuda.synchronize()
    for k in range(M):
        s = slice(k * bl, (k + 1) * bl)
        b1, u1 = beta0[s].clone(), u0[s].clone()
        h1 = torch.zeros(bl, dtype=torch.float64, device=DEV)
        w1 = torch.full((bl,), float("nan"), dtype=w_dtype, device=DEV)
        g1 = torch.zeros(bl, dtype=torch.float64, device=DEV)
        combine_update([m[s].contiguous() for m in msgs], coefs, b1, u1, dx, decay[k], gm[k], l2[k], 0.4, rule,
                       hist=h1, beta_w=w1, g_out=g1)
        torch.cuda.synchronize()
        for got, ref in ((beta[s], b1), (u[s], u1), (hist[s], h1), (bw[s], w1), (g[s], g1)):
            assert torch.equal(got, ref), k
        assert bool((beta[s][dx:] == 0).all()) and bool((bw[s][dx:] == 0).all())


# ---- 5. the engine on the GPU
def _gpu_run(name, rule, device_loop="auto", **kw):
    cfg, src, sch, parts = make(CASES[name], rule, **kw)
    cfg.device_loop = device_loop
    tr = Trainer(cfg, DistEnv(device=torch.device(DEV)), src, scheme=sch)
    res = tr.run()
    return tr, res, evaluate(tr, res, write=False)


@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_sweep_matches_cpu_sweep_and_single_gpu_runs(name, rule, native):
    sweep = dict(sweep_alpha=ALPHAS, sweep_lr=LRS)
    tg, rg, eg = _gpu_run(name, rule, **sweep)
    assert tg.native_loop and isinstance(tg.plan, MultiModelGradPlan)
    assert tg.rank_report()["round_loop"] != "arbiter"
    cfg, src, sch, parts = make(CASES[name], rule, **sweep)
    tc = Trainer(cfg, DistEnv(), src, scheme=sch)
    rc = tc.run()
    ec = evaluate(tc, rc, write=False)
    np.testing.assert_allclose(rg.betaset, rc.betaset, **TOL)
    assert arrival_sets(rg) == arrival_sets(rc)
    for what in ("training_loss", "testing_loss", "auc"):
        np.testing.assert_allclose(getattr(eg, what), getattr(ec, what), **TOL)
    assert eg.best == ec.best
    got = losses.sweep_unpack(rg.betaset, 3, tg.d_x)
    assert np.all(rg.betaset.reshape(-1, 3, tg.ld_x)[:, :, tg.d_x:] == 0.0)
    for k in range(3):
        t1, r1, e1 = _gpu_run(name, rule, alpha=ALPHAS[k], lr=LRS[k])
        np.testing.assert_allclose(got[:, k], r1.betaset, **TOL)
        assert arrival_sets(rg) == arrival_sets(r1)
        for what in ("training_loss", "testing_loss", "auc"):
            np.testing.assert_allclose(getattr(eg, what)[:, k], getattr(e1, what), **TOL)


@pytest.mark.parametrize("prec_name", ["fp32", "fp32x64"])
def test_gpu_sweep_in_the_fp32_storage_precisions(prec_name, native):
    """fp32x64 keeps the fp64 tolerance against its CPU run (the same stored values, fp64 arithmetic); fp32 is held
    to the project's fp32 engine tolerance, 2e-4 of the largest entry (tests/test_engine_gpu.py)."""
    sweep = dict(sweep_alpha=ALPHAS, sweep_lr=LRS, precision=prec_name)
    tg, rg, _ = _gpu_run("agc_uneven", "AGD", **sweep)
    cfg, src, sch, parts = make(CASES["agc_uneven"], "AGD", **sweep)
    rc = Trainer(cfg, DistEnv(), src, scheme=sch).run()
    if prec_name == "fp32x64":
        np.testing.assert_allclose(rg.betaset, rc.betaset, **TOL)
    else:
        err = np.max(np.abs(rg.betaset - rc.betaset)) / np.max(np.abs(rc.betaset))
        assert err < 2e-4, err
    assert np.all(rg.betaset.reshape(-1, 3, tg.ld_x)[:, :, tg.d_x:] == 0.0)


@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_stream_loop_and_native_pump_agree_bitwise(rule, native):
    sweep = dict(sweep_alpha=ALPHAS, sweep_lr=LRS)
    ts, rs, _ = _gpu_run("agc_uneven", rule, "stream", **sweep)
    to, ro, _ = _gpu_run("agc_uneven", rule, "off", **sweep)
    assert ts.device_loop == "stream" and to.device_loop is None
    assert ts.rank_report()["round_loop"] == "stream" and to.rank_report()["round_loop"] == "native pump"
    np.testing.assert_array_equal(rs.betaset, ro.betaset)
    tg, rg, _ = _gpu_run("agc_uneven", rule, "graph", **sweep)
    assert tg.device_loop == "graph"
    np.testing.assert_array_equal(rg.betaset, ro.betaset)


# ---- 6. three ranks sharing the GPU over the IPC mailbox
def test_three_ranks_over_ipc_match_the_replay(tmp_path, native):
    out = str(tmp_path / "multimodel_ipc.npz")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", EH_MULTIMODEL_OUT=out,
               EH_MULTIMODEL_DEVICE="cuda")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr",
           "127.0.0.1", f"--master-port={port}", os.path.join(HERE, "mp_multimodel_run.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out, allow_pickle=True)
    assert str(z["transport"]) == "ipc"
    assert str(z["round_loop"]) == "native pump"  # per-model coefficients: never the device arbiter
    check_against_replay(z)
