"""L1 / elastic net on the GPU (GPU only): the proximal update kernel (csrc/kernels/update.hip combine_update_prox)
against the existing update kernels on the same inputs, the engine against the CPU engine, the round loops, and
three ranks sharing the GPU over the IPC mailbox.

The kernel's new beta, history row and worker copy must be BITWISE the soft threshold of what combine_update (one
model) or combine_update_blocks (M models) writes: the combine and the update expressions are the same code.  u (AGD)
and g_out are compared with NumPy at rtol 1e-13; their atol 1e-12 is the one tests/test_kernels_gpu.py gives
combine_update (a sum of O(1) terms that may cancel has no relative bound).
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from elastic_net_cases import (ALPHAS, CASES, KERNEL_BLOCKS, KERNEL_NMSG, KERNEL_SHAPES, L1, L1S, LRS, MARGIN, TOL,
                               make, replay)
from erasurehead_amd.engine import Trainer, evaluate
from erasurehead_amd.models import losses
from erasurehead_amd.models.losses import soft_threshold
from erasurehead_amd.ops.update import combine_update, combine_update_blocks, combine_update_prox
from erasurehead_amd.parallel.dist import DistEnv
from test_elastic_net_cpu import check_against_replay, same_bits
from test_multimodel_cpu import arrival_sets

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = [(m, w) for m in (torch.float64, torch.float32) for w in (torch.float64, torch.float32)]
THETA = 0.4
CLOSE = dict(rtol=1e-13, atol=1e-12)


def coefs_of(rng, M):
    return list(1.0 - rng.rand(M) * 0.1), list(rng.rand(M) * 0.1), list(rng.rand(M) * 0.1)


def reference(msgs, coefs, beta0, u0, M, ld, d, decay, gm, l2, rule, w_dtype):
    """The existing kernel on the same inputs: (beta, u, hist, beta_w, g_out) as NumPy / torch."""
    beta, u = beta0.clone(), u0.clone()
    hist = torch.zeros(M * ld, dtype=torch.float64, device=DEV)
    bw = torch.full((M * ld,), float("nan"), dtype=w_dtype, device=DEV)
    g = torch.zeros(M * ld, dtype=torch.float64, device=DEV)
    if M == 1:
        combine_update(msgs, coefs, beta, u, d, decay[0], gm[0], l2[0], THETA, rule, hist=hist, beta_w=bw, g_out=g)
    else:
        combine_update_blocks(msgs, coefs, beta, u, ld, d, decay, gm, l2, THETA, rule, hist=hist, beta_w=bw, g_out=g)
    torch.cuda.synchronize()
    return beta.cpu().numpy(), u.cpu().numpy(), hist.cpu().numpy(), bw, g.cpu().numpy()


def prox(msgs, coefs, beta0, u0, M, ld, d, decay, gm, l2, thr, rule, w_dtype, outputs=True):
    beta, u = beta0.clone(), u0.clone()
    hist = torch.zeros(M * ld, dtype=torch.float64, device=DEV) if outputs else None
    bw = torch.full((M * ld,), float("nan"), dtype=w_dtype, device=DEV) if outputs else None
    g = torch.zeros(M * ld, dtype=torch.float64, device=DEV) if outputs else None
    combine_update_prox(msgs, coefs, beta, u, ld, d, decay, gm, l2, list(thr), THETA, rule, hist=hist, beta_w=bw, g_out=g)
    torch.cuda.synchronize()
    return beta, u, hist, bw, g


def check_prox(msgs, coefs, beta0, u0, M, ld, d, decay, gm, l2, thr, rule, w_dtype, ref, what):
    """combine_update_prox on the inputs of ``ref`` (reference()'s result): bitwise S_t of the reference beta."""
    rb, _, _, _, rg = ref
    want = soft_threshold(rb.reshape(M, ld), np.asarray(thr, dtype=np.float64)[:, None]).ravel()
    data = (np.arange(M * ld) % ld) < d
    assert np.all(want[~data] == 0.0)
    beta, u, hist, bw, g = prox(msgs, coefs, beta0, u0, M, ld, d, decay, gm, l2, thr, rule, w_dtype)
    assert same_bits(beta.cpu().numpy(), want), what
    assert same_bits(hist.cpu().numpy()[data], want[data]) and np.all(hist.cpu().numpy()[~data] == 0.0), what
    bwh = bw.cpu().double().numpy()  # exact: every W value is an fp64 value
    assert same_bits(bwh[data], torch.from_numpy(want).to(w_dtype).double().numpy()[data]), what
    assert np.all(bwh[~data] == 0.0), what  # padded beta_w is written, as zero
    b0 = beta0.cpu().numpy()
    finite = np.isfinite(want)
    gh = sum(c * m.double().cpu().numpy() for c, m in zip(coefs, msgs))
    np.testing.assert_allclose(g.cpu().numpy()[data & finite], gh[data & finite], **CLOSE, err_msg=what)
    assert same_bits(g.cpu().numpy(), rg), what  # the same fma chain as the existing kernel
    if rule == 1:
        uref = b0 + (want - b0) * (1.0 / THETA)  # formed from the thresholded beta
        np.testing.assert_allclose(u.cpu().numpy()[data & finite], uref[data & finite], **CLOSE, err_msg=what)
        assert np.all(u.cpu().numpy()[~data] == u0.cpu().numpy()[~data]), what
    else:
        assert torch.equal(u, u0), what
    # without the optional outputs: the same beta and u
    beta2, u2, _, _, _ = prox(msgs, coefs, beta0, u0, M, ld, d, decay, gm, l2, thr, rule, w_dtype, outputs=False)
    assert same_bits(beta2.cpu().numpy(), want) and same_bits(u2.cpu().numpy(), u.cpu().numpy()), what
    return want


# ---- 1. the kernel against the existing kernel
@pytest.mark.parametrize("nmsg", KERNEL_NMSG)
@pytest.mark.parametrize("M", [1] + KERNEL_BLOCKS)
@pytest.mark.parametrize("d,ld", KERNEL_SHAPES, ids=[f"d{d}" for d, _ in KERNEL_SHAPES])
def test_kernel_is_the_threshold_of_the_existing_kernel(d, ld, M, nmsg, native):
    rng = np.random.RandomState(1000 * d + 10 * M + nmsg)
    for m_dtype, w_dtype in DTYPES:
        msgs = [torch.from_numpy(losses.sweep_pack(rng.randn(M, d), ld)).to(m_dtype).to(DEV) for _ in range(nmsg)]
        coefs = list(rng.randn(nmsg))
        decay, gm, l2 = coefs_of(rng, M)
        beta0 = torch.from_numpy(losses.sweep_pack(rng.randn(M, d), ld)).to(DEV)
        u0 = torch.from_numpy(losses.sweep_pack(rng.randn(M, d), ld)).to(DEV)
        for rule in (0, 1):
            ref = reference(msgs, coefs, beta0, u0, M, ld, d, decay, gm, l2, rule, w_dtype)
            x = np.abs(ref[0].reshape(M, ld)[:, :d])
            col = rng.randint(0, d, M)  # one chosen column per block: its |x| as that block's threshold
            sets = {"zero": np.zeros(M), "distinct": 0.1 + 0.8 * rng.rand(M), "all": np.full(M, 2.0 * x.max() + 1.0),
                    "exact": x[np.arange(M), col]}
            for name, thr in sets.items():
                what = f"{name} {m_dtype} {w_dtype} rule {rule}"
                want = check_prox(msgs, coefs, beta0, u0, M, ld, d, decay, gm, l2, thr, rule, w_dtype, ref, what)
                got = want.reshape(M, ld)[:, :d]
                if name == "zero":
                    assert same_bits(got, ref[0].reshape(M, ld)[:, :d]), what  # no x is +-0 here: S_0 is the identity
                if name == "all":
                    assert same_bits(got, np.zeros((M, d))), what
                if name == "exact":
                    assert same_bits(got[np.arange(M), col], np.zeros(M)), what
                    assert np.count_nonzero(got) == np.count_nonzero(x > thr[:, None]), what
                if name == "distinct":
                    assert (0 < np.count_nonzero(got) < M * d) or d == 1, what


@pytest.mark.parametrize("M", [1, 3])
def test_kernel_keeps_nan_and_inf_and_clears_negative_zero(M, native):
    d, ld, nmsg = 37, 40, 9
    tiny = 5e-324
    for m_dtype, w_dtype in DTYPES:
        rng = np.random.RandomState(7)
        host = [losses.sweep_pack(rng.randn(M, d), ld).reshape(M, ld) for _ in range(nmsg)]
        host[2][:, 3], host[8][:, 4], host[0][:, 5] = np.nan, np.inf, -np.inf
        for h in host:
            h[:, 6:12] = 0.0  # zero gradient: x = decay * beta there
        msgs = [torch.from_numpy(h.ravel()).to(m_dtype).to(DEV) for h in host]
        coefs = [1.0] * nmsg
        b0 = losses.sweep_pack(rng.randn(M, d), ld).reshape(M, ld)
        b0[:, 6], b0[:, 7], b0[:, 8], b0[:, 9], b0[:, 10], b0[:, 11] = -0.0, 0.0, tiny, -tiny, 3 * tiny, -1e-310
        beta0 = torch.from_numpy(b0.ravel()).to(DEV)
        u0 = torch.zeros(M * ld, dtype=torch.float64, device=DEV)
        decay, gm, l2 = [1.0] * M, [0.125] * M, [0.0] * M
        for thr in (0.0, tiny, 0.25):
            ref = reference(msgs, coefs, beta0, u0, M, ld, d, decay, gm, l2, 0, w_dtype)
            assert np.signbit(ref[0].reshape(M, ld)[:, 6]).all()  # the existing kernel does give -0.0 here
            want = check_prox(msgs, coefs, beta0, u0, M, ld, d, decay, gm, l2, [thr] * M, 0, w_dtype, ref,
                              f"hostile thr {thr} {m_dtype} {w_dtype}").reshape(M, ld)
            beta = prox(msgs, coefs, beta0, u0, M, ld, d, decay, gm, l2, [thr] * M, 0, w_dtype)[0].cpu().numpy()
            got = beta.reshape(M, ld)
            assert np.isnan(got[:, 3]).all()  # a diverged column stays NaN: never a zero
            assert np.all(got[:, 4] == -np.inf) and np.all(got[:, 5] == np.inf)  # x = -gm * (+-inf)
            assert np.all(got[:, 6] == 0.0) and not np.signbit(got[:, 6]).any()  # -0.0 becomes +0.0, at t = 0 too
            assert np.all(got[:, 7] == 0.0) and not np.signbit(got[:, 7]).any()
            if thr == 0.0:
                assert same_bits(got[:, 8:12], np.tile([tiny, -tiny, 3 * tiny, -1e-310], (M, 1)))
            if thr == tiny:
                assert same_bits(got[:, 8:12], np.tile([0.0, 0.0, 2 * tiny, -1e-310 + tiny], (M, 1)))
            if thr == 0.25:
                assert same_bits(got[:, 8:12], np.zeros((M, 4)))
            assert np.all(got[:, d:] == 0.0) and same_bits(got, want)
        # AGD with a NaN message: beta and u of that column are NaN, the others finite
        beta, u, _, _, _ = prox(msgs, coefs, beta0, u0, M, ld, d, decay, gm, l2, [0.25] * M, 1, w_dtype)
        assert np.isnan(beta.cpu().numpy().reshape(M, ld)[:, 3]).all() and np.isnan(u.cpu().numpy().reshape(M, ld)[:, 3]).all()
        assert np.isfinite(beta.cpu().numpy().reshape(M, ld)[:, 6:]).all()


def test_invalid_threshold_or_shape_raises_before_any_launch(native):
    M, ld, d = 3, 40, 37
    rng = np.random.RandomState(0)
    msgs = [torch.from_numpy(losses.sweep_pack(rng.randn(M, d), ld)).to(DEV) for _ in range(2)]
    beta0 = torch.from_numpy(losses.sweep_pack(rng.randn(M, d), ld)).to(DEV)
    beta, u = beta0.clone(), torch.zeros_like(beta0)
    co = [1.0] * M

    def raw(thr=(0.1, 0.2, 0.3), block_ld=ld, d_x=d, decay=co, gm=co, l2=co, b=beta, uu=u):
        native.combine_update_prox(msgs, [1.0, 1.0], b, uu, None, None, None, block_ld, d_x, list(decay), list(gm),
                                   list(l2), list(thr), THETA, 0)

    for thr in ((0.1, -1e-300, 0.3), (float("nan"), 0.2, 0.3), (0.1, 0.2, -float("inf"))):
        with pytest.raises(RuntimeError, match="invalid"):  # the launcher's own check: hipErrorInvalidValue
            raw(thr=thr)
        with pytest.raises(ValueError, match="threshold"):
            combine_update_prox(msgs, [1.0, 1.0], beta, u, ld, d, co, co, co, list(thr), THETA, 0)
    bad = [dict(d_x=ld + 1), dict(d_x=0), dict(block_ld=0, d_x=0), dict(thr=(0.1, 0.2)), dict(block_ld=ld - 1, d_x=d),
           dict(decay=[1.0] * 9, gm=[1.0] * 9, l2=[1.0] * 9, thr=[0.1] * 9), dict(decay=[], gm=[], l2=[], thr=[])]
    for kw in bad:  # the binding's own shape checks (invalid_argument) stand before the launcher's
        with pytest.raises((RuntimeError, ValueError)):
            raw(**kw)
    with pytest.raises(ValueError):
        combine_update_prox(msgs, [1.0, 1.0], beta, u, ld, ld + 1, co, co, co, [0.1] * M, THETA, 0)
    torch.cuda.synchronize()
    assert torch.equal(beta, beta0) and not bool(u.any())  # nothing ran
    raw()
    torch.cuda.synchronize()
    assert not torch.equal(beta, beta0)


# ---- 2. the engine on the GPU against the CPU engine
def _gpu_run(name, rule, device_loop="auto", **kw):
    cfg, src, sch, parts = make(CASES[name], rule, **kw)
    cfg.device_loop = device_loop
    tr = Trainer(cfg, DistEnv(device=torch.device(DEV)), src, scheme=sch)
    res = tr.run()
    return tr, res, evaluate(tr, res, write=False)


def _cpu_run(name, rule, **kw):
    cfg, src, sch, parts = make(CASES[name], rule, **kw)
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    res = tr.run()
    return tr, res, evaluate(tr, res, write=False), (cfg, sch, parts)


@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_engine_matches_the_cpu_engine(name, rule, native):
    tc, rc, ec, (cfg, sch, parts) = _cpu_run(name, rule, l1=L1)
    # thresholding is discontinuous: the supports can be compared exactly because, on the CPU run, no pre-threshold
    # magnitude lies within MARGIN (relative) of its threshold in any round
    _, margin = replay(sch, parts, tc.beta0, rc.arrivals, rule, cfg.alpha_value, cfg.n_rows, cfg.eta(), L1)
    assert margin > MARGIN, margin
    tg, rg, eg = _gpu_run(name, rule, l1=L1)
    assert tg.native_loop and tg.prox and tg.rank_report()["prox"] is True
    assert arrival_sets(rg) == arrival_sets(rc)
    np.testing.assert_allclose(rg.betaset, rc.betaset, **TOL)
    np.testing.assert_array_equal(rg.betaset == 0, rc.betaset == 0)
    np.testing.assert_array_equal(eg.nnz, ec.nnz)
    assert 0 < eg.nnz[-1] < 33
    for what in ("training_loss", "testing_loss", "auc", "l1_penalty"):
        np.testing.assert_allclose(getattr(eg, what), getattr(ec, what), **TOL)


@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_gpu_sweep_over_l1_matches_the_cpu_sweep(rule, native):
    sweep = dict(sweep_alpha=ALPHAS, sweep_lr=LRS, sweep_l1=L1S)
    tc, rc, ec, (cfg, sch, parts) = _cpu_run("agc_uneven", rule, **sweep)
    etas = cfg.sweep_etas()
    b0 = tc.beta0.reshape(3, tc.ld_x)[:, : tc.d_x]
    for k in range(3):
        _, margin = replay(sch, parts, b0[k], rc.arrivals, rule, ALPHAS[k], cfg.n_rows, etas[k], L1S[k])
        assert margin > MARGIN, (k, margin)
    tg, rg, eg = _gpu_run("agc_uneven", rule, **sweep)
    assert tg.rank_report()["round_loop"] in ("stream", "graph") and tg.rank_report()["l1"] == L1S
    assert arrival_sets(rg) == arrival_sets(rc)
    np.testing.assert_allclose(rg.betaset, rc.betaset, **TOL)
    np.testing.assert_array_equal(rg.betaset == 0, rc.betaset == 0)
    np.testing.assert_array_equal(eg.nnz, ec.nnz)
    assert np.all(rg.betaset.reshape(-1, 3, tg.ld_x)[:, :, tg.d_x:] == 0.0)
    for what in ("training_loss", "testing_loss", "auc", "l1_penalty"):
        np.testing.assert_allclose(getattr(eg, what), getattr(ec, what), **TOL)


@pytest.mark.parametrize("prec_name", ["fp32", "fp32x64"])
def test_gpu_engine_in_the_fp32_storage_precisions(prec_name, native):
    """The rules of tests/test_multimodel_gpu.py: fp32x64 keeps the fp64 tolerance against its CPU run (the same stored
    values, fp64 arithmetic); fp32 is held to the project's fp32 engine tolerance, 2e-4 of the largest entry."""
    tc, rc, ec, _ = _cpu_run("agc_uneven", "AGD", l1=L1, precision=prec_name)
    tg, rg, eg = _gpu_run("agc_uneven", "AGD", l1=L1, precision=prec_name)
    if prec_name == "fp32x64":
        np.testing.assert_allclose(rg.betaset, rc.betaset, **TOL)
        np.testing.assert_array_equal(eg.nnz, ec.nnz)
    else:
        err = np.max(np.abs(rg.betaset - rc.betaset)) / np.max(np.abs(rc.betaset))
        assert err < 2e-4, err
    assert np.all(rg.betaset[:, tg.d_x:] == 0.0) and 0 < eg.nnz[-1] < 33


# ---- 3. the round loops
@pytest.mark.parametrize("rule", ["GD", "AGD"])
def test_stream_graph_and_native_pump_agree_bitwise(rule, native):
    ts, rs, _ = _gpu_run("agc_uneven", rule, "stream", l1=L1)
    to, ro, _ = _gpu_run("agc_uneven", rule, "off", l1=L1)
    tg, rg, _ = _gpu_run("agc_uneven", rule, "graph", l1=L1)
    ta, ra, _ = _gpu_run("agc_uneven", rule, l1=L1)
    assert ts.rank_report()["round_loop"] == "stream" and to.rank_report()["round_loop"] == "native pump"
    assert tg.rank_report()["round_loop"] == "graph" and ta.rank_report()["round_loop"] in ("stream", "graph")
    for r in (rs, rg, ra):
        np.testing.assert_array_equal(r.betaset, ro.betaset)
    assert np.any(ro.betaset == 0.0)


def test_a_zero_lambda_run_reports_todays_loop_and_result(native):
    t0, r0, _ = _gpu_run("agc_uneven", "AGD")
    t1, r1, _ = _gpu_run("agc_uneven", "AGD", l1=0.0)
    rep0, rep1 = t0.rank_report(), t1.rank_report()
    assert rep1["round_loop"] == rep0["round_loop"] == "stream" and rep1["loop_reason"] == rep0["loop_reason"]
    assert rep1["prox"] is False and not t1.prox
    np.testing.assert_array_equal(r0.betaset, r1.betaset)
    _, s0, _ = _gpu_run("agc_uneven", "AGD", sweep_alpha=ALPHAS, sweep_lr=LRS)
    t2, s1, _ = _gpu_run("agc_uneven", "AGD", sweep_alpha=ALPHAS, sweep_lr=LRS, sweep_l1=[0.0, 0.0, 0.0])
    assert t2.rank_report()["prox"] is False
    np.testing.assert_array_equal(s0.betaset, s1.betaset)


# ---- 4. three ranks sharing the GPU over the IPC mailbox
def test_three_ranks_over_ipc_match_the_replay(tmp_path, native):
    out = str(tmp_path / "elastic_ipc.npz")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", EH_ELASTIC_OUT=out,
               EH_ELASTIC_DEVICE="cuda", EH_ELASTIC_CASE="agc_uneven")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr",
           "127.0.0.1", f"--master-port={port}", os.path.join(HERE, "mp_elastic_net_run.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out, allow_pickle=True)
    assert str(z["transport"]) == "ipc" and bool(z["prox"])
    assert str(z["round_loop"]) == "native pump"  # a proximal step: never the device arbiter
    check_against_replay(z, "agc_uneven")
