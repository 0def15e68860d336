"""Multi-class softmax gradient kernel (csrc/kernels/grad_softmax.hip) and the softmax engine on the GPU,
against this file's own fp64 NumPy oracle (GPU only).

Inputs as in test_squared_hinge_gpu.py: partitions of [257, 64, 1] rows, X = randn * 0.3 rounded to the
storage dtype before the oracle sees it, labels randint(0, C), B = randn(C, d) * 6 / sqrt(d).  For d >= 37
every case checks that the softmax is neither saturated nor flat (>= 30 % of the rows with top probability
< 0.9 and >= 25 % with top probability > 0.5): a kernel with a wrong normaliser could pass otherwise.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from erasurehead_amd.engine import Trainer, evaluate
from erasurehead_amd.models.losses import LOGISTIC
from erasurehead_amd.ops import DenseGradPlan, SoftmaxGradPlan, get_precision
from erasurehead_amd.parallel.dist import DistEnv
from test_softmax_cpu import CASES, make, replay

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = {"fp64": 1e-11, "fp32": 2e-4}  # relative to max |ref| (the dense kernels' DENSE_TOL)
CODED = [[(0, 1.0), (1, -0.7)], [(2, 2.5)], [(1, 1.0), (0, 0.3), (2, 1.0)]]  # the encode path
NAIVE = [[(0, 1.0)], [(1, 1.0)], [(2, 1.0)]]  # the direct path


# ---- oracle: z_c = x.B_c, p = softmax(z) (max subtracted), G_c = sum_rows coef (p_c - [y = c]) x
def _probs(X, B):
    Z = X @ B.T
    E = np.exp(Z - Z.max(axis=1, keepdims=True))
    return E / E.sum(axis=1, keepdims=True)


def _grad(X, y, B, coef=1.0):
    R = _probs(X, B)
    R[np.arange(len(y)), y.astype(int)] -= 1.0
    return (coef * R).T @ X


def _not_degenerate(host, B):
    top = np.concatenate([_probs(X, B).max(axis=1) for X, _ in host.values()])
    lo, hi = float(np.mean(top < 0.9)), float(np.mean(top > 0.5))
    assert lo >= 0.30 and hi >= 0.25, (lo, hi)


def _parts(rng, sizes, d, C, prec):
    parts, host = {}, {}
    for p, n in enumerate(sizes):
        X = rng.randn(n, d) * 0.3
        y = rng.randint(0, C, n).astype(np.float64)
        Xp = torch.zeros((n, prec.ld(d)), dtype=torch.float64)
        Xp[:, :d] = torch.from_numpy(X)
        Xs = Xp.to(prec.storage)
        host[p] = (Xs[:, :d].double().numpy(), y)  # the oracle sees the stored (rounded) values
        parts[p] = (Xs.to(DEV).contiguous(), torch.from_numpy(y).to(prec.acc).to(DEV))
    return parts, host


def _model(rng, C, d, prec, scale=6.0):
    """(beta [C * ld] on the device, class-major with zero padding; B [C, d] as stored)."""
    ld = prec.ld(d)
    beta = torch.zeros((C, ld), dtype=prec.acc)
    beta[:, :d] = torch.from_numpy(rng.randn(C, d) * scale / np.sqrt(d)).to(prec.acc)
    return beta.reshape(-1).to(DEV), beta[:, :d].double().numpy()


def _check(G, msgs, host, B, d, ld, tol):
    C = B.shape[0]
    for s, m in enumerate(msgs):
        ref = sum(_grad(host[p][0], host[p][1], B, c) for p, c in m)
        got = G[s].double().cpu().numpy().reshape(C, ld)
        err = np.max(np.abs(got[:, :d] - ref)) / max(1e-12, np.max(np.abs(ref)))
        assert err < tol, (s, err)
        assert np.all(got[:, d:] == 0.0)  # exact zeros in the padding columns of every class block


# ---- 1. the kernel against the oracle
@pytest.mark.parametrize("prec_name", ["fp64", "fp32"])
@pytest.mark.parametrize("d", [1, 37, 1000, 1024])
@pytest.mark.parametrize("C", [2, 3, 7, 8])
def test_kernel_is_the_oracle(C, d, prec_name, native):
    prec = get_precision(prec_name)
    ld = prec.ld(d)
    rng = np.random.RandomState(100 * C + d)
    parts, host = _parts(rng, [257, 64, 1], d, C, prec)
    beta, B = _model(rng, C, d, prec)
    if d >= 37:
        _not_degenerate(host, B)
    for msgs in (CODED, NAIVE):
        plan = SoftmaxGradPlan(msgs, parts, prec, C, d)
        assert plan.identity == (msgs is NAIVE) and plan.ld == C * ld
        G = plan.out_buffer()[0].fill_(7.0)  # every element, padding included, must be overwritten
        plan.run(beta, G)
        torch.cuda.synchronize()
        _check(G, msgs, host, B, d, ld, TOL[prec_name])
        G2 = plan.out_buffer()[0].fill_(-3.0)
        plan.native_launcher().launch(beta, G2)
        G3 = plan.out_buffer()[0]
        plan.run(beta, G3)
        torch.cuda.synchronize()
        assert torch.equal(G, G2)  # the native launcher: bitwise plan.run
        assert torch.equal(G, G3)  # a second run: bitwise the first


def test_many_workgroups_per_partition(native):
    """Partitions long enough to be split into several tasks (slab rows summed in a fixed order)."""
    prec = get_precision("fp64")
    C, d = 5, 129
    rng = np.random.RandomState(9)
    parts, host = _parts(rng, [700, 333], d, C, prec)
    beta, B = _model(rng, C, d, prec)
    msgs = [[(0, 1.0), (1, 1.0)], [(1, -2.0)]]
    plan = SoftmaxGradPlan(msgs, parts, prec, C, d)
    assert plan.ntasks > 4
    G = plan.run(beta, plan.out_buffer()[0])
    torch.cuda.synchronize()
    _check(G, msgs, host, B, d, prec.ld(d), TOL["fp64"])


# ---- 2. C = 2 against the existing logistic kernel, on the device
def test_two_classes_match_the_logistic_kernel(native):
    prec = get_precision("fp64")
    d = 1000
    ld = prec.ld(d)
    rng = np.random.RandomState(2)
    parts, host = _parts(rng, [257, 64, 1], d, 2, prec)
    beta, B = _model(rng, 2, d, prec)
    beta[:ld] = 0.0  # B_0 = 0, B_1 = beta
    G = SoftmaxGradPlan(NAIVE, parts, prec, 2, d).run(beta, torch.zeros((3, 2 * ld), dtype=torch.float64, device=DEV))
    pm = {p: (X, 2.0 * y - 1.0) for p, (X, y) in parts.items()}
    L = DenseGradPlan(NAIVE, pm, prec, LOGISTIC, d).run(beta[ld:].contiguous(),
                                                       torch.zeros((3, ld), dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    scale = float(L.abs().max())
    assert float((G[:, ld:] - L).abs().max()) / scale < 1e-11
    assert float((G[:, :ld] + L).abs().max()) / scale < 1e-11


# ---- 3. extreme logits
@pytest.mark.parametrize("prec_name", ["fp64", "fp32"])
def test_extreme_logits(prec_name, native):
    prec = get_precision(prec_name)
    C, d = 7, 1000
    rng = np.random.RandomState(3)
    parts, host = _parts(rng, [257, 64, 1], d, C, prec)
    beta, B = _model(rng, C, d, prec, scale=1000.0)  # z has std ~300: past fp32 exp's overflow at 88
    zs = np.concatenate([(X @ B.T).ravel() for X, _ in host.values()])
    assert 200.0 < zs.std() < 400.0
    plan = SoftmaxGradPlan(CODED, parts, prec, C, d)
    G = plan.run(beta, plan.out_buffer()[0])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(G).all())
    if prec_name == "fp64":
        _check(G, CODED, host, B, d, prec.ld(d), TOL["fp64"])


# ---- 4. closed gate
@pytest.mark.parametrize("msgs", [CODED, NAIVE])
def test_closed_gate_leaves_the_messages_untouched(msgs, native):
    prec = get_precision("fp64")
    C, d = 3, 37
    rng = np.random.RandomState(4)
    parts, host = _parts(rng, [257, 64, 1], d, C, prec)
    beta, B = _model(rng, C, d, prec)
    plan = SoftmaxGradPlan(msgs, parts, prec, C, d)
    L = plan.native_launcher()
    G = plan.out_buffer()[0].fill_(12345.0)
    L.launch(beta, G, gate=torch.ones(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert bool((G == 12345.0).all())
    L.launch(beta, G, gate=torch.zeros(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    _check(G, msgs, host, B, d, prec.ld(d), TOL["fp64"])


# ---- 5. limits: each a ValueError from the constructor, before any launch
def test_limits_are_value_errors(native):
    prec = get_precision("fp64")
    rng = np.random.RandomState(5)
    parts, _ = _parts(rng, [20], 6, 3, prec)
    msgs = [[(0, 1.0)]]
    wide, _ = _parts(rng, [4], 1025, 3, prec)
    with pytest.raises(ValueError, match="1024"):
        SoftmaxGradPlan(msgs, wide, prec, 3, 1025)
    bf, _ = _parts(rng, [20], 6, 3, get_precision("bf16"))
    with pytest.raises(ValueError, match="bf16"):
        SoftmaxGradPlan(msgs, bf, get_precision("bf16"), 3, 6)
    with pytest.raises(ValueError, match="2..8"):
        SoftmaxGradPlan(msgs, parts, prec, 9, 6)
    for bad in (3.0, 1.5):  # a label equal to C; a label that is no integer
        X, y = parts[0]
        yb = y.clone()
        yb[7] = bad
        with pytest.raises(ValueError, match="partition 0"):
            SoftmaxGradPlan(msgs, {0: (X, yb)}, prec, 3, 6)


# ---- 6. the engine on the GPU against the CPU engine
def _both(case, rule, device_loop, **kw):
    out = {}
    for dev in ("cpu", "cuda"):
        cfg, src, sch, parts = make(case, rule, **kw)
        cfg.device_loop = device_loop
        tr = Trainer(cfg, DistEnv(device=torch.device(dev)), src, scheme=sch)
        if dev == "cuda":
            assert tr.native_loop
        res = tr.run()
        if dev == "cuda":
            assert tr.device_loop == (None if device_loop == "off" else device_loop)
        out[dev] = (res, evaluate(tr, res, write=False))
    (rc, ec), (rg, eg) = out["cpu"], out["cuda"]
    np.testing.assert_allclose(rg.betaset, rc.betaset, rtol=1e-9, atol=1e-11)
    for name in ("training_loss", "testing_loss", "auc"):  # auc: the accuracy of a softmax run
        np.testing.assert_allclose(getattr(eg, name), getattr(ec, name), rtol=1e-9, atol=1e-11)
    assert [[(w, p) for (w, p, _t) in r] for r in rg.arrivals] == [[(w, p) for (w, p, _t) in r] for r in rc.arrivals]


@pytest.mark.parametrize("device_loop", ["graph", "stream", "off"])
@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_engine_matches_cpu_engine(name, rule, device_loop, native):
    _both(CASES[name], rule, device_loop)


def test_gpu_engine_eight_classes_headline_width(native):
    _both(CASES["naive"], "GD", "graph", C=8, d=1000, rounds=3)  # D = 8 * 1000 = 8000


# ---- 7. three ranks sharing the GPU over the IPC mailbox
def test_three_ranks_over_ipc_match_the_replay(tmp_path, native):
    out = str(tmp_path / "softmax_ipc.npz")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", EH_SOFTMAX_OUT=out,
               EH_SOFTMAX_DEVICE="cuda")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr",
           "127.0.0.1", f"--master-port={port}", os.path.join(HERE, "mp_softmax_run.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out, allow_pickle=True)
    assert str(z["transport"]) == "ipc"
    cfg, src, sch, parts = make(CASES["agc_uneven"], "AGD")
    C, d_x, ld_x = 3, 33, 34
    arrivals = [[tuple(a) for a in rnd] for rnd in z["arrivals"]]
    B0 = np.asarray(z["beta0"]).reshape(C, ld_x)[:, :d_x]
    ref = replay(sch, parts, B0, arrivals, "AGD", cfg.alpha_value, cfg.n_rows, cfg.eta())
    got = np.asarray(z["betaset"]).reshape(-1, C, ld_x)
    assert np.all(got[:, :, d_x:] == 0.0)
    np.testing.assert_allclose(got[:, :, :d_x], ref, rtol=1e-9, atol=1e-11)
