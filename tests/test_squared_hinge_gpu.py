"""Squared-hinge (L2-SVM) loss on the gfx950 kernels against this file's own fp64 NumPy oracle (GPU only).

Every gradient / evaluation case with d >= 37 checks that its rows straddle the kink of max(0, 1 - y z):
a test whose rows are all active (where the loss equals least squares on +-1 labels) or all inactive
would pass on a kernel that gets the max wrong.  Dense beta: std 10 / sqrt(d) over X = randn * 0.3
(z has std ~3); sparse rows of 5-9 non-zeros: std 1.
"""
import collections

import numpy as np
import pytest
import scipy.sparse as sps
import torch

from erasurehead_amd.models.losses import SQUARED_HINGE, roc_auc
from erasurehead_amd.ops import DenseGradPlan, SparseGradPlan, get_precision, loss_sums
from erasurehead_amd.ops.eval import predictions_and_loss, sparse_eval_device
from erasurehead_amd.ops.grad import KernelChoice

pytestmark = pytest.mark.gpu
DEV = "cuda"
DENSE_TOL = {"fp64": 1e-11, "fp32": 2e-4, "bf16": 2e-4}  # relative to max |ref|
SPARSE_TOL = {"fp64": 1e-11, "fp32": 1e-4}
EVAL_TOL = {"fp64": 1e-11, "fp32": 2e-5, "bf16": 2e-5}


# ---- oracle: z = X beta, m = max(0, 1 - y z), g = -2 X^T(coef y m), loss per row m^2
def _margin(X, y, beta):
    return np.maximum(0.0, 1.0 - y * np.asarray(X.dot(beta)).ravel())


def _grad(X, y, beta, coef=1.0):
    return np.asarray(X.T.dot(-2.0 * coef * y * _margin(X, y, beta))).ravel()


def _straddles(pairs, beta):
    """The share of rows with y z < 1 over every (X, y) lies in [0.3, 0.9]."""
    act = np.concatenate([y * np.asarray(X.dot(beta)).ravel() < 1.0 for X, y in pairs])
    share = float(act.mean())
    assert 0.3 <= share <= 0.9, share


def _parts(rng, sizes, d, prec):
    parts, host = {}, {}
    for p, n in enumerate(sizes):
        X = rng.randn(n, d) * 0.3
        y = rng.choice([-1.0, 1.0], n)
        Xp = torch.zeros((n, prec.ld(d)), dtype=torch.float64)
        Xp[:, :d] = torch.from_numpy(X)
        Xs = Xp.to(prec.storage)
        host[p] = (Xs[:, :d].double().numpy(), y)  # the oracle sees the stored (rounded) values
        parts[p] = (Xs.to(DEV).contiguous(), torch.from_numpy(y).to(prec.acc).to(DEV))
    return parts, host


def _beta(rng, d, prec):
    beta = torch.zeros(prec.ld(d), dtype=prec.acc, device=DEV)
    beta[:d] = torch.from_numpy(rng.randn(d) * 10.0 / np.sqrt(d)).to(prec.acc)
    return beta, beta[:d].double().cpu().numpy()


def _check(G, msgs, host, bh, d, tol):
    if d >= 37:
        _straddles([host[p] for p in sorted(host)], bh)
    for s, m in enumerate(msgs):
        ref = sum(_grad(host[p][0], host[p][1], bh, c) for p, c in m)
        got = G[s, :d].double().cpu().numpy()
        err = np.max(np.abs(got - ref)) / max(1e-12, np.max(np.abs(ref)))
        assert err < tol, (s, err)
    assert torch.all(G[:, d:] == 0)


@pytest.mark.parametrize("prec_name", ["fp64", "fp32", "bf16"])
@pytest.mark.parametrize("d", [1, 37, 1000, 2048, 2500, 9000])
def test_dense_grad(prec_name, d, native):
    """Fused / one-wave (d <= 2048), wide single-pass and two-pass kernels; plan.run and the native launcher."""
    prec = get_precision(prec_name)
    rng = np.random.RandomState(d + SQUARED_HINGE)
    parts, host = _parts(rng, [257, 64, 1], d, prec)
    msgs = [[(0, 1.0), (1, -0.7)], [(2, 2.5)], [(1, 1.0), (0, 0.3), (2, 1.0)]]
    plan = DenseGradPlan(msgs, parts, prec, SQUARED_HINGE, d, target_tasks=7)
    beta, bh = _beta(rng, d, prec)
    G = plan.out_buffer()[0]
    plan.run(beta, G)
    torch.cuda.synchronize()
    _check(G, msgs, host, bh, d, DENSE_TOL[prec_name])
    G2 = plan.out_buffer()[0]
    plan.native_launcher().launch(beta, G2)
    torch.cuda.synchronize()
    assert torch.equal(G, G2)


MULTI3 = [(rows, d, p, form) for rows, d, p in [(64, 1000, "fp64"), (37, 1000, "fp64"), (256, 250, "fp64"),
                                                (64, 1000, "fp32"), (37, 1000, "bf16")]
          for form in ("fold-lane", "fold-wave", "fold-pair", "unfolded")
          if form != "fold-pair" or d == 250]  # pair rows: <= 8 columns per lane


@pytest.mark.parametrize("rows,d,prec_name,form", MULTI3)
def test_one_wave_bundles_of_three(rows, d, prec_name, form, native):
    """grad_dense_multi R = 3 (bundles of 3, of 2 padded to 3, odd-length bundles), every epilogue."""
    prec = get_precision(prec_name)
    rng = np.random.RandomState(5)
    parts, host = _parts(rng, [700, 501, 300], d, prec)
    msgs = [[(0, 1.0), (1, 1.0)]] * 2 + [[(0, -0.5), (1, 2.0)]] + [[(2, 1.0)], [(2, -3.0)]]
    plan = DenseGradPlan(msgs, parts, prec, SQUARED_HINGE, d,
                         choice=KernelChoice("multi", replicas=3, bundle_rows=rows, fold=form != "unfolded",
                                             lane_epi=form == "fold-lane", pair=form == "fold-pair"))
    assert plan.bundle_rows == rows
    beta, bh = _beta(rng, d, prec)
    G = plan.out_buffer()[0]
    plan.native_launcher().launch(beta, G)
    torch.cuda.synchronize()
    _check(G, msgs, host, bh, d, DENSE_TOL[prec_name])


@pytest.mark.parametrize("form", ["fold-lane", "fold-wave", "unfolded"])
@pytest.mark.parametrize("rows,d,prec_name", [(64, 1000, "fp64"), (37, 1000, "fp64"), (256, 250, "fp64"),
                                              (64, 1000, "fp32")])
def test_one_wave_bundles_of_two(rows, d, prec_name, form, native):
    prec = get_precision(prec_name)
    rng = np.random.RandomState(8)
    parts, host = _parts(rng, [700, 501, 300, 64], d, prec)
    msgs = [[(0, 1.0), (1, 1.0)], [(0, 0.5), (1, -2.0)], [(2, 1.0), (3, 1.0)], [(2, -1.0), (3, 3.0)]]
    plan = DenseGradPlan(msgs, parts, prec, SQUARED_HINGE, d,
                         choice=KernelChoice("multi", replicas=2, bundle_rows=rows, fold=form != "unfolded",
                                             lane_epi=form == "fold-lane"))
    assert plan.bundle_rows == rows and plan.max_rep == 2
    beta, bh = _beta(rng, d, prec)
    G = plan.out_buffer()[0]
    plan.native_launcher().launch(beta, G)
    torch.cuda.synchronize()
    _check(G, msgs, host, bh, d, DENSE_TOL[prec_name])


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("rows,d,prec_name", [(64, 1000, "fp64"), (37, 1000, "fp32"), (256, 250, "fp64"),
                                              (37, 1000, "bf16")])
def test_one_wave_bundles_of_one(rows, d, prec_name, fold, native):
    """Distinct rows through grad_dense_multi with one replica per bundle."""
    prec = get_precision(prec_name)
    rng = np.random.RandomState(17)
    parts, host = _parts(rng, [900, 700, 333, 64], d, prec)
    msgs = [[(0, 1.0), (1, 0.5)], [(2, -1.0)], [(3, 2.0)]]
    plan = DenseGradPlan(msgs, parts, prec, SQUARED_HINGE, d,
                         choice=KernelChoice("multi", replicas=1, bundle_rows=rows, fold=fold))
    assert plan.choice.kind == "multi" and plan.max_rep == 1 and plan.bundle_rows == rows
    beta, bh = _beta(rng, d, prec)
    G = plan.out_buffer()[0]
    plan.native_launcher().launch(beta, G)
    torch.cuda.synchronize()
    _check(G, msgs, host, bh, d, DENSE_TOL[prec_name])


@pytest.mark.parametrize("layout", ["mixed", "pairs"])
@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("rows,d,prec_name", [(64, 1000, "fp64"), (37, 1000, "fp64"), (256, 250, "fp64"),
                                              (64, 1000, "fp32"), (64, 1000, "bf16")])
def test_staged_bundles(rows, d, prec_name, pair, layout, native):
    """LDS-staged replica bundles: bundles of 5 and 3 (a wave per replica) or of 2 (two waves per replica)."""
    prec = get_precision(prec_name)
    rng = np.random.RandomState(21)
    parts, host = _parts(rng, [700, 500, 301], d, prec)
    if layout == "mixed":
        msgs = [[(0, 1.0), (1, 1.0)]] * 3 + [[(1, 0.5), (2, -1.0)]] * 2 + [[(2, 1.0)]]
    else:
        msgs = [[(0, 1.0)]] * 2 + [[(1, 1.0), (2, 0.5)], [(1, -1.0), (2, 2.0)]]
    R = max(collections.Counter(p for m in msgs for p, _ in m).values())
    plan = DenseGradPlan(msgs, parts, prec, SQUARED_HINGE, d,
                         choice=KernelChoice("staged", replicas=R, bundle_rows=rows, pair=pair))
    assert plan.bundle_rows == rows
    beta, bh = _beta(rng, d, prec)
    G = plan.out_buffer()[0]
    plan.native_launcher().launch(beta, G)
    torch.cuda.synchronize()
    _check(G, msgs, host, bh, d, DENSE_TOL[prec_name])


@pytest.mark.parametrize("rows,d,prec_name", [(16, 4096, "fp64"), (33, 3000, "fp64"), (16, 4096, "fp32"),
                                              (33, 3000, "bf16"), (33, 5000, "fp32"), (16, 2100, "fp32")])
def test_wide_row_bundles(rows, d, prec_name, native):
    """grad_dense_wide with replica bundles (the full-, half- and quarter-width instances)."""
    prec = get_precision(prec_name)
    rng = np.random.RandomState(9)
    parts, host = _parts(rng, [301, 200, 77], d, prec)
    msgs = [[(0, 1.0), (1, 1.0)]] * 2 + [[(0, -0.5), (1, 2.0)]] + [[(2, 1.0)], [(2, -3.0)]]
    plan = DenseGradPlan(msgs, parts, prec, SQUARED_HINGE, d, choice=KernelChoice("wide", replicas=3, bundle_rows=rows))
    assert plan.cpl == 256 and plan.bundle_rows == rows and plan.choice.bundled
    beta, bh = _beta(rng, d, prec)
    G = plan.out_buffer()[0]
    plan.native_launcher().launch(beta, G)
    torch.cuda.synchronize()
    _check(G, msgs, host, bh, d, DENSE_TOL[prec_name])


MFMA_MSGS = [[(0, 1.0), (1, 1.0)], [(1, 1.0), (0, 1.0)], [(0, 1.0), (1, 1.0)],  # group of 3, rotated
             [(2, 1.0)], [(2, 1.0)],  # group of 2
             [(0, 0.5), (2, -1.25)], [(1, 2.0)]]  # distinct coefficients


@pytest.mark.parametrize("d", [1000, 333, 8])
@pytest.mark.parametrize("pack", [True, False])
def test_mfma_bf16_bundles(d, pack, native):
    """bf16 replica bundles on the matrix cores, packed terms (R <= 4) and one MFMA per term."""
    prec = get_precision("bf16")
    rng = np.random.RandomState(d + 7 * SQUARED_HINGE)
    parts, host = _parts(rng, [1500, 1501, 777], d, prec)
    native.set_mfma_pack(pack)
    try:
        plan = DenseGradPlan(MFMA_MSGS, parts, prec, SQUARED_HINGE, d)
        assert plan.choice.kind == "mfma" and plan.choice.replicas == 4
        beta, bh = _beta(rng, d, prec)
        G = plan.out_buffer()[0]
        plan.run(beta, G)
        torch.cuda.synchronize()
    finally:
        native.set_mfma_pack(True)
    _check(G, MFMA_MSGS, host, bh, d, DENSE_TOL["bf16"])


def test_mfma_vgpr_ring_is_bitwise_the_lds_ring(native):
    prec = get_precision("bf16")
    d, sizes = 1000, [37, 5, 70]
    rng = np.random.RandomState(d + sum(sizes))
    parts, host = _parts(rng, sizes, d, prec)
    msgs = [[(0, 1.0), (1, 1.0)]] * 3 + [[(1, 0.5), (2, -1.0)]] * 2 + [[(2, 1.0)]]
    plan = DenseGradPlan(msgs, parts, prec, SQUARED_HINGE, d)
    assert plan.choice.kind == "mfma"
    beta, bh = _beta(rng, d, prec)
    out = []
    try:
        for on in (0, 3, 4):
            native.set_mfma_stream(on)
            G = plan.out_buffer()[0]
            plan.native_launcher().launch(beta, G)
            torch.cuda.synchronize()
            out.append(G)
    finally:
        native.set_mfma_stream(0)  # the default
    assert all(torch.equal(out[0], o) for o in out[1:])
    _check(out[0], msgs, host, bh, d, DENSE_TOL["bf16"])


def _sparse_check(plan, msgs, parts, d, prec, tol, rng):
    beta = torch.zeros(prec.ld(d), dtype=prec.acc, device=DEV)
    beta[:d] = torch.from_numpy(rng.randn(d) * 1.0).to(prec.acc)
    bh = beta[:d].double().cpu().numpy()
    _straddles([parts[p] for p in sorted(parts)], bh)
    G, G2 = plan.out_buffer()[0], plan.out_buffer()[0]
    plan.run(beta, G)
    plan.native_launcher().launch(beta, G2)
    torch.cuda.synchronize()
    assert torch.equal(G, G2)  # bitwise, run to run
    for s, m in enumerate(msgs):
        ref = sum(_grad(parts[p][0], parts[p][1], bh, c) for p, c in m)
        got = G[s, :d].double().cpu().numpy()
        err = np.max(np.abs(got - ref)) / max(1e-12, np.max(np.abs(ref)))
        assert err < tol, (s, err)
    assert torch.all(G[:, d:] == 0)
    return G


@pytest.mark.parametrize("prec_name", ["fp64", "fp32"])
@pytest.mark.parametrize("pattern_only", [True, False])
@pytest.mark.parametrize("use_ell", [True, False])
def test_sparse_grad(prec_name, pattern_only, use_ell, native):
    """ELL (beta in LDS), valued ELL and CSR row passes against scipy."""
    prec = get_precision(prec_name)
    rng = np.random.RandomState(3)
    d = 700
    parts = {}
    for p in range(3):
        n = 400 + 37 * p
        cols = np.stack([rng.choice(d, 5, replace=False) for _ in range(n)])
        vals = np.ones(cols.size) if pattern_only else rng.randn(cols.size)
        X = sps.csr_matrix((vals, cols.ravel(), np.arange(0, cols.size + 1, 5)), shape=(n, d))
        parts[p] = (X, rng.choice([-1.0, 1.0], n))
    msgs = [[(0, 1.0), (1, 0.5)], [(2, -1.5)], [(0, 1.0)]]
    plan = SparseGradPlan(msgs, parts, prec, SQUARED_HINGE, d, device=DEV, use_ell=use_ell)
    assert plan.pattern_only == pattern_only and plan.ell == use_ell
    _sparse_check(plan, msgs, parts, d, prec, SPARSE_TOL[prec_name], rng)


@pytest.mark.parametrize("prec_name", ["fp64", "fp32"])
def test_sparse_frc_units(prec_name, native):
    """FRC groups stacked into units: the UNITS column pass reads the row passes' squared-hinge residuals."""
    from erasurehead_amd.data.synthetic import onehot_partitions

    prec = get_precision(prec_name)
    parts_l, _, d = onehot_partitions(4 * 1500, 1800, 9, 4, seed=6)
    parts = {p: xy for p, xy in enumerate(parts_l)}
    msgs = [[(0, 1.0), (1, 1.0)], [(0, 1.0), (1, 1.0)], [(2, 1.0), (3, 1.0)], [(2, 1.0), (3, 1.0)], [(2, 1.0), (3, 1.0)]]
    plan = SparseGradPlan(msgs, parts, prec, SQUARED_HINGE, d, device=DEV, use_ell=True)
    assert plan.units == [(0, 1), (2, 3)] and plan.identity
    G = _sparse_check(plan, msgs, parts, d, prec, SPARSE_TOL[prec_name], np.random.RandomState(2))
    assert torch.equal(G[0], G[1]) and torch.equal(G[2], G[4])


@pytest.mark.parametrize("prec_name", ["fp64", "fp32", "bf16"])
@pytest.mark.parametrize("R", [1, 16, 130])
def test_eval_gemm_loss(prec_name, R, native):
    prec = get_precision(prec_name)
    tol = EVAL_TOL[prec_name]
    rng = np.random.RandomState(R)
    n, d = 1000, 333
    y = rng.choice([-1.0, 1.0], n)
    Xp = torch.zeros((n, prec.ld(d)), dtype=torch.float64)
    Xp[:, :d] = torch.from_numpy(rng.randn(n, d) * 0.3)
    Xs = Xp.to(prec.storage)
    Xh = Xs[:, :d].double().numpy()
    B = torch.zeros((R, prec.ld(d)), dtype=torch.float64)
    B[:, :d] = torch.from_numpy(rng.randn(R, d) * 10.0 / np.sqrt(d))
    Bh = B[:, :d].to(prec.acc).double().numpy()
    for j in range(R):
        _straddles([(Xh, y)], Bh[j])
    Pref = Xh @ Bh.T
    ref = np.array([np.sum(_margin(Xh, y, Bh[j]) ** 2) for j in range(R)])
    Xd, Bd, yd = Xs.to(DEV), B.to(DEV), torch.from_numpy(y).to(DEV)
    sums, nn = loss_sums([(Xd, yd)], Bd, d, SQUARED_HINGE)
    assert nn == n
    assert np.max(np.abs(sums - ref) / ref) < tol
    P, tsum = predictions_and_loss(Xd, yd, Bd, d, SQUARED_HINGE)
    assert np.max(np.abs(tsum - ref) / ref) < tol
    np.testing.assert_allclose(P.double().cpu().numpy(), Pref, rtol=tol * 10, atol=tol * 10)


def test_sparse_eval_kernel(native):
    rng = np.random.RandomState(4)
    n, d, R = 3000, 700, 37
    nnz = rng.randint(5, 9, n)
    ptr = np.concatenate([[0], np.cumsum(nnz)])
    cols = np.concatenate([np.sort(rng.choice(d, k, replace=False)) for k in nnz])
    X = sps.csr_matrix((rng.uniform(0.5, 1.5, cols.size), cols, ptr), shape=(n, d))
    y = rng.choice([-1.0, 1.0], n)
    B = rng.randn(R, d) * 1.0
    for j in range(R):
        _straddles([(X, y)], B[j])
    Bt = torch.from_numpy(np.ascontiguousarray(B.T)).to(DEV)
    P, s = sparse_eval_device(X, torch.from_numpy(y), Bt, SQUARED_HINGE, True)
    Pref = np.asarray(X @ B.T)
    np.testing.assert_allclose(P.cpu().numpy(), Pref, rtol=1e-12, atol=1e-12)
    sref = (np.maximum(0.0, 1.0 - y[:, None] * Pref) ** 2).sum(0)
    assert np.max(np.abs(s.cpu().numpy() - sref) / sref) < 1e-11
    _, s2 = sparse_eval_device(X, torch.from_numpy(y), Bt, SQUARED_HINGE, False)  # loss only, no P
    assert np.max(np.abs(s2.cpu().numpy() - sref) / sref) < 1e-11


@pytest.mark.parametrize("case", [(1, 0, 3, 9, 2, 6), (1, 0, 0, 7, 2, 0)])  # AGC with uneven groups; cyclic s = 2
@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("native_loop,device_loop", [(True, "graph"), (True, "stream"), (True, "off")])
def test_gpu_engine_matches_cpu(case, rule, native_loop, device_loop, native):
    """--loss squared_hinge end to end: the native pump and the device-driven loops against the CPU engine.
    Labels follow a planted direction, so the trajectory leaves rows past the margin within the 8 rounds."""
    from erasurehead_amd.codes import make_scheme, scheme_key
    from erasurehead_amd.config import RunConfig
    from erasurehead_amd.data.source import ArraySource
    from erasurehead_amd.engine import Trainer, evaluate
    from erasurehead_amd.parallel.dist import DistEnv

    is_coded, P, ver, n_procs, s, k = case
    W, d, rows = n_procs - 1, 33, 40
    key = scheme_key(is_coded, P, ver)
    uneven = W % (s + 1) != 0
    n_parts = make_scheme(key, W, s, rows * W, k, P, allow_uneven=uneven, rng=np.random.RandomState(0)).n_partition_files
    n = rows * n_parts
    rng = np.random.RandomState(0)
    w = rng.randn(d)
    data = []
    for _ in range(n_parts + 1):
        X = rng.randn(rows, d) * 0.3
        data.append((X, np.where(X @ w >= 0, 1.0, -1.0)))
    src = ArraySource(data[:-1], data[-1])
    out = {}
    for dev in ("cpu", "cuda"):
        cfg = RunConfig(n_procs, n, d, "/tmp/eh_gpu_sqh/", 0, "x", is_coded, s, P, ver, k, 0, rule, num_itrs=8, seed=0,
                        verbose=False, native_loop=native_loop, device_loop=device_loop, loss="squared_hinge", lr=1.0,
                        allow_uneven_groups=uneven)
        sch = make_scheme(key, W, s, n, k, P, allow_uneven=uneven, rng=np.random.RandomState(0))
        tr = Trainer(cfg, DistEnv(device=torch.device(dev)), src, scheme=sch)
        assert tr.loss == SQUARED_HINGE and tr.native_loop == (dev == "cuda")
        res = tr.run()
        if dev == "cuda":
            assert tr.device_loop == (None if device_loop == "off" else device_loop)
        ev = evaluate(tr, res, write=False)
        out[dev] = (res.betaset, ev.training_loss, ev.testing_loss, ev.auc)
    Xa = np.vstack([p[0] for p in data[:-1]])
    ya = np.concatenate([p[1] for p in data[:-1]])
    assert np.mean(ya * (Xa @ out["cpu"][0][-1]) < 1.0) < 0.95  # rows on both sides of the kink
    np.testing.assert_allclose(out["cuda"][0], out["cpu"][0], rtol=1e-9, atol=1e-11)
    for a, b in zip(out["cuda"][1:], out["cpu"][1:]):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-11)
    Xte, yte = data[-1]
    assert out["cuda"][3][-1] == pytest.approx(roc_auc(yte, Xte @ out["cuda"][0][-1]), rel=1e-12)


def test_unknown_loss_code_raises_and_computes_nothing(native):
    prec = get_precision("fp64")
    d = 37
    rng = np.random.RandomState(1)
    parts, _ = _parts(rng, [64, 33], d, prec)
    plan = DenseGradPlan([[(0, 1.0), (1, 1.0)]], parts, prec, SQUARED_HINGE, d)
    beta, _ = _beta(rng, d, prec)
    G = torch.full((plan.nslots, plan.ld), 123.0, dtype=prec.acc, device=DEV)
    with pytest.raises(RuntimeError):
        native.GradLauncher.dense(prec.code, 7, plan.cpl, plan.segs, plan.tasks, plan.slab, plan.slot_task_begin,
                                  plan.part, plan.ld, choice=plan._native_choice).launch(beta, G)
    torch.cuda.synchronize()
    assert torch.all(G == 123.0)
    plan.run(beta, G)  # the same operands with a known code
    torch.cuda.synchronize()
    assert not torch.any(G[:, :d] == 123.0)
