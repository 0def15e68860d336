"""The sparse gradient and evaluation kernels on hostile inputs at every edge of their control flow (GPU only).

Every gradient case of tests/sparse_edge_cases.py builds its plan, checks that the plan took the row pass and the
column-pass form the case names, runs it three ways and holds every column of every message to its own
forward-error bound against the long-double oracle of tests/numerics.py (K_SPARSE); columns without an entry,
the padding and dead messages must be exactly zero.  The evaluation kernel is held entry by entry to
oracle_eval's bounds at its wave, column-set and chunk boundaries."""
import functools

import numpy as np
import pytest
import torch

import numerics as nx
import sparse_edge_cases as sc
from erasurehead_amd.ops import SparseGradPlan, loss_sums
from erasurehead_amd.ops.eval import predictions_and_loss, sparse_eval_device

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = sc.GRADIENT
BY_ID = {c.id: c for c in CASES}
WORST = {"ratio": 0.0, "where": ""}  # the largest err / bound any gradient case reached (printed per case with -s)


@functools.lru_cache(maxsize=None)
def _oracle(cid, s):
    case = BY_ID[cid]
    prec, parts, beta, bh = sc.build(case)
    return nx.oracle_sparse_message(case.loss, case.msgs[s], parts, bh, prec)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gradient_case(case, native):
    prec, parts, beta_h, bh = sc.build(case)
    d, ld, e = case.d, prec.ld(case.d), case.expect
    msgs = [list(m) for m in case.msgs]
    plan = SparseGradPlan(msgs, parts, prec, case.loss, d, device=DEV, use_ell=case.use_ell)
    # the path the case names
    assert plan.ell == (e["path"] == "ell") and plan.idx16 == e["idx16"]
    assert (plan.csr_fixed > 0) == (e["path"] == "csr_fixed") and (plan.row_ptr is not None) == (e["path"] != "ell")
    if e["path"] != "csr":
        m = int(np.diff(parts[0][0].indptr)[0])
        assert (plan.ell_m if plan.ell else plan.csr_fixed) == m
    assert plan.pattern_only == (not case.valued)
    assert (plan.units is not None) == e["units"] and plan.identity == e["identity"]
    assert (plan.sub_begin is not None) == e["blocked"] and plan.nsub == e["nsub"]
    assert plan.wg_spans and plan.row16 and plan.wg_tiles == sc.MAX_WG_TILES
    if e["units"]:
        assert plan.units == sc.claimed_units(case) and plan.row_block == sc.UNIT_ROWS
    beta = beta_h.to(DEV)
    out = []
    for how in ("run", "launcher", "run"):
        G = plan.out_buffer()[0]
        if how == "run":
            plan.run(beta, G)
        else:
            plan.native_launcher().launch(beta, G)
        torch.cuda.synchronize()
        out.append(G)
    G = out[0]
    Gh = G.double().cpu().numpy()
    worst = 0.0
    for s, m in enumerate(msgs):
        ref, bound = _oracle(case.id, s)
        q = nx.column_ratio(Gh[s, :d], ref, bound)
        if q > WORST["ratio"]:
            WORST.update(ratio=q, where=f"{case.id} message {s}")
        worst = max(worst, q)
        nx.check_columns(Gh[s, :d], ref, bound, f"{case.id} message {s}", k=nx.K_SPARSE)
        assert np.all(Gh[s, :d][bound == 0] == 0), "a column without an entry in the message must be exactly zero"
    print(f"{case.id}: largest err / bound {worst:.4f} (K_SPARSE = {nx.K_SPARSE}); so far {WORST['ratio']:.4f} at {WORST['where']}")
    assert torch.all(G[:, d:] == 0), "padding columns must be exactly zero"
    dead = sc.dead_messages(case)
    assert dead or case.id.startswith("unit")  # (unit messages all carry coefficient 1 and live partitions)
    assert torch.all(G[dead] == 0), "a message of coefficient 0.0 or of empty partitions must be exactly zero"
    assert torch.equal(out[0], out[1]), "plan.run and the native launcher differ"
    assert torch.equal(out[0], out[2]), "two launches differ"
    if e["units"]:
        sets = sc.message_sets(case.msgs)
        for u in set(sets):
            rows = [i for i, s_ in enumerate(sets) if s_ == u]
            assert len(rows) > 1 and all(torch.equal(G[rows[0]], G[r]) for r in rows[1:]), "unit members differ"


# ---- evaluation -------------------------------------------------------------------------------------
def _check_P(P, Pref, dP, what):
    got = P.double().cpu().numpy()
    assert got.shape == Pref.shape
    assert np.all(np.isfinite(got)), f"{what}: an entry of P was not written"
    err = np.abs(got.astype(nx.LD) - Pref)
    assert np.all(err <= dP), f"{what}: P beyond its bound at {np.argwhere(~(err <= dP))[:4].tolist()}"


def _check_sums(s, sref, bound, what):
    s = np.asarray(s, np.float64)
    assert np.all(np.isfinite(s))
    err = np.abs(s.astype(nx.LD) - sref)
    bad = np.nonzero(~(err <= bound))[0]
    assert bad.size == 0, (f"{what}: loss sums beyond their bound at columns {bad[:4].tolist()}: err "
                           f"{err[bad[:4]].astype(float).tolist()} bound {bound[bad[:4]].astype(float).tolist()}")


@functools.lru_cache(maxsize=None)
def _eval_oracle(cid, loss):
    case = next(c for c in sc.EVAL if c.id == cid)
    prec, X, y, Bt, Bh = sc.build_eval(case)
    return nx.oracle_eval(loss, X.toarray(), y, Bh, prec, k=nx.K_SPARSE)


@pytest.mark.parametrize("case", sc.EVAL, ids=[c.id for c in sc.EVAL])
def test_eval_case(case, native):
    """sparse_eval_device with and without P for the three losses: every entry of P and every loss sum inside
    oracle_eval's bound (the sums are added with atomics: compared to the bound, not bitwise)."""
    prec, X, y, Bt, Bh = sc.build_eval(case)
    yt, Btd = torch.from_numpy(y), Bt.to(DEV)
    for loss in nx.LOSSES:
        what = f"{case.id} {nx.LOSS_IDS[loss]}"
        Pref, dP, sref, ds = _eval_oracle(case.id, loss)
        P, s = sparse_eval_device(X, yt, Btd, loss, True)
        assert P.dtype == prec.acc and s.dtype == torch.float64
        _check_P(P, Pref, dP, what)
        _check_sums(s.cpu().numpy(), sref, ds, what)
        P2, s2 = sparse_eval_device(X, yt, Btd, loss, False)
        assert P2 is None
        _check_sums(s2.cpu().numpy(), sref, ds, what + " (no P)")


def test_eval_of_no_rows_is_zero(native):
    import scipy.sparse as sps
    for dt in (torch.float64, torch.float32):
        Bt = torch.randn(sc.EVAL_D, 65, dtype=dt, device=DEV)
        P, s = sparse_eval_device(sps.csr_matrix((0, sc.EVAL_D)), torch.zeros(0), Bt, nx.LOGISTIC, True)
        assert P.shape == (0, 65) and s.shape == (65,) and torch.all(s == 0)
        _, s = sparse_eval_device(sps.csr_matrix((0, sc.EVAL_D)), torch.zeros(0), Bt, nx.SQUARED_HINGE, False)
        assert torch.all(s == 0)


@pytest.mark.parametrize("pn", sc.PRECS)
def test_eval_257_columns_are_its_two_chunks(pn, native):
    """R = 257 runs as a 256-column pass and a 1-column pass: the same as the two run on their own, within the
    bound (P) and the bound on the sums."""
    case = next(c for c in sc.EVAL if c.R == 257 and c.prec == pn and c.valued)
    prec, X, y, Bt, Bh = sc.build_eval(case)
    yt, Btd = torch.from_numpy(y), Bt.to(DEV)
    for loss in nx.LOSSES:
        Pref, dP, sref, ds = _eval_oracle(case.id, loss)
        P, s = sparse_eval_device(X, yt, Btd, loss, True)
        Pa, sa = sparse_eval_device(X, yt, Btd[:, :256].contiguous(), loss, True)
        Pb, sb = sparse_eval_device(X, yt, Btd[:, 256:].contiguous(), loss, True)
        Pc, scat = torch.cat([Pa, Pb], dim=1), torch.cat([sa, sb])
        _check_P(Pc, Pref, dP, f"{case.id} chunks")
        assert np.all(np.abs((P - Pc).double().cpu().numpy()) <= dP.astype(np.float64))
        _check_sums(scat.cpu().numpy(), sref, ds, f"{case.id} chunks")
        assert np.all(np.abs((s - scat).cpu().numpy()) <= ds.astype(np.float64))


@pytest.mark.parametrize("valued", [True, False], ids=["val", "pat"])
def test_eval_through_predictions_and_loss_and_loss_sums(valued, native):
    """The public callers (fp64 betas): predictions_and_loss on one matrix, loss_sums over two chunks of it."""
    case = next(c for c in sc.EVAL if c.R == 129 and c.prec == "fp64" and c.valued == valued)
    prec, X, y, Bt, Bh = sc.build_eval(case)
    B = Bt.t().contiguous().to(DEV)
    yt = torch.from_numpy(y)
    for loss in nx.LOSSES:
        Pref, dP, sref, ds = _eval_oracle(case.id, loss)
        P, s = predictions_and_loss(X, yt, B, sc.EVAL_D, loss)
        _check_P(P, Pref, dP, f"{case.id} predictions_and_loss")
        _check_sums(s, sref, ds, f"{case.id} predictions_and_loss")
        k = case.n // 2
        sums, rows = loss_sums([(X[:k], yt[:k]), (X[k:], yt[k:])], B, sc.EVAL_D, loss)
        assert rows == case.n
        _check_sums(sums, sref, ds, f"{case.id} loss_sums")
