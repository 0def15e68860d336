"""The evaluation GEMM (both kernels) and combine_update at their tile edges, on hostile inputs (GPU only).

eval_gemm_loss_v2 tiles 128 rows x 112 columns with a 32-deep K tile, the unaligned eval_gemm_loss 64 x 128;
combine_update loads messages in batches of 8, up to MAX_MSGS.  Shapes sit on, one below and one above each
of those; X is tests/numerics.py's hostile partition, the betas are scaled like hostile_beta so margins
reach the hundreds, and every entry is held to the bounds of tests/numerics.py."""
import functools

import numpy as np
import pytest
import torch

import numerics as nx
from erasurehead_amd.models.losses import UpdateRule
from erasurehead_amd.ops import combine_update, get_precision, loss_sums, predictions
from erasurehead_amd.ops.eval import predictions_and_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECS = ("fp64", "fp32", "bf16")

# pairwise-covering subsets: every pair of values of two different factors meets in some shape
V2_N, V2_D, V2_R = (1, 127, 128, 129), (1, 31, 32, 33, 65), (1, 111, 112, 113)
V2_SHAPES = [(n, d, V2_R[(i + j) % 4]) for i, d in enumerate(V2_D) for j, n in enumerate(V2_N)]
V1_N, V1_R, V1_D = (63, 64, 65), (127, 128, 129), (33, 65, 257)
V1_SHAPES = [(n, V1_D[(i + j) % 3], R) for i, n in enumerate(V1_N) for j, R in enumerate(V1_R)]


def test_shape_subsets_cover_every_pair():
    for shapes, factors in ((V2_SHAPES, (V2_N, V2_D, V2_R)), (V1_SHAPES, (V1_N, V1_D, V1_R))):
        for a in range(3):
            for b in range(a + 1, 3):
                assert {(s[a], s[b]) for s in shapes} == {(x, y) for x in factors[a] for y in factors[b]}


@functools.lru_cache(maxsize=None)
def _case(prec_name, n, d, R, padded):
    """Hostile X [n, ld] (or unpadded [n, d]: odd row strides), labels, R hostile betas; generated once."""
    prec = get_precision(prec_name)
    rng = np.random.RandomState(100000 + 1009 * n + 31 * d + R + prec.code)
    X, y, Xh = nx.hostile_partition(rng, n, d, prec)
    B = torch.stack([nx.hostile_beta(rng, d, prec)[0] for _ in range(R)])  # [R, ld] accumulator dtype
    if not padded:
        X, B = X[:, :d].contiguous(), B[:, :d].contiguous()
    return prec, X, y, Xh, B, B[:, :d].double().numpy()


@functools.lru_cache(maxsize=None)
def _oracle(prec_name, n, d, R, padded, loss):
    prec, X, y, Xh, B, Bh = _case(prec_name, n, d, R, padded)
    return nx.oracle_eval(loss, Xh, y.double().numpy(), Bh, prec)


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


@pytest.mark.parametrize("prec_name", PRECS)
@pytest.mark.parametrize("n,d,R", V2_SHAPES)
def test_aligned_eval_gemm_at_tile_edges(n, d, R, prec_name, native):
    """eval_gemm_loss_v2 (16-byte aligned rows) through loss_sums, predictions_and_loss and predictions."""
    prec, X, y, Xh, B, Bh = _case(prec_name, n, d, R, True)
    Xd, yd, Bd = X.to(DEV), y.to(DEV), B.to(DEV)
    for loss in nx.LOSSES:
        what = f"{prec_name} n={n} d={d} R={R} {nx.LOSS_IDS[loss]}"
        Pref, dP, sref, ds = _oracle(prec_name, n, d, R, True, loss)
        sums, rows = loss_sums([(Xd, yd)], Bd, d, loss)
        assert rows == n
        _check_sums(sums, sref, ds, what + " loss_sums")
        P, s2 = predictions_and_loss(Xd, yd, Bd, d, loss)
        _check_P(P, Pref, dP, what + " predictions_and_loss")
        _check_sums(s2, sref, ds, what + " predictions_and_loss")
        # the kernel itself into a NaN-filled P: every entry must be written
        Pn = torch.full((n, R), float("nan"), dtype=prec.acc, device=DEV)
        s3 = torch.zeros(R, dtype=torch.float64, device=DEV)
        native.eval_gemm_loss(loss, Xd, n, d, yd, Bd, s3, Pn)
        _check_P(Pn, Pref, dP, what + " kernel")
        _check_sums(s3.cpu().numpy(), sref, ds, what + " kernel")
    Pref, dP, _, _ = _oracle(prec_name, n, d, R, True, nx.LOGISTIC)
    _check_P(predictions(Xd, Bd, d), Pref, dP, f"{prec_name} n={n} d={d} R={R} predictions")


@pytest.mark.parametrize("prec_name", PRECS)
@pytest.mark.parametrize("n,d,R", V1_SHAPES)
def test_unaligned_eval_gemm_at_tile_edges(n, d, R, prec_name, native):
    """Rows of an odd stride take the scalar-staging kernel (64 x 128 tiles)."""
    prec, X, y, Xh, B, Bh = _case(prec_name, n, d, R, False)
    assert X.shape[1] % 2 == 1 and B.shape[1] % 2 == 1
    Xd, yd, Bd = X.to(DEV), y.to(DEV), B.to(DEV)
    for loss in nx.LOSSES:
        what = f"{prec_name} n={n} d={d} R={R} {nx.LOSS_IDS[loss]} unaligned"
        Pref, dP, sref, ds = _oracle(prec_name, n, d, R, False, loss)
        Pn = torch.full((n, R), float("nan"), dtype=prec.acc, device=DEV)
        s = torch.zeros(R, dtype=torch.float64, device=DEV)
        native.eval_gemm_loss(loss, Xd, n, d, yd, Bd, s, Pn)
        _check_P(Pn, Pref, dP, what)
        _check_sums(s.cpu().numpy(), sref, ds, what)
        s2 = torch.zeros(R, dtype=torch.float64, device=DEV)
        native.eval_gemm_loss(loss, Xd, n, d, yd, Bd, s2, None)  # loss only
        _check_sums(s2.cpu().numpy(), sref, ds, what + " (no P)")


@pytest.mark.parametrize("prec_name", PRECS)
@pytest.mark.parametrize("loss", nx.LOSSES, ids=[nx.LOSS_IDS[k] for k in nx.LOSSES])
def test_two_chunk_loss_sums_add_the_chunk_oracles(loss, prec_name, native):
    """loss_sums over a 128-row chunk and a single-row chunk: the sum of the per-chunk oracles, within the
    sum of their bounds."""
    n, d, R = 129, 65, 113
    prec, X, y, Xh, B, Bh = _case(prec_name, n, d, R, True)
    yh = y.double().numpy()
    chunks = [(X[:128].contiguous().to(DEV), y[:128].to(DEV)), (X[128:].contiguous().to(DEV), y[128:].to(DEV))]
    sums, rows = loss_sums(chunks, B.to(DEV), d, loss)
    assert rows == n
    parts = [nx.oracle_eval(loss, Xh[a:b], yh[a:b], Bh, prec) for a, b in ((0, 128), (128, 129))]
    _check_sums(sums, parts[0][2] + parts[1][2], parts[0][3] + parts[1][3], f"{prec_name} two chunks")


# ---- combine_update -------------------------------------------------------------------------------
MAX_MSGS = 128  # csrc kMaxMsgs (asserted against the extension below)


@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("msg_dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("nmsg", [1, 7, 8, 9, 16, 17, MAX_MSGS])
def test_combine_update_message_counts(nmsg, msg_dtype, rule, native):
    """1, 7, 8, 9, 16, 17 and MAX_MSGS messages (load batches of 8): g against the long-double combine
    within 2 * 2^-52 sum_m |coef_m msg_m| per column; beta, u and the history row against UpdateRule.apply
    on that g, to the rounding of the update's own few operations; the worker copy and the padding."""
    assert native.MAX_MSGS == MAX_MSGS
    rng = np.random.RandomState(1000 * nmsg + (msg_dtype == torch.float32))
    d, ld = 1001, 1002
    scale = 10.0 ** rng.uniform(-3, 1, ld)
    msgs_t = [torch.from_numpy(rng.randn(ld) * scale).to(msg_dtype) for _ in range(nmsg)]
    coefs = list(rng.randn(nmsg))
    if nmsg > 1:
        coefs[nmsg // 2] = 0.0
        coefs[-1] = -abs(coefs[-1])
    b0, u0 = rng.randn(ld) * scale, rng.randn(ld) * scale
    b0[d:] = 0
    u0[d:] = 0
    beta, u = torch.from_numpy(b0.copy()).to(DEV), torch.from_numpy(u0.copy()).to(DEV)
    hist = torch.full((ld,), float("nan"), dtype=torch.float64, device=DEV)
    bw = torch.full((ld,), 7.0, dtype=torch.float32, device=DEV)
    g_out = torch.full((ld,), float("nan"), dtype=torch.float64, device=DEV)
    up = UpdateRule(rule, 1e-3, 5000)
    i, eta = 3, 10.0
    decay, gm, l2, theta, code = up.coeffs(i, eta)
    combine_update([m.to(DEV) for m in msgs_t], coefs, beta, u, d, decay, gm, l2, theta, code, hist=hist, beta_w=bw,
                   g_out=g_out)
    torch.cuda.synchronize()
    M = np.stack([m.double().numpy() for m in msgs_t]).astype(nx.LD)[:, :d]
    c = np.asarray(coefs, nx.LD)[:, None]
    gref, gabs = (c * M).sum(0), np.abs(c * M).sum(0)
    g = g_out[:d].cpu().numpy()
    assert np.all(np.abs(g.astype(nx.LD) - gref) <= 2 * 2.0 ** -52 * gabs)
    # the update on that g: a handful of fp64 operations, each (or its contraction into an fma) within
    # half an ulp of its result, so 4 ulp of the terms' magnitudes; u divides the step by theta
    bref, uref = b0[:d].copy(), u0[:d].copy()
    up.apply(i, eta, bref, uref, g)
    ulp = 2.0 ** -52
    if rule == "GD":
        terms = np.abs(decay * b0[:d]) + np.abs(gm * g)
    else:
        terms = np.abs((1 - theta) * b0[:d]) + np.abs(theta * u0[:d]) + np.abs(gm * g) + np.abs(l2 * b0[:d])
    bgot = beta[:d].cpu().numpy()
    assert np.all(np.abs(bgot - bref) <= 4 * ulp * terms)
    assert torch.equal(hist[:d], beta[:d])
    if rule == "AGD":
        assert np.all(np.abs(u[:d].cpu().numpy() - uref) <= 8 * ulp * (np.abs(b0[:d]) + (terms + np.abs(b0[:d])) / theta))
    else:
        assert torch.equal(u.cpu(), torch.from_numpy(u0))
    assert torch.all(beta[d:] == 0) and torch.all(bw[d:] == 0)
    assert torch.equal(bw[:d], beta[:d].float())


def test_combine_update_refuses_more_than_max_msgs(native):
    ld = 8
    z = torch.zeros(ld, dtype=torch.float64, device=DEV)
    msgs = [z] * (native.MAX_MSGS + 1)
    with pytest.raises(ValueError):
        combine_update(msgs, [1.0] * len(msgs), z.clone(), z.clone(), ld, 1.0, 0.1, 0.0, 1.0, 0)
