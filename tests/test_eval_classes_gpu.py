"""The multi-class evaluation kernel (csrc/kernels/eval_classes.hip) through ops/eval.class_loss_sums, against a plain
NumPy longdouble reference, at the smallest shapes its tiling can get wrong: rows and rounds on, one below and one
above a workgroup's share, every class padding (C = 2 | 3, 4 | 5, 8), a ragged K tile, padded and unaligned rows.

Loss sums.  fp64 and fp32x64 are held to the engine's evaluation tolerance, rtol 1e-9 / atol 1e-11.  fp32 logits carry
the GEMM's fp32 rounding, so its bound is measured: FP32's rtol is four times the largest relative deviation of the
torch path the kernel replaces (engine/evaluate._softmax_sums / _ovr_sums with fused=False) from the same reference on
these very cases: the constants below (docs/PERF_NOTES.md "Multi-class evaluation in the GEMM epilogue").

Hit counts are exact.  A computed logit is within d u sum_k |x_k b_k| of the true one (u = 2^-24 for fp32, 2^-53 for
fp64 arithmetic), so rows whose two largest reference logits lie closer than the sum of their two bounds in some round
are left out when the case is drawn; at most 2 % of the drawn rows may go."""
import functools

import numpy as np
import pytest
import torch

from erasurehead_amd.ops.eval import class_loss_sums

pytestmark = pytest.mark.gpu
LD = np.longdouble
DTYPES = {"fp64": (torch.float64, torch.float64), "fp32": (torch.float32, torch.float32),
          "fp32x64": (torch.float32, torch.float64)}
TOL64 = dict(rtol=1e-9, atol=1e-11)
# Largest relative deviation of the torch path from the reference, measured on the MI355X: 9.329e-08 over the fp32 CASES
# below (the fused kernel measured the same 9.329e-08: it sums K in the same order), 7.630e-07 over the fp32 cases of the
# common-logit test (fused: 7.630e-07), whose logits near 800 carry an absolute fp32 error of ~5e-5 into a loss of ~3.
FP32 = dict(rtol=4 * 9.329e-08, atol=0.0)
FP32_COMMON = dict(rtol=4 * 7.630e-07, atol=0.0)
ROWS, COLS = 128, 112  # a workgroup's rows and staged columns; held to the kernel's constants in every case


def _n(k, dn):
    return k * ROWS + dn


def _rounds(C, k, dr):
    return k * (COLS // (2 if C <= 2 else 4 if C <= 4 else 8)) + dr


@functools.lru_cache(maxsize=None)
def _case(prec, C, d, n, R, pad, twins=None, common=0.0):
    """X [n, d + pad] (NaN in the padding), class labels y, B [R * C, d + pad]; twins (a, b): class b's model rows
    are bitwise class a's, twice as large; common: a column of ones whose weight is ``common`` in every model."""
    xt, at = DTYPES[prec]
    rng = np.random.RandomState(7 * C + 13 * d + 101 * n + R + len(prec))
    draw = n + 8 + n // 8
    X = torch.from_numpy(rng.randn(draw, d)).to(xt).double().numpy()
    B = torch.from_numpy(3.0 * rng.randn(R, C, d) / np.sqrt(d)).to(at).double().numpy()
    if twins:
        B[:, twins[0]] *= 2.0
        B[:, twins[1]] = B[:, twins[0]]
    if common:
        X[:, d - 1], B[:, :, d - 1] = 1.0, common
    B = B.reshape(R * C, d)
    Z = (X.astype(LD) @ B.astype(LD).T).reshape(draw, R, C)
    bound = (d * 2.0 ** (-24 if at == torch.float32 else -53)) * (np.abs(X) @ np.abs(B).T).reshape(draw, R, C)
    if twins:  # the later twin ties exactly and never wins: it takes no part in the gap
        Z, bound = np.delete(Z, twins[1], 2), np.delete(bound, twins[1], 2)
    top = np.sort(Z, axis=2)
    sure = np.all(top[:, :, -1] - top[:, :, -2] > 2 * bound.max(axis=2), axis=1)
    assert sure.mean() >= 0.98, f"{1 - sure.mean():.3f} of the rows left out"
    X = X[sure][:n]
    y = rng.randint(0, C, n).astype(np.float64)
    y[0], y[-1] = 0, C - 1
    if twins:
        y[n // 2] = twins[1]
    Xp, Bp = np.full((n, d + pad), np.nan), np.full((R * C, d + pad), np.nan)
    Xp[:, :d], Bp[:, :d] = X, B
    return torch.from_numpy(Xp).to(xt), torch.from_numpy(y).to(at), torch.from_numpy(Bp).to(at)


def reference(X, y, B, C, d, mode):
    """(loss sums [R], hit counts [R]) in longdouble from Z = X[:, :d] @ B[:, :d].T."""
    X, y, B = (t.double().numpy().astype(LD) for t in (X, y, B))
    Z = (X[:, :d] @ B[:, :d].T).reshape(X.shape[0], -1, C)
    own = y[:, None, None] == np.arange(C)[None, None, :]
    if mode == 0:
        m = Z.max(axis=2)
        loss = np.log(np.exp(Z - m[:, :, None]).sum(axis=2)) + m - np.where(own, Z, 0).sum(axis=2)
    else:
        t = np.where(own, Z, -Z)
        loss = (np.log1p(np.exp(-np.abs(t))) + np.maximum(-t, 0) if mode == 1 else np.maximum(1 - t, 0) ** 2).sum(axis=2)
    loss = np.where(own.any(axis=2), loss, np.nan)  # a label that is no class
    return loss.sum(axis=0), (Z.argmax(axis=2) == y[:, None]).sum(axis=0)


def _check(native, prec, C, d, mode, X, y, B, loss_tol=None):
    assert (native.EVAL_CLASS_ROWS, native.EVAL_CLASS_COLS) == (ROWS, COLS)
    want_loss, want_hits = reference(X, y, B, C, d, mode)
    loss, hits = class_loss_sums(X.cuda(), y.cuda(), B.cuda(), C, d, mode, acc=DTYPES[prec][1])
    dev = np.max(np.abs(loss - want_loss) / np.maximum(np.abs(want_loss), 1e-300))
    print(f"{prec} C={C} d={d} mode={mode} n={X.shape[0]} R={len(loss)}: loss deviation {float(dev):.3e}")
    np.testing.assert_array_equal(hits, want_hits.astype(np.float64))
    np.testing.assert_allclose(loss, want_loss.astype(np.float64), **(loss_tol or (FP32 if prec == "fp32" else TOL64)))


# (precision, mode, C, d, padding columns, n = k * ROWS + dn, R = k * (rounds of a workgroup) + dr); fp32 at d = 1000
# only with few rounds (its logit bound leaves out ~0.3 % of the rows per round)
CASES = [
    ("fp64", 0, 2, 37, 3, (1, 1), (1, 1)), ("fp64", 1, 2, 1000, 0, (1, 0), (1, 0)), ("fp32x64", 2, 2, 1, 3, (1, -1), (1, -1)),
    ("fp64", 0, 3, 1000, 4, (1, -1), (1, 1)), ("fp32x64", 1, 4, 37, 3, (1, 1), (1, 0)), ("fp64", 2, 3, 37, 0, (0, 1), (1, -1)),
    ("fp64", 0, 8, 37, 0, (1, 0), (1, 1)), ("fp64", 1, 5, 1000, 4, (1, 1), (1, 0)), ("fp32x64", 0, 5, 37, 3, (1, -1), (1, -1)),
    ("fp64", 2, 8, 1, 0, (1, 1), (0, 1)), ("fp32x64", 0, 4, 1000, 0, (2, 1), (0, 1)),
    ("fp32", 0, 2, 37, 3, (1, 1), (1, 1)), ("fp32", 1, 4, 37, 0, (1, 0), (1, 1)), ("fp32", 0, 8, 37, 3, (1, -1), (1, 1)),
    ("fp32", 2, 5, 1000, 4, (1, 1), (0, 1)), ("fp32", 0, 3, 1000, 0, (1, 1), (0, 2)), ("fp32", 1, 8, 1, 3, (1, 0), (1, 0)),
]


@pytest.mark.parametrize("prec,mode,C,d,pad,nk,rk", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_loss_and_hits_at_the_tile_edges(prec, mode, C, d, pad, nk, rk, native):
    _check(native, prec, C, d, mode, *_case(prec, C, d, _n(*nk), _rounds(C, *rk), pad))


@pytest.mark.parametrize("prec,C,twins", [("fp64", 4, (1, 3)), ("fp32", 4, (1, 3)), ("fp64", 8, (0, 7)), ("fp32x64", 8, (0, 7))])
def test_exact_ties_go_to_the_first_class(prec, C, twins, native):
    """Two classes with bitwise equal model rows tie exactly (at C = 8 across the two lanes of a class group): the
    earlier one is the prediction, so a row labelled with the later twin misses."""
    X, y, B = _case(prec, C, 37, ROWS + 1, 3, 3, twins=twins)
    assert (y == twins[1]).any() and (y == twins[0]).any()
    _check(native, prec, C, 37, 0, X, y, B)


@pytest.mark.parametrize("prec,C", [(p, C) for p in ("fp64", "fp32x64", "fp32") for C in (3, 8)])
def test_softmax_with_a_large_common_logit(prec, C, native):
    """Every logit sits near 800: exp(800) overflows, the max subtraction must make that harmless."""
    X, y, B = _case(prec, C, 37, ROWS - 1, 2, 3, common=800.0)
    _check(native, prec, C, 37, 0, X, y, B, loss_tol=FP32_COMMON if prec == "fp32" else None)


@pytest.mark.parametrize("bad,mode,C", [(3.0, 0, 3), (-1.0, 1, 8), (0.5, 2, 2), (8.0, 0, 8)])
def test_a_label_that_is_no_class_gives_nan_and_no_hit(bad, mode, C, native):
    X, y, B = _case("fp64", C, 37, ROWS + 1, _rounds(C, 1, 1), 3)
    y = y.clone()
    y[5] = bad
    want_loss, want_hits = reference(X, y, B, C, 37, mode)
    loss, hits = class_loss_sums(X.cuda(), y.cuda(), B.cuda(), C, 37, mode)
    assert np.all(np.isnan(want_loss)) and np.all(np.isnan(loss))
    np.testing.assert_array_equal(hits, want_hits.astype(np.float64))


def test_the_logits_are_never_stored(native):
    n, R, C, d = 16384, 64, 8, 37  # the logits [n, R * C] in fp64 would take 64 MiB
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn(n, 40, dtype=torch.float64, device="cuda", generator=g)
    B = torch.randn(R * C, 40, dtype=torch.float64, device="cuda", generator=g)
    y = torch.randint(0, C, (n,), device="cuda", generator=g).double()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss, hits = class_loss_sums(X, y, B, C, d, 0)
    assert torch.cuda.max_memory_allocated() - before < n * R * C * 8
    assert np.all(np.isfinite(loss)) and np.all((hits >= 0) & (hits <= n))


@pytest.mark.parametrize("C,mode,xdtype", [(1, 0, torch.float64), (9, 0, torch.float64), (3, 3, torch.float64),
                                           (3, 0, torch.bfloat16)])
def test_rejections_on_the_host(C, mode, xdtype, native):
    X = torch.zeros(4, 8, dtype=xdtype, device="cuda")
    with pytest.raises(RuntimeError):
        class_loss_sums(X, torch.zeros(4, device="cuda"), torch.zeros(2 * C, 8, device="cuda"), C, 8, mode)

