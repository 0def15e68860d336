"""The hostile generator, the long-double oracle and the per-column bound of tests/numerics.py, on the
CPU: the generator saturates, the plain torch plan path stays within the bound at the K measured on
it, and the bound catches what the old max-normalised measure lets through."""
import functools

import numpy as np
import pytest
import torch

import numerics as nx
from erasurehead_amd.ops import DenseGradPlan, get_precision

GRID_D = (37, 1000, 4097)
GRID_N = (1, 65, 257)
PRECS = ("fp64", "fp32", "bf16")
MSGS = [[(0, 1.0), (1, -0.7)], [(1, 2.5)]]


def _seed(d, n, prec_name):
    """Seeds picked so that the generator conditions below hold for every partition of 65 rows or more at
    every shape of the grid (the saturated share then runs from 0.11 to 0.85).  Every partition draws its own
    column scales, so at d = 37 most offsets leave some partition whose large columns miss beta's."""
    return 7 * 100003 + 1000 * d + 10 * n + PRECS.index(prec_name)


@functools.lru_cache(maxsize=None)
def _case(d, n, prec_name):
    """Two hostile partitions (n and n // 4 + 1 rows) and a hostile beta; generated once per shape."""
    prec = get_precision(prec_name)
    rng = np.random.RandomState(_seed(d, n, prec_name))
    parts, host = {}, {}
    for p, rows in enumerate((n, n // 4 + 1)):
        X, y, Xh = nx.hostile_partition(rng, rows, d, prec)
        parts[p] = (X, y)
        host[p] = (Xh, y.double().numpy())
    beta, bh = nx.hostile_beta(rng, d, prec)
    return prec, parts, host, beta, bh


def _run_cpu(d, n, prec_name, loss):
    prec, parts, host, beta, bh = _case(d, n, prec_name)
    plan = DenseGradPlan(MSGS, parts, prec, loss, d)
    G = torch.full((len(MSGS), prec.ld(d)), float("nan"), dtype=prec.acc)
    plan.run(beta, G)
    return prec, host, bh, G


@pytest.mark.parametrize("prec_name", PRECS)
@pytest.mark.parametrize("n", [n for n in GRID_N if n >= 65])
@pytest.mark.parametrize("d", GRID_D)
def test_generator_saturates_with_both_signs(d, n, prec_name):
    """Conditions on the test input, read off the oracle's own z: between 10 % and 90 % of the rows have
    |z| > 30, and saturated rows occur with both signs of y z.  A case that violates them is a broken
    input, not a tolerance."""
    prec, parts, host, beta, bh = _case(d, n, prec_name)
    assert host[0][0].shape == (n, d)
    for p, (Xh, yh) in host.items():
        if Xh.shape[0] < 65:
            continue
        z = np.asarray(Xh, nx.LD) @ np.asarray(bh, nx.LD)
        sat = np.abs(z) > nx.SATURATED
        share = sat.mean()
        print(f"d={d} n={n} {prec_name} partition {p} ({Xh.shape[0]} rows): saturated share {share:.2f}")
        assert 0.10 <= share <= 0.90
        yz = yh * z
        assert np.any(yz[sat] > 0) and np.any(yz[sat] < 0)


def test_generator_contract():
    """Exact zeros (about 5 %), zero padding, four decades of column scale, and an empty partition."""
    prec = get_precision("bf16")
    rng = np.random.RandomState(0)
    X, y, Xh = nx.hostile_partition(rng, 257, 1001, prec)
    assert X.shape == (257, 1008) and X.dtype == torch.bfloat16 and y.dtype == torch.float32
    assert torch.all(X[:, 1001:] == 0)
    assert 0.03 < (Xh == 0).mean() < 0.08
    col = np.abs(Xh).max(0)
    assert col.max() / col.min() > 1e3
    X0, y0, Xh0 = nx.hostile_partition(rng, 0, 1001, prec)
    assert X0.shape == (0, 1008) and y0.shape == (0,) and Xh0.shape == (0, 1001)
    beta, bh = nx.hostile_beta(rng, 1001, prec)
    assert beta.shape == (1008,) and torch.all(beta[1001:] == 0) and bh.shape == (1001,)


@pytest.mark.parametrize("prec_name", PRECS)
@pytest.mark.parametrize("loss", nx.LOSSES, ids=[nx.LOSS_IDS[k] for k in nx.LOSSES])
def test_cpu_plan_path_meets_the_bound(loss, prec_name):
    """DenseGradPlan._run_torch (the same-precision torch path) against the long-double oracle, every
    column within its own bound at numerics.K, over the whole grid.  The largest ratio err / (u sum)
    seen here is what K was derived from (numerics.MEASURED_CPU_RATIO); it is printed."""
    worst, where = 0.0, None
    for d in GRID_D:
        for n in GRID_N:
            prec, host, bh, G = _run_cpu(d, n, prec_name, loss)
            assert torch.all(G[:, d:] == 0)
            for s, m in enumerate(MSGS):
                ref, bound = nx.oracle_message(loss, m, host, bh, prec)
                got = G[s, :d].double().numpy()
                nx.check_columns(got, ref, bound, f"d={d} n={n} message {s}")
                _, unit = nx.oracle_message(loss, m, host, bh, prec, k=1)
                q = nx.column_ratio(got, ref, unit)
                if q > worst:
                    worst, where = q, (d, n, s)
    print(f"{prec_name} {nx.LOSS_IDS[loss]}: largest err / (u sum) = {worst:.3f} at (d, n, message) = {where} (K = {nx.K})")
    assert worst <= nx.K


def test_k_is_eight_times_the_measured_ratio():
    assert nx.K == 2 ** int(np.ceil(np.log2(8 * nx.MEASURED_CPU_RATIO)))


# ---- the bound has teeth -------------------------------------------------------------------------
TEETH = dict(d=37, n=65, prec_name="fp32", loss=nx.LEAST_SQUARES)


# The bound grows like the row count while a gradient entry of random signs grows like its root, so
# 100 u relative lies beyond the bound at short messages only: message 0 of the n = 1 case has two rows.
TEETH_SHORT = dict(TEETH, n=1, prec_name="fp64")


def _teeth_case(case=TEETH):
    prec, parts, host, beta, bh = _case(case["d"], case["n"], case["prec_name"])
    ref, bound = nx.oracle_message(case["loss"], MSGS[0], host, bh, prec)
    return prec, host, bh, ref, bound


def _fails(got, ref, bound):
    return ~(np.abs(np.asarray(got, nx.LD) - ref) <= bound)


def test_bound_catches_a_small_column_the_old_measure_misses():
    """The oracle itself, perturbed by 100 u relative in the live column of smallest scale: beyond that
    column's bound, while the old measure max|delta| / max|ref| < 2e-4 passes it by orders of magnitude."""
    prec, host, bh, ref, bound = _teeth_case(TEETH_SHORT)
    scale = sum(np.abs(host[p][0]).sum(0) for p, _ in MSGS[0])
    j = int(np.argmin(np.where(ref != 0, scale, np.inf)))
    assert scale[j] < 1e-2 * scale.max()  # a small-scale column
    got = ref.copy()
    got[j] *= 1 + nx.LD(100 * nx.acc_eps(prec))
    bad = _fails(got, ref, bound)
    assert bad[j] and bad.sum() == 1
    old = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    assert old < 2e-4
    # and the whole column wrong by half still passes the old measure
    got[j] = ref[j] / 2
    assert float(np.max(np.abs(got - ref)) / np.max(np.abs(ref))) < 2e-4 and _fails(got, ref, bound)[j]
    with pytest.raises(AssertionError, match=f"worst column {j}"):
        nx.check_columns(np.asarray(got, np.float64), ref, bound)


def test_bound_catches_a_zeroed_last_live_column():
    prec, host, bh, ref, bound = _teeth_case()
    got = ref.copy()
    got[-1] = 0
    bad = _fails(got, ref, bound)
    assert bad[-1] and bad.sum() == 1


def test_bound_catches_a_dropped_row():
    """One row's contribution r_i x_i left out: the columns that row touches are beyond their bounds (all but
    the few where its entry is negligible against the message's other rows, whose partition may have a far
    larger scale in that column), and no column it does not touch."""
    prec, host, bh, ref, bound = _teeth_case()
    p, coef = MSGS[0][0]
    Xh, yh = host[p]
    _, _, _, z = nx.oracle_segment(TEETH["loss"], Xh, yh, bh, coef)
    r = nx.oracle_residual(TEETH["loss"], z, yh, coef)
    i = int(np.argmax(np.abs(r)))
    got = ref - r[i] * np.asarray(Xh[i], nx.LD)
    bad = _fails(got, ref, bound)
    touched = Xh[i] != 0
    assert touched.sum() > TEETH["d"] // 2
    assert not np.any(bad & ~touched)
    assert bad.sum() >= 0.9 * touched.sum()


def test_oracle_matches_the_package_losses():
    """The independent oracle and erasurehead_amd.models.losses agree on a benign input (a cross-check of
    the oracle, not of the kernels)."""
    from erasurehead_amd.models import losses as L

    rng = np.random.RandomState(3)
    X, y, b = rng.randn(50, 7) * 0.3, rng.choice([-1.0, 1.0], 50), rng.randn(7)
    fns = {nx.LOGISTIC: L.logistic_grad, nx.LEAST_SQUARES: L.least_squares_grad}
    for loss, f in fns.items():
        g = nx.oracle_segment(loss, X, y, b, -0.7)[0]
        np.testing.assert_allclose(np.asarray(g, np.float64), f(X, y, b, -0.7), rtol=1e-12, atol=1e-13)
