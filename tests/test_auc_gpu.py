"""The native AUC pair count (csrc/kernels/auc.hip) and auc_columns on GPU tensors against plain NumPy.

Reference, on the same scores with -0.0 taken as 0.0:
    U2 = sum over positives p of searchsorted(sort(neg), p, 'left') + searchsorted(sort(neg), p, 'right')
an exact integer, AUC = U2 / (2 n+ n-).
"""
import numpy as np
import pytest
import torch

from erasurehead_amd.models.losses import roc_auc
from erasurehead_amd.ops import auc_columns

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 16384  # the count kernel's tile; test_pair_sums holds it to the binding's AUC_TILE
SPECIAL = [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1e-310, -1e-310, 1e-40, -1e-40, 1e-45, 1.5, -1.5, 3e38, -3e38]


def _case(m, small_is_pos, dtype, R, seed=0):
    """(y, P on the CPU in ``dtype``) with m rows of the smaller class, classes interleaved at random; the columns
    are heavy ties, a constant, the special values, a random one and a second tied one."""
    nq = 201 if m == 1 else m + 333  # >= m, no multiple of 256, once below 256
    rng = np.random.default_rng(seed + m)
    n = m + nq
    y = np.full(n, -1.0 if small_is_pos else 1.0)
    y[rng.permutation(n)[:m]] = 1.0 if small_is_pos else -1.0
    cols = [np.round(rng.standard_normal(n), 1), np.full(n, 0.25), rng.choice(SPECIAL, n), rng.standard_normal(n),
            np.round(rng.standard_normal(n) * 3.0, 0)]
    return y, torch.from_numpy(np.stack(cols[:R], 1)).to(dtype)


def _u2(y, P):
    """Exact U2 of every column (Python ints)."""
    S = P.double().numpy()
    S = np.where(S == 0, 0.0, S)
    out = []
    for s in S.T:
        neg, p = np.sort(s[y != 1]), s[y == 1]
        out.append(int(np.searchsorted(neg, p, "left").sum()) + int(np.searchsorted(neg, p, "right").sum()))
    return out


def _device(P, sliced):
    if not sliced:
        return P.to(DEV)
    wide = torch.full((P.shape[0], P.shape[1] + 5), float("nan"), dtype=P.dtype, device=DEV)
    wide[:, 2:2 + P.shape[1]] = P.to(DEV)
    return wide[:, 2:2 + P.shape[1]]


@pytest.mark.parametrize("dtype,sliced,R", [(torch.float64, False, 5), (torch.float32, True, 5),
                                            (torch.float64, True, 1), (torch.float32, False, 1)])
@pytest.mark.parametrize("small_is_pos", [False, True])
@pytest.mark.parametrize("m", [1, T - 1, T, T + 1, 2 * T + 3])
def test_pair_sums(m, small_is_pos, dtype, sliced, R, native):
    """The integer sums, exactly: tile edges, both orientations, both dtypes, contiguous and a column slice."""
    assert native.AUC_TILE == T
    y, P = _case(m, small_is_pos, dtype, R)
    yd = torch.from_numpy(y).to(DEV)
    small = torch.nonzero(yd == (1 if small_is_pos else -1)).squeeze(1)
    large = torch.nonzero(yd == (-1 if small_is_pos else 1)).squeeze(1)
    sums = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    flags = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    native.auc_pair_sums(_device(P, sliced), small.int() if sliced else small, large.int() if sliced else large, R,
                         sums, flags)
    want = [2 * small.numel() * large.numel() - u if small_is_pos else u for u in _u2(y, P)]
    assert flags.tolist() == [0] * R
    assert sums.tolist() == want


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("small_is_pos", [False, True])
def test_auc_columns_native(small_is_pos, dtype, monkeypatch):
    """auc_columns on GPU tensors is U2 / (2 n+ n-) to one division's rounding, agrees with roc_auc and sorts
    nothing in torch."""
    y, P = _case(T + 1, small_is_pos, dtype, 5)
    n_pos = int((y == 1).sum())
    want = np.array([float(u) / (2.0 * n_pos * (len(y) - n_pos)) for u in _u2(y, P)])

    def no_sort(*a, **k):
        raise AssertionError("torch.sort on the native AUC path")

    monkeypatch.setattr(torch, "sort", no_sort)
    got = auc_columns(torch.from_numpy(y).to(DEV), P.to(DEV), chunk=2)
    monkeypatch.undo()
    np.testing.assert_allclose(got, want, rtol=4.5e-16, atol=0)
    finite = [0, 1, 3, 4]  # roc_auc finds ties by np.diff, which is NaN between equal infinities
    np.testing.assert_allclose(got[finite], [roc_auc(y, P[:, j].double().numpy()) for j in finite], rtol=1e-12)


def test_nan_column_falls_back(native, monkeypatch):
    """A column with a NaN equals the CPU result, its neighbours the integer path; one class launches nothing."""
    y, P = _case(T + 1, False, torch.float64, 3)
    P[5, 1] = float("nan")
    yd, Pd = torch.from_numpy(y).to(DEV), P.to(DEV)
    got = auc_columns(yd, Pd)
    cpu = auc_columns(torch.from_numpy(y), P)
    assert got[1] == cpu[1]
    n_pos = int((y == 1).sum())
    u2 = _u2(y, P)
    np.testing.assert_allclose(got[[0, 2]], [float(u2[j]) / (2.0 * n_pos * (len(y) - n_pos)) for j in (0, 2)],
                               rtol=4.5e-16, atol=0)

    def no_launch(*a, **k):
        raise AssertionError("a single-class y must not launch")

    monkeypatch.setattr(native, "auc_pair_sums", no_launch)
    assert np.all(np.isnan(auc_columns(torch.ones_like(yd), Pd)))


@pytest.mark.parametrize("bad", ["bf16", "row == n", "rows on the CPU"])
def test_bad_operands_raise_before_launch(bad, native):
    n = 300
    P = torch.randn(n, 2, dtype=torch.float64, device=DEV)
    small = torch.arange(0, 100, device=DEV)
    large = torch.arange(100, n, device=DEV)
    if bad == "bf16":
        P = P.bfloat16()
    elif bad == "row == n":
        large[-1] = n
    else:
        small = small.cpu()
    sums = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    flags = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    with pytest.raises((ValueError, RuntimeError)):
        native.auc_pair_sums(P, small, large, 2, sums, flags)
    torch.cuda.synchronize()
    assert sums.tolist() == [-7, -7] and flags.tolist() == [-7, -7]
