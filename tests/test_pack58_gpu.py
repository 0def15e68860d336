"""The packed dense gradient (grad_dense_packed.hip) against the plain one, bit for bit (GPU only).

Two partitions of 3 * 32 + 5 rows in 32-row bundles (a short last bundle; the second shape adds a fifth bundle and
so three pad bundles in its second folded workgroup), N(0, 1) data with, per partition, an out-of-window value
planted in bundle 1 and +-0 and both window edges in bundle 2.  The packed path is forced by the plan argument;
the plain plan is what --pack off gives (pack=False).
"""
import numpy as np
import pytest
import torch

from erasurehead_amd.models.losses import LOGISTIC, SQUARED_HINGE
from erasurehead_amd.ops import DenseGradPlan, get_precision
from erasurehead_amd.ops.grad import PACK58_ROW_BYTES, KernelChoice

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (1 << 52) - 1
# AGC (W = 8, s = 2) on one GPU bundles the three replicas of a group's partitions, and the two of the last group
# padded to three: partition 0 read by three messages, partition 1 by two.  naive: one message per partition.
LAYOUTS = {"agc-lane": (3, True, [[(0, 1.0), (1, 1.0)], [(0, 0.5), (1, -2.0)], [(0, -1.5)]]),
           "agc-wave": (3, False, [[(0, 1.0), (1, 1.0)], [(0, 0.5), (1, -2.0)], [(0, -1.5)]]),
           "frc": (2, True, [[(0, 1.0), (1, 1.0)], [(0, 0.5), (1, -2.0)]]),
           "naive": (1, False, [[(0, 1.0)], [(1, 1.0)]])}


def bits(sign, e, mant):
    return float(np.array([(sign << 63) | (e << 52) | mant], dtype=np.uint64).view(np.float64)[0])


def ieq(a, b):
    return np.array_equal(a.detach().cpu().numpy().view(np.int64), b.detach().cpu().numpy().view(np.int64))


def make_parts(d, sizes, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    parts = {}
    for p, n in enumerate(sizes):
        X = rng.standard_normal((n, d)) * scale
        y = rng.choice([-1.0, 1.0], n)
        parts[p] = (torch.from_numpy(X).to(DEV).contiguous(), torch.from_numpy(y).to(DEV))
    return parts


def choice_of(layout):
    R, lane, msgs = LAYOUTS[layout]
    return KernelChoice("multi", replicas=R, bundle_rows=32, fold=True, lane_epi=lane), msgs


def written_slab(plan):
    """The slab rows a folded launch writes: those of the first bundle of every workgroup."""
    R = plan.choice.replicas
    t = plan.tasks.cpu().numpy().reshape(-1, R, 5)
    rows = sorted(int(t[b, q, 4]) for b in range(0, t.shape[0], 4) for q in range(R) if t[b, q, 1] >= 0)
    return plan.slab[torch.tensor(rows, device=DEV)]


def three_rounds(plan, d, n):
    """Three gradient-descent rounds from one start; every round's messages, the slab rows and the betas."""
    g = torch.Generator().manual_seed(1)
    beta = torch.zeros(plan.ld, dtype=torch.float64, device=DEV)
    beta[:d] = (torch.randn(d, generator=g, dtype=torch.float64) * 0.1).to(DEV)
    beta[7] = 0.0  # the planted column: keeps z finite
    out = []
    for _ in range(3):
        G = plan.out_buffer()[0]
        plan.run(beta, G)
        torch.cuda.synchronize()
        out += [G.clone(), written_slab(plan).clone()]
        beta = beta - (0.5 / n) * G.sum(0)
        beta[7] = 0.0
        out.append(beta.clone())
    return out


@pytest.mark.parametrize("sizes", [(101, 101), (101, 133)])
@pytest.mark.parametrize("loss", [LOGISTIC, SQUARED_HINGE])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("d", [1000, 520])
def test_packed_is_bitwise_the_plain_gradient(d, layout, loss, sizes, native):
    prec = get_precision("fp64")
    choice, msgs = choice_of(layout)
    parts = make_parts(d, sizes, seed=d + len(msgs))
    probe = DenseGradPlan(msgs, parts, prec, loss, d, choice=choice, pack=True)
    assert probe.packed and probe.plain_bundles == 0  # N(0, 1) fits its window whole
    for p, (X, _) in parts.items():
        e0 = probe.pack_e0[p]
        X[32 + 3, 7] = 1e300  # bundle 1: out of the window
        X[64 + 1, 0], X[64 + 2, d - 1] = 0.0, -0.0  # bundle 2: zeros and both edges of the window
        X[64 + 5, 11], X[64 + 6, d - 2] = bits(0, e0, 0), bits(1, e0 + 30, FULL)
    del probe
    packed = DenseGradPlan(msgs, parts, prec, loss, d, choice=choice, pack=True)
    assert packed.packed and sorted(packed.pack_e0) == sorted(parts)
    R = choice.replicas
    lead = packed.tasks.cpu().numpy().reshape(-1, R, 5)[:, 0, :]
    live = lead[:, 1] >= 0
    assert live.sum() == sum(-(-n // 32) for n in sizes) and len(live) % 4 == 0
    assert (len(live) - live.sum() > 0) == (sizes[1] == 133)  # the second shape has pad bundles
    want = live & (lead[:, 2] != 32)  # the planted bundle of every partition, and only it, reads the plain rows
    assert np.array_equal(packed.bundle_flags, want)
    assert packed.packed_bundles == want.sum() and packed.plain_bundles == len(sizes)
    nrows = lead[:, 3] - lead[:, 2]
    assert packed.x_stream_bytes == nrows[want].sum() * PACK58_ROW_BYTES + 32 * len(sizes) * packed.ld * 8
    assert packed.distinct_bytes == sum(sizes) * packed.ld * 8

    plain = DenseGradPlan(msgs, parts, prec, loss, d, choice=choice, pack=False)
    assert not plain.packed and plain.packed_bundles == 0 and plain.x_stream_bytes == plain.distinct_bytes
    n = sum(sizes)
    a, b = three_rounds(packed, d, n), three_rounds(plain, d, n)
    for k, (x, y) in enumerate(zip(a, b)):
        assert ieq(x, y), ("messages", "slab rows", "beta")[k % 3] + f" of round {k // 3}"
    assert torch.isfinite(a[-1]).all() and (a[-1][:d] != a[2][:d]).any()
    again = three_rounds(packed, d, n)  # a second run of the packed plan is the first
    assert all(ieq(x, y) for x, y in zip(a, again))
    fresh = packed.native_launcher()  # a further launcher of the plan reuses the packed copy
    assert fresh.packed
    G = packed.out_buffer()[0]
    beta0 = torch.zeros(packed.ld, dtype=torch.float64, device=DEV)
    fresh.launch(beta0, G)
    G2 = plain.out_buffer()[0]
    plain.run(beta0, G2)
    torch.cuda.synchronize()
    assert ieq(G, G2)


@pytest.mark.parametrize("layout", ["agc-lane", "naive"])
def test_a_plan_of_plain_bundles_only_is_the_plain_plan(layout, native):
    """Rows scaled by 2^200 against the window of the unscaled ones: NaN-free, and every bundle is flag 0."""
    prec, d, sizes = get_precision("fp64"), 1000, (101, 101)
    choice, msgs = choice_of(layout)
    e0 = DenseGradPlan(msgs, make_parts(d, sizes, 3), prec, LOGISTIC, d, choice=choice, pack=True).pack_e0[0]
    parts = make_parts(d, sizes, 3, scale=2.0 ** 200)
    packed = DenseGradPlan(msgs, parts, prec, LOGISTIC, d, choice=choice, pack=True, pack_e0=e0)
    assert packed.packed and packed.packed_bundles == 0 and packed.plain_bundles == 8
    assert packed.x_stream_bytes == packed.distinct_bytes
    plain = DenseGradPlan(msgs, parts, prec, LOGISTIC, d, choice=choice, pack=False)
    beta = torch.full((packed.ld,), 2.0 ** -210, dtype=torch.float64, device=DEV)
    G, G2 = packed.out_buffer()[0], plain.out_buffer()[0]
    packed.run(beta, G)
    plain.run(beta, G2)
    torch.cuda.synchronize()
    assert ieq(G, G2) and ieq(written_slab(packed), written_slab(plain)) and torch.isfinite(G).all()
    # the window that holds the scaled rows packs all of them
    auto = DenseGradPlan(msgs, parts, prec, LOGISTIC, d, choice=choice, pack=True)
    assert auto.pack_e0[0] == e0 + 200 and auto.plain_bundles == 0
    G3 = auto.out_buffer()[0]
    auto.run(beta, G3)
    torch.cuda.synchronize()
    assert ieq(G3, G2)


@pytest.mark.parametrize("prec_name", ["fp32", "bf16", "fp32x64"])
def test_other_precisions_stay_plain(prec_name, native):
    prec, d = get_precision(prec_name), 1000
    rng = np.random.default_rng(0)
    parts = {p: (torch.from_numpy(rng.standard_normal((101, prec.ld(d)))).to(prec.storage).to(DEV).contiguous(),
                 torch.from_numpy(rng.choice([-1.0, 1.0], 101)).to(prec.acc).to(DEV)) for p in range(2)}
    msgs = LAYOUTS["agc-lane"][2]
    plan = DenseGradPlan(msgs, parts, prec, LOGISTIC, d)
    assert not plan.packed and plan.packed_bundles == 0 and plan.x_stream_bytes == plan.distinct_bytes
    choice = KernelChoice("multi", replicas=3, bundle_rows=32, fold=True, lane_epi=True)
    if prec_name != "bf16":  # (bf16 rows take other kernels; fp32 / fp32x64 run this one, plain)
        with pytest.raises(ValueError):
            DenseGradPlan(msgs, parts, prec, LOGISTIC, d, choice=choice, pack=True)


def test_small_fp64_plans_stay_plain_by_default(native):
    """Below the long-stream rule the default is the plain plan, whatever the switch says."""
    prec, d = get_precision("fp64"), 1000
    plan = DenseGradPlan(LAYOUTS["agc-lane"][2], make_parts(d, (101, 101), 5), prec, LOGISTIC, d)
    assert not plan.packed and plan.packed_bundles == 0
