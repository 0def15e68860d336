"""Dense-gradient kernels on hostile inputs at every selector edge (GPU only).

Every case builds a plan over six small partitions (one of them empty), runs it three ways and holds
every column of every message to its own forward-error bound against the long-double oracle of
tests/numerics.py; the case tables are in tests/dense_edge_cases.py."""
import functools

import numpy as np
import pytest
import torch

import dense_edge_cases as ec
import numerics as nx
from erasurehead_amd.ops import DenseGradPlan, get_precision
from erasurehead_amd.ops.grad import KernelChoice, fill_splits

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _host_case(prec_name, d, sizes):
    """Hostile partitions and beta, generated once per (precision, width, row counts) and left unchanged."""
    prec = get_precision(prec_name)
    rng = np.random.RandomState((7919 * d + 31 * sum(sizes) + prec.code) % 2 ** 31)
    parts, host = {}, {}
    for p, n in enumerate(sizes):
        X, y, Xh = nx.hostile_partition(rng, n, d, prec)
        parts[p] = (X, y)
        host[p] = (Xh, y.double().numpy())
    beta, bh = nx.hostile_beta(rng, d, prec)
    return prec, parts, host, beta, bh


@functools.lru_cache(maxsize=None)
def _oracle(prec_name, d, sizes, loss, segments):
    prec, parts, host, beta, bh = _host_case(prec_name, d, sizes)
    return nx.oracle_message(loss, segments, host, bh, prec)


def _assert_no_task_reads_an_empty_segment(plan, msgs, sizes):
    """Host check before any launch: an empty partition's X pointer is null and must stay unread, so no task
    may name its segment and every task's row range is non-empty (pad slots of a bundle carry seg -1)."""
    seg_rows = [sizes[p] for m in msgs for p, _ in m]
    t = plan.tasks.cpu().numpy()
    live = t[t[:, 1] >= 0]
    assert live.shape[0] > 0
    assert np.all(live[:, 3] > live[:, 2]), "a task with an empty row range"
    for seg, r0, r1 in live[:, 1:4]:
        assert seg_rows[seg] > 0, f"a task reads segment {seg} of an empty partition"
        assert 0 <= r0 < r1 <= seg_rows[seg]


def _run_case(case, native):
    prec, parts, host, beta_h, bh = _host_case(case.prec, case.d, case.sizes)
    d, ld = case.d, prec.ld(case.d)
    msgs = ec.messages(case.replicas)
    dev = {p: (X.to(DEV), y.to(DEV)) for p, (X, y) in parts.items()}
    assert dev[ec.EMPTY][0].shape == (0, ld)
    plan = DenseGradPlan(msgs, dev, prec, case.loss, d, choice=case.choice)
    if case.choice is not None:
        assert plan.choice == case.choice
    else:
        assert plan.choice == ec.default_choice(prec, d, case.sizes, case.replicas)
    _assert_no_task_reads_an_empty_segment(plan, msgs, case.sizes)
    beta = beta_h.to(DEV)
    out = []
    for how in ("run", "launcher", "run"):
        G = torch.full((len(msgs), ld), float("nan"), dtype=prec.acc, device=DEV)
        if how == "run":
            plan.run(beta, G)
        else:
            plan.native_launcher().launch(beta, G)
        torch.cuda.synchronize()
        out.append(G)
    G = out[0]
    Gh = G.double().cpu().numpy()
    what = f"{case.id} [{plan.choice.label()}]"
    for s, m in enumerate(msgs):
        ref, bound = _oracle(case.prec, d, case.sizes, case.loss, tuple(m))
        nx.check_columns(Gh[s, :d], ref, bound, f"{what} message {s}")
    assert torch.all(G[:, d:] == 0), "padding columns must be exactly zero"
    only_empty = [s for s, m in enumerate(msgs) if all(p == ec.EMPTY for p, _ in m)]
    assert only_empty and torch.all(G[only_empty] == 0), "a message of empty partitions must be exactly zero"
    assert torch.equal(out[0], out[1]), "plan.run and the native launcher differ"
    assert torch.equal(out[0], out[2]), "two launches differ"
    return plan


DEFAULT = ec.default_cases()
FORCED = ec.forced_cases()
BUNDLE_ROWS = ec.bundle_row_cases(8) + [c for c in ec.bundle_row_cases(16) if "-R3-" in c.id or "-R9-" in c.id]


@pytest.mark.parametrize("case", DEFAULT, ids=[c.id for c in DEFAULT])
def test_default_choice_at_every_width_edge(case, native):
    """choose_kernel's own pick at d = T - 1, T, T + 1 of every selector threshold, and d = 1."""
    _run_case(case, native)


@pytest.mark.parametrize("case", FORCED, ids=[c.id for c in FORCED])
def test_forced_choice_at_its_narrowest_and_widest_row(case, native):
    """Every KernelChoice field the launchers honour, set by hand: rows in flight and beta in LDS of the fused
    kernel, every epilogue of the one-wave bundles, pair / wpr of the LDS-staged bundles, the quarter, half,
    full and 512-thread instances of the wide kernel with 1-3 replicas, MFMA bundles, the two-pass path."""
    plan = _run_case(case, native)
    if case.choice.kind == "wide" and case.replicas > 1:
        assert plan.cpl in (32, 256) and plan.choice.bundled


@pytest.mark.parametrize("case", BUNDLE_ROWS, ids=[c.id for c in BUNDLE_ROWS])
def test_bundle_row_edges(case, native):
    """Bundles of b rows over partitions of b - 1, b, b + 1, 1, 4b + 1 and 0 rows."""
    plan = _run_case(case, native)
    assert plan.bundle_rows == case.choice.bundle_rows


@pytest.mark.parametrize("prec_name,d", [("fp64", 999), ("fp32", 1000), ("bf16", 1000), ("fp64", 250)])
@pytest.mark.parametrize("replicas", [1, 3])
def test_fill_splits_the_plan_into_exactly_that_many_workgroups(prec_name, d, replicas, native):
    """KernelChoice.fill: every non-empty partition cut evenly so the folded plan has exactly ``fill``
    workgroups of 4 bundles; the empty partition gets none."""
    fill = 8
    case = ec.Case(f"{prec_name}-d{d}-fill{fill}-R{replicas}", prec_name, d, nx.LOGISTIC, ec.DEFAULT_SIZES, replicas,
                   KernelChoice("multi", replicas=replicas, bundle_rows=8, fold=True, lane_epi=replicas > 1, fill=fill))
    plan = _run_case(case, native)
    rows = {p: n for p, n in enumerate(ec.DEFAULT_SIZES)}
    splits = fill_splits(rows, fill)
    assert ec.EMPTY not in splits and sum(-(-(len(b) - 1) // 4) for b in splits.values()) == fill
    assert plan.ntasks == 4 * fill * replicas  # 4 bundles of `replicas` task slots per workgroup


def test_a_plan_of_empty_partitions_only_says_so(native):
    """Nothing to bundle: a ValueError that names the cause, not max() of an empty sequence."""
    prec = get_precision("fp64")
    X, y, _ = nx.hostile_partition(np.random.RandomState(0), 0, 1000, prec)
    parts = {0: (X.to(DEV), y.to(DEV)), 1: (X.to(DEV), y.to(DEV))}
    with pytest.raises(ValueError, match="empty"):
        DenseGradPlan([[(0, 1.0), (1, 1.0)], [(0, 1.0)]], parts, prec, nx.LOGISTIC, 1000,
                      choice=KernelChoice("multi", replicas=2, bundle_rows=8, fold=True))


def test_an_empty_partition_is_no_replica(native):
    """Two messages that share only an empty partition are distinct rows: the plan must not pick (and then
    refuse) a replica kernel for them."""
    prec, parts, host, beta, bh = _host_case("fp64", 1000, ec.DEFAULT_SIZES)
    dev = {p: (X.to(DEV), y.to(DEV)) for p, (X, y) in parts.items()}
    plan = DenseGradPlan(ec.messages(1), dev, prec, nx.LOGISTIC, 1000)
    assert plan.max_rep == 1 and plan.choice.replicas == 1
