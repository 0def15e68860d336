"""The tables of tests/newton_edge_cases.py reach what they claim, K_HVP_EDGE follows the rule of tests/numerics.py, the
block-1 bound rejects five wrong kernels, and the decode's emulator and the long-double replay agree with the NumPy twin
of ops/update.py newton_cg_update through every branch (no GPU: HvpGradPlan and the update run on CPU tensors).
"""
import numpy as np
import pytest
import torch

import block_edge_cases as bc
import newton_edge_cases as ne
import numerics as nx
import slab_edge_cases as sl
from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.hvp import HvpGradPlan
from numerics import LD

_runs = {}


def cpu_messages(d, loss, prec_name, kind):
    """G [nslots, 2 ld] of HvpGradPlan on CPU tensors (the plain same-precision torch path): computed once."""
    key = (d, loss, prec_name, kind)
    if key not in _runs:
        prec = get_precision(prec_name)
        sizes, parts, _, (beta, _) = ne.inputs(d, prec_name)
        plan = HvpGradPlan(bc.MESSAGES[kind](len(sizes)), parts, prec, loss, d)
        _runs[key] = plan.run(torch.cat([beta, ne.direction(d, prec_name)[0]]), plan.out_buffer()[0])
    return _runs[key]


# ---- the tables ------------------------------------------------------------------------------------------
def test_grid_is_the_one_described():
    assert len(ne.GRID) == len(set(ne.GRID)) == 18 + 12 + 2
    assert {(d, p) for d, _, p in ne.GRID if d not in (37, 1000)} == \
        {(d, p) for d in (1, 256, 257, 512, 513, 1024) for p in ("fp64", "fp32")} | {(129, "fp64"), (257, "fp32x64")}
    assert ne.WIDTHS == (1, 37, 256, 257, 512, 513, 1000, 1024)


@pytest.mark.parametrize("d,loss,prec_name", ne.GRID, ids=ne.GRID_IDS)
def test_tables_reach_every_stage_edge(d, loss, prec_name, monkeypatch):
    """The task table HvpGradPlan builds for these partitions: under WHOLE_TASKS every ragged-stage row count is some
    task's last stage (wpg - 1, wpg, wpg + 1, S - 1, S among them), a task of exactly 2 S rows exists, two tasks hold
    three stages or more and end in one and two rows; under ODD_TASKS tasks start at odd rows.  The squared-hinge
    margin holds with no row excluded (hvp_oracle asserts it)."""
    prec = get_precision(prec_name)
    S, wpg = bc.geometry(prec, d, 2)
    sizes, parts, _, _ = ne.inputs(d, prec_name)
    assert wpg == 4 and sizes == bc.partition_sizes(S, wpg) and sizes[-1] == 0
    assert {1, wpg - 1, wpg, wpg + 1, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S + 2} <= set(sizes)
    for rows in bc.TASK_ROWS:
        bc.forced_task_rows(monkeypatch, rows)
        for kind in ne.KINDS:
            plan = HvpGradPlan(bc.MESSAGES[kind](len(sizes)), parts, prec, loss, d)
            plan._build_tables()
            tasks = bc.assert_tasks_reach_the_edges(plan, sizes, S, rows)
            if rows == bc.WHOLE_TASKS:
                last = {(b - a - 1) % S + 1 for _, a, b in tasks if b > a}
                assert set(bc.stage_row_counts(S, wpg)) <= last, sorted(last)
                assert 2 * S in {b - a for _, a, b in tasks} and 0 in {b - a for _, a, b in tasks}
                assert {1, 2} <= {(b - a) % S for _, a, b in tasks if b - a > 2 * S}  # ragged after ring reuse
            assert plan.identity == (kind == "naive")
    for kind in ne.KINDS:
        assert len(ne.oracles(d, loss, prec_name, kind)) == len(bc.MESSAGES[kind](len(sizes)))
    coefs = [c for m in bc.coded_messages(len(sizes)) for _, c in m]
    assert 0.0 in coefs and min(coefs) < 0 and [(len(sizes) - 1, 1.0)] in bc.coded_messages(len(sizes))


def test_widths_cross_the_geometry():
    """The grid holds both sides of the columns-per-lane edges in both storage widths, d = 1 and the full width, and
    stages of 32, 31, 8, 5 or 4 rows."""
    lds = {(p, get_precision(p).ld(d)) for d, _, p in ne.GRID}
    for p in ("fp64", "fp32"):
        assert {(p, 256), (p, 512), (p, 1024)} <= lds and any(256 < ld <= 260 for q, ld in lds if q == p) and \
            any(512 < ld <= 516 for q, ld in lds if q == p)
    assert {bc.geometry(get_precision(p), d, 2)[0] for d, _, p in ne.GRID} >= {32, 31, 16, 8, 4}


# ---- the constant ------------------------------------------------------------------------------------------
def _ratio(d, loss, prec_name, kind):
    """(largest err / bound(k = 1) of block 1 over the messages, where) of the CPU plan."""
    prec = get_precision(prec_name)
    got = cpu_messages(d, loss, prec_name, kind).double().numpy().reshape(-1, 2, prec.ld(d))
    worst, where = 0.0, ""
    for s, (_, _, u, ub, _) in enumerate(ne.oracles(d, loss, prec_name, kind)):
        r = nx.column_ratio(got[s, 1, :d], u, ub)
        if r > worst:
            worst, where = r, f"d{d}-{nx.LOSS_IDS[loss]}-{prec_name} {kind} message {s} ({r:.3f})"
    return worst, where


def test_measured_hvp_ratio_is_current():
    """MEASURED_HVP_EDGE_CPU_RATIO is the largest ratio of the plain path over GRID and both message sets: reached
    within 5 % and not exceeded; K_HVP_EDGE follows the rule."""
    worst, where = max(_ratio(d, l, p, kind) for d, l, p in ne.GRID for kind in ne.KINDS)
    print(f"HvpGradPlan on CPU tensors: worst err / bound(k = 1) of block 1 = {worst:.4f} at {where}")
    assert worst <= ne.MEASURED_HVP_EDGE_CPU_RATIO <= 1.05 * worst, (worst, where)
    assert ne.K_HVP_EDGE == nx.sparse_k_rule(ne.MEASURED_HVP_EDGE_CPU_RATIO)
    assert where.startswith(ne.MEASURED_HVP_EDGE_CPU_CASE.split(" (")[0])


@pytest.mark.parametrize("d,loss,prec_name", ne.GRID, ids=ne.GRID_IDS)
def test_cpu_plan_meets_the_bounds(d, loss, prec_name):
    for kind in ne.KINDS:
        assert ne.check_messages(cpu_messages(d, loss, prec_name, kind), d, loss, prec_name, kind, "CPU plan") <= 1.0


# ---- teeth -------------------------------------------------------------------------------------------------
TEETH = [(d, l, p, m) for d, l, p in ne.GRID for m in ne.MUTANTS if ne.changes_the_mathematics(m, l)]


@pytest.mark.parametrize("d,loss,prec_name,mutant", TEETH, ids=[f"d{d}-{nx.LOSS_IDS[l]}-{p}-{m}" for d, l, p, m in TEETH])
def test_bound_rejects_the_mutants(d, loss, prec_name, mutant):
    """Each wrong kernel puts at least one column of block 1 outside K_HVP_EDGE x bound, in every grid case where it
    changes the mathematics (least squares has w = 2 wherever the curvature is taken), under both message sets (and,
    for the dropped row, both task sizes); the reference written out by rows is the oracle itself when nothing is
    mutated."""
    prec = get_precision(prec_name)
    sizes, _, host, (_, bh) = ne.inputs(d, prec_name)
    vh = ne.direction(d, prec_name)[1]
    for kind in ne.KINDS:
        msgs, orc = bc.MESSAGES[kind](len(sizes)), ne.oracles(d, loss, prec_name, kind)
        for rows in (bc.TASK_ROWS if mutant == "drop_last_row" else bc.TASK_ROWS[:1]):
            out = 0
            for m, (_, _, u, ub, tiny) in zip(msgs, orc):
                bound = ne.product_bound(ub, tiny, ne.K_HVP_EDGE)
                same = ne.block1(loss, m, host, bh, vh)
                assert np.all(np.abs(same - u) <= LD(2.0 ** -60) * (ub / LD(nx.acc_eps(prec))))  # the identity: inside
                out += int(np.sum(~(np.abs(ne.block1(loss, m, host, bh, vh, mutant, rows) - u) <= bound)))
            assert out >= 1, f"{mutant} passes in {kind} messages, tasks of {rows}: the inputs are too tame"


# ---- the decode's emulator ---------------------------------------------------------------------------------
def test_hostile_messages_are_hostile():
    for name, (npdt, _) in ne.UPDATE_DTYPES.items():
        M = ne.hostile_messages(np.random.RandomState(3), 17, 302, 301, npdt, pad=np.nan).reshape(17, 2, 302)
        live = M[:, :, :301]
        mag = np.abs(live[(live != 0) & (np.abs(live) >= np.finfo(npdt).tiny)]).astype(np.float64)
        assert np.isnan(M[:, :, 301:]).all() and np.isfinite(live).all()
        assert mag.max() / mag.min() > 1e12 and np.signbit(live[live == 0]).any() and not np.signbit(live[live == 0]).all()
        den = live[(live != 0) & (np.abs(live) < np.finfo(npdt).tiny)]
        assert den.size > 100 and np.all(M[:, :, 150] == 0) and np.signbit(M[:, :, 150]).all()
        assert np.all(np.abs(M[:, :, 300]) < np.finfo(npdt).tiny)
    for n in ne.UPDATE_NMSG:
        c = sl.update_coefs(np.random.RandomState(n), n)
        assert min(c) < 0 and (n == 1 or 0.0 in c)
    assert ne.UPDATE_NMSG[-1] == sl.MAX_MSGS and {1, 8, 16} <= set(ne.UPDATE_NMSG)
    assert {(1, 1), (256, 256), (1024, 1024)} <= set(ne.UPDATE_SHAPES) and any(d < ld for ld, d in ne.UPDATE_SHAPES)


@pytest.mark.parametrize("name", list(ne.UPDATE_DTYPES))
@pytest.mark.parametrize("nmsg", [1, 9, 17])
def test_emulator_is_the_chain_and_has_teeth(nmsg, name):
    """emulate_decode against the exact sum (every step rounds once: within nmsg ulp of sum |c m|, a step among the
    denormals to the denormals' spacing), and different in
    bits from the chain run backwards and from a plain multiply-add (where more than one message is added)."""
    ld, d, rng = 6, 5, np.random.RandomState(nmsg)
    npdt = ne.UPDATE_DTYPES[name][0]
    M, coefs = ne.hostile_messages(rng, nmsg, ld, d, npdt), sl.update_coefs(rng, nmsg)
    for block in (0, 1):
        got = ne.emulate_decode(M, coefs, ld, d, block)
        cols = M.reshape(nmsg, 2, ld)[:, block, :d].astype(LD)
        c = np.asarray(coefs, LD)[:, None]
        assert np.all(np.abs(got - (c * cols).sum(0)) <= nmsg * (LD(2.0 ** -52) * np.abs(c * cols).sum(0) + LD(2.0 ** -1074)))
    if nmsg > 1:
        wide = (rng.standard_normal((nmsg, 2 * 64)) * 10.0 ** rng.uniform(-6, 6, (nmsg, 2 * 64))).astype(npdt)
        got = ne.emulate_decode(wide, coefs, 64, 64, 0)
        back = ne.emulate_decode(wide[::-1], coefs[::-1], 64, 64, 0)
        plain = np.zeros(64)
        for m, c in zip(wide, coefs):
            plain = np.float64(c) * m[:64].astype(np.float64) + plain
        assert not np.all(sl.same_bits(got, back)) and not np.all(sl.same_bits(got, plain))
    b = rng.standard_normal(d)
    G = ne.emulate_affine(ne.GS, ne.emulate_decode(M, coefs, ld, d, 0), ne.L2C, b)
    ref = LD(ne.GS) * (np.asarray(coefs, LD)[:, None] * M.reshape(nmsg, 2, ld)[:, 0, :d].astype(LD)).sum(0) + LD(ne.L2C) * b
    assert np.all(np.abs(G - ref) <= (nmsg + 2) * LD(2.0 ** -52) * (np.abs(ref) + LD(ne.GS) * np.abs(
        np.asarray(coefs, LD)[:, None] * M.reshape(nmsg, 2, ld)[:, 0, :d].astype(LD)).sum(0) + np.abs(LD(ne.L2C) * b)))


# ---- the twin and the replay -------------------------------------------------------------------------------
def test_twin_follows_the_replay_through_every_branch():
    """SCRIPT through the NumPy twin at SCRIPT_SHAPES with MAX_MSGS messages of both types: the phase words agree with
    the long-double replay in every round (run_script asserts it), all seven modes are visited wherever CG can take
    more than one step (d > 1), and TWIN_REL is the twin's largest error per vector: not exceeded, reached within 25 %."""
    worst, where = {n: 0.0 for n in ne.VECTORS}, {}
    for ld, d in ne.SCRIPT_SHAPES:
        for name, (_, mdt) in ne.UPDATE_DTYPES.items():
            rounds, seen = ne.run_script(ld, d, sl.MAX_MSGS, mdt, "cpu")
            assert seen == (set(range(7)) if d > 1 else {0, 2, 5, 6}), (ld, d, seen)
            for i, mode, errs in rounds:
                for vec, e in errs.items():
                    if e / 2.0 ** -53 > worst[vec]:
                        worst[vec], where[vec] = e / 2.0 ** -53, f"ld={ld} d={d} {name} round {i} mode {mode}"
    print("twin error per vector in 2^-53:", {k: round(v, 3) for k, v in worst.items()}, where)
    for vec in ne.VECTORS:
        assert worst[vec] <= ne.TWIN_REL[vec] <= 1.25 * worst[vec], (vec, worst[vec], where.get(vec))
        assert where[vec] == ne.TWIN_REL_CASES[vec]


def test_replay_in_float64_is_the_twin_to_rounding():
    """The replay is written from the kernel's header, the twin from the same recurrences: in float64 the two agree to
    a few ulp of SCALE on every vector of every round (another formulation, not another method)."""
    rounds, _ = ne.run_script(6, 5, 9, torch.float64, "cpu")
    assert len(rounds) >= 10 and all(e <= 16 * 2.0 ** -53 for _, _, errs in rounds for e in errs.values())
