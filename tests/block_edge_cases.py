"""Case tables of the blocked-model edge tests (tests/test_softmax_edges_gpu.py and test_stage_edges_within_the_column_bounds
of test_multimodel_gpu.py, test_ovr_gpu.py and test_cv_gpu.py): the widths at which the kernels' geometry changes,
the row counts at which a stage, a wave's share of it or a softmax pass ends, and partitions, task sizes and messages
that reach them.  A plain module (no GPU, no tests): tests/test_block_edge_cases_cpu.py holds the geometry it reads
(erasurehead_amd.ops.blockplan stage_rows / waves_per_group) to csrc/kernels/grad_blocks.h and checks that the tables
reach what they claim, so a threshold that moves forces new cases.
"""
import collections

import numpy as np

from erasurehead_amd.ops import blockplan, get_precision
from erasurehead_amd.ops.blockplan import MAX_LD, stage_rows, waves_per_group

import numerics as nx

CPL_EDGES = (256, 512)  # the last ld of 4 and of 8 columns per lane (grad_softmax_launch, grad_models_launch)
FULL_STAGE = 32  # the most rows of a stage: its labels are one 256-byte piece
MIN_STAGE = 4  # the fewest: a row per wave
# blockplan.MIN_ROWS_PER_TASK values of forced_task_rows: every partition of partition_sizes one task, so the
# 2S + 1 and 3S + 2 row partitions are tasks of three and four stages at every width; tasks that start at the odd
# rows 37 and (for three tasks) 74, several tasks to a partition
WHOLE_TASKS = 4 * FULL_STAGE + 2
ODD_TASKS = 37
TASK_ROWS = (WHOLE_TASKS, ODD_TASKS)
SOFTMAX_PRECS = ("fp64", "fp32")
SOFTMAX_CLASSES = (2, 3, 4, 5, 6, 8)  # wpg 4, 2, 2, 1, 1, 1; an idle fourth wave at 5 and 6, an inactive cB at 3 and 5
WIDTH_CLASSES = (2, 3, 5)  # wpg 4, 2, 1
CROSS_WIDTHS = (37, 1000)  # stages of 32 and of 4 rows
MODELS = ("offset", "saturated")


def geometry(prec, d, blocks):
    """(stage rows S, waves per block pair wpg) of the blocked-model kernels at d columns of ``prec`` storage."""
    return stage_rows(prec.ld(d) * prec.storage_bytes), waves_per_group(blocks)


def width_thresholds(prec):
    """Sorted ld thresholds T <= 1024 (the next width up is another geometry): the CPL edges, the last ld whose stages
    hold 32 rows and the last ld whose stages hold more than 4 -- the latter two scanned, and absent where no ld up
    to 1024 is past them (fp32 rows never reach 4-row stages)."""
    lds = range(prec.vec, MAX_LD + 1, prec.vec)
    S = {ld: stage_rows(ld * prec.storage_bytes) for ld in lds}
    T = set(CPL_EDGES)
    for keep in (lambda s: s == FULL_STAGE, lambda s: s > MIN_STAGE):
        last = max(ld for ld in lds if keep(S[ld]))
        if last < MAX_LD:
            T.add(last)
    return sorted(T)


def edge_widths(prec):
    """d = 1, one 16-byte row, T - 1 (the last vector partly padding), T and T + 1 (the next geometry, one live column
    in its last vector) for every threshold, and the full width 1024."""
    return sorted({1, prec.vec, MAX_LD} | {T + k for T in width_thresholds(prec) for k in (-1, 0, 1)})


def leaves_full_stage(prec):
    """The T + 1 width at which stage_rows leaves 32."""
    return max(ld for ld in range(prec.vec, MAX_LD + 1, prec.vec)
               if stage_rows(ld * prec.storage_bytes) == FULL_STAGE) + 1


def stage_row_counts(S, wpg):
    """Row counts of a ragged stage: one row, a wave short of / exactly / one past a row per wave of the group, the
    same around eight rows per wave (the softmax pass loop takes its second pass past 8 wpg rows and the lane mask
    cuts a pass short before), one short of the full stage, the full stage."""
    return sorted({n for n in (1, wpg - 1, wpg, wpg + 1, 8 * wpg - 1, 8 * wpg, 8 * wpg + 1, S - 1, S) if 1 <= n <= S})


def partition_sizes(S, wpg):
    """One partition per stage_row_counts value (a single task of one ragged stage), then S + 1 (a one-row second
    stage), 2S (both buffers, full), 2S + 1 and 3S + 2 (ring reuse, then a ragged stage) and the empty partition,
    which is the last."""
    return stage_row_counts(S, wpg) + [S + 1, 2 * S, 2 * S + 1, 3 * S + 2, 0]


def forced_task_rows(monkeypatch, rows):
    """Plans built inside the test cut their partitions into tasks of ``rows`` rows (blockplan.MIN_ROWS_PER_TASK)."""
    monkeypatch.setattr(blockplan, "MIN_ROWS_PER_TASK", int(rows))


def task_bounds(plan):
    """[(partition row of Gb, row_begin, row_end)] of a plan's task table."""
    return [(t[1], t[2], t[3]) for t in plan.tasks.cpu().tolist()]


def naive_messages(nparts):
    """Every partition by itself with coefficient 1: the identity path (no encode launch)."""
    return [[(p, 1.0)] for p in range(nparts)]


def coded_messages(nparts):
    """The encode path over partitions 0 .. nparts - 1, the last of them empty: two segments with a negative
    coefficient, a coefficient of exactly 0.0, pairs over the rest, the empty partition next to a non-empty one, a
    message that reads only the empty one, and a row over every partition."""
    empty, live = nparts - 1, list(range(nparts - 1))
    assert len(live) >= 6
    msgs = [[(live[-1], 1.0), (live[0], -0.7)], [(live[1], 0.0), (live[-2], 2.5)]]
    rest = live[1:-2]
    for a, b in zip(rest[0::2], rest[1::2]):
        msgs.append([(b, 1.5), (a, 0.3)])
    if len(rest) % 2:
        msgs.append([(rest[-1], -1.25)])
    msgs.append([(live[-3], 1.5), (empty, 1.0)])
    msgs.append([(empty, 1.0)])
    msgs.append([(p, (-1.0) ** p * (0.5 + 0.125 * p)) for p in range(nparts)])
    return msgs


MESSAGES = {"naive": naive_messages, "coded": coded_messages}


# ---- softmax cases -----------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "id prec d C model")


def softmax_cases():
    """The full cross of classes x precisions x models at d = 37 and 1000; every other edge width with C in {2, 3, 5},
    the offset model, both precisions.  (Each case runs both message sets under both task sizes.)"""
    out = []
    for pn in SOFTMAX_PRECS:
        for d in CROSS_WIDTHS:
            for C in SOFTMAX_CLASSES:
                for model in MODELS:
                    out.append(Case(f"{pn}-d{d}-C{C}-{model}", pn, d, C, model))
        for d in edge_widths(get_precision(pn)):
            if d not in CROSS_WIDTHS:
                for C in WIDTH_CLASSES:
                    out.append(Case(f"{pn}-d{d}-C{C}-offset", pn, d, C, "offset"))
    return out


# (d, C) -> seed where the default 1000 + d does not do.  d = 37 with C = 2 and C = 4: the default draw has |z| > 30 in
# 23 % and 35 % of the rows (the offset model's common logit is one hostile_beta draw; 40 % are required).  d = 37 with
# C = 3: the draw in which the old max-norm measure accepts a dropped row (tests/test_block_edge_cases_cpu.py
# test_old_measure_accepts_a_dropped_row); it meets every condition on the inputs like any other.
SEEDS = {(37, 2): 2037, (37, 4): 2037, (37, 3): 38037}
_softmax, _oracles, _scalar = {}, {}, {}


def lacking_partition(sizes, S):
    """The partition that lacks class C - 1: the one of exactly one full stage."""
    return sizes.index(S)


def softmax_inputs(d, prec_name, C):
    """(sizes, partitions on the CPU {p: (X storage dtype, y class indices in the accumulator dtype)}, host
    {p: (fp64 view of X, y float64)}, models {"offset" / "saturated": (beta [C ld], fp64 view [C, d])}): drawn once
    per (d, precision, C) and never changed.  The full-stage partition has no row of class C - 1."""
    key = (d, prec_name, C)
    if key not in _softmax:
        prec = get_precision(prec_name)
        S, wpg = geometry(prec, d, C)
        sizes = partition_sizes(S, wpg)
        rng = np.random.RandomState(SEEDS.get((d, C), 1000 + d))
        parts, host = {}, {}
        for p, n in enumerate(sizes):
            Xs, _, Xh = nx.hostile_partition(rng, n, d, prec)
            y, yh = nx.hostile_class_labels(rng, n, C, prec)
            if p == lacking_partition(sizes, S):
                y[y == C - 1] = 0
                yh[yh == C - 1] = 0
            parts[p] = (Xs, y.contiguous())
            host[p] = (Xh, yh)
        _softmax[key] = (sizes, parts, host, nx.hostile_softmax_models(rng, host, d, C, prec))
    return _softmax[key]


def softmax_oracle(case, kind):
    """[(gradient, sum w |x|, sum |x|)] ([C, d] each, long double) per message of MESSAGES[kind]: computed once."""
    key = (case.d, case.prec, case.C, case.model, kind)
    if key not in _oracles:
        sizes, _, host, models = softmax_inputs(case.d, case.prec, case.C)
        Bh = models[case.model][1]
        _oracles[key] = [nx.oracle_softmax_terms(m, host, Bh) for m in MESSAGES[kind](len(sizes))]
    return _oracles[key]


def check_softmax(G, case, kind, what, k=nx.K):
    """Every class block of every message of G [nslots, C ld] within its per-column bound, exact zeros in every
    padding column.  Returns the largest share of the bound reached."""
    prec = get_precision(case.prec)
    ld = prec.ld(case.d)
    got = G.double().cpu().numpy().reshape(-1, case.C, ld)
    worst = 0.0
    for s, (ref, acc, tiny) in enumerate(softmax_oracle(case, kind)):
        bound = nx.softmax_bound(acc, tiny, case.C, prec, k)
        for c in range(case.C):
            nx.check_columns(got[s, c, :case.d], ref[c], bound[c], f"{what} {kind} message {s} class {c}", k)
            worst = max(worst, nx.column_ratio(got[s, c, :case.d], ref[c], bound[c]))
    assert np.all(got[:, :, case.d:] == 0.0), f"{what} {kind}: padding columns must be exact zeros"
    return worst


# ---- the scalar-loss kernels (sweep, one-vs-rest, cross-validation) --------------------------------------
SCALAR_BLOCKS = (2, 3, 5)  # wpg 4, 2, 1
SCALAR_PRECS = ("fp64", "fp32", "fp32x64")


def scalar_widths(prec):
    """d = 37 (stages of 32 rows), 1000 (of 4; 8 in fp32 storage) and the T + 1 width at which stage_rows leaves 32."""
    return [37, 1000, leaves_full_stage(prec)]


def scalar_grid(losses):
    """[(d, loss, precision)]: losses[0] (logistic) at every width and precision; each further loss once, at d = 37
    and at the width that leaves 32, in rotating precisions."""
    out = []
    for pn in SCALAR_PRECS:
        for d in scalar_widths(get_precision(pn)):
            out.append((d, losses[0], pn))
    for i, loss in enumerate(losses[1:]):
        pn = SCALAR_PRECS[i % len(SCALAR_PRECS)]
        out.append((37, loss, pn))
        pn = SCALAR_PRECS[(i + 1) % len(SCALAR_PRECS)]
        out.append((leaves_full_stage(get_precision(pn)), loss, pn))
    return out


def scalar_inputs(d, prec_name, blocks, seed=3000):
    """(sizes, partitions on the CPU {p: (X, y +-1)}, host {p: (fp64 view of X, y float64)}, 8 hostile betas) over
    partition_sizes at this geometry: drawn once per (d, precision, blocks) and never changed."""
    key = (d, prec_name, blocks, seed)
    if key not in _scalar:
        prec = get_precision(prec_name)
        sizes = partition_sizes(*geometry(prec, d, blocks))
        rng = np.random.RandomState(seed + d)
        parts, host = {}, {}
        for p, n in enumerate(sizes):
            Xs, y, Xh = nx.hostile_partition(rng, n, d, prec)
            parts[p] = (Xs, y.contiguous())
            host[p] = (Xh, y.double().numpy())
        _scalar[key] = (sizes, parts, host, [nx.hostile_beta(rng, d, prec) for _ in range(8)])
    return _scalar[key]


def to_device(parts, dev):
    return {p: (X.to(dev).contiguous(), y.to(dev).contiguous()) for p, (X, y) in parts.items()}


def assert_tasks_reach_the_edges(plan, sizes, S, rows):
    """What a forced task size is for, read off the plan's own task table: under WHOLE_TASKS every partition is one
    task and the two longest hold at least three stages; under ODD_TASKS a partition holds several tasks and one of
    them starts at an odd row."""
    tasks = task_bounds(plan)
    if rows == WHOLE_TASKS:
        assert len(tasks) == len(sizes) and [b - a for _, a, b in tasks] == list(sizes)
        assert sum(-(-(b - a) // S) >= 3 for _, a, b in tasks) >= 2
    else:
        assert rows == ODD_TASKS
        if max(sizes) > rows:
            assert any(a % 2 == 1 for _, a, _ in tasks) and len(tasks) > len(sizes)
    return tasks
