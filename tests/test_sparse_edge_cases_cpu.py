"""The case tables of tests/sparse_edge_cases.py are what they claim (no GPU): every edge a case names occurs in the
column pass's own tables, built with the arguments the GPU plan passes; the tables emulate to X_p^T u_p; the
measured constant of tests/numerics.py is current; the hostile inputs saturate; and the CPU plan stays inside
K_SPARSE on every case."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import numerics as nx
import sparse_edge_cases as sc
from erasurehead_amd.ops.grad import SparseGradPlan
from test_sparse_tables import emulate

CASES = sc.GRADIENT
BY_ID = {c.id: c for c in CASES}
LOGISTIC_CASES = [c for c in CASES if c.loss == nx.LOGISTIC]


@functools.lru_cache(maxsize=None)
def _oracle(cid, s):
    case = BY_ID[cid]
    prec, parts, beta, bh = sc.build(case)
    return nx.oracle_sparse_terms(case.loss, case.msgs[s], parts, bh)  # (gradient, K- and u-free sum, tiny's sum)


def _tile_fields(t):
    packed = t["tkeys"][:, 1].astype(np.int64)
    return packed & 1023, (packed >> 10) & 1023, packed >> 20


# ---- the tables -----------------------------------------------------------------------------------
def test_ids_are_unique_and_every_group_is_there():
    assert len(BY_ID) == len(CASES)
    groups = {c.id.split("-")[0] for c in CASES}
    assert groups == {"ragged", "fixed", "ell", "auto", "columns", "multitile", "rowblocks", "unit", "identity"}
    # least squares and squared hinge at least once per (row pass, column-pass form, precision) reached
    reached = {}
    for c in CASES:
        e = c.expect
        form = "units" if e["units"] else "identity" if e["identity"] else "blocked" if e["blocked"] else "encode"
        reached.setdefault((e["path"], e["lds"], e["idx16"], form, c.prec), set()).add(c.loss)
    assert all(v == set(nx.LOSSES) for v in reached.values()), reached
    assert {k[0] for k in reached} == {"csr", "csr_fixed", "ell"}
    assert {k[3] for k in reached} == {"units", "identity", "blocked", "encode"}


def test_thresholds_are_the_plans():
    """The constants the tables are built from: the plan's, and for the kernel-only ones the values the launcher
    documents (ops/grad.py MAX_WG_TILES <= kMaxWgTiles, TILE = kTileEntries)."""
    assert (sc.TILE, sc.ROW_BLOCK, sc.UNIT_ROWS, sc.MAX_DST) == (512, 4096, 8192, 4)
    assert sc.ELL_LDS_BYTES == 148 * 1024 and sc.MAX_WG_TILES == 128 and sc.WG_SLOTS == 512
    from erasurehead_amd.ops import get_precision
    assert [sc.lds_limit(get_precision(p)) for p in sc.PRECS] == [18944, 37888]
    assert sc.RUN_CAP < sc.TILE and sc.ELL_MAX_FIELDS == 1024


@pytest.mark.parametrize("case", LOGISTIC_CASES, ids=[c.id for c in LOGISTIC_CASES])
def test_the_named_row_pass_follows_from_the_data(case):
    """The preconditions of the path a case names, from its matrices alone: ragged rows for the row_ptr pass, one
    count everywhere for the fixed and ELL ones, the fields' windows against 65536, beta against the LDS limit."""
    prec, parts, beta, bh = sc.build(case)
    used = sorted({p for m in case.msgs for p, _ in m})
    nnz = np.concatenate([np.diff(parts[p][0].indptr) for p in used])
    e = case.expect
    fits = case.d <= sc.lds_limit(prec)
    fixed = nnz.size > 0 and nnz.min() == nnz.max() and nnz[0] > 0
    assert e["path"] in ("csr", "csr_fixed", "ell")
    if e["path"] == "csr":
        assert not fixed, "ragged rows (csr_fixed == 0) need differing counts"
        if case.id.split("-")[0] in ("ragged", "identity", "unit"):
            assert nnz.min() == 0, "an empty row"
            assert nnz.max() > sc.CSR_LANES or case.d <= sc.CSR_LANES, "a row longer than the 8-lane group"
    else:
        assert fixed
        want_ell = fits if case.use_ell == "auto" else bool(case.use_ell)
        assert (e["path"] == "ell") == want_ell
    if e["path"] == "ell":
        m = int(nnz[0])
        X = sps.vstack([parts[p][0] for p in used], format="csr")
        idx = X.indices.reshape(-1, m)
        width = int((idx.max(0) - idx.min(0) + 1).max())
        assert e["idx16"] == (width <= sc.ELL_WINDOW)
        if "window" in case.id:
            assert width == int(case.id.split("window")[1].split("-")[0])
        assert e["lds"] == (fits and m <= sc.ELL_MAX_FIELDS)
    all_ones = all(np.all(parts[p][0].data == 1.0) for p in used)
    assert all_ones == (not case.valued)


def test_the_ell_field_counts_sit_on_the_batches():
    """m = 1, KB - 1, KB, KB + 1, 2 KB + 1 for each ELL variant's batch, both parities of the row count, 1 and 2
    rows, kEllMaxFields and one more, d on the LDS limit, odd below it and one past it."""
    from erasurehead_amd.ops import get_precision
    for pn in sc.PRECS:
        lim = sc.lds_limit(get_precision(pn))
        for valued, kb in ((True, sc.KB_LDS_VALUED), (False, sc.KB_LDS_PATTERN16)):
            lds = [c for c in CASES if c.prec == pn and c.valued == valued and c.expect["path"] == "ell" and c.expect["lds"]]
            ms = {int(np.diff(sc.build(c)[1][0][0].indptr)[0]) for c in lds}
            assert {1, kb - 1, kb, kb + 1, 2 * kb + 1} - {0} <= ms
            rows = {sum(sc.layout_rows(c.layout)) for c in lds}
            assert {1, 2} <= rows and any(r % 2 for r in rows if r > 2) and any(r % 2 == 0 for r in rows if r > 2)
            assert {lim, lim - 1} <= {c.d for c in lds} and (lim - 1) % 2 == 1
            far = [c for c in CASES if c.prec == pn and c.valued == valued and c.expect["path"] == "ell" and not c.expect["lds"]]
            ms = {int(np.diff(sc.build(c)[1][0][0].indptr)[0]) for c in far if c.d == lim + 1}
            assert {1, sc.KB_ELL - 1, sc.KB_ELL, sc.KB_ELL + 1, 2 * sc.KB_ELL + 1} <= ms
        fields = {(int(np.diff(sc.build(c)[1][0][0].indptr)[0]), c.d <= lim) for c in CASES
                  if c.prec == pn and "fields" in c.id}
        assert fields == {(sc.ELL_MAX_FIELDS, True), (sc.ELL_MAX_FIELDS + 1, True), (sc.ELL_MAX_FIELDS, False)}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_tables_show_the_claimed_edges(case):
    """csc_tables with the production arguments: the sub-block count, the merged units, the blocked / identity form
    and every nruns, n, span flag and crossing column the case names."""
    t, blocks, rb, units = sc.production_tables(case)
    e, cl = case.expect, case.claims
    assert t["wg_spans"], "column-aligned chunks stayed on"
    assert t["row16"], "sub-blocks of at most 8192 rows keep 16-bit CSC rows"
    assert (units is not None) == e["units"] and units == sc.claimed_units(case)
    assert t["nsub"] == e["nsub"]
    assert (t["nsub"] != len(blocks)) == e["blocked"]
    basis = sorted({p for m in case.msgs for p, _ in m})
    identity = e["units"] or (not e["blocked"] and len(case.msgs) == len(basis)
                              and all(tuple(m) == ((basis[i], 1.0),) for i, m in enumerate(case.msgs)))
    assert identity == e["identity"]
    assert all(1 <= w[2] <= sc.MAX_WG_TILES and w[3] <= rb for w in t["wg"])
    if e["units"]:
        rows = [b[0].shape[0] for b in blocks]
        assert max(rows) == sc.UNIT_ROWS and min(rows) == 1 and rb == sc.UNIT_ROWS
        sets = sc.message_sets(case.msgs)
        assert max(sets.count(u) for u in units) == sc.MAX_DST
    if not cl:
        return
    n, nruns, flags = _tile_fields(t)
    if "nruns" in cl:
        assert cl["nruns"] <= set(nruns.tolist()), sorted(set(nruns.tolist()))
    if "n" in cl:
        assert cl["n"] <= set(n.tolist())
    if "flags" in cl:
        assert cl["flags"] <= set(flags.tolist())
    if "span_tiles" in cl:
        assert len(t["wspan"]) and int((t["wspan"][:, 3] - t["wspan"][:, 2] + 1).max()) >= cl["span_tiles"]
    if "boundary_column" in cl:  # the column after the 8-tile one starts a tile, which has no head
        k = np.nonzero((t["tkeys"][:, 3] == cl["boundary_column"]) & (flags & 1 == 0))[0]
        assert k.size and np.all(t["tiles"][k, 1] % sc.TILE == 0)
        assert int((t["wspan"][:, 3] - t["wspan"][:, 2] + 1).max()) == sc.ROW_BLOCK // sc.TILE
    if cl.get("spans_in_subs"):
        sub_rows = [min(rb, A.shape[0] - r) for A, _ in blocks for r in range(0, max(A.shape[0], 1), rb)]
        with_span = set(t["wspan"][:, 0].tolist())
        assert all(s in with_span for s, r in enumerate(sub_rows) if r >= 2 * sc.TILE)
        assert sorted(r for r in sub_rows if r) == [1, 1, sc.ROW_BLOCK - 1] + [sc.ROW_BLOCK] * 4
    if case.id.startswith("columns"):
        # compacted and uncompacted tiles each carry a head and a tail somewhere, and a 1-run tile has both
        compact = nruns <= sc.RUN_CAP
        for bit in (1, 2):
            assert np.any(compact & (flags & bit != 0)) and np.any(~compact & (flags & bit != 0))
        assert np.any((nruns == 1) & (flags == 3)) and np.any((nruns == 1) & (flags == 0) & (n == sc.TILE))
        assert np.any((n == sc.TILE - 1) & (flags & 1 != 0)) and np.any((n == 1) & (nruns == 1))


def test_unit_fallbacks_are_one_past_the_limits():
    by = {c.id.split("-fp")[0]: c for c in CASES if c.id.startswith("unit") and c.loss == nx.LOGISTIC}
    rows = sc.layout_rows(by["unit-8193"].layout)
    assert rows[0] + rows[1] == sc.UNIT_ROWS + 1 and sc.claimed_units(by["unit-8193"]) is None
    sets = sc.message_sets(by["unit-5members"].msgs)
    assert max(sets.count(s) for s in sets) == sc.MAX_DST + 1 and sc.claimed_units(by["unit-5members"]) is None
    merged = by["unit-8192x4"]
    assert sc.claimed_units(merged) == [(0, 1), (2, 3)] and sc.layout_rows(merged.layout)[3] == 0
    assert len(set(np.diff(sc.build(merged)[1][0][0].indptr).tolist())) > 1  # ragged rows inside the unit


EMULATED = [c for c in LOGISTIC_CASES if c.id.split("-")[0] in ("columns", "multitile", "rowblocks", "unit", "identity")
            or c.id.startswith("ragged-fp64-val-d37")]


@pytest.mark.parametrize("case", EMULATED, ids=[c.id for c in EMULATED])
def test_tables_emulate_to_the_transposed_product(case):
    """tests/test_sparse_tables.py's emulation of the keyed column pass on the production tables: every column of
    every sub-block written exactly once, and the sub-block sums are X_p^T u_p."""
    t, blocks, rb, units = sc.production_tables(case)
    rng = np.random.RandomState(1)
    u = [rng.randn(A.shape[0]) for A, _ in blocks]
    u_sub = [u[j][r:r + rb] for j, (A, _) in enumerate(blocks) for r in range(0, max(A.shape[0], 1), rb)]
    assert len(u_sub) == t["nsub"]
    got = emulate(t, u_sub, case.d, keyed=True)
    sb = t["sub_begin"]
    for j, (A, _) in enumerate(blocks):
        acc = np.zeros(case.d)
        for s in range(sb[j], sb[j + 1]):
            acc = acc + got[s]
        np.testing.assert_allclose(acc, A.T.dot(u[j]), rtol=1e-12, atol=1e-12)


# ---- the measured constant --------------------------------------------------------------------------
def _plain_message(case, s, npacc):
    """The plain same-precision path: scipy CSR X.dot(b), the residual in the accumulator dtype, X.T.dot(r)."""
    prec, parts, beta, bh = sc.build(case)
    b = bh.astype(npacc)
    g = np.zeros(case.d, npacc)
    one = npacc(1)
    with np.errstate(over="ignore"):
        for p, coef in case.msgs[s]:
            A, y = parts[p]
            A, y, c = A.astype(npacc), y.astype(npacc), npacc(coef)
            z = A.dot(b)
            if case.loss == nx.LOGISTIC:
                r = -(c * y) * (one / (one + np.exp(y * z)))
            elif case.loss == nx.LEAST_SQUARES:
                r = npacc(-2) * c * (y - z)
            else:
                r = npacc(-2) * c * y * np.maximum(npacc(0), one - y * z)
            assert z.dtype == npacc and r.dtype == npacc
            g = g + A.T.dot(r)
    assert g.dtype == npacc
    return g


def test_measured_sparse_ratio_is_current():
    """MEASURED_SPARSE_CPU_RATIO is the largest err_j / (u sum ...) of the plain path over every gradient case, in
    the case's own precision: not below the re-measured value, at most 1.25 x it; K_SPARSE follows the rule."""
    worst, where = 0.0, ""
    for case in CASES:
        prec = sc.build(case)[0]
        npacc = np.float64 if prec.acc == torch.float64 else np.float32
        for s in range(len(case.msgs)):
            ref, acc, _ = _oracle(case.id, s)
            q = nx.column_ratio(_plain_message(case, s, npacc), ref, nx.LD(nx.acc_eps(prec)) * acc)
            if q > worst:
                worst, where = q, f"{case.id} message {s}"
    print(f"measured sparse CPU ratio {worst:.4f} at {where}")
    assert np.isfinite(worst)
    assert worst <= nx.MEASURED_SPARSE_CPU_RATIO <= 1.25 * worst, (worst, where)
    assert nx.K_SPARSE == nx.sparse_k_rule(nx.MEASURED_SPARSE_CPU_RATIO)
    assert nx.K == 8 and nx.MEASURED_CPU_RATIO == 0.72  # the dense constant is untouched


# ---- the inputs -------------------------------------------------------------------------------------
def test_margins_saturate_and_stay_live():
    """Every case of at least 5 non-zeros per row on average (and at least sparse_edge_cases.MIN_SHARE_ROWS rows: a
    share of a 1-, 2- or 11-row case is not a property of its draw): >= 10 % of the rows with |z| > 30 and
    >= 30 % with |z| < 30, by the oracle's own z.  No column is excluded from any check: there is no skip list."""
    seen = 0
    for case in LOGISTIC_CASES:
        prec, parts, beta, bh = sc.build(case)
        used = sorted({p for m in case.msgs for p, _ in m})
        rows = sum(parts[p][0].shape[0] for p in used)
        nnz = sum(parts[p][0].nnz for p in used)
        if not sc.shares_apply(rows, nnz):
            assert rows < sc.MIN_SHARE_ROWS or nnz < 5 * rows
            continue
        z = np.concatenate([nx.oracle_sparse_segment(case.loss, parts[p][0], parts[p][1], bh, 1.0)[3] for p in used])
        z = np.abs(z.astype(np.float64))
        assert np.mean(z > nx.SATURATED) >= 0.10 and np.mean(z < nx.SATURATED) >= 0.30, (
            case.id, float(np.mean(z > nx.SATURATED)), float(np.mean(z < nx.SATURATED)))
        seen += 1
    assert seen >= 50


def test_hostile_sparse_partition_is_what_it_says():
    from erasurehead_amd.ops import get_precision
    rng = np.random.RandomState(0)
    for pn in sc.PRECS:
        prec = get_precision(pn)
        A, y = nx.hostile_sparse_partition(rng, 300, 37, sc.RAGGED_COUNTS, True, prec)
        c = np.diff(A.indptr)
        assert set(c.tolist()) <= {min(k, 37) for k in sc.RAGGED_COUNTS} and 0 in c and 37 in c
        for i in range(300):
            row = A.indices[A.indptr[i]:A.indptr[i + 1]]
            assert np.all(np.diff(row) > 0) and (row.size == 0 or (row[0] >= 0 and row[-1] < 37))
        assert set(y.tolist()) == {-1.0, 1.0}
        if pn == "fp32":
            assert np.array_equal(A.data, A.data.astype(np.float32).astype(np.float64))
        P, _ = nx.hostile_sparse_partition(rng, 50, 37, (0, 5), False, prec)
        assert np.all(P.data == 1.0)
        Z, yz = nx.hostile_sparse_partition(rng, 0, 37, (3,), True, prec)
        assert Z.shape == (0, 37) and Z.nnz == 0 and yz.size == 0


def test_zero_bound_columns_have_a_zero_oracle():
    """A column without an entry in any partition of a message, and every column of a coefficient-0.0 message, has
    bound 0 and an oracle of exactly 0."""
    for case in LOGISTIC_CASES[::7]:
        for s in sc.dead_messages(case):
            ref, acc, tiny = _oracle(case.id, s)
            assert np.all(acc == 0) and np.all(tiny == 0) and np.all(ref == 0)
        ref, acc, tiny = _oracle(case.id, 0)
        assert np.all(ref[acc == 0] == 0) and np.all(tiny[acc == 0] == 0)


def test_eval_row_counts_cover_the_wave_edges():
    """Host check of the inputs: among the small cases every count of EVAL_COUNTS heads some row (an empty row, 63 /
    64 / 65 around a wave, 130 for a third step of the 64-entry loop)."""
    seen = set()
    for case in sc.EVAL:
        seen |= set(np.diff(sc.build_eval(case)[1].indptr).tolist())
    assert set(sc.EVAL_COUNTS) <= seen
    assert {c.R for c in sc.EVAL} == set(sc.EVAL_R) and {c.n for c in sc.EVAL} == set(sc.EVAL_N) | {sc.EVAL_N_STRIDE}


# ---- the CPU plan -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_cpu_plan_is_inside_k_sparse(case):
    prec, parts, beta, bh = sc.build(case)
    plan = SparseGradPlan([list(m) for m in case.msgs], parts, prec, case.loss, case.d, device="cpu")
    assert plan.pattern_only == (not case.valued)
    G = plan.run(beta, plan.out_buffer()[0])
    Gh = G.double().numpy()
    for s in range(len(case.msgs)):
        ref, acc, tiny = _oracle(case.id, s)
        nx.check_columns(Gh[s, :case.d], ref, nx.sparse_bound(acc, tiny, prec), f"{case.id} message {s}", k=nx.K_SPARSE)
    assert torch.all(G[:, case.d:] == 0)
    dead = sc.dead_messages(case)
    assert dead or case.id.startswith("unit")  # (unit messages all carry coefficient 1 and live partitions)
    assert torch.all(G[dead] == 0)


# ---- input checks -----------------------------------------------------------------------------------
def _tiny_parts():
    A = sps.csr_matrix((np.ones(4), np.array([0, 2, 1, 2], dtype=np.int32), np.array([0, 2, 3, 4], dtype=np.int32)),
                       shape=(3, 3))
    return A, np.array([1.0, -1.0, 1.0])


@pytest.mark.parametrize("what", ["index-high", "index-negative", "indptr-decreasing", "indptr-start", "indptr-end",
                                  "labels-nan", "labels-inf"])
def test_constructor_rejects_a_broken_partition(what):
    """A column index outside [0, d) (what a wrong d produces: scipy's constructor does not look), a row pointer
    that is not non-decreasing from 0 to nnz, non-finite labels: ValueError naming the partition, before
    anything else touches the matrix."""
    from erasurehead_amd.ops import get_precision
    A, y = _tiny_parts()
    good = (A.copy(), y.copy())
    d = 3
    if what == "index-high":
        A.indices[1] = 3
    elif what == "index-negative":
        A.indices[2] = -1
    elif what == "indptr-decreasing":
        A.indptr[:] = [0, 3, 2, 4]
    elif what == "indptr-start":
        A.indptr[0] = 1
    elif what == "indptr-end":
        A.indptr[-1] = 5
    elif what == "labels-nan":
        y[1] = np.nan
    else:
        y[2] = np.inf
    with pytest.raises(ValueError, match="partition 7"):
        SparseGradPlan([[(2, 1.0), (7, 1.0)]], {2: good, 7: (A, y)}, get_precision("fp64"), nx.LOGISTIC, d)
    plan = SparseGradPlan([[(2, 1.0)]], {2: good}, get_precision("fp64"), nx.LOGISTIC, d)  # the good one passes
    assert plan.nrows == 3
