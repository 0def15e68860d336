"""Case tables of tests/test_sparse_edges_gpu.py: the thresholds of the sparse gradient plan and of the sparse
evaluation kernel, read off ops/grad.py SparseGradPlan where it has them (the kernel-only ones are named below
with the line they mirror), and the smallest hostile shapes that sit on them.  A plain module (no GPU, no tests):
tests/test_sparse_edge_cases_cpu.py checks from the column pass's own tables that every claimed edge occurs, so
a threshold that moves forces new cases."""
import collections
import zlib

import numpy as np
import scipy.sparse as sps
import torch

from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.grad import SparseGradPlan

import numerics as nx

TILE = SparseGradPlan.TILE
ROW_BLOCK = SparseGradPlan.ROW_BLOCK_ROWS
UNIT_ROWS = SparseGradPlan.UNIT_ROWS
MAX_DST = SparseGradPlan.MAX_DST
ELL_LDS_BYTES = SparseGradPlan.ELL_LDS_BYTES
MAX_WG_TILES = SparseGradPlan.MAX_WG_TILES
WG_SLOTS = SparseGradPlan.WG_SLOTS
# constants of csrc/kernels/grad_sparse.hip without a Python twin
RUN_CAP = 128            # constexpr int kRunCap = 128: runs per tile compacted in LDS
ELL_MAX_FIELDS = 1024    # constexpr int kEllMaxFields = 1024: window starts ell_rows_lds keeps in LDS
KB_ELL = 16              # ell_rows: constexpr int KB = 16
KB_LDS_VALUED = 4        # ell_rows_lds: constexpr int KB = VALS ? 4 : IDX16 ? 16 : 8
KB_LDS_PATTERN16 = 16
CSR_LANES = 8            # grad_sparse_launch: constexpr int Gs = 8 lanes per CSR row
ELL_WINDOW = 65536       # ops/grad.py _build_device: 16-bit offsets while every field's window is <= 65536
# csrc/kernels/eval_sparse.hip: a wave per row, 64 entries per step, 64 NC columns per lane set, 256 per launch
EVAL_COUNTS = (0, 1, 7, 8, 9, 63, 64, 65, 72, 130)
EVAL_R = (1, 63, 64, 65, 128, 129, 192, 193, 256, 257)
EVAL_N = (1, 3, 4, 5)
EVAL_N_STRIDE = 4 * 8192 + 5  # past the 8192-block grid: the grid-stride loop
EVAL_D = 140

PRECS = ("fp64", "fp32")
RAGGED_COUNTS = (0, 1, 7, 8, 9, 17, 64, 65, 100)  # the 8-lane row group at 7 / 8 / 9, multiples, empty rows

Case = collections.namedtuple("Case", "id prec loss d valued layout msgs use_ell expect claims")
# layout: one spec per partition --
#   ("h", rows, counts)          numerics.hostile_sparse_partition
#   ("heavy", rows, counts)      the same in columns 1.., and column 0 in every row
#   ("win", rows, W)             two entries per row: column 0 or W - 1 (both occur), and one in [W, d)
#   ("cols", name)               one entry per row, column lengths COLUMN_BLOCKS[name] per 4096-row sub-block
#   ("full", rows, extra)        column 5 in every row, column 9 in the first `extra` rows as well
# expect: path ("csr" | "csr_fixed" | "ell"), idx16, lds (the launcher's ELL kernel: beta and the fields fit LDS),
#         units, identity, blocked, nsub.  claims: what the column pass's tables must show (the CPU test).


def lds_limit(prec):
    """Largest d whose beta the ELL row pass stages in LDS."""
    return ELL_LDS_BYTES // (8 if prec.acc == torch.float64 else 4)


# one sub-block (or a partition's last, shorter one) per entry: the lengths of its columns in column order
COLUMN_BLOCKS = {
    "edges": (
        # 4096 rows = 8 tiles: 512 runs of 1 (uncompacted) | exactly 128 runs | exactly 129 | one 512-entry column
        # from boundary to boundary | 50 short runs and a column of 924 that leaves the tile (compacted tail),
        # fills the next (head and tail) and ends 100 into the one after (head), 206 short runs behind it
        # (uncompacted head) | 64 runs of 8
        [1] * TILE + [4] * RUN_CAP + [3] * RUN_CAP + [TILE - 3 * RUN_CAP] + [TILE]
        + [4] * 50 + [TILE - 200 + TILE + 100] + [2] * 206 + [8] * 64,
        # 1023 rows: 300 runs of 1 and a column leaving the tile (uncompacted tail) | its 100-entry head and three
        # columns of 137 (compacted head): a last tile of n = 511
        [1] * 300 + [TILE - 300 + 100] + [137] * 3,
    ),
    "one-left": ([2] * (TILE // 2) + [1],),  # 513 rows: a full tile and a last tile of n = 1
}


def _values(rng, cols, d, valued, prec):
    if not valued:
        return np.ones(cols.size)
    npacc = np.float64 if prec.acc == torch.float64 else np.float32
    scale = 10.0 ** rng.uniform(-3.0, 1.0, d)
    return (rng.randn(cols.size) * scale[cols]).astype(npacc).astype(np.float64)


def _partition(rng, spec, d, valued, prec):
    kind = spec[0]
    if kind == "h":
        return nx.hostile_sparse_partition(rng, spec[1], d, spec[2], valued, prec)
    if kind == "heavy":
        n = spec[1]
        A, y = nx.hostile_sparse_partition(rng, n, d - 1, spec[2], valued, prec)
        c = np.diff(A.indptr)
        indptr = A.indptr + np.arange(n + 1)
        cols = np.zeros(A.nnz + n, dtype=np.int32)
        data = np.zeros(A.nnz + n)
        first = indptr[:-1]
        rest = np.ones(A.nnz + n, dtype=bool)
        rest[first] = False
        cols[rest], data[rest] = A.indices + 1, A.data
        data[first] = _values(rng, np.zeros(n, dtype=np.int64), d, valued, prec)
        assert np.all(np.diff(indptr) == c + 1)
        return sps.csr_matrix((data, cols, indptr), shape=(n, d)), y
    if kind == "win":
        n, W = spec[1], spec[2]
        f0 = rng.choice([0, W - 1], n)
        f0[:2] = [0, W - 1]
        cols = np.stack([f0, rng.randint(W, d, n)], axis=1).ravel().astype(np.int32)
        return (sps.csr_matrix((_values(rng, cols, d, valued, prec), cols, np.arange(0, 2 * n + 1, 2)), shape=(n, d)),
                rng.choice([-1.0, 1.0], n))
    if kind == "cols":
        rows = []
        for lengths in COLUMN_BLOCKS[spec[1]]:
            ids = np.sort(rng.choice(d, len(lengths), replace=False))
            sub = np.repeat(ids, lengths)
            assert sub.size <= ROW_BLOCK
            rng.shuffle(sub)  # the rows permuted
            rows.append(sub)
        assert all(r.size == ROW_BLOCK for r in rows[:-1])
        cols = np.concatenate(rows).astype(np.int32)
        n = cols.size
        return (sps.csr_matrix((_values(rng, cols, d, valued, prec), cols, np.arange(n + 1)), shape=(n, d)),
                rng.choice([-1.0, 1.0], n))
    if kind == "full":
        n, extra = spec[1], spec[2]
        c = np.where(np.arange(n) < extra, 2, 1)
        indptr = np.concatenate([[0], np.cumsum(c)])
        cols = np.full(int(indptr[-1]), 5, dtype=np.int32)
        cols[indptr[:extra] + 1] = 9
        return (sps.csr_matrix((_values(rng, cols, d, valued, prec), cols, indptr), shape=(n, d)),
                rng.choice([-1.0, 1.0], n))
    raise ValueError(kind)


_BUILT = {}


def build(case):
    """(precision, {partition: (CSR, y)}, beta [ld] accumulator dtype, its fp64 view [d]); generated once per case and
    left unchanged."""
    if case.id not in _BUILT:
        prec = get_precision(case.prec)
        rng = np.random.RandomState(zlib.crc32(case.id.encode()) % 2 ** 31)
        parts = {p: _partition(rng, spec, case.d, case.valued, prec) for p, spec in enumerate(case.layout)}
        rows = sum(A.shape[0] for A, _ in parts.values())
        nnz = sum(A.nnz for A, _ in parts.values())
        for _ in range(50):  # condition the draw on the property the inputs are hostile for
            beta, bh = nx.hostile_sparse_beta(rng, case.d, prec, nnz / max(1, rows))
            if not shares_apply(rows, nnz) or shares_hold(np.concatenate([A.dot(bh) for A, _ in parts.values()])):
                break
        else:
            raise AssertionError(f"{case.id}: no beta in 50 draws saturates 10 % of the rows and leaves 30 % live")
        _BUILT[case.id] = (prec, parts, beta, bh)
    return _BUILT[case.id]


MIN_SHARE_ROWS = 40  # below this a share of 10 % is under four rows: not a property one draw can be held to


def shares_apply(rows, nnz):
    """The saturation shares are asked of a case of at least 5 non-zeros per row on average (shorter rows rarely
    reach |z| = 30 with beta scaled for them) and at least MIN_SHARE_ROWS rows."""
    return rows >= MIN_SHARE_ROWS and nnz >= 5 * rows


def shares_hold(z):
    z = np.abs(np.asarray(z, dtype=np.float64))
    return bool(np.mean(z > nx.SATURATED) >= 0.10 and np.mean(z < nx.SATURATED) >= 0.30)


def layout_rows(layout):
    out = []
    for spec in layout:
        out.append(sum(sum(b) for b in COLUMN_BLOCKS[spec[1]]) if spec[0] == "cols" else spec[1])
    return out


def message_sets(msgs):
    return [tuple(sorted(p for p, _ in m)) for m in msgs]


def claimed_units(case):
    """The merged FRC / AGC units a case claims (None: the partition basis), from the rule in words: every
    coefficient 1, a set used twice, sets identical or disjoint, at most MAX_DST messages per set and at most
    UNIT_ROWS rows per unit."""
    rows = layout_rows(case.layout)
    sets = message_sets(case.msgs)
    if any(c != 1.0 for m in case.msgs for _, c in m) or len(set(sets)) == len(sets):
        return None
    units = sorted(set(sets))
    flat = [p for u in units for p in u]
    if len(flat) != len(set(flat)) or any(sets.count(u) > MAX_DST for u in units):
        return None
    if any(sum(rows[p] for p in u) > UNIT_ROWS for u in units):
        return None
    return units


def claimed_nsub(case):
    """Sub-blocks the column pass cuts the case into: ROW_BLOCK rows each (an empty block still is one), or one per
    merged unit."""
    rows = layout_rows(case.layout)
    units = claimed_units(case)
    if units is not None:
        return len(units)
    used = sorted({p for m in case.msgs for p, _ in m})
    return sum(max(1, -(-rows[p] // ROW_BLOCK)) for p in used)


def production_tables(case):
    """The column pass's host tables with the arguments SparseGradPlan._build_device passes on the GPU:
    (tables, device blocks [(CSR, y)] in row order, row_block, merged units or None)."""
    prec, parts, beta, bh = build(case)
    plan = SparseGradPlan([list(m) for m in case.msgs], parts, prec, case.loss, case.d, device="cpu")
    units = plan._merge_units()
    pos = {p: j for j, p in enumerate(plan.basis)}
    if units is None:
        blocks = plan.blocks
    else:
        blocks = []
        for u in units:
            A = sps.vstack([plan.blocks[pos[p]][0] for p in u], format="csr")
            blocks.append((sps.csr_matrix((A.data, A.indices, A.indptr), shape=(A.shape[0], case.d)),
                           np.concatenate([plan.blocks[pos[p]][1] for p in u])))
    rb = ROW_BLOCK if units is None else max(ROW_BLOCK, max(b[0].shape[0] for b in blocks))
    t = SparseGradPlan.csc_tables([b[0] for b in blocks], case.d, TILE, row_block=rb, wg_tiles=MAX_WG_TILES,
                                  wg_spans=SparseGradPlan.WG_SPANS, slots=WG_SLOTS)
    return t, blocks, rb, units


def messages(main, second, other, zero=None, empty=None):
    """As dense_edge_cases.messages: two segments and a negative coefficient, a coefficient of exactly 0.0 next to a
    live one, a message of coefficient 0.0 only, a zero-row partition next to a non-empty one, a message reading
    only the zero-row partition, and one reading only the partition whose rows are all empty."""
    msgs = [((main, 1.0), (second, -0.7)), ((other, 0.0), (second, 2.5)), ((other, 0.0),)]
    if zero is not None:
        msgs += [((other, 1.5), (zero, 1.0)), ((zero, 1.0),)]
    if empty is not None:
        msgs += [((empty, 1.0),)]
    return tuple(msgs)


def dead_messages(case):
    """Message slots that must be exactly zero in their whole row: every coefficient 0.0, or only partitions without
    an entry."""
    rows = layout_rows(case.layout)
    out = []
    for s, m in enumerate(case.msgs):
        if all(c == 0.0 for _, c in m) or all(rows[p] == 0 or case.layout[p][0] == "h" and case.layout[p][2] == (0,)
                                                for p, _ in m):
            out.append(s)
    return out


def _expect(path, *, idx16=False, lds=False, units=False, identity=False, blocked=False):
    return dict(path=path, idx16=idx16, lds=lds, units=units, identity=identity, blocked=blocked)


def gradient_cases():
    out, seen = [], set()

    def add(tag, pn, d, valued, layout, msgs, use_ell, expect, claims=None, form="encode"):
        """logistic always; least squares and squared hinge the first time a (row pass, column-pass form, precision)
        is reached."""
        losses = [nx.LOGISTIC]
        key = (expect["path"], expect["lds"], expect["idx16"], form, pn)
        if key not in seen:
            seen.add(key)
            losses += [nx.LEAST_SQUARES, nx.SQUARED_HINGE]
        for loss in losses:
            cid = f"{tag}-{pn}-{'val' if valued else 'pat'}-d{d}-{nx.LOSS_IDS[loss]}"
            c = Case(cid, pn, loss, d, valued, tuple(layout), tuple(msgs), use_ell, dict(expect), dict(claims or {}))
            c.expect["nsub"] = claimed_nsub(c)
            out.append(c)

    C = RAGGED_COUNTS
    # ragged CSR (csr_fixed == 0): 4097 rows (two sub-blocks), 33, 5 rows that are all empty, no rows at all, 9
    ragged = (("h", ROW_BLOCK + 1, C), ("h", 33, C), ("h", 5, (0,)), ("h", 0, C), ("h", 9, C))
    for pn in PRECS:
        for valued in (True, False):
            for d in (1, 37, 800):
                add("ragged", pn, d, valued, ragged, messages(0, 1, 4, zero=3, empty=2), "auto",
                    _expect("csr", blocked=True), form="blocked")
    # fixed-nnz CSR (use_ell=False): m = 1, 8, 9 entries in every row
    for pn in PRECS:
        for valued in (True, False):
            for m in (1, CSR_LANES, CSR_LANES + 1):
                lay = (("h", 65, (m,)), ("h", 33, (m,)), ("h", 0, (m,)), ("h", 9, (m,)))
                add(f"fixed-m{m}", pn, 37, valued, lay, messages(0, 1, 3, zero=2), False, _expect("csr_fixed"))
    # ELL rows: beta in LDS (d small, d at the limit, d odd just below it) and not (one column past the limit)
    small = [((0, 1.0),), ((0, -0.7), (1, 1.0)), ((1, 1.0),), ((0, 0.0),)]
    for pn in PRECS:
        prec = get_precision(pn)
        lim = lds_limit(prec)
        for valued in (True, False):
            kb = KB_LDS_VALUED if valued else KB_LDS_PATTERN16
            for i, m in enumerate((1, kb - 1, kb, kb + 1, 2 * kb + 1)):
                if m < 1:
                    continue
                sizes = (33, 2, 0, 8 + i % 2)  # 43 rows (a padded pair row) or 44
                lay = tuple(("h", n, (m,)) for n in sizes)
                add(f"ell-lds-m{m}-n{sum(sizes)}", pn, 200, valued, lay, messages(0, 1, 3, zero=2), True,
                    _expect("ell", idx16=True, lds=True))
            for n in (1, 2):
                lay = (("h", n, (kb + 1,)), ("h", 0, (kb + 1,)))
                add(f"ell-lds-m{kb + 1}-n{n}", pn, 200, valued, lay, small, True, _expect("ell", idx16=True, lds=True))
            for d in (lim, lim - 1 - lim % 2):  # exactly the limit; odd, just below
                lay = tuple(("h", n, (kb + 1,)) for n in (33, 2, 0, 8))
                add(f"ell-lds-limit-m{kb + 1}", pn, d, valued, lay, messages(0, 1, 3, zero=2), True,
                    _expect("ell", idx16=True, lds=True))
            for i, m in enumerate((1, KB_ELL - 1, KB_ELL, KB_ELL + 1, 2 * KB_ELL + 1)):
                lay = tuple(("h", n, (m,)) for n in (33, 2, 0, 8 + i % 2))
                add(f"ell-m{m}", pn, lim + 1, valued, lay, messages(0, 1, 3, zero=2), True, _expect("ell", idx16=True))
        # use_ell="auto" at the limit: ELL while beta fits, CSR (fixed nnz) one column later
        lay = tuple(("h", n, (5,)) for n in (33, 2, 0, 8))
        add("auto-fits", pn, lim, pn == "fp64", lay, messages(0, 1, 3, zero=2), "auto", _expect("ell", idx16=True, lds=True))
        add("auto-past", pn, lim + 1, pn == "fp64", lay, messages(0, 1, 3, zero=2), "auto", _expect("csr_fixed"))
    # the ELL window: 65536 columns keep 16-bit offsets, 65537 need int32 columns; kEllMaxFields and one more
    for k, pn in enumerate(PRECS):
        for valued in (True, False):
            lay = (("win", 9, ELL_WINDOW), ("win", 4, ELL_WINDOW), ("h", 0, (2,)), ("win", 3, ELL_WINDOW))
            add("ell-window65536", pn, ELL_WINDOW + 6, valued, lay, messages(0, 1, 3, zero=2), True,
                _expect("ell", idx16=True))
            lay = tuple((s[0], s[1], ELL_WINDOW + 1) if s[0] == "win" else s for s in lay)
            add("ell-window65537", pn, ELL_WINDOW + 6, valued, lay, messages(0, 1, 3, zero=2), True, _expect("ell"))
        valued = bool(k)
        for m, d, lds in ((ELL_MAX_FIELDS, 1100, True), (ELL_MAX_FIELDS + 1, 1100, False),
                          (ELL_MAX_FIELDS, lds_limit(get_precision(pn)) + 1, False)):
            lay = (("h", 5, (m,)), ("h", 2, (m,)), ("h", 0, (m,)), ("h", 4, (m,)))
            add(f"ell-fields{m}", pn, d, valued, lay, messages(0, 1, 3, zero=2), True, _expect("ell", idx16=True, lds=lds))
    # the column pass: prescribed column lengths, one entry per row
    for pn in PRECS:
        for valued in (True, False):
            lay = (("cols", "edges"), ("cols", "one-left"), ("h", 0, (1,)))
            msgs = (((0, 1.0), (1, -0.7)), ((0, 0.5),), ((1, 2.0), (2, 1.0)), ((2, 1.0),), ((1, 0.0),))
            add("columns", pn, 5000, valued, lay, msgs, "auto", _expect("ell", idx16=True, lds=True, blocked=True),
                dict(nruns={1, RUN_CAP, RUN_CAP + 1, TILE}, n={1, TILE - 1, TILE}, flags={0, 1, 2, 3}, span_tiles=3),
                form="blocked")
            # a column in all 4096 rows of a sub-block: 8 tiles end to end, the next column starts on the boundary
            lay = (("full", ROW_BLOCK, 700), ("h", 33, (0, 1, 2)), ("h", 0, (1,)), ("h", 9, (0, 1, 2)))
            add("multitile", pn, 37, valued, lay, messages(0, 1, 3, zero=2), "auto", _expect("csr"),
                dict(nruns={1}, n={TILE}, flags={0, 1, 2, 3}, span_tiles=ROW_BLOCK // TILE, boundary_column=9))
    # row-blocking: 4095 / 4096 / 4097 / 8193 rows, a heavy column in each
    for pn in PRECS:
        valued = pn == "fp32"
        lay = tuple(("heavy", n, (1, 3)) for n in (ROW_BLOCK - 1, ROW_BLOCK, ROW_BLOCK + 1, 2 * ROW_BLOCK + 1)) + (("h", 0, (1,)),)
        msgs = (((0, 1.0), (1, -0.7)), ((2, 0.5), (3, 2.0)), ((3, 1.0), (4, 1.0)), ((4, 1.0),), ((1, 0.0),))
        add("rowblocks", pn, 37, valued, lay, msgs, "auto", _expect("csr", blocked=True),
            dict(flags={0, 1, 2, 3}, span_tiles=2, spans_in_subs=True), form="blocked")
    # FRC / AGC units
    rag = (0, 1, 7, 9)
    for pn in PRECS:
        valued = pn == "fp64"
        group = lambda k, a, b: [((a, 1.0), (b, 1.0))] * k  # noqa: E731
        # 4096 + 4096 = UNIT_ROWS rows and MAX_DST members: merged; a unit of 1 row with a zero-row partition
        lay = (("h", UNIT_ROWS // 2, rag), ("h", UNIT_ROWS // 2, rag), ("h", 1, (3,)), ("h", 0, rag))
        add("unit-8192x4", pn, 37, valued, lay, group(MAX_DST, 0, 1) + group(2, 2, 3), "auto",
            _expect("csr", units=True, identity=True), form="units")
        # one row more: the partition basis and the encoding
        lay = (("h", UNIT_ROWS // 2, rag), ("h", UNIT_ROWS // 2 + 1, rag), ("h", 1, (3,)), ("h", 0, rag))
        add("unit-8193", pn, 37, valued, lay, group(2, 0, 1) + group(2, 2, 3), "auto", _expect("csr", blocked=True),
            form="blocked")
        # one member more than MAX_DST: the same
        lay = (("h", 33, rag), ("h", 9, rag), ("h", 1, (3,)), ("h", 0, rag))
        add("unit-5members", pn, 37, valued, lay, group(MAX_DST + 1, 0, 1) + group(2, 2, 3), "auto", _expect("csr"))
    # the naive identity plan: ragged rows, columns empty in some partitions, an all-empty and a zero-row partition
    for pn in PRECS:
        for valued in (True, False):
            lay = (("h", 33, C), ("h", 65, C), ("h", 5, (0,)), ("h", 0, C))
            add("identity", pn, 800, valued, lay, tuple(((p, 1.0),) for p in range(4)), "auto",
                _expect("csr", identity=True), form="identity")
    return out


GRADIENT = gradient_cases()

EvalCase = collections.namedtuple("EvalCase", "id prec n R valued")


def eval_cases():
    """Every R with every precision, valued and pattern-only; n rotates over them; the grid-stride row count runs
    pattern-only with R = 1."""
    out = []
    for i, R in enumerate(EVAL_R):
        for k, pn in enumerate(PRECS):
            for valued in (True, False):
                n = EVAL_N[(i + k + valued) % len(EVAL_N)]
                out.append(EvalCase(f"{pn}-n{n}-R{R}-{'val' if valued else 'pat'}", pn, n, R, valued))
    for pn in PRECS:
        out.append(EvalCase(f"{pn}-n{EVAL_N_STRIDE}-R1-pat", pn, EVAL_N_STRIDE, 1, False))
    return out


EVAL = eval_cases()
_EVAL_BUILT = {}


def build_eval(case):
    """(precision, CSR [n, EVAL_D], y, Bt [EVAL_D, R] accumulator dtype, B fp64 view [R, EVAL_D]).  The first rows
    take EVAL_COUNTS in order (an empty row, a row longer than two waves), the rest draw from them."""
    if case.id not in _EVAL_BUILT:
        prec = get_precision(case.prec)
        rng = np.random.RandomState(zlib.crc32(("eval" + case.id).encode()) % 2 ** 31)
        if case.n <= 16:
            counts = [EVAL_COUNTS[(q + case.R) % len(EVAL_COUNTS)] for q in range(case.n)]
            mats = [nx.hostile_sparse_partition(rng, 1, EVAL_D, (c,), case.valued, prec) for c in counts]
            X = sps.vstack([m[0] for m in mats], format="csr")
            y = np.concatenate([m[1] for m in mats])
        else:
            X, y = nx.hostile_sparse_partition(rng, case.n, EVAL_D, EVAL_COUNTS, case.valued, prec)
        X = sps.csr_matrix((X.data, X.indices, X.indptr), shape=(case.n, EVAL_D))
        X.sort_indices()
        mean = X.nnz / max(1, case.n)
        B = torch.stack([nx.hostile_sparse_beta(rng, EVAL_D, prec, mean)[0][:EVAL_D] for _ in range(case.R)])
        _EVAL_BUILT[case.id] = (prec, X, y, B.t().contiguous(), B.double().numpy())
    return _EVAL_BUILT[case.id]
