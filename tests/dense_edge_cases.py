"""Case tables of tests/test_dense_edges_gpu.py: the width thresholds of the dense-gradient selectors, read
off the selectors themselves, and the default / forced kernel choices to run at them.  A plain module (no
GPU, no tests): tests/test_dense_edge_cases_cpu.py checks the tables against choose_cpl and WIDE_EPT, so a
threshold that moves forces new cases."""
import collections

from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.grad import MAX_BUNDLE, WIDE_EPT, KernelChoice, choose_cpl, choose_kernel

import numerics as nx

PRECS = ("fp64", "fp32", "bf16")
DEFAULT_SIZES = (1, 15, 16, 17, 33, 0)  # the main-loop / tail boundary of 1, 2, 4 rows x 4 waves; one row; empty
EMPTY = 5  # the empty partition
Case = collections.namedtuple("Case", "id prec d loss sizes replicas choice")


def wide_thresholds(prec):
    """{ld: instance} of launch_wide_nv's rule: a 256- or 512-thread row of EPT elements per thread, the
    half-width instance, and for kernels of 8 or more vectors per thread (not bf16) the quarter."""
    ept = WIDE_EPT[prec.vec]
    out = {256 * ept // 2: "256-half", 256 * ept: "256-full", 512 * ept // 2: "512-half", 512 * ept: "512-full"}
    if ept // prec.vec >= 8:
        out[256 * ept // 4] = "256-quarter"
    return out


def width_thresholds(prec):
    """Sorted ld thresholds: where choose_cpl changes its answer (scanned, not assumed), and where
    launch_wide_nv changes the instance."""
    vec = prec.vec
    last = 512 * WIDE_EPT[vec] + 4 * vec
    T = {ld for ld in range(vec, last, vec) if choose_cpl(ld, vec) != choose_cpl(ld + vec, vec)}
    return sorted(T | set(wide_thresholds(prec)))


def edge_widths(prec):
    """d = 1, and T - 1 (the last vector partly padding), T, T + 1 (the next instance, one live column in
    its last vector) for every threshold."""
    return sorted({1} | {T + k for T in width_thresholds(prec) for k in (-1, 0, 1)})


def messages(replicas, main=4, second=1):
    """Messages over six partitions (EMPTY has no rows): two segments, a negative coefficient, a coefficient
    of exactly 0.0, the empty partition next to a non-empty one and a message that reads only the empty
    one.  Partition ``main`` is read by ``replicas`` messages, ``second`` by min(replicas, 2)."""
    msgs = [[(main, 1.0), (second, -0.7)]]
    for q in range(1, replicas):
        msgs.append([(main, 0.5 + 0.25 * q)] + ([(second, 2.0)] if q == 1 else []))
    others = [p for p in range(5) if p not in (main, second)]
    msgs.append([(others[0], 0.0), (others[1], 2.5)])
    msgs.append([(others[2], 1.5), (EMPTY, 1.0)])
    msgs.append([(EMPTY, 1.0)])
    return msgs


def default_choice(prec, d, sizes, replicas):
    """choose_kernel's pick for the plan of messages(replicas) over partitions of ``sizes`` rows."""
    ld = prec.ld(d)
    used = sorted({p for m in messages(replicas) for p, _ in m})
    rows = [sizes[p] for p in used]
    return choose_kernel(prec.code, ld, choose_cpl(ld, prec.vec), replicas, sum(rows), part_rows=rows)


def default_cases():
    """Every edge width with choose_kernel's pick, distinct rows and 3 co-located replicas: logistic at every
    width; least squares and squared hinge at the first width of every (kernel kind, precision) reached."""
    out, seen = [], set()
    for pn in PRECS:
        prec = get_precision(pn)
        for d in edge_widths(prec):
            for rep in (1, 3):
                kind = default_choice(prec, d, DEFAULT_SIZES, rep).kind
                losses = [nx.LOGISTIC]
                if (pn, kind, rep) not in seen:
                    seen.add((pn, kind, rep))
                    losses += [nx.LEAST_SQUARES, nx.SQUARED_HINGE]
                for loss in losses:
                    out.append(Case(f"{pn}-d{d}-R{rep}-{nx.LOSS_IDS[loss]}", pn, d, loss, DEFAULT_SIZES, rep, None))
    return out


def _cpls(prec):
    return [c for c in (2, 4, 8, 16, 32) if c % prec.vec == 0]


def staged_wpr(replicas, want):
    """Waves per replica grad_dense.hip staged_geometry runs for KernelChoice.wpr = want."""
    return want if 1 <= want <= 4 and replicas * want <= 8 else max(1, 4 // replicas)


def forced_cases(bundle_rows=8):
    """The honoured KernelChoice fields at the narrowest and widest legal row of each family, at d = T - 1
    and T; the losses rotate over the widths of each form, logistic (the hardware sigmoid forms) first: a form
    that runs at four widths meets all three in every precision, one that runs at two meets logistic and,
    across precisions and replica counts, both others."""
    out = []
    seen = collections.Counter()

    def add(pn, d, rep, choice, tag, sizes=DEFAULT_SIZES):
        other = (PRECS.index(pn) + rep) % 2
        loss = (nx.LOGISTIC, nx.LOSSES[1 + other], nx.LOSSES[2 - other])[seen[pn, tag] % 3]
        seen[pn, tag] += 1
        out.append(Case(f"{pn}-d{d}-{tag}-{nx.LOSS_IDS[loss]}", pn, d, loss, sizes, rep, choice))

    for pn in PRECS:
        prec = get_precision(pn)
        cpls = _cpls(prec)
        # fused: rows in flight x beta in registers / LDS, and the replica-interleaved dispatch
        for c in (cpls[0], cpls[-1]):
            for d in (64 * c - 1, 64 * c):
                for rows in (1, 2, 4):
                    for bl in (False, True):
                        add(pn, d, 1, KernelChoice("fused", rows=rows, beta_lds=bl), f"fused-rows{rows}-bl{int(bl)}")
                    add(pn, d, 3, KernelChoice("fused", rows=rows, interleave=True), f"fused-rows{rows}-interleave")
        # multi: one-wave bundles, every epilogue
        multi = [c for c in cpls if c <= 16]
        for form in ("unfolded", "fold-wave", "fold-lane", "fold-pair"):
            legal = [c for c in multi if c <= 8] if form == "fold-pair" else multi
            for c in sorted({legal[0], legal[-1]}):
                for d in (64 * c - 1, 64 * c):
                    for rep in (1, 2, 3):
                        ch = KernelChoice("multi", replicas=rep, bundle_rows=bundle_rows, fold=form != "unfolded",
                                          lane_epi=form == "fold-lane", pair=form == "fold-pair")
                        add(pn, d, rep, ch, f"multi-{form}-R{rep}")
        # staged: LDS ring, a wave (or wpr waves) per replica; 9 replicas split into 8 + 1 padded
        for c in (cpls[0], cpls[-1]):
            for d in (64 * c - 1, 64 * c):
                for rep in (2, 4, 8, 9):
                    R = min(rep, MAX_BUNDLE)
                    for pair in (False, True):
                        for wpr in (0, 1, 2):
                            if wpr and staged_wpr(R, wpr) != wpr:
                                continue  # staged_geometry would fall back to its default
                            ch = KernelChoice("staged", replicas=R, bundle_rows=bundle_rows, pair=pair, wpr=wpr)
                            add(pn, d, rep, ch, f"staged-R{rep}-pair{int(pair)}-wpr{wpr}")
        # wide: a workgroup per row; quarter / half / full 256-thread instances, rows of 32 columns per lane,
        # the 512-thread replica instance (R > 1, full-width rows), and 512-thread rows
        wt = wide_thresholds(prec)
        for T in sorted(set(wt) | {64 * 32}):
            for d in (T - 1, T):
                cpl = choose_cpl(prec.ld(d), prec.vec)
                for rep in (1, 2, 3):
                    if rep > 1 and cpl not in (32, 256):
                        continue  # replica bundles are 256-thread rows
                    ch = KernelChoice("wide", replicas=rep, bundle_rows=bundle_rows if rep > 1 else 0)
                    add(pn, d, rep, ch, f"wide-{wt.get(T, 'cpl32')}-R{rep}")
        # two-pass: the first width past the one-pass kernels
        add(pn, 512 * WIDE_EPT[prec.vec] + 1, 3, KernelChoice("twopass"), "twopass")
    # mfma: bf16 replica bundles on the matrix cores (16 replicas: two bundles of 8)
    for d in (8, 1016, 1024):
        for rep in (1, 3, 4, 5, 16):
            ch = KernelChoice("mfma", replicas=min(rep, MAX_BUNDLE), bundle_rows=bundle_rows)
            add("bf16", d, rep, ch, f"mfma-R{rep}")
    return out


def bundle_row_cases(b=8):
    """Bundle kinds at partitions of [b - 1, b, b + 1, 1, 4b + 1, 0] rows: partial bundles, pad bundles at a
    partition's end inside a folded workgroup, a bundle ending on either register buffer."""
    sizes = (b - 1, b, b + 1, 1, 4 * b + 1, 0)
    out = []
    n = collections.Counter()

    def add(pn, d, rep, choice, tag):
        loss = nx.LOSSES[(n[pn] + PRECS.index(pn)) % 3]  # each form meets a different loss in each precision
        n[pn] += 1
        out.append(Case(f"{pn}-d{d}-{tag}-b{b}-{nx.LOSS_IDS[loss]}", pn, d, loss, sizes, rep, choice))

    for pn in PRECS:
        prec = get_precision(pn)
        d = 1000 if pn != "fp64" else 999
        for rep in (1, 2, 3):
            for form in ("unfolded", "fold-wave", "fold-lane"):
                add(pn, d, rep, KernelChoice("multi", replicas=rep, bundle_rows=b, fold=form != "unfolded",
                                             lane_epi=form == "fold-lane"), f"multi-{form}-R{rep}")
            add(pn, 500, rep, KernelChoice("multi", replicas=rep, bundle_rows=b, fold=True, pair=True),
                f"multi-fold-pair-R{rep}")
            if rep > 1:
                add(pn, 3000, rep, KernelChoice("wide", replicas=rep, bundle_rows=b), f"wide-R{rep}")
        for rep in (2, 4, 9):
            for pair in (False, True):
                add(pn, d, rep, KernelChoice("staged", replicas=min(rep, MAX_BUNDLE), bundle_rows=b, pair=pair),
                    f"staged-R{rep}-pair{int(pair)}")
    for rep in (1, 3, 5):
        add("bf16", 1000, rep, KernelChoice("mfma", replicas=rep, bundle_rows=b), f"mfma-R{rep}")
    return out
