"""Case tables of tests/test_fp32x64_cpu.py and tests/test_fp32x64_gpu.py: the width thresholds of the dense
selectors for the fp32-storage, fp64-arithmetic precision, built the way tests/dense_edge_cases.py builds them
but from ``wide_ept(prec)`` (its ``wide_thresholds`` reads ``WIDE_EPT[prec.vec]``, the fp32 tile of 32 elements
per thread; this precision runs fp64's 16), and the default / forced kernel choices to run at them.  A plain
module (no GPU, no tests)."""
import collections

import dense_edge_cases as ec
import numerics as nx
from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.grad import MAX_BUNDLE, KernelChoice, choose_cpl, choose_kernel, wide_ept

NAME = "fp32x64"
Case = ec.Case
CPLS = (4, 8, 16, 32)  # columns per lane that are multiples of the 4-element vector


def prec():
    return get_precision(NAME)


def cpl_of(ld):
    p = prec()
    return choose_cpl(ld, p.vec, wide_ept(p))


def wide_thresholds():
    """{ld: instance} of launch_wide_nv's rule at 16 elements per thread (4 vectors: no quarter instance)."""
    ept = wide_ept(prec())
    return {256 * ept // 2: "256-half", 256 * ept: "256-full/512-half", 512 * ept: "512-full"}


def width_thresholds():
    p = prec()
    vec, ept = p.vec, wide_ept(p)
    last = 512 * ept + 4 * vec
    T = {ld for ld in range(vec, last, vec) if choose_cpl(ld, vec, ept) != choose_cpl(ld + vec, vec, ept)}
    return sorted(T | set(wide_thresholds()))


def edge_widths():
    return sorted({1} | {T + k for T in width_thresholds() for k in (-1, 0, 1)})


def default_choice(d, sizes, replicas):
    p = prec()
    ld = p.ld(d)
    used = sorted({q for m in ec.messages(replicas) for q, _ in m})
    rows = [sizes[q] for q in used]
    return choose_kernel(p.code, ld, cpl_of(ld), replicas, sum(rows), part_rows=rows)


def default_cases():
    """Every edge width with choose_kernel's pick, distinct rows and 3 co-located replicas: logistic at every
    width; least squares and squared hinge at the first width of every kernel kind reached."""
    out, seen = [], set()
    for d in edge_widths():
        for rep in (1, 3):
            kind = default_choice(d, ec.DEFAULT_SIZES, rep).kind
            losses = [nx.LOGISTIC]
            if (kind, rep) not in seen:
                seen.add((kind, rep))
                losses += [nx.LEAST_SQUARES, nx.SQUARED_HINGE]
            for loss in losses:
                out.append(Case(f"d{d}-R{rep}-{nx.LOSS_IDS[loss]}", NAME, d, loss, ec.DEFAULT_SIZES, rep, None))
    return out


def forced_cases(bundle_rows=8):
    """Every family at its narrowest and widest legal row (d = T - 1 and T), every honoured KernelChoice field;
    the losses rotate over the widths of each form, logistic first."""
    out = []
    seen = collections.Counter()

    def add(d, rep, choice, tag):
        loss = (nx.LOGISTIC, nx.LOSSES[1 + rep % 2], nx.LOSSES[2 - rep % 2])[seen[tag] % 3]
        seen[tag] += 1
        out.append(Case(f"d{d}-{tag}-{nx.LOSS_IDS[loss]}", NAME, d, loss, ec.DEFAULT_SIZES, rep, choice))

    for c in (CPLS[0], CPLS[-1]):
        for d in (64 * c - 1, 64 * c):
            for rows in (1, 2, 4):
                for bl in (False, True):
                    add(d, 1, KernelChoice("fused", rows=rows, beta_lds=bl), f"fused-rows{rows}-bl{int(bl)}")
                add(d, 3, KernelChoice("fused", rows=rows, interleave=True), f"fused-rows{rows}-interleave")
    multi = [c for c in CPLS if c <= 16]
    for form in ("unfolded", "fold-wave", "fold-lane", "fold-pair"):
        legal = [c for c in multi if c <= 8] if form == "fold-pair" else multi
        for c in sorted({legal[0], legal[-1]}):
            for d in (64 * c - 1, 64 * c):
                for rep in (1, 2, 3):
                    ch = KernelChoice("multi", replicas=rep, bundle_rows=bundle_rows, fold=form != "unfolded",
                                      lane_epi=form == "fold-lane", pair=form == "fold-pair")
                    add(d, rep, ch, f"multi-{form}-R{rep}")
    for c in (CPLS[0], CPLS[-1]):
        for d in (64 * c - 1, 64 * c):
            for rep in (2, 4, 8, 9):
                R = min(rep, MAX_BUNDLE)
                for pair in (False, True):
                    for wpr in (0, 1, 2):
                        if wpr and ec.staged_wpr(R, wpr) != wpr:
                            continue
                        ch = KernelChoice("staged", replicas=R, bundle_rows=bundle_rows, pair=pair, wpr=wpr)
                        add(d, rep, ch, f"staged-R{rep}-pair{int(pair)}-wpr{wpr}")
    wt = wide_thresholds()
    for T in sorted(wt):
        for d in (T - 1, T):
            cpl = cpl_of(prec().ld(d))
            for rep in (1, 2, 3):
                if rep > 1 and cpl not in (32, 256):
                    continue  # replica bundles are 256-thread rows
                ch = KernelChoice("wide", replicas=rep, bundle_rows=bundle_rows if rep > 1 else 0)
                add(d, rep, ch, f"wide-{wt[T]}-R{rep}")
    add(512 * wide_ept(prec()) + 1, 3, KernelChoice("twopass"), "twopass")
    return out


def kernel_names(choice, cpl, ld, loss):
    """Substrings of the mangled names of the instantiations launch_fused_cpl / launch_wide /
    grad_dense_twopass_launch run for ``choice`` (csrc/kernels/grad_dense.hip), storage float, accumulator
    double."""
    R = choice.replicas
    if choice.kind == "twopass":
        return [f"rowdot_residualIfdLi{loss}E", "xt_r_tilesIfd"]
    if choice.kind == "wide" or cpl >= 256:
        bs, R = (cpl if cpl >= 256 else 256), (R if choice.kind == "wide" else 1)
        nv = 4
        half = bs * (nv // 2) * 4 >= ld
        if bs == 256 and R > 1 and not half:
            return [f"grad_dense_wideIfdLi{nv // 2}ELi512ELi{loss}ELi{R}ELb1E"]
        return [f"grad_dense_wideIfdLi{nv // 2 if half else nv}ELi{bs}ELi{loss}ELi{R}ELb0E"]
    if choice.kind == "multi":
        epi = 2 if choice.pair else 1 if (choice.lane_epi and choice.fold) else 0
        return [f"grad_dense_multiIfdLi{cpl}ELi{loss}ELi{R}ELb{int(choice.fold)}ELi{epi}E"]
    if choice.kind == "staged":
        return [f"grad_dense_stagedIfdLi{cpl}ELi{loss}ELb{int(choice.pair)}E"]
    assert choice.kind == "fused"
    if choice.rows == 2 and not choice.beta_lds:
        return [f"grad_dense_fused_pairIfdLi{cpl}ELi{loss}E"]
    return [f"grad_dense_fusedIfdLi{cpl}ELi{loss}ELi{choice.rows}ELb{int(choice.beta_lds)}E"]
