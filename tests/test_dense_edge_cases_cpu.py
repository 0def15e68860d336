"""The case tables of tests/dense_edge_cases.py against the selectors they are derived from (no GPU): every
threshold of choose_cpl, WIDE_EPT and the wide kernel's half / quarter rule appears in the collected ids of
tests/test_dense_edges_gpu.py for every precision that has it, so a threshold that moves forces new cases."""
import dataclasses

import pytest

import dense_edge_cases as ec
import numerics as nx
from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.grad import WIDE_EPT, KernelChoice, choose_cpl

EXPECTED = {  # the widths the suite never ran before, per precision (ld elements)
    "fp64": [128, 256, 512, 1024, 2048, 4096, 8192],
    "fp32": [256, 512, 1024, 2048, 4096, 8192, 16384],
    "bf16": [512, 1024, 2048, 4096, 8192, 16384],
}


@pytest.mark.parametrize("prec_name", ec.PRECS)
def test_thresholds_follow_the_selectors(prec_name):
    prec = get_precision(prec_name)
    vec, ept = prec.vec, WIDE_EPT[prec.vec]
    T = ec.width_thresholds(prec)
    want = {64 * c for c in (2, 4, 8, 16, 32) if c % vec == 0} | {256 * ept // 2, 256 * ept, 512 * ept // 2, 512 * ept}
    if prec_name != "bf16":  # kernels of 8 vectors per thread have a quarter instance; bf16 has 4
        want.add(256 * ept // 4)
    assert set(T) == want and T == EXPECTED[prec_name]
    for t in T:  # each is a multiple of the vector width, and choose_cpl or the wide instance changes there
        assert t % vec == 0
        assert choose_cpl(t, vec) != choose_cpl(t + vec, vec) or t in ec.wide_thresholds(prec)
    assert choose_cpl(T[-1], vec) == 512 and choose_cpl(T[-1] + vec, vec) is None


@pytest.mark.parametrize("prec_name", ec.PRECS)
def test_every_threshold_is_in_the_collected_ids(prec_name):
    import test_dense_edges_gpu as t

    ids = {c.id for c in t.DEFAULT}
    prec = get_precision(prec_name)
    for T in ec.width_thresholds(prec):
        for d in (T - 1, T, T + 1):
            for rep in (1, 3):
                assert f"{prec_name}-d{d}-R{rep}-logistic" in ids
    assert f"{prec_name}-d1-R1-logistic" in ids
    # least squares and squared hinge at least once per (kernel kind, precision) the defaults reach
    kinds = {}
    for c in t.DEFAULT:
        if c.prec == prec_name:
            kinds.setdefault(ec.default_choice(prec, c.d, c.sizes, c.replicas).kind, set()).add(c.loss)
    assert set(kinds) >= {"fused", "multi", "wide", "twopass"}
    assert all(v == set(nx.LOSSES) for v in kinds.values()), kinds
    assert max(c.d for c in t.DEFAULT + t.FORCED) == 16385


def test_case_ids_are_unique_and_messages_have_the_required_segments():
    import test_dense_edges_gpu as t

    for table in (t.DEFAULT, t.FORCED, t.BUNDLE_ROWS):
        assert len({c.id for c in table}) == len(table)
    for rep in (1, 2, 3, 9, 16):
        msgs = ec.messages(rep)
        coefs = [c for m in msgs for _, c in m]
        assert any(len(m) == 2 for m in msgs) and min(coefs) < 0 and 0.0 in coefs
        assert any(len(m) == 2 and m[1][0] == ec.EMPTY and m[0][0] != ec.EMPTY for m in msgs)
        assert [(ec.EMPTY, 1.0)] in msgs
        reads = [p for m in msgs for p, _ in m if p != ec.EMPTY]
        assert max(reads.count(p) for p in set(reads)) == rep


def test_every_honoured_choice_field_is_set_in_some_case():
    """Every KernelChoice field launch_cpl, launch_wide or launch_fused_cpl reads (and the plan-side
    interleave / fill) takes a non-default value in at least one case of its family."""
    import test_dense_edges_gpu as t

    defaults = {f.name: f.default for f in dataclasses.fields(KernelChoice)}
    seen = set()
    for c in t.FORCED + t.BUNDLE_ROWS:
        for name, default in defaults.items():
            if name != "kind" and getattr(c.choice, name) != default:
                seen.add((c.choice.kind, name))
    want = {("fused", "rows"), ("fused", "beta_lds"), ("fused", "interleave"),
            ("multi", "replicas"), ("multi", "fold"), ("multi", "lane_epi"), ("multi", "pair"), ("multi", "bundle_rows"),
            ("staged", "replicas"), ("staged", "pair"), ("staged", "wpr"), ("staged", "bundle_rows"),
            ("wide", "replicas"), ("wide", "bundle_rows"), ("mfma", "replicas"), ("mfma", "bundle_rows")}
    assert want <= seen, want - seen
    for rep, wpr in ((2, 2), (4, 2), (8, 1)):  # the wpr values the cases set are the ones the kernel runs
        assert ec.staged_wpr(rep, wpr) == wpr
    assert ec.staged_wpr(8, 2) == 1
