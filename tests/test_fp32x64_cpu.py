"""The fp32-storage, fp64-arithmetic precision ``fp32x64`` without a GPU: the precision entry, the plan selectors
at every width edge, the built instantiations, the CPU engine against the fp64 NumPy replay on the rounded rows,
and the plumbing around it (sparse sources, softmax rejection, the CLI flag, the rounding report)."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import dense_edge_cases as ec
import fp32x64_cases as fc
import numerics as nx
from erasurehead_amd.codes import make_scheme, scheme_key
from erasurehead_amd.config import RunConfig
from erasurehead_amd.data.source import ArraySource
from erasurehead_amd.engine import Trainer
from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.grad import WIDE_EPT, KernelChoice, choose_cpl, choose_kernel, wide_ept, wide_slots_per_cu
from erasurehead_amd.parallel.dist import DistEnv
from oracle import replay
from test_engine_cpu import make
from test_isa_checks import READELF, _code_objects, _kernel_regs

# naive, cyclic s = 2, FRC s = 1, AGC with uneven groups: (is_coded, partitions, coded_ver, n_procs, s, num_collect)
ENGINE_CASES = {"naive": (0, 0, 0, 5, 0, 0), "cyclic-s2": (1, 0, 0, 7, 2, 0), "frc-s1": (1, 0, 1, 7, 1, 0),
                "agc-uneven": (1, 0, 3, 9, 2, 6)}


# ---- the precision entry ---------------------------------------------------------------------------
def test_precision_entry():
    prec = get_precision("fp32x64")
    assert (prec.name, prec.code, prec.storage, prec.acc, prec.vec) == ("fp32x64", 3, torch.float32, torch.float64, 4)
    assert prec.storage_bytes == 4
    assert [prec.ld(d) for d in (1, 4, 5, 1000, 1001)] == [4, 4, 8, 1000, 1004]
    assert nx.acc_eps(prec) == 2.0 ** -52
    # codes 0-2 are what they were
    assert [(p.name, p.code, p.vec) for p in map(get_precision, ("fp64", "fp32", "bf16"))] == \
        [("fp64", 0, 2), ("fp32", 1, 4), ("bf16", 2, 8)]


# ---- selectors -------------------------------------------------------------------------------------
def test_wide_tile_follows_the_accumulator():
    assert wide_ept(get_precision("fp32x64")) == 16
    for name in ("fp64", "fp32", "bf16"):  # the selector agrees with the table for what the table describes
        p = get_precision(name)
        assert wide_ept(p) == WIDE_EPT[p.vec]
    assert WIDE_EPT == {2: 16, 4: 32, 8: 32}
    for ld in (4, 2048, 4096, 8192, 8196, 16384):  # existing signature, unchanged answers
        assert choose_cpl(ld, 4) == choose_cpl(ld, 4, 32)
    assert wide_slots_per_cu(3, 2048, 3) == 2 and wide_slots_per_cu(3, 2052, 3) == 1 and wide_slots_per_cu(3, 2052, 1) == 2


def test_thresholds():
    assert fc.width_thresholds() == [256, 512, 1024, 2048, 4096, 8192]
    assert fc.cpl_of(8192) == 512 and fc.cpl_of(8196) is None
    assert [fc.cpl_of(ld) for ld in (4, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096, 4100)] == \
        [4, 4, 8, 8, 16, 16, 32, 32, 256, 256, 512]


def _launcher_accepts(choice, cpl, ld, replicas):
    """The checks of make_dense / launch_fused_cpl / launch_cpl / launch_wide, on the host."""
    if choice.kind == "twopass":
        return cpl is None
    if cpl is None:
        return False
    if cpl <= 32 and not (cpl % 4 == 0 and cpl * 64 >= ld):
        return False
    if cpl > 32 and not (cpl in (256, 512) and cpl * 16 >= ld):
        return False
    if choice.kind == "mfma":
        return False  # bf16 only
    if choice.kind == "wide" or cpl >= 256:
        R = choice.replicas if choice.kind == "wide" else 1
        bs = cpl if cpl >= 256 else 256
        return 1 <= R <= 3 and (bs == 256 or R == 1) and bs * 16 >= ld
    if choice.kind == "multi":
        return cpl <= 16 and 1 <= choice.replicas <= 3 and (not choice.pair or (cpl <= 8 and choice.fold))
    if choice.kind == "staged":
        return 1 <= choice.replicas <= 8
    return choice.kind == "fused" and choice.rows in (1, 2, 4)


# (kind, replicas, fold, lane_epi, pair) of choose_kernel's pick at every edge width, distinct rows / 3 replicas
TABLE = {
    1: (("multi", 1, 1, 0, 1), ("multi", 3, 1, 0, 1)),
    255: (("multi", 1, 1, 0, 1), ("multi", 3, 1, 0, 1)),
    256: (("multi", 1, 1, 0, 1), ("multi", 3, 1, 0, 1)),
    257: (("fused", 1, 0, 0, 0), ("multi", 3, 1, 0, 1)),
    511: (("fused", 1, 0, 0, 0), ("multi", 3, 1, 0, 1)),
    512: (("fused", 1, 0, 0, 0), ("multi", 3, 1, 0, 1)),
    513: (("multi", 1, 1, 0, 0), ("multi", 3, 1, 1, 0)),
    1023: (("multi", 1, 1, 0, 0), ("multi", 3, 1, 1, 0)),
    1024: (("multi", 1, 1, 0, 0), ("multi", 3, 1, 1, 0)),
    1025: (("fused", 1, 0, 0, 0), ("wide", 3, 0, 0, 0)),
    2047: (("fused", 1, 0, 0, 0), ("wide", 3, 0, 0, 0)),
    2048: (("fused", 1, 0, 0, 0), ("wide", 3, 0, 0, 0)),
    2049: (("wide", 1, 0, 0, 0), ("wide", 3, 0, 0, 0)),
    4095: (("wide", 1, 0, 0, 0), ("wide", 3, 0, 0, 0)),
    4096: (("wide", 1, 0, 0, 0), ("wide", 3, 0, 0, 0)),
    4097: (("wide", 1, 0, 0, 0), ("wide", 1, 0, 0, 0)),
    8191: (("wide", 1, 0, 0, 0), ("wide", 1, 0, 0, 0)),
    8192: (("wide", 1, 0, 0, 0), ("wide", 1, 0, 0, 0)),
    8193: (("twopass", 1, 0, 0, 0), ("twopass", 1, 0, 0, 0)),
}


def test_default_choice_table():
    prec = fc.prec()
    assert fc.edge_widths() == sorted(TABLE)
    for d, want in TABLE.items():
        ld = prec.ld(d)
        for rep, w in zip((1, 3), want):
            c = fc.default_choice(d, ec.DEFAULT_SIZES, rep)
            assert (c.kind, c.replicas, int(c.fold), int(c.lane_epi), int(c.pair)) == w, (d, rep, c)
            assert _launcher_accepts(c, fc.cpl_of(ld), ld, rep), (d, rep, c)
            if c.kind == "fused":  # the interleaved pair kernel (fp64's rule), one row in flight at 32 columns per
                assert c.rows == (1 if fc.cpl_of(ld) == 32 else 2) and not c.beta_lds  # lane; never the spilling 4 rows
    # more replicas than a one-wave bundle holds, and the headline shapes: the fp64 residency rules, but for long
    # streams of replica bundles, which fill two workgroups per CU (half the rows per bundle)
    rows_of = {}
    for ld, rep, rows in ((1000, 4, 10 ** 6), (2048, 8, 10 ** 5), (1000, 3, 10 ** 6), (1000, 2, 10 ** 6), (1000, 1, 10 ** 6),
                          (1000, 3, 125000), (1000, 2, 125000), (1000, 1, 125000)):
        c3 = choose_kernel(3, ld, fc.cpl_of(ld), rep, rows)
        c0 = choose_kernel(0, ld, fc.cpl_of(ld), rep, rows)  # fp64 rules at the same columns per lane
        assert dataclasses.replace(c3, bundle_rows=0) == dataclasses.replace(c0, bundle_rows=0), (ld, rep, c3, c0)
        assert _launcher_accepts(c3, fc.cpl_of(ld), ld, rep), (ld, rep, c3)
        rows_of[ld, rep, rows] = (c3.bundle_rows, c0.bundle_rows)
    assert rows_of == {(1000, 4, 10 ** 6): (512, 512), (2048, 8, 10 ** 5): (256, 256),
                       (1000, 3, 10 ** 6): (512, 1024), (1000, 2, 10 ** 6): (512, 1024), (1000, 1, 10 ** 6): (1024, 1024),
                       (1000, 3, 125000): (128, 128), (1000, 2, 125000): (128, 128), (1000, 1, 125000): (128, 128)}
    assert choose_kernel(3, 1000, 16, 3, 10 ** 6).kind != "mfma"


def test_forced_cases_are_legal_and_cover_every_family():
    prec = fc.prec()
    cases = fc.forced_cases()
    assert len({c.id for c in cases}) == len(cases)
    for c in cases:
        ld = prec.ld(c.d)
        assert _launcher_accepts(c.choice, fc.cpl_of(ld), ld, c.replicas), c.id
    assert {c.choice.kind for c in cases} == {"fused", "multi", "staged", "wide", "twopass"}
    for kind, lo, hi in (("fused", 255, 2048), ("multi", 255, 1024), ("staged", 255, 2048), ("wide", 2047, 8192)):
        ds = [c.d for c in cases if c.choice.kind == kind]
        assert (min(ds), max(ds)) == (lo, hi), kind


# ---- the built library -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def regs(tmp_path_factory):
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not installed")
    out = {}
    for co in _code_objects(tmp_path_factory.mktemp("co")):
        out.update(_kernel_regs(co))
    return out


def test_instantiations_exist(regs):
    for R in (1, 2, 3):
        assert any(f"grad_dense_multiIfdLi16ELi0ELi{R}E" in n for n in regs), R
    assert any("grad_dense_stagedIfd" in n for n in regs)
    assert any("grad_dense_wideIfd" in n for n in regs)
    assert any("eval_gemm_loss_v2Ifd" in n for n in regs) and any("eval_gemm_lossIfd" in n for n in regs)
    # 16 elements per thread: no instance of 8 vectors of fp32 rows with fp64 accumulators (it spills)
    assert not any("grad_dense_wideIfdLi8E" in n for n in regs)


def test_no_default_choice_names_a_spilling_instantiation(regs):
    prec = fc.prec()
    shapes = [(d, rep, sum(ec.DEFAULT_SIZES)) for d in fc.edge_widths() for rep in (1, 3)]
    shapes += [(d, rep, rows) for d in (256, 1000, 2048, 4096) for rep in (1, 2, 3, 4, 8) for rows in (10 ** 5, 10 ** 6)]
    checked = 0
    for d, rep, rows in shapes:
        ld = prec.ld(d)
        cpl = fc.cpl_of(ld)
        c = choose_kernel(prec.code, ld, cpl, rep, rows)
        for loss in nx.LOSSES:
            for key in fc.kernel_names(c, cpl, ld, loss):
                hit = {n: r for n, r in regs.items() if key in n}
                assert len(hit) == 1, (key, sorted(hit))
                (v, spill), = hit.values()
                assert spill == 0, f"d = {d}, R = {rep}: {c.label()} runs {key}, which spills {spill} VGPRs"
                if c.kind == "multi":
                    assert v <= 256, (key, v)
                checked += 1
    assert checked >= 3 * len(shapes)


# ---- the CPU engine --------------------------------------------------------------------------------
def _rounded(parts):
    return [(X.astype(np.float32).astype(np.float64), y) for X, y in parts]


@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", sorted(ENGINE_CASES))
def test_engine_matches_the_fp64_replay_on_the_rounded_rows(name, rule):
    cfg, src, sch, parts = make(ENGINE_CASES[name], rule, precision="fp32x64")
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    assert tr.prec.name == "fp32x64"
    for X, y in tr._parts.values():
        assert X.dtype == torch.float32 and y.dtype == torch.float64 and X.shape[1] == 20
    res = tr.run()
    ref = replay(sch, _rounded(parts), tr.beta0, res.arrivals, rule, cfg.alpha_value, cfg.n_rows, cfg.eta())
    np.testing.assert_allclose(res.betaset, ref, rtol=1e-9, atol=1e-11)
    # the rounding is what separates it from the fp64 trajectory: the unrounded replay is visibly elsewhere
    far = replay(sch, parts, tr.beta0, res.arrivals, rule, cfg.alpha_value, cfg.n_rows, cfg.eta())
    assert np.max(np.abs(res.betaset - far)) > 1e-11
    rep = tr.rank_report()
    assert 0.0 < rep["storage_max_rel_rounding"] <= 2.0 ** -24


def exact_source(case, rows=30, d=17, seed=0):
    """The partitions of test_engine_cpu.make with entries that fp32 holds exactly: multiples of 2^-8, |x| < 4."""
    is_coded, P, ver, n_procs, s, k = case
    W = n_procs - 1
    key = scheme_key(is_coded, P, ver)
    uneven = key in ("approx", "replication") and W % (s + 1) != 0
    n_parts = make_scheme(key, W, s, rows * W, k, P, allow_uneven=uneven).n_partition_files
    rng = np.random.RandomState(seed)
    parts = [(rng.randint(-1023, 1024, (rows, d)) / 256.0, rng.choice([-1.0, 1.0], rows)) for _ in range(n_parts)]
    test = (rng.randint(-1023, 1024, (2 * rows, d)) / 256.0, rng.choice([-1.0, 1.0], 2 * rows))
    return ArraySource(parts, test)


@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", sorted(ENGINE_CASES))
def test_engine_equals_fp64_on_fp32_exact_data(name, rule):
    out = {}
    for precision in ("fp64", "fp32x64"):
        cfg, _, sch, _ = make(ENGINE_CASES[name], rule, precision=precision)
        tr = Trainer(cfg, DistEnv(), exact_source(ENGINE_CASES[name]), scheme=sch)
        out[precision] = tr.run().betaset
        assert tr.rank_report()["storage_max_rel_rounding"] == 0.0
    assert np.array_equal(out["fp32x64"], out["fp64"])


def test_sparse_source_equals_the_fp64_run():
    import scipy.sparse as sps

    case = ENGINE_CASES["agc-uneven"]
    out = {}
    for precision in ("fp64", "fp32x64"):
        cfg, src, sch, parts = make(case, "AGD", precision=precision)
        rng = np.random.RandomState(5)
        sp = [(sps.csr_matrix(X * (rng.uniform(size=X.shape) < 0.3)), y) for X, y in parts]
        Xt, yt = src._test
        tr = Trainer(cfg, DistEnv(), ArraySource(sp, (sps.csr_matrix(Xt), yt), sparse=True), scheme=sch)
        out[precision] = tr.run().betaset
        assert tr.rank_report()["storage_max_rel_rounding"] is None
    assert np.array_equal(out["fp32x64"], out["fp64"])


def test_synthetic_rows_are_drawn_in_storage_precision():
    cfg = RunConfig(5, 400, 9, "/tmp/eh_x64/", 0, "synthetic", 0, 0, 0, 0, 0, 0, "GD", num_itrs=2, data="synthetic",
                    seed=0, verbose=False, precision="fp32x64")
    tr = Trainer(cfg, DistEnv())
    for X, y in tr._parts.values():
        assert X.dtype == torch.float32 and y.dtype == torch.float64
    assert tr.rank_report()["storage_max_rel_rounding"] is None
    assert np.all(np.isfinite(tr.run().betaset))


# ---- plumbing --------------------------------------------------------------------------------------
def test_softmax_is_rejected_by_name():
    from erasurehead_amd.ops.softmax import SoftmaxGradPlan

    with pytest.raises(ValueError, match="fp32x64"):
        SoftmaxGradPlan.check_supported(get_precision("fp32x64"), 3)
    SoftmaxGradPlan.check_supported(get_precision("fp64"), 3)
    SoftmaxGradPlan.check_supported(get_precision("fp32"), 3)


def test_cli_parses_the_flag():
    from erasurehead_amd import cli

    parser = cli.build_parser()
    flags = {a.dest: a for a in parser._actions}
    assert "fp32x64" in flags["precision"].choices and flags["precision"].default == "fp64"


def test_eval_takes_the_accumulator_from_the_precision():
    from erasurehead_amd.ops.eval import loss_sums, predictions, predictions_and_loss

    prec = get_precision("fp32x64")
    rng = np.random.RandomState(3)
    X, y, Xh = nx.hostile_partition(rng, 65, 33, prec)
    B = torch.stack([nx.hostile_beta(rng, 33, prec)[0] for _ in range(3)])
    P = predictions(X, B, 33, acc=prec)
    assert P.dtype == torch.float64 and predictions(X, B, 33).dtype == torch.float32  # the default rule stays
    for loss in nx.LOSSES:
        Pref, dP, sref, ds = nx.oracle_eval(loss, Xh, y.numpy(), B[:, :33].numpy(), prec)
        assert np.all(np.abs(P.numpy().astype(nx.LD) - Pref) <= dP)
        P2, s2 = predictions_and_loss(X, y, B, 33, loss, acc=prec)
        s1, n = loss_sums([(X, y)], B, 33, loss, acc=prec)
        assert n == 65 and np.all(np.abs(s1.astype(nx.LD) - sref) <= ds) and np.all(np.abs(s2.astype(nx.LD) - sref) <= ds)
