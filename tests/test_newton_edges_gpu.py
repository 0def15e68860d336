"""Stage-edge, hostile-input conformance tests of the Newton-CG kernels: grad_hvp (csrc/kernels/grad_hvp.hip) at every
edge of the blocked-model transport against the long-double oracles and per-column bounds of tests/newton_edge_cases.py,
newton_cg_update (csrc/kernels/newton_cg.hip) bit for bit against the documented fma chain and branch by branch against
a long-double replay.  Tables, oracles, emulators and constants: tests/newton_edge_cases.py, held to what they claim by
tests/test_newton_edge_cases_cpu.py.

Block 1 is held to K_HVP_EDGE, which follows the rule of tests/numerics.py (measured on the torch path, never on the
kernel).  A vector of an update round is held to BOUND_FACTOR x max(the twin's recorded error on it, FLOOR) of its SCALE,
the constants those of tests/test_lbfgs_cpu.py.

Measured on an MI355X (the tests print them), all 181 cases pass, the slowest (the 1024-column decode of 127 and 128
messages, nearly all of it the exact-fma emulator on the host) takes 1.6 s:
  grad_hvp, worst err / (K_HVP_EDGE bound) of block 1 over both task sizes and both message sets; fp64 / fp32 / fp32x64
    d=37    logistic 0.034 / 0.018 / 0.017   least squares 0.044 / 0.029 / 0.032   squared hinge 0.054 / 0.039 / 0.038
    d=1000  logistic 0.001 / 0.005 / 0.003   least squares 0.024 / 0.024 / 0.032   squared hinge 0.029 / 0.037 / 0.031
    logistic, fp64 / fp32:  d=1 0.025 / 0.027   d=256 0.005 / 0.003   d=257 0.010 / 0.001   d=512 0.002 / 0.004
                            d=513 0.003 / 0.015   d=1024 0.002 / 0.006   d=129 fp64 0.009   d=257 fp32x64 0.001
    so the kernel stays within 0.055 of the K_HVP_EDGE = 16 bound, 0.87 u sum ..., below the torch path's own 1.02.
  newton_cg_update, worst err / bound per vector over SCRIPT with 128 messages; fp64 / fp32 messages
    (ld, d)        x              r              dir            G0             beta
    (1, 1)       0.037 / 0.015  0.007 / 0.010  0.001 / 0.002  0.007 / 0.010  0.028 / 0.012
    (256, 256)   0.012 / 0.010  0.010 / 0.011  0.012 / 0.011  0.010 / 0.011  0.004 / 0.006
    (1024, 1024) 0.008 / 0.011  0.016 / 0.013  0.012 / 0.012  0.016 / 0.017  0.005 / 0.005
    (302, 301)   0.006 / 0.007  0.011 / 0.014  0.006 / 0.009  0.011 / 0.014  0.005 / 0.005
  every bitwise check (the fma chain in G0 and in the scratch row, -G in the state and on the wire, block 0 under five
  directions, the 2^+-8 scaling, the closed gates) holds as written: no finding.
"""
import numpy as np
import pytest
import torch

from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.hvp import HvpGradPlan
from erasurehead_amd.ops.update import newton_cg_update, newton_state
import block_edge_cases as bc
import newton_edge_cases as ne
import numerics as nx
import slab_edge_cases as sl
from numerics import LD, LEAST_SQUARES, LOGISTIC, SQUARED_HINGE
from test_lbfgs_cpu import BOUND_FACTOR, FLOOR

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
_dev_parts = {}


def inputs(d, prec_name):
    """(sizes, partitions on the device, host views, beta [ld] on the CPU, its fp64 view)."""
    sizes, cpu_parts, host, (beta, bh) = ne.inputs(d, prec_name)
    if (d, prec_name) not in _dev_parts:
        _dev_parts[(d, prec_name)] = bc.to_device(cpu_parts, DEV)
    return sizes, _dev_parts[(d, prec_name)], host, beta, bh


def launch_twice(plan, model):
    """G of plan.run and of a second launch through the native launcher into a NaN-filled buffer: bitwise equal."""
    G = plan.run(model, plan.out_buffer()[0].fill_(NAN))
    G2 = plan.out_buffer()[0].fill_(NAN)
    plan.native_launcher().launch(model, G2)
    torch.cuda.synchronize()
    assert torch.equal(G, G2) and not torch.isnan(G).any()
    return G


# ---- grad_hvp ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,loss,prec_name", ne.GRID, ids=ne.GRID_IDS)
def test_stage_edges_within_the_column_bounds(d, loss, prec_name, native, monkeypatch):
    prec = get_precision(prec_name)
    sizes, parts, _, beta, _ = inputs(d, prec_name)
    S = native._blocks_geometry(prec.ld(d) * prec.storage_bytes, 2)[0]
    assert S == bc.geometry(prec, d, 2)[0]
    model = torch.cat([beta, ne.direction(d, prec_name)[0]]).to(DEV)
    worst = 0.0
    for rows in bc.TASK_ROWS:
        bc.forced_task_rows(monkeypatch, rows)
        for kind in ne.KINDS:
            plan = HvpGradPlan(bc.MESSAGES[kind](len(sizes)), parts, prec, loss, d)
            assert plan.identity == (kind == "naive")
            bc.assert_tasks_reach_the_edges(plan, sizes, S, rows)
            G = launch_twice(plan, model)
            worst = max(worst, ne.check_messages(G, d, loss, prec_name, kind, f"tasks of {rows}"))
    print(f"grad_hvp edges d={d} {nx.LOSS_IDS[loss]} {prec_name}: worst err / (K_HVP_EDGE bound) = {worst:.4f}")


@pytest.mark.parametrize("prec_name", ["fp64", "fp32"])
@pytest.mark.parametrize("d", [37, 257, 513, 1000])
def test_block0_does_not_see_the_direction(d, prec_name, native, monkeypatch):
    """z = x . beta and q = x . v share one reduce-scatter: block 0 keeps its bits whatever v holds."""
    prec = get_precision(prec_name)
    ld = prec.ld(d)
    sizes, parts, _, beta, _ = inputs(d, prec_name)
    bc.forced_task_rows(monkeypatch, bc.ODD_TASKS)
    msgs = bc.coded_messages(len(sizes))
    plan = HvpGradPlan(msgs, parts, prec, LOGISTIC, d)
    empty = msgs.index([(len(sizes) - 1, 1.0)])
    v = ne.direction(d, prec_name)[0]
    zero, inf = torch.zeros_like(v), v.clone()
    inf[d - 1] = float("inf")
    nan = zero.clone()
    nan[:d] = NAN
    first = None
    for name, direction in (("hostile", v), ("zero", zero), ("negative zero", -zero), ("nan", nan), ("inf", inf)):
        G = plan.run(torch.cat([beta, direction]).to(DEV), plan.out_buffer()[0].fill_(NAN)).cpu().reshape(-1, 2, ld)
        first = G if first is None else first
        assert np.array_equal(bits(G[:, 0].numpy()), bits(first[:, 0].numpy())), f"block 0 moved under the {name} v"
        assert not torch.isnan(G[:, 0]).any()
        if name in ("zero", "negative zero"):
            assert bool((G[:, 1] == 0.0).all()), f"v = {name}: u must be exactly 0"
        if name == "nan":
            assert bool((G[empty] == 0.0).all()) and torch.isnan(G[0, 1, :d]).all()
    assert torch.signbit(-zero).all() and not torch.equal(first[:, 1], torch.zeros_like(first[:, 1]))


SCALED = [(d, l, p) for d, l, p in ne.GRID if l in (LEAST_SQUARES, SQUARED_HINGE)]


@pytest.mark.parametrize("d,loss,prec_name", SCALED, ids=[f"d{d}-{nx.LOSS_IDS[l]}-{p}" for d, l, p in SCALED])
def test_product_scales_exactly_with_the_direction(d, loss, prec_name, native, monkeypatch):
    """w in {0, 2} is exact, so every operation behind q is a product with, or a sum of, values that carry the power
    of two: block 1 under 2^+-8 v is bitwise 2^+-8 times block 1 under v, as long as nothing nears the ends of the
    exponent range -- a condition on the inputs, asserted on the long-double reference."""
    prec = get_precision(prec_name)
    ld = prec.ld(d)
    sizes, parts, host, beta, bh = inputs(d, prec_name)
    v, vh = ne.direction(d, prec_name)
    assert ne.scaling_is_exact(loss, host, bh, vh, prec)
    bc.forced_task_rows(monkeypatch, bc.ODD_TASKS)
    plan = HvpGradPlan(bc.coded_messages(len(sizes)), parts, prec, loss, d)
    run = lambda direction: plan.run(torch.cat([beta, direction]).to(DEV),  # noqa: E731
                                     plan.out_buffer()[0].fill_(NAN)).cpu().reshape(-1, 2, ld).clone()
    base = run(v)
    assert base[:, 1].abs().max() > 0
    for k in (8, -8):
        G = run(v * 2.0 ** k)
        assert torch.equal(G[:, 0], base[:, 0]) and torch.equal(G[:, 1], base[:, 1] * 2.0 ** k), f"2^{k} v"


@pytest.mark.parametrize("kind", ne.KINDS)
def test_closed_gate_leaves_the_messages_untouched(kind, native):
    sizes, parts, _, beta, _ = inputs(37, "fp64")
    plan = HvpGradPlan(bc.MESSAGES[kind](len(sizes)), parts, get_precision("fp64"), LOGISTIC, 37)
    L, model = plan.native_launcher(), torch.cat([beta, ne.direction(37, "fp64")[0]]).to(DEV)
    G = plan.out_buffer()[0].fill_(NAN)
    L.launch(model, G, gate=torch.ones(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert bool(torch.isnan(G).all())
    L.launch(model, G, gate=torch.zeros(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert ne.check_messages(G, 37, LOGISTIC, "fp64", kind, "open gate") <= 1.0


# ---- newton_cg_update --------------------------------------------------------------------------------------
def fresh(ld, d, beta_h, mdt):
    """(beta, state, scal, phase, hist, beta_w) on the device: a fresh state, NaN where the kernel must write."""
    return (torch.from_numpy(beta_h.copy()).to(DEV), *newton_state(ld, DEV), ne.history_row(ld, d, DEV),
            torch.full((2 * ld,), NAN, dtype=mdt, device=DEV))


def round_on_gpu(t, M, coefs, ld, d, xi=1e-9, **kw):
    newton_cg_update([torch.from_numpy(m).to(DEV) for m in M], coefs, *t[:4], ld, d, 3, ne.ETA, ne.GS, ne.L2C, xi, 0.9,
                     hist=t[4], beta_w=t[5], **kw)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in t]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32 if x.itemsize == 4 else np.uint8)


@pytest.mark.parametrize("name", list(ne.UPDATE_DTYPES))
@pytest.mark.parametrize("nmsg", ne.UPDATE_NMSG)
@pytest.mark.parametrize("ld,d", ne.UPDATE_SHAPES)
def test_decode_is_the_documented_fma_chain(ld, d, nmsg, name, native):
    assert native.MAX_MSGS == sl.MAX_MSGS == max(ne.UPDATE_NMSG)
    npdt, mdt = ne.UPDATE_DTYPES[name]
    rng = np.random.RandomState(100 * ld + nmsg)
    coefs, beta_h = sl.update_coefs(rng, nmsg), ne.hostile_model(rng, ld, d)
    rounds = [ne.hostile_messages(rng, nmsg, ld, d, npdt) for _ in range(2)]
    runs = []
    for pad in (0.0, NAN):  # NaN in the padding columns of every message changes nothing
        t, outs = fresh(ld, d, beta_h, mdt), []
        for M in rounds:
            M = M.reshape(nmsg, 2, ld).copy()
            M[:, :, d:] = pad
            outs.append(round_on_gpu(t, M.reshape(nmsg, 2 * ld), coefs, ld, d))
        runs.append(outs)
    for a, b in zip(runs[0], runs[1]):
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b)), "NaN padding columns of the messages were read"
    (b1, st1, sc1, ph1, h1, w1), (b2, st2, sc2, ph2, h2, w2) = runs[0]
    # the gradient round from the fresh state
    G = ne.emulate_affine(ne.GS, ne.emulate_decode(rounds[0], coefs, ld, d, 0), ne.L2C, beta_h[:d])
    assert np.all(sl.same_bits(st1[3, :d], G)), "G0 is not the documented fma chain"
    ref = float((G.astype(LD) ** 2).sum())
    assert np.isfinite(ref) and ref > 0 and ph1.tolist() == [1, 0, 0, 0]  # it starts CG
    assert abs(LD(sc1[0]) - LD(ref)) <= (-(-d // 256) + 10) * 2.0 ** -52 * ref and sc1[1] == sc1[0]
    assert np.all(st1[0] == 0) and np.all(sl.same_bits(st1[1, :d], -G)) and np.all(sl.same_bits(st1[2, :d], -G))
    assert np.all(sl.same_bits(w1[ld:ld + d], (-G).astype(w1.dtype))) and np.all(sl.same_bits(w1[:d], beta_h[:d].astype(w1.dtype)))
    assert np.all(sl.same_bits(b1, beta_h)) and np.all(sl.same_bits(h1[:d], beta_h[:d]))
    # the CG round that follows
    Hv = ne.emulate_affine(ne.GS, ne.emulate_decode(rounds[1], coefs, ld, d, 1), ne.L2C, -G)
    assert np.all(sl.same_bits(st2[4, :d], Hv)), "the H dir scratch row is not the documented fma chain"
    assert ph2[0] in (0, 1) and ph2[2] in range(1, 6)
    for b, st, h, w in ((b1, st1, h1, w1), (b2, st2, h2, w2)):
        assert np.all(b[d:] == 0) and np.all(h[d:] == 0) and np.all(w[d:ld] == 0) and np.all(w[ld + d:] == 0)
        assert np.all(st[:, d:] == 0)


@pytest.mark.parametrize("name", list(ne.UPDATE_DTYPES))
@pytest.mark.parametrize("ld,d", ne.SCRIPT_SHAPES)
def test_every_branch_at_the_edges(ld, d, name, native):
    rounds, seen = ne.run_script(ld, d, sl.MAX_MSGS, ne.UPDATE_DTYPES[name][1], DEV)
    assert seen == (set(range(7)) if d > 1 else {0, 2, 5, 6})
    worst = {}
    for i, mode, errs in rounds:
        for vec, e in errs.items():
            bound = BOUND_FACTOR * max(ne.TWIN_REL[vec] * 2.0 ** -53, FLOOR)
            worst[vec] = max(worst.get(vec, 0.0), e / bound)
            assert e <= bound, f"round {i} mode {mode}: {vec} {e / 2.0 ** -53:.2f} x 2^-53 of its scale"
    print(f"newton_cg_update edges ld={ld} d={d} {name}: err / bound " + " ".join(f"{k} {v:.4f}" for k, v in worst.items()))


@pytest.mark.parametrize("ld,d", [(6, 5), (1024, 1024)])
def test_zero_gradient_takes_the_gd_mode(ld, d, native):
    """rs == 0: CG cannot start; the GD step from a zero gradient leaves beta = 0 as it is (the s1 == 0 path)."""
    t = fresh(ld, d, np.zeros(2 * ld), torch.float64)
    t[3][3] = 4  # outer iterations finished so far
    b, st, sc, ph, h, w = round_on_gpu(t, np.zeros((9, 2 * ld)), sl.update_coefs(np.random.RandomState(0), 9), ld, d)
    assert ph.tolist() == [0, 0, 6, 5]
    assert not b.any() and not np.signbit(b).any() and not h.any() and not w.any() and not st.any() and not sc.any()


@pytest.mark.parametrize("ld,d", [(6, 5), (302, 301), (1024, 1024)])
def test_foreign_state_is_a_gradient_round(ld, d, native):
    """phase[0] = 2 with NaN in the scratch row and in the padding columns of the state: bitwise the round from a
    fresh state in the columns below d, exact zeros in the padding of what the round writes."""
    rng = np.random.RandomState(ld)
    coefs, beta_h = sl.update_coefs(rng, 9), ne.hostile_model(rng, ld, d)
    M = ne.hostile_messages(rng, 9, ld, d, np.float64)
    want = round_on_gpu(fresh(ld, d, beta_h, torch.float32), M, coefs, ld, d)
    t = fresh(ld, d, beta_h, torch.float32)
    t[1][4] = NAN
    t[1][:, d:] = NAN
    t[3][:] = torch.tensor([2, 7, 3, 0], dtype=torch.int32)  # neither 0 nor 1; a stale inner count and mode
    b, st, sc, ph, h, w = round_on_gpu(t, M, coefs, ld, d)
    assert ph.tolist() == want[3].tolist() == [1, 0, 0, 0]
    assert np.array_equal(bits(st[:4, :d]), bits(want[1][:4, :d])) and np.array_equal(bits(sc), bits(want[2]))
    for x, y in ((b, want[0]), (h, want[4]), (w, want[5])):
        assert np.array_equal(bits(x), bits(y))
    assert np.all(b[d:] == 0) and np.all(h[d:] == 0) and np.all(w[d:ld] == 0) and np.all(w[ld + d:] == 0)


@pytest.mark.parametrize("phase0", [0, 1])
def test_closed_gate_writes_nothing(phase0, native):
    ld, d = 302, 301
    rng = np.random.RandomState(5)
    coefs, beta_h = sl.update_coefs(rng, 9), ne.hostile_model(rng, ld, d)
    M = ne.hostile_messages(rng, 9, ld, d, np.float64)
    t = list(fresh(ld, d, beta_h, torch.float32))
    t[1].copy_(torch.from_numpy(rng.standard_normal((5, ld))))
    t[2].copy_(torch.tensor([1.5, 2.5], dtype=torch.float64))
    t[3].copy_(torch.tensor([phase0, 1, 1, 3], dtype=torch.int32))
    t[4].fill_(NAN)
    before = [x.cpu().numpy().copy() for x in t]
    after = round_on_gpu(t, M, coefs, ld, d, gate=torch.ones(1, dtype=torch.int32, device=DEV))
    for x, y in zip(before, after):
        assert np.array_equal(bits(x), bits(y))
    assert np.isnan(after[4]).all() and np.isnan(after[5]).all()
    after = round_on_gpu(t, M, coefs, ld, d, gate=torch.zeros(1, dtype=torch.int32, device=DEV))
    assert after[3][2] != 1 or after[3].tolist() != before[3].tolist()  # the open gate runs the round
    assert not np.isnan(after[4][:d]).any()
