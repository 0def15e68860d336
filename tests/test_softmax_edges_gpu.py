"""The softmax gradient kernel (csrc/kernels/grad_softmax.hip) at the edges of its geometry, on hostile inputs, held to
the long-double oracle and the per-class, per-column bound of tests/numerics.py (GPU only).

Cases, partitions, task sizes and messages are tests/block_edge_cases.py's (tests/test_block_edge_cases_cpu.py checks
that they reach what they claim): every class count's wave layout, both models (a common logit of hundreds that only
the max subtraction removes; rows whose top probability is exactly 1), every width at which columns per lane or stage
rows change, stages of every ragged row count around a row per wave, eight rows per wave (the second softmax pass) and
the full stage, tasks of three and four stages (ring reuse) and tasks that start at odd rows.  Every case checks

  * every class block of every message against oracle_softmax_message, column by column,
  * exact zeros in every padding column, over an output buffer filled with NaN,
  * the native launcher bitwise equal to plan.run, and a second run bitwise equal to the first.
"""
import numpy as np
import pytest
import torch

import block_edge_cases as bc
import numerics as nx
from erasurehead_amd.ops import SoftmaxGradPlan, get_precision

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = bc.softmax_cases()
_dev, _shares = {}, {}


def device_parts(d, prec_name, C):
    """The partitions of block_edge_cases.softmax_inputs on the device: copied once, never changed."""
    key = (d, prec_name, C)
    if key not in _dev:
        _dev[key] = bc.to_device(bc.softmax_inputs(d, prec_name, C)[1], DEV)
    return _dev[key]


def build(case, kind, rows, monkeypatch, parts=None):
    """The case's plan over MESSAGES[kind] with tasks of ``rows`` rows, its task table checked for what the task size
    is for."""
    prec = get_precision(case.prec)
    sizes = bc.softmax_inputs(case.d, case.prec, case.C)[0]
    bc.forced_task_rows(monkeypatch, rows)
    plan = SoftmaxGradPlan(bc.MESSAGES[kind](len(sizes)), parts or device_parts(case.d, case.prec, case.C), prec,
                           case.C, case.d)
    assert plan.identity == (kind == "naive") and plan.ld == case.C * prec.ld(case.d)
    bc.assert_tasks_reach_the_edges(plan, sizes, bc.geometry(prec, case.d, case.C)[0], rows)
    return plan


def run(plan, beta):
    G = plan.out_buffer()[0].fill_(float("nan"))  # every element, padding included, must be overwritten
    plan.run(beta, G)
    return G


# ---- 1. the kernel against the long-double oracle
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_kernel_within_the_column_bounds(case, native, monkeypatch):
    beta = bc.softmax_inputs(case.d, case.prec, case.C)[3][case.model][0].to(DEV)
    for rows in bc.TASK_ROWS:
        for kind in ("naive", "coded"):
            plan = build(case, kind, rows, monkeypatch)
            G = run(plan, beta)
            G2 = plan.out_buffer()[0].fill_(float("nan"))
            plan.native_launcher().launch(beta, G2)
            G3 = run(plan, beta)
            torch.cuda.synchronize()
            share = bc.check_softmax(G, case, kind, f"{case.id} tasks of {rows}")
            assert torch.equal(G, G2)  # the native launcher: bitwise plan.run
            assert torch.equal(G, G3)  # a second run: bitwise the first
            _shares[(case.id, kind, rows)] = share
    worst = max((v, k) for k, v in _shares.items() if k[0] == case.id)
    print(f"largest share of the bound: {worst[0]:.4f} at {worst[1]}")  # the figure in tests/numerics.py's comment


# ---- 2. stale logit slots
@pytest.mark.parametrize("prec_name", bc.SOFTMAX_PRECS)
@pytest.mark.parametrize("d", bc.CROSS_WIDTHS)
@pytest.mark.parametrize("C", [3, 5])
def test_dead_logit_slots_are_never_read(C, d, prec_name, native, monkeypatch):
    """A stage's logit rows have 8 slots of which C are live; the max and the denominator go over the row's own
    classes.  The C-class plan runs, then an 8-class plan over the same rows whose classes 5..7 have logits of
    hundreds to thousands (so whatever LDS a later workgroup inherits may hold large values in slots C..7), then the
    C-class plan again: bitwise its first result, which is within the bounds.  Which CU a workgroup lands on and what
    its LDS held before cannot be arranged from Python, so the reference is this module's own earlier run, not a
    fresh process; nothing is asserted about LDS contents."""
    case = bc.Case(f"{prec_name}-d{d}-C{C}-offset", prec_name, d, C, "offset")
    prec = get_precision(prec_name)
    sizes, _, host, models = bc.softmax_inputs(d, prec_name, C)
    parts = device_parts(d, prec_name, C)
    beta = models["offset"][0].to(DEV)
    plan = build(case, "coded", bc.WHOLE_TASKS, monkeypatch)
    first = run(plan, beta).clone()
    big, _ = nx.hostile_softmax_models(np.random.RandomState(5), host, d, 8, prec)["saturated"]
    big = big.reshape(8, -1).clone()
    big[5:] *= 10.0
    dirty = SoftmaxGradPlan(bc.naive_messages(len(sizes)), parts, prec, 8, d)
    for _ in range(3):
        Gd = run(dirty, big.reshape(-1).to(DEV))
    again = run(plan, beta)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Gd).all())
    bc.check_softmax(first, case, "coded", case.id)
    assert torch.equal(first, again)


# ---- 3. the labels of a partition reach the messages that read it, and no other
@pytest.mark.parametrize("C,d,prec_name,kind", [(3, 37, "fp64", "coded"), (5, 1000, "fp32", "coded"),
                                                (2, 129, "fp64", "naive"), (6, 37, "fp32", "naive")])
def test_labels_reach_exactly_the_messages_that_read_them(C, d, prec_name, kind, native, monkeypatch):
    case = bc.Case(f"{prec_name}-d{d}-C{C}-offset", prec_name, d, C, "offset")
    sizes, _, _, models = bc.softmax_inputs(d, prec_name, C)
    parts = device_parts(d, prec_name, C)
    beta = models["offset"][0].to(DEV)
    msgs = bc.MESSAGES[kind](len(sizes))
    clean = run(build(case, kind, bc.ODD_TASKS, monkeypatch), beta)
    for p in (0, len(sizes) - 3):  # the one-row partition; 2S + 1 rows (several tasks where 2S + 1 > 37)
        changed = dict(parts)
        X, y = parts[p]
        changed[p] = (X, ((y + 1) % C).contiguous())
        G = run(build(case, kind, bc.ODD_TASKS, monkeypatch, parts=changed), beta)
        torch.cuda.synchronize()
        for s, m in enumerate(msgs):
            reads = any(q == p and c != 0.0 for q, c in m)
            assert torch.equal(G[s], clean[s]) != reads, (p, s, m)


# ---- 4. launcher validation: an error, not a launch
def test_launcher_rejects_invalid_arguments(native):
    i32 = dict(dtype=torch.int32, device=DEV)
    segs = torch.zeros(32, dtype=torch.uint8, device=DEV)
    tasks, ptb = torch.zeros((0, 5), **i32), torch.zeros(1, **i32)
    buf = torch.zeros(8 * 1024, dtype=torch.float64, device=DEV)

    def call(dtype=0, classes=3, d_x=37, ld_x=38):
        native._grad_softmax_raw(dtype, classes, segs, tasks, ptb, buf, buf, buf, d_x, ld_x)

    call()
    call(dtype=1, ld_x=40)
    call(classes=2)
    call(classes=8, d_x=1024, ld_x=1024)
    bad = [dict(classes=1), dict(classes=9), dict(ld_x=0, d_x=0), dict(ld_x=1026, d_x=1000), dict(d_x=0), dict(d_x=39),
           dict(ld_x=37, d_x=37), dict(dtype=1, ld_x=38), dict(dtype=2, ld_x=40), dict(dtype=3, ld_x=40), dict(dtype=4),
           dict(dtype=-1)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="invalid"):
            call(**kw)
    torch.cuda.synchronize()
