"""The seven slab-reduction kernels and encode_messages against the order emulators of tests/slab_edge_cases.py, bit
for bit, on hostile slabs the test supplies itself (GPU only).

The raw entry points (_slab_reduce_raw, _slab_update_raw, encode_messages with sub_begin / gate) run the launchers on
caller-supplied tensors.  Every output is prefilled with a sentinel and has a guard region behind it; the rows of the
slab outside the messages are NaN, and so is the partial buffer before a launch, so a read past a message or of a
stale partial poisons a sum.  A NaN of the emulator has to be a NaN of the device (its payload is not compared).

The fp32 denormal column assumes the kernels keep fp32 denormals (the build passes no flush flag).
"""
import contextlib
import functools
import uuid

import numpy as np
import pytest
import torch

import slab_edge_cases as se

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECS = ("fp64", "fp32")
CODE = {"fp64": 0, "fp32": 1}
TORCH = {"fp64": torch.float64, "fp32": torch.float32}
SENTINEL = -7.25  # no sum of a hostile slab (asserted)
GUARD = 96  # elements behind every output
RANK = 3

REDUCE = se.reduce_cases()
PUTS = se.put_cases()
ENCODE = se.encode_cases()


# ---- helpers -------------------------------------------------------------------------------------------------
def _guarded(rows, ld, dtype, fill=SENTINEL):
    """(buffer, its first rows * ld elements as [rows, ld]): the view is what a launch gets, the rest is the guard."""
    buf = torch.full((rows * ld + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:rows * ld].view(rows, ld)


def _guard_intact(buf, rows, ld, fill=SENTINEL):
    return bool(torch.all(buf[rows * ld:] == fill))


def _untouched(buf, fill=SENTINEL):
    return bool(torch.all(buf == fill))


def _part(nslots, ld, dtype):
    return torch.full((nslots * se.SPLITS * ld,), float("nan"), dtype=dtype, device=DEV)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the references are read-only


def _same(got_t, want):
    return bool(np.all(se.same_bits(got_t.cpu().numpy(), want)))


@contextlib.contextmanager
def _mode(C, mode):
    C.set_slab_reduce_mode(mode)
    try:
        yield
    finally:
        C.set_slab_reduce_mode(1)


@functools.lru_cache(maxsize=None)
def _slab_ref(seed, counts, lead, ld, prec):
    """(slab, stb, the emulator's G), computed once per case and left unchanged."""
    dtype = se.DTYPES[prec]
    slab, stb = se.slab_case(seed, counts, lead, ld, dtype)
    want = se.emulate_slab(slab, stb, dtype)
    assert not np.any(want == SENTINEL)
    for a in (slab, stb, want):
        a.setflags(write=False)
    return slab, stb, want


def _put_counts(nslots):
    return tuple(se.PUT_COUNTS[i % len(se.PUT_COUNTS)] for i in range(nslots))


def _update_counts(nslots):
    return tuple(se.UPDATE_TASKS[i % len(se.UPDATE_TASKS)] for i in range(nslots))


@pytest.fixture(scope="module")
def flags(native):
    f = native.ShmFlags("/eh_t_" + uuid.uuid4().hex[:12], 2, True)
    yield f
    f.close()


def test_case_tables_are_the_extension_s(native):
    g = native._slab_geometry()
    assert (g["splits"], g["put_one_elems"], g["put_one_slots"]) == (se.SPLITS, se.PUT_ONE_ELEMS, se.PUT_ONE_SLOTS)
    assert native.MAX_MSGS == se.MAX_MSGS


# ---- plain forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mode", [0, 1], ids=["two-stage", "fused"])
@pytest.mark.parametrize("case", REDUCE, ids=[c.id for c in REDUCE])
def test_plain_forms_sum_in_the_documented_order(case, mode, prec, native):
    """slab_reduce_partial + slab_reduce_final (mode 0) and slab_reduce_fused (mode 1): G is the emulator's, every
    live element written, the guard untouched; under a closed gate G keeps the sentinel."""
    C, dt = native, TORCH[prec]
    slab, stb, want = _slab_ref(REDUCE.index(case), case.counts, case.lead, case.ld, prec)
    nslots = len(case.counts)
    slab_d, stb_d = _dev(slab), _dev(stb)
    buf, G = _guarded(nslots, case.ld, dt)
    shut, Gs = _guarded(nslots, case.ld, dt)
    with _mode(C, mode):
        C._slab_reduce_raw(CODE[prec], slab_d, stb_d, _part(nslots, case.ld, dt), G)
        C._slab_reduce_raw(CODE[prec], slab_d, stb_d, _part(nslots, case.ld, dt), Gs,
                           gate=torch.ones(1, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
    bad = ~se.same_bits(G.cpu().numpy(), want)
    assert not bad.any(), (case.id, mode, prec, np.argwhere(bad)[:8].tolist())
    assert _guard_intact(buf, nslots, case.ld) and _untouched(shut)


# ---- put forms -----------------------------------------------------------------------------------------------
def _tags_of(rows, value):
    """The MsgTags a put of these rows must write: (round1, rank, sum_c bits_c (2c + 1) mod 2^64), from the bits."""
    a = rows.cpu().numpy()
    bits = a.view(np.uint64 if a.dtype == np.float64 else np.uint32).astype(np.uint64)
    odd = 2 * np.arange(a.shape[1], dtype=np.uint64) + np.uint64(1)
    with np.errstate(over="ignore"):
        sums = (bits * odd[None, :]).sum(axis=1, dtype=np.uint64)
    want = np.zeros(a.shape[0], dtype=[("round1", "<u4"), ("rank", "<u4"), ("sum", "<u8")])
    want["round1"], want["rank"], want["sum"] = value, RANK, sums
    return want


class _Put:
    """The operands of one tagged put: sentinel-filled G and dst with guards, zero tags, counters and scratch."""

    def __init__(self, nslots, ld, dt, flags, value, abort=False):
        self.nslots, self.ld = nslots, ld
        self.gbuf, self.G = _guarded(nslots, ld, dt)
        self.dbuf, self.dst = _guarded(nslots, ld, dt)
        self.tags = torch.zeros(nslots * 16 + 16, dtype=torch.uint8, device=DEV)
        self.counters = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.csum = torch.zeros(nslots + 1, dtype=torch.int64, device=DEV)
        self.desc = dict(dst=self.dst, tags=self.tags, flag=flags.dev_addr(0), value=value, rank=RANK,
                         counters=self.counters, csum=self.csum)
        if abort:
            self.desc["abort"] = torch.ones(1, dtype=torch.int32, device=DEV)

    def scratch_is_zero(self):
        return int(self.counters.abs().sum()) == 0 and int(self.csum.abs().sum()) == 0

    def tags_host(self):
        return self.tags.cpu().numpy()[:self.nslots * 16].view([("round1", "<u4"), ("rank", "<u4"), ("sum", "<u8")])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["two-stage", "fused", "fused-plain"])
@pytest.mark.parametrize("case", PUTS, ids=[c.id for c in PUTS])
def test_put_forms_carry_the_emulator_s_bits_and_tags(case, mode, prec, native, flags):
    """slab_reduce_fused_put (mode 1) and, by the selectors, slab_reduce_final_put1 / slab_reduce_final_put (modes 0
    and 2): G and dst hold the emulator's bits, every tag is the checksum of the stored row with its round and rank,
    the flag holds the value and the sender scratch is back to zero; an empty message carries a zero checksum.
    Abort word set: G written, dst, tags and flag untouched, scratch zero.  Gate closed: nothing written."""
    C, dt = native, TORCH[prec]
    nslots, ld = case.nslots, case.ld
    counts = _put_counts(nslots)
    slab, stb, want = _slab_ref(1000 + PUTS.index(case), counts, 0, ld, prec)
    slab_d, stb_d = _dev(slab), _dev(stb)
    value = 100 + 10 * PUTS.index(case) + mode
    flags.store(0, 1)
    with _mode(C, mode):
        live = _Put(nslots, ld, dt, flags, value)
        C._slab_reduce_raw(CODE[prec], slab_d, stb_d, _part(nslots, ld, dt), live.G, put=live.desc)
        torch.cuda.synchronize()
        assert flags.load(0) == value
        gone = _Put(nslots, ld, dt, flags, value + 1, abort=True)
        C._slab_reduce_raw(CODE[prec], slab_d, stb_d, _part(nslots, ld, dt), gone.G, put=gone.desc)
        shut = _Put(nslots, ld, dt, flags, value + 2)
        C._slab_reduce_raw(CODE[prec], slab_d, stb_d, _part(nslots, ld, dt), shut.G,
                           gate=torch.ones(1, dtype=torch.int32, device=DEV), put=shut.desc)
        torch.cuda.synchronize()
    assert flags.load(0) == value  # neither the aborted nor the gated put announced anything
    # the live put
    assert _same(live.G, want) and _same(live.dst, want), (case.id, mode, prec)
    assert _guard_intact(live.gbuf, nslots, ld) and _guard_intact(live.dbuf, nslots, ld)
    got, tags = live.tags_host(), _tags_of(live.dst, value)
    assert np.array_equal(got, tags), (case.id, mode, prec)
    assert not np.any(live.tags.cpu().numpy()[nslots * 16:])
    assert C.verify_rows(live.dst, live.tags, value, RANK) == {}
    assert live.scratch_is_zero()
    for s, n in enumerate(counts):
        if n == 0:
            assert not np.any(live.dst[s].cpu().numpy().view(np.uint8)) and got["sum"][s] == 0
    # the aborted put: the local copy only
    assert _same(gone.G, want) and _guard_intact(gone.gbuf, nslots, ld)
    assert _untouched(gone.dbuf) and not np.any(gone.tags.cpu().numpy()) and gone.scratch_is_zero()
    # the gated put: nothing at all
    assert _untouched(shut.gbuf) and _untouched(shut.dbuf) and not np.any(shut.tags.cpu().numpy())
    assert shut.scratch_is_zero()


# ---- update form ---------------------------------------------------------------------------------------------
def _update_cases():
    return [(p, c) for p in PRECS for c in se.update_cases(p)]


@pytest.mark.parametrize("prec,case", _update_cases(), ids=[f"{p}-{c.id}" for p, c in _update_cases()])
def test_update_form_is_the_emulator_then_combine_update(prec, case, native):
    """slab_reduce_partial + slab_final_update: G is the emulator's; beta, u, hist and beta_w are, bit for bit, what
    combine_update gives from the same G rows, slot list and coefficients (its own long-double test:
    test_eval_edges_gpu.py); columns d..ld of beta_w are exact zeros, and beta, u and hist are untouched there."""
    C, dt = native, TORCH[prec]
    nslots, ld, d = case.nslots, case.ld, case.d
    key = 2000 + 10 * nslots + (prec == "fp32")
    slab, stb, want = _slab_ref(key, _update_counts(nslots), 0, ld, prec)
    rng = np.random.RandomState(key + case.nmsg)
    slots, coefs = se.slot_list(nslots, case.nmsg), se.update_coefs(rng, case.nmsg)
    scale = 10.0 ** rng.uniform(-3, 3, ld)
    b0, u0 = rng.standard_normal(ld) * scale, rng.standard_normal(ld) * scale
    h0 = np.full(ld, 5.5)
    decay, gm, l2, theta = 0.999, 1e-3, 2e-4, 0.3

    def state():
        return _dev(b0.copy()), _dev(u0.copy()), _dev(h0.copy()), torch.full((ld,), 7.0, dtype=dt, device=DEV)

    beta, u, hist, bw = state()
    buf, G = _guarded(nslots, ld, dt)
    C._slab_update_raw(CODE[prec], _dev(slab), _dev(stb), _part(nslots, ld, dt), G, slots, coefs, beta, u, hist, bw, d,
                       case.rule, decay, gm, l2, theta)
    torch.cuda.synchronize()
    assert _same(G, want) and _guard_intact(buf, nslots, ld), case.id
    rbeta, ru, rhist, rbw = state()
    C.combine_update([G[s] for s in slots], coefs, rbeta, ru, rhist, rbw, None, d, decay, gm, l2, theta, case.rule)
    torch.cuda.synchronize()
    for name, got, ref in (("beta", beta, rbeta), ("u", u, ru), ("hist", hist, rhist), ("beta_w", bw, rbw)):
        assert _same(got, ref.cpu().numpy()), (case.id, name)
    # the padding, by the test's own word
    assert not np.any(bw[d:].cpu().numpy().view(np.uint8))
    assert np.array_equal(beta[d:].cpu().numpy(), b0[d:]) and np.array_equal(u[d:].cpu().numpy(), u0[d:])
    assert np.array_equal(hist[d:].cpu().numpy(), h0[d:])
    if d:
        assert not np.array_equal(beta[:d].cpu().numpy(), b0[:d])  # ... and something was updated
        assert (case.rule == 1) != np.array_equal(u[:d].cpu().numpy(), u0[:d])  # GD leaves u alone


# ---- encode --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _encode_ref(ld, sub, prec):
    dtype = se.DTYPES[prec]
    ptr, idx, coef, sb, rows, live = se.encode_tables(sub)
    Gb = se.hostile_slab(np.random.RandomState(3000 + ld + sub), rows, ld, dtype, live=live)
    want = se.emulate_encode(Gb, ptr, idx, coef, dtype, sb)
    assert not np.any(want == SENTINEL)
    return Gb, ptr, idx, coef, sb, want


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", ENCODE, ids=[c.id for c in ENCODE])
def test_encode_is_the_emulated_fma_chain(case, prec, native):
    """Both modes of encode_messages: the emulator's bits, exact +0.0 in a slot without nonzeros, the guard
    untouched; an open gate changes nothing and a closed one leaves G alone."""
    C, dt = native, TORCH[prec]
    Gb, ptr, idx, coef, sb, want = _encode_ref(case.ld, case.sub, prec)
    nslots = len(ptr) - 1
    ops = [_dev(Gb), _dev(ptr), _dev(idx), _dev(coef)]
    sbd = _dev(sb) if case.sub else None
    buf, G = _guarded(nslots, case.ld, dt)
    opened, Go = _guarded(nslots, case.ld, dt)
    shut, Gs = _guarded(nslots, case.ld, dt)
    C.encode_messages(*ops, G, sub_begin=sbd)
    C.encode_messages(*ops, Go, sub_begin=sbd, gate=torch.zeros(1, dtype=torch.int32, device=DEV))
    C.encode_messages(*ops, Gs, sub_begin=sbd, gate=torch.ones(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    bad = ~se.same_bits(G.cpu().numpy(), want)
    assert not bad.any(), (case.id, prec, np.argwhere(bad)[:8].tolist())
    assert torch.equal(buf.view(torch.uint8), opened.view(torch.uint8)) and _guard_intact(buf, nslots, case.ld)
    assert _untouched(shut)
    empty = [s for s in range(nslots) if ptr[s] == ptr[s + 1]]
    assert empty and not np.any(G[empty].cpu().numpy().view(np.uint8))


# ---- launcher validation -------------------------------------------------------------------------------------
class _Valid:
    """A valid call of the raw bindings on a small slab; the tests break one operand at a time."""

    def __init__(self, prec="fp64"):
        self.dt = TORCH[prec]
        self.counts, self.ld = (5, 0, 17), 65
        self.nslots = len(self.counts)
        slab, stb, _ = _slab_ref(4000, self.counts, 0, self.ld, prec)
        self.slab, self.stb = _dev(slab), _dev(stb)
        self.part = _part(self.nslots, self.ld, self.dt)
        self.buf, self.G = _guarded(self.nslots, self.ld, self.dt)
        self.code = CODE[prec]

    def args(self, **over):
        a = dict(dtype=self.code, slab=self.slab, stb=self.stb, part=self.part, G=self.G)
        a.update(over)
        return [a[k] for k in ("dtype", "slab", "stb", "part", "G")]

    def nothing_ran(self):
        torch.cuda.synchronize()
        return _untouched(self.buf)


def _stb(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _bad_operands(v):
    other = torch.float32 if v.dt == torch.float64 else torch.float64
    rows = v.slab.shape[0]
    return {
        "storage code": dict(dtype=7),
        "slab on the host": dict(slab=v.slab.cpu()),
        "slab of another type": dict(slab=v.slab.to(other)),
        "part of another type": dict(part=v.part.to(other)),
        "G of another type": dict(G=v.G.to(other)),
        "slab of another width": dict(slab=v.slab[:, :v.ld - 1].contiguous()),
        "slab not contiguous": dict(slab=v.slab.t().contiguous().t()),
        "stb too short": dict(stb=_stb(0, 5, 22)),
        "stb int64": dict(stb=v.stb.long()),
        "stb steps back": dict(stb=_stb(0, 6, 5, 22)),
        "stb starts below the slab": dict(stb=_stb(-1, 5, 5, 22)),
        "stb ends past the slab": dict(stb=_stb(0, 5, 5, rows + 1)),
        "part too small": dict(part=v.part[:-1]),
    }


def test_reduce_binding_rejects_before_any_launch(native, flags):
    C = native
    v = _Valid()
    for what, over in _bad_operands(v).items():
        with pytest.raises(ValueError):
            C._slab_reduce_raw(*v.args(**over))
        assert v.nothing_ran(), what
    with pytest.raises(ValueError):
        C._slab_reduce_raw(*v.args(), gate=torch.ones(1, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        C._slab_reduce_raw(*v.args(), gate=torch.ones(1, dtype=torch.int32))
    good = _Put(v.nslots, v.ld, v.dt, flags, 9)
    flags.store(0, 1)
    bad_puts = {
        "dst of another shape": dict(dst=good.dst[:, :v.ld - 1].contiguous()),
        "dst of another type": dict(dst=good.dst.float()),
        "tags too short": dict(tags=good.tags[:v.nslots * 16 - 1]),
        "csum int32": dict(csum=good.csum.int()),
        "csum too short": dict(csum=good.csum[:v.nslots - 1]),
        "counters int64": dict(counters=good.counters.long()),
        "no flag": dict(flag=0),
        "abort on the host": dict(abort=torch.ones(1, dtype=torch.int32)),
    }
    for what, over in bad_puts.items():
        with pytest.raises(ValueError):
            C._slab_reduce_raw(*v.args(), put=dict(good.desc, **over))
        assert v.nothing_ran() and _untouched(good.dbuf) and flags.load(0) == 1, what
    lacking = dict(good.desc)
    del lacking["csum"]
    with pytest.raises(ValueError):
        C._slab_reduce_raw(*v.args(), put=lacking)
    # more messages than one tagged put has tag rows (integrity.h kMaxTagRows = 1024)
    n = 1025
    wide = dict(slab=torch.zeros(n, 1, dtype=v.dt, device=DEV), stb=torch.arange(n + 1, dtype=torch.int32, device=DEV),
                part=_part(n, 1, v.dt), G=torch.full((n, 1), SENTINEL, dtype=v.dt, device=DEV))
    many = _Put(n, 1, v.dt, flags, 9)
    with pytest.raises(ValueError):
        C._slab_reduce_raw(*v.args(**wide), put=many.desc)
    torch.cuda.synchronize()
    assert _untouched(wide["G"]) and _untouched(many.dbuf) and flags.load(0) == 1


def test_update_binding_rejects_before_any_launch(native):
    C = native
    v = _Valid()
    ld = v.ld

    def state(**over):
        s = dict(slots=[2, 0], coefs=[1.0, -1.0], beta=torch.ones(ld, dtype=torch.float64, device=DEV),
                 u=torch.ones(ld, dtype=torch.float64, device=DEV), hist=torch.ones(ld, dtype=torch.float64, device=DEV),
                 beta_w=torch.ones(ld, dtype=v.dt, device=DEV), d=ld - 1, rule=0)
        s.update(over)
        return [s[k] for k in ("slots", "coefs", "beta", "u", "hist", "beta_w", "d", "rule")] + [1.0, 0.1, 0.0, 0.5]

    keep = state()
    for what, over in _bad_operands(v).items():
        with pytest.raises(ValueError):
            C._slab_update_raw(*v.args(**over), *keep)
        assert v.nothing_ran(), what
    bad = {
        "a slot past G": dict(slots=[2, v.nslots]),
        "a negative slot": dict(slots=[-1, 0]),
        "slots and coefs differ": dict(coefs=[1.0]),
        "too many messages": dict(slots=[0] * (se.MAX_MSGS + 1), coefs=[1.0] * (se.MAX_MSGS + 1)),
        "d past ld": dict(d=ld + 1),
        "negative d": dict(d=-1),
        "rule": dict(rule=2),
        "beta too short": dict(beta=torch.ones(ld - 1, dtype=torch.float64, device=DEV)),
        "beta fp32": dict(beta=torch.ones(ld, dtype=torch.float32, device=DEV)),
        "u on the host": dict(u=torch.ones(ld, dtype=torch.float64)),
        "hist too short": dict(hist=torch.ones(ld - 1, dtype=torch.float64, device=DEV)),
        "beta_w of another type": dict(beta_w=torch.ones(ld, dtype=torch.float32, device=DEV)),
        "beta_w too short": dict(beta_w=torch.ones(ld - 1, dtype=v.dt, device=DEV)),
    }
    for what, over in bad.items():
        s = state(**over)
        with pytest.raises(ValueError):
            C._slab_update_raw(*v.args(), *s)
        assert v.nothing_ran(), what
        assert all(bool(torch.all(t == 1)) for t in s[2:6]), what
    # the limit itself is accepted: MAX_MSGS messages, d = ld
    s = state(slots=[0] * se.MAX_MSGS, coefs=[0.5] * se.MAX_MSGS, d=ld)
    C._slab_update_raw(*v.args(), *s)
    assert not v.nothing_ran()


def test_encode_binding_checks_the_tables_of_the_row_block_mode(native):
    C = native
    Gb, ptr, idx, coef, sb, _ = _encode_ref(255, True, "fp64")
    ops = dict(Gb=_dev(Gb), ptr=_dev(ptr), idx=_dev(idx), coef=_dev(coef))
    buf, G = _guarded(len(ptr) - 1, 255, torch.float64)
    past = sb.copy()
    past[-1] = Gb.shape[0] + 1
    back = sb.copy()
    back[2] = back[1] - 1
    wrong = idx.copy()
    wrong[0] = len(sb) - 1
    back_ptr = ptr.copy()
    back_ptr[2] = back_ptr[1] + 5
    for what, over, sub in (("sub_begin past Gb", {}, past), ("sub_begin steps back", {}, back),
                            ("idx past the partitions", dict(idx=_dev(wrong)), sb),
                            ("ptr steps back", dict(ptr=_dev(back_ptr)), sb),
                            ("sub_begin int64", {}, sb.astype(np.int64))):
        a = dict(ops, **over)
        with pytest.raises(ValueError):
            C.encode_messages(a["Gb"], a["ptr"], a["idx"], a["coef"], G, sub_begin=_dev(sub))
        torch.cuda.synchronize()
        assert _untouched(buf), what
    with pytest.raises(ValueError):
        C.encode_messages(ops["Gb"], ops["ptr"], ops["idx"], ops["coef"], G, gate=torch.ones(1, dtype=torch.int32))
    torch.cuda.synchronize()
    assert _untouched(buf)
