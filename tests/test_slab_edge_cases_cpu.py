"""The tables of tests/slab_edge_cases.py sit on the selectors of the slab reduction, its order emulator is a sum and
has teeth against the orders a wrong kernel would run, and the encode emulator's fused step rounds once (no GPU).
"""
import fractions
import os
import re

import numpy as np
import pytest

import slab_edge_cases as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
REDUCE = se.reduce_cases()
QUARTER = 0.25  # the least share of finite columns a wrong order has to change (a condition, not a
# measurement: the least share measured on these cases is 0.36)


def _geometry():
    """kSlabSplits, kPutOneElems, kPutOneSlots, kMaxMsgs: from the extension when it loads, else from the headers."""
    try:
        from erasurehead_amd._ext import native

        C = native(build_if_missing=False)
        g = C._slab_geometry()
        return int(g["splits"]), int(g["put_one_elems"]), int(g["put_one_slots"]), int(C.MAX_MSGS)
    except Exception:
        text = "".join(open(os.path.join(ROOT, "csrc", "kernels", f)).read() for f in ("launchers.h", "slab_reduce.h"))
        return tuple(int(re.search(name + r"\s*=\s*(\d+)", text).group(1))
                     for name in ("kSlabSplits", "kPutOneElems", "kPutOneSlots", "kMaxMsgs"))


# ---- the tables --------------------------------------------------------------------------------------------
def test_tables_are_held_to_the_headers():
    assert _geometry() == (se.SPLITS, se.PUT_ONE_ELEMS, se.PUT_ONE_SLOTS, se.MAX_MSGS)
    header = open(os.path.join(ROOT, "csrc", "kernels", "slab_reduce.h")).read()
    assert "kPutOneElems" in header and "kPutOneSlots" in header
    assert "constexpr int kPutOne" not in open(os.path.join(ROOT, "csrc", "kernels", "slab_reduce.hip")).read()


def _splits(n):
    """Rows of each of the 16 splits of a message of n rows, None for a split that starts past the end."""
    per = se.ceil_per(n)
    return [None if k * per >= n and n else max(0, min(n, (k + 1) * per) - k * per) for k in range(se.SPLITS)]


def test_task_counts_reach_the_split_edges():
    assert len(se.TASKS) == 14 and set(se.ALL_TASKS) == set(se.TASKS)
    assert _splits(17) == [2] * 8 + [1] + [None] * 7  # splits of 2, 2, ..., 1 and seven that start past the end
    assert _splits(16) == [1] * 16 and _splits(15) == [1] * 15 + [None] and _splits(1) == [1] + [None] * 15
    assert _splits(128) == [8] * 16  # one full 8-row step of fused_split_sum
    assert _splits(127) == [8] * 15 + [7] and _splits(129) == [9] * 14 + [3, None]  # tail only; step + tail
    assert _splits(145) == [10] * 14 + [5, None] and _splits(272) == [17] * 16  # two steps + tail
    assert {r % 8 for n in se.TASKS for r in _splits(n) if r} >= {0, 1, 2, 3, 5, 7}
    # short and empty messages stand between long ones, and one layout starts inside the slab
    for counts in (se.ALL_TASKS, se.LAYOUTS[0]):
        assert any(counts[i - 1] >= 17 and counts[i] == 0 and counts[i + 1] >= 1 for i in range(1, len(counts) - 1))
    assert se.LAYOUTS[0] == (17, 0, 1, 129, 0, 33) and (0,) in se.LAYOUTS and (17,) in se.LAYOUTS
    assert [c.lead for c in REDUCE if c.counts == se.LAYOUTS[se.LEAD_LAYOUT]] == [se.LEAD, se.LEAD]
    assert {c.ld for c in REDUCE if c.counts == se.ALL_TASKS} == set(se.WIDTHS)
    assert set(se.WIDTHS) == {1, 63, 64, 65, 255, 256, 257, 1000, 1024}


def test_put_cases_sit_on_the_selectors():
    P = {(c.nslots, c.ld): c for c in se.put_cases()}
    rows = se.PUT_ONE_ELEMS // 1024
    assert {(rows, 1024), (rows + 1, 1024), (se.PUT_ONE_SLOTS, 256), (se.PUT_ONE_SLOTS + 1, 8)} <= set(P)
    assert rows * 1024 == se.PUT_ONE_ELEMS == se.PUT_ONE_SLOTS * 256 and (se.PUT_ONE_SLOTS + 1) * 8 <= se.PUT_ONE_ELEMS
    for (n, ld), c in P.items():
        assert se.put_kernel(n, ld, 0) == se.put_kernel(n, ld, 2) == c.kernel
        assert se.put_kernel(n, ld, 1) == "slab_reduce_fused_put"
    one = [k for k, c in P.items() if c.kernel == "slab_reduce_final_put1"]
    assert any(se.last_pair_single(*k) for k in one) and any(not se.last_pair_single(*k) for k in one)
    assert se.last_pair_single(3, 1000) and se.last_pair_single(1, 1) and not se.last_pair_single(rows, 1024)
    # the many-block put on its 256-column block boundary; every case holds an empty (all-zero) message
    assert {(17, 255), (17, 257)} <= {k for k, c in P.items() if c.kernel == "slab_reduce_final_put"}
    assert all(0 in [se.PUT_COUNTS[i % len(se.PUT_COUNTS)] for i in range(n)] or n == 1 for n, _ in P)


def test_update_cases_reach_the_wave_loop_and_the_lds_limit():
    for prec, size in (("fp64", 8), ("fp32", 4)):
        cases = se.update_cases(prec)
        assert {c.nslots for c in cases} == set(se.UPDATE_NSLOTS) - ({129} if prec == "fp32" else set())
        assert {c.nmsg for c in cases} == {1, 8, 9, se.MAX_MSGS} and {c.rule for c in cases} == {0, 1}
        assert any(c.d < c.ld for c in cases) and all(c.d <= c.ld for c in cases)
        lds = [c.nslots * 64 * size for c in cases]
        assert (max(lds) > 65536) == (prec == "fp64")
    assert 128 * 64 * 8 == 65536 < 129 * 64 * 8  # 129 fp64 slots: the first count past 64 KiB
    for nslots in se.UPDATE_NSLOTS:
        for nmsg in se.UPDATE_NMSG:
            s = se.slot_list(nslots, nmsg)
            assert len(s) == nmsg and all(0 <= x < nslots for x in s)
            if nmsg > 1:
                assert len(set(s)) < len(s)  # a slot repeats
            if nslots > 1:
                assert nslots // 2 not in s  # a slot is left unused
            if nslots > 2 and nmsg > 2:
                assert s[0] > s[1]  # backwards
            c = se.update_coefs(np.random.RandomState(0), nmsg)
            assert c[-1] < 0 and (nmsg == 1 or 0.0 in c)


def test_encode_tables_have_the_hostile_shapes():
    nnz = [len(m) for m in se.ENCODE_MSGS]
    assert set(nnz) == {0, 1, 2, 3, 4} and se.ENCODE_BLOCKS == (0, 1, 15, 16, 17, 33)
    assert any(c == 0.0 for m in se.ENCODE_MSGS for _, c in m) and any(c < 0 for m in se.ENCODE_MSGS for _, c in m)
    assert {p for m in se.ENCODE_MSGS for p, _ in m} == set(range(len(se.ENCODE_BLOCKS)))
    assert {c.ld for c in se.encode_cases()} == {1, 255, 256, 257} and {c.sub for c in se.encode_cases()} == {False, True}
    for sub in (False, True):
        ptr, idx, coef, sb, rows, live = se.encode_tables(sub)
        assert len(ptr) == len(se.ENCODE_MSGS) + 1 and ptr[-1] == len(idx) == len(coef)
        if sub:
            assert list(np.diff(sb)) == list(se.ENCODE_BLOCKS) and sb[0] == se.LEAD and sb[-1] + se.TAIL == rows
            assert idx.max() < len(sb) - 1
        else:
            assert live[0] <= idx.min() and idx.max() < live[1] and live[1] + se.TAIL == rows


# ---- the hostile slab ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_hostile_slab_has_its_features(prec):
    dtype = se.DTYPES[prec]
    seen = set()
    for i, case in enumerate(REDUCE):
        slab, stb = se.slab_case(i, case.counts, case.lead, case.ld, dtype)
        lo, hi = int(stb[0]), int(stb[-1])
        assert slab.dtype == dtype and slab.shape == (hi + se.TAIL, case.ld)
        assert np.all(np.isnan(slab[:lo])) and np.all(np.isnan(slab[hi:]))
        live, cols = slab[lo:hi], se.special_columns(case.ld)
        plain = np.delete(live, list(cols.values()), axis=1)
        if plain.size >= 4000:
            assert 0.03 < np.mean(plain == 0) < 0.07 and np.any(np.signbit(plain[plain == 0]))
            mag = np.abs(plain[plain != 0])
            assert mag.min() < 1e-5 and mag.max() > 1e5  # twelve decades
        G = se.emulate_slab(slab, stb, dtype)
        if "neg_zero" in cols and hi > lo:
            c = cols["neg_zero"]
            assert np.all(np.signbit(live[:, c])) and not np.any(live[:, c])
            assert not np.any(G[:, c]) and not np.any(np.signbit(G[:, c]))  # the sum of -0.0 from +0.0 is +0.0
        if "denormal" in cols:
            assert np.all(np.abs(live[:, cols["denormal"]]) < np.finfo(dtype).tiny)
        if len(cols) == len(se.SPECIALS) and hi - lo >= 17:
            seen |= {k for k in ("inf", "inf_minus_inf", "nan", "overflow") if not np.all(np.isfinite(G[:, cols[k]]))}
            if np.any(np.isposinf(G[:, cols["overflow"]])) and np.all(np.isfinite(live[:, cols["overflow"]])):
                seen.add("overflow from finite values")
            if np.any(np.isnan(G[:, cols["inf_minus_inf"]])) and not np.any(np.isnan(live[:, cols["inf_minus_inf"]])):
                seen.add("inf - inf")
            pairs = live[:, cols["pairs"]]
            assert np.array_equal(pairs[0:len(pairs) // 2 * 2:2], -pairs[1::2])
    assert seen == {"inf", "inf_minus_inf", "nan", "overflow", "overflow from finite values", "inf - inf"}


# ---- the emulator is a sum, and another order is another result -----------------------------------------------
def _finite_entries(slab, stb, G, min_rows, skip=lambda n: False):
    """Mask over G: messages of at least min_rows rows (and not skipped), columns whose rows and sum are finite."""
    mask = np.zeros(G.shape, bool)
    for s in range(len(stb) - 1):
        n = int(stb[s + 1] - stb[s])
        if n >= min_rows and not skip(n):
            mask[s] = np.all(np.isfinite(slab[stb[s]:stb[s + 1]]), axis=0) & np.isfinite(G[s])
    return mask


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_emulator_is_within_the_plain_bound_of_the_long_double_sum(prec):
    """|emulate_slab - the long-double column sum| <= (n + 4) u sum |x| in every column that holds numbers."""
    dtype = se.DTYPES[prec]
    u = float(np.finfo(dtype).eps) / 2
    for i, case in enumerate(REDUCE):
        slab, stb = se.slab_case(i, case.counts, case.lead, case.ld, dtype)
        G = se.emulate_slab(slab, stb, dtype)
        mask = _finite_entries(slab, stb, G, 0)
        for s in range(len(stb) - 1):
            rows = slab[stb[s]:stb[s + 1]].astype(LD)
            n = rows.shape[0]
            with np.errstate(all="ignore"):  # the columns of inf and NaN are masked below
                err = np.abs(G[s].astype(LD) - rows.sum(0))
                bound = (n + 4) * LD(u) * np.abs(rows).sum(0)
            assert np.all(err[mask[s]] <= bound[mask[s]]), (case.id, s)
            if n == 0:
                assert not np.any(G[s]) and not np.any(np.signbit(G[s]))


_shares = {}


def _mutant_shares(prec):
    """{case id: (share against row order, share against the floor split or None)} over the finite entries of the
    messages the mutant can differ in."""
    if prec not in _shares:
        dtype = se.DTYPES[prec]
        out = {}
        for i, case in enumerate(REDUCE):
            if max(case.counts) < 17:
                continue
            slab, stb = se.slab_case(i, case.counts, case.lead, case.ld, dtype)
            G = se.emulate_slab(slab, stb, dtype)
            rows = _finite_entries(slab, stb, G, 17)
            a = np.mean(~se.same_bits(se.row_order_sum(slab, stb, dtype), G)[rows])
            floor = _finite_entries(slab, stb, G, 17, skip=lambda n: n % se.SPLITS == 0)
            b = None
            if floor.any():
                b = np.mean(~se.same_bits(se.emulate_slab(slab, stb, dtype, per_of=lambda n: n // se.SPLITS), G)[floor])
            out[case.id] = (a, b)
        _shares[prec] = out
    return _shares[prec]


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_other_orders_change_a_quarter_of_the_columns(prec):
    """On every hostile case with 17 or more rows in some message, summing in row order changes at least a quarter
    of the finite columns of those messages, and so does per = floor(n / 16) where 16 does not divide the count."""
    shares = _mutant_shares(prec)
    assert len(shares) >= len(se.WIDTHS) + 8
    print(f"{prec}: row order differs in {min(a for a, _ in shares.values()):.2f} .. "
          f"{max(a for a, _ in shares.values()):.2f} of the finite columns, floor split in "
          f"{min(b for _, b in shares.values() if b is not None):.2f} .. "
          f"{max(b for _, b in shares.values() if b is not None):.2f}")
    for cid, (a, b) in shares.items():
        assert a >= QUARTER, (cid, a)
        assert b is None or b >= QUARTER, (cid, b)


def test_sixteen_rows_or_fewer_test_indexing_not_order():
    """With at most 16 rows every split holds one row and the orders coincide (where no NaN stands)."""
    for prec, dtype in se.DTYPES.items():
        slab, stb = se.slab_case(5, (16, 15, 5, 4, 1, 0), 0, 257, dtype)
        G = se.emulate_slab(slab, stb, dtype)
        assert np.all(se.same_bits(se.row_order_sum(slab, stb, dtype), G))


# ---- the fused step of the encode emulator ------------------------------------------------------------------
def test_round_f32_is_one_correct_rounding():
    rng = np.random.RandomState(3)
    # a double is its own exact value: np.float32 of it is one rounding, and so must round_f32 be
    x = np.concatenate([rng.standard_normal(2000) * 10.0 ** rng.uniform(-44, 38, 2000),
                        np.float64(np.float32(rng.standard_normal(200))),  # already float32
                        [2.0 ** -149, 2.0 ** -150 * 1.0000001, 2.0 ** -126, 3.4028235e38, 3.4028236e38, 1e39, -1e39]])
    with np.errstate(over="ignore"):  # the last four overflow on purpose
        for v in x:
            got, want = se.round_f32(fractions.Fraction(float(v))), np.float32(v)
            assert got.dtype == np.float32 and got.view(np.uint32) == want.view(np.uint32), v
    F, one = fractions.Fraction, fractions.Fraction(1)
    ulp = F(1, 2 ** 23)
    assert se.round_f32(one + ulp / 2) == np.float32(1.0)  # a tie: to even, down
    assert se.round_f32(one + 3 * ulp / 2) == np.float32(1.0 + 2.0 ** -22)  # a tie: to even, up
    assert se.round_f32(-(one + ulp / 2)) == np.float32(-1.0)
    assert se.round_f32(one + ulp / 2 + F(1, 2 ** 60)) == np.float32(1.0 + 2.0 ** -23)  # just past the tie
    assert np.float32(np.float64(one + ulp / 2 + F(1, 2 ** 60))) == np.float32(1.0)  # ... where two roundings go down
    assert se.round_f32(F(1, 2 ** 150)) == 0 and se.round_f32(F(3, 2 ** 150)) == np.float32(2.0 ** -148)  # subnormal ties
    assert se.round_f32(F(3, 2 ** 151)) == np.float32(2.0 ** -149)
    big = F(2) ** 128 - F(2) ** 103  # halfway between the largest float32 and 2^128: a tie that overflows
    assert np.isposinf(se.round_f32(big)) and se.round_f32(big - 1) == np.finfo(np.float32).max


def test_fma_rounds_once_and_keeps_the_ieee_special_cases():
    f64, f32 = np.float64, np.float32
    assert se.fma(1 + 2.0 ** -30, 1 - 2.0 ** -30, -1.0, f64) == -2.0 ** -60  # a * b + c unfused is 0
    assert se.fma(f32(1 + 2.0 ** -12), f32(1 - 2.0 ** -12), f32(-1), f32) == f32(-2.0 ** -24)
    for t in (f64, f32):
        mx = np.finfo(t).max
        assert np.isnan(se.fma(0.0, np.inf, 1.0, t)) and np.isnan(se.fma(2.0, np.inf, -np.inf, t))
        assert np.isnan(se.fma(1.0, 2.0, np.nan, t)) and se.fma(-2.0, np.inf, 5.0, t) == -np.inf
        assert se.fma(mx, mx, -np.inf, t) == -np.inf  # the exact product is finite
        assert se.fma(mx, 2.0, -mx, t) == mx  # a rounded product would be inf
        assert np.isposinf(se.fma(mx, 2.0, mx, t))
        z = se.fma(0.0, 5.0, -0.0, t)
        assert z == 0 and not np.signbit(z)  # +0 + -0
        z = se.fma(-0.0, 5.0, -0.0, t)
        assert z == 0 and np.signbit(z)  # -0 + -0
        z = se.fma(3.0, 2.0, -6.0, t)
        assert z == 0 and not np.signbit(z)  # an exact cancellation
        assert se.fma(0.0, 7.0, -3.5, t) == t(-3.5) and se.fma(1.0, 1.0, 1.0, t).dtype == t
    rng = np.random.RandomState(11)
    for _ in range(300):  # fp32 operands: the fp64 a * b + c rounds an exact-enough value once more; compare where safe
        a, b, c = (f32(v) for v in rng.standard_normal(3) * 10.0 ** rng.uniform(-3, 3, 3))
        exact = fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c))
        assert se.fma(a, b, c, f32) == se.round_f32(exact)
        assert abs(float(se.fma(a, b, c, f32)) - float(exact)) <= 2.0 ** -24 * abs(float(exact))


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_encode_emulator_is_within_the_plain_bound(prec):
    """Against the long-double encoding: (terms + 2) (u sum |coef x| + the smallest subnormal) per column, terms =
    rows added + nonzeros (a product in the subnormal range rounds to the subnormal spacing, not relatively)."""
    dtype = se.DTYPES[prec]
    u, tiny = float(np.finfo(dtype).eps) / 2, LD(np.finfo(dtype).smallest_subnormal)
    for sub in (False, True):
        ptr, idx, coef, sb, rows, live = se.encode_tables(sub)
        Gb = se.hostile_slab(np.random.RandomState(7), rows, 257, dtype, live=live)
        G = se.emulate_encode(Gb, ptr, idx, coef, dtype, sb)
        for slot in range(len(ptr) - 1):
            ref, mag, terms, ok = np.zeros(257, LD), np.zeros(257, LD), 0, np.ones(257, bool)
            for k in range(ptr[slot], ptr[slot + 1]):
                p = idx[k]
                blk = Gb[sb[p]:sb[p + 1]] if sub else Gb[p:p + 1]
                a = LD(dtype(coef[k]))
                ok &= np.all(np.isfinite(blk), axis=0)
                with np.errstate(all="ignore"):
                    ref += a * blk.astype(LD).sum(0)
                    mag += abs(a) * np.abs(blk.astype(LD)).sum(0)
                terms += blk.shape[0] + 1
            ok &= np.isfinite(G[slot])
            with np.errstate(all="ignore"):
                err = np.abs(G[slot].astype(LD) - ref)
            assert np.all(err[ok] <= (terms + 2) * (LD(u) * mag[ok] + tiny)), (sub, slot)
            if ptr[slot] == ptr[slot + 1]:
                assert not np.any(G[slot]) and not np.any(np.signbit(G[slot]))  # an empty slot is +0.0
