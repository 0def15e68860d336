"""Order emulators, hostile slabs and case tables of tests/test_slab_edges_gpu.py.  A plain module (no GPU, no tests,
nothing of the package): tests/test_slab_edge_cases_cpu.py holds the tables to the selectors of slab_reduce.h and gives
the emulators teeth.

The emulators are written from the comments of csrc/kernels/slab_reduce.hip and encode.hip, in NumPy scalars and
arrays of the accumulator type, one IEEE operation per step:

* a message of rows tb .. te - 1 is cut into SPLITS = 16 splits of per = ceil(n / 16) rows, split k covering
  t0 = tb + k per .. min(te, t0 + per) (nothing when t0 is past the end); a split keeps four sums, row t going to sum
  (t - t0) mod 4 in row order, folded (a0 + a1) + (a2 + a3); the 16 split sums are added in order from 0;
* an encoded message is s = fma(A(coef), g, s) over its nonzeros in order from 0, g a row of Gb or, with sub_begin,
  the sum of a partition's rows added in row order from 0.
"""
import collections
import fractions
import math

import numpy as np

SPLITS = 16          # launchers.h kSlabSplits
PUT_ONE_ELEMS = 4096  # slab_reduce.h kPutOneElems
PUT_ONE_SLOTS = 16    # slab_reduce.h kPutOneSlots
MAX_MSGS = 128        # launchers.h kMaxMsgs
DTYPES = {"fp64": np.float64, "fp32": np.float32}


# ---- the slab reduction's order ----------------------------------------------------------------------------
def ceil_per(n):
    return -(-n // SPLITS)


def emulate_slab(slab, stb, dtype, per_of=ceil_per):
    """G [len(stb) - 1][ld] of the documented order; ``per_of`` is there for the mutants of the CPU test."""
    slab = np.asarray(slab)
    assert slab.dtype == dtype and slab.ndim == 2
    ld = slab.shape[1]
    G = np.zeros((len(stb) - 1, ld), dtype)
    with np.errstate(all="ignore"):
        for s in range(len(stb) - 1):
            tb, te = int(stb[s]), int(stb[s + 1])
            per = per_of(te - tb)
            total = np.zeros(ld, dtype)
            for k in range(SPLITS):
                t0 = tb + k * per
                t1 = min(te, t0 + per)
                acc = [np.zeros(ld, dtype) for _ in range(4)]
                for t in range(t0, t1):
                    acc[(t - t0) % 4] = acc[(t - t0) % 4] + slab[t]
                total = total + ((acc[0] + acc[1]) + (acc[2] + acc[3]))
            G[s] = total
    return G


def row_order_sum(slab, stb, dtype):
    """The first mutant: every message's rows added one after the other."""
    G = np.zeros((len(stb) - 1, slab.shape[1]), dtype)
    with np.errstate(all="ignore"):
        for s in range(len(stb) - 1):
            for t in range(int(stb[s]), int(stb[s + 1])):
                G[s] = G[s] + slab[t]
    return G


def same_bits(got, want):
    """Elementwise: the same bits where ``want`` is a number, a NaN where it is one."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    u = np.uint64 if want.dtype == np.float64 else np.uint32
    nan = np.isnan(want)
    return np.where(nan, np.isnan(got), got.view(u) == want.view(u))


# ---- the encoding's order ----------------------------------------------------------------------------------
def round_f32(q):
    """The float32 nearest to the rational q, ties to even, with subnormals and overflow (q != 0)."""
    sign, q = (-1.0, -q) if q < 0 else (1.0, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()  # 2^(e-1) < q < 2^(e+1)
    if q < fractions.Fraction(2) ** e:
        e -= 1
    e = max(e, -126)  # below the normal range the spacing stays 2^-149
    scaled = q / fractions.Fraction(2) ** (e - 23)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > fractions.Fraction(1, 2) or (rem == fractions.Fraction(1, 2) and n % 2):
        n += 1
    if n * fractions.Fraction(2) ** (e - 23) >= fractions.Fraction(2) ** 128:
        return np.float32(sign * math.inf)
    return np.float32(sign * math.ldexp(n, e - 23))  # n < 2^25 and the result is a float32: exact


def round_f64(q):
    try:
        return np.float64(float(q))  # int / int is correctly rounded, subnormals included
    except OverflowError:
        return np.float64(math.inf if q > 0 else -math.inf)


def fma(a, g, s, dtype):
    """fma(a, g, s) of three values of ``dtype``: exact product and sum, one rounding."""
    a, g, s = dtype(a), dtype(g), dtype(s)
    with np.errstate(all="ignore"):
        if np.isnan(s) or not (np.isfinite(a) and np.isfinite(g)):
            return dtype(dtype(a * g) + s)  # a NaN or an infinite product: nothing is rounded
        if np.isinf(s):
            return s  # the exact product is finite, whatever a rounded one would be
        if a == 0 or g == 0:
            return dtype(dtype(a * g) + s)  # a signed zero plus s: exact
    q = fractions.Fraction(float(a)) * fractions.Fraction(float(g)) + fractions.Fraction(float(s))
    if q == 0:
        return dtype(0.0)  # a nonzero product cancelled exactly: +0.0 under round-to-nearest
    return round_f32(q) if dtype == np.float32 else round_f64(q)


def emulate_encode(Gb, ptr, idx, coef, dtype, sub_begin=None):
    """G [len(ptr) - 1][ld] of encode_messages; with ``sub_begin`` idx names partitions of row blocks of Gb."""
    Gb = np.asarray(Gb)
    assert Gb.dtype == dtype
    ld = Gb.shape[1]
    G = np.zeros((len(ptr) - 1, ld), dtype)
    with np.errstate(all="ignore"):
        for slot in range(len(ptr) - 1):
            s = np.zeros(ld, dtype)
            for k in range(int(ptr[slot]), int(ptr[slot + 1])):
                p = int(idx[k])
                if sub_begin is None:
                    g = Gb[p]
                else:
                    g = np.zeros(ld, dtype)
                    for q in range(int(sub_begin[p]), int(sub_begin[p + 1])):
                        g = g + Gb[q]
                a = dtype(coef[k])
                s = np.array([fma(a, g[c], s[c], dtype) for c in range(ld)], dtype)
            G[slot] = s
    return G


# ---- hostile inputs ----------------------------------------------------------------------------------------
SPECIALS = ("neg_zero", "pairs", "denormal", "inf", "inf_minus_inf", "nan", "overflow")


def special_columns(ld):
    """{kind: column} of the dedicated columns: spread over the width with the last column among them; a slab
    narrower than 16 columns keeps column 0 plain and gives the others away in order."""
    if ld >= 16:
        cols = [round(i * (ld - 1) / 6) for i in range(7)]
    else:
        cols = list(range(1, min(ld, 8)))
    return dict(zip(SPECIALS, cols))


def hostile_slab(rng, rows, ld, dtype, live=None):
    """[rows][ld]: randn * 10**U(-6, 6), 5 % exact zeros (a fifth of them -0.0), the dedicated columns of
    special_columns, and NaN in every row outside live = (first, end) (default: all rows live)."""
    lo, hi = live if live is not None else (0, rows)
    S = (rng.standard_normal((rows, ld)) * 10.0 ** rng.uniform(-6, 6, (rows, ld))).astype(dtype)
    z = rng.uniform(size=(rows, ld))
    S[z < 0.05] = 0.0
    S[z < 0.01] = -0.0
    fi = np.finfo(dtype)
    n = hi - lo
    for kind, c in special_columns(ld).items():
        if kind == "neg_zero":
            S[:, c] = -0.0
        elif kind == "pairs":
            x = S[lo:hi:2, c].copy()
            S[lo:hi:2, c] = x
            S[lo + 1:hi:2, c] = -x[:len(range(lo + 1, hi, 2))]
        elif kind == "denormal":
            S[:, c] = (rng.randint(-7, 8, rows) * float(fi.smallest_subnormal)).astype(dtype)
        elif n >= 1:
            r = lo + rng.choice(n, size=min(2, n), replace=False)
            if kind == "inf":
                S[r[0], c] = np.inf
            elif kind == "nan":
                S[r[0], c] = np.nan
            elif kind == "inf_minus_inf":
                S[r[0], c], S[r[-1], c] = np.inf, -np.inf
            else:  # two finite values whose sum overflows, next to each other so that one message holds both
                a = lo + rng.randint(max(1, n - 1))
                S[a:min(hi, a + 2), c] = fi.max * dtype(0.75)
    S[:lo] = np.nan
    S[hi:] = np.nan
    return S


# ---- case tables -------------------------------------------------------------------------------------------
TASKS = (0, 1, 4, 5, 15, 16, 17, 33, 65, 127, 128, 129, 145, 272)
WIDTHS = (1, 63, 64, 65, 255, 256, 257, 1000, 1024)
# every task count in one launch, short and empty messages between long ones
ALL_TASKS = (17, 0, 1, 129, 0, 33, 272, 4, 127, 5, 145, 15, 128, 16, 65)
LAYOUTS = ((17, 0, 1, 129, 0, 33), (5, 272, 0, 16, 17), (0, 0, 65, 1), (145, 15, 128, 4), (17,), (0,), (1,))
LEAD_LAYOUT = 1  # this layout starts at slab row LEAD (stb[0] > 0)
LEAD, TAIL = 3, 2  # NaN rows in front of the first message (where a case has them) and behind the last
PUT_COUNTS = (17, 0, 1, 129, 33, 16, 5)  # tasks of slot i of a put case: PUT_COUNTS[i % 7]

ReduceCase = collections.namedtuple("ReduceCase", "id counts lead ld")
PutCase = collections.namedtuple("PutCase", "id nslots ld kernel")
UpdateCase = collections.namedtuple("UpdateCase", "id nslots nmsg ld d rule")
EncodeCase = collections.namedtuple("EncodeCase", "id ld sub")


def stb_of(counts, lead=0):
    return np.concatenate([[lead], lead + np.cumsum(counts)]).astype(np.int32)


def slab_case(seed, counts, lead, ld, dtype):
    """(slab with TAIL NaN rows behind the last message, stb) of a layout."""
    stb = stb_of(counts, lead)
    rng = np.random.RandomState(seed)
    return hostile_slab(rng, int(stb[-1]) + TAIL, ld, dtype, live=(lead, int(stb[-1]))), stb


def reduce_cases():
    """Every task count at every width in one launch (at 257 columns behind LEAD NaN rows), and the layouts at 65
    and 1000 columns."""
    out = [ReduceCase(f"all-ld{ld}", ALL_TASKS, LEAD if ld == 257 else 0, ld) for ld in WIDTHS]
    for ld in (65, 1000):
        for i, counts in enumerate(LAYOUTS):
            out.append(ReduceCase("n" + "_".join(map(str, counts)) + f"-ld{ld}", counts, LEAD if i == LEAD_LAYOUT else 0,
                                  ld))
    return out


def put_kernel(nslots, ld, mode):
    """The kernel slab_reduce_launch gives a put of this shape in this mode."""
    if mode == 1:
        return "slab_reduce_fused_put"
    return "slab_reduce_final_put1" if nslots <= PUT_ONE_SLOTS and nslots * ld <= PUT_ONE_ELEMS else "slab_reduce_final_put"


def put_cases():
    """(nslots, ld) on and one past each selector of the one-block put, element counts whose last pair of the
    one-block put is single (3 x 1000, 7 x 413, 1 x 1), and the many-block put on its 256-column boundary."""
    one, many = "slab_reduce_final_put1", "slab_reduce_final_put"
    rows = PUT_ONE_ELEMS // 1024
    shapes = [(rows, 1024, one), (rows + 1, 1024, many), (PUT_ONE_SLOTS, 256, one), (PUT_ONE_SLOTS + 1, 8, many),
              (3, 1000, one), (7, 413, one), (1, 1, one), (15, 65, one), (17, 255, many), (17, 257, many)]
    return [PutCase(f"{n}x{ld}", n, ld, k) for n, ld, k in shapes]


def last_pair_single(nslots, ld, threads=1024):
    """slab_reduce_final_put1 takes elements e and e + threads together, 2 * threads a step: some thread's last e has
    no partner unless the steps divide the element count."""
    return (nslots * ld) % (2 * threads) != 0


UPDATE_NSLOTS = (1, 15, 16, 17, 33, 129)  # 129 in fp64 only: the first count past 64 KiB of LDS
UPDATE_NMSG = (1, 8, 9, MAX_MSGS)
UPDATE_TASKS = (17, 0, 1, 33, 5)  # tasks of slot i: UPDATE_TASKS[i % 5]


def update_cases(prec):
    out = []
    widths = ((65, 64), (257, 255), (130, 1), (64, 64))  # (ld, d): d < ld but in the last, which has no padding
    for i, nslots in enumerate(UPDATE_NSLOTS):
        if nslots == 129 and prec != "fp64":
            continue
        for j, nmsg in enumerate(UPDATE_NMSG):
            ld, d = widths[(i + j) % 4]
            rule = (i + j // 2) % 2
            out.append(UpdateCase(f"s{nslots}-m{nmsg}-ld{ld}-d{d}-{'AGD' if rule else 'GD'}", nslots, nmsg, ld, d, rule))
    return out


def slot_list(nslots, nmsg):
    """Backwards over the slots without the middle one, cycled to nmsg entries, the last repeating the first."""
    order = [s for s in reversed(range(nslots)) if nslots == 1 or s != nslots // 2]
    slots = [order[m % len(order)] for m in range(nmsg)]
    if nmsg > 1:
        slots[-1] = slots[0]
    return slots


def update_coefs(rng, nmsg):
    coefs = list(rng.standard_normal(nmsg))
    if nmsg > 1:
        coefs[nmsg // 2] = 0.0
    coefs[-1] = -abs(coefs[-1]) - 0.25
    return coefs


ENCODE_WIDTHS = (1, 255, 256, 257)
ENCODE_BLOCKS = (0, 1, 15, 16, 17, 33)  # row blocks of partition p (the sub_begin mode)
# nonzeros (partition, coefficient) of every message: none, one to four, a coefficient of exactly 0.0, negative ones,
# the partition without row blocks
ENCODE_MSGS = ((), ((2, 1.0),), ((0, 1.0),), ((5, -0.7), (3, 0.0)), ((1, 0.5), (4, 2.0), (0, -1.0)),
               ((5, 1.0), (2, -1.0), (3, 0.3), (4, 1e-3)), ())


def encode_cases():
    return [EncodeCase(f"ld{ld}-{'sub' if sub else 'rows'}", ld, sub) for ld in ENCODE_WIDTHS for sub in (False, True)]


def encode_tables(sub):
    """(ptr, idx, coef, sub_begin or None, rows of Gb, (first, end) of its live rows).  Without sub_begin partition p
    is row LEAD + p of Gb."""
    ptr, idx, coef = [0], [], []
    for m in ENCODE_MSGS:
        for p, c in m:
            idx.append(p if sub else LEAD + p)
            coef.append(c)
        ptr.append(len(idx))
    if sub:
        sb = stb_of(ENCODE_BLOCKS, LEAD)
        live = (LEAD, int(sb[-1]))
    else:
        sb, live = None, (LEAD, LEAD + len(ENCODE_BLOCKS))
    return (np.asarray(ptr, np.int32), np.asarray(idx, np.int32), np.asarray(coef, np.float64), sb, live[1] + TAIL, live)
