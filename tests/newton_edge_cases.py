"""Case tables, oracles and emulators of the Newton-CG edge tests (tests/test_newton_edges_gpu.py).  A plain module (no
GPU, no tests): tests/test_newton_edge_cases_cpu.py checks that the tables reach what they claim, measures the constant
of the block-1 bound by the rule of tests/numerics.py, gives the bound teeth and records the NumPy twin's error.

grad_hvp (csrc/kernels/grad_hvp.hip).  Block 1 of a message, u_j = sum_p c_p sum_i w_i q_i x_ij with q = x . v, is held
per column to the bound of hvp_oracle (moved here from tests/test_newton_gpu.py, whose K_HVP = 2 was measured on the
kernel itself).  K_HVP_EDGE follows the rule instead: HvpGradPlan on CPU tensors, the plain same-precision torch path,
reaches at most MEASURED_HVP_EDGE_CPU_RATIO of the k = 1 bound over GRID and both message sets, and K_HVP_EDGE is 8 x
that, rounded up to a power of two.  Block 0 keeps the project's K.

newton_cg_update (csrc/kernels/newton_cg.hip).  The decode is documented as an fma chain in message order; its result
is observable in the state (G0 in a gradient round, the H dir scratch row in a CG round), so emulate_decode and
emulate_affine rebuild both bit for bit from slab_edge_cases.fma.  replay_round is one round of the recurrences of the
kernel's header comment in any NumPy number type; in long double it is the reference of the branch tests, which measure
every vector against the magnitude of the operands it was formed from (SCALE below: max |ref| is no measure where CG
cancels the residual, as it does completely at d = 1).
"""
import numpy as np
import torch
from scipy.special import expit

from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.update import newton_cg_update, newton_state

import block_edge_cases as bc
import numerics as nx
import slab_edge_cases as sl
from numerics import LD, LEAST_SQUARES, LOGISTIC, LOSSES, SQUARED_HINGE

# ---- grad_hvp: the grid ------------------------------------------------------------------------------------
WIDTHS = (1, 37, 256, 257, 512, 513, 1000, 1024)
KINDS = ("naive", "coded")


def grid():
    """[(d, loss, precision)]: all three losses x bc.SCALAR_PRECS at d = 37 and 1000; logistic in fp64 and fp32 at
    every other width; logistic in fp64, fp32 and fp32x64 at the width that leaves 32-row stages."""
    out = [(d, l, p) for d in (37, 1000) for l in LOSSES for p in bc.SCALAR_PRECS]
    out += [(d, LOGISTIC, p) for d in WIDTHS if d not in (37, 1000) for p in ("fp64", "fp32")]
    for p in bc.SCALAR_PRECS:
        case = (bc.leaves_full_stage(get_precision(p)), LOGISTIC, p)
        if case not in out:
            out.append(case)
    return out


GRID = grid()
GRID_IDS = [f"d{d}-{nx.LOSS_IDS[l]}-{p}" for d, l, p in GRID]

MEASURED_HVP_EDGE_CPU_RATIO = 1.02
MEASURED_HVP_EDGE_CPU_CASE = "d37-lsq-fp64 naive message 9 (1.020)"
K_HVP_EDGE = 16  # 8 x MEASURED_HVP_EDGE_CPU_RATIO, rounded up to a power of two (nx.sparse_k_rule)

# (d, precision) -> seed of bc.scalar_inputs where its default 3000 does not do.  d = 512 and d = 1024 in fp32: under the
# default draw the last row of every partition is saturated (w = s (1 - s) below the fp32 bound's Lipschitz term), so
# the dropped-row mutant of tests/test_newton_edge_cases_cpu.py passes in the naive messages under whole tasks.
SEEDS = {(512, "fp32"): 6000, (1024, "fp32"): 6000}
V_SEED = 9000  # + d: the direction's own stream, so that bc.scalar_inputs stays what the sibling tests draw
_directions, _oracles = {}, {}


def inputs(d, prec_name):
    """(sizes, CPU partitions, host views, (beta [ld], its fp64 view)) of bc.scalar_inputs(d, precision, 2): the
    partitions of test_precond_gpu.py, but for SEEDS."""
    sizes, parts, host, betas = bc.scalar_inputs(d, prec_name, 2, SEEDS.get((d, prec_name), 3000))
    return sizes, parts, host, betas[0]


def direction(d, prec_name):
    """(v [ld] accumulator dtype, its fp64 view [d]): randn(d) 10**U(-3, 1) / sqrt(d), zero padding; drawn once per
    (d, precision) and never changed."""
    if (d, prec_name) not in _directions:
        prec, rng = get_precision(prec_name), np.random.RandomState(V_SEED + d)
        v = torch.zeros(prec.ld(d), dtype=prec.acc)
        v[:d] = torch.from_numpy(rng.randn(d) * 10.0 ** rng.uniform(-3.0, 1.0, d) / np.sqrt(d)).to(prec.acc)
        _directions[(d, prec_name)] = (v, v[:d].double().numpy())
    return _directions[(d, prec_name)]


def curvature(loss, z, y):
    """(w = l''(z), its Lipschitz constant in z) in long double."""
    if loss == LOGISTIC:
        s = expit(-(y * z))
        return s * (1 - s), LD(1) / (6 * np.sqrt(LD(3)))
    return (np.full_like(z, 2) if loss == LEAST_SQUARES else np.where(y * z < 1, LD(2), LD(0))), LD(0)


def hvp_oracle(loss, segments, host, bh, vh, prec, k):
    """(u [d], per-column bound [d]) of block 1 of one message in long double; asserts the squared-hinge margin."""
    d = len(bh)
    u, acc, tiny = np.zeros(d, LD), np.zeros(d, LD), np.zeros(d, LD)
    b, v = np.asarray(bh, LD), np.asarray(vh, LD)
    for p, coef in segments:
        X, y = np.asarray(host[p][0], LD), np.asarray(host[p][1], LD)
        z, az, q, aq = X @ b, np.abs(X) @ np.abs(b), X @ v, np.abs(X) @ np.abs(v)
        if loss == LOGISTIC:
            s = expit(-(y * z))
            w, lip = s * (1 - s), LD(1) / (6 * np.sqrt(LD(3)))
        else:
            w, lip = (np.full_like(z, 2) if loss == LEAST_SQUARES else np.where(y * z < 1, LD(2), LD(0))), LD(0)
        if loss == SQUARED_HINGE:
            assert np.all(np.abs(1 - y * z) > nx.K * nx.acc_eps(prec) * az), "a row sits on the squared hinge's jump"
        u += LD(coef) * (X.T @ (w * q))
        acc += abs(coef) * (np.abs(X).T @ (np.abs(w * q) + w * aq + lip * np.abs(q) * az))
        tiny += abs(coef) * np.abs(X).sum(0)
    return u, LD(k * nx.acc_eps(prec)) * acc + LD(nx.acc_tiny(prec)) * tiny


def oracles(d, loss, prec_name, kind):
    """[(gradient, its K bound, product, its k = 1 bound, the bound's k-free tiny term)] per message of
    bc.MESSAGES[kind] at betas[0] and the direction of (d, precision): computed once."""
    key = (d, loss, prec_name, kind)
    if key not in _oracles:
        prec = get_precision(prec_name)
        sizes, _, host, (_, bh) = inputs(d, prec_name)
        vh = direction(d, prec_name)[1]
        _oracles[key] = [nx.oracle_message(loss, m, host, bh, prec) + hvp_oracle(loss, m, host, bh, vh, prec, 1)
                         + (hvp_oracle(loss, m, host, bh, vh, prec, 0)[1],) for m in bc.MESSAGES[kind](len(sizes))]
    return _oracles[key]


def product_bound(ub, tiny, k):
    """hvp_oracle's bound at the constant k from its values at k = 1 and k = 0 (it is affine in k)."""
    return LD(k) * (ub - tiny) + tiny


def check_messages(G, d, loss, prec_name, kind, what, k=None):
    """Block 0 of every message of G [nslots, 2 ld] within nx.K times its bound, block 1 within K_HVP_EDGE (or k)
    times its own, exact zeros in the padding columns of both and in the message that reads only the empty partition.
    Returns the largest share of the block-1 bound reached (err / (k bound))."""
    k = K_HVP_EDGE if k is None else k
    prec = get_precision(prec_name)
    ld = prec.ld(d)
    got = G.double().cpu().numpy().reshape(-1, 2, ld)
    sizes = inputs(d, prec_name)[0]
    msgs, worst = bc.MESSAGES[kind](len(sizes)), 0.0
    for s, (g, gb, u, ub, tiny) in enumerate(oracles(d, loss, prec_name, kind)):
        nx.check_columns(got[s, 0, :d], g, gb, f"{what} {kind} message {s} gradient")
        nx.check_columns(got[s, 1, :d], u, product_bound(ub, tiny, k), f"{what} {kind} message {s} product", k)
        worst = max(worst, nx.column_ratio(got[s, 1, :d], u, product_bound(ub, tiny, k)))
        if all(sizes[p] == 0 for p, _ in msgs[s]):
            assert np.all(got[s] == 0.0), f"{what} {kind} message {s} reads only the empty partition: exact zeros"
    assert np.all(got[:, :, d:] == 0.0), f"{what} {kind}: padding columns of both blocks must be exact zeros"
    return worst


# ---- grad_hvp: mutants of the block-1 reference ------------------------------------------------------------
MUTANTS = ("drop_last_row", "curvature_at_q", "previous_q", "no_weight", "beta_for_v")


def changes_the_mathematics(mutant, loss):
    """Least squares has the constant w = 2: its curvature is the same wherever it is taken."""
    return not (mutant == "curvature_at_q" and loss == LEAST_SQUARES)


def block1(loss, segments, host, bh, vh, mutant=None, task_rows=bc.WHOLE_TASKS):
    """u [d] of one message in long double, written out by rows; ``mutant`` names one wrong kernel:
    the last row of every task of ``task_rows`` rows dropped, the curvature taken at q instead of z, q of the previous
    row of the partition (0 for the first) used for the current one, the weight w left out, beta in place of v."""
    assert mutant is None or mutant in MUTANTS
    b, v = np.asarray(bh, LD), np.asarray(vh, LD)
    u = np.zeros(len(bh), LD)
    for p, coef in segments:
        X, y = np.asarray(host[p][0], LD), np.asarray(host[p][1], LD)
        n = X.shape[0]
        z, q = X @ b, X @ (b if mutant == "beta_for_v" else v)
        if mutant == "previous_q":
            q = np.concatenate([np.zeros(min(n, 1), LD), q[:-1]])
        w = curvature(loss, q if mutant == "curvature_at_q" else z, y)[0]
        if mutant == "no_weight":
            w = np.ones_like(z)
        keep = np.ones(n, bool)
        if mutant == "drop_last_row":
            keep[[min(n, r0 + task_rows) - 1 for r0 in range(0, n, task_rows)]] = False
        u += LD(coef) * (X[keep].T @ (w * q)[keep])
    return u


# ---- grad_hvp: exact scaling with the direction ------------------------------------------------------------
SCALING_MARGIN = 2.0 ** 40


def scaling_is_exact(loss, host, bh, vh, prec):
    """The condition on the inputs under which block 1 scales bitwise with a power of two of v (w in {0, 2}): no
    nonzero product |x_ik v_k| or |w q x_ij| of the long-double reference lies within 2^40 of the accumulator's
    smallest normal or largest finite value, so neither 2^8 nor 2^-8 moves a rounding."""
    fi = np.finfo(np.float64 if prec.acc == torch.float64 else np.float32)
    lo, hi = LD(fi.tiny) * LD(SCALING_MARGIN), LD(fi.max) / LD(SCALING_MARGIN)
    b, v = np.asarray(bh, LD), np.asarray(vh, LD)
    for X, y in host.values():
        X, y = np.asarray(X, LD), np.asarray(y, LD)
        w = curvature(loss, X @ b, y)[0]
        for prod in (np.abs(X * v[None, :]), np.abs((w * (X @ v))[:, None] * X)):
            nz = prod[prod != 0]
            if nz.size and not (nz.min() > lo and nz.max() < hi):
                return False
    return True


# ---- newton_cg_update: hostile messages and the decode's emulator ------------------------------------------
UPDATE_NMSG = (1, 7, 8, 9, 16, 17, 127, 128)  # a batch short of / exactly / one past one and two batches of eight; MAX_MSGS
UPDATE_SHAPES = ((1, 1), (6, 5), (256, 256), (257, 256), (302, 301), (1024, 1024), (1024, 1000))  # (ld, d)
UPDATE_DTYPES = {"fp64": (np.float64, torch.float64), "fp32": (np.float32, torch.float32)}
ETA, GS, L2C = 0.01, 0.1, 0.1  # the round's coefficients: eta, gs = 1 / n, l2c = 2 alpha


def special_columns(d):
    """{kind: column}: a column of -0.0 and a column of denormals in every message (d >= 3; a narrower model has
    only the scattered ones)."""
    return {"neg_zero": d // 2, "denormal": d - 1} if d >= 3 else {}


def hostile_messages(rng, nmsg, ld, d, dtype, pad=0.0):
    """[nmsg][2 ld] of ``dtype``: randn 10**U(-6, 6) (twelve decades), 5 % exact zeros (a fifth of them -0.0), 3 %
    denormals, the dedicated columns of special_columns in both blocks, ``pad`` in the columns d .. ld of both."""
    fi = np.finfo(dtype)
    M = (rng.standard_normal((nmsg, 2, ld)) * 10.0 ** rng.uniform(-6, 6, (nmsg, 2, ld))).astype(dtype)
    z = rng.uniform(size=M.shape)
    den = (rng.randint(-7, 8, M.shape) * float(fi.smallest_subnormal)).astype(dtype)
    M[z < 0.05] = 0.0
    M[z < 0.01] = -0.0
    M[z > 0.97] = den[z > 0.97]
    for kind, c in special_columns(d).items():
        M[:, :, c] = -0.0 if kind == "neg_zero" else den[:, :, c]
    M[:, :, d:] = pad
    return M.reshape(nmsg, 2 * ld)


def hostile_model(rng, ld, d):
    """beta [2 ld] fp64: randn in the live columns of block 0, an exact 0.0 under the -0.0 column (the sign of G = +-0
    then shows), zeros elsewhere."""
    beta = np.zeros(2 * ld)
    beta[:d] = rng.standard_normal(d)
    if "neg_zero" in special_columns(d):
        beta[special_columns(d)["neg_zero"]] = 0.0
    return beta


def emulate_decode(msgs, coefs, ld, d, block):
    """The decode of one block as documented: from 0, s = fma(c_m, double(msg_m[block ld + c]), s) over the messages
    in order, every column by itself."""
    s = np.zeros(d, np.float64)
    for m, c in zip(msgs, coefs):
        col = np.asarray(m[block * ld: block * ld + d]).astype(np.float64)  # a float32 widens exactly
        s = np.array([sl.fma(c, col[j], s[j], np.float64) for j in range(d)], np.float64)
    return s


def emulate_affine(gs, dec, l2c, vec):
    """fma(gs, dec, l2c * vec): G from (g, beta) in a gradient round, H dir from (u, dir) in a CG round."""
    with np.errstate(all="ignore"):
        prod = np.float64(l2c) * np.asarray(vec, np.float64)
    return np.array([sl.fma(gs, dec[j], prod[j], np.float64) for j in range(len(dec))], np.float64)


# ---- newton_cg_update: one round in any number type --------------------------------------------------------
VECTORS = ("beta", "x", "r", "dir", "G0")


def replay_round(T, msgs, coefs, beta, st, sc, ph, d, ld, J, eta, gs, l2c, xi, tau):
    """One round of the header comment of newton_cg.hip in the number type T, full-length vectors, from the state
    (st [5][ld], sc [2], ph [4]) before it.  Returns ({name: vector [d]} over VECTORS after the round, the wire
    direction [d], {name: SCALE}, [rs, g0norm2], phase [4]).

    SCALE of a vector the round formed is the largest magnitude its sum could have reached, max_j sum |terms_j|, the
    decoded sums counted by sum_m |c_m msg_m| (a forward error is proportional to that, not to what is left after
    cancellation); a vector the round did not touch has no scale and must not move at all."""
    b = np.asarray(beta[:d], T)
    x, r, dr, G0 = (np.array(st[k, :d], dtype=T) for k in range(4))
    dec, mag = np.zeros((2, d), T), np.zeros((2, d), T)
    for m, c in zip(msgs, coefs):
        mm = np.asarray(m, T).reshape(2, ld)[:, :d]
        dec += T(c) * mm
        mag += np.abs(T(c) * mm)
    cg = int(ph[0]) == 1  # anything else: a gradient round
    inner, outer = (int(ph[1]) if cg else 0), int(ph[3])
    rs, g0n = T(sc[0]), T(sc[1])
    gs, l2c, eta, tau, xi = T(gs), T(l2c), T(eta), T(tau), T(xi)
    scale = {}
    top = lambda v: float(np.max(np.abs(v[~np.isnan(v)]), initial=0.0))  # noqa: E731
    ok = lambda v: bool(np.isfinite(v) and v > 0)  # noqa: E731
    with np.errstate(all="ignore"):
        if not cg:
            G0 = gs * dec[0] + l2c * b
            scale["G0"] = top(np.abs(gs) * mag[0] + np.abs(l2c * b))
            s1 = G0 @ G0
            if ok(s1):
                mode, x, r, dr, rs, g0n = 0, np.zeros(d, T), -G0, -G0, s1, s1
                scale["x"] = scale["r"] = scale["dir"] = scale["G0"]
            else:
                mode = 6
        else:
            Hv, aHv = gs * dec[1] + l2c * dr, np.abs(gs) * mag[1] + np.abs(l2c * dr)
            kappa = dr @ Hv
            if not ok(kappa):
                mode = 5 if inner == 0 else 4
            else:
                a = rs / kappa
                scale["x"], scale["r"] = top(np.abs(x) + np.abs(a * dr)), top(np.abs(r) + np.abs(a) * aHv)
                x, r = x + a * dr, r - a * Hv
                rs2, inner = r @ r, inner + 1
                mode = 2 if not rs2 > xi * xi * g0n else 3 if inner >= J else 1
                if mode == 1:
                    scale["dir"] = top(np.abs(r) + np.abs((rs2 / rs) * dr))
                    dr, rs = r + (rs2 / rs) * dr, rs2
        cont = mode in (0, 1)
        if cont:
            nb, wire = b, dr
        else:
            step = -eta * G0 if mode >= 5 else tau * x
            nb, wire = b + step, np.zeros(d, T)
            scale["beta"] = top(np.abs(b) + np.abs(step))
    return (dict(beta=nb, x=x, r=r, dir=dr, G0=G0), wire, scale, [rs, g0n],
            [int(cont), inner, mode, outer + int(not cont)])


# ---- newton_cg_update: the script of rounds ----------------------------------------------------------------
# (xi, what is wrong with the round's messages, at which CG step): one outer iteration each, as tests/test_newton_gpu.py
SCRIPT = [(1e-9, None, 0),     # the J cap: start, continue, continue, step-cap
          (0.9, None, 0),      # the tolerance: start, step-tolerance
          (1e-9, "neg", 0),    # kappa <= 0 on the first CG round: the GD step from G0
          (1e-9, "neg", 1),    # kappa <= 0 on a later one: the x held
          (1e-9, "nan", -1)]   # a NaN message in the gradient round: the GD step
SCRIPT_SHAPES = ((1, 1), (256, 256), (1024, 1024), (302, 301))  # (ld, d), each with MAX_MSGS messages
SCRIPT_J, SCRIPT_TAU = 3, 0.9
# The largest |x - ref| / SCALE the NumPy twin of ops/update.py reaches on each vector over SCRIPT at SCRIPT_SHAPES
# with fp64 and fp32 messages, in units of 2^-53, and where (tests/test_newton_edge_cases_cpu.py
# test_twin_follows_the_replay_through_every_branch pins them: not exceeded, reached within 25 %).  The kernel's bound on a vector is
# BOUND_FACTOR x max(this, FLOOR) with the two constants of tests/test_lbfgs_cpu.py.
TWIN_REL = {"beta": 2.54, "x": 3.09, "r": 3.64, "dir": 25.7, "G0": 3.64}
TWIN_REL_CASES = {"beta": "ld=302 d=301 fp64 round 5 mode 2", "x": "ld=302 d=301 fp64 round 5 mode 2",
                  "r": "ld=302 d=301 fp32 round 6 mode 0", "dir": "ld=1024 d=1024 fp32 round 2 mode 1",
                  "G0": "ld=302 d=301 fp32 round 6 mode 0"}


def history_row(ld, d, dev):
    """A row of the history as an update kernel meets it: NaN where the kernel must write (the live columns of block 0
    and all of block 1), the zeros of the zero-initialised history in the padding columns of block 0, which no update
    kernel of the project writes."""
    hist = torch.full((2 * ld,), float("nan"), dtype=torch.float64, device=dev)
    hist[d:ld] = 0.0
    return hist


def run_script(ld, d, nmsg, mdt, dev):
    """SCRIPT through ops.update.newton_cg_update on ``dev`` (the kernel on a GPU, the NumPy twin on the CPU): a
    diagonal quadratic (loss Hessian A in [1, 4], a new linear term every outer iteration), the round's [g ; u]
    split over nmsg coded messages of type mdt.  Every round is replayed in long double from the state the device
    held before it; the phase words must agree, untouched vectors must not move, beta_w and hist must be the casts
    of beta and the direction.  Returns [(round, mode, {name: |x - ref| / SCALE})] and the modes seen."""
    rng = np.random.RandomState(1000 * ld + nmsg)
    A = rng.uniform(1.0, 4.0, d)
    beta = torch.from_numpy(np.pad(rng.randn(d), (0, 2 * ld - d))).to(dev)
    state, scal, phase = newton_state(ld, dev)
    hist = history_row(ld, d, dev)
    bw = torch.full((2 * ld,), float("nan"), dtype=mdt, device=dev)
    coefs = rng.uniform(0.5, 1.5, nmsg) * np.where(np.arange(nmsg) % 3 == 1, -0.5, 1.0)
    share = rng.uniform(0.5, 1.5, nmsg)
    share /= coefs.dot(share)
    out, seen, i = [], set(), 0
    for xi, fault, at in SCRIPT:
        outer, c = int(phase[3]), rng.randn(d)
        while int(phase[3]) == outer:
            b0, st0, sc0, ph0 = beta.cpu().numpy().copy(), state.cpu().numpy().copy(), scal.cpu().numpy().copy(), phase.tolist()
            cg = ph0[0] == 1
            sign = -1.0 if fault == "neg" and cg and ph0[1] == at else 1.0
            full = np.zeros((2, ld))
            full[0, :d], full[1, :d] = A * b0[:d] - c, sign * A * (st0[2, :d] if cg else 0.0)
            msgs = [torch.from_numpy(s * full.ravel()).to(mdt) for s in share]
            if fault == "nan":
                msgs[-1][d // 2] = float("nan")
            newton_cg_update([m.to(dev) for m in msgs], coefs, beta, state, scal, phase, ld, d, SCRIPT_J, ETA, GS, L2C, xi,
                             SCRIPT_TAU, hist=hist, beta_w=bw)
            ref, wire, scale, _, ph = replay_round(LD, [m.double().numpy() for m in msgs], coefs, b0, st0, sc0, ph0, d, ld,
                                                   SCRIPT_J, ETA, GS, L2C, xi, SCRIPT_TAU)
            assert phase.tolist() == ph, f"round {i}: phase {phase.tolist()}, the replay's {ph}"
            b, st = beta.cpu().numpy(), state.cpu().numpy()
            got, before = dict(beta=b[:d], x=st[0, :d], r=st[1, :d], dir=st[2, :d], G0=st[3, :d]), \
                dict(beta=b0[:d], x=st0[0, :d], r=st0[1, :d], dir=st0[2, :d], G0=st0[3, :d])
            errs = {}
            for name in VECTORS:
                if name not in scale:
                    assert np.all(sl.same_bits(got[name], before[name])), f"round {i}: {name} moved in mode {ph[2]}"
                    continue
                nan = np.isnan(np.asarray(ref[name], np.float64))
                assert np.array_equal(np.isnan(got[name]), nan) and nan.sum() == (fault == "nan"), f"round {i}: {name}"
                err = np.abs(np.where(nan, 0, got[name]).astype(LD) - np.where(nan, 0, ref[name]))
                errs[name] = float(err.max() / LD(scale[name])) if err.max() else 0.0
            h, w = hist.cpu().numpy(), bw.cpu().numpy()
            shown = st[2, :d] if ph[0] == 1 else np.zeros(d)
            assert np.all(sl.same_bits(h[:d], b[:d])) and np.all(h[d:] == 0) and np.all(b[d:] == 0), f"round {i}: hist"
            assert np.all(sl.same_bits(w[:d], b[:d].astype(w.dtype))) and np.all(w[d:ld] == 0) and np.all(w[ld + d:] == 0) \
                and np.all(sl.same_bits(w[ld:ld + d], shown.astype(w.dtype))), f"round {i}: the wire model"
            assert np.all(st[:4, d:] == 0), f"round {i}: padding columns of the state"
            seen.add(ph[2])
            out.append((i, ph[2], errs))
            i += 1
    return out, seen
