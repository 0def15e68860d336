"""Master decode-combine + GD/AGD update (K5/K7/K8; csrc/kernels/update.hip).

``combine_update`` computes g = sum_m coef_m * msg_m and applies the reference update
(ref src/naive.py:112-122) to the fp64 master state in one launch, also writing the
betaset history row and the worker-precision copy of the new beta.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .._ext import native


def combine_update(msgs: Sequence[torch.Tensor], coefs: Sequence[float], beta: torch.Tensor, u: torch.Tensor,
                   d: int, decay: float, gm: float, l2: float, theta: float, rule: int,
                   hist: Optional[torch.Tensor] = None, beta_w: Optional[torch.Tensor] = None,
                   g_out: Optional[torch.Tensor] = None) -> None:
    if beta.is_cuda:
        C = native()
        if len(msgs) > C.MAX_MSGS:
            raise ValueError(f"at most {C.MAX_MSGS} messages per combine")
        C.combine_update(list(msgs), [float(c) for c in coefs], beta, u, hist, beta_w, g_out, int(d),
                         float(decay), float(gm), float(l2), float(theta), int(rule))
        return
    _update_torch(msgs, coefs, beta, u, d, decay, gm, l2, theta, rule, hist, beta_w, g_out)


def combine_update_blocks(msgs: Sequence[torch.Tensor], coefs: Sequence[float], beta: torch.Tensor, u: torch.Tensor,
                          block_ld: int, d_x: int, decay: Sequence[float], gm: Sequence[float], l2: Sequence[float],
                          theta: float, rule: int, hist: Optional[torch.Tensor] = None,
                          beta_w: Optional[torch.Tensor] = None, g_out: Optional[torch.Tensor] = None) -> None:
    """combine_update for a model of ``len(decay)`` blocks of ``block_ld`` columns (``d_x`` of them data) with their
    own (decay, gm, l2): a multi-model run (ops/multimodel.py).  Block k gets exactly what ``combine_update`` gives
    that block alone; padding columns stay zero."""
    _update_blocked("combine_update_blocks", msgs, coefs, beta, u, block_ld, d_x, decay, gm, l2, None, theta, rule,
                    hist, beta_w, g_out)


def combine_update_prox(msgs: Sequence[torch.Tensor], coefs: Sequence[float], beta: torch.Tensor, u: torch.Tensor,
                        block_ld: int, d_x: int, decay: Sequence[float], gm: Sequence[float], l2: Sequence[float],
                        thr: Sequence[float], theta: float, rule: int, hist: Optional[torch.Tensor] = None,
                        beta_w: Optional[torch.Tensor] = None, g_out: Optional[torch.Tensor] = None) -> None:
    """combine_update_blocks followed by the proximal step of an L1 penalty: block k's new beta is
    ``S_t(x) = |x| <= t ? +0.0 : x - copysign(t, x)`` of the updated x with t = ``thr[k]``, and the AGD momentum is
    formed from the thresholded beta.  A single model is one block (``block_ld = ld``, ``d_x = d``)."""
    _update_blocked("combine_update_prox", msgs, coefs, beta, u, block_ld, d_x, decay, gm, l2, thr, theta, rule,
                    hist, beta_w, g_out)


def combine_update_precond(msgs: Sequence[torch.Tensor], coefs: Sequence[float], beta: torch.Tensor, u: torch.Tensor,
                           ld_x: int, d_x: int, eta: float, gs: float, l2c: float, damp: float, theta: float,
                           rule: int, hist: Optional[torch.Tensor] = None,
                           beta_w: Optional[torch.Tensor] = None) -> None:
    """The Jacobi-preconditioned (diagonal-Newton) combine + update of a ``[2][ld_x]`` model (ops/precond.py): block 0
    of the messages decodes to the gradient g, block 1 to the curvature diagonal h, and per data column
    ``P = gs * max(h, 0) + l2c + damp``, ``step = eta * (gs * g + l2c * beta) / P``; GD ``beta -= step``, AGD
    ``beta' = (1 - theta) beta + theta u - step`` with the usual momentum.  Block 1 of beta_w and hist is written as
    zeros.  Native on GPU tensors, torch on CPU tensors."""
    ld_x, d_x, damp = int(ld_x), int(d_x), float(damp)
    if not (1 <= d_x <= ld_x and beta.numel() == 2 * ld_x and u.numel() == 2 * ld_x):
        raise ValueError(f"combine_update_precond: two blocks of {ld_x} columns do not describe this model")
    if not (damp > 0.0 and damp != float("inf")):
        raise ValueError(f"combine_update_precond: the damping must be finite and > 0, got {damp}")
    if beta.is_cuda:
        C = native()
        if len(msgs) > C.MAX_MSGS:
            raise ValueError(f"at most {C.MAX_MSGS} messages per combine")
        C.combine_update_precond(list(msgs), [float(c) for c in coefs], beta, u, hist, beta_w, ld_x, d_x, float(eta),
                                 float(gs), float(l2c), damp, float(theta), int(rule))
        return
    g = torch.zeros(d_x, dtype=torch.float64)
    h = torch.zeros(d_x, dtype=torch.float64)
    for m, c in zip(msgs, coefs):
        g += float(c) * m[:d_x].double()
        h += float(c) * m[ld_x: ld_x + d_x].double()
    b = beta[:d_x]
    P = gs * torch.where(h < 0, torch.zeros_like(h), h) + (l2c + damp)
    step = eta * (gs * g + l2c * b) / P
    if rule == 0:
        nb = b - step
    else:
        nb = (1.0 - theta) * b + theta * u[:d_x] - step
        u[:d_x] = b + (nb - b) * (1.0 / theta)
    beta[:d_x] = nb
    if hist is not None:
        hist[:d_x] = nb
        hist[ld_x:] = 0.0
    if beta_w is not None:
        beta_w.zero_()
        beta_w[:d_x] = nb.to(beta_w.dtype)


LBFGS_MAX_MEMORY = 7  # 2 * 7 + 1 columns of V = [s_1..s_k, y_1..y_k, G] fill one 16-wide MFMA tile (lbfgs.hip)


def lbfgs_state(memory: int, ld: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """A fresh L-BFGS state for a model of ``ld`` elements: ``state`` fp64 ``[2 * memory + 3, ld]`` (the ring's s rows,
    its y rows, beta_prev, G_prev and a row that keeps the last step's direction) and ``ring`` int32 ``[4]`` (head,
    count, 1 once a round has been seen, the last step's mode: 0 quasi-Newton, 1 GD without a pair, 2 GD and the ring
    emptied).  ``lbfgs_update`` advances both in place."""
    memory = int(memory)
    if not 1 <= memory <= LBFGS_MAX_MEMORY:
        raise ValueError(f"--lbfgs: the memory must be in 1..{LBFGS_MAX_MEMORY}, got {memory}")
    return (torch.zeros((2 * memory + 3, int(ld)), dtype=torch.float64, device=device),
            torch.zeros(4, dtype=torch.int32, device=device))


def lbfgs_pairs(state: torch.Tensor, ring: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(S, Y) of the pairs the state holds, ``[count, ld]`` each, oldest first."""
    memory = (state.shape[0] - 3) // 2
    head, count = (int(x) for x in ring[:2].tolist())
    rows = [(head + j) % memory for j in range(count)]
    return state[rows], state[[memory + r for r in rows]]


def lbfgs_update(msgs: Sequence[torch.Tensor], coefs: Sequence[float], beta: torch.Tensor, state: torch.Tensor,
                 ring: torch.Tensor, d: int, eta: float, gs: float, l2c: float, tau: float,
                 hist: Optional[torch.Tensor] = None, beta_w: Optional[torch.Tensor] = None,
                 gate: Optional[torch.Tensor] = None) -> None:
    """One limited-memory BFGS combine + update on the state of :func:`lbfgs_state` (csrc/kernels/lbfgs.hip): g = sum_m
    coef_m msg_m, ``G = gs g + l2c beta``, the candidate pair ``(beta - beta_prev, G - G_prev)`` enters the ring iff
    ``s.y > 1e-8 sqrt(s.s y.y)`` with finite dots, and the step is ``beta -= tau p`` with p the two-loop recursion over
    the held pairs -- ``beta -= eta G`` while none is held, or, with the ring emptied, when ``G.p`` is not finite and
    > 0.  Native on GPU tensors; on CPU tensors a NumPy twin of the same Gram-space algorithm (every dot product read
    off ``V^T V``, the recursion on coefficient vectors)."""
    memory, ld, d, tau = (int(state.shape[0]) - 3) // 2, int(beta.numel()), int(d), float(tau)
    if state.dim() != 2 or state.shape[0] != 2 * memory + 3 or not 1 <= memory <= LBFGS_MAX_MEMORY or \
            state.shape[1] != ld or state.dtype != torch.float64 or ring.numel() != 4 or ring.dtype != torch.int32:
        raise ValueError(f"lbfgs_update: state must be float64 [2 * memory + 3, {ld}] with memory in 1.."
                         f"{LBFGS_MAX_MEMORY} and ring int32 [4], got {list(state.shape)} and {list(ring.shape)}")
    if not 1 <= d <= ld:
        raise ValueError(f"lbfgs_update: d must be in 1..{ld}, got {d}")
    if not (tau > 0.0 and tau != float("inf")):
        raise ValueError(f"lbfgs_update: the step must be finite and > 0, got {tau}")
    if beta.is_cuda:
        C = native()
        if len(msgs) > C.MAX_MSGS:
            raise ValueError(f"at most {C.MAX_MSGS} messages per combine")
        C.lbfgs_update(list(msgs), [float(c) for c in coefs], beta, hist, beta_w, state, ring, memory, d, float(eta),
                       float(gs), float(l2c), tau, gate)
        return
    if gate is not None and int(gate.reshape(-1)[0]) != 0:
        return
    st, rg, b = state.numpy(), ring.numpy(), beta.numpy()[:d].copy()
    g = np.zeros(d)
    for m, c in zip(msgs, coefs):
        g += float(c) * m[:d].double().numpy()
    G = gs * g + l2c * b
    head, count, started = int(rg[0]), int(rg[1]), bool(rg[2])
    with np.errstate(all="ignore"):
        if started:
            s, y = b - st[2 * memory, :d], G - st[2 * memory + 1, :d]
            sy, ss, yy = s.dot(y), s.dot(s), y.dot(y)
            if np.isfinite([sy, ss, yy]).all() and sy > 1e-8 * np.sqrt(ss * yy):
                slot = (head + count) % memory if count < memory else head
                st[slot, :d], st[memory + slot, :d] = s, y
                head, count = (head, count + 1) if count < memory else ((head + 1) % memory, count)
        mode, p = 1, G
        if count:
            k, rows = count, [(head + j) % memory for j in range(count)]
            V = np.stack([st[r, :d] for r in rows] + [st[memory + r, :d] for r in rows] + [G], axis=1)  # [d, 2k + 1]
            Wg, c = V.T.dot(V), np.zeros(2 * k + 1)
            c[2 * k] = 1.0
            a = np.zeros(k)
            for j in range(k - 1, -1, -1):
                a[j] = Wg[j].dot(c) / Wg[j, k + j]
                c[k + j] -= a[j]
            c *= Wg[k - 1, 2 * k - 1] / Wg[2 * k - 1, 2 * k - 1]
            for j in range(k):
                c[j] += a[j] - Wg[k + j].dot(c) / Wg[j, k + j]
            gp = Wg[2 * k].dot(c)
            mode = 0 if np.isfinite(gp) and gp > 0 else 2
            if mode == 0:
                p = V.dot(c)
        nb = b - tau * p if mode == 0 else b - eta * G
    st[2 * memory, :d], st[2 * memory + 1, :d], st[2 * memory + 2, :d] = b, G, p
    rg[:] = (0 if mode == 2 else head, 0 if mode == 2 else count, 1, mode)
    new = torch.from_numpy(nb)
    beta[:d] = new
    if hist is not None:
        hist[:d] = new
    if beta_w is not None:
        beta_w.zero_()
        beta_w[:d] = new.to(beta_w.dtype)


NEWTON_MAX_INNER = 32  # csrc/kernels/launchers.h kNewtonMaxInner


def newton_state(ld_x: int, device=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """A fresh Newton-CG state for a model of ``ld_x`` columns: ``state`` fp64 ``[5, ld_x]`` (the accumulated step x,
    the CG residual, the direction, the gradient at the outer iterate and a scratch row that holds H dir within a
    round), ``scal`` fp64 ``[2]`` (rs, g0norm2) and ``phase`` int32 ``[4]`` (0 / 1: a gradient / a CG round is next,
    the CG steps taken in this outer iteration, the last round's mode -- models/losses.py NEWTON_MODES -- and the outer
    iterations finished).  ``newton_cg_update`` advances all three in place."""
    return (torch.zeros((5, int(ld_x)), dtype=torch.float64, device=device),
            torch.zeros(2, dtype=torch.float64, device=device), torch.zeros(4, dtype=torch.int32, device=device))


def newton_cg_update(msgs: Sequence[torch.Tensor], coefs: Sequence[float], beta: torch.Tensor, state: torch.Tensor,
                     scal: torch.Tensor, phase: torch.Tensor, ld_x: int, d_x: int, J: int, eta: float, gs: float,
                     l2c: float, xi: float, tau: float, hist: Optional[torch.Tensor] = None,
                     beta_w: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None) -> None:
    """One round of truncated Newton on the state of :func:`newton_state` (csrc/kernels/newton_cg.hip).  beta, the
    messages and beta_w are ``[2][ld_x]``; block 0 of the messages decodes to g and block 1 to u, ``G = gs g + l2c
    beta`` and ``H dir = gs u + l2c dir``.  A gradient round (phase 0) starts linear CG on ``H x = -G`` and writes
    ``[beta ; dir]`` to beta_w; a CG round takes one step and either writes the next direction or ends the outer
    iteration with ``beta += tau x`` (``beta -= eta G`` where CG could not start or take a first step) and writes
    ``[beta' ; 0]``.  hist takes ``[beta' ; 0]`` in every round.  Native on GPU tensors; on CPU tensors a NumPy twin of
    the same recurrences."""
    ld_x, d_x, J, xi, tau = int(ld_x), int(d_x), int(J), float(xi), float(tau)
    if not (1 <= d_x <= ld_x and beta.numel() == 2 * ld_x):
        raise ValueError(f"newton_cg_update: two blocks of {ld_x} columns do not describe this model")
    if tuple(state.shape) != (5, ld_x) or state.dtype != torch.float64 or scal.numel() != 2 or \
            scal.dtype != torch.float64 or phase.numel() != 4 or phase.dtype != torch.int32:
        raise ValueError(f"newton_cg_update: state must be float64 [5, {ld_x}], scal float64 [2] and phase int32 [4]")
    if not 1 <= J <= NEWTON_MAX_INNER:
        raise ValueError(f"newton_cg_update: J must be in 1..{NEWTON_MAX_INNER}, got {J}")
    for name, v in (("tolerance", xi), ("step", tau)):
        if not (v > 0.0 and v != float("inf")):
            raise ValueError(f"newton_cg_update: the {name} must be finite and > 0, got {v}")
    if beta.is_cuda:
        C = native()
        if len(msgs) > C.MAX_MSGS:
            raise ValueError(f"at most {C.MAX_MSGS} messages per combine")
        C.newton_cg_update(list(msgs), [float(c) for c in coefs], beta, hist, beta_w, state, scal, phase, ld_x, d_x, J,
                           float(eta), float(gs), float(l2c), xi, tau, gate)
        return
    if gate is not None and int(gate.reshape(-1)[0]) != 0:
        return
    st, sc, ph, b = state.numpy(), scal.numpy(), phase.numpy(), beta.numpy()[:d_x].copy()
    g, u = np.zeros(d_x), np.zeros(d_x)
    for m, c in zip(msgs, coefs):
        g += float(c) * m[:d_x].double().numpy()
        u += float(c) * m[ld_x: ld_x + d_x].double().numpy()
    x, r, dr, G0 = (st[k, :d_x] for k in range(4))
    cg, inner, nd = ph[0] == 1, (int(ph[1]) if ph[0] == 1 else 0), np.zeros(d_x)
    ok = lambda v: bool(np.isfinite(v) and v > 0)  # noqa: E731
    with np.errstate(all="ignore"):
        if not cg:
            G0[:] = gs * g + l2c * b
            rs = float(G0.dot(G0))
            if ok(rs):
                mode, sc[:] = 0, rs
                x[:], r[:], dr[:] = 0.0, -G0, -G0
            else:
                mode = 6
        else:
            Hv = gs * u + l2c * dr
            kappa = float(dr.dot(Hv))
            if not ok(kappa):
                mode = 5 if inner == 0 else 4
            else:
                a = sc[0] / kappa
                x += a * dr
                r -= a * Hv
                rs, inner = float(r.dot(r)), inner + 1
                mode = 2 if not rs > xi * xi * sc[1] else 3 if inner >= J else 1
                if mode == 1:
                    dr[:] = r + (rs / sc[0]) * dr
                    sc[0] = rs
        if mode in (0, 1):
            nb, nd = b, dr.copy()
        else:
            nb = b - eta * G0 if mode >= 5 else b + tau * x
    ph[:] = (int(mode in (0, 1)), inner, mode, int(ph[3]) + int(mode not in (0, 1)))
    new = torch.from_numpy(nb)
    beta[:d_x] = new
    if hist is not None:
        hist[:d_x] = new
        hist[ld_x:] = 0.0
    if beta_w is not None:
        beta_w.zero_()
        beta_w[:d_x] = new.to(beta_w.dtype)
        beta_w[ld_x: ld_x + d_x] = torch.from_numpy(nd).to(beta_w.dtype)


def _update_blocked(name, msgs, coefs, beta, u, block_ld, d_x, decay, gm, l2, thr, theta, rule, hist, beta_w,
                    g_out) -> None:
    """The two blocked forms: ``thr`` None is combine_update_blocks, a sequence is combine_update_prox."""
    M = len(decay)
    if not ((thr is None or (1 <= M and len(thr) == M)) and len(gm) == M and len(l2) == M
            and beta.numel() == M * block_ld and 1 <= d_x <= block_ld):
        raise ValueError(f"{name}: {M} blocks of {block_ld} columns do not describe this model")
    if thr is not None and not all(float(t) >= 0.0 for t in thr):
        raise ValueError(f"{name}: thresholds must be >= 0 and not NaN, got {list(thr)}")
    if beta.is_cuda:
        C = native()
        if len(msgs) > C.MAX_MSGS:
            raise ValueError(f"at most {C.MAX_MSGS} messages per combine")
        coefs_k = [[float(x) for x in v] for v in ((decay, gm, l2) if thr is None else (decay, gm, l2, thr))]
        getattr(C, name)(list(msgs), [float(c) for c in coefs], beta, u, hist, beta_w, g_out, int(block_ld), int(d_x),
                         *coefs_k, float(theta), int(rule))
        return
    for k in range(M):
        s = slice(k * block_ld, (k + 1) * block_ld)
        _update_torch([m[s] for m in msgs], coefs, beta[s], u[s], d_x, decay[k], gm[k], l2[k], theta, rule,
                      None if hist is None else hist[s], None if beta_w is None else beta_w[s],
                      None if g_out is None else g_out[s], thr=None if thr is None else float(thr[k]))


def _soft_threshold(x: torch.Tensor, t: float) -> torch.Tensor:
    return torch.where(x.abs() <= t, torch.zeros_like(x), x - torch.copysign(torch.full_like(x, t), x))


def _update_torch(msgs, coefs, beta, u, d, decay, gm, l2, theta, rule, hist, beta_w, g_out, thr=None) -> None:
    g = torch.zeros(d, dtype=torch.float64)
    for m, c in zip(msgs, coefs):
        g += float(c) * m[:d].double()
    b = beta[:d]
    if rule == 0:
        nb = decay * b - gm * g
        if thr is not None:
            nb = _soft_threshold(nb, thr)
    else:
        yt = (1.0 - theta) * b + theta * u[:d]
        nb = yt - gm * g - l2 * b
        if thr is not None:
            nb = _soft_threshold(nb, thr)
        u[:d] = b + (nb - b) * (1.0 / theta)
    beta[:d] = nb
    if hist is not None:
        hist[:d] = nb
    if beta_w is not None:
        beta_w.zero_()
        beta_w[:d] = nb.to(beta_w.dtype)
    if g_out is not None:
        g_out[:d] = g
