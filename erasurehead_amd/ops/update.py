"""Master decode-combine + GD/AGD update (K5/K7/K8; csrc/kernels/update.hip).

``combine_update`` computes g = sum_m coef_m * msg_m and applies the reference update
(ref src/naive.py:112-122) to the fp64 master state in one launch, also writing the
betaset history row and the worker-precision copy of the new beta.
"""
from __future__ import annotations

from typing import Optional, Sequence

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
