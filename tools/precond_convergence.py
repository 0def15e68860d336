"""Rounds to a common training loss: plain GD at its best ``--lr`` against ``--precondition diag --lr 1``.

    python tools/precond_convergence.py [--out FILE] [--device cpu|cuda]

An illustration, not a benchmark and not a guarantee.  Logistic regression on a two-component Gaussian mixture
(n = 8000, d = 50, the shape of ``--data synthetic``'s generator) whose columns are rescaled by 10**U(-2, 2), handed to
the engine as an ``ArraySource``; naive scheme, four workers, GD, beta_0 = 0 scale (seeded), alpha = 1 / n.  Plain GD runs
ROUNDS rounds at every lr of a grid of powers of two; its best lr is the one with the lowest final training loss
(a diverged run counts as infinite).  The preconditioned run takes ``--lr 1`` and, because a Jacobi step of length 1
is not a contraction when the columns are correlated (the mixture's mean makes them so), also every lr of 2**-6 .. 2.
The common loss is the plain run's final loss at its best lr; reported are the rounds every run needs to reach it and
the loss curves' ends.  One JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, W, ROUNDS, DECADES = 8000, 50, 4, 200, 2.0


def main():
    import numpy as np
    import torch

    from erasurehead_amd.config import RunConfig
    from erasurehead_amd.data.source import ArraySource
    from erasurehead_amd.engine import Trainer, evaluate
    from erasurehead_amd.parallel.dist import DistEnv

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "precond_convergence.json"))
    ap.add_argument("--device", default="cpu")
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    mu = rng.randn(D) / np.sqrt(D) * 2.0
    y = rng.choice([-1.0, 1.0], N + N // 4)
    X = (rng.randn(len(y), D) + y[:, None] * mu) * 10.0 ** rng.uniform(-DECADES, DECADES, D)
    parts = [(X[k:N:W], y[k:N:W]) for k in range(W)]
    env = DistEnv() if a.device == "cpu" else DistEnv(device=torch.device(a.device))

    def curve(**kw):
        cfg = RunConfig(W + 1, N, D, "/tmp/eh_precond_convergence/", 0, "x", 0, 0, 0, 0, 0, 0, "GD", num_itrs=ROUNDS,
                        seed=0, verbose=False, loss="logistic", **kw)
        tr = Trainer(cfg, env, ArraySource(parts, (X[N:], y[N:])))
        loss = np.asarray(evaluate(tr, tr.run(), write=False).training_loss, dtype=np.float64)
        return np.where(np.isfinite(loss), loss, np.inf)

    grid = [2.0 ** k for k in range(-30, 8)]
    plain = {lr: curve(lr=lr) for lr in grid}
    best = min(grid, key=lambda lr: plain[lr][-1])
    target = float(plain[best][-1])
    pres = {lr: curve(lr=lr, precondition="diag") for lr in [2.0 ** k for k in range(-6, 2)]}
    pbest = min(pres, key=lambda lr: pres[lr][-1])

    def rounds_to(c):
        hit = np.nonzero(c <= target)[0]
        return int(hit[0]) + 1 if hit.size else None

    r = {"n": N, "d": D, "column_scale_decades": 2 * DECADES, "rounds": ROUNDS, "plain_best_lr": best,
         "common_loss": target, "plain_rounds_to_common_loss": ROUNDS,
         "precond_lr1_rounds_to_common_loss": rounds_to(pres[1.0]),
         "precond_lr1_loss_first_last": [float(pres[1.0][0]), float(pres[1.0][-1])],
         "precond_best_lr": pbest, "precond_best_rounds_to_common_loss": rounds_to(pres[pbest]),
         "precond_best_loss_first_last": [float(pres[pbest][0]), float(pres[pbest][-1])],
         "precond_rounds_by_lr": {str(lr): rounds_to(c) for lr, c in pres.items()},
         "plain_loss_first_last": [float(plain[best][0]), target],
         "device": a.device}
    print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
