"""Rounds to the common training loss of tools/precond_convergence.py for ``--newton-cg J``, on that tool's exact data.

    python tools/newton_convergence.py [--out FILE] [--device cpu|cuda] [--inner 8] [--tol 0.1] [--step 1] [--zero-start]

An illustration on one data set, not a benchmark and not a claim.  The data, the scheme and the round count are those
of tools/precond_convergence.py and tools/lbfgs_convergence.py (logistic regression, a column-rescaled two-component
mixture, n = 8000, d = 50, naive scheme, four workers, 200 rounds); the plain run's best ``--lr`` and the common loss are
read from its recorded result (profiles/precond/convergence.json), next to the L-BFGS study's
(profiles/lbfgs/convergence.json).  A round of a Newton-CG run is a gradient round or a CG round, so its rounds count
like any other run's.  Reported: the rounds to the common loss, the first and last training loss, the outer iterations
finished, or that the run diverged.  One JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, W, ROUNDS, DECADES = 8000, 50, 4, 200, 2.0  # tools/precond_convergence.py


def main():
    import numpy as np
    import torch

    from erasurehead_amd.codes import make_scheme
    from erasurehead_amd.config import RunConfig
    from erasurehead_amd.data.source import ArraySource
    from erasurehead_amd.engine import Trainer, evaluate
    from erasurehead_amd.parallel.dist import DistEnv

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "newton_convergence.json"))
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--tol", type=float, default=0.1)
    ap.add_argument("--step", type=float, default=1.0)
    ap.add_argument("--zero-start", action="store_true", help="beta_0 = 0 instead of the naive scheme's random draw")
    a = ap.parse_args()
    with open(os.path.join(ROOT, "profiles", "precond", "convergence.json")) as f:
        ref = json.loads(f.readline())
    with open(os.path.join(ROOT, "profiles", "lbfgs", "convergence.json")) as f:
        lb = json.loads(f.readline())
    rng = np.random.RandomState(0)
    mu = rng.randn(D) / np.sqrt(D) * 2.0
    y = rng.choice([-1.0, 1.0], N + N // 4)
    X = (rng.randn(len(y), D) + y[:, None] * mu) * 10.0 ** rng.uniform(-DECADES, DECADES, D)
    parts = [(X[k:N:W], y[k:N:W]) for k in range(W)]
    env = DistEnv() if a.device == "cpu" else DistEnv(device=torch.device(a.device))
    cfg = RunConfig(W + 1, N, D, "/tmp/eh_newton_convergence/", 0, "x", 0, 0, 0, 0, 0, 0, "GD", num_itrs=ROUNDS, seed=0,
                    verbose=False, loss="logistic", lr=float(ref["plain_best_lr"]), newton_cg=a.inner, newton_tol=a.tol,
                    newton_step=a.step)
    sch = make_scheme("naive", W, 0, N, 0, 0)
    sch.init_zero = bool(a.zero_start)  # (the naive scheme draws beta_0 from N(0, 1))
    tr = Trainer(cfg, env, ArraySource(parts, (X[N:], y[N:])), scheme=sch)
    loss = np.asarray(evaluate(tr, tr.run(), write=False).training_loss, dtype=np.float64)
    loss = np.where(np.isfinite(loss), loss, np.inf)
    hit = np.nonzero(loss <= ref["common_loss"])[0]
    r = {"n": N, "d": D, "rounds": ROUNDS, "newton_cg": a.inner, "newton_tol": a.tol, "newton_step": a.step, "zero_start": bool(a.zero_start),
         "fallback_lr": ref["plain_best_lr"], "common_loss": ref["common_loss"],
         "rounds_to_common_loss": int(hit[0]) + 1 if hit.size else None,
         "loss_first_last": [float(loss[0]), float(loss[-1])], "loss_min": float(loss.min()),
         "diverged": bool(not np.isfinite(loss[-1]) or loss[-1] > loss[0]),
         "phase_at_the_end": [int(x) for x in tr.newton_state[2].tolist()],
         "plain_rounds_to_common_loss": ref["plain_rounds_to_common_loss"],
         "precond_best_lr": ref["precond_best_lr"],
         "precond_best_rounds_to_common_loss": ref["precond_best_rounds_to_common_loss"],
         "lbfgs5_rounds_to_common_loss": lb["rounds_to_common_loss"], "lbfgs5_loss_last": lb["loss_first_last"][1],
         "device": a.device}
    print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
