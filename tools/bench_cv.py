"""ms per round of a ``--cv 8`` logistic run against one binary logistic run, on one MI355X.

    python tools/bench_cv.py [PRECISIONS] [--out FILE]        e.g.  python tools/bench_cv.py fp64,fp32x64

The headline shape and scheme (1e6 x 1000, AGC with 8 workers, s = 2, k = 6, AGD, one process), synthetic data of the
same shape and seed for both runs.  The two runs alternate, three of each per precision; 60 untimed rounds, then 60
timed ones between device synchronisations (``Trainer.run(timed_start=...)``, as bench.py times its headline).  One
JSON line per run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, STEPS, REPS, FOLDS = 60, 60, 3, 8


def main():
    import numpy as np
    import torch

    from erasurehead_amd.config import RunConfig
    from erasurehead_amd.engine import Trainer
    from erasurehead_amd.parallel.dist import DistEnv

    ap = argparse.ArgumentParser()
    ap.add_argument("precisions", nargs="?", default="fp64,fp32x64")
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "cv_engine.jsonl"))
    a = ap.parse_args()
    out = []
    for prec in a.precisions.split(","):
        for rep in range(REPS):
            for name, kw in (("binary_logistic", {}), ("cv8_logistic", {"cv": FOLDS})):
                cfg = RunConfig(9, 1_000_000, 1000, "/tmp/eh_bench_cv/", 0, "synthetic", 1, 2, 0, 3, 6, 0, "AGD",
                                num_itrs=WARM + STEPS, precision=prec, data="synthetic", data_seed=1234, seed=0,
                                allow_uneven_groups=True, verbose=False, loss="logistic", lr=1.0, evaluate=False, **kw)
                tr = Trainer(cfg, DistEnv(device=torch.device("cuda")))
                res = tr.run(timed_start=WARM)
                r = {"run": name, "precision": prec, "rep": rep, "rounds": res.timed_rounds,
                     "ms_per_round": 1e3 * res.timed_seconds / res.timed_rounds,
                     "round_loop": str(tr.rank_report()["round_loop"]), "plan": type(tr.plan).__name__,
                     "finite": bool(np.all(np.isfinite(res.betaset)))}
                out.append(r)
                print(json.dumps(r), flush=True)
                tr.close()
                del tr, res
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
