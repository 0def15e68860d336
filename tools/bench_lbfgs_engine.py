"""ms per round of a ``--lbfgs 5`` logistic run against the plain GD run, on one MI355X.

    python tools/bench_lbfgs_engine.py [--memory 5] [--out FILE]

The headline shape and scheme (1e6 x 1000, fp64, AGC with 8 workers, s = 2, k = 6, one process) with update rule GD on
both sides (``--lbfgs`` rejects AGD), synthetic data of the same shape and seed.  The plain run takes the fused dense
path it always took; the L-BFGS run launches the gradient and lbfgs_update separately.  The two runs alternate, three
of each; 60 untimed rounds, then 60 timed ones between device synchronisations (``Trainer.run(timed_start=...)``, as
bench.py times its headline).  One JSON line per run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, STEPS, REPS = 60, 60, 3


def main():
    import numpy as np
    import torch

    from erasurehead_amd.config import RunConfig
    from erasurehead_amd.engine import Trainer
    from erasurehead_amd.parallel.dist import DistEnv

    ap = argparse.ArgumentParser()
    ap.add_argument("--memory", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "lbfgs_engine.jsonl"))
    a = ap.parse_args()
    out = []
    for rep in range(REPS):
        for name, kw in (("plain_gd", {}), (f"lbfgs_{a.memory}", {"lbfgs": a.memory})):
            cfg = RunConfig(9, 1_000_000, 1000, "/tmp/eh_bench_lbfgs/", 0, "synthetic", 1, 2, 0, 3, 6, 0, "GD",
                            num_itrs=WARM + STEPS, precision="fp64", data="synthetic", data_seed=1234, seed=0,
                            allow_uneven_groups=True, verbose=False, loss="logistic", lr=1.0, evaluate=False, **kw)
            tr = Trainer(cfg, DistEnv(device=torch.device("cuda")))
            res = tr.run(timed_start=WARM)
            r = {"run": name, "rep": rep, "rounds": res.timed_rounds,
                 "ms_per_round": 1e3 * res.timed_seconds / res.timed_rounds,
                 "round_loop": str(tr.rank_report()["round_loop"]), "finite": bool(np.all(np.isfinite(res.betaset)))}
            if tr.lbfgs_state is not None:  # (head, count, started, mode) as the run ended
                r["ring"] = tr.lbfgs_state[1].tolist()
            out.append(r)
            print(json.dumps(r), flush=True)
            tr.close()
            del tr, res
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(r) + "\n" for r in out)


if __name__ == "__main__":
    main()
