"""What the proximal step (--l1 > 0) costs: the headline shape end to end, and the update kernels alone.

    python tools/bench_l1.py rounds  [--l1s 0,1e-4] [--reps 3] [--steps 20] [--warmup 5] [--out FILE.jsonl]
    python tools/bench_l1.py kernels [--launches 200] [--out FILE.jsonl]

``rounds`` runs bench.py's headline configuration (AGC, 8 workers, s = 2, k = 6, 1e6 x 1000, fp64, AGD, synthetic
data, one GPU, the device-driven stream loop) once per value of --l1s and repeats that --reps times, so the values
alternate inside one process on one box; it prints one JSON line per run (ms per round, the round loop, prox).  A run
with l1 = 0 takes the fused gradient + slab reduction + update launch; a run with l1 > 0 takes the separate
combine_update_prox launch, as a sweep does.

``kernels`` launches combine_update / combine_update_prox at d = 1000 and combine_update_blocks / combine_update_prox
at M = 8 x 1000 (6 fp64 messages, AGD, history row and worker copy written) back to back, alternating, and prints the
HIP-event time per launch of each batch.  Run it under ``rocprofv3 --kernel-trace --stats`` for the kernels' own
durations.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def rounds(a):
    from erasurehead_amd.config import RunConfig
    from erasurehead_amd.engine import Trainer
    from erasurehead_amd.parallel.dist import DistEnv

    env = DistEnv(device=torch.device("cuda"))
    est_round_ms = max(0.02, a.n_rows * a.n_cols * 8 / 6e9)
    w0 = int(np.ceil(a.clock_warmup_ms / est_round_ms)) + a.warmup  # bench.py's untimed clock warm-up + warm-up
    for rep in range(a.reps):
        for l1 in a.l1s:
            cfg = RunConfig(9, a.n_rows, a.n_cols, "/tmp/erasurehead_bench/", 0, "synthetic", 1, 2, 0, 3, 6, 0, "AGD",
                            num_itrs=w0 + a.steps, data="synthetic", data_seed=1234, seed=0, allow_uneven_groups=True,
                            verbose=False, l1=l1)
            tr = Trainer(cfg, env)
            res = tr.run(timed_start=w0)
            rep_ = tr.rank_report()
            emit({"bench": "rounds", "rep": rep, "l1": l1, "ms_per_round": 1e3 * res.timed_seconds / res.timed_rounds,
                  "round_loop": rep_["round_loop"], "prox": rep_["prox"], "steps": a.steps,
                  "nnz_final": int(np.count_nonzero(res.betaset[-1]))}, a.out)
            tr.close()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()


def kernels(a):
    from erasurehead_amd.ops.update import combine_update, combine_update_blocks, combine_update_prox

    dev = "cuda"
    rng = np.random.RandomState(0)
    for M in (1, 8):
        ld = 1000
        n = M * ld
        msgs = [torch.from_numpy(rng.randn(n)).to(dev) for _ in range(6)]
        coefs = [1.0] * 6
        beta, u = torch.from_numpy(rng.randn(n)).to(dev), torch.zeros(n, dtype=torch.float64, device=dev)
        hist, bw = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
        decay, gm, l2, thr = [0.999] * M, [1e-6] * M, [1e-3] * M, [1e-3] * M

        def plain():
            if M == 1:
                combine_update(msgs, coefs, beta, u, ld, decay[0], gm[0], l2[0], 0.4, 1, hist=hist, beta_w=bw)
            else:
                combine_update_blocks(msgs, coefs, beta, u, ld, ld, decay, gm, l2, 0.4, 1, hist=hist, beta_w=bw)

        def prox():
            combine_update_prox(msgs, coefs, beta, u, ld, ld, decay, gm, l2, thr, 0.4, 1, hist=hist, beta_w=bw)

        for rep in range(3):
            for name, fn in (("plain", plain), ("prox", prox)):
                for _ in range(20):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    fn()
                e1.record()
                e1.synchronize()
                emit({"bench": "kernels", "M": M, "d": ld, "kernel": name, "rep": rep,
                      "us_per_launch": 1e3 * e0.elapsed_time(e1) / a.launches}, a.out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("what", choices=["rounds", "kernels"])
    ap.add_argument("--l1s", type=lambda s: [float(x) for x in s.split(",")], default=[0.0, 1e-4])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clock-warmup-ms", type=float, default=60.0)
    ap.add_argument("--n-rows", type=int, default=1_000_000)
    ap.add_argument("--n-cols", type=int, default=1000)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU"
    (rounds if a.what == "rounds" else kernels)(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
