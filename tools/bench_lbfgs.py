#!/usr/bin/env python
"""Microseconds per launch, back to back, of lbfgs_update (csrc/kernels/lbfgs.hip) next to combine_update and
combine_update_precond: the median over `--repeats` alternating series of `--iters` launches each between two HIP
events, one JSON line per case.  Where a kernel is shorter than the host takes to issue it (the two baselines, and
lbfgs_update at narrow widths) the figure is the launch issue rate, not the kernel's duration.

    python tools/bench_lbfgs.py [--widths 1000,54] [--memories 1,3,7] [--msgs 4] [--out profiles/lbfgs/kernels.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from erasurehead_amd.ops.update import combine_update, combine_update_precond, lbfgs_state, lbfgs_update  # noqa: E402


def timed(fn, iters):
    for _ in range(20):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="1000,54")
    ap.add_argument("--memories", default="1,3,7")
    ap.add_argument("--msgs", type=int, default=4)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev, rows = "cuda", []
    for d in (int(x) for x in a.widths.split(",")):
        ld = d + (d & 1)
        msgs = [torch.randn(2 * ld, dtype=torch.float64, device=dev) for _ in range(a.msgs)]
        coefs = [1.0] * a.msgs
        beta, u = torch.randn(ld, dtype=torch.float64, device=dev), torch.zeros(ld, dtype=torch.float64, device=dev)
        b2, u2 = torch.randn(2 * ld, dtype=torch.float64, device=dev), torch.zeros(2 * ld, dtype=torch.float64, device=dev)
        hist, bw = torch.zeros(2 * ld, dtype=torch.float64, device=dev), torch.zeros(2 * ld, dtype=torch.float64, device=dev)
        rings = {}
        cases = {"combine_update": lambda: combine_update(msgs, coefs, beta, u, d, 0.999, 1e-3, 1e-3, 0.5, 0,
                                                          hist=hist[:ld], beta_w=bw[:ld]),
                 "combine_update_precond": lambda: combine_update_precond(msgs, coefs, b2, u2, ld, d, 0.5, 1e-3, 1e-3, 1e-6,
                                                                          0.5, 0, hist=hist, beta_w=bw)}
        for m in (int(x) for x in a.memories.split(",")):
            state, ring = lbfgs_state(m, ld, dev)
            state[:m, :d].normal_()  # a full ring of pairs with s.y > 0; the candidates are whatever the steps give
            state[m:2 * m, :d] = 2.0 * state[:m, :d]
            ring[1] = m

            def step(state=state, ring=ring, bl=beta.clone()):
                lbfgs_update(msgs, coefs, bl, state, ring, d, 1e-3, 1e-3, 1e-3, 1e-3, hist=hist[:ld], beta_w=bw[:ld])
            cases[f"lbfgs_update M={m}"] = step
            rings[f"lbfgs_update M={m}"] = ring
        series = {k: [] for k in cases}
        for _ in range(a.repeats):  # alternating: every repeat visits every case
            for k, fn in cases.items():
                series[k].append(timed(fn, a.iters))
        for k, v in series.items():
            rows.append(dict(kernel=k, d=d, msgs=a.msgs, us=round(statistics.median(v), 3), series=[round(x, 3) for x in v]))
            if k in rings:  # (head, count, started, mode) after the last launch: mode 0 = the quasi-Newton path was timed
                rows[-1]["ring"] = rings[k].tolist()
            print(json.dumps(rows[-1]))
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
