"""Time auc_columns alone: the native pair count (csrc/kernels/auc.hip) against the torch sort path it replaced.

    python tools/profile_auc.py [--rounds 100] [--n-test 200000] [--dtype fp64] [--out FILE]
    python tools/profile_auc.py --cold native|torch     # the first call of a fresh process only

Scores are random normals (no ties), labels a fair coin.  Every timing is a host clock around the call and a device
synchronise, as tools/profile_eval.py takes its ``auc_s``.  Warm: the two paths alternate ``--reps`` times, each turn
the median of 5 calls.  ``--tiles`` also times the binding alone (row lists built once) for several tile sizes.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--n-test", type=int, default=200_000)
    ap.add_argument("--dtype", choices=["fp64", "fp32"], default="fp64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cold", choices=["native", "torch"], default=None)
    ap.add_argument("--tiles", type=int, nargs="*", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from erasurehead_amd._ext import native
    from erasurehead_amd.ops import eval as ev

    dev = torch.device("cuda")
    n, R = a.n_test, a.rounds
    g = torch.Generator(device=dev).manual_seed(1)
    P = torch.randn(n, R, generator=g, device=dev, dtype=torch.float64 if a.dtype == "fp64" else torch.float32)
    y = torch.where(torch.rand(n, generator=g, device=dev) < 0.5, -1.0, 1.0).double()
    C = native()

    def torch_path():
        pos = y == 1
        n_pos = int(pos.sum().item())
        out = np.full(R, np.nan)
        ev._auc_torch(pos, P, n_pos, n - n_pos, max(1, min(R, (1 << 26) // n)), out)
        return out

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t, r

    rec = {"R": R, "n_test": n, "dtype": a.dtype, "tile": C.AUC_TILE}
    if a.cold:
        rec["cold_path"] = a.cold
        rec["cold_s"], _ = timed(torch_path if a.cold == "torch" else lambda: ev.auc_columns(y, P))
    else:
        (_, want), (_, got) = timed(torch_path), timed(lambda: ev.auc_columns(y, P))  # warm-up, and the same answer
        rec["max_abs_diff"] = float(np.max(np.abs(want - got)))
        turns = {"native": [], "torch": []}
        for _ in range(a.reps):
            turns["native"].append(float(np.median([timed(lambda: ev.auc_columns(y, P))[0] for _ in range(5)])))
            turns["torch"].append(float(np.median([timed(torch_path)[0] for _ in range(5)])))
        rec["warm_s"] = turns
        small, large = torch.nonzero(y == 1).squeeze(1), torch.nonzero(y != 1).squeeze(1)
        if small.numel() > large.numel():
            small, large = large, small
        k = max(1, min(R, (1 << 26) // n))  # one chunk of the wrapper's rule
        sums = torch.empty(k, dtype=torch.int64, device=dev)
        flags = torch.empty(k, dtype=torch.int32, device=dev)
        for T in a.tiles:
            run = lambda: C.auc_pair_sums(P[:, :k], small, large, k, sums, flags, T)  # noqa: E731
            run()
            rec.setdefault("binding_s", {})[str(T)] = {"cols": k, "s": float(np.median([timed(run)[0] for _ in range(5)]))}
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
