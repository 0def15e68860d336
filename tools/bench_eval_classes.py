"""Multi-class evaluation: the GEMM with the loss and accuracy in its epilogue (csrc/kernels/eval_classes.hip) against
the torch epilogue it replaces (engine/evaluate.py ``fused=False``: prediction GEMM, then logsumexp / gather / argmax or
the one-vs-rest chain over the stored logits), on the same tensors.

    python tools/bench_eval_classes.py [--out FILE] [--rows 125000] [--cols 1000] [--rounds 100] [--reps 9]

Default shapes: one partition of the headline (125 000 x 1000) with R = 100 stored rounds; C in {2, 4, 8} and the
padded C = 3 and 5; softmax and one-vs-rest logistic; fp64 and fp32.  Both paths are warmed, then timed alternately
(a host clock around calls that end in a device-to-host copy, so every timing includes its synchronise); a record
carries the median and the extremes of each path, their ratio, the largest relative difference of the loss sums and the
difference of the hit counts.  One JSON line per shape.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=125_000)
    ap.add_argument("--cols", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--classes", type=int, nargs="+", default=[2, 4, 8, 3, 5])
    a = ap.parse_args()
    import torch

    from erasurehead_amd.engine.evaluate import _ovr_sums, _softmax_sums
    from erasurehead_amd.models.losses import LOGISTIC
    from erasurehead_amd.ops import get_precision

    assert torch.cuda.is_available(), "bench_eval_classes.py measures on the GPU only"
    dev = torch.device("cuda")
    n, d, R = a.rows, a.cols, a.rounds
    g = torch.Generator(device=dev).manual_seed(1234)
    out = open(a.out, "w") if a.out else None
    for prec_name in ("fp64", "fp32"):
        prec = get_precision(prec_name)
        ld = prec.ld(d)
        X = torch.zeros((n, ld), dtype=prec.storage, device=dev)
        X[:, :d] = torch.randn(n, d, device=dev, dtype=torch.float64, generator=g).to(prec.storage)
        for C in a.classes:
            # what evaluate() holds: the fp64 models of every round, [R * C, ld_x]; logits of order one
            B = torch.zeros((R * C, ld), dtype=torch.float64, device=dev)
            B[:, :d] = torch.randn(R * C, d, device=dev, dtype=torch.float64, generator=g) / np.sqrt(d)
            y = torch.randint(0, C, (n,), device=dev, generator=g).to(prec.acc)
            for name, sums in (("softmax", _softmax_sums), ("ovr_logistic", _ovr_sums)):
                spec = SimpleNamespace(classes=C, d_x=d, loss=LOGISTIC)
                paths = {"fused": lambda: sums(X, y, B, spec, prec, fused=True),
                         "torch": lambda: sums(X, y, B, spec, prec, fused=False)}
                res = {k: f() for k, f in paths.items()}  # warm-up: code objects, allocator
                for f in paths.values():
                    f()
                ts = {k: [] for k in paths}
                for _ in range(a.reps):
                    for k, f in paths.items():  # alternate the two paths
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                        f()
                        ts[k].append(time.perf_counter() - t)
                rec = {"precision": prec_name, "loss": name, "n": n, "d": d, "R": R, "C": C, "reps": a.reps}
                for k, v in ts.items():
                    rec[k + "_ms"] = {"median": 1e3 * float(np.median(v)), "min": 1e3 * min(v), "max": 1e3 * max(v)}
                rec["torch_over_fused"] = rec["torch_ms"]["median"] / rec["fused_ms"]["median"]
                rec["gemm_TFps_fused"] = 2.0 * n * d * R * C / (rec["fused_ms"]["median"] * 1e-3) / 1e12
                rec["loss_rel_diff"] = float(np.max(np.abs(res["fused"][0] - res["torch"][0]) / np.abs(res["torch"][0])))
                rec["hits_abs_diff"] = float(np.max(np.abs(res["fused"][1] - res["torch"][1])))
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
    if out:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
