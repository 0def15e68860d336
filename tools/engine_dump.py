#!/usr/bin/env python3
"""Dump what a fixed matrix of seeded CPU engine runs computes, bit for bit, to compare two trees:

    python tools/engine_dump.py out.json      # in each tree; the two files must be identical

Per case and update rule: beta_0, the trajectory, the arrival sets, the evaluation (arrays, console lines and
result files, with the measured times replaced by fixed ones), rank_report() without its timings, and the
checkpoint of round 4.  Floats are written with float.hex()."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from erasurehead_amd.codes import make_scheme, scheme_key  # noqa: E402
from erasurehead_amd.config import RunConfig  # noqa: E402
from erasurehead_amd.data.source import ArraySource  # noqa: E402
from erasurehead_amd.engine import Trainer, evaluate  # noqa: E402
from erasurehead_amd.parallel.dist import DistEnv  # noqa: E402

SCHEMES = {"naive": (0, 0, 0, 5, 0, 0), "frc": (1, 0, 1, 7, 2, 0), "agc_uneven": (1, 0, 3, 9, 2, 6),
           "cyclic": (1, 0, 0, 7, 2, 0)}  # (is_coded, partitions, coded_ver, n_procs, s, num_collect)
SWEEP = dict(sweep_alpha=[1e-3, 1e-2, 1e-1], sweep_lr=[1.0, 1.0, 3.0])
CASES = {**{name: (name, {}) for name in SCHEMES},  # single logistic model on every scheme, the rest on naive
         "least_squares": ("naive", dict(loss="least_squares", lr=0.1, save_linear=True)),
         "squared_hinge": ("naive", dict(loss="squared_hinge", lr=0.1)),
         "class_weighted": ("naive", dict(class_weight=(2.0, 0.5))),
         "l1": ("naive", dict(l1=0.02)),
         "sweep3": ("naive", SWEEP),
         "sweep3_l1s": ("naive", dict(SWEEP, sweep_l1=[0.0, 0.02, 0.05])),
         "softmax3": ("naive", dict(loss="softmax", classes=3)),
         "ovr3_logistic": ("naive", dict(ovr=3)),
         "ovr3_squared_hinge": ("naive", dict(ovr=3, loss="squared_hinge", lr=0.1))}
ROWS, D, ROUNDS = 40, 33, 8


def hexed(x):
    """JSON-able copy with every float as float.hex()."""
    if isinstance(x, torch.Tensor):
        x = x.numpy()
    if isinstance(x, np.ndarray):
        x = x.tolist()
    if isinstance(x, dict):
        return {str(k): hexed(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [hexed(v) for v in x]
    return float(x).hex() if isinstance(x, (float, np.floating)) else x


def build(scheme, rule, out_dir, rounds=ROUNDS, **kw):
    is_coded, P, ver, n_procs, s, k = SCHEMES[scheme]
    W, key = n_procs - 1, scheme_key(is_coded, P, ver)
    uneven = key in ("approx", "replication") and W % (s + 1) != 0
    n_parts = make_scheme(key, W, s, ROWS * W, k, P, allow_uneven=uneven).n_partition_files
    rng = np.random.RandomState(0)
    C = kw.get("ovr") or (kw.get("classes") if kw.get("loss") == "softmax" else None)

    def draw(m):
        return rng.randn(m, D) * 0.3, (rng.randint(0, C, m).astype(np.float64) if C else rng.choice([-1.0, 1.0], m))

    src = ArraySource([draw(ROWS) for _ in range(n_parts)], draw(2 * ROWS))
    kw.setdefault("lr", 1.0)
    cfg = RunConfig(n_procs, ROWS * n_parts, D, out_dir + "/", 0, "x", is_coded, s, P, ver, k, 0, rule, num_itrs=rounds,
                    seed=0, verbose=True, allow_uneven_groups=uneven, **kw)
    sch = make_scheme(key, W, s, cfg.n_rows, k, P, allow_uneven=uneven, rng=np.random.RandomState(7))
    return Trainer(cfg, DistEnv(), src, scheme=sch)


def dump_case(scheme, rule, kw):
    with tempfile.TemporaryDirectory() as tmp:
        tr = build(scheme, rule, tmp, **kw)
        res = tr.run(log=lambda _line: None)
        res.timeset, res.total_time = 0.125 * (1.0 + np.arange(ROUNDS)), 2.5
        res.worker_timeset = 0.0625 * (1.0 + np.arange(res.worker_timeset.size)).reshape(res.worker_timeset.shape)
        lines = []
        ev = evaluate(tr, res, log=lines.append)
        files = {k: open(p).read() for k, p in sorted((ev.files or {}).items())}
        rep = {k: v for k, v in tr.rank_report().items() if not k.endswith("_us")}
        ck = os.path.join(tmp, "ck.pt")
        build(scheme, rule, tmp, rounds=4, checkpoint_every=4, checkpoint_path=ck, **kw).run(log=lambda _line: None)
        st = torch.load(ck, map_location="cpu", weights_only=True)
        st = {k: (None if k in ("timeset", "worker_timeset") else v) for k, v in st.items()}  # measured times
        return hexed({"beta0": tr.beta0, "betaset": res.betaset,
                      "arrivals": [[(w, p) for (w, p, _t) in r] for r in res.arrivals],
                      "eval": {k: v for k, v in vars(ev).items() if k != "files"}, "lines": lines, "files": files,
                      "rank_report": rep, "checkpoint": st})


def main(path):
    out = {f"{name}/{rule}": dump_case(scheme, rule, kw)
           for name, (scheme, kw) in CASES.items() for rule in ("GD", "AGD")}
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print(f"{len(out)} runs -> {path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "engine_dump.json")
