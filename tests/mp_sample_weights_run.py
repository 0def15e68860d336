"""One rank of a multi-process run with class and sample weights (torchrun from tests/test_sample_weights_gpu.py).

python -m torch.distributed.run --nproc-per-node N tests/mp_sample_weights_run.py
  EH_WEIGHTS_OUT     the .npz rank 0 writes: betaset, beta0, the per-round arrival lists, the transport's name, the
                     round loop and the report's weight fields
  EH_WEIGHTS_DEVICE  cpu (gloo) or cuda (ranks sharing one GPU: IPC mailboxes, integrity tags on)
  EH_WEIGHTS_CASE    a case of tests/test_multimodel_cpu.py CASES (default agc_uneven), run with AGD, the logistic
                     loss, --class-weight balanced and the sample weights of tests/test_sample_weights_cpu.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402


def main():
    from erasurehead_amd.engine import Trainer
    from erasurehead_amd.parallel.dist import init_distributed
    from test_multimodel_cpu import CASES
    from test_sample_weights_cpu import make_weighted

    env = init_distributed(os.environ.get("EH_WEIGHTS_DEVICE", "cuda"))
    cfg, src, sch, parts, wts = make_weighted(CASES[os.environ.get("EH_WEIGHTS_CASE", "agc_uneven")], "AGD",
                                              class_weight="balanced")
    cfg.integrity = True
    tr = Trainer(cfg, env, src, scheme=sch)
    res = tr.run()
    if env.is_master:
        rep = tr.rank_report()
        arr = np.array([[(w, p, 0.0) for (w, p, _) in a] for a in res.arrivals], dtype=object)
        np.savez(os.environ["EH_WEIGHTS_OUT"], betaset=res.betaset, beta0=tr.beta0, arrivals=arr,
                 transport=np.array(tr.transport), round_loop=np.array(str(rep["round_loop"])),
                 weighted=np.array(bool(rep["weighted"])), class_weight=np.array(rep["class_weight"]),
                 weight_sum_over_n=np.array(rep["weight_sum_over_n"]))
    env.barrier()
    tr.close()
    env.shutdown()


if __name__ == "__main__":
    main()
