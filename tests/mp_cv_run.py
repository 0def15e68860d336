"""One rank of a multi-process cross-validation run (torchrun from tests/test_cv_cpu.py / test_cv_gpu.py).

python -m torch.distributed.run --nproc-per-node N tests/mp_cv_run.py
  EH_CV_OUT     the .npz rank 0 writes: betaset, beta0, the per-round arrival lists, the transport's name, the
                round loop
  EH_CV_DEVICE  cpu (gloo) or cuda (ranks sharing one GPU: IPC mailboxes, integrity tags on)
Builds the seeded AGC case of tests/cv_cases.py::make (uneven groups, logistic, K = 3, d_x = 33, AGD).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402


def main():
    from cv_cases import CASES, MP_CASE, MP_K, MP_RULE, make
    from erasurehead_amd.engine import Trainer
    from erasurehead_amd.parallel.dist import init_distributed

    env = init_distributed(os.environ.get("EH_CV_DEVICE", "cuda"))
    cfg, src, sch, parts = make(CASES[MP_CASE], MP_RULE, MP_K)
    cfg.integrity = True
    tr = Trainer(cfg, env, src, scheme=sch)
    res = tr.run()
    if env.is_master:
        arr = np.array([[(w, p, 0.0) for (w, p, _) in a] for a in res.arrivals], dtype=object)
        np.savez(os.environ["EH_CV_OUT"], betaset=res.betaset, beta0=tr.beta0, arrivals=arr,
                 transport=np.array(tr.transport), round_loop=np.array(str(tr.rank_report()["round_loop"])))
    env.barrier()
    tr.close()
    env.shutdown()


if __name__ == "__main__":
    main()
