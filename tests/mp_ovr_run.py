"""One rank of a multi-process one-vs-rest run (torchrun from tests/test_ovr_cpu.py / test_ovr_gpu.py).

python -m torch.distributed.run --nproc-per-node N tests/mp_ovr_run.py
  EH_OVR_OUT     the .npz rank 0 writes: betaset, beta0, the per-round arrival lists, the transport's name, the
                 round loop
  EH_OVR_DEVICE  cpu (gloo) or cuda (ranks sharing one GPU: IPC mailboxes, integrity tags on)
Builds the seeded AGC case of tests/test_ovr_cpu.py::make (uneven groups, logistic, C = 3, d_x = 33, AGD).
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
    from test_ovr_cpu import CASES, make

    env = init_distributed(os.environ.get("EH_OVR_DEVICE", "cuda"))
    cfg, src, sch, parts = make(CASES["agc_uneven"], "AGD")
    cfg.integrity = True
    tr = Trainer(cfg, env, src, scheme=sch)
    res = tr.run()
    if env.is_master:
        arr = np.array([[(w, p, 0.0) for (w, p, _) in a] for a in res.arrivals], dtype=object)
        np.savez(os.environ["EH_OVR_OUT"], betaset=res.betaset, beta0=tr.beta0, arrivals=arr,
                 transport=np.array(tr.transport), round_loop=np.array(str(tr.rank_report()["round_loop"])))
    env.barrier()
    tr.close()
    env.shutdown()


if __name__ == "__main__":
    main()
