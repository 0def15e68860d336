"""One rank of a multi-process run with an L1 penalty (torchrun from tests/test_elastic_net_cpu.py / _gpu.py).

python -m torch.distributed.run --nproc-per-node N tests/mp_elastic_net_run.py
  EH_ELASTIC_OUT     the .npz rank 0 writes: betaset, beta0, the per-round arrival lists, the transport's name, the
                     round loop and the report's prox flag
  EH_ELASTIC_DEVICE  cpu (gloo) or cuda (ranks sharing one GPU: IPC mailboxes, integrity tags on)
  EH_ELASTIC_CASE    a case of tests/elastic_net_cases.py CASES (default agc_uneven), run with AGD and l1 = L1
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402


def main():
    from elastic_net_cases import CASES, L1, make
    from erasurehead_amd.engine import Trainer
    from erasurehead_amd.parallel.dist import init_distributed

    env = init_distributed(os.environ.get("EH_ELASTIC_DEVICE", "cuda"))
    cfg, src, sch, parts = make(CASES[os.environ.get("EH_ELASTIC_CASE", "agc_uneven")], "AGD", l1=L1)
    cfg.integrity = True
    tr = Trainer(cfg, env, src, scheme=sch)
    res = tr.run()
    if env.is_master:
        rep = tr.rank_report()
        arr = np.array([[(w, p, 0.0) for (w, p, _) in a] for a in res.arrivals], dtype=object)
        np.savez(os.environ["EH_ELASTIC_OUT"], betaset=res.betaset, beta0=tr.beta0, arrivals=arr,
                 transport=np.array(tr.transport), round_loop=np.array(str(rep["round_loop"])),
                 prox=np.array(bool(rep["prox"])))
    env.barrier()
    tr.close()
    env.shutdown()


if __name__ == "__main__":
    main()
