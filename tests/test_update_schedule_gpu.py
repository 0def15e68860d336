"""The Python master loop on GPU tensors (native_loop=False): UpdateSchedule.apply's blocked and proximal forms
launch combine_update_blocks / combine_update_prox on the device, where the per-feature GPU files only run the
native pump.  The run is held to the CPU engine at the engine tolerance of tests/test_engine_gpu.py
::test_gpu_matches_cpu (the soft threshold is 1-Lipschitz: it does not widen it)."""
import numpy as np
import pytest
import torch

from erasurehead_amd.engine import Trainer
from erasurehead_amd.parallel.dist import DistEnv
from test_multimodel_cpu import ALPHAS, CASES, LRS, arrival_sets, make

pytestmark = pytest.mark.gpu
RUNS = {"sweep3": dict(sweep_alpha=ALPHAS, sweep_lr=LRS), "single_l1": dict(l1=0.02),
        "sweep3_l1s": dict(sweep_alpha=ALPHAS, sweep_lr=LRS, sweep_l1=[0.0, 0.02, 0.05])}


@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", ["naive", "frc"])
@pytest.mark.parametrize("run", sorted(RUNS))
def test_python_loop_on_the_gpu_matches_the_cpu_engine(run, name, rule, native):
    out = {}
    for dev in ("cpu", "cuda"):
        cfg, src, sch, _ = make(CASES[name], rule, native_loop=False, **RUNS[run])  # 40 rows, d = 33, 8 rounds, fp64
        tr = Trainer(cfg, DistEnv(device=torch.device(dev)), src, scheme=sch)
        assert not tr.native_loop and tr.prox == (run != "sweep3") and tr.models == (1 if run == "single_l1" else 3)
        out[dev] = tr.run()
        assert tr.device_loop is None and tr.rank_report()["round_loop"] == "python"
    np.testing.assert_allclose(out["cuda"].betaset, out["cpu"].betaset, rtol=1e-9, atol=1e-11)
    assert arrival_sets(out["cuda"]) == arrival_sets(out["cpu"])
