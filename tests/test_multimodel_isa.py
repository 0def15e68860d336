"""Static check of the multi-model gradient kernels in the built gfx950 code object (no GPU needed): a wave keeps
the model and the gradient accumulators of its two models, and the row it is working on, in registers
(csrc/kernels/grad_multimodel.hip), which only pays if none of them spills."""
import os

import pytest

from test_isa_checks import READELF, _code_objects, _kernel_regs


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_multimodel_kernels_do_not_spill(tmp_path):
    regs = {}
    for co in _code_objects(tmp_path):
        regs.update(_kernel_regs(co))
    mm = {n: r for n, r in regs.items() if "grad_models" in n}
    # (fp64, fp32, fp32 storage with fp64 accumulators) x (4, 8, 16 columns per lane) x three scalar losses
    assert len(mm) == 27, sorted(mm)
    for n, (v, spill) in mm.items():
        print(n, v, spill)
        assert spill == 0, f"{n} spills {spill} VGPRs"
        assert v <= 256, f"{n} needs {v} VGPRs: more than two workgroups per CU allow"
