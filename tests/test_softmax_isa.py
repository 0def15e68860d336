"""Static check of the softmax gradient kernels in the built gfx950 code object (no GPU needed): a wave keeps
the model and the gradient accumulators of its two classes in registers (csrc/kernels/grad_softmax.hip),
which only pays if none of them spills."""
import os

import pytest

from test_isa_checks import READELF, _code_objects, _kernel_regs


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_softmax_kernels_do_not_spill(tmp_path):
    regs = {}
    for co in _code_objects(tmp_path):
        regs.update(_kernel_regs(co))
    sm = {n: r for n, r in regs.items() if "grad_softmax" in n}
    assert len(sm) == 6, sorted(sm)  # fp64 and fp32 at 4, 8 and 16 columns per lane
    for n, (v, spill) in sm.items():
        print(n, v, spill)
        assert spill == 0, f"{n} spills {spill} VGPRs"
