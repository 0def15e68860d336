"""Static check of the cross-validation gradient kernels in the built gfx950 code object (no GPU needed): like the
multi-model kernels whose text they share (csrc/kernels/grad_models_kernel.h), a wave keeps the model and the gradient
accumulators of its two fold models, and the row it is working on, in registers, which only pays if none of them
spills; the fold counter lives in scalar registers."""
import os

import pytest

from test_isa_checks import READELF, _code_objects, _kernel_regs


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_cv_kernels_do_not_spill(tmp_path):
    regs = {}
    for co in _code_objects(tmp_path):
        regs.update(_kernel_regs(co))
    cv = {n: r for n, r in regs.items() if "grad_folds" in n}
    # (fp64, fp32, fp32 storage with fp64 accumulators) x (4, 8, 16 columns per lane) x (logistic, least squares,
    # squared hinge)
    assert len(cv) == 27, sorted(cv)
    for n, (v, spill) in cv.items():
        print(n, v, spill)
        assert spill == 0, f"{n} spills {spill} VGPRs"
        assert v <= 256, f"{n} needs {v} VGPRs: more than two workgroups per CU allow"
