"""The kernels of the Exact moments' gradients (scikit-gpuppy_amd/csrc/exact_grad.hip) must not spill and must fit what their launch bounds
state.  The build kernel recomputes the transformed differences per k precisely so that no lane holds d of them: scratch traffic in that
loop would undo it.  It is launched with __launch_bounds__(256, 2) -- two workgroups per CU, which is what its LDS footprint at d = 64
allows: 2 [d][64] doubles, requested dynamically at the launch -- so two waves per SIMD share the 512 registers of a lane: 256 each.  The
finish kernel states four workgroups per CU: 128.  This test compiles the source for gfx950 with -Rpass-analysis=kernel-resource-usage (no
GPU needed), as tests/test_sensitivity_resources.py does."""
import os
import re

import pytest

from test_sensitivity_resources import CSRC, resource_usage

GPX_MAX_D = 64
LDS_PER_CU = 160 * 1024


@pytest.mark.timeout(900)
def test_gradient_kernels_fit_their_budgets_without_scratch(tmp_path):
    usage = resource_usage("exact_grad.hip", tmp_path)
    src = open(os.path.join(CSRC, "exact_grad.hip")).read()
    cols = int(re.search(r"constexpr int EG_COLS = (\d+);", src).group(1))
    assert "sizeof(double) * 2 * EG_COLS * d" in src                       # the largest dynamic request of the build's launcher
    build = {k: v for k, v in usage.items() if "exact_grad_build_kernel" in k}
    finish = {k: v for k, v in usage.items() if "exact_grad_finish_kernel" in k}
    assert len(build) == 2 and len(finish) == 1, sorted(usage)              # <true>, <false>; the finish
    for group, budget, dynamic in ((build, 256, 8 * 2 * cols * GPX_MAX_D), (finish, 128, 0)):
        for name, u in group.items():
            print(name, u, "dynamic LDS at d = 64:", dynamic)
            assert u["ScratchSize"] == 0, (name, u)
            assert u["VGPRs"] + u.get("AGPRs", 0) <= budget, (name, u)
            assert 2 * (u["LDS"] + dynamic) <= LDS_PER_CU, (name, u)        # two workgroups per CU
