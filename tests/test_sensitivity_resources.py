"""The pair kernel of the variance decomposition (scikit-gpuppy_amd/csrc/sensitivity.hip, sens_pair_kernel) keeps 17 accumulators and eight
exponentials in flight per lane.  It is bound by fp64 vector issue and must neither spill (scratch traffic in the inner loop) nor grow past
128 vector registers, the budget it is launched for: two workgroups per CU by its LDS footprint, with room for four waves per SIMD.  This
test compiles the source for gfx950 with -Rpass-analysis=kernel-resource-usage (no GPU needed), as tests/test_kernel_resources.py does,
and checks both instantiations (with and without the total-effect sums)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scikit-gpuppy_amd", "csrc")


def resource_usage(src, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, src), "-o",
                          str(tmp_path / (src + ".o")), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return usage


@pytest.mark.timeout(900)
def test_pair_kernel_fits_its_register_budget_without_scratch(tmp_path):
    usage = resource_usage("sensitivity.hip", tmp_path)
    pair = {k: v for k, v in usage.items() if "sens_pair_kernel" in k}
    assert len(pair) == 2, sorted(usage)                      # <true> and <false>
    for name, u in pair.items():
        print(name, u)
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 128, (name, u)
        assert 2 * u["LDS"] <= 160 * 1024, (name, u)          # two workgroups per CU
