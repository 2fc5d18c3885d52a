"""emu_i8_gemm_kernel (csrc/emu.hip) runs one workgroup of 512 threads per CU: two waves per SIMD, so a wave may hold 256 registers at
the most (arch + accumulation, in granules of 8), nothing may spill, and the two stage buffers (which the epilogue reuses for its tile
image) must fit the CU's 160 KiB of LDS.  Compiled for gfx950 in both MFMA shapes with -Rpass-analysis=kernel-resource-usage; no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scikit-gpuppy_amd", "csrc")
FIELDS = r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs Spill|SGPRs Spill): (\d+)"


def product_kernel_usage(shape16, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DEMU_MFMA_16=%d" % shape16, "-c",
                          os.path.join(CSRC, "emu.hip"), "-o", str(tmp_path / ("emu%d.o" % shape16)), "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(FIELDS, line)
        if m and name and "emu_i8_gemm_kernel" in name:
            usage[m.group(1)] = int(m.group(2))
    assert {"VGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]"} <= set(usage), out.stderr[-2000:]
    return usage


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("shape16", [0, 1], ids=["mfma_32x32x32", "mfma_16x16x64"])
def test_product_kernel_fits_two_waves_per_simd(shape16, tmp_path):
    u = product_kernel_usage(shape16, tmp_path)
    print(shape16, u)
    assert u["ScratchSize [bytes/lane]"] == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, u
    assert (u["VGPRs"] + 7) // 8 * 8 + (u.get("AGPRs", 0) + 7) // 8 * 8 <= 256, u
    assert u["LDS Size [bytes/block]"] <= 160 * 1024, u
