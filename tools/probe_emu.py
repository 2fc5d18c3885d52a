"""The int8 residue product of the emulated update (csrc/emu.hip) alone at the C3 deep-update shape, against the vendor int8 GEMM
(torch._int_mm, this script only).  Usage: python tools/probe_emu.py [rows cols K [warm_seconds]]
warm_seconds > 0: that long of back-to-back 16-modulus launches first, so that the timed launches see the clock the chip settles at."""
import ctypes
import os
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scikit-gpuppy_amd")]
import torch  # noqa: E402
from skgpuppy_amd import _gpx  # noqa: E402

rows, cols, K = (int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (16384, 8192, 8192)
warm = float(sys.argv[4]) if len(sys.argv) > 4 else 0.0
t_end = time.perf_counter() + warm
while time.perf_counter() < t_end:
    ms = ctypes.c_double()
    _gpx.check(_gpx.lib.gpx_bench_emu_i8(rows, cols, K, 16, 8, ctypes.byref(ms)), "gpx_bench_emu_i8")
for nmod, iters in ((1, 40), (16, 4), (16, 8)):
    ms = ctypes.c_double()
    _gpx.check(_gpx.lib.gpx_bench_emu_i8(rows, cols, K, nmod, iters, ctypes.byref(ms)), "gpx_bench_emu_i8")
    print("emu_i8_gemm_kernel %dx%dx%d x %2d moduli: %8.3f ms/launch  %.3f POPS" % (rows, cols, K, nmod, ms.value, 2.0 * rows * cols * K * nmod / ms.value * 1e-12))
try:
    a = torch.randint(-128, 128, (rows, K), dtype=torch.int8, device="cuda")
    b = torch.randint(-128, 128, (cols, K), dtype=torch.int8, device="cuda").t()
    for _ in range(3):
        torch._int_mm(a, b)
    torch.cuda.synchronize()
    n = 20
    t0 = time.perf_counter()
    for _ in range(n):
        torch._int_mm(a, b)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    print("vendor torch._int_mm %dx%dx%d: %8.3f ms  %.3f POPS" % (rows, cols, K, dt * 1e3, 2.0 * rows * cols * K / dt * 1e-15))
except Exception as e:   # not every torch build has an int8 GEMM
    print("vendor torch._int_mm: not available (%s)" % e)
