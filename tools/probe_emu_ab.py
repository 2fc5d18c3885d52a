"""One arm of an A/B of emu_i8_gemm_kernel alone (csrc/emu.hip): gpx_bench_emu_i8 on random residues, 16 moduli, 20 launches per figure,
after one second of warm launches.  The library is the in-tree one or GPX_LIB; run the arms as separate processes, interleaved.
Usage: [GPX_LIB=.../libgpx.so] python tools/probe_emu_ab.py TAG rows cols K [K ...]"""
import ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scikit-gpuppy_amd")]
import torch  # noqa
from skgpuppy_amd import _gpx
tag, rows, cols = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
ms = ctypes.c_double()
t_end = time.perf_counter() + 1.0
while time.perf_counter() < t_end:
    _gpx.check(_gpx.lib.gpx_bench_emu_i8(rows, cols, 8192, 16, 8, ctypes.byref(ms)), "bench")
for K in (int(v) for v in sys.argv[4:]):
    _gpx.check(_gpx.lib.gpx_bench_emu_i8(rows, cols, K, 16, 20, ctypes.byref(ms)), "bench")
    print("%-8s %dx%dx%d x16: %8.1f us/launch  %.3f POPS" % (tag, rows, cols, K, ms.value * 1e3, 2.0 * rows * cols * K * 16 / ms.value * 1e-12), flush=True)
