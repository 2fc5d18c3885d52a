"""The clock the chip holds inside emu_i8_gemm_kernel's k loop (csrc/emu.hip), from in-kernel s_memtime / s_memrealtime stamps.

Needs a diagnostic library built with -DEMU_STAMP (never the shipped one), for instance
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -DEMU_STAMP -c emu.hip -o emu_stamp.o   and the link line of csrc/Makefile
with emu_stamp.o in place of emu.o, named by GPX_LIB.  Two seconds of warm launches, one timed call, then the stamps of every workgroup.
Usage: GPX_LIB=.../libgpx.so python tools/probe_emu_clock.py rows cols K"""
import ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scikit-gpuppy_amd")]
import numpy as np
import torch  # noqa
from skgpuppy_amd import _gpx
rows, cols, K = (int(v) for v in sys.argv[1:4])
ms = ctypes.c_double()
t_end = time.perf_counter() + 2.0
while time.perf_counter() < t_end:
    _gpx.check(_gpx.lib.gpx_bench_emu_i8(rows, cols, K, 16, 8, ctypes.byref(ms)), "bench")
_gpx.check(_gpx.lib.gpx_bench_emu_i8(rows, cols, K, 16, 8, ctypes.byref(ms)), "bench")
n = rows // 256 * (cols // 256) * 16
buf = np.zeros((n, 4), np.uint64)
f = _gpx.lib.gpx_emu_stamps
f.restype = ctypes.c_int
f.argtypes = [ctypes.c_void_p, ctypes.c_int]
assert f(buf.ctypes.data, n) == 0
dc = (buf[:, 1] - buf[:, 0]).astype(np.float64)
dr = (buf[:, 3] - buf[:, 2]).astype(np.float64)
ok = dr > 0
ghz = dc[ok] / dr[ok] * 0.1
print("%s %dx%dx%d x16: %.3f ms/launch; k loop per workgroup: %.1f us (median, 100 MHz counter), clock median %.3f GHz, 5%%..95%% %.3f..%.3f GHz, %d workgroups"
      % (os.path.basename(os.path.dirname(os.environ.get("GPX_LIB", ""))), rows, cols, K, ms.value, np.median(dr[ok]) * 0.01, np.median(ghz), np.percentile(ghz, 5), np.percentile(ghz, 95), ok.sum()))
