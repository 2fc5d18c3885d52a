"""The clock the chip holds inside emu_i8_gemm_kernel (csrc/emu.hip) and the cycles of its k loop and of its epilogue per tile, from
in-kernel s_memtime / s_memrealtime stamps.

Needs a diagnostic library built with -DEMU_STAMP (never the shipped one), for instance
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -DEMU_STAMP [-DEMU_MFMA_16=1] -c emu.hip -o emu_stamp.o   and the link line of csrc/Makefile
with emu_stamp.o in place of emu.o, named by GPX_LIB.  Two seconds of warm launches, one timed call, then the stamps of every workgroup:
{cycles, 100 MHz ticks} before the k loop, after it, and (libraries with gpx_emu_stamp_width) at kernel exit once the stores have landed.
Usage: GPX_LIB=.../libgpx.so python tools/probe_emu_clock.py rows cols K [K ...]"""
import ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scikit-gpuppy_amd")]
import numpy as np
import torch  # noqa
from skgpuppy_amd import _gpx
rows, cols = (int(v) for v in sys.argv[1:3])
f = _gpx.lib.gpx_emu_stamps
f.restype = ctypes.c_int
f.argtypes = [ctypes.c_void_p, ctypes.c_int]
width = _gpx.lib.gpx_emu_stamp_width() if hasattr(_gpx.lib, "gpx_emu_stamp_width") else 4
tag = os.path.basename(os.path.dirname(os.environ.get("GPX_LIB", "")))
for K in (int(v) for v in sys.argv[3:]):
    ms = ctypes.c_double()
    t_end = time.perf_counter() + 2.0
    while time.perf_counter() < t_end:
        _gpx.check(_gpx.lib.gpx_bench_emu_i8(rows, cols, K, 16, 8, ctypes.byref(ms)), "bench")
    _gpx.check(_gpx.lib.gpx_bench_emu_i8(rows, cols, K, 16, 8, ctypes.byref(ms)), "bench")
    n = rows // 256 * (cols // 256) * 16
    buf = np.zeros((n, width), np.uint64)
    assert f(buf.ctypes.data, n) == 0
    dc = (buf[:, 1] - buf[:, 0]).astype(np.float64)
    dr = (buf[:, 3] - buf[:, 2]).astype(np.float64)
    ok = dr > 0
    ghz = dc[ok] / dr[ok] * 0.1
    line = ("%s %dx%dx%d x16: %.3f ms/launch; k loop per workgroup: %.1f us, %.0f cycles (medians, 100 MHz counter), clock median %.3f GHz, "
            "5%%..95%% %.3f..%.3f GHz, %d workgroups" % (tag, rows, cols, K, ms.value, np.median(dr[ok]) * 0.01, np.median(dc[ok]), np.median(ghz),
                                                         np.percentile(ghz, 5), np.percentile(ghz, 95), ok.sum()))
    if width >= 6:
        ec = (buf[:, 4] - buf[:, 1]).astype(np.float64)[ok]
        er = (buf[:, 5] - buf[:, 3]).astype(np.float64)[ok]
        line += "; epilogue to the last store: %.0f cycles, %.2f us (medians; 5%%..95%% %.0f..%.0f cycles)" % (
            np.median(ec), np.median(er) * 0.01, np.percentile(ec, 5), np.percentile(ec, 95))
    print(line, flush=True)
