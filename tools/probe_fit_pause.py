"""fit_ms after a predict on either route (GPX_EMU_LEFT), with and without a pause between the predict and the next fit: one process per setting.
Usage: GPX_EMU_LEFT=0|1 python tools/probe_fit_pause.py PAUSE_SECONDS   (profiles/r12_left_looking.txt, section 4)"""
import ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scikit-gpuppy_amd")]
import numpy as np
import torch
import bench
from skgpuppy_amd import _gpx
pause = float(sys.argv[1])
wl = bench.WORKLOADS["c3"]
N, d, M = wl["N"], wl["d"], wl["M"]
x, t, xs, theta = bench.recipe(N, d, M)
dev = torch.device("cuda:0")
xd, td, xsd = (torch.as_tensor(a).to(dev) for a in (x, t - t.mean(), xs))
mean_d = torch.empty(M, dtype=torch.float64, device=dev); var_d = torch.empty_like(mean_d)
th = np.ascontiguousarray(theta)
vp = lambda tt: ctypes.c_void_p(tt.data_ptr())
torch.cuda.synchronize()
fits, preds = [], []
for i in range(9):
    h = ctypes.c_void_p()
    a = time.perf_counter()
    _gpx.check(_gpx.lib.gpx_fit(vp(xd), vp(td), N, d, _gpx.ptr(th), None, ctypes.byref(h)), "fit")
    b = time.perf_counter()
    _gpx.check(_gpx.lib.gpx_predict(h, vp(xsd), M, vp(mean_d), vp(var_d)), "predict")
    c = time.perf_counter()
    _gpx.lib.gpx_free(h)
    if pause: time.sleep(pause)
    if i >= 3: fits.append((b - a) * 1e3); preds.append((c - b) * 1e3)
print("GPX_EMU_LEFT=%s pause %.0f ms: fit_ms mean %.2f min %.2f max %.2f ; predict_ms mean %.2f" % (os.environ.get("GPX_EMU_LEFT", "1"), pause * 1e3,
      np.mean(fits), min(fits), max(fits), np.mean(preds)), flush=True)
