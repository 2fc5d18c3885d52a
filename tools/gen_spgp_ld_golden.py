#!/usr/bin/env python
"""Writes tests/golden/spgp_ld.npz: the long-double values (tests/_spgp_ld.py) of the SPGP cases of tests/test_spgp_bounds.py that are too
slow to evaluate inside a test (m > 130 or N > 1500: 6 s to 40 s each on one core).

Per case: nll, the gradient, the 77 predictions (mean less mean(t), variance), all rounded to float64, and the SHA-256 of the seeded
inputs' bytes, which the test checks before it uses the values.  CPU only; the archive is written with fixed member dates and no
compression, so a second run reproduces the committed file bit for bit.

    python tools/gen_spgp_ld_golden.py [--check]      (--check: compare with the committed file instead of writing it)
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _spgp_ld as ld  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "spgp_ld.npz")

# name: (N, d, m), (wlo, whi, jit)
CASES = {
    "n300_d3_m520": ((300, 3, 520), (2.0, 8.0, 0.3)),
    "n300_d9_m520": ((300, 9, 520), (2.0, 8.0, 0.3)),
    "n300_d9_m520_wide": ((300, 9, 520), (0.05, 0.2, 0.3)),
    "n200_d3_m1030": ((200, 3, 1030), (2.0, 8.0, 0.3)),
    "n16384_d3_m130": ((16384, 3, 130), (0.5, 2.0, 0.05)),
}


def build():
    out = {}
    for name, ((N, d, m), recipe) in CASES.items():
        x, t, theta, xs = ld.make_case(N, d, m, *recipe)
        val = ld.evaluate(x, t, theta, m, xs)
        out[name + "__nll"] = np.array(np.float64(val["nll"]))
        for key in ("grad", "mean", "var"):
            out[name + "__" + key] = val[key].astype(np.float64)
        out[name + "__sha256"] = np.array(ld.input_hash(x, t, theta, xs))
        print(name, "nll %.17g" % out[name + "__nll"], flush=True)
    return out


def serialise(arrays):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for key in sorted(arrays):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asarray(arrays[key]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue())
    return buf.getvalue()


def main():
    data = serialise(build())
    if "--check" in sys.argv:
        with open(OUT, "rb") as f:
            same = f.read() == data
        print("identical" if same else "DIFFERENT")
        return 0 if same else 1
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "wb") as f:
        f.write(data)
    print(OUT, len(data), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
