"""The host logic of the left-looking solve (slab order, workspace arithmetic, the image that does not fit, which calls take the route, the
rerun of a chunk whose status word is raised) as a stand-alone program
under the host sanitizers: tools/native/replay_left.hip compiles csrc/tsolve.hip and csrc/emu.hip with every launch replaced by a check
that the launch stays inside the blocks the driver took.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scikit-gpuppy_amd", "csrc")


def test_replay_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "replay_left")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, '-DTSOLVE_PATH="%s"' % os.path.join(CSRC, "tsolve.hip"),
           '-DEMU_PATH="%s"' % os.path.join(CSRC, "emu.hip"), os.path.join(ROOT, "tools", "native", "replay_left.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    assert out.strip().endswith("ok (0 failed checks, 0 wrong results)") and "runtime error" not in r.stderr and "ERROR" not in r.stderr
    # the flagship shape: two equal row tiles, 55 + 55 bits, slabs 4 .. 15 emulated with one int8 launch per row tile
    c3 = out.split("== rows 16384 npad 16384 tile_rows 0 budget -1")[1].split("==")[0]
    assert "2 tile(s) of 8192 rows" in c3 and "abits 55 bbits 55" in c3
    assert c3.count("  int8 32 x 4 tiles") == 2 * 12 and c3.count("  split B") == 12 and c3.count("  split slab") == 2 * 15
    assert out.count("no room") == 3
    assert out.count("pass(es)") == 8 and "use_left 1 status 1 error 0: 2 pass(es)" in out      # the guard: every combination, one rerun
