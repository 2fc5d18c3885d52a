"""The host logic of the other two emulated-update drivers (csrc/emu.hip: the recursion's emu_gemm_nt_sub and the factorisation's symmetric
update emu_syrk_split / emu_syrk_panel) as a stand-alone program under the host sanitizers: tools/native/replay_left.hip, run with the
argument `drives`, compiles csrc/tsolve.hip and csrc/emu.hip with every launch replaced by a check that the launch stays inside the
blocks the driver took, that its grid matches the tile counts and that the symmetric update's B window lies inside the image on a
1024-row boundary of a row tile (tests/test_left_driver_replay.py is the left-looking solve's).  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scikit-gpuppy_amd", "csrc")


@pytest.fixture(scope="module")
def drives(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("replay") / "replay_drives")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, '-DTSOLVE_PATH="%s"' % os.path.join(CSRC, "tsolve.hip"),
           '-DEMU_PATH="%s"' % os.path.join(CSRC, "emu.hip"), os.path.join(ROOT, "tools", "native", "replay_left.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("GPX_") and k != "REPLAY_LOG"}   # the counts below are the defaults'
    r = subprocess.run([exe, "drives"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "ERROR" not in r.stderr
    return r.stdout


def _section(out, head):
    assert out.count("== " + head + "\n") == 1, head
    return out.split("== " + head + "\n")[1].split("==")[0]


def _counts(sec):
    return tuple(sec.count(s) for s in ("  split A", "  split B", "  int8 ", "  rebuild "))


def test_every_check_held(drives):
    assert drives.strip().endswith("ok (0 failed checks, 0 wrong results)") and "CHECK FAILED" not in drives
    assert drives.count("\nrc 0\n") == 4 + 2 * 4 and drives.count("\nrc -2\n") == 2


def test_rectangular_update_tilings(drives):
    # emu_cap = 1024 at K = 130944 with 16 moduli: 2 row tiles x 2 column tiles, A split once per row tile, B once per pair
    sec = _section(drives, "gemm 1100 x 1060 x 130944")
    assert _counts(sec) == (2, 4, 4, 4)
    for shape in ("4 x 4", "4 x 1", "1 x 4", "1 x 1"):
        assert sec.count("  int8 %s tiles, K 130944, lda 130944" % shape) == 1
    assert sec.count("  rebuild 1024 x 1024") == 1 and sec.count("  rebuild 76 x 36") == 1
    # one row tile of 46080; 46080 x 3072 x 16 bytes of product residues pass 2^31, so the column tile shrinks to 2816: 2 column tiles
    sec = _section(drives, "gemm 46000 x 3000 x 128")
    assert _counts(sec) == (1, 2, 2, 2)
    assert "  split A 46080 x 128" in sec and "  split B 2816 x 128" in sec and "  split B 256 x 128" in sec
    assert "  int8 180 x 11 tiles" in sec and "  int8 180 x 1 tiles" in sec and "  rebuild 46000 x 2816" in sec and "  rebuild 46000 x 184" in sec
    # the C3 recursion's deepest update: one tile of each
    sec = _section(drives, "gemm 16384 x 8192 x 8192")
    assert _counts(sec) == (1, 1, 1, 1) and "  int8 64 x 32 tiles, K 8192, lda 8192" in sec and "  rebuild 16384 x 8192" in sec
    # ragged on both sides: residues padded to 512 x 256, 300 x 200 rebuilt
    sec = _section(drives, "gemm 300 x 200 x 4096")
    assert _counts(sec) == (1, 1, 1, 1) and "  split A 512 x 4096" in sec and "  split B 256 x 4096" in sec
    assert "  int8 2 x 1 tiles" in sec and "  rebuild 300 x 200" in sec


@pytest.mark.parametrize("dt", [1, 32])
def test_symmetric_update_tilings(drives, dt):
    # one row tile, 8 column panels: one split (the scales' launch and the residues'), then a product and a rebuild per panel
    sec = _section(drives, "syrk rows 8192 K 4096 tile_rows 0 diag_tile %d plan_rows 0 budget -1" % dt)
    assert "1 tile(s) of 8192 rows" in sec and _counts(sec) == (1, 0, 8, 8) and sec.count("  B scales 8192 x 4096") == 1
    assert [sec.count("  int8 %d x 4 tiles" % tm) for tm in (32, 28, 24, 20, 16, 12, 8, 4)] == [1] * 8
    # 3 row tiles (1024, 1024, 256), 3 column panels over the tiles at and below them: 3 + 2 + 1; panels 1 and 2 take B from tiles 1 and 2
    sec = _section(drives, "syrk rows 2304 K 4096 tile_rows 1024 diag_tile %d plan_rows 0 budget -1" % dt)
    assert "3 tile(s) of 1024 rows" in sec and _counts(sec) == (3, 0, 6, 6)
    assert sec.count("  int8 4 x 4 tiles") == 3 and sec.count("  int8 1 x 4 tiles") == 2 and sec.count("  int8 1 x 1 tiles") == 1
    assert sec.count("  rebuild 1024 x 1024") == 3 and sec.count("  rebuild 256 x 1024") == 2 and sec.count("  rebuild 256 x 256") == 1
    # ragged rows and a ragged last panel
    sec = _section(drives, "syrk rows 1100 K 512 tile_rows 0 diag_tile %d plan_rows 0 budget -1" % dt)
    assert "1 tile(s) of 1280 rows" in sec and _counts(sec) == (1, 0, 2, 2)
    assert "  int8 5 x 4 tiles" in sec and "  rebuild 1100 x 1024" in sec and "  int8 1 x 1 tiles" in sec and "  rebuild 76 x 76" in sec
    # the fit's order: reserved and allocated for 28672 rows, the plan of 8192 rows used before the split -- the geometry of 8192 rows
    sec = _section(drives, "syrk rows 8192 K 4096 tile_rows 0 diag_tile %d plan_rows 28672 budget -1" % dt)
    assert "1 tile(s) of 8192 rows, image 536870912 bytes" in sec and _counts(sec) == (1, 0, 8, 8)
    # a pool with room for the image alone: refused, and the image has gone back
    sec = _section(drives, "syrk rows 8192 K 4096 tile_rows 0 diag_tile %d plan_rows 0 budget %d" % (dt, 8192 * 4096 * 16 + 4096))
    assert "no room: rc -2, 0 blocks held" in sec and _counts(sec) == (0, 0, 0, 0)
