"""The plan's tile records (visual-slam_amd/csrc/plan_tables.h, plan_build_tile_records) built on the host and compared with the prologue the
blurring k_resize2 used to run, over a sweep of image sizes, edge thresholds, scale factors and level counts (tests/native/tile_records_check.cpp
states the sweep and the checks).  Built once plain and once under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_record_sweep(tmp_path, flags):
    exe = str(tmp_path / "tile_records_check")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "native", "tile_records_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    line = out.stdout.strip().splitlines()[-1]
    assert line.startswith("tile records: plans ") and line.endswith(" bad 0"), line
    words = line.split()
    # the sweep is not empty on any side: plans, fused levels, interior records and records whose window leaves the level
    for key in ("plans", "levels", "records", "fused", "interior", "border"):
        assert int(words[words.index(key) + 1]) > 0, line
