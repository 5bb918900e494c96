"""The plan's table block (visual-slam_amd/csrc/plan_tables.h) built and walked on the host, under AddressSanitizer and UBSan: every
table aligned and inside the block, every tile and strip entry inside its level's tiling, the prefix sums of the blur tables."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", path, os.path.join(ROOT, "tests", "native", "plan_check.cpp")])
    return path


# (w, h, nfeatures, scale_factor, nlevels, edge_threshold, max_batch) -> describe tiles
@pytest.mark.parametrize("case,dtiles", [
    ((96, 80, 100, 1.2, 3, 31, 4), 2),       # level 2 (67 x 56) has no border region: no strips, no describe tiles on it
    ((160, 120, 300, 1.2, 4, 31, 4), None),
    ((333, 96, 300, 2.0, 2, 31, 4), None),   # level 1 is 166 wide from 333: the gather resize
    ((64, 64, 300, 1.2, 2, 32, 1), 0),       # no level has a border region (at 31 level 0 keeps one of 2 x 2)
    ((64, 64, 300, 1.2, 8, 31, 1), 1),
    ((640, 480, 2000, 1.2, 8, 31, 1), None),
    ((640, 480, 2000, 1.2, 8, 19, 8), None), # blur margin 0: both blur tables alike
    ((4095, 4095, 5000, 1.2, 12, 31, 1), None),
])
def test_block_walk(exe, case, dtiles):
    out = subprocess.run([exe, *map(str, case)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    line = out.stdout.strip().splitlines()[-1]
    assert line.startswith("plan %dx%d levels %d " % (case[0], case[1], case[4])) and line.endswith(" bad 0"), line
    if dtiles is not None:
        assert " dtiles %d " % dtiles in line
