"""The FAST arc network of k_fast on raw circle pixels (visual-slam_amd/csrc/fast_score.h), compiled for the host with
std::min / std::max, against the oracle's corner test and cornerScore: 10^6 random circles plus every bright / dark circle mask
at contrasts t - 1, t, t + 1, all-equal circles and 0 / 255 extremes, at thresholds 0, 1, 7, 20 and 254."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")
def test_fast_network_matches_oracle(tmp_path):
    exe = str(tmp_path / "fast_network_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "fast_network_check.cpp")])
    out = subprocess.run([exe, "1000000", "20261016"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("mismatches 0"), out.stdout
