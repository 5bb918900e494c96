"""The homography branch of the two-view stage without a device: the header (visual-slam_amd/csrc/homography.h) compiled for the host,
and the numpy restatement (tests/hf_restatement.py) on the scenes of tests/hf_cases.py against ground truth.

Header tolerances: the closed-form four-point H is measured against numpy's SVD solution of the same four correspondences and may
differ from it by ten times the difference between two formulations of numpy's own solution (SVD of the 8x9 design matrix, eigh of
its normal matrix), both taken as the worst case over the same 10^5 quadruples; both figures are recorded in profiles/hf_parity.txt.

Pose bounds on the planes (the way tests/test_oracle_geom.py derives its own): a homography fitted to N inliers with sigma = 0.5 px
of noise per coordinate has its transfer map known to about sigma / sqrt(N / 4) px (8 parameters, 2 N equations); the decomposition
turns a transfer error of e px over an image half-width of w px into an angle of e / w for R and, for t, that angle divided by the
motion's own signal t / d (baseline over plane distance, 1 / 8 here, times the focal length in pixels).  With N = 200, w = 320, f = 320:
e = 0.07 px, dR = 2.2e-4 rad, dt = e / (f / 8) = 1.8e-3.  The bounds below take five times that (a 5-sigma event per case), and they
sit two orders of magnitude below what the essential path returns on the same scenes (0.1 in R, more than 0.9 in t), which is what the
capability test shows.  Noise-free cases are bounded by the float32 pixel rounding instead (2^-24 x 640 px = 4e-5 px -> 1e-6)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import hf_cases as C
from tests import hf_restatement as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")

R_BOUND, T_BOUND = 5 * 2.2e-4, 5 * 1.8e-3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("hf") / "homography_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", path, os.path.join(ROOT, "tests", "native", "homography_check.cpp")])
    return path


def _run(exe, *args):
    out = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def _unit_fixed(H):
    H = H / np.linalg.norm(H, axis=(-2, -1), keepdims=True)
    k = np.argmax(np.abs(H.reshape(len(H), 9)), axis=1)
    return H * np.sign(H.reshape(len(H), 9)[np.arange(len(H)), k])[:, None, None]


def _design4(p):
    """(n, 4, 4) correspondences -> (n, 8, 9) DLT design matrices in Hartley-normalised coordinates, and the normalisations"""
    x1, x2 = p[:, :, :2], p[:, :, 2:]
    out = []
    nms = []
    for x in (x1, x2):
        c = x.mean(axis=1, keepdims=True)
        s = np.sqrt(2.0) / np.sqrt(((x - c) ** 2).sum(axis=2)).mean(axis=1)
        out.append((x - c) * s[:, None, None])
        nms.append((s, c[:, 0, 0], c[:, 0, 1]))
    a, b = out
    z, o = np.zeros(a.shape[:2]), np.ones(a.shape[:2])
    r1 = np.stack([z, z, z, -a[..., 0], -a[..., 1], -o, b[..., 1] * a[..., 0], b[..., 1] * a[..., 1], b[..., 1]], axis=2)
    r2 = np.stack([a[..., 0], a[..., 1], o, z, z, z, -b[..., 0] * a[..., 0], -b[..., 0] * a[..., 1], -b[..., 0]], axis=2)
    return np.concatenate([r1, r2], axis=1), nms


def _denorm(Hn, nms):
    def T(nm, inv):
        s, cx, cy = nm
        M = np.zeros((len(s), 3, 3))
        if inv:
            M[:, 0, 0] = M[:, 1, 1] = 1.0 / s; M[:, 0, 2] = cx; M[:, 1, 2] = cy
        else:
            M[:, 0, 0] = M[:, 1, 1] = s; M[:, 0, 2] = -s * cx; M[:, 1, 2] = -s * cy
        M[:, 2, 2] = 1.0
        return M
    return T(nms[1], True) @ Hn @ T(nms[0], False)


@needs_gxx
def test_four_point_homography_recovers_h_within_ten_times_numpys_own_spread(exe, tmp_path):
    n = 100000
    dump = str(tmp_path / "h4.bin")
    line = _run(exe, "h4", n, 20261020, dump).strip().splitlines()[-1]
    assert line.startswith("h4 cases %d nomodel 0 " % n), line
    rec = np.fromfile(dump, np.float64).reshape(n, 25)
    A, nms = _design4(rec[:, :16].reshape(n, 4, 4))
    A9 = np.concatenate([A, np.zeros((n, 1, 9))], axis=1)  # a reduced SVD of 8 rows has no ninth right vector
    H_svd = _unit_fixed(_denorm(np.linalg.svd(A9)[2][:, -1, :].reshape(n, 3, 3), nms))
    H_eig = _unit_fixed(_denorm(np.linalg.eigh(np.einsum("nki,nkj->nij", A, A))[1][:, :, 0].reshape(n, 3, 3), nms))
    H_hdr = _unit_fixed(rec[:, 16:].reshape(n, 3, 3))
    e_hdr = float(np.abs(H_hdr - H_svd).max())
    e_self = float(np.abs(H_eig - H_svd).max())
    print("header vs numpy SVD %.3e; numpy eigh vs numpy SVD %.3e; header vs the true H: %s" % (e_hdr, e_self, line))
    assert e_hdr <= 10.0 * e_self


@needs_gxx
def test_degenerate_samples_give_no_model(exe):
    assert _run(exe, "degenerate").strip().endswith("degenerate bad 0")


@needs_gxx
def test_decomposition_contains_the_truth(exe):
    """eight candidates from H = K (R + t n' / d) K^-1, one of them (R, t / |t|, n): 1e-9 leaves four orders of magnitude over the
    worst case seen (1.6e-13) and is far below any distance between two candidates"""
    out = _run(exe, "decompose", 20000, 5).strip()
    assert " failed 0 " in out, out
    assert float(out.split()[-1]) < 1e-9, out


@needs_gxx
def test_equal_singular_values_give_no_decomposition(exe):
    assert _run(exe, "rotation", 2000, 6).strip().endswith("rotation bad 0")


@needs_gxx
def test_the_four_sample_is_the_first_four_of_sample8(exe):
    from oracle.geom_oracle import sample8
    for seed, h, m, pair in [(4096, 0, 15, 0), (4096, 5, 100, 3), (123456789, 511, 2000, 7), (2 ** 63 + 5, 17, 9, 1), (4096, 3, 4, 0)]:
        s = (seed + pair * 0x632BE59BD9B4E019) % 2 ** 64
        got = [int(x) for x in _run(exe, "sample", s, h, m).split()]
        if m >= 8:
            assert got == sample8(seed, h, m, pair)[:4]
        else:
            assert sorted(got) == [0, 1, 2, 3]


def test_the_ctypes_mirror_has_the_headers_layout(tmp_path):
    """sizeof / offsetof of mo_hf_params and mo_hf_result as a C compiler sees include/vslam_amd.h == vslam_amd.HfParams / HfResult"""
    import ctypes
    import vslam_amd as V
    if shutil.which("gcc") is None:
        pytest.skip("needs a host C compiler")
    structs = [("mo_hf_params", V.HfParams), ("mo_hf_result", V.HfResult)]
    body = ""
    for cname, cls in structs:
        body += '  printf("%%zu\\n", sizeof(%s));\n' % cname
        body += "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0]) for f in cls._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vslam_amd.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    k = 0
    for cname, cls in structs:
        offs = [getattr(cls, f[0]).offset for f in cls._fields_]
        assert got[k] == ctypes.sizeof(cls) and got[k + 1:k + 1 + len(offs)] == offs, cname
        k += 1 + len(offs)


# ---- the restatement on the case list: ground-truth facts -----------------------------------------------------------------------------
def _clear_of_the_threshold(r, rh_threshold=0.40):
    return abs(r["RH"] - rh_threshold) >= 0.02  # a condition on the inputs: a decision this close to the threshold is not asserted


@pytest.mark.parametrize("name", [k for k, (_, e) in C.CASES.items() if e == "H"])
def test_planes_choose_the_homography_and_recover_the_pose(name):
    s, r = C.scene(name), C.restated(name)
    assert _clear_of_the_threshold(r), r["RH"]
    assert r["model"] == 1 and r["accepted"], (r["model"], r["accepted"], r["RH"])
    clean = C.CASES[name][0].get("noise_px", 0.0) == 0.0
    eR, et = C.rel_err(r["R"], s["R"]) / np.sqrt(3.0), C.rel_err(r["t"], s["t"])  # (|R|_F = sqrt 3: an angle in radians)
    print("%s: R %.2e t %.2e (essential path: R %.2e t %.2e)" % (name, eR, et, C.rel_err(r["R_e"], s["R"]) / np.sqrt(3.0), C.rel_err(r["t_e"], s["t"])))
    assert eR < (1e-6 if clean else R_BOUND) and et < (1e-6 if clean else T_BOUND)
    # the map points of the selected model lie on the true plane's points
    pm = r["pose_mask"] & ~s["outlier"]
    assert pm.sum() > 0.6 * (~s["outlier"]).sum()
    assert np.median(np.linalg.norm(r["X"][pm] - s["X"][pm], axis=1) / np.linalg.norm(s["X"][pm], axis=1)) < (1e-5 if clean else 10 * T_BOUND)


@pytest.mark.parametrize("name", [k for k, (_, e) in C.CASES.items() if e == "F"])
def test_general_scenes_choose_the_fundamental_matrix(name):
    r, e = C.restated(name), C.essential(name)
    assert _clear_of_the_threshold(r), r["RH"]
    assert r["model"] == 0 and r["accepted"]
    assert r["R"] is e["R"] and r["t"] is e["t"] and r["pose_mask"] is e["pose_mask"] and r["X"] is e["X"]  # the essential path's own result


@pytest.mark.parametrize("name", [k for k, (_, e) in C.CASES.items() if e == "reject"])
def test_pure_rotation_is_not_accepted(name):
    r = C.restated(name)
    assert not r["accepted"]
    # whichever model RH names: the homography's four d' > 0 candidates all pass with no parallax, the essential path triangulates nothing
    assert r["parallax_h"][r["best_h"]] < 0.5 and r["n_good_e"] <= 50


def test_the_eight_way_ambiguity_resolves_on_planes():
    for name, (_, e) in C.CASES.items():
        if e == "H":
            r = C.restated(name)
            g = np.sort(r["n_good_h"])[::-1]
            assert g[1] < 0.75 * g[0], (name, g)


@pytest.mark.parametrize("name", list(C.CASES))
def test_cases_keep_clear_of_every_threshold(name):
    """What the device comparison (tests/test_gpu_hf.py) presumes of its inputs: no compared error within 1e-9 relative of its
    threshold, and the best and second-best hypothesis costs more than 1e-6 apart (relative)."""
    r = C.restated(name)
    assert r["margin"] > 1e-9, r["margin"]
    c = np.sort(r["cost"].astype(np.float64))
    assert np.isfinite(c[0]) and (len(c) < 2 or c[1] - c[0] > 1e-6 * c[0]), c[:2]


def test_low_triangulation_counts_use_the_last_sorted_value():
    """m = 40: fewer than 51 passed points, so the parallax is the value at index count - 1; refused by min_triangulated = 50,
    accepted with 20"""
    r50, r20 = C.restated("plane_m40"), C.restated("plane_m40", min_triangulated=20)
    assert r50["model"] == 1 and 20 < r50["n_good"] <= 40
    assert not r50["accepted"] and r20["accepted"]
    s = C.scene("plane_m40")
    assert C.rel_err(r20["R"], s["R"]) < 1e-6 and C.rel_err(r20["t"], s["t"]) < 1e-5


def test_a_scene_on_one_line_has_no_homography():
    l = C.line_scene()
    r = HR.hf_two_view(l["p1"], l["p2"], l["K"], 3.0, C.N_HYP, C.SEED, C.N_HYP_H)
    assert r["winner_h"] == -1 and r["SH"] == 0.0 and r["RH"] == 0.0 and not np.isfinite(r["H"]).any()
    assert r["model"] in (0, -1) and (r["model"] == 0 or not r["accepted"])


def test_svd_and_eigh_formulations_agree():
    """the two formulations the parity bounds are measured with make the same decisions on every case"""
    for name in C.CASES:
        a, b = C.restated(name), C.restated(name, "eigh")
        assert a["model"] == b["model"] and a["winner_h"] == b["winner_h"] and np.array_equal(a["h_mask"], b["h_mask"]), name
        assert np.array_equal(a["n_good_h"], b["n_good_h"]) and np.array_equal(a["pose_mask"], b["pose_mask"]), name
