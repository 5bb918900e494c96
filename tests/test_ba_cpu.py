"""Bundle adjustment without a GPU: the numpy restatement of mo_map_bundle_adjust's rules (tests/ba_restatement.py) on the constructed
scene (tests/ba_scene.py), the rules on small arrays, the host build of csrc/ba.h, and the header <-> ctypes layout of the new structs."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.ba_restatement import add_observations, bundle_adjust, problem
from tests.ba_scene import K, Scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Recovery of the noise-free scene (f32 keypoints, f32 start positions): the restatement reaches 5.9e-7 on the pose entries and
# 1.58e-5 on the point coordinates (the points at up to 12 units of depth, seen over a 0.35 baseline).  The bounds are 10 x that - the
# margin covers a different summation order, nothing more.  The GPU test takes them from here.
RECOVERY_BOUND = (5.9e-6, 1.58e-4)
# Noise and outliers: 0.5 px Gaussian noise, scene seed 21, moved edges seed 9: the restatement flags 169 of 169 moved edges and 6 of
# 3026 untouched ones (0.2 %).
NOISE, NOISE_SEED = 0.5, 21


def test_restatement_recovers_the_noise_free_scene():
    """measured: pose error 4.2e-2 -> 5.9e-7, point error 0.43 -> 1.58e-5, cost 1.06e5 -> 9.4e-8, steps [5, 1], all accepted"""
    s = Scene()
    poses, xyz = s.perturbed()
    r = s.restate(poses, xyz)
    loc = ~np.isnan(r["points"][:, 0])
    e_pose, e_pt = s.pose_error(r["poses"]), float(np.abs(r["points"][loc] - s.X[loc]).max())
    print("pose error %.3g -> %.3g, point error %.3g -> %.3g, cost %s, steps %s accepted %s"
          % (s.pose_error(poses), e_pose, np.abs(xyz[loc] - s.X[loc]).max(), e_pt, r["cost"], r["steps"], r["accepted"]))
    assert r["ok"] and r["free"] == [2, 3, 4, 5, 6, 7] and r["fixed"] == [0, 1]
    assert r["cost"][2] < 1e-6 * r["cost"][0] and not (r["edge_inlier"] == 2).any()
    assert r["n_inliers"] == r["n_edges"] == (r["edge_inlier"] == 1).sum()
    assert e_pose < RECOVERY_BOUND[0] and e_pt < RECOVERY_BOUND[1]
    assert np.array_equal(r["xyz"][loc], r["points"][loc].astype(np.float32)) and np.array_equal(r["xyz"][~loc], xyz[~loc])
    for k in r["fixed"]:
        assert np.array_equal(r["poses"][k], poses[k][:3, :4])


def test_restatement_with_noise_and_outliers():
    s = Scene(pixel_noise=NOISE, seed=NOISE_SEED)
    poses, xyz = s.perturbed()
    r = s.restate(poses, xyz)
    print("noise: pose error %.3g -> %.3g" % (s.pose_error(poses), s.pose_error(r["poses"])))
    assert r["ok"] and s.pose_error(r["poses"]) < s.pose_error(poses)
    moved = s.move_edges()
    r = s.restate(poses, xyz)
    ei = r["edge_inlier"]
    clean = ~moved & (ei > 0)
    print("outliers: %d of %d moved flagged, %d of %d untouched flagged" % ((ei[moved] == 2).sum(), moved.sum(), (ei[clean] == 2).sum(), clean.sum()))
    assert r["ok"] and (ei[moved] == 2).all() and (ei[clean] == 2).sum() <= 0.01 * clean.sum()


def _csr(obs):
    off, okf, okp = [0], [], []
    for o in obs:
        for k, r in o:
            okf.append(k); okp.append(r)
        off.append(len(okf))
    return np.array(off, np.int32), np.array(okf, np.int32), np.array(okp, np.int32)


def test_window_gauge_and_validity_rules():
    counts = np.array([10] * 6)
    # points: seen by (0, 1), (1, 2, 3), (3, 4, 5), (4, 5), one edge only, an entry naming nothing + 2 valid through negative indices
    off, okf, okp = _csr([[(0, 1), (1, 1)], [(1, 2), (2, 2), (3, 2)], [(3, 3), (4, 3), (5, 3)], [(4, 4), (5, 4)], [(5, 5)],
                          [(9, 0), (-1, -1), (-2, 10), (-3, 0)]])
    local, free, fixed, edges = problem(off, okf, okp, counts, 10)
    assert local.tolist() == [True, True, True, True, False, True] and edges[5] == [(5, 9, 12), (3, 0, 14)]
    assert fixed == [0, 1] and free == [2, 3, 4, 5]                      # position 0 never free, the gauge takes position 1
    local, free, fixed, _ = problem(off, okf, okp, counts, 2)            # candidates 4, 5
    assert local.tolist() == [False, False, True, True, False, True] and fixed == [3, 4] and free == [5]
    local, free, fixed, _ = problem(off, okf, okp, counts, 1)            # candidate 5; fixed 3, 4
    assert fixed == [3, 4] and free == [5]
    # a single keyframe pair: both fixed by the gauge, nothing free
    off2, okf2, okp2 = _csr([[(0, 1), (1, 1)]] * 3)
    assert problem(off2, okf2, okp2, np.array([5, 5]), 10)[1] == []
    with pytest.raises(ValueError):
        problem(off, okf, okp, np.array([10] * 18), 0)                   # 17 candidates
    problem(off, okf, okp, np.array([10] * 17), 0)
    with pytest.raises(ValueError):
        problem(off, okf, okp, np.array([10] * 40), 17)


def test_empty_cases():
    z = np.zeros(0, np.int32)
    r = bundle_adjust(np.zeros(1, np.int32), z, z, np.zeros(0, np.int32), [], [], np.zeros((0, 3), np.float32), K, np.zeros((0, 3, 4)))
    assert not r["ok"] and r["steps"] == [0, 0]
    off, okf, okp = _csr([[(0, 1)], [(1, 1)]])                           # no point with two edges
    T = np.tile(np.eye(4)[:3], (2, 1, 1))
    xy = [np.zeros((5, 2), np.float32)] * 2
    r = bundle_adjust(off, okf, okp, np.array([5, 5]), xy, [np.zeros(5, int)] * 2, np.ones((2, 3), np.float32), K, T)
    assert not r["ok"] and r["n_local"] == 0 and np.isnan(r["points"]).all() and np.array_equal(r["poses"], T)


def test_add_observations_rules():
    counts = np.array([10, 10, 10])
    off, okf, okp = _csr([[(0, 1), (1, 1)], [(1, 2), (2, 2)], [], [(2, 30), (0, 3)]])
    point = np.array([1, -1, 7, 0, 0, 3, 2])
    row = np.array([5, 6, 7, 8, 9, 4, 3])
    o2, k2, p2 = add_observations(off, okf, okp, counts, 2, point, row)
    # point 1 has a valid observation in 2: skipped; -1 and 7: skipped; point 0 gains row 8 (the lower entry wins); point 3's entry in
    # 2 names row 30 of 10: not valid, so it gains (2, 4) at the end; point 2 gains its first
    assert o2.tolist() == [0, 3, 5, 6, 9]
    assert k2.tolist() == [0, 1, 2, 1, 2, 2, 2, 0, 2] and p2.tolist() == [1, 1, 8, 2, 2, 3, 30, 3, 4]
    o3, k3, p3 = add_observations(off, okf, okp, counts, 3, point)   # the next keyframe; rows default to the entry index
    assert np.diff(o3).tolist() == [3, 3, 1, 3] and k3[o3[1:] - 1].tolist() == [3, 3, 3, 3] and p3[o3[1:] - 1].tolist() == [3, 0, 6, 5]
    with pytest.raises(ValueError):
        add_observations(off, okf, okp, counts, 4, point)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")
def test_ba_native_cpu(tmp_path):
    exe = str(tmp_path / "ba_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "native", "ba_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("ok ") == 6 and "FAIL" not in out.stdout


def test_struct_layouts_and_symbols(tmp_path):
    import vslam_amd as V
    structs = [("mo_map_ba_params", V.MapBaParams), ("mo_map_ba_out", V.MapBaOut)]
    body = ""
    for cname, cls in structs:
        body += '  printf("%%zu\\n", sizeof(%s));\n' % cname
        body += "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0].rstrip("_")) for f in cls._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vslam_amd.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    k = 0
    for cname, cls in structs:
        assert got[k] == C.sizeof(cls), cname
        offs = [getattr(cls, f[0]).offset for f in cls._fields_]
        assert got[k + 1:k + 1 + len(offs)] == offs, cname
        k += 1 + len(offs)
    lib = V.load_library()
    assert hasattr(lib, "mo_map_bundle_adjust") and hasattr(lib, "mo_map_add_observations")
    from vslam_amd.mapper import LocalMapper
    import inspect
    assert "tracked" in inspect.signature(LocalMapper.add_keyframe).parameters and hasattr(LocalMapper, "bundle_adjust")
