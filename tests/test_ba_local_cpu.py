"""The set form of the local bundle adjustment and the observation erase without a GPU: the numpy restatement
(tests/ba_local_restatement.py, driving tests/ba_restatement's steps) on the revisit world (tests/ba_local_worlds.py) and on
tests/ba_scene.Scene, the gauge rules on small sets, and the header <-> ctypes layout of the new structs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import ba_local_restatement as LR
from tests import ba_local_worlds as LW
from tests.ba_restatement import problem
from tests.ba_scene import Scene
from tests.test_ba_cpu import NOISE, NOISE_SEED, RECOVERY_BOUND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


@pytest.mark.parametrize("window", [3, 6, 10])
def test_the_windows_set_gives_the_window_calls_result(window):
    s = Scene()
    poses, xyz = s.perturbed()
    lo = s.n_kf - window if 0 < window < s.n_kf else 0
    cand = [k for k in range(max(lo, 1), s.n_kf)]
    a = s.restate(poses, xyz, window=window)
    b = LR.restate_set(s, poses, xyz, cand)
    assert b.pop("candidates") == cand
    _equal(a, b)
    p0, p1 = problem(s.obs_off, s.obs_kf, s.obs_kp, s.counts, window), LR.problem_set(s.obs_off, s.obs_kf, s.obs_kp, s.counts, cand)
    assert np.array_equal(p0[0], p1[0]) and p0[1] == p1[1] and sorted(p0[2]) == sorted(p1[2])


def test_revisit_world_covisible_set_recovers_and_the_window_does_not():
    """measured: the set form ends at pose error 2.9e-7 and point error 1.04e-5 with 2472 of 2472 edges inliers; window=6 holds keyframes
    1 .. 4 fixed at their wrong poses, keeps 2418 of 3061 edges and moves the poses from 0.0368 to 0.0379 off the truth"""
    s = LW.Revisit()
    W = LR.covisibility(s.obs_off, s.obs_kf, s.obs_kp, s.counts)
    assert W[11].tolist() == LW.REVISIT_W11
    cand = LR.candidates(W)
    assert cand == LW.REVISIT_SET
    assert [k for k in range(6, 12)] == problem(s.obs_off, s.obs_kf, s.obs_kp, s.counts, 6)[1]
    poses, xyz = LW.perturbed_set(s, cand)
    r = LR.restate_set(s, poses, xyz, cand)
    loc = ~np.isnan(r["points"][:, 0])
    e_pose, e_pt = s.pose_error(r["poses"]), float(np.abs(r["points"][loc] - s.X[loc]).max())
    print("set form: free %s fixed %s, %d of %d edges inliers, pose error %.3g -> %.3g, point error %.3g, steps %s"
          % (r["free"], r["fixed"], r["n_inliers"], r["n_edges"], s.pose_error(poses), e_pose, e_pt, r["steps"]))
    assert r["ok"] and r["free"] == cand and r["n_inliers"] == r["n_edges"] and not (r["edge_inlier"] == 2).any()
    assert e_pose < RECOVERY_BOUND[0] and e_pt < RECOVERY_BOUND[1]
    w = s.restate(poses, xyz, window=6)
    print("window=6: free %s fixed %s, %d of %d edges inliers, pose error %.3g -> %.3g"
          % (w["free"], w["fixed"], w["n_inliers"], w["n_edges"], s.pose_error(poses), s.pose_error(w["poses"])))
    assert set(w["fixed"]) >= {1, 2, 3, 4} and w["n_inliers"] < w["n_edges"]
    assert s.pose_error(w["poses"]) > s.pose_error(poses)


def _csr(obs):
    off, okf, okp = [0], [], []
    for o in obs:
        for k, r in o:
            okf.append(k); okp.append(r)
        off.append(len(okf))
    return np.array(off, np.int32), np.array(okf, np.int32), np.array(okp, np.int32)


def test_candidate_and_gauge_rules():
    s = LW.Revisit()
    a = (s.obs_off, s.obs_kf, s.obs_kp, s.counts)
    _, free, fixed, _ = LR.problem_set(*a, [1, 2])
    assert free == [1, 2] and sorted(fixed) == [0, 3, 4, 10, 11]
    # a set none of whose points has an outside observer: its two lowest positions are the gauge
    counts = np.array([10] * 7)
    off, okf, okp = _csr([[(4, 1), (5, 1)], [(4, 2), (5, 2), (6, 2)], [(5, 3), (6, 3)], [(0, 4), (1, 4)], [(2, 5)]])
    local, free, fixed, _ = LR.problem_set(off, okf, okp, counts, [4, 5, 6])
    assert local.tolist() == [True, True, True, False, False] and fixed == [4, 5] and free == [6]
    # a candidate without an edge to a local point (3: no point at all; 2: a single-edge point) is outside the problem
    local, free, fixed, _ = LR.problem_set(off, okf, okp, counts, [2, 3, 4, 5, 6])
    assert fixed == [4, 5] and free == [6] and local.tolist() == [True, True, True, False, False]
    # nothing in C, or position 0 alone (dropped): nothing runs
    assert LR.mask_candidates([0], 7) == [] and LR.mask_candidates(np.zeros(7, bool), 7) == []
    local, free, fixed, _ = LR.problem_set(off, okf, okp, counts, [])
    assert not local.any() and free == [] and fixed == []
    s2 = Scene()
    r = LR.restate_set(s2, s2.poses, s2.X, [])
    assert not r["ok"] and r["steps"] == [0, 0] and r["n_local"] == 0 and np.isnan(r["points"]).all()
    # position 0 in a mask is dropped, and 0 plus 16 others is accepted; 17 others are refused
    assert LR.mask_candidates(list(range(0, 17)), 20) == list(range(1, 17))
    with pytest.raises(ValueError):
        LR.mask_candidates(list(range(1, 18)), 20)
    # the covisible rule: heaviest first, ties to the later position, the floor max(min_weight, 1), truncation, position 0 dropped
    W = np.array([[9, 5, 0, 0, 7], [5, 9, 3, 3, 3], [0, 3, 9, 0, 0], [0, 3, 0, 9, 0], [7, 3, 0, 0, 9]])
    assert LR.candidates(W, 1, n_best=2, min_weight=0) == [1, 4]          # 0 (5) is taken and dropped; of the three 3s the latest
    assert LR.candidates(W, 1, n_best=3, min_weight=0) == [1, 3, 4]
    assert LR.candidates(W, 1, n_best=15, min_weight=4) == [1]
    assert LR.candidates(W, 2, n_best=15, min_weight=0) == [1, 2]          # (a weight of 0 never counts)
    assert LR.candidates(W, -1, n_best=0) == [4] and LR.candidates(W, 0, n_best=0) == []


def test_erase_rules_on_small_arrays():
    off, okf, okp = _csr([[(0, 1), (1, 1), (2, 1)], [(1, 2)], [], [(9, 9), (2, 3)], [(0, 4), (1, 4)]])
    flags = np.array([0, 1, 0, 1, 1, 0, 0, 0])
    o2, k2, p2, n_erased, n_under = LR.erase_entries(off, okf, okp, flags)
    assert o2.tolist() == [0, 2, 2, 2, 3, 5] and k2.tolist() == [0, 2, 2, 0, 1] and p2.tolist() == [1, 1, 3, 4, 4]
    assert n_erased == 3 and n_under == 2          # point 1 lost its only entry, point 3 its stale one (one left); point 0 keeps two
    o3, k3, p3, n3, u3 = LR.erase_entries(off, okf, okp, np.zeros(8, np.uint8))
    assert np.array_equal(o3, off) and np.array_equal(k3, okf) and np.array_equal(p3, okp) and (n3, u3) == (0, 0)
    o4, k4, _, n4, u4 = LR.erase_entries(off, okf, okp, np.ones(8, np.uint8))
    assert o4.tolist() == [0] * 6 and len(k4) == 0 and (n4, u4) == (8, 4)


def test_erase_of_the_flagged_outliers_on_the_noisy_scene():
    """measured: 175 entries flagged, all 169 moved edges among them; the second adjustment has 3020 edges, the first call's inliers,
    flags none, and starts at the cost the first ended with (375.62)"""
    s = Scene(pixel_noise=NOISE, seed=NOISE_SEED)
    poses, xyz = s.perturbed()
    moved = s.move_edges()
    r = s.restate(poses, xyz)
    flags = LR.outlier_flags(r)
    print("flagged %d, moved %d, moved and flagged %d; inliers %d of %d, end cost %.6g" % (flags.sum(), moved.sum(), (flags & moved).sum(),
                                                                                          r["n_inliers"], r["n_edges"], r["cost"][2]))
    assert flags.sum() == 175 and moved.sum() == 169 and (flags & moved).sum() == 169
    off, okf, okp, n_erased, n_under = LR.erase_entries(s.obs_off, s.obs_kf, s.obs_kp, flags)
    assert n_erased == 175 and len(okf) == len(s.obs_kf) - 175
    from tests.ba_restatement import bundle_adjust
    from tests.ba_scene import K
    r2 = bundle_adjust(off, okf, okp, s.counts, s.kxy, s.octave, r["xyz"], K, r["poses"])
    print("second adjustment: %d edges, %d outliers, cost %s; n_under %d" % (r2["n_edges"], (r2["edge_inlier"] == 2).sum(), r2["cost"], n_under))
    assert r2["n_edges"] == r["n_inliers"] == 3020 and not (r2["edge_inlier"] == 2).any()
    assert abs(r2["cost"][0] - r["cost"][2]) <= 1e-4 * r["cost"][2]   # (the points were rounded to f32 in between)
    # nothing is erased behind an adjustment that is not ok
    assert not LR.outlier_flags(r, min_inliers=r["n_inliers"] + 1).any()


def test_local_struct_layouts_and_symbols(tmp_path):
    import vslam_amd as V
    structs = [("mo_map_ba_local_params", V.MapBaLocalParams), ("mo_map_ba_local_out", V.MapBaLocalOut), ("mo_map_obserase_out", V.MapObsEraseOut),
               ("mo_map_ba_params", V.MapBaParams), ("mo_map_ba_out", V.MapBaOut)]
    body = ""
    for cname, cls in structs:
        body += '  printf("%%zu\\n", sizeof(%s));\n' % cname
        body += "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0].rstrip("_")) for f in cls._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vslam_amd.h"\nint main(void) {\n' + body
                   + '  printf("%d\\n", MO_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    k = 0
    for cname, cls in structs:
        assert got[k] == C.sizeof(cls), cname
        offs = [getattr(cls, f[0]).offset for f in cls._fields_]
        assert got[k + 1:k + 1 + len(offs)] == offs, cname
        k += 1 + len(offs)
    assert got[k] == 7                     # the ABI version stays
    lib = V.load_library()
    assert hasattr(lib, "mo_map_bundle_adjust_local") and hasattr(lib, "mo_map_erase_observations")
    from vslam_amd.mapper import LocalMapper
    import inspect
    prm = inspect.signature(LocalMapper.bundle_adjust).parameters
    assert list(prm)[-6:] == ["local", "kf_position", "n_best", "min_weight", "free", "erase_outliers"]
    assert prm["local"].default == "window" and prm["free"].default is None and prm["erase_outliers"].default is False
    assert hasattr(LocalMapper, "erase_observations")
