"""CPU checks of tracking against the map: the mo_map_track boundary (export, ABI, struct layouts against the ctypes mirror) and the
numpy restatement's rules on hand-built cases."""
import os
import subprocess

import numpy as np

from tests import track_restatement as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])


def test_track_is_exported_and_bound():
    import vslam_amd as V
    lib = V.load_library()
    assert hasattr(lib, "mo_map_track") and "mo_map_track" in V.SIGNATURES
    assert lib.mo_abi_version() == V.ABI_VERSION == 7


def test_track_struct_layouts_match_the_header(tmp_path):
    import ctypes as C
    import vslam_amd as V
    structs = [("mo_map_track_params", V.MapTrackParams), ("mo_map_track_out", V.MapTrackOut)]
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
        assert got[k] == C.sizeof(cls), cname
        offs = [getattr(cls, f[0]).offset for f in cls._fields_]
        assert got[k + 1:k + 1 + len(offs)] == offs, cname
        k += 1 + len(offs)


def _desc(bits):
    """a descriptor with the given bit positions set"""
    d = np.zeros(32, np.uint8)
    for b in bits:
        d[b // 8] |= np.uint8(1 << (b % 8))
    return d


def _kps(xy, octave=None):
    import vslam_amd as V
    k = np.zeros(len(xy), V.KP_DTYPE)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    k["x"] = xy[:, 0]; k["y"] = xy[:, 1]; k["size"] = 31.0
    if octave is not None:
        k["octave"] = octave
    return k


def test_representative_median_and_ties():
    # three observations: distances a-b 4, a-c 6, b-c 2 -> sorted rows [0 4 6], [0 2 4], [0 2 6]: medians 4, 2, 2 -> b (the earlier of
    # the tie with c)
    a, b, c = _desc([]), _desc([0, 1, 2, 3]), _desc([0, 1, 2, 3, 4, 5])
    assert T.representative(np.stack([a, b, c])) == 1
    # all medians equal: the first
    assert T.representative(np.stack([a, a, a])) == 0
    # two observations: medians are element 0 = 0 for both -> the first
    assert T.representative(np.stack([c, a])) == 0
    # four: element (4 - 1) // 2 = 1 of each sorted row
    d = _desc([100])
    assert T.representative(np.stack([d, a, a, b])) == 1


def test_valid_observations_and_window_edge():
    off = np.array([0, 2, 3, 5])
    okf = np.array([0, -1, 1, 0, 7])      # -1 = the last position (2); 7 names nothing
    okp = np.array([0, -1, 1, 1, 0])
    obs = T.valid_observations(off, okf, okp, [2, 2, 2])
    assert obs == [[(0, 0), (2, 1)], [(1, 1)], [(0, 1)]]
    # window 1: position 2 only; window 2: positions 1, 2; window 0 or >= n_kf: everything
    assert T.local_points(obs, 3, 1).tolist() == [True, False, False]
    assert T.local_points(obs, 3, 2).tolist() == [True, True, False]
    assert T.local_points(obs, 3, 0).tolist() == [True, True, True]
    assert T.local_points(obs, 3, 5).tolist() == [True, True, True]


def _one_point_search(kxy, kdesc, koct, rep, ref=0, radius=15.0, ratio=0.8, max_dist=100):
    pose = np.eye(4)
    xyz = np.array([[0.0, 0.0, 5.0]], np.float32)      # projects to the principal point (320, 240)
    return T.search(K, pose, xyz, rep[None, :], [ref], _kps(kxy, koct), np.stack(kdesc), 640, 480, radius, 1.2, max_dist, ratio)


def test_search_ratio_edge_and_window():
    rep = _desc([])
    near = [(321.0, 240.0), (310.0, 245.0)]
    # best 8, second 10: 8 <= 0.8 * 10 is accepted (the edge), 9 is not
    p, d, nc = _one_point_search(near, [_desc(range(8)), _desc(range(10))], [0, 0], rep)
    assert nc == 1 and p.tolist() == [0, -1] and d.tolist() == [8, -1]
    p, _, _ = _one_point_search(near, [_desc(range(9)), _desc(range(10))], [0, 0], rep)
    assert p.tolist() == [-1, -1]
    # equal distances: the lower keypoint is best, the second has the same distance -> 5 <= 0.8 * 5 fails
    p, _, _ = _one_point_search(near, [_desc(range(5)), _desc(range(5))], [0, 0], rep)
    assert p.tolist() == [-1, -1]
    # a single keypoint in the window: no second, only max_dist
    p, d, _ = _one_point_search([(320.0, 240.0), (340.0, 240.0)], [_desc(range(100)), _desc([])], [0, 0], rep)
    assert p.tolist() == [0, -1] and d.tolist() == [100, -1]
    p, _, _ = _one_point_search([(320.0, 240.0)], [_desc(range(101))], [0], rep)
    assert p.tolist() == [-1]
    # |x - u| < r is strict: 15 px away at radius 15 is outside; at octave 1 the window is 15 * 1.2 = 18 px
    p, _, _ = _one_point_search([(335.0, 240.0)], [_desc([])], [0], rep)
    assert p.tolist() == [-1]
    p, _, _ = _one_point_search([(335.0, 240.0)], [_desc([])], [1], rep, ref=1)
    assert p.tolist() == [0]


def test_search_octave_gate():
    rep = _desc([])
    kxy = [(320.0, 240.0), (322.0, 240.0), (324.0, 240.0)]
    # ref_octave 2: keypoints at octaves 0 (out), 1 and 3 (in)
    p, d, _ = _one_point_search(kxy, [_desc([]), _desc(range(3)), _desc(range(20))], [0, 1, 3], rep, ref=2)
    assert p.tolist() == [-1, 0, -1] and d.tolist() == [-1, 3, -1]
    p, _, _ = _one_point_search(kxy, [_desc([]), _desc(range(3)), _desc(range(20))], [0, 4, 4], rep, ref=2)
    assert p.tolist() == [-1, -1, -1]


def test_search_conflict_tie_goes_to_the_lower_point():
    # two points projecting to the same pixel claim keypoint 0 with the same distance: point 0 keeps it; a lower distance wins
    pose = np.eye(4)
    xyz = np.array([[0.0, 0.0, 5.0], [0.0, 0.0, 10.0], [0.0, 0.0, 7.0]], np.float32)
    kps = _kps([(320.0, 240.0)], [0])
    desc = np.stack([_desc(range(4))])
    reps = np.stack([_desc([]), _desc([]), _desc([0])])
    p, d, nc = T.search(K, pose, xyz, reps, [0, 0, 0], kps, desc, 640, 480, 15.0)
    assert nc == 3 and p.tolist() == [2] and d.tolist() == [3]
    reps[2] = _desc([])
    p, d, _ = T.search(K, pose, xyz, reps, [0, 0, 0], kps, desc, 640, 480, 15.0)
    assert p.tolist() == [0] and d.tolist() == [4]
    # outside the local map, behind the camera, outside the image: no candidate
    xyz2 = np.array([[0.0, 0.0, -5.0], [100.0, 0.0, 5.0], [0.0, 0.0, 5.0]], np.float32)
    p, _, nc = T.search(K, pose, xyz2, reps, [0, 0, None], kps, desc, 640, 480, 15.0)
    assert nc == 0 and p.tolist() == [-1]


def _tiny_map(n_pts, seed=0):
    """one keyframe observing n_pts points in front of the identity camera; its rows = the points in order"""
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.uniform(-2, 2, n_pts), rng.uniform(-1.5, 1.5, n_pts), rng.uniform(4, 8, n_pts)]).astype(np.float32)
    desc = rng.integers(0, 256, (n_pts, 32)).astype(np.uint8)
    u, v, _ = T.project(K, np.eye(4), X)
    return X, desc, np.column_stack([u, v])


def test_retry_doubles_the_radius_and_a_second_failure_ends_the_call():
    X, desc, uv = _tiny_map(30)
    off = np.arange(31)
    okf = np.zeros(30, np.int64)
    okp = np.arange(30)
    octs = [np.zeros(30, np.int64)]
    # every keypoint 6 px right of its projection: outside radius 4, inside the retry's 8
    kps = _kps(uv + [6.0, 0.0], np.zeros(30, np.int64))
    r = T.track(K, np.eye(4), X, off, okf, okp, [desc], octs, kps, desc, 640, 480, radii=(4.0,), min_matches=20, min_inliers=10,
                refine_pose=False)
    ps = r["passes"][0]
    assert ps["radius"] == 8.0 and ps["matches"] == 30 and ps["cand"] == 30
    # 12 px: outside both -> the call ends after the retry
    kps = _kps(uv + [12.0, 0.0], np.zeros(30, np.int64))
    r = T.track(K, np.eye(4), X, off, okf, okp, [desc], octs, kps, desc, 640, 480, radii=(4.0, 4.0), min_matches=20)
    assert len(r["passes"]) == 1 and r["passes"][0]["matches"] == 0 and r["passes"][0]["radius"] == 8.0 and not r["ok"]
    assert np.array_equal(r["pose"], np.eye(4))


def test_refinement_recovers_a_perturbed_pose():
    X, desc, uv = _tiny_map(60, seed=4)
    kps = _kps(uv, np.zeros(60, np.int64))
    w = np.array([0.01, -0.02, 0.015])
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    pose0 = np.eye(4)
    pose0[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    pose0[:3, 3] = [0.03, -0.02, 0.04]
    x = np.column_stack([kps["x"], kps["y"]]).astype(np.float64)
    x[:5] += 40.0   # five outliers
    pose, inl, n = T.refine(K, pose0, X.astype(np.float64), x, np.zeros(60, np.int64))
    assert n == 55 and not inl[:5].any()
    assert np.abs(pose - np.eye(4)).max() < 1e-4
