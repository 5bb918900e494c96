"""LocalMapper.point_views (mo_map_point_views) and the frustum mode of track_local_map and fuse_map_points (mo_map_track_frustum,
mo_map_fuse_frustum) on the device against the numpy restatement (tests/view_restatement.py) on worlds with real octaves
(tests/view_worlds.py).  Every comparison of integers is made on inputs whose gates are decided by a margin above 1e-9 (asserted here
for what the device was given, and in tests/test_view_cpu.py for the worlds)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import track_restatement as TR
from tests import view_restatement as VR
from tests import view_worlds as VW
from tests.fuse_worlds import map_inputs
from tests.map_worlds import remove_keyframes

pytestmark = pytest.mark.gpu

K, W_IMG, H_IMG = VW.K, VW.W_IMG, VW.H_IMG
MARGIN = 1e-9


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _ulps(a, b):
    """distance in units of the last place between two f32 arrays (0 and -0 are equal)"""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


def _restated_views(m, **kw):
    a, P, _, octv, desc = map_inputs(m)
    obs = TR.valid_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], [len(d) for d in desc])
    C = VR.centres(P)
    return VR.point_views(a["xyz"], obs, octv, C, **kw), C, obs


def _check_views(m, label):
    got = m.point_views()
    want, C, obs = _restated_views(m)
    for f in ("ref_pos", "ref_octave", "n_valid"):
        assert np.array_equal(got[f], want[f]), f
    assert np.allclose(got["centre"], C, rtol=1e-12, atol=0.0)
    worst = {f: int(_ulps(got[f], want[f]).max()) for f in ("normal", "min_dist", "max_dist")}
    print("%s: %d points, ulps from the restatement %s, centres bit-equal: %s" % (label, len(obs), worst, np.array_equal(got["centre"], C)))
    assert max(worst.values()) <= 1, worst
    return got, obs


def test_point_views_equal_the_restatement_also_after_keyframe_removal():
    ctx = _ctx()
    m = VW.world("scaled").build(ctx)
    got, obs = _check_views(m, "scaled world")
    assert (got["n_valid"] >= 1).all() and len(set(got["ref_pos"].tolist())) >= 6 and got["n_valid"].max() >= 3
    two_sided = np.linalg.norm(got["normal"], axis=1) < 0.5
    assert two_sided.any() and (~two_sided).any()   # (points seen from both sides: the mean direction is short)
    stored_first = m.arrays()["obs_kf"][m.arrays()["obs_off"][:-1]]
    remove_keyframes(m, [0, 3])
    m._cache = None
    got2, obs2 = _check_views(m, "after removing keyframes 0 and 3")
    # the stored keys were not renumbered: first entries now name another keyframe or none, and the reference passed on
    first_now = np.array([v[0][0] if v else -1 for v in obs2])
    assert (first_now != stored_first).any() and (got2["ref_pos"] == first_now).all()
    assert (got2["ref_pos"] == -1).any() and (got2["max_dist"][got2["ref_pos"] == -1] == 0).all()
    m.close(); ctx.close()


def _local_views(m, window, local_kf=None, n_levels=8):
    a, P, _, octv, desc = map_inputs(m)
    local = None
    if local_kf is not None:
        obs = TR.valid_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], [len(d) for d in desc])
        local = np.array([any(k in local_kf for k, _ in v) for v in obs], bool)
    return a, VR.local_views(a["xyz"], a["obs_off"], a["obs_kf"], a["obs_kp"], desc, octv, P, window=window, n_levels=n_levels, local=local)


def _same_pass(info, ps, k, last):
    assert info["pass_in_image"][k] == ps["in_image"] and info["pass_cand"][k] == ps["cand"] and info["pass_matches"][k] == ps["matches"]
    assert info["pass_radius"][k] == ps["radius"]
    if last:
        assert np.array_equal(info["point"], ps["point"]) and np.array_equal(info["dist"], ps["dist"]) and np.array_equal(info["level"], ps["level"])


@pytest.mark.parametrize("local", ["window", "covisible"])
def test_track_under_the_frustum_equals_the_restatement(local):
    ctx = _ctx()
    c = VW.track_case("track")
    m = c["w"].build(ctx)
    kps, desc, pose0 = c["kps"], c["desc"], c["pose0"]
    kw = dict(frustum=True, window=5, local=local)
    ok1, _, i1 = m.track_local_map(kps, desc, pose0, radii=(15.0,), **kw)
    local_kf = set(i1["local_keyframes"]) if local == "covisible" else None
    if local_kf is not None:
        assert 0 < len(local_kf) < VW.N_KF
    a, lv = _local_views(m, 5, local_kf)
    mg = VR.new_margins()
    r1 = VR.track_frustum(K, pose0, a["xyz"], lv, kps, desc, W_IMG, H_IMG, radii=(15.0,), margins=mg)
    assert i1["n_local"] == r1["n_local"] < len(a["xyz"])
    _same_pass(i1, r1["passes"][0], 0, True)
    assert i1["pass_cand"][0] < i1["pass_in_image"][0] and i1["pass_matches"][0] >= 20
    # two passes: pass 2 restated from the device's pass-1 pose; the final pose = the restated refinement of the device's matches
    ok, pose, info = m.track_local_map(kps, desc, pose0, **kw)
    assert info["n_pass_run"] == 2 and np.array_equal(info["pass_pose"][0], i1["pass_pose"][0])
    r2 = VR.track_frustum(K, pose0, a["xyz"], lv, kps, desc, W_IMG, H_IMG, poses=[pose0, info["pass_pose"][0]], margins=mg)
    _same_pass(info, r2["passes"][0], 0, False)
    _same_pass(info, r2["passes"][1], 1, True)
    assert VR.min_margin(mg) > MARGIN, mg
    q = np.flatnonzero(info["point"] >= 0)
    ref, inl, n_inl = TR.refine(K, info["pass_pose"][0], a["xyz"][info["point"][q]].astype(np.float64),
                                np.column_stack([kps["x"][q], kps["y"][q]]).astype(np.float64), kps["octave"][q])
    assert np.allclose(pose, ref, rtol=1e-9, atol=1e-9), pose - ref
    assert np.array_equal(info["inlier"][q], inl) and info["pass_inliers"][1] == n_inl
    assert ok and np.abs(pose - c["T"]).max() < 1e-6
    print("%s: %s in image, %s candidates, %s matches, %s inliers" % (local, info["pass_in_image"], info["pass_cand"], info["pass_matches"],
                                                                     info["pass_inliers"]))
    m.close(); ctx.close()


def test_approach_from_half_the_depth():
    """the map seen from half the depth it was built at: every octave is four or five levels up.  The plain search loses every point at
    its octave gate (today's behaviour, pinned here); the frustum search predicts the level and tracks"""
    ctx = _ctx()
    c = VW.track_case("approach")
    m = c["w"].build(ctx)
    ok0, pose_plain, i0 = m.track_local_map(c["kps"], c["desc"], c["pose0"])
    assert not ok0 and i0["pass_matches"][0] < 20 and i0["pass_cand"][0] > 500
    ok, pose, info = m.track_local_map(c["kps"], c["desc"], c["pose0"], frustum=True)
    print("approach: plain %s matches of %s candidates; frustum %s matches of %s candidates (%s in image), %s inliers, pose error %.2e"
          % (i0["pass_matches"], i0["pass_cand"], info["pass_matches"], info["pass_cand"], info["pass_in_image"], info["pass_inliers"],
             np.abs(pose - c["T"]).max()))
    assert ok and np.abs(pose - c["T"]).max() < 1e-6, pose - c["T"]
    matched = info["point"] >= 0
    d = info["level"][matched] - c["kps"]["octave"][matched]
    assert d.min() >= 0 and d.max() <= 1 and (info["level"][~matched] == -1).all()
    m.close(); ctx.close()


@pytest.mark.parametrize("name", ["far_side", "beyond", "inside"])
def test_view_angle_and_range(name):
    """points seen from behind, from beyond 1.2 max_dist or from inside 0.8 min_dist project into the image and are not searched"""
    ctx = _ctx()
    c = VW.track_case(name)
    w = c["w"]
    m = w.build(ctx)
    _, _, info = m.track_local_map(c["kps"], c["desc"], c["pose0"], radii=(15.0,), frustum=True, window=0)
    a, lv = _local_views(m, 0)
    mg = VR.new_margins()
    r = VR.track_frustum(K, c["pose0"], a["xyz"], lv, c["kps"], c["desc"], W_IMG, H_IMG, radii=(15.0,), margins=mg)
    assert VR.min_margin(mg) > MARGIN, mg
    _same_pass(info, r["passes"][0], 0, True)
    views = lv[4]
    u, v, z = TR.project(K, c["pose0"], a["xyz"])
    in_image = (z > 0) & (u >= 0) & (u < W_IMG) & (v >= 0) & (v < H_IMG)
    C = VR.camera_centre(c["pose0"])
    dist = np.linalg.norm(a["xyz"].astype(np.float64) - C, axis=1)
    if name == "far_side":
        out = in_image & (w.faces[w.world] == 1)                        # seen from side A only, looked at from side B
    elif name == "beyond":
        out = in_image & (dist > 1.2001 * views["max_dist"])
    else:
        out = in_image & (dist < 0.7999 * views["min_dist"])
    passes = np.array([VR.frustum(a["xyz"][i].astype(np.float64), views["normal"][i], views["max_dist"][i], C)[0] for i in range(len(dist))])
    assert out.sum() >= 50 and not passes[out].any()
    assert info["pass_in_image"][0] == int(in_image.sum()) and info["pass_cand"][0] == int((in_image & passes).sum()) <= int((in_image & ~out).sum())
    matched = info["point"][info["point"] >= 0]
    assert not out[matched].any()
    print("%s: %d in image, %d of them outside the frustum by construction, %d candidates, %d matches"
          % (name, in_image.sum(), out.sum(), info["pass_cand"][0], info["pass_matches"][0]))
    m.close(); ctx.close()


def _obs_lists(a):
    return [list(zip(a["obs_kf"][a["obs_off"][i]:a["obs_off"][i + 1]].tolist(), a["obs_kp"][a["obs_off"][i]:a["obs_off"][i + 1]].tolist()))
            for i in range(len(a["obs_off"]) - 1)]


def test_fuse_under_the_frustum_merges_duplicates_three_octaves_apart():
    ctx = _ctx()
    w = VW.world("duplicates")
    m = w.build(ctx)
    a, P, xy, octv, desc = map_inputs(m)
    want, into, cnt, mg = VR.fuse_frustum(a, P, xy, octv, desc, W_IMG, H_IMG, window=0)
    assert VR.min_margin(mg) > MARGIN, mg
    info = m.fuse_map_points(window=0, frustum=True)
    for f in cnt:
        assert info[f] == cnt[f], (f, info[f], cnt[f])
    assert np.array_equal(info["into"], into)
    m._cache = None
    after = m.arrays()
    assert _obs_lists(after) == _obs_lists(want) and np.array_equal(after["xyz"], want["xyz"]) and np.array_equal(after["id"], want["id"])
    assert all(into[i] == into[j] for i, j in w.pairs) and info["n_absorbed"] == len(w.pairs) > 100
    # the plain call on a copy of the same map: none of them
    m0 = w.build(ctx)
    i0 = m0.fuse_map_points(window=0)
    assert not any(i0["into"][i] == i0["into"][j] for i, j in w.pairs) and i0["n_cand"] == info["n_cand"]
    print("duplicates: frustum %d edges, %d absorbed of %d pairs; plain %d proposals" % (info["n_edges"], info["n_absorbed"], len(w.pairs), i0["n_proposals"]))
    m.close(); m0.close(); ctx.close()


def test_degenerate_inputs():
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    rng = np.random.default_rng(8)
    kps = VW.kps_array(np.column_stack([rng.uniform(0, 640, 300), rng.uniform(0, 480, 300)]), np.full(300, 2))
    desc = rng.integers(0, 256, (300, 32)).astype(np.uint8)
    img = np.zeros((H_IMG, W_IMG), np.uint8)
    T0 = VW.camera("A", 10.0)
    empty = LocalMapper(K, save_every_keyframe=False, context=ctx)
    v = empty.point_views()
    assert v["normal"].shape == (0, 3) and v["centre"].shape == (0, 3) and len(v["max_dist"]) == 0
    ok, pose, info = empty.track_local_map(kps, desc, T0, frustum=True)
    assert not ok and info["n_pass_run"] == 0 and (info["point"] == -1).all() and (info["level"] == -1).all() and np.array_equal(pose, T0)
    assert empty.fuse_map_points(frustum=True)["n_cand"] == 0
    empty.add_keyframe(img, kps, desc, T0)   # one keyframe, no map point
    v = empty.point_views()
    assert v["normal"].shape == (0, 3) and np.allclose(v["centre"], [[0.0, 0.0, -10.0]], atol=1e-12)
    ok, pose, info = empty.track_local_map(kps, desc, T0, frustum=True)
    assert not ok and info["n_pass_run"] == 0 and (info["level"] == -1).all()
    assert empty.fuse_map_points(frustum=True)["n_cand"] == 0
    # a point in its reference camera centre (exactly: an unrotated camera at integer coordinates) next to an ordinary one
    empty.update_map_points([{"id": 0, "position": np.array([0.0, 0.0, -10.0], np.float32), "color": np.zeros(3, np.uint8), "observed_keyframes": {0: 0}},
                             {"id": 1, "position": np.array([0.5, 0.25, 2.0], np.float32), "color": np.zeros(3, np.uint8), "observed_keyframes": {0: 1}}])
    v = empty.point_views()
    assert v["ref_pos"].tolist() == [0, 0] and v["n_valid"].tolist() == [0, 1] and v["max_dist"][0] == 0 and v["max_dist"][1] > 0
    back = VW.camera("A", 14.0)   # sees both points in front of it
    ok, _, info = empty.track_local_map(kps, desc, back, radii=(15.0,), frustum=True)
    assert not ok and info["pass_in_image"] == [2] and info["pass_cand"] == [1]
    c = VW.track_case("track")
    m = c["w"].build(ctx)
    ok, pose, info = m.track_local_map(np.zeros(0, V.KP_DTYPE), np.zeros((0, 32), np.uint8), c["pose0"], frustum=True)
    assert not ok and len(info["level"]) == 0 and info["n_pass_run"] == 0
    # one pyramid level: every point is searched at level 0, against octaves -1 .. 0, within [0.8, 1.2] of its one distance
    _, _, info = m.track_local_map(c["kps"], c["desc"], c["pose0"], radii=(15.0,), frustum=True, n_levels=1, window=0)
    a, lv = _local_views(m, 0, n_levels=1)
    r = VR.track_frustum(K, c["pose0"], a["xyz"], lv, c["kps"], c["desc"], W_IMG, H_IMG, radii=(15.0,), n_levels=1)
    _same_pass(info, r["passes"][0], 0, True)
    assert info["level"].max() <= 0
    v1 = m.point_views(n_levels=1)
    assert np.array_equal(v1["min_dist"], v1["max_dist"])
    empty.close(); m.close(); ctx.close()


def _same(a, b):
    (oa, pa, ia), (ob, pb, ib) = a, b
    assert oa == ob and np.array_equal(pa, pb)
    for f in ("point", "dist", "inlier", "level"):
        if f in ia or f in ib:
            assert np.array_equal(ia[f], ib[f]), f
    for f in ("pass_radius", "pass_cand", "pass_matches", "pass_inliers", "pass_in_image", "n_local", "n_pass_run"):
        if f in ia or f in ib:
            assert ia[f] == ib[f], f
    assert all(np.array_equal(x, y) for x, y in zip(ia["pass_pose"], ib["pass_pose"]))


def _same_views(a, b):
    assert all(a[f].tobytes() == b[f].tobytes() for f in a)


def test_no_leak_determinism_and_paths():
    """on the survey8d keyframes with real detections (the map of tests/test_gpu_track_map.py's path test): the map is not changed, two
    calls give equal bytes, the resident token equals the host arrays, a map with tiny capacities agrees, and the plain call is what it
    was before a frustum call ran"""
    import vslam_amd as V
    from tests.test_gpu_mapper import _rz
    from tests.test_gpu_relocalize import _sequence_map
    from vslam_amd.mapper import predict_pose
    from vslam_amd.synth import Survey8dScene, frame_roll_deg
    import torch
    ctx = _ctx()
    m, _, _ = _sequence_map(ctx)
    sc = Survey8dScene(torch, "cpu")

    def truth(g):
        R = _rz(np.deg2rad(frame_roll_deg(sc.seed, g)))
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = -R @ np.array([g * 0.05, 0.0, 0.0])
        return T
    g = 7
    (kps, desc), = ctx.orb_detect_compute(sc.frame(g).numpy(), V.orb_params(nfeatures=2000))
    kh, dh = np.array(kps).copy(), np.array(desc).copy()
    pred = predict_pose(truth(g - 2), truth(g - 1))
    before = {f: v.copy() for f, v in m.arrays().items()}
    lo, ids = (x.copy() for x in m.list_arrays())
    plain = m.track_local_map(kps, desc, pred)
    views = m.point_views()
    res = m.track_local_map(kps, desc, pred, frustum=True)
    assert res[2]["from_token"] and res[0], res[2]
    print("real frames: plain %s matches, frustum %s matches of %s candidates (%s in image), %s inliers"
          % (plain[2]["pass_matches"], res[2]["pass_matches"], res[2]["pass_cand"], res[2]["pass_in_image"], res[2]["pass_inliers"]))
    host = m.track_local_map(kh, dh, pred, frustum=True)
    assert not host[2]["from_token"]
    _same(res, host)
    _same(host, m.track_local_map(kh, dh, pred, frustum=True))
    _same(plain, m.track_local_map(kps, desc, pred))
    _same_views(views, m.point_views())
    cov = m.track_local_map(kh, dh, pred, frustum=True, local="covisible")
    _same(cov, m.track_local_map(kh, dh, pred, frustum=True, local="covisible"))
    m._cache = None; m._lists = None
    after = m.arrays()
    assert all(np.array_equal(before[f], after[f]) for f in before)
    assert all(np.array_equal(x, y) for x, y in zip((lo, ids), m.list_arrays()))
    m2, _, _ = _sequence_map(ctx, capacity=(2, 16, 16, 32))
    _same(host, m2.track_local_map(kh, dh, pred, frustum=True))
    _same_views(views, m2.point_views())
    m.close(); m2.close(); ctx.close()


def test_results_do_not_depend_on_stale_scratch():
    """with every scratch buffer filled with one byte and then another before each call, the frustum track, the frustum fuse and
    point_views return what they return without"""
    ctx = _ctx()
    c = VW.track_case("track")
    wd = VW.world("duplicates")

    def run():
        m = c["w"].build(ctx)
        views = m.point_views()
        trk = m.track_local_map(c["kps"], c["desc"], c["pose0"], frustum=True)
        trk_c = m.track_local_map(c["kps"], c["desc"], c["pose0"], frustum=True, local="covisible")
        md = wd.build(ctx)
        fi = md.fuse_map_points(window=0, frustum=True)
        md._cache = None
        fa = {f: v.copy() for f, v in md.arrays().items()}
        m.close(); md.close()
        return views, trk, trk_c, fi, fa
    want = run()
    try:
        for byte in (0xAB, 0x5C):
            ctx._check(ctx.lib.mo_dbg_set_poison(ctx.h, byte))
            views, trk, trk_c, fi, fa = run()
            _same_views(views, want[0])
            _same(trk, want[1])
            _same(trk_c, want[2])
            assert all(np.array_equal(fi[f], want[3][f]) for f in fi)
            assert all(np.array_equal(fa[f], want[4][f]) for f in fa)
    finally:
        ctx._check(ctx.lib.mo_dbg_set_poison(ctx.h, -1))
    ctx.close()


def test_run_frames_tracks_and_fuses_under_the_frustum(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "visual-slam_amd", "examples"))
    try:
        from run_frames import synthetic_sequence
    finally:
        sys.path.pop(0)
    path = tmp_path / "frames.npy"
    np.save(path, np.stack(list(synthetic_sequence(40, seed=7))))
    r = subprocess.run([sys.executable, os.path.join(root, "visual-slam_amd", "examples", "run_frames.py"), "--frames", str(path), "--max-frames", "40",
                        "--keyframe-every", "5", "--map", str(tmp_path / "map.ply"), "--track-map", "--frustum", "--fuse"], capture_output=True,
                       text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ": track map " in ln]
    print("\n".join(lines + [ln for ln in r.stdout.splitlines() if ": fuse " in ln]))
    assert lines, r.stdout[-3000:]
