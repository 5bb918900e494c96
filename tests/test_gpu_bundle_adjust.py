"""LocalMapper.bundle_adjust (mo_map_bundle_adjust) and LocalMapper.add_observations / add_keyframe(tracked=) on the device against the
numpy restatement (tests/ba_restatement.py) and against the known poses and points of the constructed scene (tests/ba_scene.py)."""
import numpy as np
import pytest

from tests.ba_restatement import add_observations as restate_add
from tests.ba_scene import H_IMG, K, W_IMG, Scene
from tests.test_ba_cpu import NOISE, NOISE_SEED, RECOVERY_BOUND

pytestmark = pytest.mark.gpu

INT_KEYS = ("ok", "n_free", "n_fixed", "n_local", "n_edges", "n_inliers", "steps", "accepted", "free", "fixed")
# largest |device - restatement| over the pose entries and the f64 points after the full two rounds, as measured on an MI355X
# (profiles/ba_parity.txt); the assertion is 100 x that, never looser than 1e-6
PARITY_MEASURED = 8.88e-14
PARITY_BOUND = min(100 * PARITY_MEASURED, 1e-6)


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _mapper(ctx, s, poses, xyz, capacity=None):
    """the scene as a device map: keyframes stored with the true poses (random descriptors: no growth step finds a model), the points
    injected with their observations, then kf["pose"] set to `poses`"""
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    rng = np.random.default_rng(77)
    kw = {"capacity": capacity} if capacity else {}
    m = LocalMapper(K, save_every_keyframe=False, context=ctx, **kw)
    img = np.zeros((H_IMG, W_IMG), np.uint8)
    for k in range(s.n_kf):
        kp = np.zeros(len(s.kxy[k]), V.KP_DTYPE)
        kp["x"] = s.kxy[k][:, 0]; kp["y"] = s.kxy[k][:, 1]; kp["size"] = 31.0; kp["octave"] = s.octave[k]
        m.add_keyframe(img, kp, rng.integers(0, 256, (len(kp), 32)).astype(np.uint8), s.poses[k])
    assert len(m.map_points) == 0
    m.update_map_points([{"id": j, "position": xyz[j], "color": np.zeros(3, np.uint8), "observed_keyframes": s.obs[j]} for j in range(len(xyz))])
    for k in range(s.n_kf):
        m.keyframes[k]["pose"][:] = poses[k]
    return m


def _same_integers(info, ok, ref):
    got = dict(info, ok=ok)
    for k in INT_KEYS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert np.array_equal(info["edge_inlier"], ref["edge_inlier"])


def _diff(info, ref):
    loc = ~np.isnan(ref["points"][:, 0])
    assert np.array_equal(loc, ~np.isnan(info["points"][:, 0]))
    return max(float(np.abs(info["poses"] - ref["poses"]).max()), float(np.abs(info["points"][loc] - ref["points"][loc]).max()))


def test_one_step_and_two_rounds_against_the_restatement():
    ctx = _ctx()
    s = Scene()
    poses, xyz = s.perturbed()
    ref1 = s.restate(poses, xyz, max_steps=(1, 0))
    m = _mapper(ctx, s, poses, xyz)
    ok, info = m.bundle_adjust(max_steps=(1, 0), want_points=True)
    _same_integers(info, ok, ref1)
    np.testing.assert_allclose(info["poses"], ref1["poses"], rtol=1e-9, atol=1e-9)
    loc = ~np.isnan(ref1["points"][:, 0])
    np.testing.assert_allclose(info["points"][loc], ref1["points"][loc], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(info["cost"], ref1["cost"], rtol=1e-9)
    print("one step: largest difference %.3g" % _diff(info, ref1))
    ref = s.restate(poses, xyz)
    m = _mapper(ctx, s, poses, xyz)
    ok, info = m.bundle_adjust(want_points=True)
    print("two rounds: steps %s accepted %s (restatement %s %s), cost %s" % (info["steps"], info["accepted"], ref["steps"], ref["accepted"], info["cost"]))
    d = _diff(info, ref)
    print("two rounds: largest difference to the restatement %.3g (bound %.3g)" % (d, PARITY_BOUND))
    _same_integers(info, ok, ref)
    assert d <= PARITY_BOUND


def test_recovery_noise_and_outliers_against_ground_truth():
    ctx = _ctx()
    s = Scene()
    poses, xyz = s.perturbed()
    m = _mapper(ctx, s, poses, xyz)
    ok, info = m.bundle_adjust(want_points=True)
    loc = ~np.isnan(info["points"][:, 0])
    e_pose, e_pt = s.pose_error(info["poses"]), float(np.abs(info["points"][loc] - s.X[loc]).max())
    print("noise-free: cost %s, pose error %.3g, point error %.3g" % (info["cost"], e_pose, e_pt))
    assert ok and info["cost"][2] < 1e-6 * info["cost"][0] and not (info["edge_inlier"] == 2).any()
    assert e_pose < RECOVERY_BOUND[0] and e_pt < RECOVERY_BOUND[1]
    s = Scene(pixel_noise=NOISE, seed=NOISE_SEED)
    poses, xyz = s.perturbed()
    m = _mapper(ctx, s, poses, xyz)
    ok, info = m.bundle_adjust()
    print("%.1f px noise: pose error %.3g -> %.3g" % (NOISE, s.pose_error(poses), s.pose_error(info["poses"])))
    assert ok and s.pose_error(info["poses"]) < s.pose_error(poses)
    moved = s.move_edges()
    m = _mapper(ctx, s, poses, xyz)
    ok, info = m.bundle_adjust()
    ei = info["edge_inlier"]
    clean = ~moved & (ei > 0)
    print("outliers: %d of %d moved edges flagged, %d of %d untouched edges flagged" % ((ei[moved] == 2).sum(), moved.sum(), (ei[clean] == 2).sum(), clean.sum()))
    assert ok and (ei[moved] == 2).all() and (ei[clean] == 2).sum() <= 0.01 * clean.sum()


def test_what_is_written_and_determinism():
    ctx = _ctx()
    s = Scene()
    poses, xyz = s.perturbed()
    m = _mapper(ctx, s, poses, xyz)
    before = {k: v.copy() for k, v in m.arrays().items()}
    lists = [a.copy() for a in m.list_arrays()]
    kf_poses = [kf["pose"].copy() for kf in m.keyframes]
    ok, info = m.bundle_adjust(want_points=True)
    assert ok
    after = m.arrays()
    loc = ~np.isnan(info["points"][:, 0])
    assert loc.sum() == info["n_local"]
    assert np.array_equal(after["xyz"][loc], info["points"][loc].astype(np.float32))
    assert np.array_equal(after["xyz"][~loc], before["xyz"][~loc])
    assert not np.array_equal(after["xyz"][loc], before["xyz"][loc])
    for k in before:
        if k != "xyz":
            assert np.array_equal(after[k], before[k]), k
    for a, b in zip(lists, m.list_arrays()):
        assert np.array_equal(a, b)
    for k, kf in enumerate(m.keyframes):
        if k in info["free"]:
            assert np.array_equal(kf["pose"][:3, :4], info["poses"][k]) and not np.array_equal(kf["pose"], kf_poses[k])
        else:
            assert np.array_equal(kf["pose"], kf_poses[k])
    # two maps built alike (the second with tiny capacities: every buffer regrown): the same bytes
    m2 = _mapper(ctx, s, poses, xyz, capacity=(2, 16, 16, 32))
    ok2, info2 = m2.bundle_adjust(want_points=True)
    assert ok2 == ok
    for k in info:
        assert np.array_equal(np.asarray(info[k]), np.asarray(info2[k]), equal_nan=True), k
    for k, v in m2.arrays().items():
        assert np.array_equal(v, after[k]), k
    # a second call starts from the refined state (the points rounded to f32)
    ok3, info3 = m.bundle_adjust()
    assert ok3 and info3["cost"][0] < 1e-6 * info["cost"][0]


def test_window_gauge_and_empty_cases():
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    s = Scene()
    poses, xyz = s.perturbed(first_free=5)
    m = _mapper(ctx, s, poses, xyz)
    ref = s.restate(poses, xyz, window=3)
    ok, info = m.bundle_adjust(window=3, want_points=True)
    _same_integers(info, ok, ref)
    assert info["free"] == [5, 6, 7] and 0 not in info["free"]
    empty = LocalMapper(K, save_every_keyframe=False, context=ctx)
    ok, info = empty.bundle_adjust()
    assert not ok and info["n_free"] == 0 and info["steps"] == [0, 0]
    big = Scene(n_w=300, n_kf=19)
    mb = _mapper(ctx, big, big.poses, big.X)
    with pytest.raises(V.NativeError):
        mb.bundle_adjust(window=0)
    with pytest.raises(ValueError):
        big.restate(big.poses, big.X, window=0)
    ok, info = mb.bundle_adjust(window=16, want_points=True)
    _same_integers(info, ok, big.restate(big.poses, big.X, window=16))
    assert 0 < info["n_free"] <= 16


def test_add_observations_against_the_restatement():
    ctx = _ctx()
    s = Scene()
    m = _mapper(ctx, s, s.poses, s.X)
    a = {k: v.copy() for k, v in m.arrays().items()}
    n = len(s.X)
    rng = np.random.default_rng(4)
    point = rng.integers(-5, n + 5, 300).astype(np.int32)      # out of range on both sides, duplicates
    point[10] = point[3]
    row = rng.integers(0, 50, 300).astype(np.int32)
    for kf_pos in (4, s.n_kf):
        m = _mapper(ctx, s, s.poses, s.X)
        m.add_observations(kf_pos, point, row)
        off, okf, okp = restate_add(a["obs_off"], a["obs_kf"], a["obs_kp"], s.counts, kf_pos, point, row)
        b = m.arrays()
        assert np.array_equal(b["obs_off"], off) and np.array_equal(b["obs_kf"], okf) and np.array_equal(b["obs_kp"], okp)
        assert len(okf) > len(a["obs_kf"])
        for k in ("xyz", "color", "id", "dref_kf", "dref_row"):
            assert np.array_equal(a[k], b[k]), k


def test_add_keyframe_with_tracked_observations():
    """a frame tracked against the map becomes a keyframe: its inlier matches are third observations of their points"""
    ctx = _ctx()
    s = Scene()
    import vslam_amd as V
    m = _mapper(ctx, s, s.poses, s.X)
    plain = _mapper(ctx, s, s.poses, s.X)
    n_pts = len(s.X)
    # the new frame sees the points of keyframe 7 from a pose a little further along x; rows in point order, some not matched
    T = s.poses[7].copy()
    T[:3, 3] -= T[:3, :3] @ np.array([0.2, 0.0, 0.0])
    pts = np.array([j for j in range(n_pts) if 7 in s.obs[j]])
    x = (K @ (T[:3, :3] @ s.X[pts].astype(np.float64).T + T[:3, 3:4])).T
    kp = np.zeros(len(pts) + 20, V.KP_DTYPE)
    kp["x"][:len(pts)] = x[:, 0] / x[:, 2]; kp["y"][:len(pts)] = x[:, 1] / x[:, 2]; kp["size"] = 31.0
    point = np.full(len(kp), -1, np.int32)
    point[:len(pts)] = pts
    inlier = np.zeros(len(kp), bool)
    inlier[:len(pts):2] = True
    desc = np.random.default_rng(5).integers(0, 256, (len(kp), 32)).astype(np.uint8)
    img = np.zeros((H_IMG, W_IMG), np.uint8)
    before = m.arrays()["obs_off"].copy()
    m.add_keyframe(img, kp, desc, T, tracked=(point, inlier))
    plain.add_keyframe(img, kp, desc, T)
    a, b = m.arrays(), plain.arrays()
    gained = pts[::2]
    pos = {int(i): k for k, i in enumerate(a["id"])}
    for j in gained:
        k = pos[int(j)]   # (a gaining point has two observations at least: the cull keeps it)
        assert a["obs_off"][k + 1] - a["obs_off"][k] == len(s.obs[int(j)]) + 1 and a["obs_kf"][a["obs_off"][k + 1] - 1] == 8
    assert (np.diff(a["obs_off"]) >= 3).sum() > (np.diff(b["obs_off"]) >= 3).sum()
    assert m.get_map_statistics()["avg_observations_per_point"] > plain.get_map_statistics()["avg_observations_per_point"] > 2
    # co-visibility: points shared with every keyframe the gaining points were observed in
    want = {}
    for j in gained:
        for k in s.obs[int(j)]:
            want[k] = want.get(k, 0) + 1
    for k, c in want.items():
        assert m.co_visibility_graph[8][k] - plain.co_visibility_graph[8][k] == c and m.co_visibility_graph[k][8] - plain.co_visibility_graph[k][8] == c
    # a stale row (beyond the new keyframe's keypoints) is the cull's IndexError
    m3 = _mapper(ctx, s, s.poses, s.X)
    m3.add_observations(8, pts[:3], np.array([0, 1, len(kp) + 7], np.int32))
    with pytest.raises(IndexError):
        m3.add_keyframe(img, kp, desc, T)


def test_tracking_after_bundle_adjust_lands_on_the_refined_map():
    """keyframe 5's own keypoints tracked from a pose 0.5 degree / 2 cm off its true one: against the perturbed map the pose inherits the
    points' errors, against the refined map it does not"""
    from tests.ba_scene import rot
    ctx = _ctx()
    s = Scene()
    poses, xyz = s.perturbed()
    # (points outside the problem - a single observation - are not refined: they keep their true positions here, so that every point
    # the frame can match is either exact or refined and the bound below speaks about the refinement alone)
    from tests.ba_restatement import problem
    local = problem(s.obs_off, s.obs_kf, s.obs_kp, s.counts, 10)[0]
    xyz[~local] = s.X[~local]
    m = _mapper(ctx, s, poses, xyz)
    kf = m.keyframes[5]
    kps, desc = np.array(kf["keypoints"]).copy(), np.array(kf["descriptors"]).copy()
    P = np.eye(4)
    P[:3, :3] = rot([0.0, np.deg2rad(0.5), 0.0]); P[:3, 3] = [0.02, 0.0, 0.0]
    pred = P @ s.poses[5]

    def err(T):
        return float(np.abs(T[:3, :4] - s.poses[5][:3, :4]).max())
    ok0, T0, i0 = m.track_local_map(kps, desc, pred, image_size=(W_IMG, H_IMG))
    okb, info = m.bundle_adjust()
    ok1, T1, i1 = m.track_local_map(kps, desc, pred, image_size=(W_IMG, H_IMG))
    print("tracked pose error: before BA %.3g (ok %s, inliers %s), after %.3g (ok %s, inliers %s); refined keyframe pose %.3g"
          % (err(T0), ok0, i0["pass_inliers"], err(T1), ok1, i1["pass_inliers"], err(m.keyframes[5]["pose"])))
    assert okb and ok1 and err(T1) <= err(T0)
    assert err(T1) < 10 * RECOVERY_BOUND[0] + 1e-6   # (tracking's own bound on exact data, < 1e-6, on top of the map's)


def _survey():
    from tests.test_gpu_mapper import K as KM, _sequence
    return KM, _sequence()


def _perturb(rng, T, deg, shift):
    from tests.ba_scene import rot
    d, c = rng.normal(size=3), rng.normal(size=3)
    P = np.eye(4)
    P[:3, :3] = rot(np.deg2rad(deg) * d / np.linalg.norm(d)); P[:3, 3] = shift * c / np.linalg.norm(c)
    return P @ T


def test_sequence_with_tracked_observations():
    """the survey8d keyframes with real detect_and_compute: from the third keyframe on each frame is tracked against the map first and
    hands its matches over.  Points gain observations beyond two, the co-visibility counts equal a recount from the arrays, and a mapper
    that is never given `tracked` produces the bytes of one that passes tracked=None."""
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    KM, (frames, poses) = _survey()
    ctx = _ctx()
    prm = V.orb_params(nfeatures=2000)
    m = LocalMapper(KM, save_every_keyframe=False, context=ctx)
    plain = LocalMapper(KM, save_every_keyframe=False, context=ctx)
    none = LocalMapper(KM, save_every_keyframe=False, context=ctx)
    checked = 0
    for k, (fr, T) in enumerate(zip(frames, poses)):
        (kps, desc), = ctx.orb_detect_compute(fr, prm)
        kh, dh = np.array(kps).copy(), np.array(desc).copy()
        plain.add_keyframe(fr, kh, dh, T)
        none.add_keyframe(fr, kh, dh, T, tracked=None)
        tracked = None
        if k >= 2 and len(m.map_points):
            ok, _, info = m.track_local_map(kh, dh, T)
            if ok:
                tracked = (info["point"], info["inlier"])
        if tracked is None:
            m.add_keyframe(fr, kh, dh, T)
            continue
        a = {f: v.copy() for f, v in m.arrays().items()}
        sel = np.unique(tracked[0][tracked[1] & (tracked[0] >= 0)])
        want = {}
        for p in sel.tolist():
            for q in a["obs_kf"][a["obs_off"][p]:a["obs_off"][p + 1]].tolist():
                want[q] = want.get(q, 0) + 1
        n_kf = len(m.keyframes)
        graph = {i: dict(v) for i, v in m.co_visibility_graph.items()}
        m.add_keyframe(fr, kh, dh, T, tracked=tracked)
        if len(m.keyframes) == n_kf + 1:     # (no keyframe was culled: ids are still the positions of before)
            want[n_kf - 1] = want.get(n_kf - 1, 0) + m.last["n_new"]
            for q, cnt in want.items():
                assert m.co_visibility_graph[n_kf][q] - graph.get(n_kf, {}).get(q, 0) == cnt, (k, q)
                assert m.co_visibility_graph[q][n_kf] - graph.get(q, {}).get(n_kf, 0) == cnt, (k, q)
            checked += 1
    cnt, cnt_plain = np.diff(m.arrays()["obs_off"]), np.diff(plain.arrays()["obs_off"])
    st = m.get_map_statistics()
    print("tracked run: %d keyframes, %d points, %d with >= 3 observations, %.3f observations per point (plain run: %d points, at most %d each); "
          "%d keyframe steps recounted" % (len(m.keyframes), len(cnt), (cnt >= 3).sum(), st["avg_observations_per_point"], len(cnt_plain),
                                            cnt_plain.max(), checked))
    assert checked >= 3 and (cnt >= 3).sum() > 0 and cnt_plain.max() == 2 and st["avg_observations_per_point"] > 2
    pa, na = plain.arrays(), none.arrays()
    for f in pa:
        assert np.array_equal(pa[f], na[f]), f
    for x, y in zip(plain.list_arrays(), none.list_arrays()):
        assert np.array_equal(x, y)
    # a stale row: an observation of the next keyframe beyond its keypoints is the cull's IndexError
    m.add_observations(len(m.keyframes), np.array([0], np.int32), np.array([10 ** 6], np.int32))
    with pytest.raises(IndexError):
        m.add_keyframe(frames[-1], kh, dh, poses[-1])


def _pipeline(ba):
    """the survey8d keyframes; keyframes 0 and 1 at their true poses, every later one tracked against the map from a prediction 0.3 degree
    / 5 mm off, and the tracked pose moved by 0.15 degree / 3 mm before it is stored (the same draws with and without BA); returns the mean
    distance of the stored keyframes' camera centres to the truth, in units of the 0.05 baseline, and the mean rotation error in degrees"""
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    KM, (frames, poses) = _survey()
    ctx = _ctx()
    rng = np.random.default_rng(11)
    prm = V.orb_params(nfeatures=2000)
    m = LocalMapper(KM, save_every_keyframe=False, context=ctx)
    n_ba = 0
    for k, (fr, T) in enumerate(zip(frames, poses)):
        (kps, desc), = ctx.orb_detect_compute(fr, prm)
        kh, dh = np.array(kps).copy(), np.array(desc).copy()
        pred, tracked, Tk = _perturb(rng, T, 0.3, 0.005), None, T
        if k >= 2:
            Tk = pred
            if len(m.map_points):
                ok, Tt, info = m.track_local_map(kh, dh, pred)
                if ok:
                    Tk, tracked = Tt, (info["point"], info["inlier"])
            Tk = _perturb(rng, Tk, 0.15, 0.003)
        m.add_keyframe(fr, kh, dh, Tk, tracked=tracked)
        m.keyframes[-1]["truth"] = T
        if ba and k >= 2:
            ok, info = m.bundle_adjust()
            n_ba += ok
    ec, er = [], []
    for kf in m.keyframes:
        P, T = kf["pose"], kf["truth"]
        ec.append(np.linalg.norm(P[:3, :3].T @ P[:3, 3] - T[:3, :3].T @ T[:3, 3]) / 0.05)
        er.append(np.degrees(np.arccos(np.clip((np.trace(P[:3, :3] @ T[:3, :3].T) - 1) / 2, -1, 1))))
    st = m.get_map_statistics()
    m.close(); ctx.close()
    return float(np.mean(ec)), float(np.mean(er)), n_ba, st


def test_pipeline_keyframe_poses_with_and_without_bundle_adjust():
    c0, r0, _, st0 = _pipeline(False)
    c1, r1, n_ba, st1 = _pipeline(True)
    print("mean keyframe pose error without BA: centre %.4f baselines, rotation %.4f deg (%d points, %.2f observations each)"
          % (c0, r0, st0["num_map_points"], st0["avg_observations_per_point"]))
    print("mean keyframe pose error with BA:    centre %.4f baselines, rotation %.4f deg (%d points, %.2f observations each; %d calls ok)"
          % (c1, r1, st1["num_map_points"], st1["avg_observations_per_point"], n_ba))
    assert n_ba > 0 and c1 < c0 and r1 < r0


def test_run_frames_with_local_ba(tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "visual-slam_amd", "examples"))
    try:
        from run_frames import synthetic_sequence
    finally:
        sys.path.pop(0)
    path = tmp_path / "frames.npy"
    np.save(path, np.stack(list(synthetic_sequence(40, seed=7))))
    base = [sys.executable, os.path.join(root, "visual-slam_amd", "examples", "run_frames.py"), "--frames", str(path), "--max-frames", "40",
            "--keyframe-every", "5", "--map", str(tmp_path / "map.ply"), "--track-map"]
    outs = []
    for extra in ([], [], ["--local-ba", "--ba-window", "8"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append([ln for ln in r.stdout.splitlines() if " frames in " not in ln])   # (the timing line differs from run to run)
    assert outs[0] == outs[1] and not any("bundle adjust" in ln for ln in outs[0])   # without the flag: the output of before, run after run
    ba = [ln for ln in outs[2] if "bundle adjust" in ln]
    print("\n".join(ba))
    assert ba and ba[-1].startswith("bundle adjustment: ") and len(ba) >= 2
    first = outs[2].index(next(ln for ln in outs[2] if ": bundle adjust " in ln))
    # the same run up to the first keyframe that hands its matches over (its "Saved map" line stands right before the BA line)
    assert outs[2][first - 1].startswith("Saved map") and outs[2][:first - 1] == outs[0][:first - 1]
