"""LocalMapper.track_local_map (mo_map_track) on the device against the numpy restatement (tests/track_restatement.py) and against
known poses."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import track_restatement as TR
from tests.test_gpu_relocalize import H_IMG, K, W_IMG, _World, _ctx, _flip, _kps, _pose, _project, _rot, _rot_deg, _sequence_map

pytestmark = pytest.mark.gpu


def _query(w, T, noise=0.0, seed=5):
    """every map point visible from T as a keypoint at its projection (+ noise) with its descriptor and up to 8 more bits flipped; 10 %
    of them moved by 5 - 12 px (wrong matches the search still finds), plus 30 % random distractor keypoints"""
    rng = np.random.default_rng(seed)
    a = w.m.arrays()
    xy, z = _project(T, a["xyz"].astype(np.float64))
    vis = np.flatnonzero((z > 0) & (xy[:, 0] > 0) & (xy[:, 0] < W_IMG) & (xy[:, 1] > 0) & (xy[:, 1] < H_IMG))
    d = _flip(rng, w.base[a["id"][vis]], 8)
    xy = xy[vis] + (rng.normal(0, noise, (len(vis), 2)) if noise else 0.0)
    wrong = rng.random(len(vis)) < 0.1
    ang = rng.uniform(0, 2 * np.pi, wrong.sum())
    xy[wrong] += rng.uniform(5, 12, wrong.sum())[:, None] * np.column_stack([np.cos(ang), np.sin(ang)])
    n_extra = int(0.3 * len(vis))
    xy = np.vstack([xy, np.column_stack([rng.uniform(0, W_IMG, n_extra), rng.uniform(0, H_IMG, n_extra)])]).astype(np.float32)
    d = np.vstack([d, rng.integers(0, 256, (n_extra, 32)).astype(np.uint8)])
    perm = rng.permutation(len(xy))
    return _kps(xy[perm]), d[perm]


def _restate(m, kps, desc, pose0, **kw):
    a = m.arrays()
    kf_desc = [np.asarray(kf["descriptors"]) for kf in m.keyframes]
    kf_oct = [np.asarray(kf["keypoints"])["octave"] for kf in m.keyframes]
    return TR.track(K if "K" not in kw else kw.pop("K"), pose0, a["xyz"], a["obs_off"], a["obs_kf"], a["obs_kp"], kf_desc, kf_oct, kps, desc,
                    W_IMG if "w" not in kw else kw.pop("w"), H_IMG if "h" not in kw else kw.pop("h"), **kw)


def _perturbed(T):
    """about 2 degrees (mostly about the optical axis) and 5 cm off"""
    return _pose(_rot([0.005, 0.005, 0.033]), np.array([0.03, -0.03, 0.025])) @ T


def _same_pass(info, ps, k):
    assert info["pass_cand"][k] == ps["cand"] and info["pass_matches"][k] == ps["matches"] and info["pass_radius"][k] == ps["radius"]


@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_constructed_map(noise):
    ctx = _ctx()
    w = _World(ctx)
    T = w.poses[6] @ _pose(_rot([0.01, -0.02, 0.01]), np.array([0.1, -0.05, 0.05]))
    pose0 = _perturbed(T)
    kps, desc = _query(w, T, noise=noise)
    # pass 1 alone: integers equal to the restatement from pose0
    ok1, _, i1 = w.m.track_local_map(kps, desc, pose0, radii=(15.0,))
    r1 = _restate(w.m, kps, desc, pose0, radii=(15.0,), refine_pose=False)
    assert i1["n_local"] == r1["n_local"]
    assert np.array_equal(i1["point"], r1["passes"][0]["point"]) and np.array_equal(i1["dist"], r1["passes"][0]["dist"])
    _same_pass(i1, r1["passes"][0], 0)
    # two passes: pass 2 equal to the restatement from the device's pass-1 pose; the final pose = the restated refinement of the device's
    # matches from that pose
    ok, pose, info = w.m.track_local_map(kps, desc, pose0)
    assert info["n_pass_run"] == 2 and np.array_equal(info["pass_pose"][0], i1["pass_pose"][0])
    r2 = _restate(w.m, kps, desc, pose0, poses=[pose0, info["pass_pose"][0]], refine_pose=False)
    assert np.array_equal(info["point"], r2["passes"][1]["point"]) and np.array_equal(info["dist"], r2["passes"][1]["dist"])
    _same_pass(info, r2["passes"][1], 1)
    q = np.flatnonzero(info["point"] >= 0)
    a = w.m.arrays()
    ref, inl, n_inl = TR.refine(K, info["pass_pose"][0], a["xyz"][info["point"][q]].astype(np.float64),
                                np.column_stack([kps["x"][q], kps["y"][q]]).astype(np.float64), kps["octave"][q])
    assert np.allclose(pose, ref, rtol=1e-9, atol=1e-9), pose - ref
    assert np.array_equal(info["inlier"][q], inl) and not info["inlier"][info["point"] < 0].any()
    assert info["pass_inliers"][1] == n_inl == int(info["inlier"].sum())
    rot, terr = _rot_deg(pose[:3, :3], T[:3, :3]), np.linalg.norm(pose[:3, 3] - T[:3, 3])
    print("noise %.1f: %s candidates, %s matches, %s inliers, rotation error %.2e deg, translation error %.2e"
          % (noise, info["pass_cand"], info["pass_matches"], info["pass_inliers"], rot, terr))
    assert ok and n_inl >= 30
    if noise == 0.0:
        assert np.abs(pose - T).max() < 1e-6, pose - T
    else:
        assert rot < 0.1 and terr < 1e-3 * np.linalg.norm(T[:3, 3])
    w.m.close(); ctx.close()


def test_retry_then_refine_over_three_passes():
    """a first radius too small for min_matches: the retry at twice the radius succeeds and is refined, then two more passes run; every
    pass's counts, the last pass's matches and the first refinement equal the restatement"""
    ctx = _ctx()
    w = _World(ctx)
    T = w.poses[4] @ _pose(_rot([0.01, 0.02, -0.01]), np.array([-0.05, 0.04, 0.06]))
    pose0 = _pose(_rot([0.0, 0.003, 0.0]), np.zeros(3)) @ T   # every projection ~1.5 px off
    kps, desc = _query(w, T, seed=13)
    radii = (1.0, 4.0, 4.0)
    ok, pose, info = w.m.track_local_map(kps, desc, pose0, radii=radii)
    assert info["n_pass_run"] == 3 and info["pass_radius"] == [2.0, 4.0, 4.0], info["pass_radius"]
    r = _restate(w.m, kps, desc, pose0, radii=radii, refine_pose=False, poses=[pose0] + info["pass_pose"][:2])
    for k in range(3):
        _same_pass(info, r["passes"][k], k)
    assert np.array_equal(info["point"], r["passes"][2]["point"]) and np.array_equal(info["dist"], r["passes"][2]["dist"])
    # the refinement of the retried pass, restated on the restated matches of that pass
    p0 = r["passes"][0]["point"]
    q = np.flatnonzero(p0 >= 0)
    a = w.m.arrays()
    ref, _, n_inl = TR.refine(K, pose0, a["xyz"][p0[q]].astype(np.float64), np.column_stack([kps["x"][q], kps["y"][q]]).astype(np.float64),
                              kps["octave"][q])
    assert np.allclose(info["pass_pose"][0], ref, rtol=1e-9, atol=1e-9) and info["pass_inliers"][0] == n_inl
    assert ok and np.abs(pose - T).max() < 1e-6
    w.m.close(); ctx.close()


def test_window():
    ctx = _ctx()
    w = _World(ctx)
    T = w.poses[5]
    kps, desc = _query(w, T, seed=9)
    a = w.m.arrays()
    n_kf = len(w.m.keyframes)
    obs = TR.valid_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], [len(kf["descriptors"]) for kf in w.m.keyframes])
    in_window = TR.local_points(obs, n_kf, 2)
    ok, _, info = w.m.track_local_map(kps, desc, T, window=2, radii=(8.0,), min_matches=1, min_inliers=1)
    r = _restate(w.m, kps, desc, T, window=2, radii=(8.0,), min_matches=1, min_inliers=1, refine_pose=False)
    assert info["n_local"] == r["n_local"] == int(in_window.sum()) < len(obs)
    assert np.array_equal(info["point"], r["passes"][0]["point"])
    matched = info["point"][info["point"] >= 0]
    assert len(matched) > 0 and in_window[matched].all()
    ok0, _, info0 = w.m.track_local_map(kps, desc, T, window=0, radii=(8.0,))
    assert info0["n_local"] == len(obs)
    m0 = info0["point"][info0["point"] >= 0]
    assert (~in_window[m0]).any() and len(m0) > len(matched)
    w.m.close(); ctx.close()


def _nothing(ok, pose, info, n, pose0):
    assert not ok and len(info["point"]) == n and (info["point"] == -1).all() and (info["dist"] == -1).all() and not info["inlier"].any()
    assert np.array_equal(pose, pose0)


def test_degenerate_inputs():
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    rng = np.random.default_rng(8)
    kps = _kps(np.column_stack([rng.uniform(0, 640, 300), rng.uniform(0, 480, 300)]).astype(np.float32))
    desc = rng.integers(0, 256, (300, 32)).astype(np.uint8)
    pose0 = np.eye(4)
    empty = LocalMapper(K, save_every_keyframe=False, context=ctx)
    ok, pose, info = empty.track_local_map(kps, desc, pose0)
    _nothing(ok, pose, info, 300, pose0)
    assert info["n_pass_run"] == 0 and info["n_local"] == 0
    empty.add_keyframe(np.zeros((H_IMG, W_IMG), np.uint8), kps, desc, pose0)   # one keyframe, no map point
    ok, pose, info = empty.track_local_map(kps, desc, pose0)
    _nothing(ok, pose, info, 300, pose0)
    w = _World(ctx)
    ok, pose, info = w.m.track_local_map(np.zeros(0, V.KP_DTYPE), np.zeros((0, 32), np.uint8), w.poses[3])
    _nothing(ok, pose, info, 0, w.poses[3])
    away = _pose(_rot([0.0, np.pi, 0.0]), np.zeros(3)) @ w.poses[3]   # looking away from every point
    ok, pose, info = w.m.track_local_map(kps, desc, away)
    _nothing(ok, pose, info, 300, away)
    assert info["n_pass_run"] == 1 and info["pass_cand"] == [0] and info["pass_matches"] == [0] and info["pass_radius"] == [30.0]
    assert info["n_local"] > 0
    empty.close(); w.m.close(); ctx.close()


def _same(a, b):
    (oa, pa, ia), (ob, pb, ib) = a, b
    assert oa == ob and np.array_equal(pa, pb)
    for f in ("point", "dist", "inlier"):
        assert np.array_equal(ia[f], ib[f]), f
    for f in ("pass_radius", "pass_cand", "pass_matches", "pass_inliers", "n_local", "n_pass_run"):
        assert ia[f] == ib[f], f
    assert all(np.array_equal(x, y) for x, y in zip(ia["pass_pose"], ib["pass_pose"]))


_SC = {}


def _scene():
    if not _SC:
        import torch
        from vslam_amd.synth import Survey8dScene
        _SC["sc"] = Survey8dScene(torch, "cpu")
    return _SC["sc"]


def test_real_images_paths_and_determinism():
    """the survey8d keyframes (every second frame, ground-truth poses); the odd frames in between tracked from the constant-velocity
    prediction of the two frames before them"""
    import vslam_amd as V
    from vslam_amd.mapper import predict_pose
    from tests.test_gpu_mapper import _rz
    from vslam_amd.synth import frame_roll_deg
    ctx = _ctx()
    m, _, _ = _sequence_map(ctx)
    sc = _scene()

    def truth(g):
        R = _rz(np.deg2rad(frame_roll_deg(sc.seed, g)))
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = -R @ np.array([g * 0.05, 0.0, 0.0])
        return T
    prm = V.orb_params(nfeatures=2000)
    worst_r, worst_t, first = 0.0, 0.0, None
    for k in range(1, 11):
        g = 2 * k + 1
        fr = sc.frame(g).numpy()
        (kps, desc), = ctx.orb_detect_compute(fr, prm)
        kh, dh = np.array(kps).copy(), np.array(desc).copy()
        pred = predict_pose(truth(g - 2), truth(g - 1))
        res = m.track_local_map(kps, desc, pred)
        ok, pose, info = res
        T = truth(g)
        rot, terr = _rot_deg(pose[:3, :3], T[:3, :3]), np.linalg.norm(pose[:3, 3] - T[:3, 3])
        print("frame %d: ok %s, %d local, candidates %s, matches %s, inliers %s, rotation error %.4f deg, translation error %.2e (%.3f %% "
              "of 0.05)" % (g, ok, info["n_local"], info["pass_cand"], info["pass_matches"], info["pass_inliers"], rot, terr, 100 * terr / 0.05))
        assert info["from_token"]
        assert ok, info
        worst_r, worst_t = max(worst_r, rot), max(worst_t, terr)
        if first is None:
            first = (kh, dh, pred, res)
    print("worst: rotation %.4f deg, translation %.2e (%.3f %% of 0.05)" % (worst_r, worst_t, 100 * worst_t / 0.05))
    # measured on an MI355X: worst 0.076 deg and 2.38 % of the 0.05 baseline (frame 9).  The relocalization bound of 1 % does not hold
    # here: the points were triangulated from detected keypoints over two-frame baselines (and keyframe 5's pose is perturbed on purpose),
    # and a frame between keyframes inherits their depth errors; the restatement tests above pin the arithmetic itself
    assert worst_r < 0.1 and worst_t < 0.03 * 0.05
    # the map is not changed; the same call twice; the host arrays equal the token path; a map with tiny capacities agrees
    kh, dh, pred, res = first
    before = {f: v.copy() for f, v in m.arrays().items()}
    lo, ids = (x.copy() for x in m.list_arrays())
    host = m.track_local_map(kh, dh, pred)
    assert not host[2]["from_token"]
    _same(res, host)
    _same(host, m.track_local_map(kh, dh, pred))
    m._cache = None; m._lists = None
    after = m.arrays()
    assert all(np.array_equal(before[f], after[f]) for f in before)
    assert all(np.array_equal(x, y) for x, y in zip((lo, ids), m.list_arrays()))
    m2, _, _ = _sequence_map(ctx, capacity=(2, 16, 16, 32))
    _same(host, m2.track_local_map(kh, dh, pred))
    m.close(); m2.close(); ctx.close()


def test_run_frames_tracks_against_the_map(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "visual-slam_amd", "examples"))
    try:
        from run_frames import synthetic_sequence
    finally:
        sys.path.pop(0)
    path = tmp_path / "frames.npy"
    np.save(path, np.stack(list(synthetic_sequence(40, seed=7))))
    r = subprocess.run([sys.executable, os.path.join(root, "visual-slam_amd", "examples", "run_frames.py"), "--frames", str(path), "--max-frames", "40",
                        "--keyframe-every", "5", "--map", str(tmp_path / "map.ply"), "--track-map"], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ": track map " in ln]
    print("\n".join(lines))
    assert lines, r.stdout[-3000:]
