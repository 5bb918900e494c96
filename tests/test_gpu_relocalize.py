"""LocalMapper.relocalize (mo_map_relocalize) on the device against the numpy restatement of its integer steps
(tests/reloc_restatement.py) and against known poses."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.reloc_restatement import restate

pytestmark = pytest.mark.gpu

K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])
W_IMG, H_IMG = 640, 480


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _rot(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _pose(R, c):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ c
    return T


def _project(T, X):
    x = (K @ (T[:3, :3] @ X.T + T[:3, 3:4])).T
    return x[:, :2] / x[:, 2:3], x[:, 2]


def _flip(rng, d, max_bits):
    d = d.copy()
    for i in range(len(d)):
        for b in rng.choice(256, rng.integers(0, max_bits + 1), replace=False):
            d[i, b // 8] ^= np.uint8(1 << (b % 8))
    return d


def _kps(xy):
    import vslam_amd as V
    k = np.zeros(len(xy), V.KP_DTYPE)
    k["x"] = xy[:, 0]; k["y"] = xy[:, 1]; k["size"] = 31.0
    return k


class _World:
    """eight keyframes along x, 5000 points each observed by keyframes a, a + 2, a + 4 (where visible) with its own descriptor (up to
    4 bits flipped per keyframe), rows shuffled among 400 random rows per keyframe; the points injected with exact positions and
    observations after the keyframes.  Consecutive keyframes share no descriptor: no growth step finds a model."""

    def __init__(self, ctx, capacity=None, seed=21):
        from vslam_amd.mapper import LocalMapper
        rng = np.random.default_rng(seed)
        self.rng = rng
        n_w, n_kf = 5000, 8
        self.X = np.column_stack([rng.uniform(-3.0, 5.5, n_w), rng.uniform(-2.0, 2.0, n_w), rng.uniform(3.0, 12.0, n_w)]).astype(np.float32)
        self.base = rng.integers(0, 256, (n_w, 32)).astype(np.uint8)
        win = rng.integers(0, n_kf, n_w)
        self.poses = [_pose(_rot([0.0, rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02)]), np.array([0.35 * k, 0.05 * np.sin(k), 0.0]))
                      for k in range(n_kf)]
        kw = {"capacity": capacity} if capacity else {}
        self.m = LocalMapper(K, save_every_keyframe=False, context=ctx, **kw)
        self.rows, self.desc = [], []
        obs = [dict() for _ in range(n_w)]
        img = np.zeros((H_IMG, W_IMG), np.uint8)
        for k, T in enumerate(self.poses):
            xy, z = _project(T, self.X.astype(np.float64))
            vis = np.flatnonzero((win <= k) & (k <= win + 4) & ((k - win) % 2 == 0) & (z > 0) & (xy[:, 0] > 5) & (xy[:, 0] < W_IMG - 5) & (xy[:, 1] > 5)
                                 & (xy[:, 1] < H_IMG - 5))
            n_rand = 400
            n = len(vis) + n_rand
            perm = rng.permutation(n)
            kxy = np.zeros((n, 2), np.float32)
            d = np.zeros((n, 32), np.uint8)
            kxy[perm[:len(vis)]] = xy[vis]
            d[perm[:len(vis)]] = _flip(rng, self.base[vis], 4)
            kxy[perm[len(vis):]] = np.column_stack([rng.uniform(0, W_IMG, n_rand), rng.uniform(0, H_IMG, n_rand)])
            d[perm[len(vis):]] = rng.integers(0, 256, (n_rand, 32))
            for j, r in zip(vis, perm[:len(vis)]):
                obs[j][k] = int(r)
            self.m.add_keyframe(img, _kps(kxy), d, T)
            self.rows.append(perm[:len(vis)]); self.desc.append(d)
        self.obs = obs
        assert len(self.m.map_points) == 0
        self.m.update_map_points([{"id": j, "position": self.X[j], "color": np.zeros(3, np.uint8), "observed_keyframes": obs[j]}
                                  for j in range(n_w) if obs[j]])
        assert len(self.m.keyframes) == n_kf

    def query(self, k, T, noise=0.0, seed=5):
        """keyframe k's visible points seen from T (descriptors with up to 10 flipped bits), 20 % of them moved to wrong positions,
        plus random extra keypoints (together ~35 % outliers)"""
        rng = np.random.default_rng(seed)
        a = self.m.arrays()
        pts = [i for i in range(len(a["id"])) if k in dict(zip(a["obs_kf"][a["obs_off"][i]:a["obs_off"][i + 1]].tolist(),
                                                                   a["obs_kp"][a["obs_off"][i]:a["obs_off"][i + 1]].tolist()))]
        pts = np.array(pts)
        xyz = a["xyz"][pts].astype(np.float64)
        xy, z = _project(T, xyz)
        vis = (z > 0) & (xy[:, 0] > 0) & (xy[:, 0] < W_IMG) & (xy[:, 1] > 0) & (xy[:, 1] < H_IMG)
        pts, xy = pts[vis], xy[vis]
        rows = np.array([dict(zip(a["obs_kf"][a["obs_off"][i]:a["obs_off"][i + 1]].tolist(),
                                  a["obs_kp"][a["obs_off"][i]:a["obs_off"][i + 1]].tolist()))[k] for i in pts])
        d = _flip(rng, self.desc[k][rows], 10)
        xy = xy + rng.normal(0, noise, xy.shape) if noise else xy
        wrong = rng.random(len(xy)) < 0.2
        xy[wrong] = np.column_stack([rng.uniform(0, W_IMG, wrong.sum()), rng.uniform(0, H_IMG, wrong.sum())])
        n_extra = int(0.15 * len(xy))
        xy = np.vstack([xy, np.column_stack([rng.uniform(0, W_IMG, n_extra), rng.uniform(0, H_IMG, n_extra)])]).astype(np.float32)
        d = np.vstack([d, rng.integers(0, 256, (n_extra, 32)).astype(np.uint8)])
        perm = rng.permutation(len(xy))
        return _kps(xy[perm]), d[perm]


def _restated(w, q_desc, max_candidates=4):
    a = w.m.arrays()
    return restate(q_desc, [kf["descriptors"] for kf in w.m.keyframes], a["obs_off"], a["obs_kf"], a["obs_kp"], 0.75, max_candidates)


def _recheck(w, kps, info, pose, thr=3.0):
    """inlier flags of the returned pose recomputed in numpy (f64), with the correspondences within 1e-9 of the threshold exempt"""
    a = w.m.arrays()
    q = np.flatnonzero(info["point"] >= 0)
    X = a["xyz"][info["point"][q]].astype(np.float64)
    P = K @ pose[:3, :]
    x = (P @ np.column_stack([X, np.ones(len(X))]).T).T
    e2 = (x[:, 0] / x[:, 2] - kps["x"][q].astype(np.float64)) ** 2 + (x[:, 1] / x[:, 2] - kps["y"][q].astype(np.float64)) ** 2
    want = (x[:, 2] > 0) & (e2 < thr * thr)
    exempt = np.abs(e2 - thr * thr) < 1e-9
    got = info["inlier"][q]
    assert not info["inlier"][info["point"] < 0].any()
    assert np.array_equal(got[~exempt], want[~exempt]), (got != want).sum()


def _rot_deg(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_constructed_map(noise):
    ctx = _ctx()
    w = _World(ctx)
    k = 5
    T = w.poses[k] @ _pose(_rot([0.02, -0.03, 0.01]), np.array([0.08, -0.05, 0.1]))
    kps, desc = w.query(k, T, noise=noise)
    ok, pose, info = w.m.relocalize(kps, desc)
    r = _restated(w, desc)
    # integer results: bit-equal to the restatement
    assert [c[0] for c in info["candidates"]] == r["candidates"]
    assert [c[1] for c in info["candidates"]] == [r["scores"][p] for p in r["candidates"]]
    qi, pi = r["C"][info["kf_pos"]]
    assert np.array_equal(np.flatnonzero(info["point"] >= 0), qi) and np.array_equal(info["point"][qi], pi)
    assert info["n_corr"] == len(qi)
    # the right keyframe and pose
    assert ok and info["kf_pos"] == k and info["kf_id"] == w.m.keyframes[k]["id"], info["candidates"]
    assert len(info["candidates"]) >= 2
    if noise == 0.0:
        assert np.abs(pose[:3, :3] - T[:3, :3]).max() < 1e-6 and np.abs(pose[:3, 3] - T[:3, 3]).max() < 1e-6, pose - T
    else:
        print("0.5 px noise: rotation error %.4f deg, translation error %.3g of %.3g" % (_rot_deg(pose[:3, :3], T[:3, :3]),
                                                                                   np.linalg.norm(pose[:3, 3] - T[:3, 3]), np.linalg.norm(T[:3, 3])))
        assert _rot_deg(pose[:3, :3], T[:3, :3]) < 0.1
        assert np.linalg.norm(pose[:3, 3] - T[:3, 3]) < 1e-3 * np.linalg.norm(T[:3, 3])
    _recheck(w, kps, info, pose)
    assert info["n_inliers"] == int(info["inlier"].sum()) >= 50
    w.m.close(); ctx.close()


def test_nothing_to_find():
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    rng = np.random.default_rng(8)
    empty = LocalMapper(K, save_every_keyframe=False, context=ctx)
    kps = _kps(np.column_stack([rng.uniform(0, 640, 500), rng.uniform(0, 480, 500)]).astype(np.float32))
    desc = rng.integers(0, 256, (500, 32)).astype(np.uint8)
    ok, pose, info = empty.relocalize(kps, desc)
    assert not ok and pose is None and info["kf_pos"] == -1 and info["candidates"] == []
    w = _World(ctx)
    ok, pose, info = w.m.relocalize(kps, desc)
    assert not ok and info["candidates"] == [] and (info["point"] == -1).all()
    ok, pose, info = w.m.relocalize(np.zeros(0, V.KP_DTYPE), np.zeros((0, 32), np.uint8))
    assert not ok and pose is None
    empty.close(); w.m.close(); ctx.close()


def test_relocalize_does_not_change_the_map():
    ctx = _ctx()
    w = _World(ctx)
    before = {f: v.copy() for f, v in w.m.arrays().items()}
    lo, ids = (x.copy() for x in w.m.list_arrays())
    kps, desc = w.query(3, w.poses[3])
    w.m.relocalize(kps, desc)
    w.m._cache = None; w.m._lists = None
    after = w.m.arrays()
    assert all(np.array_equal(before[f], after[f]) for f in before)
    assert all(np.array_equal(a, b) for a, b in zip((lo, ids), w.m.list_arrays()))
    w.m.close(); ctx.close()


def _same(a, b):
    (oa, pa, ia), (ob, pb, ib) = a, b
    assert oa == ob and ia["candidates"] == ib["candidates"] and ia["kf_pos"] == ib["kf_pos"]
    assert np.array_equal(ia["point"], ib["point"]) and np.array_equal(ia["inlier"], ib["inlier"])
    assert (pa is None and pb is None) or np.array_equal(pa, pb)


_SEQ = {}


def _sequence_map(ctx, capacity=None):
    """the twelve-keyframe survey8d sequence of test_gpu_mapper (every second frame, ground-truth poses), real detect_and_compute"""
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    from tests.test_gpu_mapper import K as KM, _sequence
    frames, poses = _sequence()
    kw = {"capacity": capacity} if capacity else {}
    m = LocalMapper(KM, save_every_keyframe=False, context=ctx, **kw)
    prm = V.orb_params(nfeatures=2000)
    for fr, T in zip(frames, poses):
        (kps, desc), = ctx.orb_detect_compute(fr, prm)
        m.add_keyframe(fr, kps, desc, T)
    return m, frames, poses


def test_pipeline_self_consistency_paths_and_determinism():
    import vslam_amd as V
    ctx = _ctx()
    m, frames, poses = _sequence_map(ctx)
    j = 8
    kf = m.keyframes[j]
    kps, desc = np.array(kf["keypoints"]).copy(), np.array(kf["descriptors"]).copy()
    res = m.relocalize(kps, desc)
    ok, pose, info = res
    assert ok and info["kf_pos"] == j, info["candidates"]
    rot = _rot_deg(pose[:3, :3], poses[j][:3, :3])
    base = np.linalg.norm((poses[j] @ np.linalg.inv(poses[j - 1]))[:3, 3])
    terr = np.linalg.norm(pose[:3, 3] - poses[j][:3, 3])
    print("self-consistency: keyframe %d, %d inliers of %d, rotation error %.4f deg, translation error %.3g (%.2f %% of the baseline)"
          % (j, info["n_inliers"], info["n_corr"], rot, terr, 100 * terr / base))
    assert rot < 0.1 and terr < 0.01 * base
    # the same call twice, and by token (the frame detected again: resident on the device) against the host arrays
    _same(res, m.relocalize(kps, desc))
    (k2, d2), = ctx.orb_detect_compute(frames[j], V.orb_params(nfeatures=2000))
    assert V.resident_token(ctx, d2)
    tok = m.relocalize(k2, d2)
    assert tok[2]["from_token"] and not res[2]["from_token"]
    _same(res, tok)
    # a map built with tiny capacities (every buffer regrown) gives the same result
    m2, _, _ = _sequence_map(ctx, capacity=(2, 16, 16, 32))
    _same(res, m2.relocalize(kps, desc))
    m.close(); m2.close(); ctx.close()


def test_run_frames_relocalizes_after_a_break(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "visual-slam_amd", "examples"))
    try:
        from run_frames import synthetic_sequence
    finally:
        sys.path.pop(0)
    frames = np.stack(list(synthetic_sequence(40, seed=7)))
    other = np.stack(list(synthetic_sequence(40, seed=99)))
    frames[26:29] = other[26:29]
    path = tmp_path / "frames.npy"
    np.save(path, frames)
    r = subprocess.run([sys.executable, os.path.join(root, "visual-slam_amd", "examples", "run_frames.py"), "--frames", str(path), "--max-frames", "40",
                        "--keyframe-every", "5", "--map", str(tmp_path / "map.ply"), "--relocalize"], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ": relocalize " in ln]
    print("\n".join(lines))
    assert any(": relocalize ok" in ln for ln in lines), r.stdout[-3000:]
