"""Worlds and cases for the reference-keyframe tracking tests (tests/trackref_restatement.py), in numpy alone so that the CPU tests
restate on them what the GPU tests run: keypoint angles for tests/bow_worlds.RelocWorld, the far frame of the contrast case, small
worlds at the sizes where the kernels take another path, and the restatement of a call on a device map as it stands."""
import numpy as np

from tests import bow_restatement as B
from tests import bow_worlds as BW
from tests import reloc_restatement as RR
from tests import trackref_restatement as TF
from tests.map_worlds import flip, kps_array

ROLL = 30.0          # degrees between a keyframe row's angle and its frame row's: rot / 12 = 2.5, so the noise fills bins 2 and 3
KF = 4               # the reference keyframe of the RelocWorld cases


def uniform_angles(rng, n):
    """n f32 angles in [0, 360)"""
    a = rng.uniform(0.0, 360.0, n).astype(np.float32)
    a[a >= np.float32(360.0)] = 0.0
    return a


def frame_angles(rng, kf_desc, kf_angle, f_desc, roll=ROLL, sigma=2.0, frac_random=0.05, max_bits=10):
    """f32 angles of a frame's rows.  A row of a true point - its descriptor is within max_bits bits of a keyframe row, which is how
    the worlds here make their frames - gets that keyframe row's angle minus `roll`, plus N(0, sigma) degrees, wrapped into [0, 360);
    every other row and frac_random of all rows get a uniform angle."""
    n = len(f_desc)
    out = uniform_angles(rng, n)
    if n and len(kf_desc):
        d = B.hamming(f_desc, kf_desc)
        near = np.argmin(d, axis=1)
        true = d[np.arange(n), near] <= max_bits
        a = np.mod(kf_angle[near].astype(np.float64) - roll + rng.normal(0.0, sigma, n), 360.0).astype(np.float32)
        a[a >= np.float32(360.0)] = 0.0
        keep = true & (rng.random(n) >= frac_random)
        out[keep] = a[keep]
    return out


def with_angles(xy, angle, octave=None):
    k = kps_array(xy, octave)
    k["angle"] = angle
    return k


def far_pose(w, k=KF):
    """the pose of the contrast case: the map's projections land a median 126 px from their keypoints under the keyframe's pose"""
    return w.poses[k] @ BW.pose(BW.rot([0.05, 0.3, 0.3]), np.array([0.8, 0.1, 0.3]))


_CASE = {}


def reloc_keyframes():
    """the RelocWorld's keyframes as keypoint records with the helper's angles, by position"""
    if "kf" not in _CASE:
        w = BW.reloc_world()
        _CASE["kf"] = [with_angles(w.kf_xy[k], uniform_angles(np.random.default_rng(1000 + k), len(w.kf_xy[k]))) for k in range(w.n_kf)]
    return _CASE["kf"]


def reloc_frame(which):
    """(keypoints with angles, descriptors, true pose) of the RelocWorld frames: "near" = query(4, query_pose(4)), "far" = the contrast
    case's frame"""
    if which not in _CASE:
        w = BW.reloc_world()
        T = w.query_pose(KF) if which == "near" else far_pose(w)
        xy, d = w.query(KF, T)
        ang = frame_angles(np.random.default_rng(77), w.kf_desc[KF], reloc_keyframes()[KF]["angle"], d)
        _CASE[which] = (with_angles(xy, ang), d, T)
    return _CASE[which]


def reloc_point_of():
    if "tab" not in _CASE:
        w = BW.reloc_world()
        _CASE["tab"] = RR.point_of(w.obs_off, w.obs_kf, w.obs_kp, [len(d) for d in w.kf_desc])
    return _CASE["tab"]


def reloc_restated(which, n_words, **kw):
    """the restated call on the RelocWorld against keyframe 4 from its stored pose, once per (frame, vocabulary size, parameters)"""
    key = (which, n_words, tuple(sorted(kw.items())))
    if key not in _CASE:
        w = BW.reloc_world()
        words, _, _ = BW.vocabulary("reloc", n_words)
        kps, d, _ = reloc_frame(which)
        _CASE[key] = TF.track_reference(BW.K, w.poses[KF], w.X[w.world], reloc_point_of()[KF], reloc_keyframes()[KF], w.kf_desc[KF],
                                        B.quantise(w.kf_desc[KF], words), kps, d, B.quantise(d, words), n_words, **kw)
    return _CASE[key]


def build_reloc(ctx, capacity=None):
    """BW.RelocWorld.build with the keyframes' angles"""
    from vslam_amd.mapper import LocalMapper
    w = BW.reloc_world()
    kw = {"capacity": capacity} if capacity else {}
    m = LocalMapper(BW.K, save_every_keyframe=False, context=ctx, **kw)
    img = np.zeros((BW.H_IMG, BW.W_IMG), np.uint8)
    for k in range(w.n_kf):
        m.add_keyframe(img, reloc_keyframes()[k], w.kf_desc[k], w.poses[k])
    assert len(m.map_points) == 0
    m.update_map_points([{"id": int(j), "position": w.X[j], "color": np.zeros(3, np.uint8), "observed_keyframes": o} for j, o in zip(w.world, w.obs)])
    return m


class SmallWorld:
    """n_kf keyframes of `rows` rows with independent random descriptors (no growth step finds a model); a tenth of each keyframe's
    rows are near copies of other rows of it, so that candidates dispute frame rows and second distances are small.  n_pts points, point
    i observed by keyframes i % n_kf and (i + 1) % n_kf at rows of their own; bare=True adds a last keyframe that observes nothing."""

    def __init__(self, n_kf=3, rows=70, seed=5, bare=False):
        rng = np.random.default_rng(seed)
        self.n_kf, self.rows = n_kf + (1 if bare else 0), rows
        n_pts = int(0.7 * rows)
        self.X = np.column_stack([rng.uniform(-2.0, 2.0, n_pts), rng.uniform(-1.5, 1.5, n_pts), rng.uniform(4.0, 10.0, n_pts)]).astype(np.float32)
        self.poses = [BW.pose(BW.rot([0.0, 0.01 * k, 0.0]), np.array([0.1 * k, 0.0, 0.0])) for k in range(self.n_kf)]
        self.kf_desc, self.kf_kps = [], []
        for k in range(self.n_kf):
            d = rng.integers(0, 256, (rows, 32)).astype(np.uint8)
            dup = rng.choice(rows, max(rows // 10, 1), replace=False)
            d[dup] = flip(rng, d[(dup + 1) % rows], 2)
            self.kf_desc.append(d)
            xy = np.column_stack([rng.uniform(0, BW.W_IMG, rows), rng.uniform(0, BW.H_IMG, rows)])
            self.kf_kps.append(with_angles(xy, uniform_angles(rng, rows), rng.integers(0, 4, rows)))
        self.obs = [dict() for _ in range(n_pts)]
        for k in range(n_kf):
            at = rng.permutation(rows)[:n_pts]
            xy, _ = BW.project(self.poses[k], self.X.astype(np.float64))
            for i in range(n_pts):
                if k in (i % n_kf, (i + 1) % n_kf):
                    self.obs[i][k] = int(at[i])
                    self.kf_kps[k]["x"][at[i]], self.kf_kps[k]["y"][at[i]] = xy[i]   # (the next keyframe's cull keeps the point)
        off, okf, okp = [0], [], []
        for o in self.obs:
            okf += list(o.keys()); okp += list(o.values())
            off.append(len(okf))
        self.obs_off, self.obs_kf, self.obs_kp = np.array(off, np.int32), np.array(okf, np.int32), np.array(okp, np.int32)

    def vocabulary(self, n_words):
        return B.train(*BW.rows_of(self.kf_desc), n_words, 10)

    def query(self, k, T, n_extra=10, seed=2, angles=True):
        """keyframe k's points seen from T (up to 6 flipped bits), a tenth of them at wrong places, plus n_extra random rows"""
        rng = np.random.default_rng(seed)
        pts = np.array([i for i, o in enumerate(self.obs) if k in o], np.int64)
        rows = np.array([self.obs[i][k] for i in pts], np.int64)
        xy, _ = BW.project(T, self.X[pts].astype(np.float64))
        d = flip(rng, self.kf_desc[k][rows], 6)
        wrong = rng.random(len(xy)) < 0.1
        xy[wrong] = np.column_stack([rng.uniform(0, BW.W_IMG, wrong.sum()), rng.uniform(0, BW.H_IMG, wrong.sum())])
        if n_extra < 0:   # as many rows as the keyframes have
            n_extra = max(self.rows - len(xy), 0)
        xy = np.vstack([xy, np.column_stack([rng.uniform(0, BW.W_IMG, n_extra), rng.uniform(0, BW.H_IMG, n_extra)])])
        d = np.vstack([d, rng.integers(0, 256, (n_extra, 32)).astype(np.uint8)])
        perm = rng.permutation(len(xy))
        xy, d = xy[perm], d[perm]
        ang = frame_angles(rng, self.kf_desc[k], self.kf_kps[k]["angle"], d, max_bits=6) if angles else np.full(len(d), -1.0, np.float32)
        return with_angles(xy, ang, rng.integers(0, 4, len(d))), d

    def build(self, ctx, capacity=None, angles=True):
        from vslam_amd.mapper import LocalMapper
        kw = {"capacity": capacity} if capacity else {}
        m = LocalMapper(BW.K, save_every_keyframe=False, context=ctx, n_hyp=8, **kw)
        img = np.zeros((BW.H_IMG, BW.W_IMG), np.uint8)
        for k in range(self.n_kf):
            kps = self.kf_kps[k].copy()
            if not angles:
                kps["angle"] = -1.0
            m.add_keyframe(img, kps, self.kf_desc[k], self.poses[k])
        assert len(m.map_points) == 0
        m.update_map_points([{"id": i, "position": self.X[i], "color": np.zeros(3, np.uint8), "observed_keyframes": o} for i, o in enumerate(self.obs)])
        return m


def restate_on_map(m, words, kf_position, kps, desc, pose0=None, **kw):
    """the restated call on the device map m as it stands: its arrays, its keyframes' records and descriptors by position"""
    a = m.arrays()
    n_kf = len(m.keyframes)
    pos = kf_position + n_kf if kf_position < 0 else kf_position
    counts = [len(kf["descriptors"]) for kf in m.keyframes]
    tab = RR.point_of(a["obs_off"], a["obs_kf"], a["obs_kp"], counts)[pos]
    kf = m.keyframes[pos]
    kd = np.asarray(kf["descriptors"], np.uint8).reshape(-1, 32)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    return TF.track_reference(BW.K, kf["pose"] if pose0 is None else pose0, a["xyz"], tab, kf["keypoints"], kd, B.quantise(kd, words), kps, desc,
                              B.quantise(desc, words) if len(desc) else np.zeros(0, np.int32), len(words), **kw)
