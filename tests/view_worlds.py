"""A constructed world with real octaves, for the tests of the point views and the frustum mode (tests/test_view_cpu.py,
tests/test_gpu_view.py).  Plain numpy; build() makes the device map and imports the library when called.

Every world point has a physical size S.  Seen from distance d its keypoint has octave floor(log_1.2(S / d) + 0.5): the pyramid level
at which a feature of that size is the detector's patch.  It is observed only where that octave lies in [0, 7].  Under this model
ORB-SLAM2's predicted level L of a point seen again from any distance is the true octave or the one above (scale_gate_holds asserts it),
so the [L - 1, L] gate always contains the true keypoint, while ref_octave +- 1 loses it as soon as the distance changes by 1.2^2.

The scene is a thin slab around the origin (|z| <= 0.5).  Eight keyframes: positions 0 - 4 stand on side A (z < 0, looking along +z) at
the depths of `depths` in turn, positions 5 - 7 on side B (z > 0, looking back along -z).  A point faces side A, side B or both, and has
a parity: it is observed only by keyframes of its parity, so two consecutive keyframes never share a point and no growth step of
add_keyframe finds a model (the rule of tests/test_gpu_relocalize._World).  Each observation is also dropped with probability 0.25, so
the observation lists differ in length and in their first entry."""
import numpy as np

from tests.ba_scene import pose, rot

K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])
W_IMG, H_IMG = 640, 480
SF, N_LEVELS = 1.2, 8
N_KF, N_A = 8, 5


def octave_of(S, d):
    """the scale model: floor(log_1.2(S / d) + 0.5)"""
    return np.floor(np.log(np.asarray(S, np.float64) / np.asarray(d, np.float64)) / np.log(SF) + 0.5).astype(np.int64)


def project(T, X):
    x = (K @ (T[:3, :3] @ np.asarray(X, np.float64).T + T[:3, 3:4])).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return x[:, :2] / x[:, 2:3], x[:, 2]


def centre_of(T):
    return -T[:3, :3].T @ T[:3, 3]


def camera(side, depth, cx=0.0, cy=0.0, tilt=(0.0, 0.0, 0.0)):
    """a camera at (cx, cy, -+depth) looking at the slab: side "A" along +z, side "B" along -z"""
    R = rot(list(tilt)) @ (np.eye(3) if side == "A" else rot([0.0, np.pi, 0.0]))
    return pose(R, np.array([cx, cy, -depth if side == "A" else depth]))


def flip(rng, d, max_bits):
    d = np.array(d, np.uint8).reshape(-1, 32).copy()
    for i in range(len(d)):
        for b in rng.choice(256, rng.integers(0, max_bits + 1), replace=False):
            d[i, b // 8] ^= np.uint8(1 << (b % 8))
    return d


def kps_array(xy, octave):
    import vslam_amd as V
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    k = np.zeros(len(xy), V.KP_DTYPE)
    k["x"] = xy[:, 0]; k["y"] = xy[:, 1]; k["size"] = 31.0; k["octave"] = octave
    return k


class ViewWorld:
    """X [n_w][3] f32, S [n_w], faces [n_w] (1: side A, 2: side B, 3: both), base [n_w][32]; per keyframe position kf_poses, kf_xy,
    kf_oct, kf_desc; the map points in injection order: world (world point of each), xyz, obs (dicts {position: row})"""

    def __init__(self, seed=31, n_w=1200, s_range=(8.0, 40.0), depths=(11.0, 12.0, 13.0), n_rand=150, drop=0.25, layout=None, split_by=None):
        """layout: [(side, depth, cx, cy, group)] per keyframe position in place of the eight above (a point of group g is observed by
        the keyframes of group g only); split_by: an octave difference - every point with exactly two observations whose octaves differ
        by it becomes two map points of one observation each, next to each other (`pairs` lists them)"""
        rng = np.random.default_rng(seed)
        if layout is None:
            layout = [("A" if k < N_A else "B", depths[k % len(depths)], 0.5 * (k % N_A) - 1.0, 0.2 * np.sin(k), k % 2) for k in range(N_KF)]
        n_groups = 1 + max(g for *_, g in layout)
        self.X = np.column_stack([rng.uniform(-4.0, 4.0, n_w), rng.uniform(-3.0, 3.0, n_w), rng.uniform(-0.5, 0.5, n_w)]).astype(np.float32)
        self.S = np.exp(rng.uniform(np.log(s_range[0]), np.log(s_range[1]), n_w))
        self.faces = rng.choice([1, 2, 3], n_w, p=[0.4, 0.2, 0.4])
        group = rng.integers(0, n_groups, n_w)
        self.base = rng.integers(0, 256, (n_w, 32)).astype(np.uint8)
        self.depths = tuple(d for _, d, *_ in layout)
        self.kf_poses, self.kf_side = [], []
        for side, depth, cx, cy, _ in layout:
            self.kf_side.append(side)
            self.kf_poses.append(camera(side, depth, cx, cy, (0.0, rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02))))
        self.kf_xy, self.kf_oct, self.kf_desc = [], [], []
        obs = [dict() for _ in range(n_w)]
        for k, T in enumerate(self.kf_poses):
            xy, z = project(T, self.X)
            d = np.linalg.norm(self.X.astype(np.float64) - centre_of(T), axis=1)
            o = octave_of(self.S, d)
            face = (self.faces & (1 if self.kf_side[k] == "A" else 2)) != 0
            vis = np.flatnonzero(face & (group == layout[k][4]) & (z > 0) & (xy[:, 0] > 5) & (xy[:, 0] < W_IMG - 5) & (xy[:, 1] > 5) & (xy[:, 1] < H_IMG - 5)
                                 & (o >= 0) & (o <= N_LEVELS - 1) & (rng.random(n_w) >= drop))
            n = len(vis) + n_rand
            perm = rng.permutation(n)
            kxy = np.zeros((n, 2), np.float32)
            dsc = np.zeros((n, 32), np.uint8)
            octv = np.zeros(n, np.int32)
            rows = perm[:len(vis)]
            kxy[rows] = xy[vis]; dsc[rows] = flip(rng, self.base[vis], 4); octv[rows] = o[vis]
            kxy[perm[len(vis):]] = np.column_stack([rng.uniform(0, W_IMG, n_rand), rng.uniform(0, H_IMG, n_rand)])
            dsc[perm[len(vis):]] = rng.integers(0, 256, (n_rand, 32))
            octv[perm[len(vis):]] = rng.integers(0, N_LEVELS, n_rand)
            for j, r in zip(vis.tolist(), rows.tolist()):
                obs[j][k] = int(r)
            self.kf_xy.append(kxy); self.kf_oct.append(octv); self.kf_desc.append(dsc)
        self.world, self.obs, self.pairs = [], [], []
        for j in range(n_w):
            items = list(obs[j].items())
            if split_by is not None and len(items) == 2 and abs(int(self.kf_oct[items[0][0]][items[0][1]]) - int(self.kf_oct[items[1][0]][items[1][1]])) == split_by:
                self.pairs.append((len(self.obs), len(self.obs) + 1))
                self.world += [j, j]; self.obs += [dict(items[:1]), dict(items[1:])]
            elif items:
                self.world.append(j); self.obs.append(obs[j])
        self.world = np.array(self.world, np.int64)
        self.xyz = self.X[self.world]
        self.index_of = {int(j): i for i, j in enumerate(self.world)}

    # -- the arrays the restatements read (a map as injected: keys = positions) ---------------------------------------------------------
    def arrays(self):
        from tests.fuse_restatement import as_arrays
        return as_arrays(self.xyz, [list(o.items()) for o in self.obs])

    def kf_P(self):
        from tests.track_restatement import projection_matrix
        return [projection_matrix(K, T) for T in self.kf_poses]

    def point_dicts(self):
        return [{"id": i, "position": self.xyz[i], "color": np.zeros(3, np.uint8), "observed_keyframes": self.obs[i]}
                for i in range(len(self.obs))]

    def build(self, ctx, capacity=None):
        """the world as a device map: the keyframes, then the points with their exact positions and observations"""
        from vslam_amd.mapper import LocalMapper
        kw = {"capacity": capacity} if capacity else {}
        m = LocalMapper(K, save_every_keyframe=False, context=ctx, **kw)
        img = np.zeros((H_IMG, W_IMG), np.uint8)
        for k, T in enumerate(self.kf_poses):
            m.add_keyframe(img, kps_array(self.kf_xy[k], self.kf_oct[k]), self.kf_desc[k], T)
            assert m.last["n_new"] == 0 and len(m.map_points) == 0   # no growth step found a model
        m.update_map_points(self.point_dicts())
        assert len(m.keyframes) == len(self.kf_poses) and len(m.map_points) == len(self.obs)
        return m

    # -- query frames -----------------------------------------------------------------------------------------------------------------
    def query(self, T, faces=3, seed=5, wrong=0.1, extra=0.3, flips=8, clip=True):
        """_query of tests/test_gpu_track_map.py with the scale model: every map point that faces the camera's side (faces: a mask of
        1 = A, 2 = B), is visible from T and whose octave there lies in [0, 7] (clip=False: asserts that none had to be left out) as a
        keypoint at its projection with that octave and its descriptor (up to `flips` bits flipped); a share `wrong` moved by 5 - 12 px of
        its own pyramid level (x 1.2^octave: inside the search window of its level and, like _query's 5 - 12 px at octave 0, beyond the
        inlier threshold sqrt(5.991) 1.2^octave of its information), `extra` random keypoints on top.  Returns (keypoints, descriptors, truth): truth [nq] = the map point of each keypoint that
        stands at its projection (-1: displaced or random)."""
        rng = np.random.default_rng(seed)
        xy, z = project(T, self.xyz)
        d = np.linalg.norm(self.xyz.astype(np.float64) - centre_of(T), axis=1)
        o = octave_of(self.S[self.world], d)
        inside = (z > 0) & (xy[:, 0] > 0) & (xy[:, 0] < W_IMG) & (xy[:, 1] > 0) & (xy[:, 1] < H_IMG) & ((self.faces[self.world] & faces) != 0)
        scale_ok = (o >= 0) & (o <= N_LEVELS - 1)
        if not clip:
            assert scale_ok[inside].all(), "an octave of the query is clipped"
        vis = np.flatnonzero(inside & scale_ok)
        dsc = flip(rng, self.base[self.world[vis]], flips)
        xy = xy[vis]
        truth = vis.copy()
        bad = rng.random(len(vis)) < wrong
        ang = rng.uniform(0, 2 * np.pi, bad.sum())
        xy[bad] += (rng.uniform(5, 12, bad.sum()) * SF ** o[vis][bad])[:, None] * np.column_stack([np.cos(ang), np.sin(ang)])
        truth[bad] = -1
        n_extra = int(extra * len(vis))
        xy = np.vstack([xy, np.column_stack([rng.uniform(0, W_IMG, n_extra), rng.uniform(0, H_IMG, n_extra)])]).astype(np.float32)
        dsc = np.vstack([dsc, rng.integers(0, 256, (n_extra, 32)).astype(np.uint8)])
        octv = np.concatenate([o[vis], rng.integers(0, N_LEVELS, n_extra)]).astype(np.int32)
        truth = np.concatenate([truth, np.full(n_extra, -1)])
        perm = rng.permutation(len(xy))
        return kps_array(xy[perm], octv[perm]), dsc[perm], truth[perm]


def scale_gate_holds(w, T):
    """for every map point of w seen from T with an octave in [0, 7]: the level predicted from its (exact) view contains the true octave
    in [L - 1, L].  Returns the number of points checked."""
    from tests import view_restatement as VR
    from tests.track_restatement import valid_observations
    a = w.arrays()
    obs = valid_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], [len(d) for d in w.kf_desc])
    views = VR.point_views(w.xyz, obs, w.kf_oct, VR.centres(w.kf_P()), SF, N_LEVELS)
    C = centre_of(T)
    d = np.linalg.norm(w.xyz.astype(np.float64) - C, axis=1)
    o = octave_of(w.S[w.world], d)
    n = 0
    for i in np.flatnonzero((o >= 0) & (o <= N_LEVELS - 1)).tolist():
        s, L = 1.0, 0
        while L < N_LEVELS - 1 and d[i] * s < float(views["max_dist"][i]):
            s *= SF
            L += 1
        assert L - 1 <= o[i] <= L, (i, L, o[i])
        n += 1
    return n


# near, near, far, far: keyframes 0 / 2 share the points of group 0, keyframes 1 / 3 those of group 1; neighbours share none
FUSE_LAYOUT = [("A", 7.0, -0.3, 0.1, 0), ("A", 7.0, 0.3, -0.1, 1), ("A", 7.0 * SF ** 3, -0.2, 0.0, 0), ("A", 7.0 * SF ** 3, 0.2, 0.1, 1)]


# ---- the worlds and poses shared by the CPU and the GPU tests, built once ----------------------------------------------------------------
_W = {}


def world(name):
    """"scaled": sizes over a factor of five, octaves 0 - 7 at the keyframes, many points observed by part of the keyframes only;
    "approach": sizes chosen so that a camera at half the depth of the nearest keyframe clips no octave;
    "duplicates": four keyframes of side A, two near and two 1.2^3 times as far; a point is seen by one near and one far keyframe, and
    where its two octaves differ by exactly three it stands in the map twice, once per observation"""
    if name not in _W:
        _W[name] = {"scaled": lambda: ViewWorld(seed=31), "approach": lambda: ViewWorld(seed=33, s_range=(14.5, 19.0)),
                    "duplicates": lambda: ViewWorld(seed=35, n_w=600, s_range=(12.0, 25.0), n_rand=60, drop=0.0, split_by=3, layout=FUSE_LAYOUT)}[name]()
    return _W[name]


def perturbed(T):
    """about 2 degrees and 5 cm off (tests/test_gpu_track_map.py's _perturbed)"""
    return pose(rot([0.005, 0.005, 0.033]), np.array([0.03, -0.03, 0.025])) @ T


def track_pose():
    """a camera of side A near keyframe 2, at a depth of its own"""
    return camera("A", 10.0, 0.3, -0.1, (0.01, -0.02, 0.01))


def approach_pose(w):
    """side A at half the depth of the nearest keyframe: at most half the depth of every keyframe that built the map"""
    return camera("A", 0.5 * min(w.depths), 0.2, 0.1, (0.0, 0.01, -0.01))


def far_side_pose():
    """side B: behind every point that only side A has seen"""
    return camera("B", 12.0, -0.2, 0.1, (0.0, 0.02, 0.0))


def beyond_pose():
    """side A from so far that many points are beyond 1.2 max_dist"""
    return camera("A", 30.0, 0.0, 0.0)


def inside_pose():
    """side A from so near that many points are inside 0.8 min_dist"""
    return camera("A", 2.5, 0.1, 0.0)


# the tracking cases: (world, true pose, which faces the query shows, predicted pose given to the call)
_C = {}


def track_case(name):
    if name not in _C:
        w, T, faces, clip = {"track": lambda: (world("scaled"), track_pose(), 1, True),
                             "approach": lambda: (world("approach"), approach_pose(world("approach")), 1, False),
                             "far_side": lambda: (world("scaled"), far_side_pose(), 2, True),
                             "beyond": lambda: (world("scaled"), beyond_pose(), 1, True),
                             "inside": lambda: (world("scaled"), inside_pose(), 1, True)}[name]()
        kps, desc, truth = w.query(T, faces=faces, clip=clip)
        _C[name] = {"w": w, "T": T, "pose0": perturbed(T) if name in ("track", "approach") else T, "kps": kps, "desc": desc, "truth": truth}
    return _C[name]


TRACK_CASES = ("track", "approach", "far_side", "beyond", "inside")
