"""A pan-back world for the covisibility tests, on the conventions of tests/map_worlds.py (BASE_K, 640 x 480, code-word descriptors, the
attributes build_map reads): a camera that turns from region A over a transition strip to region B, stays there for longer than the
default window of 10 keyframes, and comes back.

20 keyframes around one spot, yaw growing: positions 0 - 5 see region A, 4 - 8 the strip, 7 - 19 region B.  1500 points: 300 in A and
120 in the strip carry code words of the 256-bit Hadamard code (any two 128 or 256 bits apart: the query frame sees these), 1080 in B
random descriptors (the query frame does not see B).  A point is observed from keyframes of one parity only (a, a + 2, a + 4, ...), so
no two neighbouring keyframes share a point and the growth step of add_keyframe finds no model (map_worlds' "skip" pattern).  Points
with 1, 2 and 3 observations everywhere, with 6 in B; a dozen points are observed twice in one keyframe, the second time through a
negative key that names the same position.  No keyframe is removed: position = slot.

The query frame stands near keyframe 5 and sees A and the strip.  The seeds are what a frame half-way back (yaw 48 degrees) would have
matched: strip and B points, as a `point` array with -1 entries in between."""
import numpy as np

from tests import track_restatement as TR
from tests.ba_scene import pose, rot
from tests.map_worlds import BASE_K, BASE_SIZE, MapWorld, flip, kps_array, project

N_KF = 20
A_KF, STRIP_KF, B_KF = range(0, 6), range(4, 9), range(7, 20)
YAW = [-6.0, -3.0, 0.0, 3.0, 12.0, 18.0, 40.0, 60.0, 66.0] + [70.0 + 2.5 * k for k in range(11)]   # degrees, by position
N_A, N_STRIP, N_B = 300, 120, 1080
QUERY_YAW, SEED_YAW = 17.0, 48.0


def _camera(yaw_deg, c=(0.0, 0.0, 0.0)):
    """looking along +z turned by yaw about y (x to the right, y down)"""
    return pose(rot([0.0, np.deg2rad(yaw_deg), 0.0]).T, np.asarray(c, np.float64))


class PanBackWorld:
    """the attributes of map_worlds.MapWorld that build_map, the restatements and the tests read"""
    point_dicts = MapWorld.point_dicts
    arrays = MapWorld.arrays

    def __init__(self, seed=41, n_rand=60):
        rng = np.random.default_rng(seed)
        self.K, self.image_size, self.variant, self.removed = BASE_K.copy(), BASE_SIZE, "clean", ()
        self.n_kf0, self.survivors = N_KF, list(range(N_KF))
        W, H = self.image_size
        n_w = N_A + N_STRIP + N_B
        self.region = np.array([0] * N_A + [1] * N_STRIP + [2] * N_B)   # of each world point: A, strip, B
        phi = np.deg2rad(np.concatenate([rng.uniform(-20, 22, N_A), rng.uniform(36, 44, N_STRIP), rng.uniform(66, 104, N_B)]))
        elev = np.deg2rad(rng.uniform(-18, 18, n_w))
        d = rng.uniform(4.0, 10.0, n_w)
        X = np.column_stack([d * np.sin(phi), d * np.tan(elev), d * np.cos(phi)]).astype(np.float32)
        i = np.arange(256)
        par = np.array([[bin(a & b).count("1") & 1 for b in i] for a in i], np.uint8)
        self.code = np.packbits(np.vstack([par, 1 - par]), axis=1) ^ rng.integers(0, 256, (1, 32)).astype(np.uint8)
        base = np.vstack([self.code[:N_A + N_STRIP], rng.integers(0, 256, (N_B, 32)).astype(np.uint8)])
        self.slot_poses = [_camera(y, [0.05 * np.sin(k), 0.02 * np.cos(k), 0.0]) for k, y in enumerate(YAW)]
        vis, xy_all = np.zeros((N_KF, n_w), bool), []
        for k, T in enumerate(self.slot_poses):
            xy, z = project(self.K, T, X)
            xy_all.append(xy)
            vis[k] = (z > 0) & (xy[:, 0] > 5) & (xy[:, 0] < W - 5) & (xy[:, 1] > 5) & (xy[:, 1] < H - 5)
        span = {0: A_KF, 1: STRIP_KF, 2: B_KF}
        seen = [[] for _ in range(n_w)]
        for j in range(n_w):
            ks = [k for k in span[int(self.region[j])] if vis[k, j]]
            par_j = int(rng.integers(0, 2))
            ks = [k for k in ks if k % 2 == par_j]
            if not ks:
                continue
            want = int(rng.choice([1, 2, 3, 6], p=[0.15, 0.2, 0.45, 0.2])) if self.region[j] == 2 else int(rng.choice([1, 2, 3], p=[0.15, 0.25, 0.6]))
            a = int(rng.integers(0, max(len(ks) - want, 0) + 1))
            seen[j] = ks[a:a + want]
        self.base, self.X_world = base, X
        self.slot_xy, self.slot_oct, self.slot_desc = [], [], []
        row_of, self.extra_rows = {}, []
        for k in range(N_KF):
            pts = np.array([j for j in range(n_w) if k in seen[j]], np.int64)
            nr = n_rand + 7 * (k % 5)
            n = len(pts) + nr
            perm = rng.permutation(n)
            kxy, dsc = np.zeros((n, 2), np.float32), np.zeros((n, 32), np.uint8)
            rows = perm[:len(pts)]
            kxy[rows] = xy_all[k][pts]
            dsc[rows] = flip(rng, base[pts], 4)
            kxy[perm[len(pts):]] = np.column_stack([rng.uniform(0, W, nr), rng.uniform(0, H, nr)])
            dsc[perm[len(pts):]] = rng.integers(0, 256, (nr, 32))
            for j, r in zip(pts.tolist(), rows.tolist()):
                row_of[(j, k)] = r
            self.extra_rows.append(perm[len(pts):])
            self.slot_xy.append(kxy); self.slot_oct.append(np.zeros(n, np.int32)); self.slot_desc.append(dsc)
        self.kf_xy, self.kf_oct, self.kf_desc, self.kf_poses = self.slot_xy, self.slot_oct, self.slot_desc, self.slot_poses
        self.counts = np.array([len(x) for x in self.kf_xy], np.int32)
        self.world, self.obs, self.twice = [], [], []
        for j in range(n_w):
            if not seen[j]:
                continue
            o = {k: row_of[(j, k)] for k in seen[j]}
            if len(seen[j]) == 3 and j % 25 == 0:   # observed twice in its middle keyframe: the second key counts from the end
                k = seen[j][1]
                o[k - N_KF] = int(self.extra_rows[k][len(self.twice) % len(self.extra_rows[k])])
                self.twice.append(len(self.world))
            self.world.append(j); self.obs.append(o)
        self.world = np.array(self.world, np.int64)
        self.xyz = X[self.world]
        self.ids = self.world.astype(np.int32)
        off, okf, okp = [0], [], []
        for o in self.obs:
            okf += list(o.keys()); okp += list(o.values())
            off.append(len(okf))
        self.obs_off, self.obs_kf, self.obs_kp = np.array(off, np.int32), np.array(okf, np.int32), np.array(okp, np.int32)
        self.index_of = {int(j): i for i, j in enumerate(self.world)}
        self.point_region = self.region[self.world]
        self.valid = TR.valid_observations(self.obs_off, self.obs_kf, self.obs_kp, self.counts)
        self.a_only = self.point_region == 0   # the points of A: observed from the keyframes 0 - 5 alone
        self.query_pose = _camera(QUERY_YAW, [0.08, -0.03, 0.05])
        self.seed_pose = _camera(SEED_YAW, [0.04, 0.0, 0.02])

    def visible(self, T):
        W, H = self.image_size
        xy, z = project(self.K, T, self.xyz)
        return xy, (z > 0) & (xy[:, 0] > 0) & (xy[:, 0] < W) & (xy[:, 1] > 0) & (xy[:, 1] < H)

    def seeds(self):
        """the `point` array of a frame at seed_pose that matched the strip and B points it sees: one entry per keypoint, -1 between"""
        _, vis = self.visible(self.seed_pose)
        pts = np.flatnonzero(vis & (self.point_region != 0))
        out = np.full(2 * len(pts) + 3, -1, np.int32)
        out[1:2 * len(pts):2] = pts
        return out

    def query(self, seed=9, extra=0.3, flips=8):
        """the frame at query_pose: every map point it sees as a keypoint at its projection with the representative descriptor of the
        point (over all its observations) and up to `flips` bits flipped, `extra` keypoints with unused code words at random places"""
        rng = np.random.default_rng(seed)
        W, H = self.image_size
        rep, _ = TR.representatives(self.valid, self.kf_desc, self.kf_oct, np.ones(len(self.valid), bool))
        xy, vis = self.visible(self.query_pose)
        vis = np.flatnonzero(vis)
        n_extra = int(extra * len(vis))
        spare = self.code[N_A + N_STRIP:]
        d = np.vstack([flip(rng, rep[vis], flips), flip(rng, spare[np.arange(n_extra) % len(spare)], flips)])
        xy = np.vstack([xy[vis], np.column_stack([rng.uniform(0, W, n_extra), rng.uniform(0, H, n_extra)])]).astype(np.float32)
        perm = rng.permutation(len(xy))
        return kps_array(xy[perm]), d[perm]


_W = {}


def pan_back():
    if "w" not in _W:
        _W["w"] = PanBackWorld()
    return _W["w"]
