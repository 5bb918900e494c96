"""Worlds for the place-recognition tests, in numpy alone so that the CPU tests can restate on them what the GPU tests run.

RelocWorld is built like `_World` of tests/test_gpu_relocalize.py: eight keyframes along x, 5000 points each observed by keyframes
a, a + 2, a + 4 (where visible) with its own descriptor (up to 4 bits flipped per keyframe), rows shuffled among 400 random rows per
keyframe; consecutive keyframes share no descriptor, so no growth step finds a model and the points are injected with exact positions
and observations after the keyframes.  build(ctx) makes the device map of it."""
import numpy as np

from tests.map_worlds import flip, kps_array

K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])
W_IMG, H_IMG = 640, 480


def rot(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def pose(R, c):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ c
    return T


def project(T, X):
    x = (K @ (T[:3, :3] @ X.T + T[:3, 3:4])).T
    return x[:, :2] / x[:, 2:3], x[:, 2]


class RelocWorld:
    def __init__(self, seed=21, n_w=5000, n_kf=8, n_rand=400):
        rng = np.random.default_rng(seed)
        self.n_kf = n_kf
        self.X = np.column_stack([rng.uniform(-3.0, 5.5, n_w), rng.uniform(-2.0, 2.0, n_w), rng.uniform(3.0, 12.0, n_w)]).astype(np.float32)
        self.base = rng.integers(0, 256, (n_w, 32)).astype(np.uint8)
        win = rng.integers(0, n_kf, n_w)
        self.poses = [pose(rot([0.0, rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02)]), np.array([0.35 * k, 0.05 * np.sin(k), 0.0]))
                      for k in range(n_kf)]
        self.kf_xy, self.kf_desc = [], []
        obs = [dict() for _ in range(n_w)]
        for k, T in enumerate(self.poses):
            xy, z = project(T, self.X.astype(np.float64))
            vis = np.flatnonzero((win <= k) & (k <= win + 4) & ((k - win) % 2 == 0) & (z > 0) & (xy[:, 0] > 5) & (xy[:, 0] < W_IMG - 5) & (xy[:, 1] > 5)
                                 & (xy[:, 1] < H_IMG - 5))
            n = len(vis) + n_rand
            perm = rng.permutation(n)
            kxy = np.zeros((n, 2), np.float32)
            d = np.zeros((n, 32), np.uint8)
            kxy[perm[:len(vis)]] = xy[vis]
            d[perm[:len(vis)]] = flip(rng, self.base[vis], 4)
            kxy[perm[len(vis):]] = np.column_stack([rng.uniform(0, W_IMG, n_rand), rng.uniform(0, H_IMG, n_rand)])
            d[perm[len(vis):]] = rng.integers(0, 256, (n_rand, 32))
            for j, r in zip(vis, perm[:len(vis)]):
                obs[j][k] = int(r)
            self.kf_xy.append(kxy); self.kf_desc.append(d)
        self.world = np.array([j for j in range(n_w) if obs[j]], np.int64)   # the map points in injection order
        self.obs = [obs[j] for j in self.world]
        off, okf, okp = [0], [], []
        for o in self.obs:
            okf += list(o.keys()); okp += list(o.values())
            off.append(len(okf))
        self.obs_off, self.obs_kf, self.obs_kp = np.array(off, np.int32), np.array(okf, np.int32), np.array(okp, np.int32)

    def query(self, k, T, seed=5):
        """keyframe k's points seen from T (descriptors with up to 10 flipped bits), 20 % of them moved to wrong positions, plus random
        extra keypoints"""
        rng = np.random.default_rng(seed)
        pts = np.array([i for i, o in enumerate(self.obs) if k in o])
        xy, z = project(T, self.X[self.world[pts]].astype(np.float64))
        vis = (z > 0) & (xy[:, 0] > 0) & (xy[:, 0] < W_IMG) & (xy[:, 1] > 0) & (xy[:, 1] < H_IMG)
        pts, xy = pts[vis], xy[vis]
        rows = np.array([self.obs[i][k] for i in pts])
        d = flip(rng, self.kf_desc[k][rows], 10)
        wrong = rng.random(len(xy)) < 0.2
        xy[wrong] = np.column_stack([rng.uniform(0, W_IMG, wrong.sum()), rng.uniform(0, H_IMG, wrong.sum())])
        n_extra = int(0.15 * len(xy))
        xy = np.vstack([xy, np.column_stack([rng.uniform(0, W_IMG, n_extra), rng.uniform(0, H_IMG, n_extra)])]).astype(np.float32)
        d = np.vstack([d, rng.integers(0, 256, (n_extra, 32)).astype(np.uint8)])
        perm = rng.permutation(len(xy))
        return xy[perm], d[perm]

    def query_pose(self, k):
        return self.poses[k] @ pose(rot([0.02, -0.03, 0.01]), np.array([0.08, -0.05, 0.1]))

    def build(self, ctx, capacity=None):
        from vslam_amd.mapper import LocalMapper
        kw = {"capacity": capacity} if capacity else {}
        m = LocalMapper(K, save_every_keyframe=False, context=ctx, **kw)
        img = np.zeros((H_IMG, W_IMG), np.uint8)
        for k in range(self.n_kf):
            m.add_keyframe(img, kps_array(self.kf_xy[k]), self.kf_desc[k], self.poses[k])
        assert len(m.map_points) == 0
        m.update_map_points([{"id": int(j), "position": self.X[j], "color": np.zeros(3, np.uint8), "observed_keyframes": o}
                             for j, o in zip(self.world, self.obs)])
        return m


_W = {}


def reloc_world():
    if "w" not in _W:
        _W["w"] = RelocWorld()
    return _W["w"]


_VOC = {}


def vocabulary(name, words):
    """(words, weights, iterations) of the restatement, trained once per process on the keyframe descriptors of the named world
    ("pan": tests/covis_worlds.pan_back, "reloc": reloc_world), 10 iterations"""
    from tests import bow_restatement as B
    if (name, words) not in _VOC:
        if name == "pan":
            from tests.covis_worlds import pan_back
            arrays = pan_back().kf_desc
        else:
            arrays = reloc_world().kf_desc
        desc, off = rows_of(arrays)
        _VOC[(name, words)] = B.train(desc, off, words, 10)
    return _VOC[(name, words)]


def rows_of(arrays):
    """(descriptors [n][32], image offsets [n_img + 1]) of a list of per-image descriptor arrays"""
    arrays = [np.asarray(a, np.uint8).reshape(-1, 32) for a in arrays]
    off = np.zeros(len(arrays) + 1, np.int64)
    off[1:] = np.cumsum([len(a) for a in arrays])
    return np.vstack(arrays), off


def tiny_map_frames(n_kf, rows=8, seed=3, n_base=40):
    """n_kf keyframes of `rows` rows drawn (with up to 3 flipped bits) from n_base base descriptors: many keyframes share words, scores
    tie and differ"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n_base, 32)).astype(np.uint8)
    return [flip(rng, base[rng.integers(0, n_base, rows)], 3) for _ in range(n_kf)], base


def _with_bits(bits):
    d = np.zeros(32, np.uint8)
    for b in bits:
        d[b // 8] |= np.uint8(1 << (b % 8))
    return d


def hand_split():
    """(desc [8][32], img_off, W = 2): rows 0 - 3 near the zero descriptor (initial word 0 = row 0), rows 4 - 7 near the all-ones
    descriptor (initial word 1 = row 4).  Among the first four, bit 5 is set in two (a 2 / 2 split: bit 0) and bit 9 in three (3 / 1:
    bit 1); among the last four, bit 200 is clear in two (2 / 2 set: bit 0) and bit 77 clear in one (3 / 1 set: bit 1)."""
    ones = np.full(32, 255, np.uint8)
    a = [_with_bits([]), _with_bits([5, 9]), _with_bits([5, 9]), _with_bits([9])]
    b = [ones ^ _with_bits([]), ones ^ _with_bits([200]), ones ^ _with_bits([200, 77]), ones ^ _with_bits([])]
    return np.array(a + b, np.uint8), np.array([0, 3, 8], np.int64), 2


def hand_duplicates():
    """(desc [6][32], img_off, W = 3): the initial words are rows 0, 2, 4; rows 0 and 2 are equal, so word 1 duplicates word 0 and never
    has a member (ties go to the lower word): it keeps its bits.  Word 0 keeps its bits too (bits 7 and 8 are set in one of its four
    members each); word 2 loses bit 100 (set in one of its two members), so the first iteration changes a word and the second none."""
    ones = np.full(32, 255, np.uint8)
    rows = [_with_bits([3, 4]), _with_bits([3, 4, 7]), _with_bits([3, 4]), _with_bits([3, 4, 8]), ones, ones ^ _with_bits([100])]
    return np.array(rows, np.uint8), np.array([0, 6], np.int64), 3


def hand_equidistant():
    """(descriptor, words [3][32]): the descriptor is 2 bits from word 1 and from word 2 and 4 from word 0: it goes to word 1"""
    return _with_bits([0, 1]), np.array([_with_bits([2, 3]), _with_bits([0, 1, 10, 11]), _with_bits([0, 1, 20, 21])], np.uint8)
