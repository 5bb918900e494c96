"""Constructed maps for the tests of the device map's read paths (relocalization, tracking, bundle adjustment, add_observations) after
keyframes were removed: the world of tests/test_gpu_relocalize.py (_World) generalised, as arrays.  Plain numpy; the device map is built
from a world by build_map, which imports the library when called.

A world is `n_kf` keyframes along x and `n_w` points, each observed from some of the keyframes (rows shuffled among random extra rows, a
different number of them per keyframe, so keypoint counts differ).  `removed` names keyframe positions that mo_map_remove_keyframes
erases: the surviving keyframes keep their store slots, so position != slot from the first removed one on.

variant "clean": the observation keys are written in the positions AFTER the removal (observations of removed keyframes are dropped):
                 a geometrically exact map behind a non-identity position -> slot table.
variant "stale": the keys are written in the positions BEFORE the removal, as the reference leaves them: a key now names the keyframe
                 that moved into that position (its row may be beyond that keyframe's keypoints) or no keyframe at all; a share of the
                 keys is written negative (counting from the end).  Every such key is input the header documents as skipped.

obs_pattern "skip":        the keyframes a, a + 2, a + 4 of _World, each observation with the point's own descriptor (up to 4 bits
                           flipped).  No growth step may find a model, in the map or in its twin: a point is never observed in two
                           keyframes that are neighbours in the original order or in the surviving order (the later one is dropped).
obs_pattern "consecutive": the keyframes a .. a + c - 1, c = 1 .. 6 (tests/ba_scene.py gives the reason: bundle adjustment needs one
                           connected map); every observation has a random descriptor and every descriptor stands at least twice in its
                           keyframe, so the ratio test of a growth step keeps no match.

codebook=True draws the points' descriptors from a 256-bit Hadamard code (any two 128 bits apart) in place of random ones, for frames
in which no keypoint may come within max_dist of another point's descriptor by chance.

Ties of the representative descriptor (ComputeDistinctiveDescriptors: smallest median distance, the earlier observation keeps a tie):
points with exactly three observations get descriptors at equal pairwise distance 12 (all medians 12); points with exactly four get
D0, D1, D0, D1 (duplicated: all medians 0).  `ties` lists them with the descriptor the rule picks and the one a later-wins rule would."""
import numpy as np

from tests import ba_restatement as BA
from tests import track_restatement as TR
from tests.ba_scene import pose, rot
from tests.map_restatement import cull_arrays

BASE_K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])
BASE_SIZE = (640, 480)


def scaled_K(image_size):
    """the 640 x 480 camera of the other map tests scaled to image_size: the same field of view"""
    w, h = image_size
    return np.array([[500.0 * w / 640.0, 0, w / 2.0], [0, 500.0 * h / 480.0, h / 2.0], [0, 0, 1.0]])


def project(K, T, X):
    x = (K @ (T[:3, :3] @ np.asarray(X, np.float64).T + T[:3, 3:4])).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return x[:, :2] / x[:, 2:3], x[:, 2]


def flip(rng, d, max_bits):
    """copies of the descriptors d [n][32] with at most max_bits bits flipped each"""
    d = np.array(d, np.uint8).reshape(-1, 32).copy()
    n = len(d)
    bits = rng.integers(0, 256, (n, max(max_bits, 1)))
    use = np.arange(max(max_bits, 1))[None, :] < rng.integers(0, max_bits + 1, n)[:, None]
    r, c = np.nonzero(use)
    np.bitwise_xor.at(d, (r, bits[r, c] // 8), (1 << (bits[r, c] % 8)).astype(np.uint8))
    return d


def with_bits(d, bits):
    d = np.array(d, np.uint8).copy()
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def kps_array(xy, octave=None):
    import vslam_amd as V
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    k = np.zeros(len(xy), V.KP_DTYPE)
    k["x"] = xy[:, 0]; k["y"] = xy[:, 1]; k["size"] = 31.0
    if octave is not None:
        k["octave"] = octave
    return k


class MapWorld:
    """by original keyframe index (= store slot): slot_xy, slot_oct, slot_desc, slot_poses.  By position after the removal: survivors
    (original indices), kf_xy, kf_oct, kf_desc, kf_poses, counts.  The map points in injection order: world (world point of each), xyz
    f32, ids, obs (dicts {key: row} as injected), obs_off / obs_kf / obs_kp.  ref_oct per world point (None without octaves)."""

    def __init__(self, image_size=BASE_SIZE, K=None, octaves=None, removed=(), variant="clean", obs_pattern="skip", n_w=2000, n_kf=10,
                 n_rand=150, n_points=None, negative_share=0.2, seed=21, codebook=False):
        assert variant in ("clean", "stale") and obs_pattern in ("skip", "consecutive")
        rng = np.random.default_rng(seed)
        self.image_size, self.variant, self.obs_pattern = tuple(image_size), variant, obs_pattern
        self.K = scaled_K(image_size) if K is None else np.asarray(K, np.float64)
        W, H = self.image_size
        self.removed = tuple(sorted(int(r) for r in removed))
        self.n_kf0 = n_kf
        self.survivors = [k for k in range(n_kf) if k not in self.removed]
        new_pos = {k: p for p, k in enumerate(self.survivors)}
        n_new = len(self.survivors)
        X = np.column_stack([rng.uniform(-3.0, 5.5, n_w), rng.uniform(-2.0, 2.0, n_w), rng.uniform(3.0, 12.0, n_w)]).astype(np.float32)
        base = rng.integers(0, 256, (n_w, 32)).astype(np.uint8)
        self.code = None
        if codebook:
            # the 512 rows of a 256-bit Hadamard code and their complements under one random mask: any two are 128 or 256 bits apart, so
            # after the flips below (4 per observation, 8 per frame keypoint) no frame keypoint is within 100 of another point's descriptor
            assert n_w <= 448
            i = np.arange(256)
            par = np.array([[bin(a & b).count("1") & 1 for b in i] for a in i], np.uint8)
            self.code = np.packbits(np.vstack([par, 1 - par]), axis=1) ^ rng.integers(0, 256, (1, 32)).astype(np.uint8)
            base = self.code[:n_w].copy()
        start = rng.integers(0, n_kf, n_w)
        length = rng.integers(1, 7, n_w)
        self.ref_oct = rng.integers(0, 8, n_w) if octaves is not None else None
        self.slot_poses = [pose(rot([0.0, rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02)]), np.array([0.35 * k, 0.05 * np.sin(k), 0.0]))
                           for k in range(n_kf)]
        m = max(2, min(W, H) // 100)   # visibility margin (5 px at 640 x 480)
        vis = np.zeros((n_kf, n_w), bool)
        xy_all = []
        for k, T in enumerate(self.slot_poses):
            xy, z = project(self.K, T, X)
            xy_all.append(xy)
            vis[k] = (z > 0) & (xy[:, 0] > m) & (xy[:, 0] < W - m) & (xy[:, 1] > m) & (xy[:, 1] < H - m)

        def neighbours(a, b):
            return abs(a - b) == 1 or (a in new_pos and b in new_pos and abs(new_pos[a] - new_pos[b]) == 1)
        seen = [[] for _ in range(n_w)]   # original keyframe indices observing each world point, ascending
        for j in range(n_w):
            a = int(start[j])
            cand = (a, a + 2, a + 4) if obs_pattern == "skip" else range(a, a + int(length[j]))
            for k in cand:
                if k >= n_kf or not vis[k, j]:
                    continue
                if obs_pattern == "skip" and any(neighbours(k, p) for p in seen[j]):
                    continue
                seen[j].append(k)
        # descriptor of every observation; the tie constructions on points all of whose observations survive the removal
        odesc = {}
        self.ties = []   # (world point, descriptor the rule picks, descriptor a later-wins rule picks)
        for j in range(n_w):
            s = seen[j]
            if not s:
                continue
            d = flip(rng, np.repeat(base[j:j + 1], len(s), 0), 4) if obs_pattern == "skip" else rng.integers(0, 256, (len(s), 32)).astype(np.uint8)
            whole = all(k in new_pos for k in s)
            if whole and len(s) == 3 and j % 2 == 0:
                b = rng.permutation(256)[:18]
                d[0] = base[j]; d[1] = with_bits(base[j], b[:12]); d[2] = with_bits(base[j], b[6:])
                self.ties.append((j, d[0].copy(), d[2].copy()))
            elif whole and len(s) == 4 and j % 2 == 0:
                d[0] = base[j]; d[1] = with_bits(base[j], rng.permutation(256)[:40]); d[2] = d[0]; d[3] = d[1]
                self.ties.append((j, d[0].copy(), d[3].copy()))
            for k, dk in zip(s, d):
                odesc[(j, k)] = dk
        self.base, self.X_world = base, X
        # the keyframes: observed rows shuffled among random rows
        self.slot_xy, self.slot_oct, self.slot_desc = [], [], []
        row_of = {}
        for k in range(n_kf):
            pts = np.array([j for j in range(n_w) if k in seen[j]], np.int64)
            nr = n_rand + 37 * ((k * 5) % 7)
            if obs_pattern == "consecutive":
                nr = max(nr, len(pts) + 2)
            n = len(pts) + nr
            perm = rng.permutation(n)
            kxy = np.zeros((n, 2), np.float32)
            d = np.zeros((n, 32), np.uint8)
            octv = rng.integers(0, 8, n).astype(np.int32) if octaves is not None else np.zeros(n, np.int32)
            rows = perm[:len(pts)]
            kxy[rows] = xy_all[k][pts]
            if len(pts):
                d[rows] = np.stack([odesc[(int(j), k)] for j in pts])
            if octaves is not None:
                octv[rows] = np.clip(self.ref_oct[pts] + rng.integers(-1, 2, len(pts)), 0, None)
            kxy[perm[len(pts):]] = np.column_stack([rng.uniform(0, W, nr), rng.uniform(0, H, nr)])
            d[perm[len(pts):]] = rng.integers(0, 256, (nr, 32))
            if obs_pattern == "consecutive":
                # every descriptor of the keyframe at least twice: the best two neighbours of any query are at the same distance, the
                # ratio test keeps nothing and no growth step has a match to start from (random descriptors alone let a few through)
                extra = perm[len(pts):]
                d[extra[:len(pts)]] = d[rows]
                rest = extra[len(pts):]
                d[rest[1::2]] = d[rest[0:2 * len(rest[1::2]):2]]
                if len(rest) % 2:
                    d[rest[-1]] = d[rest[-2]]
            for j, r in zip(pts.tolist(), rows.tolist()):
                row_of[(j, k)] = r
            self.slot_xy.append(kxy); self.slot_oct.append(octv); self.slot_desc.append(d)
        self.kf_xy = [self.slot_xy[k] for k in self.survivors]
        self.kf_oct = [self.slot_oct[k] for k in self.survivors]
        self.kf_desc = [self.slot_desc[k] for k in self.survivors]
        self.kf_poses = [self.slot_poses[k] for k in self.survivors]
        self.counts = np.array([len(x) for x in self.kf_xy], np.int32)
        # the map points and their keys
        self.world, self.obs = [], []
        for j in range(n_w):
            if variant == "clean":
                o = {new_pos[k]: row_of[(j, k)] for k in seen[j] if k in new_pos}
            else:
                o = {}
                for k in seen[j]:
                    key, r = k, row_of[(j, k)]
                    if rng.random() < negative_share and k < n_new:
                        key = k - n_new                      # names position k from the end
                    elif rng.random() < negative_share and k < n_new and r < self.counts[k]:
                        r = r - int(self.counts[k])          # names row r of the keyframe now at position k from the end
                    o[key] = r
            if o:
                self.world.append(j); self.obs.append(o)
        if n_points is not None:
            assert len(self.world) >= n_points, (len(self.world), n_points)
            self.world, self.obs = self.world[:n_points], self.obs[:n_points]
        self.world = np.array(self.world, np.int64)
        self.xyz = X[self.world]
        self.ids = self.world.astype(np.int32)
        off, okf, okp = [0], [], []
        for o in self.obs:
            okf += list(o.keys()); okp += list(o.values())
            off.append(len(okf))
        self.obs_off, self.obs_kf, self.obs_kp = np.array(off, np.int32), np.array(okf, np.int32), np.array(okp, np.int32)
        self.index_of = {int(j): i for i, j in enumerate(self.world)}   # world point -> map point

    # -- what a kernel that skipped the position -> slot table would read: position p names slot p ------------------------------------
    def slot_order(self):
        n = len(self.survivors)
        return self.slot_xy[:n], self.slot_oct[:n], self.slot_desc[:n], self.slot_poses[:n]

    def key_kinds(self):
        """how many observation keys are of each kind (stale worlds): out-of-range position / row, negative position / row"""
        n = len(self.survivors)
        kinds = {"position_out_of_range": 0, "row_out_of_range": 0, "negative_position": 0, "negative_row": 0, "valid": 0}
        for k, r in zip(self.obs_kf.tolist(), self.obs_kp.tolist()):
            kinds["negative_position"] += k < 0
            kinds["negative_row"] += r < 0
            p = k + n if k < 0 else k
            if not 0 <= p < n:
                kinds["position_out_of_range"] += 1
                continue
            q = r + int(self.counts[p]) if r < 0 else r
            if not 0 <= q < self.counts[p]:
                kinds["row_out_of_range"] += 1
                continue
            kinds["valid"] += 1
        return kinds

    # -- query frames -----------------------------------------------------------------------------------------------------------------
    def reloc_query(self, pos, T, noise=0.0, seed=5, pairs=None):
        """_World.query: the points with a key naming position `pos` seen from T (their keyframe descriptors with up to 10 bits flipped),
        20 % moved to wrong places, 15 % random extra keypoints"""
        rng = np.random.default_rng(seed)
        W, H = self.image_size
        if pairs is None:
            pts = np.array([i for i, o in enumerate(self.obs) if pos in o], np.int64)
            rows = np.array([self.obs[i][pos] for i in pts], np.int64)
        else:   # (map points, rows of the keyframe at `pos`) given by the caller: a stale world's valid observations
            pts, rows = (np.asarray(a, np.int64) for a in pairs)
        xy, z = project(self.K, T, self.xyz[pts])
        vis = (z > 0) & (xy[:, 0] > 0) & (xy[:, 0] < W) & (xy[:, 1] > 0) & (xy[:, 1] < H)
        pts, xy, rows = pts[vis], xy[vis], rows[vis]
        d = flip(rng, self.kf_desc[pos][rows], 10)
        xy = xy + rng.normal(0, noise, xy.shape) if noise else xy
        wrong = rng.random(len(xy)) < 0.2
        xy[wrong] = np.column_stack([rng.uniform(0, W, wrong.sum()), rng.uniform(0, H, wrong.sum())])
        n_extra = int(0.15 * len(xy))
        xy = np.vstack([xy, np.column_stack([rng.uniform(0, W, n_extra), rng.uniform(0, H, n_extra)])]).astype(np.float32)
        d = np.vstack([d, rng.integers(0, 256, (n_extra, 32)).astype(np.uint8)])
        perm = rng.permutation(len(xy))
        return kps_array(xy[perm]), d[perm]

    def track_query(self, T, noise=0.0, seed=5, wrong=0.1, extra=0.3, octave_spread=0, flips=8, point_desc=None):
        """_query of tests/test_gpu_track_map.py: every map point visible from T as a keypoint at its projection with its descriptor (up
        to `flips` more bits flipped), a share `wrong` moved by 5 - 12 px, `extra` random keypoints on top.  With octaves each keypoint
        carries its point's reference octave + d, d uniform in -octave_spread .. octave_spread (never below 0); random keypoints 0 .. 9.
        point_desc [map point][32]: the descriptors to start from in place of the world points' own (a stale world's representatives)."""
        rng = np.random.default_rng(seed)
        W, H = self.image_size
        xy, z = project(self.K, T, self.xyz)
        vis = np.flatnonzero((z > 0) & (xy[:, 0] > 0) & (xy[:, 0] < W) & (xy[:, 1] > 0) & (xy[:, 1] < H))
        d = flip(rng, self.base[self.world[vis]] if point_desc is None else np.asarray(point_desc)[vis], flips)
        xy = xy[vis] + (rng.normal(0, noise, (len(vis), 2)) if noise else 0.0)
        bad = rng.random(len(vis)) < wrong
        ang = rng.uniform(0, 2 * np.pi, bad.sum())
        xy[bad] += rng.uniform(5, 12, bad.sum())[:, None] * np.column_stack([np.cos(ang), np.sin(ang)])
        n_extra = int(extra * len(vis))
        xy = np.vstack([xy, np.column_stack([rng.uniform(0, W, n_extra), rng.uniform(0, H, n_extra)])]).astype(np.float32)
        if self.code is None:
            d = np.vstack([d, rng.integers(0, 256, (n_extra, 32)).astype(np.uint8)])
        else:   # the unused code words: as far from every point's descriptor as the points are from each other
            spare = self.code[len(self.base):]
            d = np.vstack([d, flip(rng, spare[np.arange(n_extra) % len(spare)], flips)])
        octv = np.zeros(len(xy), np.int32)
        if self.ref_oct is not None:
            octv[:len(vis)] = np.clip(self.ref_oct[self.world[vis]] + rng.integers(-octave_spread, octave_spread + 1, len(vis)), 0, None)
            octv[len(vis):] = rng.integers(0, 10, n_extra)
        perm = rng.permutation(len(xy))
        return kps_array(xy[perm], octv[perm]), d[perm]

    def arrays(self):
        return {"xyz": self.xyz, "obs_off": self.obs_off, "obs_kf": self.obs_kf, "obs_kp": self.obs_kp}

    def point_dicts(self, xyz=None):
        xyz = self.xyz if xyz is None else xyz
        return [{"id": int(self.ids[i]), "position": xyz[i], "color": np.zeros(3, np.uint8), "observed_keyframes": self.obs[i]}
                for i in range(len(self.obs))]


def remove_keyframes(m, positions):
    """_cull_keyframes' outcome for the given positions, with the mapper's own host bookkeeping (as
    test_cull_kernel_on_a_large_synthetic_map does it): the device table, the keyframe list, the list rows, the ids renumbered"""
    import ctypes as C
    pos = sorted((int(p) for p in positions), reverse=True)
    if not pos:
        return
    m._check(m.lib.mo_map_remove_keyframes(m._h, np.array(pos, np.int32).ctypes.data_as(C.c_void_p), len(pos)))
    for i in pos:
        m.keyframes.pop(i); m._list_rows.pop(i)
    for i, kf in enumerate(m.keyframes):
        kf["id"] = i


def build_map(ctx, w, twin=False, poses=None, xyz=None, capacity=None):
    """the world as a device map.  twin: the map that never had the removed keyframes (identity slots), the same points and keys.
    poses: the surviving keyframes' poses by position in place of the world's (the store's P and kf["pose"]); xyz: the injected
    positions in place of the exact ones."""
    from vslam_amd.mapper import LocalMapper
    kw = {"capacity": capacity} if capacity else {}
    m = LocalMapper(w.K, save_every_keyframe=False, context=ctx, **kw)
    img = np.zeros((w.image_size[1], w.image_size[0]), np.uint8)

    new_pos = {k: p for p, k in enumerate(w.survivors)}

    def add(k):
        T = w.slot_poses[k] if poses is None or k not in new_pos else np.asarray(poses[new_pos[k]], np.float64)
        m.add_keyframe(img, kps_array(w.slot_xy[k], w.slot_oct[k]), w.slot_desc[k], T)
        assert m.last["n_new"] == 0 and len(m.map_points) == 0   # no growth step found a model

    def inject():
        m.update_map_points(w.point_dicts(xyz))
    if twin:
        for k in w.survivors:
            add(k)
        inject()
    elif w.variant == "clean":
        for k in range(w.n_kf0):
            add(k)
        remove_keyframes(m, w.removed)
        inject()
    else:
        for k in range(w.n_kf0):
            add(k)
        inject()
        remove_keyframes(m, w.removed)
    assert len(m.keyframes) == len(w.survivors) and len(m.map_points) == len(w.obs)
    assert [kf["id"] for kf in m.keyframes] == list(range(len(w.survivors)))
    return m


def perturbed(w, seed=3, angle=np.deg2rad(1.0), shift=0.03, depth=0.02, first_free=2):
    """Scene.perturbed of tests/ba_scene.py on a world: (poses by position with those from first_free on turned and moved, xyz f32 moved
    along the distance to the origin)"""
    rng = np.random.default_rng(seed)
    poses = [T.copy() for T in w.kf_poses]
    for k in range(first_free, len(poses)):
        d, c = rng.normal(size=3), rng.normal(size=3)
        P = np.eye(4)
        P[:3, :3] = rot(angle * d / np.linalg.norm(d)); P[:3, 3] = shift * c / np.linalg.norm(c)
        poses[k] = P @ poses[k]
    X = w.xyz.astype(np.float64)
    X = X + rng.normal(0, depth / np.sqrt(3.0), X.shape) * np.linalg.norm(X, axis=1, keepdims=True)
    return poses, X.astype(np.float32)


# ---- the worlds and cases shared by tests/test_map_worlds_cpu.py and tests/test_gpu_map_reads.py ----------------------------------------
REMOVED = (1, 4)
BA_REMOVED, BA_WINDOW, BA_FIRST_FREE = (1, 5), 6, 4
# Steps per round of the bundle adjustments compared with the device.  The constructed scene is noise-free: after five steps the cost
# sits at the floor the f32 rounding of the keypoints leaves (4e-8), and whether one more step lowers it is decided in the tenth digit
# of two sums that device and restatement add in different orders.  (3, 2) stops while every step still lowers the cost by percents;
# decisions_are_clear asserts that, so that steps / accepted are integers both sides must agree on.
BA_STEPS = (3, 2)
STALE_BA_STEPS = (5, 0)   # on the stale world: three rejected steps, one accepted, one rejected, each by 20 % of the cost or more
_W = {}


def world(name):
    """the worlds shared with tests/test_gpu_map_reads.py, built once"""
    if name not in _W:
        _W[name] = {"clean": lambda: MapWorld(removed=REMOVED),
                    "stale": lambda: MapWorld(removed=REMOVED, variant="stale"),
                    "octave": lambda: MapWorld(removed=REMOVED, octaves=True, seed=22, n_w=448, codebook=True),
                    "ba": lambda: MapWorld(removed=BA_REMOVED, obs_pattern="consecutive", octaves=True, n_w=1500, n_kf=12, n_rand=100, seed=23),
                    "ba_stale": lambda: MapWorld(removed=BA_REMOVED, obs_pattern="consecutive", variant="stale", octaves=True, n_w=1500,
                                                 n_kf=12, n_rand=100, seed=23)}[name]()
    return _W[name]


# relocalization with preselection on the clean world: the vocabulary size, the keyframes preselected, the queries (the positions of
# test_relocalize_after_removal, with its pose offsets)
PRE_WORDS, PRE_N, PRE_QUERIES = 256, 3, (3, 6, 0)
_VOC = {}


def clean_vocabulary():
    """(words, weights, iterations) of tests/bow_restatement.train on the clean world's keyframes by position, PRE_WORDS words and 10
    iterations, trained once per process"""
    from tests import bow_restatement as B
    from tests.bow_worlds import rows_of
    if "clean" not in _VOC:
        _VOC["clean"] = B.train(*rows_of(world("clean").kf_desc), PRE_WORDS, 10)
    return _VOC["clean"]


def clean_reloc_query(pos):
    """(keypoints, descriptors, pose) of the relocalization query near position pos of the clean world"""
    w = world("clean")
    T = pose_near(w, pos, (0.02, -0.03, 0.01), (0.08, -0.05, 0.1))
    return w.reloc_query(pos, T) + (T,)


def pose_near(w, pos, d_rot=(0.01, -0.02, 0.01), d_c=(0.1, -0.05, 0.05)):
    return w.kf_poses[pos] @ pose(rot(list(d_rot)), np.array(d_c))


def perturbed_pose(T):
    """about 2 degrees and 5 cm off (tests/test_gpu_track_map.py's _perturbed)"""
    return pose(rot([0.005, 0.005, 0.033]), np.array([0.03, -0.03, 0.025])) @ T


def track(w, kps, desc, pose0, lists=None, **kw):
    _, oct_, desc_, _ = lists if lists is not None else (None, w.kf_oct, w.kf_desc, None)
    W, H = w.image_size
    return TR.track(w.K, pose0, w.xyz, w.obs_off, w.obs_kf, w.obs_kp, desc_, oct_, kps, desc, W, H, **kw)


def ba_problem_edges(w, lists=None, window=BA_WINDOW):
    """(free, fixed, [(point, position, x, y)] over the local points' edges)"""
    xy = w.kf_xy if lists is None else lists[0]
    counts = [len(a) for a in xy]
    local, free, fixed, edges = BA.problem(w.obs_off, w.obs_kf, w.obs_kp, counts, window)
    return free, fixed, [(i, k, float(xy[k][r][0]), float(xy[k][r][1])) for i in np.flatnonzero(local) for k, r, _ in edges[i]]


def ba_restated(w, poses, xyz, **kw):
    kw.setdefault("max_steps", BA_STEPS)
    return BA.bundle_adjust(w.obs_off, w.obs_kf, w.obs_kp, w.counts, w.kf_xy, w.kf_oct, xyz, w.K, np.array([T[:3, :4] for T in poses]),
                            window=BA_WINDOW, **kw)


def decisions_are_clear(trace):
    """every accept / reject decision of a restated run changes the cost by more than 1e-6 of it, and no update is near the 1e-10 that
    ends a round: a device whose sums round differently (1e-10 relative on these costs) takes the same decisions"""
    assert trace
    for rnd, cur, trial, upd in trace:
        assert abs(trial - cur) > 1e-6 * cur and upd > 1e-8, (rnd, cur, trial, upd)


def stale_queries(w):
    """a tracking and a relocalization frame for a stale world, built from what its valid observations name"""
    counts = [len(d) for d in w.kf_desc]
    obs = TR.valid_observations(w.obs_off, w.obs_kf, w.obs_kp, counts)
    local = TR.local_points(obs, len(counts), 10)
    rep, _ = TR.representatives(obs, w.kf_desc, w.kf_oct, local)
    T = pose_near(w, 4)
    tk = w.track_query(T, point_desc=rep, octave_spread=0)
    pos = 3
    pairs = [(i, r) for i, v in enumerate(obs) for k, r in v if k == pos]
    rq = w.reloc_query(pos, w.kf_poses[pos], pairs=(np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])))
    return T, tk, pos, rq


_BA = {}


def ba_case():
    """the consecutive world with the free keyframes' poses and the points perturbed, and its restated bundle adjustment"""
    if not _BA:
        w = world("ba")
        poses, xyz = perturbed(w, first_free=BA_FIRST_FREE)
        trace = []
        _BA.update(w=w, poses=poses, xyz=xyz, ref=ba_restated(w, poses, xyz, trace=trace), trace=trace)
    return _BA


def cull_after_ba(w, poses, ref, where="slot"):
    """the map-point cull of the keyframe added after the bundle adjustment, in numpy: keep mask and the points within 1e-9 px of the
    threshold.  where: "none" the store's P as before the call, "slot" the refined P of the free keyframes at their slots, "position"
    at kP[position] (what a write-back without the table would do)"""
    n0 = w.n_kf0
    P_slot = [None] * n0
    for p, s in enumerate(w.survivors):
        P_slot[s] = w.K @ np.asarray(poses[p], np.float64)[:3, :4]
    for s in range(n0):
        if P_slot[s] is None:
            P_slot[s] = w.K @ w.slot_poses[s][:3, :4]
    if where != "none":
        for p in ref["free"]:
            P_slot[w.survivors[p] if where == "slot" else p] = w.K @ ref["poses"][p]
    P_pos = [P_slot[s] for s in w.survivors] + [w.K @ w.kf_poses[-1][:3, :4]]   # (the keyframe being added: no observation names it)
    xy_pos = w.kf_xy + [w.kf_xy[-1]]
    return cull_arrays(P_pos, xy_pos, ref["xyz"], w.obs_off, w.obs_kf, w.obs_kp)
