"""Constructed maps for the tests of LocalMapper.fuse_map_points (tests/test_gpu_fuse.py): a MapWorld of tests/map_worlds.py taken apart
and extended.  Plain numpy; build_map of tests/map_worlds.py makes the device map.

FuseWorld copies a MapWorld and lets a test add keypoints to keyframes (by store slot), add map points, split points in two and
withhold observations; finish() rebuilds the arrays build_map and the restatements read.  Observation keys are written as the base
world writes them (positions after the removal for a clean world, before it for a stale one).
large_split_world: the split world at the mapper's keyframe size (about 2000 rows); row_cases: hand maps of up to 2049 rows at the
row edges of the search (csrc/map_fuse.hip, k_trk_grid)."""
import numpy as np

from tests import fuse_restatement as FR
from tests.map_worlds import MapWorld, kps_array, project  # noqa: F401  (kps_array: re-exported for the tests)


class FuseWorld:
    def __init__(self, base):
        self.world0 = base
        for f in ("K", "image_size", "removed", "survivors", "n_kf0", "variant", "slot_poses", "code", "ref_oct"):
            setattr(self, f, getattr(base, f))
        self.slot_xy = [a.copy() for a in base.slot_xy]
        self.slot_oct = [a.copy() for a in base.slot_oct]
        self.slot_desc = [a.copy() for a in base.slot_desc]
        self.obs = [dict(o) for o in base.obs]
        self.xyz = [x.copy() for x in base.xyz]
        self.ids = [int(i) for i in base.ids]
        self.origin = list(range(len(self.obs)))   # the base world's map point each point came from (-1: added)
        self.finish()

    def add_keypoint(self, slot, xy, desc, octave=0):
        self.slot_xy[slot] = np.vstack([self.slot_xy[slot], np.asarray(xy, np.float32).reshape(1, 2)])
        self.slot_oct[slot] = np.append(self.slot_oct[slot], np.int32(octave))
        self.slot_desc[slot] = np.vstack([self.slot_desc[slot], np.asarray(desc, np.uint8).reshape(1, 32)])
        return len(self.slot_xy[slot]) - 1

    def projection(self, slot, X):
        xy, z = project(self.K, self.slot_poses[slot], np.asarray(X, np.float32).astype(np.float64).reshape(1, 3))
        W, H = self.image_size
        assert z[0] > 0 and 5 < xy[0, 0] < W - 5 and 5 < xy[0, 1] < H - 5, (slot, xy, z)
        return xy[0]

    def add_point(self, X, obs, pid=None):
        self.obs.append(dict(obs)); self.xyz.append(np.asarray(X, np.float32)); self.origin.append(-1)
        self.ids.append(max(self.ids, default=0) + 1 if pid is None else int(pid))
        return len(self.obs) - 1

    def split(self, first=1):
        """every point with >= 2 observations becomes two next to each other: its first `first` observations / the rest, same position
        and id.  Returns the number of splits"""
        obs, xyz, ids, origin, n = [], [], [], [], 0
        for o, x, i, g in zip(self.obs, self.xyz, self.ids, self.origin):
            items = list(o.items())
            parts = [items] if len(items) < 2 else [items[:first], items[first:]]
            n += len(parts) - 1
            for p in parts:
                obs.append(dict(p)); xyz.append(x); ids.append(i); origin.append(g)
        self.obs, self.xyz, self.ids, self.origin = obs, xyz, ids, origin
        return n

    def withhold(self, pick):
        """drops the observations pick(point index, [(key, row)]) names from the map; their keypoints stay.  Returns them as
        [(point, key, row)]"""
        out = []
        for i, o in enumerate(self.obs):
            for k in pick(i, list(o.items())):
                out.append((i, k, o.pop(k)))
        return out

    def finish(self):
        self.kf_xy = [self.slot_xy[k] for k in self.survivors]
        self.kf_oct = [self.slot_oct[k] for k in self.survivors]
        self.kf_desc = [self.slot_desc[k] for k in self.survivors]
        self.kf_poses = [self.slot_poses[k] for k in self.survivors]
        self.counts = np.array([len(x) for x in self.kf_xy], np.int32)
        a = FR.as_arrays(np.array(self.xyz, np.float32).reshape(-1, 3), [list(o.items()) for o in self.obs], ids=self.ids)
        self.obs_off, self.obs_kf, self.obs_kp = a["obs_off"], a["obs_kf"], a["obs_kp"]
        self.xyz_arr = a["xyz"]
        return self

    def slot_order(self):
        n = len(self.survivors)
        return self.slot_xy[:n], self.slot_oct[:n], self.slot_desc[:n], self.slot_poses[:n]

    def point_dicts(self, xyz=None):
        xyz = np.array(self.xyz, np.float32) if xyz is None else xyz
        return [{"id": int(self.ids[i]), "position": xyz[i], "color": np.zeros(3, np.uint8), "observed_keyframes": self.obs[i]}
                for i in range(len(self.obs))]


def map_inputs(m):
    """what the restatement reads of a device map: (arrays copied, P per position as the mapper stored it, xy, octave, descriptors)"""
    from orbslam2.utils import compute_projection_matrix
    m._cache = None
    a = {f: v.copy() for f, v in m.arrays().items()}
    P = [np.ascontiguousarray(compute_projection_matrix(kf["pose"][:3, :3], kf["pose"][:3, 3], m.camera_matrix), np.float64) for kf in m.keyframes]
    kps = [np.asarray(kf["keypoints"]) for kf in m.keyframes]
    return (a, P, [np.column_stack([k["x"], k["y"]]).astype(np.float32).reshape(-1, 2) for k in kps], [k["octave"].astype(np.int32) for k in kps],
            [np.asarray(kf["descriptors"], np.uint8).reshape(-1, 32) for kf in m.keyframes])


def restate(m, size, lists=None, **kw):
    """FR.fuse of the device map as it stands.  lists = (xy, octave, descriptors, P) per position in place of the map's own (what a
    reader without the position -> slot table would see)"""
    a, P, xy, octv, desc = map_inputs(m)
    if lists is not None:
        xy, octv, desc, P = lists
    return FR.fuse(a, P, xy, octv, desc, size[0], size[1], **kw)


def skip_world(n_w=500, n_kf=10, removed=(), variant="clean", seed=41, **kw):
    return MapWorld(removed=removed, variant=variant, obs_pattern="skip", n_w=n_w, n_kf=n_kf, n_rand=60, seed=seed, **kw)


def split_world(**kw):
    """(world with every multi-view point in two, the unsplit world, number of splits)"""
    base = skip_world(**kw)
    w = FuseWorld(base)
    n = w.split()
    return w.finish(), FuseWorld(base), n


def withheld_world(**kw):
    """the last observation of every point with three is withheld; for five such points p, two more points are added at p's place, each
    observing one of p's keypoints: all three claim p's free keypoint.  Returns (world, withheld [(point, key, row)])"""
    base = skip_world(**kw)
    w = FuseWorld(base)
    held = w.withhold(lambda i, items: [items[-1][0]] if len(items) == 3 else [])
    assert len(held) >= 20
    for p, _, _ in held[:5]:   # clones observing one of p's keypoints each: they claim p's free keypoint too, and merge into p
        for k, r in list(w.obs[p].items()):
            w.add_point(w.xyz[p], {k: r}, pid=w.ids[p])
    return w.finish(), held


def obs_sets(a, counts):
    from tests.track_restatement import valid_observations
    return [frozenset(v) for v in valid_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], counts)]


def world_inputs(w):
    """map_inputs of the map build_map makes of a world, without a device (the seeds are chosen with this)"""
    from orbslam2.utils import compute_projection_matrix
    a = FR.as_arrays(w.xyz_arr, [list(o.items()) for o in w.obs], ids=w.ids)
    P = [np.ascontiguousarray(compute_projection_matrix(T[:3, :3], T[:3, 3], w.K), np.float64) for T in w.kf_poses]
    return a, P, w.kf_xy, w.kf_oct, w.kf_desc


def restate_world(w, lists=None, **kw):
    a, P, xy, octv, desc = world_inputs(w)
    if lists is not None:
        xy, octv, desc, P = lists
    return FR.fuse(a, P, xy, octv, desc, w.image_size[0], w.image_size[1], **kw)


def decorate(w, seed=9, share=0.2):
    """stale and negative keys on a geometrically exact world: per point, with probability `share` each, one key rewritten as counted
    from the end, one row rewritten as counted from the end, a key naming no keyframe added (row 3), a key of a keyframe the point is
    not observed in added with a row beyond that keyframe's keypoints.  Every valid observation still names the same keypoint."""
    rng = np.random.default_rng(seed)
    n_kf = len(w.survivors)
    for i, o in enumerate(w.obs):
        items = list(o.items())
        if items and rng.random() < share:
            j = int(rng.integers(len(items)))
            items[j] = (items[j][0] - n_kf, items[j][1])
        if items and rng.random() < share:
            j = int(rng.integers(len(items)))
            k = items[j][0] + n_kf if items[j][0] < 0 else items[j][0]
            items[j] = (items[j][0], items[j][1] - int(w.counts[k]))
        if rng.random() < share:
            items.insert(int(rng.integers(len(items) + 1)), (50 + i % 7, 3))
        if rng.random() < share:
            used = {k + n_kf if k < 0 else k for k, _ in items}
            free = [k for k in range(n_kf) if k not in used]
            if free:
                k = free[int(rng.integers(len(free)))]
                items.insert(int(rng.integers(len(items) + 1)), (k, int(w.counts[k]) + 2))
        w.obs[i] = dict(items)
    return w.finish()


def hand_map(ctx, K, poses, kfs, xyz, obs, size=(100, 100), capacity=None):
    """a device map of a hand-written scene: kfs per keyframe [(x, y, descriptor[, octave])], obs per point [(key, row)] as stored"""
    from vslam_amd.mapper import LocalMapper
    kw = {"capacity": capacity} if capacity else {}
    m = LocalMapper(K, save_every_keyframe=False, context=ctx, **kw)
    img = np.zeros((size[1], size[0]), np.uint8)
    for kf, T in zip(kfs, poses):
        kp = kps_array([[p[0], p[1]] for p in kf], [p[3] if len(p) > 3 else 0 for p in kf])
        m.add_keyframe(img, kp, np.array([p[2] for p in kf], np.uint8).reshape(-1, 32), T)
        assert m.last["n_new"] == 0 and len(m.map_points) == 0
    m.update_map_points([{"id": 100 + i, "position": np.asarray(x, np.float32), "color": np.zeros(3, np.uint8), "observed_keyframes": dict(o)}
                         for i, (x, o) in enumerate(zip(xyz, obs))])
    return m


# ---- worlds at the keyframe size the mapper runs at -------------------------------------------------------------------------------------
LARGE = dict(n_w=4000, n_kf=4)
LARGE_STALE = dict(n_w=3400, n_kf=6, removed=(1,), seed=43)
_LARGE = {}


def large_split_world(stale=False):
    """split_world at about 2000 rows per keyframe, built once: (world, unsplit, splits).  Checked on the CPU (tests/test_fuse_cpu.py):
    LARGE:       rows [921, 1117, 1924, 1830], 1693 splits, all absorbed again, margins["min"] 1.3e-7
    LARGE_STALE: position 1 of six removed: rows [548, 693, 1087, 1785, 1656], slot != position from position 1 on, keys decorated;
                 1928 splits, margins["min"] 1.1e-5
    In both no pair of consecutive keyframes (in slot order, as build_map adds them) has a descriptor match that survives the ratio
    test at 0.8.  At least two targets exceed 1024 rows: k_trk_grid's strided loops take a second trip, keypoints in rows >= 1024 are
    matched, and the tables strided by the store's row capacity are read past row 1024 of more than one target."""
    if stale not in _LARGE:
        w, unsplit, n = split_world(**(LARGE_STALE if stale else LARGE))
        if stale:
            decorate(w)
        assert (w.counts > 1024).sum() >= 2 and 4 <= len(w.counts) <= 6 and w.counts.max() <= 2100, w.counts
        _LARGE[stale] = (w, unsplit, n)
    return _LARGE[stale]


# ---- hand maps at the row edges of the search ---------------------------------------------------------------------------------------------
# The camera of tests/test_fuse_cpu.py: keyframe k looks down z from x = 0.1 k, the point (0, 0, 10) lands at (50 - k, 50).  The grid of
# k_trk_grid has 64 x 48 cells over the 100 x 100 image: 1.5625 x 2.0833 px each.
TILE = 1024          # the block of k_trk_grid: its strided loops take a second trip from this row on
Y_FILL = 90.0        # the image row of the fillers: 40 px from every projection (the search radius is 3 px)


def padded(n, rows):
    """a keyframe of n rows: `rows` = {row: (x, y, descriptor)}, every other row a filler at (5.25 + row % 91, Y_FILL): no |dx| is within 0.25 px of
    the search radius, so the restatement's margins stay clear.  Fillers carry the
    Walsh pattern 3, except one for each descriptor of `rows` that stands once: it carries a copy.  Every descriptor then stands at
    least twice in the keyframe, the ratio test of add_keyframe's own growth step keeps nothing and hand_map's n_new == 0 holds"""
    from tests.test_fuse_cpu import _desc
    once = {}
    for p in rows.values():
        once.setdefault(bytes(p[2]), []).append(p[2])
    copies = [v[0] for v in once.values() if len(v) == 1]
    n_fill = n - len(rows)
    assert n_fill >= len(copies) and n_fill - len(copies) != 1 and all(0 <= r < n for r in rows), (n, len(rows), len(copies))
    return [tuple(rows[r]) if r in rows else (5.25 + r % 91, Y_FILL, copies.pop() if copies else _desc(3)) for r in range(n)]


def grid_cell(x, y, w=100, h=100):
    """trk_cx / trk_cy of csrc/map_search.h for coordinates inside the image"""
    return int(x * 64 / w), int(y * 48 / h)


def row_cases():
    """hand maps that put the search of csrc/map_fuse.hip at its row edges: name -> (kfs, xyz, obs, expectations): `lists` = every
    observation list after the call, `into`, and counts (a subset of FR.COUNTS).  tests/test_fuse_cpu.py shows for every case a wrong
    reading of the rows it fails under."""
    from tests.test_fuse_cpu import _desc
    D0 = _desc(0)
    c = {}
    # target_row_past_1024: targets of 1025 and 2049 rows (the store's row stride is at least 2049: stride != count for both), the
    # keypoint of the point (0, 0, 10) in the last row of each.  A observes (0, 0), B - at the same place - observes (2, 2048).
    # Pairs: A x {1, 2}, B x {0, 1}: 4, all in the image, all with a keypoint at distance 0: 4 proposals.  (1, 1024) is free and claimed
    # by both at distance 0: the lower point, A, gains it.  (2, 2048) is B's and won by A, (0, 0) is A's and won by B: 2 edges, one
    # component, one observation each: A survives, with its own entry, then B's, then the gained one
    kfs = [[(50, 50, D0)], padded(TILE + 1, {TILE: (49, 50, D0)}), padded(2 * TILE + 1, {2 * TILE: (48, 50, D0)})]
    c["target_row_past_1024"] = (kfs, [[0, 0, 10]] * 2, [[(0, 0)], [(2, 2 * TILE)]],
                                 dict(lists=[[(0, 0), (2, 2 * TILE), (1, TILE)]], into=[0, 0], n_targets=3, n_local=2, n_pairs=4, n_cand=4, n_proposals=4,
                                      n_gained=1, n_edges=2, n_absorbed=1, n_points=1, n_obs=3))
    # crowded_cell: A observes (0, 0) and (1, 0) and projects to (48, 50) in a target of 1500 rows, cell (30, 24) = [46.875, 48.4375) x
    # [50, 52.083).  200 of its keypoints, rows 3 + 7 j, stand in that cell at (47 + (j % 20) / 16, 50 + (j // 20) / 8): at most 1 px
    # left, 1.125 px below: inside r = 3 and chi2 (at most 2.27 <= 5.991), every one a candidate keypoint.  196 are 10 bits off; those
    # of j = 160, 170 (rows 1123, 1193) and j = 180, 190 (rows 1263, 1333) are 4 bits off, two and two with other bits: the lowest row,
    # 1123.  One pair, one candidate, one proposal, the free row gained
    crowd = {}
    for j in range(200):
        d = _desc(0, range(4)) if j in (160, 170) else _desc(0, range(100, 104)) if j in (180, 190) else _desc(0, range(10))
        crowd[3 + 7 * j] = (47 + (j % 20) / 16.0, 50 + (j // 20) / 8.0, d)
    assert len(crowd) >= 200 and {grid_cell(p[0], p[1]) for p in crowd.values()} == {grid_cell(48, 50)} and sum(r >= TILE for r in crowd) >= 50
    kfs = [[(50, 50, D0)], padded(2, {0: (49, 50, D0)}), padded(1500, crowd)]
    c["crowded_cell"] = (kfs, [[0, 0, 10]], [[(0, 0), (1, 0)]],
                         dict(lists=[[(0, 0), (1, 0), (2, 1123)]], into=[0], n_targets=3, n_local=1, n_pairs=1, n_cand=1, n_proposals=1, n_gained=1,
                              n_edges=0, n_absorbed=0, n_points=1, n_obs=3))
    # empty_target: position 1 has no row.  A observes (0, 0): pairs with positions 1 and 2, both projections in the image (a candidate
    # is a projection, whatever keypoints there are): 2 and 2.  Position 2 has rows 0 and 1 at the projection and half a pixel off, both at
    # distance 0: row 0 is gained; position 1 proposes nothing
    kfs = [[(50, 50, D0)], [], [(48, 50, D0), (48.5, 50, D0)]]
    c["empty_target"] = (kfs, [[0, 0, 10]], [[(0, 0)]],
                         dict(lists=[[(0, 0), (2, 0)]], into=[0], n_targets=3, n_local=1, n_pairs=2, n_cand=2, n_proposals=1, n_gained=1, n_edges=0,
                              n_absorbed=0, n_points=1, n_obs=2))
    assert all(len(kf) <= 2 * TILE + 1 for v in c.values() for kf in v[0]) and all(len(v[0]) <= 3 for v in c.values())
    return c


MUTATIONS = ("targets_cut", "ties_high")   # a kernel that stopped after a target's first 1024 rows / that took ties upward


def run_rows(kfs, xyz, obs, mutation=None, **kw):
    """FR.fuse of a row case (window 0): (arrays after, into, counts, margins).  mutation "targets_cut": every keyframe cut to its first
    TILE rows (an observation of a row behind the cut names no row and is skipped, as any stale key); "ties_high": the wrong tie rule"""
    from tests.test_fuse_cpu import K, _poses
    assert mutation in (None,) + MUTATIONS
    if mutation == "targets_cut":
        kfs = [kf[:TILE] for kf in kfs]
    elif mutation == "ties_high":
        kw["ties"] = -1
    kf_xy = [np.array([[p[0], p[1]] for p in kf], np.float32).reshape(-1, 2) for kf in kfs]
    kf_desc = [np.array([p[2] for p in kf], np.uint8).reshape(-1, 32) for kf in kfs]
    kf_oct = [np.zeros(len(kf), np.int32) for kf in kfs]
    a = FR.as_arrays(xyz, obs, ids=np.arange(len(obs)) + 100)
    return FR.fuse(a, FR.store_P(K, _poses()), kf_xy, kf_oct, kf_desc, 100, 100, window=0, **kw)


def missed(want, a, into, cnt):
    """the expectations of a row case that a result does not meet: [] when it holds"""
    bad = [k for k in want if k in FR.COUNTS and cnt[k] != want[k]]
    if FR.lists_of(a) != want["lists"]:
        bad.append("lists")
    if np.asarray(into).tolist() != want["into"]:
        bad.append("into")
    return bad
