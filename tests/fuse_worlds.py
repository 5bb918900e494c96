"""Constructed maps for the tests of LocalMapper.fuse_map_points (tests/test_gpu_fuse.py): a MapWorld of tests/map_worlds.py taken apart
and extended.  Plain numpy; build_map of tests/map_worlds.py makes the device map.

FuseWorld copies a MapWorld and lets a test add keypoints to keyframes (by store slot), add map points, split points in two and
withhold observations; finish() rebuilds the arrays build_map and the restatements read.  Observation keys are written as the base
world writes them (positions after the removal for a clean world, before it for a stale one)."""
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
