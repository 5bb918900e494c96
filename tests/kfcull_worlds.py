"""Constructed maps for the keyframe cull by ORB-SLAM2's rule (tests/test_kfcull_cpu.py, tests/test_gpu_kfcull.py): each world is there
for one rule of mo_map_kf_redundancy, and CASES names the variant of tests/kfcull_restatement.decide that it excludes.  Plain numpy;
a world goes onto the device through tests.map_worlds.build_map, whose attributes it carries.

The common shape (_ring): keyframe T holds only points that its neighbours see too; every neighbour also holds `private` points that only
it and the asking keyframe see, so that a neighbour is never redundant itself; the asking keyframe sees every point, which makes all of
them candidates.  Descriptors stand twice in their keyframe (no growth step finds a match), geometry plays no part in the decision."""
import numpy as np

from tests import kfcull_restatement as KR
from tests.ba_scene import pose, rot
from tests.map_worlds import BASE_K, BASE_SIZE, world


class KfWorld:
    """n_kf keyframes by position; `removed`: original indices (store slots) of dummy keyframes that mo_map_remove_keyframes erases before
    the points are injected (variant "clean" of tests/map_worlds.py), so that position != slot behind the first of them"""

    def __init__(self, n_kf, removed=(), seed=1, min_rows=100):
        self.rng = np.random.default_rng(seed)
        self.K, self.image_size, self.variant = BASE_K.copy(), BASE_SIZE, "clean"
        self.removed = tuple(sorted(removed))
        self.n_kf0 = n_kf + len(self.removed)
        self.survivors = [k for k in range(self.n_kf0) if k not in self.removed]
        self.min_rows = min_rows
        self.oct = [[] for _ in range(n_kf)]   # by position: octave of every row handed out so far
        self.obs = []

    def row(self, k, octave=0):
        self.oct[k].append(int(octave))
        return len(self.oct[k]) - 1

    def point(self, entries):
        """entries: [(key, row)] as injected, in entry order (a dict: a key may not repeat, the same position may - as k and k - n_kf)"""
        d = dict(entries)
        assert len(d) == len(entries)
        self.obs.append(d)
        return len(self.obs) - 1

    def see(self, views):
        """a point seen from [(position, octave)]: a new row in each"""
        return self.point([(k, self.row(k, o)) for k, o in views])

    def finish(self, negative_share=0.0):
        rng, n_kf = self.rng, len(self.oct)
        for k in range(n_kf):   # rows no point names, up to min_rows
            while len(self.oct[k]) < self.min_rows:
                self.oct[k].append(int(rng.integers(0, 8)))
        self.kf_oct = [np.array(o, np.int32) for o in self.oct]
        self.counts = np.array([len(o) for o in self.kf_oct], np.int32)
        if negative_share:   # some keys and rows written from the end
            for d in self.obs:
                items = []
                for k, r in d.items():
                    if 0 <= k < n_kf and 0 <= r < self.counts[k]:
                        if rng.random() < negative_share and (k - n_kf) not in d:
                            k -= n_kf
                        elif rng.random() < negative_share:
                            r -= int(self.counts[k + n_kf if k < 0 else k])
                    items.append((k, r))
                d.clear(); d.update(items)
        self.slot_oct, self.slot_xy, self.slot_desc, self.slot_poses = [], [], [], []
        W, H = self.image_size
        at = {s: p for p, s in enumerate(self.survivors)}
        for s in range(self.n_kf0):
            octv = self.kf_oct[at[s]] if s in at else np.zeros(self.min_rows + 7 * s, np.int32)   # (a dummy: octave 0 in every row)
            n = len(octv)
            d = rng.integers(0, 256, ((n + 1) // 2, 32)).astype(np.uint8)
            self.slot_oct.append(octv)
            self.slot_xy.append(np.column_stack([rng.uniform(0, W, n), rng.uniform(0, H, n)]).astype(np.float32))
            self.slot_desc.append(np.repeat(d, 2, axis=0)[:n] if n > 1 else d[:n])
            self.slot_poses.append(pose(rot([0.0, 0.0, 0.0]), np.array([0.1 * s, 0.0, 0.0])))
        self.kf_xy = [self.slot_xy[s] for s in self.survivors]
        self.kf_desc = [self.slot_desc[s] for s in self.survivors]
        self.kf_poses = [self.slot_poses[s] for s in self.survivors]
        n = len(self.obs)
        self.xyz = np.column_stack([rng.uniform(-3, 5, n), rng.uniform(-2, 2, n), rng.uniform(3, 12, n)]).astype(np.float32).reshape(n, 3)
        self.ids = np.arange(n, dtype=np.int32)
        off, okf, okp = [0], [], []
        for o in self.obs:
            okf += list(o.keys()); okp += list(o.values())
            off.append(len(okf))
        self.obs_off, self.obs_kf, self.obs_kp = np.array(off, np.int32), np.array(okf, np.int32), np.array(okp, np.int32)
        return self

    def point_dicts(self, xyz=None):
        xyz = self.xyz if xyz is None else xyz
        return [{"id": int(self.ids[i]), "position": xyz[i], "color": np.zeros(3, np.uint8), "observed_keyframes": self.obs[i]}
                for i in range(len(self.obs))]


def decide(w, **kw):
    return KR.decide(w.obs_off, w.obs_kf, w.obs_kp, w.counts, w.kf_oct, **kw)


def _ring(w, T, neighbours, ask, n_shared, private=60, t_oct=1, n_oct=1, per_point=None):
    """n_shared points at T (octave t_oct), each seen by the asking keyframe and by `per_point` of the neighbours in turn (None: all of
    them) at octave n_oct; `private` points per neighbour that only it and the asking keyframe see"""
    for j in range(n_shared):
        nb = neighbours if per_point is None else [neighbours[(j + x) % len(neighbours)] for x in range(per_point)]
        w.see([(T, t_oct)] + [(k, n_oct) for k in nb] + [(ask, n_oct)])
    for k in neighbours:
        for _ in range(private):
            w.see([(k, n_oct), (ask, n_oct)])


def plain(removed=(), n_oct=1, seed=1):
    """T = 2 is seen whole from 1, 3 and 4 (and from the asking keyframe 5)"""
    w = KfWorld(6, removed=removed, seed=seed)
    _ring(w, 2, [1, 3, 4], 5, 40, n_oct=n_oct)
    return w.finish()


def mutual():
    """2 and 3 hold the same 30 points, seen besides from 1 and the asking keyframe 5: each has three other observers only while the
    other is there.  Equal weights: 3 comes first in the order and goes, 2 stays."""
    w = KfWorld(6, seed=2)
    for _ in range(30):
        w.see([(2, 0), (3, 0), (1, 0), (5, 0)])
    for _ in range(60):
        w.see([(1, 0), (5, 0)])
    return w.finish()


def threshold(n_red):
    """T = 2 holds 20 points, n_red of them with three other observers besides the asking keyframe"""
    w = KfWorld(6, seed=3)
    _ring(w, 2, [1, 3, 4], 5, n_red)
    for _ in range(20 - n_red):
        w.see([(2, 1), (5, 1)])
    return w.finish()


def first_position():
    """the keyframe seen whole from its neighbours is position 0"""
    w = KfWorld(6, seed=4)
    _ring(w, 0, [1, 3, 4], 5, 40)
    return w.finish()


def duplicate():
    """T = 2's points are seen from 3 and 5 at its own octave and twice from 1: first at octave 5, then (key 1 - n_kf) at octave 1.  With
    the first observation 1 fails the scale test and two observers remain; with the later one there are three."""
    w = KfWorld(6, seed=5)
    for _ in range(40):
        w.point([(2, w.row(2, 1)), (1, w.row(1, 5)), (1 - 6, w.row(1, 1)), (3, w.row(3, 1)), (5, w.row(5, 1))])
    for k in (1, 3):
        for _ in range(60):
            w.see([(k, 1), (5, 1)])
    return w.finish()


def negative_keys():
    """the plain world with three keys in ten, and three rows in ten of the rest, written from the end"""
    w = KfWorld(6, seed=12)
    _ring(w, 2, [1, 3, 4], 5, 40)
    return w.finish(negative_share=0.3)


def nothing_named():
    """T = 2's points are seen from 1 and 5; a key beyond the keyframes, one before the first and a row beyond keyframe 3's rows name
    nothing.  A reader that took any of them for an observer would count three."""
    w = KfWorld(6, seed=6)
    for j in range(40):
        w.point([(2, w.row(2, 1)), (1, w.row(1, 1)), (6 + j % 3, 0), (-7 - j % 2, 1), (3, 5000 + j), (4, -5000 - j), (5, w.row(5, 1))])
    for _ in range(60):
        w.see([(1, 1), (5, 1)])
    return w.finish()


def negative_octaves():
    """T = 2's keypoints carry octave -3 (read as 0), its observers octave 1: within the gap of 1.  Read as -3 they would not be."""
    w = KfWorld(6, seed=7)
    _ring(w, 2, [1, 3, 4], 5, 40, t_oct=-3, n_oct=1)
    return w.finish()


def tall():
    """T = 5 holds 1100 points (rows beyond 1024), each seen by three of ten neighbours in turn; the asking keyframe 11 sees them all"""
    w = KfWorld(12, seed=8)
    _ring(w, 5, [0, 1, 2, 3, 4, 6, 7, 8, 9, 10], 11, 1100, private=45, per_point=3)
    return w.finish()


def many():
    """130 keyframes of 8 rows; 700 points, each at the asking keyframe 129 and at 2 to 5 others (rows are shared among points): every
    keyframe is a candidate at min_weight = 1, more than a wavefront of them, with ties throughout"""
    w = KfWorld(130, seed=9, min_rows=8)
    rng = w.rng
    for k in range(130):
        for _ in range(8):
            w.row(k, rng.integers(0, 3))
    for j in range(700):
        ks = rng.choice(129, int(rng.integers(2, 6)), replace=False)
        if j < 129:
            ks[0] = j if j not in ks[1:] else ks[0]
        w.point([(int(k), int(rng.integers(0, 8))) for k in dict.fromkeys(ks.tolist())] + [(129, int(rng.integers(0, 8)))])
    return w.finish()


def no_points():
    return KfWorld(4, seed=10).finish()


def one_keyframe():
    w = KfWorld(1, seed=11)
    for _ in range(20):
        w.see([(0, 0)])
    return w.finish()


MANY_KW = dict(min_weight=1, ratio=0.5)
# name -> (builder, decide keywords, the switch of KR.decide under which the world decides differently or None, what the world removes)
CASES = {
    "plain": (plain, {}, None, [2]),
    "scale": (lambda: plain(n_oct=3), {}, "scale_test", []),
    "scale_gap_2": (lambda: plain(n_oct=3), dict(scale_gap=2), None, [2]),
    "mutual": (mutual, {}, "one_pass", [3]),
    "mutual_ties": (mutual, {}, "ties_earlier", [3]),
    "threshold_15": (lambda: threshold(15), dict(ratio=0.75), None, []),
    "threshold_16": (lambda: threshold(16), dict(ratio=0.75), None, [2]),
    "position_0": (first_position, {}, None, []),
    "protect": (plain, dict(protect=[0, 0, 1, 0, 0, 0]), None, []),
    "ask_middle": (plain, dict(kf_pos=3), None, [2]),
    "duplicate": (duplicate, {}, "later_duplicate", []),
    "negative_keys": (negative_keys, {}, None, [2]),
    "nothing_named": (nothing_named, {}, None, []),
    "negative_octaves": (negative_octaves, {}, None, [2]),
    "earlier_removals": (lambda: plain(removed=(1, 4), n_oct=3), {}, None, []),
    "tall": (tall, {}, None, [5]),
    "many": (many, MANY_KW, "one_pass", None),
    "no_points": (no_points, {}, None, []),
    "one_keyframe": (one_keyframe, {}, None, []),
}
SWITCH = {"scale_test": dict(scale_test=False), "one_pass": dict(one_pass=True), "later_duplicate": dict(later_duplicate=True),
          "ties_earlier": dict(ties_earlier=True)}


_BUILT = {}


def case(name):
    """(world, decide keywords) of a constructed case, built once"""
    if name not in _BUILT:
        _BUILT[name] = CASES[name][0]()
    return _BUILT[name], dict(CASES[name][1])


EXISTING = ("ba", "ba_stale", "clean", "octave")   # tests.map_worlds.world(name), asked from the last keyframe at min_weight 15
# the issue's table for them: candidates, weights, n_points, n_redundant, n_redundant without the scale test (None: not given)
EXISTING_NUMBERS = {
    "ba": ([8, 7, 6, 5], [231, 133, 81, 42], [346, 307, 345, 347], [118, 154, 178, 172], [138, 175, 213, 211]),
    "ba_stale": ([8, 7, 6, 5, 4], [228, 138, 80, 39, 18], [345, 306, 343, 351, 384], [80, 92, 118, 126, 136], [134, 163, 216, 231, 245]),
    "clean": ([5, 3], [316, 157], [510, 201], [0, 0], None),
    "octave": ([5, 3], [71, 33], [111, 39], [0, 0], None),
}


def any_world(name):
    """(world, decide keywords) of a constructed case or an existing world"""
    return (world(name), {}) if name in EXISTING else case(name)


ALL = tuple(CASES) + EXISTING
