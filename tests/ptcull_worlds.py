"""Constructed maps for the map-point cull by ORB-SLAM2's rule (tests/test_ptcull_cpu.py, tests/test_gpu_ptcull.py): each world is there
for one rule of mo_map_points_bad, and CASES names the switch of tests/ptcull_restatement.decide that it excludes.  Plain numpy; the
device map is built from a world by build(), which imports the library when called.

A world is a script: seven keyframes are stored (ordinals 0 .. 6), and behind keyframe g the points of group g are injected, so that they
are born at g.  All keyframes stand at one pose and hold the same 64 keypoints, each descriptor twice (no growth step finds a match); a
point sits on the ray of its row, so every add_keyframe's own cull keeps it whatever keyframes it names - except the `doomed` ones,
placed off their ray, which the next keyframe's cull removes (the records of the points behind them move up).  In front of keyframe 6
add_observations gives chosen points an entry at position 6; at the end position 6 is removed (remove_keyframes: those entries then
name nothing) or, in the orphan world, keyframes are erased (erase_keyframes).  Six keyframes remain, now = 6, and a point of group g
has age 6 - g.  `notes` are note_tracking calls with an empty local map: they move the counters through matches alone."""
import numpy as np

from tests import kfcull_restatement as KR
from tests import ptcull_restatement as PR
from tests.map_worlds import BASE_K, BASE_SIZE, kps_array

N_STORED, ROWS = 7, 64
POSE = np.eye(4)


def _keyframe():
    rng = np.random.default_rng(77)
    gx, gy = np.meshgrid(np.linspace(60, 580, 8), np.linspace(50, 430, 8))
    xy = np.column_stack([gx.ravel(), gy.ravel()]).astype(np.float32)
    d = np.repeat(rng.integers(0, 256, (ROWS // 2, 32)).astype(np.uint8), 2, axis=0)
    return xy, d


KF_XY, KF_DESC = _keyframe()


def on_ray(row, depth, off=0.0):
    """the f32 position of a point on the ray of keypoint `row` (off: metres sideways, off the ray)"""
    x, y = KF_XY[row].astype(np.float64)
    return np.array([(x - BASE_K[0, 2]) / BASE_K[0, 0] * depth + off, (y - BASE_K[1, 2]) / BASE_K[1, 1] * depth, depth], np.float32)


class PtWorld:
    """groups[g]: the points injected behind keyframe g, each a dict of `obs` ({key: row}), and optionally `late` (an entry at position 6
    by add_observations), `doomed`, `tag`.  notes: [(points, inliers)] applied in order after everything is built.  final: ("remove", [6])
    or ("erase", positions).  After the script: obs_off / obs_kf / obs_kp, xyz, ids, life, now, counts, tags."""

    def __init__(self, groups, notes=(), final=("remove", [6]), kw=None):
        self.groups, self.notes, self.final, self.kw = groups, list(notes), final, dict(kw or {})
        self.K, self.image_size = BASE_K, BASE_SIZE
        pts, life = [], np.zeros((0, 3), np.int32)
        serial = 0
        for g in range(N_STORED):
            if g >= 2:   # add_keyframe's own cull, from the second keyframe on
                keep = np.array([not p.get("doomed") for p in pts], bool)
                pts = [p for p in pts if not p.get("doomed")]
                life = PR.compacted(life, keep)
            if g == N_STORED - 1:
                for p in pts:
                    if p.get("late"):
                        p["entries"].append((N_STORED - 1, p["row"]))
                life = PR.carried(life)   # (add_observations rebuilt the store)
            new = []
            for spec in groups.get(g, []):
                row = serial % ROWS
                p = dict(spec, row=row, id=serial, entries=[(int(k), row) for k in spec["obs"]],
                         xyz=on_ray(row, 4.0 + serial % 7, 3.0 if spec.get("doomed") else 0.0))
                serial += 1
                new.append(p)
            pts += new
            life = PR.appended(life, len(new), g)
        assert not any(p.get("doomed") for p in pts)
        self.now = N_STORED - 1
        off, okf, okp = [0], [], []
        for p in pts:
            okf += [k for k, _ in p["entries"]]; okp += [r for _, r in p["entries"]]
            off.append(len(okf))
        off, okf, okp = np.array(off, np.int32), np.array(okf, np.int32), np.array(okp, np.int32)
        counts = np.full(N_STORED, ROWS, np.int32)
        if final[0] == "remove":
            counts = np.delete(counts, final[1])
        else:
            off, okf, okp, counts = KR.erase(off, okf, okp, counts, final[1])
        self.obs_off, self.obs_kf, self.obs_kp, self.counts = off, okf, okp, counts
        self.xyz = np.array([p["xyz"] for p in pts], np.float32).reshape(-1, 3)
        self.ids = np.array([p["id"] for p in pts], np.int32)
        self.tags = [p.get("tag") for p in pts]
        for point, inlier in self.notes:
            life, _ = PR.note(life, self.xyz, off, okf, okp, counts, BASE_K, POSE, *BASE_SIZE, point, inlier, local_keyframes=[])
        self.life = life

    def tagged(self, tag):
        return [i for i, t in enumerate(self.tags) if t == tag]

    def arrays(self):
        return {"xyz": self.xyz, "id": self.ids, "obs_off": self.obs_off, "obs_kf": self.obs_kf, "obs_kp": self.obs_kp}


def decide(w, **over):
    kw = dict(w.kw)
    kw.update(over)
    return PR.decide(w.life, w.now, w.obs_off, w.obs_kf, w.obs_kp, w.counts, **kw)


def build(ctx, w, capacity=None):
    """the world's script on a device map"""
    from vslam_amd.mapper import LocalMapper
    from tests.map_worlds import remove_keyframes
    kw = {"capacity": capacity} if capacity else {}
    m = LocalMapper(w.K, save_every_keyframe=False, context=ctx, **kw)
    img = np.zeros((BASE_SIZE[1], BASE_SIZE[0]), np.uint8)
    serial = 0
    late = []   # ids of the points that gain an entry at position 6
    for g in range(N_STORED):
        if g == N_STORED - 1 and late:
            ids = m.arrays()["id"]
            idx = np.array([int(np.flatnonzero(ids == s)[0]) for s in late], np.int32)
            m.add_observations(N_STORED - 1, idx, np.array([s % ROWS for s in late], np.int32))
        m.add_keyframe(img, kps_array(KF_XY), KF_DESC, POSE)
        assert m.last["n_new"] == 0
        dicts = []
        for spec in w.groups.get(g, []):
            row = serial % ROWS
            dicts.append({"id": serial, "position": on_ray(row, 4.0 + serial % 7, 3.0 if spec.get("doomed") else 0.0), "color": np.zeros(3, np.uint8),
                          "observed_keyframes": {int(k): row for k in spec["obs"]}})
            if spec.get("late"):
                late.append(serial)
            serial += 1
        m.update_map_points(dicts)
    if w.final[0] == "remove":
        remove_keyframes(m, w.final[1])
        m._kf_serials = [s for q, s in enumerate(m._kf_serials) if q not in w.final[1]]
        m._version += 1; m._cache = None
    else:
        m.erase_keyframes(w.final[1])
    for point, inlier in w.notes:
        m.note_tracking(POSE, {"point": point, "inlier": inlier}, local_keyframes=[])
    assert len(m.keyframes) == len(w.counts) and len(m.map_points) == len(w.ids)
    return m


# ---- the worlds ------------------------------------------------------------------------------------------------------------------------
def _pt(obs, **kw):
    return dict(obs=list(obs), **kw)


def _filler(g, n=20):
    """points of group g >= 2 that no rule touches: three observations"""
    return [_pt((0, 1, g), tag="filler") for _ in range(n)]


def _ratio():
    """age 1, three observations; matched without an inlier three times (visible 4, found 1: 4 found == visible, stays) or four times
    (visible 5: goes); a third set matched as inliers"""
    g = {5: [_pt((3, 4, 5), tag=t) for t in ["at"] * 30 + ["below"] * 30 + ["found"] * 30] + _filler(5)}
    w0 = PtWorld(g)
    at, below, found = w0.tagged("at"), w0.tagged("below"), w0.tagged("found")
    n = len(w0.ids)
    notes = [(np.array(at + below + [n, -1, n + 5], np.int32), np.zeros(len(at + below) + 3, bool))] * 3
    notes += [(np.array(below + found + found, np.int32), np.array([False] * len(below) + [False] * len(found) + [True] * len(found)))]
    return PtWorld(g, notes)


def _ages(extra=None, **kw):
    """ages 0 .. 5 with two and with three observations, a doomed point in front of every group"""
    g = {}
    for grp in range(1, 7):
        two = (0, 1) if grp < 3 else (grp - 2, grp - 1)
        three = (0, 1, -1) if grp < 3 else (0, grp - 2, grp - 1)
        g[grp] = ([_pt(two, doomed=True)] if grp < 6 else []) + [_pt(two, tag="two@%d" % (6 - grp)) for _ in range(15)] + \
                 [_pt(three, tag="three@%d" % (6 - grp)) for _ in range(15)]
    return PtWorld(g, kw=kw)


def _duplicate():
    """age 2, three entries, two of them at position 3 (the key -3 names it once six keyframes remain)"""
    return PtWorld({4: [_pt((3, 4, -3), tag="dup") for _ in range(40)] + _filler(4), 6: _filler(6)})


def _invalid():
    """age 2, two valid entries and one at position 6, which is removed: it names nothing"""
    return PtWorld({4: [_pt((3, 4), late=True, tag="late") for _ in range(40)] + _filler(4), 6: _filler(6)})


def _orphan():
    """ages 4 and 0: two observations, one of them at position 1, which is erased with position 6 (five keyframes remain)"""
    return PtWorld({2: [_pt((0, 1), tag="orphan@4") for _ in range(30)] + _filler(2), 3: [_pt((0, 2, 3), tag="filler") for _ in range(20)],
                    6: [_pt((1, 5), tag="orphan@0") for _ in range(30)] + [_pt((2, 3, 5), tag="filler") for _ in range(20)]}, final=("erase", [1, 6]))


def _protect():
    w = _ages()
    prot = np.zeros(len(w.ids), np.uint8)
    prot[w.tagged("two@2")[::2]] = 1
    prot[w.tagged("three@2")] = 1
    w.kw["protect"] = prot
    return w


def _large():
    """1 500 points and 3 200 entries injected behind the last keyframe: every second point has one entry (an orphan), the others three,
    the first 200 of those a fourth that names nothing and travels with its point"""
    pts = []
    for i in range(1500):
        if i % 2 == 0:
            pts.append(_pt((i // 2 % 6,), tag="orphan"))
        else:
            pts.append(_pt((0, 2, 4) + ((40,) if i < 400 else ()), tag="kept"))
    w = PtWorld({6: pts})
    assert len(w.ids) == 1500 and len(w.obs_kf) == 3200
    return w


# name -> (builder, the switch of PR.decide the world excludes, the tags removed)
CASES = {
    "ratio_boundary": (_ratio, "strict_ratio", ["below"]),
    "age_window": (_ages, "age_window", ["two@2", "two@3"]),
    "min_age": (_ages, "reason_2_needs_age", ["two@2", "two@3"]),
    "duplicate_position": (_duplicate, "once_per_position", ["dup"]),
    "invalid_entry": (_invalid, "skip_invalid", ["late"]),
    "orphan": (_orphan, "orphans", ["orphan@4", "orphan@0"]),
    "protect": (_protect, "honour_protect", None),
    "max_age_off": (lambda: _ages(max_age=-1), "negative_max_age_tests_all", ["two@2", "two@3", "two@4", "two@5"]),
    "large": (_large, "orphans", ["orphan"]),
}
_W = {}


def case(name):
    if name not in _W:
        _W[name] = CASES[name][0]()
    return _W[name]


# ---- the sequence: wrong points on the frustum tests' world -------------------------------------------------------------------------------
N_WRONG, SEQ_KEYFRAMES, SEQ_FRAMES = 50, 4, 2
_SEQ = {}


def sequence():
    """tests/view_worlds.py's world at a few hundred points, each observed by at least three keyframes, plus N_WRONG points "triangulated
    from wrong matches": a place in front of the slab and, in keyframes 0 and 1, an unused keypoint row moved to its projection (so the
    keyframes' own cull keeps it).  Then SEQ_KEYFRAMES keyframes without matches, each behind SEQ_FRAMES tracked frames that show the
    true points only.  Returns the world, the indices of the wrong points and per keyframe (pose, [(pose, keypoints, descriptors)])."""
    if _SEQ:
        return _SEQ
    from tests import view_worlds as VW
    w = VW.ViewWorld(seed=31, n_w=700, n_rand=80)
    keep = [i for i, o in enumerate(w.obs) if len(o) >= 3]
    w.world, w.obs, w.xyz = w.world[keep], [w.obs[i] for i in keep], w.xyz[keep]
    rng = np.random.default_rng(91)
    used = [set(o[k] for o in w.obs if k in o) for k in range(2)]
    free = [[r for r in range(len(w.kf_xy[k])) if r not in used[k]] for k in range(2)]
    wrong = []
    while len(wrong) < N_WRONG:
        X = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(-4.0, -2.0)], np.float32)
        rows, ok = {}, True
        for k in range(2):
            xy, z = VW.project(w.kf_poses[k], X[None])
            d = float(np.linalg.norm(X.astype(np.float64) - VW.centre_of(w.kf_poses[k])))
            o = int(VW.octave_of(np.array([20.0]), np.array([d]))[0])
            ok = ok and z[0] > 0 and 5 < xy[0, 0] < VW.W_IMG - 5 and 5 < xy[0, 1] < VW.H_IMG - 5 and 0 <= o < VW.N_LEVELS
            if ok:
                r = free[k].pop()
                w.kf_xy[k][r] = xy[0]; w.kf_oct[k][r] = o
                rows[k] = r
        if ok:
            wrong.append(len(w.obs))
            w.obs.append(rows); w.world = np.append(w.world, -1); w.xyz = np.vstack([w.xyz, X[None]])
    steps = []
    for j in range(SEQ_KEYFRAMES):
        frames = []
        for f in range(SEQ_FRAMES):
            T = VW.camera("A", 10.0 + 0.4 * j + 0.2 * f, 0.3 - 0.15 * j, -0.1 + 0.05 * f, (0.01, -0.02 + 0.01 * j, 0.01))
            true = copy_world(w, len(w.obs) - N_WRONG)
            kps, desc, _ = true.query(T, faces=1, seed=50 + 2 * j + f)
            frames.append((T, kps, desc))
        steps.append((VW.camera("A", 10.0 + 0.4 * j, 0.3 - 0.15 * j, -0.1, (0.01, -0.02 + 0.01 * j, 0.01)), frames))
    _SEQ.update(w=w, wrong=wrong, steps=steps)
    return _SEQ


def copy_world(w, n):
    """the first n map points of a ViewWorld (what a tracked frame shows)"""
    import copy
    t = copy.copy(w)
    t.world, t.obs, t.xyz = w.world[:n], w.obs[:n], w.xyz[:n]
    return t


def empty_keyframe(j):
    """120 keypoints, every descriptor twice: nothing matches, nothing grows"""
    rng = np.random.default_rng(200 + j)
    xy = np.column_stack([rng.uniform(0, 640, 120), rng.uniform(0, 480, 120)]).astype(np.float32)
    return kps_array(xy, rng.integers(0, 8, 120)), np.repeat(rng.integers(0, 256, (60, 32)).astype(np.uint8), 2, axis=0)
