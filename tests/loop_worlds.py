"""Worlds for the loop-candidate tests (mo_map_loop_candidates), in numpy alone so that the CPU tests can pin on them what the GPU tests run.

LoopWorld: tests/covis_worlds.PanBackWorld - 20 keyframes that turn from region A over a strip to region B - and then a return to A.
Return keyframes at the even positions 20, 22, 24, 26 (yaw 34, 20, 9, 1 degrees); each observes a random half of the A and strip points
it sees, every observation a NEW map point: a duplicate of the old one with the same code word (up to 4 flipped bits per observation),
shared among the return keyframes that drew it; plus 60 random rows.  The odd positions 21 .. 27 are filler keyframes of 150 random rows,
so no two consecutive keyframes share a descriptor and the growth step of add_keyframe finds no model (the "skip" pattern).  The ids tell
the pairs: an old point carries its world point j as id, its duplicate DUP_ID + j.  The pan-back world's dozen second observations
through negative keys are left out: the keys would name other keyframes once the map has 28.

steps(): the same world while it is built keyframe by keyframe, as a mapper sees it.  The old points are injected behind keyframe 19;
a duplicate is injected behind the LAST return keyframe that drew it (an observation cannot name a keyframe that is not stored yet);
every add_keyframe culls the points with fewer than two observations.

tiny_world(n_kf): tests/bow_worlds.tiny_map_frames (8 rows per keyframe, few words) with random points on top: scores, common-word
counts, W entries and acc values tie, and the tie rules decide.  Hand cases at the end."""
import numpy as np

from tests import bow_restatement as B
from tests import bow_worlds as BW
from tests.covis_worlds import _camera, pan_back
from tests.map_worlds import flip, project

RETURN_POS = (20, 22, 24, 26)
RETURN_YAW = (34.0, 20.0, 9.0, 1.0)
FILLER_POS = (21, 23, 25, 27)
N_KF = 28
DUP_ID = 10000
WORDS = 1024


class LoopWorld:
    def __init__(self, seed=7, n_rand=60, n_filler=150):
        rng = np.random.default_rng(seed)
        w = pan_back()
        self.K, self.image_size = w.K, w.image_size
        Wd, Hd = self.image_size
        self.kf_xy, self.kf_desc, self.kf_poses = list(w.kf_xy), list(w.kf_desc), list(w.kf_poses)
        old_j = np.flatnonzero(w.region != 2)
        dup_obs = {}   # world point -> {position: row} of its duplicate
        for r, (pos, yaw) in enumerate(zip(RETURN_POS, RETURN_YAW)):
            T = _camera(yaw, [0.03 * r, 0.01, 0.0])
            xy, z = project(self.K, T, w.X_world[old_j])
            vis = old_j[(z > 0) & (xy[:, 0] > 5) & (xy[:, 0] < Wd - 5) & (xy[:, 1] > 5) & (xy[:, 1] < Hd - 5)]
            drawn = np.sort(rng.choice(vis, len(vis) // 2, replace=False))
            n = len(drawn) + n_rand
            perm = rng.permutation(n)
            kxy, dsc = np.zeros((n, 2), np.float32), np.zeros((n, 32), np.uint8)
            rows = perm[:len(drawn)]
            kxy[rows] = project(self.K, T, w.X_world[drawn])[0]
            dsc[rows] = flip(rng, w.base[drawn], 4)
            kxy[perm[len(drawn):]] = np.column_stack([rng.uniform(0, Wd, n_rand), rng.uniform(0, Hd, n_rand)])
            dsc[perm[len(drawn):]] = rng.integers(0, 256, (n_rand, 32))
            for j, row in zip(drawn.tolist(), rows.tolist()):
                dup_obs.setdefault(j, {})[pos] = row
            self.kf_xy.append(kxy); self.kf_desc.append(dsc); self.kf_poses.append(T)
            # the filler behind it
            self.kf_xy.append(np.column_stack([rng.uniform(0, Wd, n_filler), rng.uniform(0, Hd, n_filler)]).astype(np.float32))
            self.kf_desc.append(rng.integers(0, 256, (n_filler, 32)).astype(np.uint8))
            self.kf_poses.append(_camera(120.0 + 10.0 * r))
        self.counts = np.array([len(d) for d in self.kf_desc], np.int32)
        # the points in injection order: the old ones, then the duplicates by (last observer, world point)
        self.points = [{"id": int(j), "position": w.X_world[j], "color": np.zeros(3, np.uint8),
                        "observed_keyframes": {k: r for k, r in o.items() if k >= 0}} for j, o in zip(w.world.tolist(), w.obs)]
        self.n_old = len(self.points)
        for j in sorted(dup_obs, key=lambda j: (max(dup_obs[j]), j)):
            self.points.append({"id": DUP_ID + j, "position": w.X_world[j], "color": np.zeros(3, np.uint8), "observed_keyframes": dup_obs[j]})
        self.obs_off, self.obs_kf, self.obs_kp = obs_arrays(self.points)
        self.ids = np.array([q["id"] for q in self.points], np.int64)

    def steps(self):
        """[(keyframe positions to add, points to inject behind them, the position that then asks)] of the build keyframe by keyframe"""
        out = [(list(range(20)), self.points[:self.n_old], 19)]
        for pos in RETURN_POS:
            inj = [q for q in self.points[self.n_old:] if max(q["observed_keyframes"]) == pos]
            out.append(([pos - 1, pos] if pos > 20 else [pos], inj, pos))
        return out

    def build(self, ctx, capacity=(32, 512, 4096, 16384)):
        """the whole world as a device map: every keyframe, then every point (no cull runs on them)"""
        m = new_mapper(ctx, self.K, capacity)
        for k in range(N_KF):
            add_keyframe(m, self, k)
        m.update_map_points(self.points)
        return m


def obs_arrays(points):
    off, okf, okp = [0], [], []
    for q in points:
        okf += list(q["observed_keyframes"].keys()); okp += list(q["observed_keyframes"].values())
        off.append(len(okf))
    return np.array(off, np.int32), np.array(okf, np.int32), np.array(okp, np.int32)


def cull(points):
    """the points add_keyframe's cull keeps on these worlds: two observations or more (every stored observation reprojects exactly)"""
    return [q for q in points if len(q["observed_keyframes"]) >= 2]


def new_mapper(ctx, K, capacity, vocabulary=None):
    """vocabulary: attached before the first keyframe (the tests attach theirs behind the last one otherwise)"""
    from vslam_amd.mapper import LocalMapper
    m = LocalMapper(K, save_every_keyframe=False, context=ctx, n_hyp=8, capacity=capacity)
    if vocabulary is not None:
        m.set_vocabulary(vocabulary)
    return m


def add_keyframe(m, w, k):
    from tests.map_worlds import kps_array
    img = np.zeros((w.image_size[1], w.image_size[0]), np.uint8)
    m.add_keyframe(img, kps_array(w.kf_xy[k]), w.kf_desc[k], w.kf_poses[k])
    assert m.last["n_new"] == 0   # no growth step found a model


_W = {}


def loop_world():
    if "loop" not in _W:
        _W["loop"] = LoopWorld()
    return _W["loop"]


def loop_vocabulary():
    """(words, weights) of the restatement trained on the loop world's own rows, 1024 words, 10 iterations"""
    if "voc" not in _W:
        words, weights, _ = B.train(*BW.rows_of(loop_world().kf_desc), WORDS, 10)
        _W["voc"] = (words, weights)
    return _W["voc"]


# ---- tiny maps ------------------------------------------------------------------------------------------------------------------------
TINY_MIN_WEIGHT = 2


class TinyWorld:
    """n_kf keyframes of 8 rows; 3 n_kf points, each observed from 2 - 5 keyframes near an anchor (and one in eight also far away), at
    random rows: several points share a row (point_of takes the lowest), W is a band of small numbers with many equal entries"""

    def __init__(self, n_kf, words, seed=5):
        rng = np.random.default_rng(seed + n_kf)
        self.n_kf = n_kf
        self.kf_desc, self.base = BW.tiny_map_frames(n_kf)
        self.K, self.image_size = BW.K, (32, 32)
        self.kf_xy = [np.random.default_rng(k).uniform(0, 32, (len(d), 2)).astype(np.float32) for k, d in enumerate(self.kf_desc)]
        self.kf_poses = [np.eye(4) for _ in range(n_kf)]
        self.words, weights, _ = B.train(*BW.rows_of(self.kf_desc[:64]), words, 10)
        self.weights = np.where(np.arange(words) % 5 == 0, 0, np.maximum(weights, 1)).astype(np.int32)   # every fifth word counts nothing
        self.points = []
        for i in range(3 * n_kf):
            a = int(rng.integers(0, n_kf))
            ks = {a}
            for _ in range(int(rng.integers(1, 5))):
                ks.add(int(np.clip(a + rng.integers(-6, 7), 0, n_kf - 1)))
            if i % 8 == 0:
                ks.add(int((a + n_kf // 2 + rng.integers(0, 3)) % n_kf))
            self.points.append({"id": i, "position": rng.uniform(-1, 1, 3).astype(np.float32), "color": np.zeros(3, np.uint8),
                                "observed_keyframes": {k: int(rng.integers(0, 8)) for k in sorted(ks)}})
        self.obs_off, self.obs_kf, self.obs_kp = obs_arrays(self.points)

    def asking(self):
        """the asking positions the tests run: the last, the first, and a few in between"""
        n = self.n_kf
        return sorted({n - 1, 0, n // 2, n // 3, (2 * n) // 3 + 1})

    def build(self, ctx):
        m = new_mapper(ctx, self.K, (self.n_kf + 75, 16, 4 * self.n_kf, 32 * self.n_kf))
        for k in range(self.n_kf):
            from tests.map_worlds import kps_array
            m.add_keyframe(np.zeros((32, 32), np.uint8), kps_array(self.kf_xy[k]), self.kf_desc[k], self.kf_poses[k])
        m.update_map_points(self.points)
        return m


TINY = {70: 16, 129: 32, 1025: 64}   # keyframes -> words: one block, past k_covis' LDS path, one more than a 1024-thread tile


def tiny_world(n_kf):
    if ("tiny", n_kf) not in _W:
        _W[("tiny", n_kf)] = TinyWorld(n_kf, TINY[n_kf])
    return _W[("tiny", n_kf)]


FEATURE_WORDS = 8


def feature_world():
    """4 keyframes of 8 rows and 12 points: the smallest tiny world, for the tests that only need every map feature to have run"""
    if "features" not in _W:
        _W["features"] = TinyWorld(4, FEATURE_WORDS)
    return _W["features"]


def feature_steps(m, w, vocabulary):
    """[(name, fn)]: one call of each of the eight map features on the built feature_world, covisibility first; keyframe 0 is the query
    frame.  Place recognition is the attached vocabulary and a query; the loop candidates need it and come behind it.  Every call gets
    past its argument checks and runs its chain on the device, whatever it finds on a map of random points."""
    from tests.map_worlds import kps_array
    kps, desc = kps_array(w.kf_xy[0]), w.kf_desc[0]

    def place():
        m.set_vocabulary(vocabulary)
        return m.query_keyframes(kps, desc, 3)
    return [("covisibility", m.covisibility),
            ("relocalize", lambda: m.relocalize(kps, desc, n_hyp=8)),
            ("track", lambda: m.track_local_map(kps, desc, np.eye(4), window=0, min_matches=1)),
            ("bundle_adjust", lambda: m.bundle_adjust(window=4)),
            ("fuse", lambda: m.fuse_map_points(image_size=w.image_size, window=0)),
            ("grow", lambda: m.create_new_map_points(window=0)),
            ("place", place),
            ("loop", lambda: m.loop_candidates(3, TINY_MIN_WEIGHT, 2, 2))]


# ---- hand cases -----------------------------------------------------------------------------------------------------------------------
def _word_desc(w, n_words=8):
    """a descriptor 0 bits from word w of hand_words()"""
    return hand_words(n_words)[w].copy()


def hand_words(n_words=8):
    """n_words words 32 bits apart from each other: word w has bits 32 w .. 32 w + 31 set"""
    d = np.zeros((n_words, 32), np.uint8)
    for w in range(n_words):
        d[w, 4 * w:4 * w + 4] = 255
    return d


def near(desc, bits):
    """desc with the given bits (of the last 32 bits: no word of hand_words(7) uses them) flipped"""
    d = np.array(desc, np.uint8).copy()
    for b in bits:
        d[28 + b // 8] ^= np.uint8(1 << (b % 8))
    return d


class HandWorld:
    """keyframes given as lists of (word, flipped bits) rows over hand_words(7), points as {position: row} dicts"""

    def __init__(self, frames, points, weights=None):
        self.words = hand_words(7)
        self.weights = np.full(7, 1024, np.int32) if weights is None else np.asarray(weights, np.int32)
        self.kf_desc = [np.array([near(self.words[w], bits) for w, bits in f], np.uint8).reshape(-1, 32) for f in frames]
        self.n_kf = len(frames)
        self.K, self.image_size = BW.K, (32, 32)
        self.kf_xy = [np.random.default_rng(k).uniform(0, 32, (len(d), 2)).astype(np.float32) for k, d in enumerate(self.kf_desc)]
        self.kf_poses = [np.eye(4) for _ in frames]
        self.points = [{"id": i, "position": np.zeros(3, np.float32), "color": np.zeros(3, np.uint8), "observed_keyframes": dict(o)}
                       for i, o in enumerate(points)]
        self.obs_off, self.obs_kf, self.obs_kp = obs_arrays(self.points) if self.points else (np.zeros(1, np.int32), np.zeros(0, np.int32),
                                                                                                 np.zeros(0, np.int32))

    def build(self, ctx, vocabulary=None):
        from tests.map_worlds import kps_array
        m = new_mapper(ctx, self.K, (8, 16, 64, 256), vocabulary)
        for k in range(self.n_kf):
            m.add_keyframe(np.zeros((32, 32), np.uint8), kps_array(self.kf_xy[k]), self.kf_desc[k], self.kf_poses[k])
        if self.points:
            m.update_map_points(self.points)
        return m


def _rows(*words):
    return [(w, []) for w in words]


def hand_cases():
    """name -> (HandWorld, keyword arguments of the call).  The asking keyframe is the last.  Keyframes alternate between two disjoint
    sets of words where it matters that no growth step matches (it needs 8 matches: no keyframe here has 8 rows in common with its
    neighbour anyway)."""
    cases = {}
    # p connected to nothing: min_score 1.0, only a keyframe with p's exact counts passes (keyframe 0 has them, keyframe 1 does not)
    cases["no_connected"] = (HandWorld([_rows(0, 1, 2), _rows(0, 1, 3), _rows(4, 5), _rows(0, 1, 2)], []), dict(min_weight=1))
    # every keyframe connected to p: max_common 0
    cases["all_connected"] = (HandWorld([_rows(0, 1), _rows(0, 2), _rows(0, 1)], [{0: 0, 1: 0, 2: 0}]), dict(min_weight=1))
    # all weights 0: no score, no common word
    cases["zero_weights"] = (HandWorld([_rows(0, 1), _rows(2, 3), _rows(0, 1)], [], weights=np.zeros(7)), dict(min_weight=1))
    # groups.  p = 4 is connected to keyframe 2 alone, which shares no word with it: min_score 0.  Keyframes 0, 1 and 3 have all four
    # words of p: S = M = {0, 1, 3}; scores 1.0, 0.8 and 2 / 3.  W[0][1] = 2, W[0][3] = 1: N_0 = [1, 3], N_1 = [0], N_3 = [0]; every best_k
    # is 0.  With n_best = 0 acc = score and best_k = k: 0 and 1 are retained (0.8 > 0.75), 3 is not: n_found = 2.
    frames = [_rows(0, 1, 2, 3), _rows(0, 1, 2, 3, 4), _rows(5, 6), _rows(0, 1, 2, 3, 5, 5), _rows(0, 1, 2, 3)]
    pts = [{0: 0, 1: 0}, {0: 1, 1: 1}, {3: 0, 0: 2}, {4: 0, 2: 0}]
    cases["groups"] = (HandWorld(frames, pts), dict(min_weight=1))
    cases["n_best_0"] = (HandWorld(frames, pts), dict(min_weight=1, n_best=0))
    cases["max_cand_0"] = (HandWorld(frames, pts), dict(min_weight=1, max_cand=0))
    cases["max_cand_1"] = (HandWorld(frames, pts), dict(min_weight=1, n_best=0, max_cand=1))   # fewer than n_found
    # matching, min_weight 2.  p = keyframe 2 is connected to keyframe 1 (two points), which shares one word with it: a low min_score;
    # it shares one point with keyframe 0, which is therefore not connected and is the candidate.  Train row 0 (word 0) is the best
    # neighbour of query rows 0 (distance 1), 1 (distance 1) and 2 (distance 2): row 0 keeps it (equal distances: the lower row).  Train
    # row 1 (word 1): query rows 3 (distance 2) and 4 (distance 1): row 4 keeps it.  Query row 5 matches train row 2, and both rows
    # belong to map point 4 (a = b): it does not count.  Query row 6 has no map point (its train row 3 has one); query row 7 has one, its
    # train row 4 has none.
    q = [(0, [0]), (0, [1]), (0, [2, 3]), (1, [0, 1]), (1, [2]), (2, []), (3, []), (4, []), (5, []), (6, [])]
    t = _rows(0, 1, 2, 3, 4)
    pts = [{2: 0}, {2: 1}, {2: 2}, {2: 3}, {2: 5, 0: 2}, {2: 4}, {0: 0}, {0: 1}, {2: 7}, {0: 3}, {2: 8, 1: 0}, {2: 9, 1: 1}]
    cases["matching"] = (HandWorld([t, _rows(5, 6, 0), q], pts), dict(min_weight=2))
    # candidates of 0 rows and of 1 row cannot be built from counts (an empty keyframe scores 0): the matching of such frames is
    # covered by match() on constructed tables in the CPU test and by "one_row" here, whose candidate has one row
    cases["one_row"] = (HandWorld([_rows(0), _rows(5, 6), [(0, [0]), (0, [1, 2])]], [{0: 0}, {2: 0}, {2: 1}]), dict(min_weight=1))
    cases["empty_keyframe"] = (HandWorld([_rows(0, 1), [], _rows(5), _rows(0, 1)], [{0: 0}, {3: 0}]), dict(min_weight=1))
    return cases
