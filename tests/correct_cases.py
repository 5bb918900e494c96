"""Small constructed maps for the tests of the loop correction (mo_map_loop_correct, visual-slam_amd/csrc/map_correct.hip) and its numpy
restatement (tests/correct_restatement.py).  Plain numpy; the device map is built from a case by build_map, which imports the library when
called.

A case (Builder) is a true world - cameras T_i and points X_w - of which the old side (the group) is stored as it is and the return side
(the corrected keyframes and the duplicates they observe) is stored drifted by a similarity D, X_d = f R_D X_w + t_D: the duplicates at
D(X_w), the return poses as [R_i R_D^T | f t_i - R_i R_D^T t_D], every projection unchanged.  The confirmed model of (p, candidate) is then
s = f, R = R_p R_c^T, t = f (t_p - R t_c); the transform of rule 1 is D^-1, and a correct call puts the return side back at the true world.
Every real keyframe is followed by a filler keyframe of four rows (consecutive keyframes share no descriptor: add_keyframe's growth step
finds no match).  Descriptors are the code words of tests/reloc_cases.CODE, 128 bits apart, with a chosen number of bits flipped.

Each case carries checks: functions of the restatement's result that assert what the case was built to show.  check(case) runs them with
the margin condition (no float decision within MARGIN, relative to the image width, of going the other way); tests/test_correct_cpu.py
does so for every case, tests/test_gpu_correct.py again before it asks a device."""
import numpy as np

from tests import correct_restatement as CR
from tests import sim3_cases as SC
from tests.confirm_cases import MARGIN, flipped
from tests.fuse_restatement import as_arrays, lists_of
from tests.reloc_cases import ABSENT, CODE, FILLER0

K = SC.BASE_K
W_IMG, H_IMG = SC.W_IMG, SC.H_IMG
KINV = np.linalg.inv(K)
PRM = dict(radius=4.0, scale_factor=1.2, max_dist=50, chi2=5.991)


def proj(T, X):
    x = K @ (T[:3, :3] @ np.asarray(X, np.float64) + T[:3, 3])
    return x[:2] / x[2], x[2]


class Builder:
    def __init__(self, name, f=1.3, w_D=(0.02, -0.03, 0.015), t_D=(0.3, -0.2, 0.4), seed=1, **prm):
        self.name, self.family = name, name.split(":")[0]
        self.rng = np.random.default_rng(seed)
        self.f, self.R_D, self.t_D = float(f), SC.rot(list(w_D)), np.asarray(t_D, np.float64)
        self.kf, self.true_pose, self.side = [], [], []    # per position; side: "old", "ret", "other", "filler"
        self.xyz, self.obs, self.world = [], [], []          # per point; world: the true position (None: not known)
        self.p = self.q = None
        self.lp = {}                                         # row of p -> point
        self.lp_null = False
        self.corrected = self.group = None                   # explicit position lists (None: every "ret" / "old" keyframe)
        self.prm = dict(PRM, **prm)
        self.checks, self.expect = [], {}
        self.junk = ()                                       # stored entries that name nothing
        self._word = 0
        self._inp = None

    # ---- keyframes, rows, points
    def keyframe(self, side, c):
        """a real keyframe with the true pose SC._cand_pose(c), and the filler behind it; returns its position"""
        T = SC._cand_pose(c)
        fi = len(self.kf) // 2
        self.kf.append({"xy": [], "oct": [], "desc": []}); self.true_pose.append(T); self.side.append(side)
        words = FILLER0 + 4 * (fi % 7) + np.arange(4)
        self.kf.append({"xy": [self.rng.uniform([0, 0], [W_IMG, H_IMG]) for _ in range(4)], "oct": [0] * 4, "desc": [CODE[w] for w in words]})
        self.true_pose.append(SC._cand_pose(40 + fi)); self.side.append("filler")
        return len(self.kf) - 2

    def drifted(self, X):
        return self.f * (self.R_D @ np.asarray(X, np.float64)) + self.t_D

    def stored_pose(self, pos):
        T = self.true_pose[pos]
        if self.side[pos] != "ret":
            return T.copy()
        S = np.eye(4)
        S[:3, :3] = T[:3, :3] @ self.R_D.T
        S[:3, 3] = self.f * T[:3, 3] - S[:3, :3] @ self.t_D
        return S

    def row(self, pos, xy, desc, octave=0):
        k = self.kf[pos]
        k["xy"].append(np.asarray(xy, np.float64)); k["oct"].append(int(octave)); k["desc"].append(np.asarray(desc, np.uint8))
        return len(k["xy"]) - 1

    def pad(self, pos, n_rows):
        while len(self.kf[pos]["xy"]) < n_rows:
            self.row(pos, self.rng.uniform([0, 0], [W_IMG, H_IMG]), CODE[ABSENT])

    def point(self, X, obs, drift=False, world=True):
        self.xyz.append((self.drifted(X) if drift else np.asarray(X, np.float64)).astype(np.float32))
        self.obs.append(list(obs))
        self.world.append(np.asarray(X, np.float64) if world else None)
        return len(self.xyz) - 1

    def word(self):
        self._word += 1
        assert self._word < FILLER0
        return self._word - 1

    def draw(self, views, edge=40.0):
        """a world point whose projections lie `edge` pixels inside the image of every keyframe of `views`"""
        T0 = np.linalg.inv(self.true_pose[views[0]])
        while True:
            Xc = (KINV @ np.append(self.rng.uniform([edge, edge], [W_IMG - edge, H_IMG - edge]), 1.0)) * self.rng.uniform(4.0, 9.0)
            X = T0[:3, :3] @ Xc + T0[:3, 3]
            if all(z > 1.0 and edge <= u[0] <= W_IMG - edge and edge <= u[1] <= H_IMG - edge for u, z in (proj(self.true_pose[v], X) for v in views)):
                return X

    def feat(self, old=(), ret=(), dup=None, rows=None, listed=False, d_old=0, d_ret=0, X=None, word=None):
        """One feature: a world point with a row at its projection in every keyframe of `old` and `rows` (default: ret); an old point
        observed by `old` (when old is not empty) and a duplicate, stored drifted, observed by `dup` (default: ret; () for none).
        listed: the row of p names the old point in loop_point.  Returns a dict with X, L (old point, -1), o (duplicate, -1), row."""
        rows = tuple(ret) if rows is None else tuple(rows)
        dup = tuple(ret) if dup is None else tuple(dup)
        w = self.word() if word is None else word
        views = list(old) + list(rows)
        X = self.draw(views) if X is None else np.asarray(X, np.float64)
        r = {}
        for v in views:
            r[v] = self.row(v, proj(self.true_pose[v], X)[0], flipped(CODE[w], d_old if v in old else d_ret))
        fe = {"X": X, "word": w, "row": r, "L": -1, "o": -1}
        if old:
            fe["L"] = self.point(X, [(v, r[v]) for v in old])
        if dup:
            fe["o"] = self.point(X, [(v, r[v]) for v in dup], drift=True)
        if listed:
            self.lp[r[self.p]] = fe["L"]
        return fe

    def that(self, fn):
        self.checks.append(fn)

    # ---- what the tests read
    def positions(self, side):
        return [i for i, s in enumerate(self.side) if s == side]

    def masks(self):
        n = len(self.kf)
        c, g = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        c[np.array(self.positions("ret") if self.corrected is None else self.corrected, np.int64)] = 1
        g[np.array(self.positions("old") if self.group is None else self.group, np.int64)] = 1
        return c, g

    def model(self):
        Tp, Tc = self.true_pose[self.p], self.true_pose[self.q]
        R = Tp[:3, :3] @ Tc[:3, :3].T
        return self.f, R, self.f * (Tp[:3, 3] - R @ Tc[:3, 3])

    def loop_point(self):
        if self.lp_null:
            return None
        lp = np.full(len(self.kf[self.p]["xy"]), -1, np.int32)
        for r, L in self.lp.items():
            lp[r] = L
        return lp

    def finish(self):
        if self._inp is None:
            for pos in range(len(self.kf)):   # (the smallest keyframe the store takes has four rows)
                self.pad(pos, 4)
            self._inp = True
        return self

    def arrays(self):
        self.finish()
        return as_arrays(np.array(self.xyz, np.float32).reshape(-1, 3), self.obs)

    def poses(self):
        return [self.stored_pose(i) for i in range(len(self.kf))]

    def restate(self, a=None, **over):
        self.finish()
        c, g = self.masks()
        return CR.correct(self.arrays() if a is None else a, K, self.poses(), [k["xy"] for k in self.kf], [k["oct"] for k in self.kf],
                          [np.array(k["desc"], np.uint8).reshape(-1, 32) for k in self.kf], self.p, self.q, self.model(), c, g, self.loop_point(),
                          W_IMG, H_IMG, **dict(self.prm, **over))

    def confirm(self):
        """what correct_loop takes: confirm_loop's info, as far as it is read"""
        s, R, t = self.model()
        return {"win": 0, "kf_pos": self.p, "loop_point": self.loop_point(), "candidates": [{"pos": self.q, "scale": s, "R": R, "t": t}]}

    def call(self, m, **over):
        c, g = self.masks()
        return m.correct_loop(self.confirm(), corrected=np.flatnonzero(c).tolist(), group=np.flatnonzero(g).tolist(), image_size=(W_IMG, H_IMG),
                              **dict(self.prm, **over))

    def build_map(self, ctx):
        from vslam_amd.mapper import LocalMapper
        from tests.map_worlds import kps_array
        self.finish()
        m = LocalMapper(K, save_every_keyframe=False, context=ctx)
        img = np.zeros((H_IMG, W_IMG), np.uint8)
        for k, T in zip(self.kf, self.poses()):
            m.add_keyframe(img, kps_array(np.array(k["xy"]), np.array(k["oct"], np.int32)), np.array(k["desc"], np.uint8), T)
        assert len(m.map_points) == 0, "a growth step found a model"
        if self.xyz:
            m.update_map_points([{"id": j, "position": self.xyz[j], "color": np.zeros(3, np.uint8), "observed_keyframes": dict(o)}
                                 for j, o in enumerate(self.obs)])
        assert len(m.keyframes) == len(self.kf)
        return m


def check(case, res=None):
    """the case's own conditions on the restatement, and the margin of every float decision"""
    res = case.restate() if res is None else res
    assert res["margins"]["min"] >= MARGIN * W_IMG, (case.name, res["margins"])
    for k, v in case.expect.items():
        assert res["counts"][k] == v, (case.name, k, res["counts"][k], v)
    for fn in case.checks:
        assert fn(res), case.name
    return res


def absorbed_into(res, o, L):
    """old index o is gone into the point old index L became, and L's own fields survive"""
    return res["fused"] and res["survivor"][o] == L and res["into"][o] == res["into"][L]


def truth_error(case, res):
    """largest distance of a corrected pose and of a surviving moved point from the true world"""
    e = 0.0
    c, _ = case.masks()
    for k in np.flatnonzero(c):
        e = max(e, np.abs(res["poses_out"][k] - case.true_pose[k][:3, :4]).max())
    for old in range(len(case.xyz)):
        if res["moved"][old] and case.world[old] is not None and (not res["fused"] or res["survivor"][old] == old):
            e = max(e, np.abs(res["arrays"]["xyz"][res["into"][old]].astype(np.float64) - case.world[old]).max())
    return e


# ---- the base scene -----------------------------------------------------------------------------------------------------------------------
def scene(name, n_ret=3, n_old=2, lead=0, f=1.3, seed=1, n_dup=4, n_free=2, n_unlisted=2, n_unseen=1, **kw):
    """`lead` other keyframes, n_old old ones (the first is the candidate), one other keyframe, n_ret return keyframes (the last is p).
    Features: n_dup listed duplicates (direct edges), n_free listed free rows (direct gains at p, search gains elsewhere), n_unlisted
    duplicates the search must find, n_unseen old points without a row on the return side."""
    b = Builder(name, f=f, seed=seed, **kw)
    for i in range(lead):
        b.keyframe("other", 30 + i)
    old = [b.keyframe("old", i) for i in range(n_old)]
    b.keyframe("other", 20)
    ret = [b.keyframe("ret", 1 + (i % 3)) for i in range(n_ret)]
    b.p, b.q = ret[-1], old[0]
    b.old, b.ret = old, ret
    b.f_dup = [b.feat(old, ret, listed=True) for _ in range(n_dup)]
    b.f_free = [b.feat(old, ret, dup=(), listed=True) for _ in range(n_free)]
    b.f_unl = [b.feat(old, ret) for _ in range(n_unlisted)]
    b.f_unseen = [b.feat(old, ()) for _ in range(n_unseen)]
    # a point of a keyframe outside both masks: never moved, never fused
    other = b.positions("other")[-1]
    b.bystander = b.point(b.draw([other]), [(other, b.row(other, [50.0, 60.0], CODE[b.word()]))], world=False)
    return b


def _expect_scene(b, extra_edges=0):
    """what the base scene gives with every corrected keyframe seeing every feature"""
    nr = len(b.ret)
    n_l = len(b.f_dup) + len(b.f_free) + len(b.f_unl) + len(b.f_unseen)
    b.expect.update(n_corrected=nr, n_loop_points=n_l, n_moved=len(b.f_dup) + len(b.f_unl), n_direct_edges=len(b.f_dup), n_direct_gained=len(b.f_free),
                    n_pairs=n_l * nr, n_proposals=(n_l - len(b.f_unseen)) * nr, n_gained=len(b.f_free) * (nr - 1),
                    n_edges=(len(b.f_dup) + len(b.f_unl)) * nr + len(b.f_free) + extra_edges, n_absorbed=len(b.f_dup) + len(b.f_unl))
    for fe in b.f_dup + b.f_unl:
        b.that(lambda res, fe=fe: absorbed_into(res, fe["o"], fe["L"]) and not res["moved"][fe["L"]])
    b.that(lambda res: not res["moved"][b.bystander] and np.array_equal(res["arrays"]["xyz"][res["into"][b.bystander]], b.xyz[b.bystander]))
    # a loop point keeps its bytes, and holds one observation per corrected keyframe that has its row
    def lists(res):
        new = lists_of(res["arrays"])
        for fe in b.f_dup + b.f_free + b.f_unl:
            j = int(res["into"][fe["L"]])
            if not np.array_equal(res["arrays"]["xyz"][j], b.xyz[fe["L"]]) or sorted(e for e in new[j] if e not in b.junk) != sorted(fe["row"].items()):
                return False
        return True
    b.that(lists)
    return b


def points(n):
    """the map holds exactly n points: one block's edge of the per-point kernels"""
    b = scene("points:%d" % n, seed=10 + n)
    other = b.positions("other")[0]
    while len(b.xyz) < n:
        b.point(b.draw([other]), [(other, b.row(other, b.rng.uniform([0, 0], [W_IMG, H_IMG]), CODE[ABSENT]))], world=False)
    b.that(lambda res: len(res["into"]) == n)
    return _expect_scene(b)


def rows(n):
    """p has n rows, the last one listed"""
    b = scene("rows:%d" % n, seed=20 + n)
    b.pad(b.p, n - 1)
    last = b.feat(b.old, b.ret, listed=True)
    b.f_dup.append(last)
    assert last["row"][b.p] == n - 1
    return _expect_scene(b)


def corrected_set(tag):
    if tag == "alone":
        b = scene("corrected:alone", n_ret=1, seed=31)
    elif tag == "scattered":
        b = scene("corrected:scattered", n_ret=4, seed=32)
        b.that(lambda res: np.flatnonzero(b.masks()[0]).tolist() == b.ret and np.diff(b.ret).min() >= 2)
    else:
        # position 0 is a return keyframe: the return side was stored first
        b = Builder("corrected:with_zero", seed=33)
        r0 = b.keyframe("ret", 1)
        old = [b.keyframe("old", 0), b.keyframe("old", 4)]
        b.keyframe("other", 20)
        ret = [r0, b.keyframe("ret", 2), b.keyframe("ret", 3)]
        b.p, b.q, b.old, b.ret = ret[-1], old[0], old, ret
        b.f_dup = [b.feat(old, ret, listed=True) for _ in range(3)]
        b.f_free = [b.feat(old, ret, dup=(), listed=True) for _ in range(2)]
        b.f_unl = [b.feat(old, ret) for _ in range(2)]
        b.f_unseen = []
        other = b.positions("other")[-1]
        b.bystander = b.point(b.draw([other]), [(other, b.row(other, [50.0, 60.0], CODE[b.word()]))], world=False)
        assert r0 == 0
    return _expect_scene(b)


def empty_group():
    """no group: no loop point, nothing fuses; the return side still moves, in place"""
    b = scene("empty_group", seed=40)
    b.group = []
    b.lp = {}
    n_moved = sum(1 for o in b.obs if any(k in b.ret for k, _ in o))
    b.expect.update(n_loop_points=0, n_pairs=0, n_proposals=0, n_direct_edges=0, n_direct_gained=0, n_absorbed=0, n_moved=n_moved)
    b.that(lambda res: not res["fused"] and np.array_equal(res["into"], np.arange(len(b.xyz))) and res["moved"].sum() == n_moved)
    b.that(lambda res: not np.array_equal(res["arrays"]["xyz"], np.array(b.xyz, np.float32)))
    return b


def loop_point_cases():
    out = []
    b = scene("loop_point:null", seed=50)
    b.lp_null = True
    # without the list the search finds every duplicate and every free row by itself
    nr, nl = len(b.ret), 9
    b.expect.update(n_direct_edges=0, n_direct_gained=0, n_proposals=(nl - 1) * nr, n_gained=2 * nr, n_edges=6 * nr, n_absorbed=6)
    out.append(b)
    b = scene("loop_point:out_of_range", seed=51)
    _expect_scene(b)
    b.pad(b.p, 12)
    free = [r for r in range(len(b.kf[b.p]["xy"])) if r not in b.lp][:4]
    for r, v in zip(free, (len(b.xyz), len(b.xyz) + 7, -7, 2 ** 31 - 1)):
        b.lp[r] = v
    out.append(b)
    # two rows of p name one L: the lower row gets it, the other stays free
    b = scene("loop_point:two_rows_one_L", seed=52, n_free=1)
    fe = b.f_free[0]
    r2 = b.row(b.p, proj(b.true_pose[b.p], fe["X"])[0] + np.array([60.0, 0.0]), CODE[b.word()])
    b.lp[r2] = fe["L"]
    assert r2 > fe["row"][b.p]
    _expect_scene(b)
    b.that(lambda res, b=b, fe=fe, r2=r2: res["drow"] == {fe["L"]: fe["row"][b.p]} and (b.p, r2) not in lists_of(res["arrays"])[res["into"][fe["L"]]])
    out.append(b)
    return out


def direct_cases():
    out = []
    # a row of p owned by a duplicate that has MORE observations than the loop point: the loop point survives all the same
    b = scene("direct:edge_fewer_obs", n_ret=4, n_old=1, seed=60)
    _expect_scene(b)
    b.that(lambda res, b=b: all(len(b.obs[fe["o"]]) > len(b.obs[fe["L"]]) for fe in b.f_dup))
    out.append(b)
    b = scene("direct:gain", n_dup=0, n_unlisted=0, n_unseen=0, n_free=3, seed=61)
    _expect_scene(b)
    b.that(lambda res, b=b: res["fused"] and res["counts"]["n_absorbed"] == 0 and res["counts"]["n_obs"] == len(sum(b.obs, [])) + 3 * len(b.ret))
    out.append(b)
    # L already observes p at another row: the free row it is named for is not gained, and p is no pair of the search for it
    b = scene("direct:already_observing", n_dup=0, n_unlisted=0, n_unseen=0, n_free=1, seed=62)
    fe = b.f_free[0]
    r2 = b.row(b.p, [33.0, 44.0], CODE[b.word()])
    b.obs[fe["L"]].append((b.p, r2))
    b.group = b.old   # (p stays outside the group although a loop point sees it)
    nr = len(b.ret)
    b.expect.update(n_direct_gained=0, n_direct_edges=0, n_pairs=nr - 1, n_proposals=nr - 1, n_gained=nr - 1, n_edges=0, n_moved=0)
    b.that(lambda res, b=b, fe=fe: (b.p, fe["row"][b.p]) not in lists_of(res["arrays"])[res["into"][fe["L"]]])
    out.append(b)
    return out


def seen_by_corrected():
    """a loop point that a corrected keyframe also observes is not moved (ORB-SLAM2 would move it)"""
    b = scene("loop_point_seen_by_corrected", seed=70)
    fe = b.f_free[0]
    k = b.ret[0]
    b.obs[fe["L"]].append((k, fe["row"][k]))
    _expect_scene(b)
    b.expect.update(n_pairs=b.expect["n_pairs"] - 1, n_proposals=b.expect["n_proposals"] - 1, n_gained=b.expect["n_gained"] - 1)
    b.that(lambda res: not res["moved"][fe["L"]] and np.array_equal(res["arrays"]["xyz"][res["into"][fe["L"]]], b.xyz[fe["L"]]))
    return b


def search_on_given_row():
    """two old points are one feature; the row of p names the first (a free row: rule 4 gives it away), the search of the second lands on
    that very row: the row counts as owned, the two old points merge"""
    b = scene("search_on_given_row", n_dup=0, n_unlisted=0, n_unseen=0, n_free=1, n_ret=1, seed=80)
    fe = b.f_free[0]
    k2 = b.old[1]
    r2 = b.row(k2, proj(b.true_pose[k2], fe["X"])[0] + np.array([30.0, 0.0]), flipped(CODE[fe["word"]], 2))
    L2 = b.point(fe["X"], [(k2, r2)])
    # claims on (p, row): L at distance 0 (itself the row's new owner: a self edge), L2 at distance 2 loses the claim ... so L2 is given a
    # lower distance than L: L's representative is flipped by 3 bits
    for v in b.old:
        b.kf[v]["desc"][fe["row"][v]] = flipped(CODE[fe["word"]], 3)
    b.kf[k2]["desc"][r2] = flipped(CODE[fe["word"]], 1)
    b.expect.update(n_direct_gained=1, n_direct_edges=0, n_pairs=2, n_proposals=2, n_gained=0, n_edges=1, n_absorbed=1)
    b.that(lambda res: res["claim"][(b.p, fe["row"][b.p])][1] == L2 and res["survivor"][L2] == fe["L"] and
           lists_of(res["arrays"])[res["into"][fe["L"]]].count((b.p, fe["row"][b.p])) == 1)
    return b


def chain():
    """o1 - L - o2: the row of p belongs to o1 (direct edge), the row of another corrected keyframe to o2 (the search's edge): three into L"""
    b = scene("chain", n_dup=0, n_unlisted=0, n_unseen=0, n_free=0, n_ret=2, seed=90)
    k2 = b.ret[0]
    X = b.draw(b.old + b.ret)
    fe = b.feat(b.old, b.ret, dup=(b.p,), listed=True, X=X)
    o2 = b.point(X, [(k2, fe["row"][k2])], drift=True)
    b.expect.update(n_direct_edges=1, n_direct_gained=0, n_pairs=2, n_proposals=2, n_edges=2, n_gained=0, n_absorbed=2, n_moved=2)
    b.that(lambda res: absorbed_into(res, fe["o"], fe["L"]) and absorbed_into(res, o2, fe["L"]) and
           sorted(lists_of(res["arrays"])[res["into"][fe["L"]]]) == sorted(fe["row"].items()))
    return b


def two_loop_points(tag):
    """two loop points in one component through the duplicate that owns the row of p: L1 is named, L2 wins the search's claim on the row
    (distance 1 against 3).  more_obs: L2 has two observations, L1 one: L2 survives.  tie: one each: the lower index."""
    b = scene("two_loop_points:" + tag, n_dup=0, n_unlisted=0, n_unseen=0, n_free=0, n_ret=1, n_old=3, seed=100 + len(tag))
    X = b.draw(b.old + b.ret)
    w = b.word()
    fe = b.feat(b.old[:1], b.ret, listed=True, X=X, word=w, d_old=3)
    v2 = b.old[1:] if tag == "more_obs" else b.old[1:2]
    r2 = {v: b.row(v, proj(b.true_pose[v], X)[0], flipped(CODE[w], 1)) for v in v2}
    L2 = b.point(X, [(v, r) for v, r in r2.items()])
    win = L2 if tag == "more_obs" else min(fe["L"], L2)
    assert fe["L"] < L2
    b.expect.update(n_direct_edges=1, n_pairs=2, n_proposals=2, n_edges=1, n_absorbed=2)
    b.that(lambda res: res["claim"][(b.p, fe["row"][b.p])][1] == L2 and all(res["survivor"][i] == win for i in (fe["L"], L2, fe["o"])))
    return b


def stale_observations():
    """entries that name nothing - a position past the map, one before its start, a row past the keyframe, a row before its start - in
    front of the valid ones; a point whose entries all name nothing is neither moved nor a loop point and keeps its bytes"""
    b = scene("stale_observations", seed=110)
    b.finish()
    n_kf = len(b.kf)
    other = b.positions("other")[-1]   # (a position no point of the scene observes: update_map_points takes one row per position)
    junk = b.junk = [(n_kf + 3, 0), (-n_kf - 2, 1), (other, 4000), (other, -300)]
    for i, fe in enumerate(b.f_dup + b.f_free + b.f_unl):
        b.obs[fe["L"]].insert(0, junk[i % 4])
        if fe["o"] >= 0:
            b.obs[fe["o"]].insert(0, junk[(i + 1) % 4])
    ghost = b.point(b.f_dup[0]["X"], [junk[0], junk[1], junk[2]], world=False)
    # a negative position that does name a keyframe: the last filler, from the end
    neg = b.point(b.draw([b.p]), [(b.p - n_kf, b.row(b.p, [77.0, 88.0], CODE[b.word()]))], drift=True)
    b._inp = None
    _expect_scene(b)
    b.expect.update(n_moved=b.expect["n_moved"] + 1)
    b.that(lambda res: not res["moved"][ghost] and res["moved"][neg] and lists_of(res["arrays"])[res["into"][ghost]] == [junk[0], junk[1], junk[2]])
    return b


def scales():
    out = [_expect_scene(scene("scale:rigid", f=1.0, w_D=(0, 0, 0), t_D=(0.5, -0.3, 0.8), seed=120)),
           _expect_scene(scene("scale:1.3", f=1.3, seed=121)), _expect_scene(scene("scale:0.5", f=0.5, seed=122))]
    for b in out:
        b.that(lambda res, b=b: abs(res["A_scale"] * b.f - 1.0) < 1e-15)
    return out


def tracking():
    """40 listed duplicates: enough of a map, once corrected, for track_local_map, fuse_map_points and bundle_adjust to work on"""
    return _expect_scene(scene("tracking", n_dup=40, n_free=0, n_unlisted=0, n_unseen=0, seed=130))


def error_calls(n_kf):
    """every error of rule 8 as (changes of the raw call, expected code name): tests/test_gpu_correct.py makes the calls"""
    nan, inf = float("nan"), float("inf")
    return [(dict(kf_pos=n_kf), "ARG"), (dict(kf_pos=-1), "ARG"), (dict(cand_pos=n_kf), "ARG"), (dict(cand_pos=-1), "ARG"), (dict(drop_p=True), "ARG"),
            (dict(both=True), "ARG"), (dict(scale=0.0), "ARG"), (dict(scale=-1.0), "ARG"), (dict(scale=nan), "ARG"), (dict(scale=inf), "ARG"),
            (dict(R0=nan), "ARG"), (dict(t0=inf), "ARG"), (dict(w=0), "ARG"), (dict(h=0), "ARG"), (dict(h=-3), "ARG")]


FAMILIES = {"points", "rows", "corrected", "empty_group", "loop_point", "direct", "loop_point_seen_by_corrected", "search_on_given_row", "chain",
            "two_loop_points", "stale_observations", "scale", "tracking", "errors"}
_CASES = []


def all_cases():
    if not _CASES:
        cs = [points(n) for n in (255, 256, 257)] + [rows(n) for n in (63, 64, 65, 1025)] + [corrected_set(t) for t in ("alone", "scattered", "with_zero")]
        cs += [empty_group()] + loop_point_cases() + direct_cases() + [seen_by_corrected(), search_on_given_row(), chain(), two_loop_points("more_obs"),
                                                                         two_loop_points("tie"), stale_observations()] + scales() + [tracking()]
        assert len({c.name for c in cs}) == len(cs)
        _CASES.extend(cs)
    return _CASES

