"""Small constructed maps for the tests of the loop confirmation (mo_map_loop_confirm, visual-slam_amd/csrc/map_confirm.hip), their numpy
restatement (tests/confirm_restatement.py) and the host replay of the refit (tests/native/confirm_replay.cpp).  Plain numpy; the device map
is built from a case by build_map, which imports the library when called.

A case (Builder) is an asking keyframe p at the last position, candidates (and the neighbours of their groups) before it, a filler
keyframe of four rows in front of every one of them (consecutive keyframes share no descriptor: add_keyframe's growth step finds no
match), and points injected through update_map_points with one or two observations (the representative is the first valid observation's
row).  The geometry is made in the camera frames: a feature is a point X2 in the candidate's camera, X1 = S12 X2 in the asking camera under
the candidate's similarity, the keypoints on the projections, the map points T1^-1 X1 and T2^-1 X2 rounded to f32.  Descriptors are the
code words of tests/reloc_cases.CODE (128 bits apart from each other) with a chosen number of bits flipped (flipped(): the first 32
through tests/loop_worlds.near, further ones in the word's first bytes).

Each case carries checks: functions of (front, replay, back) that assert what the case was built to show, on the restatement and the
replay alone.  check(case, ev) runs them with the margin conditions; tests/test_confirm_cpu.py does so for every case, and
tests/test_gpu_confirm.py again before it asks a device."""
import os
import struct
import subprocess

import numpy as np

from tests import confirm_restatement as CR
from tests import sim3_cases as SC
from tests.loop_worlds import near
from tests.reloc_cases import ABSENT, CODE, FILLER0

K = SC.BASE_K
W_IMG, H_IMG = SC.W_IMG, SC.H_IMG
MARGIN = 1e-6   # every float decision of the searches and every selection of the refit keeps this relative distance from its threshold
# Noise-free refits against the constructed truth (max abs over s, R, t).  Map points and keypoints are f32, as in tests/sim3_cases.py.
# Measured on the host replay over the noise-free cases of this file: 2.7e-8 (refit:guided_raise), 3.5e-8 (total:39, total:40), 8.2e-8
# (refit:back, whose start is 5 % / 0.05 rad off).  The replay is held to that measurement, the device to ten times it.
TRUTH_REPLAY = 8.3e-8
TRUTH_BOUND = 8.3e-7
KINV = np.linalg.inv(K)


def flipped(desc, k):
    """desc with k bits flipped: 0 .. 31 of the last 32 bits (loop_worlds.near), then bits of the first bytes"""
    d = near(desc, range(min(k, 32)))
    for b in range(max(k - 32, 0)):
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def cam_point(px, z):
    """the point of depth z on the ray of pixel px"""
    return (KINV @ np.array([px[0], px[1], 1.0])) * z


def proj(X):
    x = K @ np.asarray(X, np.float64)
    return x[:2] / x[2]


def as_tuple(S):
    return (S["s"], S["R"], S["t"])


def _sim_of(c):
    return SC.sim(0.8 + 0.1 * (c % 7), [0.02 * (c % 4) - 0.03, 0.03 * (c % 3) - 0.03, 0.01 * (c % 5) - 0.02], [0.1 * (c % 5) - 0.2, 0.05 * (c % 7) - 0.15, 0.1 * (c % 3)])


class Builder:
    def __init__(self, name, n_cand=1, seed=1, neighbours=0, rigid=False, **prm):
        """rigid: the candidates' similarities are the rigid motions between the cameras (scale 1, T1 T2^-1): a map point then lies where both
        keyframes see it, and one point can be observed from both"""
        self.name, self.family = name, name.split(":")[0]
        self.rng = np.random.default_rng(seed)
        self.kf = []     # per position: dict xy, oct, desc (lists), pose
        self.cand, self.nb = [], []
        self.sims = [_sim_of(c) for c in range(n_cand)]
        for c in range(n_cand):
            self.nb.append([self._keyframe(SC._cand_pose(20 + 3 * c + q)) for q in range(neighbours)])
            self.cand.append(self._keyframe(SC._cand_pose(c)))
        self.p = self._keyframe(SC.T_ASK)
        if rigid:
            for c, k in enumerate(self.cand):
                T = SC.T_ASK @ np.linalg.inv(self.kf[k]["pose"])
                self.sims[c] = {"s": 1.0, "R": T[:3, :3].copy(), "t": T[:3, 3].copy()}
        self.xyz, self.obs = [], []
        self.cur = {}                                   # row of p -> point
        self.match = [dict() for _ in range(n_cand)]    # row of p -> (b, j, flag)
        self.models = [as_tuple(S) for S in self.sims]
        self.group = "default"                          # the candidate and its neighbours; None: NULL; or an explicit [n_cand][n_kf] mask
        self.inlier_null = False
        self.prm = dict(radius_guided=7.5, radius_proj=10.0, max_dist=50, chi2=SC.CHI2, scale_factor=SC.SF, min_inliers=3, min_matches=40)
        self.prm.update(prm)
        self.truth = [None] * n_cand                    # per candidate the similarity a noise-free refit must return
        self.checks = []
        self._word = 0
        self._inp = None

    # ---- keyframes, rows, points
    def _keyframe(self, T):
        f = len(self.kf) // 2
        words = FILLER0 + 4 * (f % 7) + np.arange(4)
        self.kf.append({"xy": [self.rng.uniform([0, 0], [W_IMG, H_IMG]) for _ in range(4)], "oct": [0] * 4, "desc": [CODE[w] for w in words],
                        "pose": SC._cand_pose(40 + f)})
        self.kf.append({"xy": [], "oct": [], "desc": [], "pose": np.asarray(T, np.float64)})
        return len(self.kf) - 1

    def row(self, pos, xy, desc, octave=0):
        k = self.kf[pos]
        k["xy"].append(np.asarray(xy, np.float64)); k["oct"].append(int(octave)); k["desc"].append(np.asarray(desc, np.uint8))
        return len(k["xy"]) - 1

    def pad(self, pos, n_rows):
        """random rows that hold the word no feature holds, up to n_rows rows"""
        while len(self.kf[pos]["xy"]) < n_rows:
            self.row(pos, self.rng.uniform([0, 0], [W_IMG, H_IMG]), CODE[ABSENT])

    def point(self, X_cam, pos_of_frame, obs):
        """a map point: X_cam in the camera frame of keyframe pos_of_frame, obs = [(position, row)] as stored"""
        Ti = np.linalg.inv(self.kf[pos_of_frame]["pose"])
        self.xyz.append((Ti[:3, :3] @ np.asarray(X_cam, np.float64) + Ti[:3, 3]).astype(np.float32))
        self.obs.append(list(obs))
        return len(self.xyz) - 1

    def word(self):
        self._word += 1
        assert self._word < FILLER0
        return self._word - 1

    def draw(self, c, edge=40.0):
        """X2 in front of candidate c whose X1 = S12 X2 lies in front of p, both projections `edge` pixels inside the image"""
        while True:
            X2 = cam_point(self.rng.uniform([edge, edge], [W_IMG - edge, H_IMG - edge]), self.rng.uniform(3.0, 10.0))
            X1 = SC.sim_apply(self.sims[c], X2)
            if X1[2] > 1.0:
                u = proj(X1)
                if edge <= u[0] <= W_IMG - edge and edge <= u[1] <= H_IMG - edge:
                    return X2

    def feat(self, c, kind, X2=None, word=None, d1=0, d2=0, oct1=0, oct2=0, kp1=None, kp2=None, share=None, at=None, flag=1, row1=True, row2=True):
        """One feature of candidate c.  kind: "seed" (listed with flag), "guided" (both rows and both points, not listed), "free1" (the row
        of p has no point), "none" (no row of p at all).  at: the position that observes b (default: the candidate).  share: a feature
        whose X1, row of p and point a are used again (several candidates of one asking keyframe).  row2=False: no b."""
        w = self.word() if word is None else word
        f = {"c": c, "word": w}
        if share is not None:
            f["X1"], f["i"], f["a"] = share["X1"], share["i"], share["a"]
            f["X2"] = SC.sim_apply(SC.sim_inv(self.sims[c]), f["X1"])
        else:
            f["X2"] = self.draw(c) if X2 is None else np.asarray(X2, np.float64)
            f["X1"] = SC.sim_apply(self.sims[c], f["X2"])
            f["i"], f["a"] = -1, -1
            if row1 and kind != "none":
                f["i"] = self.row(self.p, proj(f["X1"]) if kp1 is None else kp1, flipped(CODE[w], d1), oct1)
                if kind != "free1":
                    f["a"] = self.point(f["X1"], self.p, [(self.p, f["i"])])
                    self.cur[f["i"]] = f["a"]
        f["j"], f["b"] = -1, -1
        if row2:
            pos = self.cand[c] if at is None else at
            f["j"] = self.row(pos, proj(f["X2"]) if kp2 is None else kp2, flipped(CODE[w], d2), oct2)
            f["b"] = self.point(f["X2"], self.cand[c], [(pos, f["j"])])
        if kind == "seed":
            self.match[c][f["i"]] = (f["b"], f["j"], flag)
        return f

    def seeds(self, c, n, **kw):
        return [self.feat(c, "seed", **kw) for _ in range(n)]

    # ---- what the tests read
    def n_kf(self):
        return len(self.kf)

    def group_mask(self):
        if self.group is None:
            return None
        if isinstance(self.group, str):
            g = np.zeros((len(self.cand), self.n_kf()), np.uint8)
            for c, k in enumerate(self.cand):
                g[c, [k] + self.nb[c]] = 1
            return g
        return np.asarray(self.group, np.uint8)

    def lists(self):
        n_p, nc = len(self.kf[self.p]["xy"]), len(self.cand)
        cur = np.full(n_p, -1, np.int32)
        for i, a in self.cur.items():
            cur[i] = a
        mpt, mrow, fl = np.full((nc, n_p), -1, np.int32), np.full((nc, n_p), -1, np.int32), np.zeros((nc, n_p), np.uint8)
        for c in range(nc):
            for i, (b, j, flag) in self.match[c].items():
                mpt[c, i], mrow[c, i], fl[c, i] = b, j, flag
        return cur, mpt, mrow, (None if self.inlier_null else fl)

    def obs_arrays(self):
        off, okf, okp = [0], [], []
        for o in self.obs:
            okf += [k for k, _ in o]; okp += [r for _, r in o]
            off.append(len(okf))
        return np.array(off, np.int32), np.array(okf, np.int32), np.array(okp, np.int32)

    def inputs(self):
        if self._inp is None:
            for pos in range(len(self.kf)):   # (the smallest keyframe the store takes has four rows)
                self.pad(pos, 4)
            cur, mpt, mrow, fl = self.lists()
            off, okf, okp = self.obs_arrays()
            self._inp = CR.Inputs(K, [k["pose"] for k in self.kf], [k["xy"] for k in self.kf], [k["oct"] for k in self.kf], [k["desc"] for k in self.kf],
                                  np.array(self.xyz, np.float32).reshape(-1, 3), off, okf, okp, self.p, self.cand, cur, mpt, mrow, fl, self.models,
                                  self.group_mask(), W_IMG, H_IMG, **self.prm)
        return self._inp

    def candidates(self):
        """the candidate dicts confirm_loop takes"""
        self.inputs()
        cur, mpt, mrow, _ = self.lists()
        g = self.group_mask()
        return [dict({"pos": k, "cur_point": cur, "match_point": mpt[c], "match_row": mrow[c]}, **({} if g is None else {"group": np.flatnonzero(g[c]).tolist()}))
                for c, k in enumerate(self.cand)]

    def alignment(self):
        """the per-candidate dicts of compute_sim3 confirm_loop takes"""
        fl = self.lists()[3]
        return [{"scale": s, "R": R, "t": t, "inlier": None if fl is None else fl[c]} for c, (s, R, t) in enumerate(self.models)]

    def call(self, m, **over):
        return m.confirm_loop(self.candidates(), self.alignment(), kf_position=self.p, image_size=(W_IMG, H_IMG), **dict(self.prm, **over))

    def build_map(self, ctx):
        from vslam_amd.mapper import LocalMapper
        from tests.map_worlds import kps_array
        self.inputs()
        m = LocalMapper(K, save_every_keyframe=False, context=ctx)
        img = np.zeros((H_IMG, W_IMG), np.uint8)
        for k in self.kf:
            m.add_keyframe(img, kps_array(np.array(k["xy"]), np.array(k["oct"], np.int32)), np.array(k["desc"], np.uint8), k["pose"])
        assert len(m.map_points) == 0, "a growth step found a model"
        m.update_map_points([{"id": j, "position": self.xyz[j], "color": np.zeros(3, np.uint8), "observed_keyframes": dict(o)} for j, o in enumerate(self.obs)])
        assert len(m.keyframes) == len(self.kf)
        return m

    def replay_input(self, fr):
        out = [K.astype("<f8").tobytes(), struct.pack("<dii", self.prm["chi2"], len(self.cand), 0)]
        for c in range(len(self.cand)):
            s, R, t = self.inputs().models[c]
            out += [struct.pack("<ii", int(fr["part"][c]), len(fr["rows"][c])), np.concatenate([[s], R.reshape(9), t]).astype("<f8").tobytes(),
                    fr["pairs"][c].astype("<f8").tobytes()]
        return b"".join(out)

    # the geometry of the searches as the device forms it (from the f32 point and the given model)
    def into_cand(self, c, a):
        inp_T1 = self.kf[self.p]["pose"]
        Y = CR.apply(CR.inverse(self.models[c]), CR.camera(inp_T1, self.xyz[a]))[0]
        return CR.project(K, Y, W_IMG, H_IMG)[:2]

    def into_p(self, c, b):
        Y = CR.apply(self.models[c], CR.camera(self.kf[self.cand[c]]["pose"], self.xyz[b]))[0]
        return CR.project(K, Y, W_IMG, H_IMG)[:2]


# ---- the replay and the whole evaluation on the host -------------------------------------------------------------------------------------
def build_replay(directory):
    return SC.build_native(directory, "confirm_replay")


def run_replay(exe, case, fr, directory):
    """the replay's output: margin, per candidate ninl, rounds, model [13], flags (bool [m])"""
    tag = case.name.replace(":", "_").replace("/", "_")
    src, dst = os.path.join(str(directory), tag + ".in"), os.path.join(str(directory), tag + ".out")
    with open(src, "wb") as f:
        f.write(case.replay_input(fr))
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(dst, "rb").read()
    os.remove(src); os.remove(dst)
    n_cand, _, margin = struct.unpack_from("<iid", raw, 0)
    at = 16
    res = {"margin": margin, "ninl": [], "rounds": [], "model": [], "flags": []}
    for c in range(n_cand):
        ninl, rounds = struct.unpack_from("<ii", raw, at); at += 8
        res["ninl"].append(ninl); res["rounds"].append(rounds)
        res["model"].append(np.frombuffer(raw, "<f8", 13, at).copy()); at += 104
        m = len(fr["rows"][c])
        res["flags"].append(np.frombuffer(raw, np.uint8, m, at).astype(bool)); at += m
    assert at == len(raw)
    return res


def model_tuple(m13):
    return (float(m13[0]), np.asarray(m13[1:10], np.float64).reshape(3, 3), np.asarray(m13[10:13], np.float64))


def evaluate(exe, case, directory):
    """(front, replay, back) of a case on the host"""
    inp = case.inputs()
    fr = CR.front(inp)
    rp = run_replay(exe, case, fr, directory)
    bk = CR.back(inp, fr, rp["flags"], rp["ninl"], [model_tuple(m) for m in rp["model"]])
    return fr, rp, bk


def truth_error(case, rp):
    worst = None
    for c, S in enumerate(case.truth):
        if S is not None:
            e = float(np.abs(rp["model"][c] - SC.model_of(S)).max())
            worst = e if worst is None else max(worst, e)
    return worst


def check(case, ev):
    fr, rp, bk = ev
    assert fr["margin"] >= MARGIN and bk["margin"] >= MARGIN and rp["margin"] >= MARGIN, (case.name, fr["margin"], bk["margin"], rp["margin"])
    assert case.checks, case.name
    for f in case.checks:
        f(fr, rp, bk)


def _that(case, fn):
    """a check: fn(front, replay, back) must hold"""
    def f(fr, rp, bk):
        assert fn(fr, rp, bk), case.name
    case.checks.append(f)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
def _expect(case, **want):
    """counts the restatement must reach: n_pairs / n_guided / ninl (lists per candidate), win, n_total, n_proj, n_loop_points, ok"""
    def f(fr, rp, bk):
        got = {"n_pairs": fr["n_pairs"], "n_guided": fr["n_guided"], "ninl": rp["ninl"], "win": bk["win"], "n_total": bk["n_total"], "n_proj": bk["n_proj"],
               "n_loop_points": bk["n_loop_points"], "n_proj_cand": bk["n_proj_cand"], "ok": bk["ok"]}
        for k, v in want.items():
            assert got[k] == v, (case.name, k, got[k], v)
    case.checks.append(f)
    return case


def rows(n_p, n_c=0):
    """one candidate, 3 seeds, 2 guided features, 1 projected, behind padding rows: p has n_p rows, the candidate n_c (0: as many as the
    features need).  n_p = 4, the smallest keyframe the store takes: 3 seeds and 1 guided feature.  Aims at the loops over the rows of p
    and of the candidate, within and past one workgroup."""
    b = Builder("rows:%d/%d" % (n_p, n_c), seed=10 + n_p)
    if n_p == 4:
        b.seeds(0, 3)
        b.feat(0, "guided")
        b.pad(b.cand[0], 5)
        return _expect(b, n_pairs=[4], n_guided=[1], ninl=[4], win=0, n_total=4)
    b.pad(b.p, n_p - 6)   # the features stand in the last rows: past 1024 at n_p = 1025
    b.pad(b.cand[0], max(n_c - 6, 0))
    b.seeds(0, 3)
    g = [b.feat(0, "guided") for _ in range(2)]
    b.feat(0, "free1")
    b.pad(b.cand[0], 4)
    assert len(b.kf[b.p]["xy"]) == n_p and (n_c == 0 or len(b.kf[b.cand[0]]["xy"]) == n_c)
    _expect(b, n_pairs=[5], n_guided=[2], ninl=[5], win=0, n_proj=1, n_total=6)
    _that(b, lambda fr, rp, bk: [fr["fwd"][0][f["i"]] == f["j"] and fr["bwd"][0][f["j"]] == f["i"] for f in g] == [True, True])
    return b


def candidates(n):
    """n candidates of one asking keyframe with 12 shared rows: candidate c keeps 12 - c % 5 of them as seeds and has c % 3 guided
    features of its own.  Candidates 0, 5, 10, 15 keep all 12 and end with 12, 14, 13 and 12 inliers: with 16 candidates the winner is
    candidate 5, not the first.  A candidate's guided features are features no other candidate sees."""
    b = Builder("candidates:%d" % n, n_cand=n, seed=50 + n)
    first = b.seeds(0, 12)
    for c in range(1, n):
        for q, f in enumerate(first):
            if q < 12 - c % 5:
                b.feat(c, "seed", share=f)
    for c in range(n):
        for _ in range(c % 3):
            b.feat(c, "guided")
        b.pad(b.cand[c], 4)
    ninl = [12 - c % 5 + c % 3 for c in range(n)]
    win = max(range(n), key=lambda c: (ninl[c], -c))
    return _expect(b, n_pairs=ninl, n_guided=[c % 3 for c in range(n)], ninl=ninl, win=win)


def tie_on_inliers():
    """two candidates, 8 seeds each: the earlier one wins; a third with 9 seeds listed behind them takes it from both"""
    b = Builder("tie_on_inliers", n_cand=3, seed=70)
    first = b.seeds(0, 8)
    for f in first:
        b.feat(1, "seed", share=f)
        b.feat(2, "seed", share=f)
    b.feat(2, "seed")
    two = Builder("tie_on_inliers:two", n_cand=2, seed=70)
    f2 = two.seeds(0, 8)
    for f in f2:
        two.feat(1, "seed", share=f)
    return [_expect(two, ninl=[8, 8], win=0), _expect(b, ninl=[8, 8, 9], win=2)]


def takes_no_part():
    """candidate 0 has a NaN in its rotation, candidate 2 a scale of 0; candidate 1 is good and wins.  Their seeds and guided features are
    there and would be found"""
    b = Builder("takes_no_part", n_cand=3, seed=80)
    first = b.seeds(0, 6)
    for f in first:
        b.feat(1, "seed", share=f)
        b.feat(2, "seed", share=f)
    for c in range(3):
        b.feat(c, "guided")
    s, R, t = b.models[0]
    R = R.copy(); R[1, 2] = np.nan
    b.models[0] = (s, R, t)
    b.models[2] = (0.0, b.models[2][1], b.models[2][2])
    _expect(b, n_pairs=[0, 7, 0], n_guided=[0, 1, 0], ninl=[0, 7, 0], win=1)
    _that(b, lambda fr, rp, bk: (np.isnan(rp["model"][0]).all() and np.isnan(rp["model"][2]).all() and (fr["fwd"][0] == -1).all()
                                        and (fr["bwd"][2] == -1).all()))
    return b


def null_arguments(which):
    """inlier NULL: the rows flagged 0 count as seeds too; group NULL: the neighbour's points are no loop points"""
    b = Builder("null:%s" % which, seed=90, neighbours=1)
    b.seeds(0, 5)
    b.seeds(0, 2, flag=0)
    b.feat(0, "free1", at=b.nb[0][0])
    if which == "inlier":
        b.inlier_null = True
        return _expect(b, n_pairs=[7], n_guided=[0], n_proj=1, n_total=8)
    if which == "group":
        b.group = None
        # the two unflagged rows are found again by the guided search: their points and rows are all there
        return _expect(b, n_pairs=[7], n_guided=[2], n_proj=0, n_total=7, n_loop_points=7)
    return _expect(b, n_pairs=[7], n_guided=[2], n_proj=1, n_total=8, n_loop_points=8)


def seeds_are_taken():
    """a seed (i, j); a row i' of p whose point projects onto j with j's word at distance 0, and a row j' of the candidate whose point
    projects onto i with i's word: neither may take the seed's rows, and the seed's rows are no sources.  Two listed rows naming one j:
    the lower row is the seed, the other becomes a source of the guided search (its own candidate row is taken: it finds nothing)."""
    b = Builder("seeds_are_taken", seed=100)
    base = b.seeds(0, 4)
    s = base[0]
    i2 = b.row(b.p, proj(s["X1"]) + [1.0, 0.5], CODE[s["word"]])
    a2 = b.point(s["X1"], b.p, [(b.p, i2)])
    b.cur[i2] = a2
    j2 = b.row(b.cand[0], proj(s["X2"]) + [0.5, -1.0], CODE[s["word"]])
    b2 = b.point(s["X2"], b.cand[0], [(b.cand[0], j2)])
    # (i2, j2) are each other's only free partner: a guided match beside the seed
    t = base[1]
    i3 = b.row(b.p, proj(t["X1"]) + [-1.0, 1.0], CODE[t["word"]])
    a3 = b.point(t["X1"], b.p, [(b.p, i3)])
    b.cur[i3] = a3
    b.match[0][i3] = (t["b"], t["j"], 1)   # a second listed row naming t's candidate row

    def f(fr, rp, bk):
        assert fr["seed"][0][s["i"]] and fr["fwd"][0][s["i"]] == -1 and fr["bwd"][0][s["j"]] == -1
        assert fr["fwd"][0][i2] == j2 and fr["bwd"][0][j2] == i2
        assert fr["seed"][0][t["i"]] and not fr["seed"][0][i3] and t["i"] < i3 and fr["fwd"][0][i3] == -1
    b.checks.append(f)
    return _expect(b, n_pairs=[5], n_guided=[1])


def _gate(b, c, i, a, du, dv, word, d2=0, oct2=0):
    """a candidate row (du, dv) off the projection of point a (at row i of p) into the candidate, its point exactly where a is"""
    u, v = b.into_cand(c, a)
    j = b.row(b.cand[c], [u + du, v + dv], flipped(CODE[word], d2), oct2)
    return j


def guided_window():
    """per octave 0 and 3 of the source row (r = 7.5 and 7.5 * 1.2^3), per axis and sign: a candidate row 0.1 % inside the window (found)
    and one 0.1 % outside (not found).  The candidate rows hold no point: only fwd is looked at."""
    b = Builder("guided_window", seed=110)
    b.seeds(0, 3)
    want = []
    for ro in (0, 3):
        r = 7.5 * 1.2 ** ro
        for ax in (0, 1):
            for sg in (-1.0, 1.0):
                for inside in (True, False):
                    f = b.feat(0, "guided", oct1=ro, row2=False)
                    d = sg * r * (0.999 if inside else 1.001)
                    j = _gate(b, 0, f["i"], f["a"], d if ax == 0 else 0.3, d if ax == 1 else -0.2, f["word"], oct2=ro)
                    want.append((f["i"], j if inside else -1))
    _that(b, lambda fr, rp, bk: [int(fr["fwd"][0][i]) for i, _ in want] == [j for _, j in want])
    return b


def guided_octaves():
    """source rows at octave 0 and 3 in one list; candidate rows at the projection with octave ref - 2, ref - 1, ref + 1, ref + 2 (as
    far as octaves go): found at +-1 only"""
    b = Builder("guided_octaves", seed=120)
    b.seeds(0, 3)
    want = []
    for ro, octs in ((0, (1, 2)), (3, (1, 2, 4, 5))):
        for o2 in octs:
            f = b.feat(0, "guided", oct1=ro, row2=False)
            j = _gate(b, 0, f["i"], f["a"], 0.4, 0.2, f["word"], oct2=o2)
            want.append((f["i"], j if abs(o2 - ro) <= 1 else -1))
    _that(b, lambda fr, rp, bk: [int(fr["fwd"][0][i]) for i, _ in want] == [j for _, j in want])
    return b


def guided_image():
    """sources that project just inside and just outside each image border of the candidate (0.5 px), with a candidate row 1 px inside the
    border in the window of both: found from inside (the window is clipped by the border), not from outside.  Candidate rows in the first
    and last grid column and row (x = 0.2, 639.8, y = 0.2, 479.8).  A source whose point lies just behind the candidate's camera (z = -0.05)
    against one just in front (z = 0.05), both with a candidate row on their pixel."""
    b = Builder("guided_image", seed=130)
    b.seeds(0, 3)
    want = []
    S12 = b.sims[0]
    for px_in, px_out, kp in (([0.5, 200.0], [-0.5, 200.0], [0.2, 201.0]), ([639.5, 210.0], [640.5, 210.0], [639.8, 209.0]),
                              ([300.0, 0.5], [300.0, -0.5], [301.0, 0.2]), ([310.0, 479.5], [310.0, 480.5], [309.0, 479.8])):
        for px, inside in ((px_in, True), (px_out, False)):
            w = b.word()
            X2 = cam_point(px, 6.0)
            X1 = SC.sim_apply(S12, X2)
            i = b.row(b.p, [50.0 + 7.0 * len(want), 60.0], CODE[w])   # (where the row of p stands plays no part in fwd)
            a = b.point(X1, b.p, [(b.p, i)])
            b.cur[i] = a
            j = b.row(b.cand[0], kp, CODE[w])
            want.append((i, j if inside else -1))
    for z in (0.05, -0.05):
        w = b.word()
        X2 = np.array([0.001, 0.001, z])
        X1 = SC.sim_apply(S12, X2)
        i = b.row(b.p, [50.0 + 7.0 * len(want), 90.0], CODE[w])
        a = b.point(X1, b.p, [(b.p, i)])
        b.cur[i] = a
        j = b.row(b.cand[0], proj(X2), CODE[w])
        want.append((i, j if z > 0 else -1))
    _that(b, lambda fr, rp, bk: [int(fr["fwd"][0][i]) for i, _ in want] == [j for _, j in want])
    return b


def distances():
    """a Hamming tie between two candidate rows (the lower row wins); distance 50 accepted, 51 refused; fwd and bwd that disagree (the
    candidate row's point prefers another row of p); a = b: one point seen by both rows, found both ways and refused as a pair"""
    b = Builder("distances", seed=140, rigid=True)
    b.seeds(0, 3)
    tie = b.feat(0, "guided", d2=3)
    u, v = b.into_cand(0, tie["a"])
    j_tie = b.row(b.cand[0], [u + 2.0, v + 1.0], near(CODE[tie["word"]], [5, 6, 7]))   # 3 bits too, other bits, a higher row
    f50, f51 = b.feat(0, "guided", d2=50), b.feat(0, "guided", d2=51)
    dis = b.feat(0, "guided", d1=4)
    u, v = b.into_p(0, dis["b"])
    i_other = b.row(b.p, [u + 1.5, v - 1.0], CODE[dis["word"]])   # no point: no source, but the better target
    same = b.feat(0, "guided")
    b.obs[same["a"]].append((b.cand[0], same["j"]))   # a is seen by the candidate's row too, and is the lower point: point_of gives a
    b.pad(b.cand[0], 4)

    def f(fr, rp, bk):
        fw, bw = fr["fwd"][0], fr["bwd"][0]
        assert fw[tie["i"]] == tie["j"] < j_tie
        assert fw[f50["i"]] == f50["j"] and bw[f50["j"]] == f50["i"] and fw[f51["i"]] == -1 and bw[f51["j"]] == -1
        assert fw[dis["i"]] == dis["j"] and bw[dis["j"]] == i_other
        assert fw[same["i"]] == same["j"] and bw[same["j"]] == same["i"] and fr["tab"][b.cand[0]][same["j"]] == same["a"]
        assert same["i"] not in fr["rows"][0].tolist() and dis["i"] not in fr["rows"][0].tolist()
    b.checks.append(f)
    return _expect(b, n_pairs=[5], n_guided=[2])


def _off(S, ds, dw, dt):
    from tests.ba_scene import rot
    return (S["s"] * ds, rot(dw) @ S["R"], S["t"] + np.asarray(dt))


def refit(tag):
    b = Builder("refit:%s" % tag, seed=150 + len(tag), min_inliers=20)
    if tag == "back":
        # 40 noise-free seeds, a start 5 % / 0.05 rad / 0.05 off.  The selection from such a start must still hold three pairs: chi2 is
        # opened for this case, the guided radius too (nothing to find: every row is a seed).
        b.seeds(0, 40)
        b.models[0] = _off(b.sims[0], 1.05, [0.03, -0.03, 0.025], [0.03, -0.03, 0.03])
        b.prm.update(chi2=1.0e5)
        b.truth = [b.sims[0]]
        return _expect(b, n_pairs=[40], ninl=[40], win=0)
    if tag == "guided_raise":
        b.seeds(0, 25)
        for _ in range(15):
            b.feat(0, "guided")
        b.truth = [b.sims[0]]
        b.prm.update(min_inliers=40)   # the seeds alone would not win
        return _expect(b, n_pairs=[40], n_guided=[15], ninl=[40], win=0, n_total=40, ok=True)
    if tag == "guided_outliers":
        b.seeds(0, 25)
        bad = []
        for q in range(6):
            f = b.feat(0, "guided", row2=False)
            # the candidate's keypoint 5 px off the point's projection: inside the window, outside chi2 (25 > 9.21)
            ang = 1.0 + q
            f["j"] = b.row(b.cand[0], proj(f["X2"]) + 5.0 * np.array([np.cos(ang), np.sin(ang)]), CODE[f["word"]])
            f["b"] = b.point(f["X2"], b.cand[0], [(b.cand[0], f["j"])])
            bad.append(f)
        _that(b, lambda fr, rp, bk: not bk["pair_inlier"][0][[f["i"] for f in bad]].any())
        # (their points b stay loop points that nothing found: the projection takes them onto their rows of p, whose keypoints are exact)
        return _expect(b, n_pairs=[31], n_guided=[6], ninl=[25], win=0, n_proj=6, n_total=31)
    n = int(tag)   # n_pairs 2 and 3
    b.prm.update(min_inliers=3)
    b.seeds(0, n - 1)
    b.feat(0, "guided")
    b.pad(b.p, 4); b.pad(b.cand[0], 4)
    if n == 2:
        _that(b, lambda fr, rp, bk: np.array_equal(rp["model"][0], SC.model_of(b.sims[0])))
        return _expect(b, n_pairs=[2], n_guided=[1], ninl=[0], win=-1, n_total=0)
    return _expect(b, n_pairs=[3], n_guided=[1], ninl=[3], win=0, n_total=3)


def min_inliers(at):
    """10 final inliers against min_inliers 10 (a winner) and 11 (none)"""
    b = Builder("min_inliers:%d" % at, seed=170, min_inliers=at)
    b.seeds(0, 8)
    b.feat(0, "guided"); b.feat(0, "guided")
    return _expect(b, ninl=[10], win=0 if at <= 10 else -1, n_total=10 if at <= 10 else 0)


def loop_points(n):
    """n points the group's neighbour observes and the candidate does not; 3 seeds.  n = 0: an all-zero group.  Every fifth of them has a
    free row of p on its projection with its word (found); the others project onto nothing that resembles them.  Aims at the grid of
    k_cf_proj (65, 1100: more than one block) and at its counters."""
    b = Builder("loop_points:%d" % n, seed=180 + n, neighbours=1)
    b.seeds(0, 3)
    if n == 0:
        b.group = np.zeros((1, b.n_kf()), np.uint8)
        b.feat(0, "free1")
        return _expect(b, n_loop_points=0, n_proj_cand=0, n_proj=0, n_total=3, win=0)
    b.group = np.zeros((1, b.n_kf()), np.uint8)
    b.group[0, b.nb[0][0]] = 1   # the neighbour alone: the seeds' points are no loop points
    hit = 0
    for q in range(n):
        if q % 5 == 0:
            b.feat(0, "free1", at=b.nb[0][0])
            hit += 1
        else:
            b.feat(0, "none", at=b.nb[0][0], word=ABSENT - 1)
    b.pad(b.nb[0][0], 4); b.pad(b.cand[0], 4)
    return _expect(b, n_loop_points=n, n_proj_cand=n, n_proj=hit, n_total=3 + hit, win=0)


def projection_rules():
    """a loop point already found by the refit is skipped; a loop point observed at p is skipped (its row at p is free and resembles it);
    a row that has a loop_point is not claimable (another loop point resembles it and projects onto it); a claim tie on the distance:
    the lower point wins; two points wanting one row at different distances: the loser gets nothing, although a second row resembles
    it further off; the neighbour's points are found."""
    b = Builder("projection_rules", seed=200, neighbours=1)
    nbp = b.nb[0][0]
    base = b.seeds(0, 4)
    s = base[0]
    # a second loop point on the seed's place with the seed row's word: the seed's row of p has a loop_point already
    x_dup = b.point(s["X2"], b.cand[0], [(nbp, b.row(nbp, [100.0, 100.0], CODE[s["word"]]))])
    # observed at p: the point has a row of p among its observations; a free row of p resembles it on its projection
    w = b.word()
    X2 = b.draw(0)
    X1 = SC.sim_apply(b.sims[0], X2)
    i_free = b.row(b.p, proj(X1), CODE[w])
    i_own = b.row(b.p, [20.0, 20.0], CODE[ABSENT])
    x_at_p = b.point(X2, b.cand[0], [(nbp, b.row(nbp, [120.0, 100.0], CODE[w])), (b.p, i_own)])
    # tie: two loop points on one place with the same word, one free row
    t = b.feat(0, "free1", at=nbp)
    x_tie = b.point(t["X2"], b.cand[0], [(nbp, b.row(nbp, [140.0, 100.0], CODE[t["word"]]))])
    # two points wanting one row: the second is 2 bits off and has another row 6 px away that is 2 bits off as well
    l = b.feat(0, "free1", at=nbp)
    x_lose = b.point(l["X2"], b.cand[0], [(nbp, b.row(nbp, [160.0, 100.0], flipped(CODE[l["word"]], 2)))])
    i_far = b.row(b.p, proj(l["X1"]) + [6.0, 0.0], flipped(CODE[l["word"]], 4))
    # the neighbour's own point
    nb_f = b.feat(0, "free1", at=nbp)
    b.pad(b.cand[0], 4)

    def f(fr, rp, bk):
        lp, src = bk["loop_point"], bk["source"]
        assert lp[s["i"]] == s["b"] and src[s["i"]] == 1 and x_dup not in lp.tolist()
        assert lp[i_free] == -1 and lp[i_own] == -1 and x_at_p not in lp.tolist()
        assert lp[t["i"]] == t["b"] < x_tie and src[t["i"]] == 3
        assert lp[l["i"]] == l["b"] and lp[i_far] == -1 and x_lose not in lp.tolist()
        assert lp[nb_f["i"]] == nb_f["b"] and src[nb_f["i"]] == 3
    b.checks.append(f)
    # loop points: 4 seeds' b, x_dup, x_at_p, t.b, x_tie, l.b, x_lose, nb_f.b = 11; candidates: all but the 4 found and x_at_p = 6
    return _expect(b, n_loop_points=11, n_proj_cand=6, n_proj=3, n_total=7, win=0)


def total(n):
    """20 seeds, 10 guided, n - 30 projected: n loop points in all against min_matches 40"""
    b = Builder("total:%d" % n, seed=220, neighbours=1)
    b.seeds(0, 20)
    for _ in range(10):
        b.feat(0, "guided")
    for _ in range(n - 30):
        b.feat(0, "free1", at=b.nb[0][0])
    b.truth = [b.sims[0]]
    return _expect(b, n_pairs=[30], ninl=[30], n_proj=n - 30, n_total=n, ok=n >= 40, win=0)


def stale_observations():
    """the observation lists of the loop points (and of a seed's points) carry entries that name nothing - a position past the map, one
    before its start, a row past the keyframe, a row before its start - in front of the valid one: the representative and every rule
    read the valid entry alone.  A point whose entries all name nothing is no loop point."""
    b = Builder("stale_observations", seed=230, neighbours=1)
    nbp = b.nb[0][0]
    base = b.seeds(0, 4)
    fs = [b.feat(0, "free1", at=nbp) for _ in range(4)] + [b.feat(0, "guided")]
    b.pad(nbp, 4)
    n_kf = b.n_kf()
    junk = [(n_kf + 3, 0), (-n_kf - 2, 1), (b.p, 4000), (b.cand[0], -300)]   # (the third would be an observation at p, were its row one)
    for q, f in enumerate(fs):
        b.obs[f["b"]].insert(0, junk[q % 4])
    b.obs[base[0]["a"]].insert(0, junk[0]); b.obs[base[1]["b"]].insert(0, junk[1])
    ghost = b.point(fs[0]["X2"], b.cand[0], [junk[0], junk[2]])
    _that(b, lambda fr, rp, bk: (ghost not in bk["loop_point"].tolist() and fr["ref"][ghost] is None))
    return _expect(b, n_pairs=[5], n_guided=[1], ninl=[5], n_proj=4, n_total=9, n_loop_points=9, win=0)


FAMILIES = {"rows", "candidates", "tie_on_inliers", "takes_no_part", "null", "seeds_are_taken", "guided_window", "guided_octaves", "guided_image",
            "distances", "refit", "min_inliers", "loop_points", "projection_rules", "total", "stale_observations"}
_CASES = []


def all_cases():
    if not _CASES:
        cs = [rows(4), rows(63), rows(64), rows(65), rows(1025), rows(70, 1025), candidates(1), candidates(16)] + tie_on_inliers()
        cs += [takes_no_part(), null_arguments("inlier"), null_arguments("group"), null_arguments("none"), seeds_are_taken(), guided_window(),
               guided_octaves(), guided_image(), distances()]
        cs += [refit(t) for t in ("back", "guided_raise", "guided_outliers", "2", "3")] + [min_inliers(10), min_inliers(11)]
        cs += [loop_points(n) for n in (0, 1, 65, 1100)] + [projection_rules(), total(39), total(40), stale_observations()]
        assert len({c.name for c in cs}) == len(cs)
        _CASES.extend(cs)
    return _CASES
