"""numpy restatement of LocalMapper.confirm_loop (mo_map_loop_confirm in include/vslam_amd.h) around its refit: front() gives the
representatives, the seeds, the guided search and the packed pairs; the refit runs in tests/native/confirm_replay.cpp over the device's own
sim3.h; back() takes its flags, counts and models and gives the winner, the loop points of its pairs and the projection of the loop's
local map.  Every f64 expression is formed in the order of the device functions (cf_camera, sim3_inverse, sim3_apply, trk_project,
trk_scale of visual-slam_amd/csrc).  Both halves return the smallest relative margin of any decision that hinges on a float: z > 0 (against the
point's largest coordinate), the image test (against w, h), |dx| < r and |dy| < r (against r; only where the other axis is within 2 r:
elsewhere the axis decides nothing).  The cell walk of trk_window decides nothing of its own: the cells are monotone in the coordinate, so the
cells of [u - r, u + r] hold every keypoint with |dx| < r, and the box test is applied to each of them."""
import numpy as np

from tests.reloc_restatement import hamming
from tests.sim3_cases import info_of
from tests.track_restatement import representatives, valid_observations

INF = float("inf")


def _power(base, o):
    s = 1.0
    for _ in range(max(int(o), 0)):
        s *= base
    return s


def camera(T, x):
    """R x + t of f32 points [n][3], each row summed left to right"""
    x = np.asarray(x, np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64)
    return np.column_stack([T[d, 0] * x[:, 0] + T[d, 1] * x[:, 1] + T[d, 2] * x[:, 2] + T[d, 3] for d in range(3)])


def inverse(S):
    """sim3_inverse on (s, R [3][3], t [3])"""
    s, R, t = S
    i_s = 1.0 / s
    iR = np.array(R, np.float64).T.copy()
    it = np.array([-i_s * (iR[i, 0] * t[0] + iR[i, 1] * t[1] + iR[i, 2] * t[2]) for i in range(3)])
    return i_s, iR, it


def apply(S, X):
    """sim3_apply on points [n][3]"""
    s, R, t = S
    X = np.asarray(X, np.float64).reshape(-1, 3)
    return np.column_stack([s * (R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1] + R[i, 2] * X[:, 2]) + t[i] for i in range(3)])


def project(K, Y, w, h):
    """trk_project under P = [K | 0]: (u, v, in the image, margin)"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    x = K[0, 0] * Y[0] + K[0, 1] * Y[1] + K[0, 2] * Y[2] + 0.0
    y = K[1, 0] * Y[0] + K[1, 1] * Y[1] + K[1, 2] * Y[2] + 0.0
    z = K[2, 0] * Y[0] + K[2, 1] * Y[1] + K[2, 2] * Y[2] + 0.0
    margin = abs(z) / max(np.abs(Y).max(), 1e-300)
    if not z > 0.0:
        return 0.0, 0.0, False, margin
    u, v = x / z, y / z
    margin = min(margin, abs(u) / w, abs(u - w) / w, abs(v) / h, abs(v - h) / h)
    return u, v, bool(u >= 0.0 and u < w and v >= 0.0 and v < h), margin


def window(u, v, r, ro, kx, ky, ko, desc, d, allowed):
    """the best row of one projected-window search: (row or -1, distance, margin).  allowed: bool per row (rows the search may visit)"""
    dx, dy = np.abs(kx - u), np.abs(ky - v)
    near_x, near_y = dy < 2.0 * r, dx < 2.0 * r
    margin = INF
    if near_x.any():
        margin = min(margin, float((np.abs(dx[near_x] - r) / r).min()))
    if near_y.any():
        margin = min(margin, float((np.abs(dy[near_y] - r) / r).min()))
    q = np.flatnonzero((dx < r) & (dy < r) & (np.abs(ko - ro) <= 1) & allowed)
    if len(q) == 0:
        return -1, -1, margin
    dist = hamming(d[None], desc[q])[0]
    o = np.lexsort((q, dist))[0]
    return int(q[o]), int(dist[o]), margin


class Inputs:
    """what the call reads: K [3][3], poses (list of 4x4), kf_xy / kf_oct / kf_desc per position, xyz f32, obs_off / obs_kf / obs_kp as
    stored, p, cand, cur_point, match_point, match_row, inlier (None: all), models (list of (s, R, t)), group (None or [n_cand][n_kf] bool)
    and the parameters"""

    def __init__(self, K, poses, kf_xy, kf_oct, kf_desc, xyz, obs_off, obs_kf, obs_kp, p, cand, cur_point, match_point, match_row, inlier, models,
                 group, w, h, radius_guided=7.5, radius_proj=10.0, max_dist=50, chi2=9.210, scale_factor=1.2, min_inliers=20, min_matches=40):
        self.K, self.poses = np.asarray(K, np.float64).reshape(3, 3), [np.asarray(T, np.float64) for T in poses]
        self.kf_xy = [np.asarray(a, np.float32).reshape(-1, 2) for a in kf_xy]
        self.kf_oct = [np.asarray(a, np.int64).reshape(-1) for a in kf_oct]
        self.kf_desc = [np.asarray(a, np.uint8).reshape(-1, 32) for a in kf_desc]
        self.xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
        self.obs_off, self.obs_kf, self.obs_kp = obs_off, obs_kf, obs_kp
        self.p, self.cand = int(p), [int(k) for k in cand]
        n_p, nc = len(self.kf_xy[self.p]), len(self.cand)
        self.cur_point = np.asarray(cur_point, np.int64).reshape(n_p)
        self.match_point = np.asarray(match_point, np.int64).reshape(nc, n_p)
        self.match_row = np.asarray(match_row, np.int64).reshape(nc, n_p)
        self.inlier = np.ones((nc, n_p), bool) if inlier is None else np.asarray(inlier).reshape(nc, n_p) != 0
        self.models = [(float(s), np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)) for s, R, t in models]
        n_kf = len(self.poses)
        if group is None:
            group = np.zeros((nc, n_kf), bool)
            for c, k in enumerate(self.cand):
                group[c, k] = True
        self.group = np.asarray(group).reshape(nc, n_kf) != 0
        self.w, self.h = int(w), int(h)
        self.radius_guided, self.radius_proj, self.max_dist = float(radius_guided), float(radius_proj), int(max_dist)
        self.chi2, self.sf, self.min_inliers, self.min_matches = float(chi2), float(scale_factor), int(min_inliers), int(min_matches)


def front(inp):
    """rules 1 - 3 and the packing of rule 4: dict with part [n_cand], rep, ref, obs, tab (point_of per position, -1: none), seed [n_cand][n_p] bool,
    fwd [n_cand][n_p], bwd [n_cand][R2], per candidate rows, pairs [m][12], kind [m], b [m]; n_pairs, n_guided; margin"""
    n_kf, n_pts, nc = len(inp.poses), len(inp.xyz), len(inp.cand)
    counts = [len(a) for a in inp.kf_xy]
    n_p = counts[inp.p]
    obs = valid_observations(inp.obs_off, inp.obs_kf, inp.obs_kp, counts)
    in_L = np.zeros(n_kf, bool)
    in_L[inp.p] = True
    for c, k in enumerate(inp.cand):
        in_L[k] = True
        in_L |= inp.group[c]
    local = np.array([any(in_L[k] for k, _ in v) for v in obs], bool)
    rep, ref = representatives(obs, inp.kf_desc, inp.kf_oct, local)
    tab = [np.full(n, -1, np.int64) for n in counts]
    for i in range(n_pts - 1, -1, -1):   # the lowest point keeps a row
        for k, r in obs[i]:
            tab[k][r] = i
    r2 = max([counts[k] for k in inp.cand] + [1])
    part = [bool(np.isfinite(s) and np.isfinite(R).all() and np.isfinite(t).all() and s > 0) for s, R, t in inp.models]
    seed = np.zeros((nc, n_p), bool)
    fwd, bwd = np.full((nc, n_p), -1, np.int64), np.full((nc, r2), -1, np.int64)
    out = {"part": part, "rep": rep, "ref": ref, "obs": obs, "tab": tab, "seed": seed, "fwd": fwd, "bwd": bwd, "rows": [], "pairs": [], "kind": [],
           "b": [], "n_pairs": [], "n_guided": []}
    margin = INF
    T1 = inp.poses[inp.p]
    kx1, ky1, ko1 = inp.kf_xy[inp.p][:, 0].astype(np.float64), inp.kf_xy[inp.p][:, 1].astype(np.float64), inp.kf_oct[inp.p]
    for c, k in enumerate(inp.cand):
        n2, T2 = counts[k], inp.poses[k]
        a, b, j = inp.cur_point, inp.match_point[c], inp.match_row[c]
        taken2 = np.zeros(n2, bool)
        if part[c]:
            listed = (a >= 0) & (a < n_pts) & (b >= 0) & (b < n_pts) & (j >= 0) & (j < n2) & inp.inlier[c]
            for i in np.flatnonzero(listed):   # ascending: the lowest row keeps a candidate row
                if not taken2[j[i]]:
                    taken2[j[i]] = True
                    seed[c, i] = True
            S12 = inp.models[c]
            S21 = inverse(S12)
            kx2, ky2, ko2 = inp.kf_xy[k][:, 0].astype(np.float64), inp.kf_xy[k][:, 1].astype(np.float64), inp.kf_oct[k]
            for i in range(n_p):
                if seed[c, i] or not 0 <= a[i] < n_pts or ref[a[i]] is None:
                    continue
                Y = apply(S21, camera(T1, inp.xyz[a[i]]))[0]
                u, v, ok, mg = project(inp.K, Y, inp.w, inp.h)
                margin = min(margin, mg)
                if ok:
                    q, d, mg = window(u, v, inp.radius_guided * _power(inp.sf, ref[a[i]]), ref[a[i]], kx2, ky2, ko2, inp.kf_desc[k], rep[a[i]], ~taken2)
                    margin = min(margin, mg)
                    if q >= 0 and d <= inp.max_dist:
                        fwd[c, i] = q
            for jj in range(n2):
                bb = tab[k][jj]
                if taken2[jj] or bb < 0 or ref[bb] is None:
                    continue
                Y = apply(S12, camera(T2, inp.xyz[bb]))[0]
                u, v, ok, mg = project(inp.K, Y, inp.w, inp.h)
                margin = min(margin, mg)
                if ok:
                    q, d, mg = window(u, v, inp.radius_guided * _power(inp.sf, ref[bb]), ref[bb], kx1, ky1, ko1, inp.kf_desc[inp.p], rep[bb], ~seed[c])
                    margin = min(margin, mg)
                    if q >= 0 and d <= inp.max_dist:
                        bwd[c, jj] = q
        rows, kind, bs, js = [], [], [], []
        for i in range(n_p):
            if seed[c, i]:
                rows.append(i); kind.append(1); bs.append(int(b[i])); js.append(int(j[i]))
            elif part[c] and fwd[c, i] >= 0 and bwd[c, fwd[c, i]] == i and tab[k][fwd[c, i]] != a[i]:
                rows.append(i); kind.append(2); bs.append(int(tab[k][fwd[c, i]])); js.append(int(fwd[c, i]))
        rows, js = np.array(rows, np.int64), np.array(js, np.int64)
        pr = np.zeros((len(rows), 12))
        if len(rows):
            pr[:, 0:3] = camera(T1, inp.xyz[a[rows]])
            pr[:, 3:6] = camera(T2, inp.xyz[np.array(bs)])
            pr[:, 6:8] = inp.kf_xy[inp.p][rows].astype(np.float64)
            pr[:, 8] = [info_of(inp.sf, o) for o in inp.kf_oct[inp.p][rows]]
            pr[:, 9:11] = inp.kf_xy[k][js].astype(np.float64)
            pr[:, 11] = [info_of(inp.sf, o) for o in inp.kf_oct[k][js]]
        out["rows"].append(rows); out["pairs"].append(pr); out["kind"].append(np.array(kind, np.uint8)); out["b"].append(np.array(bs, np.int64))
        out["n_pairs"].append(len(rows)); out["n_guided"].append(int((np.array(kind) == 2).sum()))
    out["margin"] = margin
    return out


def back(inp, fr, flags, n_inliers, models):
    """rules 5 - 7 from the refit's results (flags per candidate [m] bool, n_inliers, models (s, R, t) per candidate): dict with win, ok,
    loop_point, source, pair_inlier [n_cand][n_p], n_loop_points, n_proj_cand, n_proj, n_total, margin"""
    nc, n_p, n_pts = len(inp.cand), len(inp.kf_xy[inp.p]), len(inp.xyz)
    win = -1
    for c in range(nc):
        if fr["part"][c] and n_inliers[c] >= inp.min_inliers and (win < 0 or n_inliers[c] > n_inliers[win]):
            win = c
    lpt, src = np.full(n_p, -1, np.int64), np.zeros(n_p, np.uint8)
    pin = np.zeros((nc, n_p), bool)
    for c in range(nc):
        pin[c, fr["rows"][c][np.asarray(flags[c], bool)]] = True
    out = {"win": win, "ok": False, "loop_point": lpt, "source": src, "pair_inlier": pin, "n_loop_points": 0, "n_proj_cand": 0, "n_proj": 0,
           "n_total": 0, "margin": INF}
    if win < 0:
        return out
    f = np.asarray(flags[win], bool)
    lpt[fr["rows"][win][f]] = fr["b"][win][f]
    src[fr["rows"][win][f]] = fr["kind"][win][f]
    found = set(fr["b"][win][f].tolist())
    k, S12, T2 = inp.cand[win], models[win], inp.poses[inp.cand[win]]
    kx, ky, ko = inp.kf_xy[inp.p][:, 0].astype(np.float64), inp.kf_xy[inp.p][:, 1].astype(np.float64), inp.kf_oct[inp.p]
    free = lpt < 0
    claim = {}
    for x in range(n_pts):
        v = fr["obs"][x]
        if not any(inp.group[win][kk] for kk, _ in v):
            continue
        out["n_loop_points"] += 1
        if x in found or any(kk == inp.p for kk, _ in v):
            continue
        Y = apply(S12, camera(T2, inp.xyz[x]))[0]
        u, vv, ok, mg = project(inp.K, Y, inp.w, inp.h)
        out["margin"] = min(out["margin"], mg)
        if not ok:
            continue
        out["n_proj_cand"] += 1
        q, d, mg = window(u, vv, inp.radius_proj * _power(inp.sf, fr["ref"][x]), fr["ref"][x], kx, ky, ko, inp.kf_desc[inp.p], fr["rep"][x], free)
        out["margin"] = min(out["margin"], mg)
        if q >= 0 and d <= inp.max_dist and (q not in claim or (d, x) < claim[q]):
            claim[q] = (d, x)
    for q, (d, x) in claim.items():
        lpt[q] = x
        src[q] = 3
    out["n_proj"] = len(claim)
    out["n_total"] = int((lpt >= 0).sum())
    out["ok"] = out["n_total"] >= inp.min_matches
    return out
