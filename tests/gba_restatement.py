"""numpy restatement of LocalMapper.global_bundle_adjust (mo_map_global_ba in include/vslam_amd.h), on arrays.  It restates the rules, not
the kernels: whole-array numpy in f64, the reduced camera system ASSEMBLED (block-sparse sums over the edge pairs of every point) and
solved by numpy's dense Cholesky, where the library never forms it and iterates.  A wrong matrix-free operator cannot hide here.
The edge reading, the cost, the pose update and the information are tests/ba_restatement.py's; its dense lm_step is the cross-check of
sparse_step on problems small enough for it (tests/test_gba_cpu.py)."""
import numpy as np

from tests.ba_restatement import _classify, _cost, _residuals, info_of, lm_step, pose_update, valid_edges  # noqa: F401  (lm_step: re-exported)


def problem(obs_off, obs_kf, obs_kp, counts, fixed=None):
    """(problem-point mask, free positions, fixed positions, per-point valid edges); ValueError when the problem has points and no fixed
    position takes part"""
    n_kf = len(counts)
    edges = valid_edges(obs_off, obs_kf, obs_kp, counts)
    prob = np.array([len(v) >= 2 for v in edges], bool)
    seen = sorted(set(k for v, l in zip(edges, prob) if l for k, _, _ in v))
    held = {0} if fixed is None else set(int(k) for k in fixed if 0 <= int(k) < n_kf)
    fix = [p for p in seen if p in held]
    free = [p for p in seen if p not in held]
    if prob.any() and not fix:
        raise ValueError("no fixed position takes part in the problem")
    return prob, free, fix, edges


def sparse_step(K, T, X, E, fidx, n_free, h2, lam):
    """one damped step from (T, X) over all edges: (delta_c [6 n_free] or None when the reduced system is not positive definite,
    delta_p [n_points][3]); the reduced system assembled from the pairs of edges of every point"""
    ek, ep = E["kf"], E["pt"]
    e, _, fin, Xc, p, R = _residuals(K, T, X, ek, ep, E["xy"])
    ek, ep, e, Xc, p, R, info = ek[fin], ep[fin], e[fin], Xc[fin], p[fin], R[fin], E["info"][fin]
    n, nl = len(ek), len(X)
    e2 = info * (e ** 2).sum(axis=1)
    w = info * (np.where(e2 > h2, np.sqrt(h2) / np.sqrt(np.where(e2 > 0, e2, 1.0)), 1.0) if h2 > 0 else 1.0)
    D = np.empty((n, 2, 3))
    for r in range(2):
        D[:, r, :] = (K[r][None, :] * p[:, 2:3] - p[:, r:r + 1] * K[2][None, :]) / (p[:, 2:3] ** 2)
    skew = np.zeros((n, 3, 3))
    skew[:, 0, 1], skew[:, 0, 2], skew[:, 1, 0], skew[:, 1, 2], skew[:, 2, 0], skew[:, 2, 1] = -Xc[:, 2], Xc[:, 1], Xc[:, 2], -Xc[:, 0], -Xc[:, 1], Xc[:, 0]
    Jc = np.concatenate([D, -np.einsum("nij,njk->nik", D, skew)], axis=2)
    Jp = np.einsum("nij,njk->nik", D, R)
    V = np.zeros((nl, 3, 3)); gp = np.zeros((nl, 3))
    np.add.at(V, ep, w[:, None, None] * np.einsum("nki,nkj->nij", Jp, Jp))
    np.add.at(gp, ep, w[:, None] * np.einsum("nki,nk->ni", Jp, e))
    V[:, [0, 1, 2], [0, 1, 2]] *= 1.0 + lam
    with np.errstate(all="ignore"):
        p0 = V[:, 0, 0]
        l10, l20 = V[:, 1, 0] / np.sqrt(p0), V[:, 2, 0] / np.sqrt(p0)
        p1 = V[:, 1, 1] - l10 ** 2
        l21 = (V[:, 2, 1] - l20 * l10) / np.sqrt(p1)
        p2 = V[:, 2, 2] - l20 ** 2 - l21 ** 2
        ok = (p0 > 0) & (p1 > 0) & (p2 > 0) & np.isfinite(p0) & np.isfinite(p1) & np.isfinite(p2)
    Vi = np.zeros((nl, 3, 3))
    Vi[ok] = np.linalg.inv(V[ok])          # (a point whose V is not positive definite is held: its V^-1 is 0 in every term below)
    f = fidx[ek]
    fr = np.flatnonzero(f >= 0)
    ff, pf = f[fr], ep[fr]
    H = np.zeros((n_free, 6, 6)); g = np.zeros((n_free, 6))
    np.add.at(H, ff, w[fr, None, None] * np.einsum("nki,nkj->nij", Jc[fr], Jc[fr]))
    np.add.at(g, ff, w[fr, None] * np.einsum("nki,nk->ni", Jc[fr], e[fr]))
    Wm = w[fr, None, None] * np.einsum("nki,nkj->nij", Jc[fr], Jp[fr])      # [free edge][6][3]
    WV = np.einsum("nik,nkl->nil", Wm, Vi[pf])
    S4 = np.zeros((n_free, n_free, 6, 6))
    for i in range(n_free):
        S4[i, i] = H[i] + lam * np.diag(np.diag(H[i]))
    # every ordered pair (a, b) of free edges of one point (the edges are in point order)
    cnt = np.bincount(pf, minlength=nl)
    first = np.cumsum(cnt) - cnt
    rep = cnt[pf]
    A = np.repeat(np.arange(len(fr)), rep)
    B = np.repeat(first[pf], rep) + (np.arange(rep.sum()) - np.repeat(np.cumsum(rep) - rep, rep))
    np.subtract.at(S4, (ff[A], ff[B]), np.einsum("nil,njl->nij", WV[A], Wm[B]))
    d = 6 * n_free
    S = S4.transpose(0, 2, 1, 3).reshape(d, d)
    b = g.copy()
    np.subtract.at(b, ff, np.einsum("nil,nl->ni", WV, gp[pf]))
    b = b.reshape(d)
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return None, None
    if not np.isfinite(L).all():
        return None, None
    dc = np.linalg.solve(L.T, np.linalg.solve(L, b))
    t = gp.copy()
    np.subtract.at(t, pf, np.einsum("nil,ni->nl", Wm, dc.reshape(n_free, 6)[ff]))
    dp = np.einsum("pkl,pl->pk", Vi, t)
    return dc, dp


def global_bundle_adjust(obs_off, obs_kf, obs_kp, counts, kf_xy, kf_oct, xyz, K, poses, fixed=None, max_steps=10, step_tol=1e-10, min_inliers=50,
                         scale_factor=1.2, chi2=5.991, trace=None):
    """kf_xy [position] -> [rows][2] f32 keypoints, kf_oct [position] -> octaves, xyz [n][3] f32, poses [n_kf][3][4].  Returns the dict
    LocalMapper.global_bundle_adjust's info holds (plus ok, kf_state, and xyz: the f32 positions after the call).  trace: a list that
    receives (cost before, cost of the trial, largest update) of every step."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    n_kf, n_pts, n_obs = len(counts), len(obs_off) - 1, int(obs_off[-1]) if len(obs_off) else 0
    poses = np.array(poses, np.float64).reshape(n_kf, 3, 4)
    out = {"ok": False, "n_free": 0, "n_fixed": 0, "n_points": 0, "n_edges": 0, "n_inliers": 0, "cost": [0.0, 0.0], "steps": 0, "accepted": 0,
           "free": [], "fixed": [], "kf_state": np.zeros(n_kf, np.int32), "edge_inlier": np.zeros(n_obs, np.uint8), "poses": poses.copy(),
           "points": np.full((n_pts, 3), np.nan), "xyz": np.array(xyz, np.float32).reshape(n_pts, 3).copy()}
    if n_kf == 0 or n_pts == 0 or max_steps == 0:
        return out
    prob, free, fix, edges = problem(obs_off, obs_kf, obs_kp, counts, fixed)
    if not free or not prob.any():
        return out
    lpt = np.flatnonzero(prob)
    E = {"pt": [], "kf": [], "obs": [], "xy": [], "info": []}
    for r, i in enumerate(lpt):
        for k, row, o in edges[i]:
            E["pt"].append(r); E["kf"].append(k); E["obs"].append(o)
            E["xy"].append(np.asarray(kf_xy[k][row], np.float64)); E["info"].append(info_of(scale_factor, kf_oct[k][row]))
    E = {"pt": np.array(E["pt"]), "kf": np.array(E["kf"]), "obs": np.array(E["obs"]), "xy": np.array(E["xy"]).reshape(-1, 2), "info": np.array(E["info"])}
    fidx = np.full(n_kf, -1)
    fidx[free] = np.arange(len(free))
    T, X = poses.copy(), out["xyz"][lpt].astype(np.float64)
    n_e = len(E["pt"])
    use = np.ones(n_e, bool)
    out["cost"][0] = _cost(K, T, X, E, use, chi2)
    lam = 1e-4
    for _ in range(max_steps):
        cur = _cost(K, T, X, E, use, chi2)
        dc, dp = sparse_step(K, T, X, E, fidx, len(free), chi2, lam)
        out["steps"] += 1
        if dc is None:          # the library's solve has no such failure; its rejected step is the nearest rule
            lam *= 10.0
            if lam > 1e8:
                break
            continue
        T2 = T.copy()
        for j, pos in enumerate(free):
            T2[pos] = pose_update(dc[6 * j:6 * j + 6], T[pos])
        X2 = X + dp
        trial = _cost(K, T2, X2, E, use, chi2)
        upd = float(max(np.abs(dc).max(), np.abs(dp).max()))
        if trace is not None:
            trace.append((cur, trial, upd))
        if trial < cur:
            T, X = T2, X2
            lam /= 10.0
            out["accepted"] += 1
        else:
            lam *= 10.0
        if upd < step_tol or lam > 1e8:
            break
    inl = _classify(K, T, X, E, chi2)
    out["cost"][1] = _cost(K, T, X, E, use, chi2)
    out["edge_inlier"][E["obs"]] = np.where(inl, 1, 2)
    out["kf_state"][free] = 2
    out["kf_state"][fix] = 1
    out.update(n_free=len(free), n_fixed=len(fix), n_points=len(lpt), n_edges=n_e, n_inliers=int(inl.sum()), free=free, fixed=fix, lam=lam)
    out["poses"] = T
    out["points"][lpt] = X
    if out["accepted"]:
        out["xyz"][lpt] = X.astype(np.float32)
    out["ok"] = out["n_inliers"] >= min_inliers
    return out
