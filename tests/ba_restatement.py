"""numpy restatement of LocalMapper.bundle_adjust (mo_map_bundle_adjust in include/vslam_amd.h) and of LocalMapper.add_observations
(mo_map_add_observations), on arrays.  It restates the rules, not the kernels: whole-array numpy in f64, the Schur complement as batched
matrix products, numpy's Cholesky for the reduced system."""
import numpy as np


def valid_edges(obs_off, obs_kf, obs_kp, counts):
    """per point: [(keyframe position, row, entry)] of its valid observations in insertion order (negative values count from the end,
    entries naming nothing skipped)"""
    n_kf = len(counts)
    out = []
    for i in range(len(obs_off) - 1):
        v = []
        for o in range(int(obs_off[i]), int(obs_off[i + 1])):
            k = int(obs_kf[o])
            if k < 0:
                k += n_kf
            if not 0 <= k < n_kf:
                continue
            r = int(obs_kp[o])
            if r < 0:
                r += int(counts[k])
            if not 0 <= r < counts[k]:
                continue
            v.append((k, r, o))
        out.append(v)
    return out


def problem(obs_off, obs_kf, obs_kp, counts, window):
    """(local mask, free positions, fixed positions, per-point valid edges).  ValueError for more than 16 candidate positions."""
    n_kf = len(counts)
    lo = n_kf - window if 0 < window < n_kf else 0
    first = max(lo, 1)
    if n_kf - first > 16:
        raise ValueError("more than 16 free keyframes")
    edges = valid_edges(obs_off, obs_kf, obs_kp, counts)
    local = np.array([len(v) >= 2 and any(k >= first for k, _, _ in v) for v in edges], bool)
    seen = set(k for v, l in zip(edges, local) if l for k, _, _ in v)
    fixed = [p for p in range(min(first, n_kf)) if p in seen]
    free = []
    for p in range(first, n_kf):
        if p not in seen:
            continue
        if len(fixed) < 2:
            fixed.append(p)     # the gauge: two fixed poses pin position, orientation and scale
        else:
            free.append(p)
    return local, free, fixed, edges


def info_of(sf, octave):
    s = 1.0
    for _ in range(max(int(octave), 0)):
        s *= sf * sf
    return 1.0 / s


def _exp_so3(w):
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-8:
        a, b = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
    return np.eye(3) + a * W + b * (W @ W)


def pose_update(d, T):
    """exp(d) T for d = (rho, w): R' = exp(w) R, t' = exp(w) t + rho"""
    E = _exp_so3(d[3:])
    T2 = np.empty((3, 4))
    T2[:, :3] = E @ T[:, :3]
    T2[:, 3] = E @ T[:, 3] + d[:3]
    return T2


def _residuals(K, T, X, ek, ep, exy):
    """e = keypoint - projection [n][2], depth [n], finite mask, camera point, p = K X_cam"""
    R, t = T[ek, :, :3], T[ek, :, 3]
    Xc = np.einsum("nij,nj->ni", R, X[ep]) + t
    p = Xc @ K.T
    with np.errstate(all="ignore"):
        proj = p[:, :2] / p[:, 2:3]
        e = exy - proj
    fin = (p[:, 2] != 0) & np.isfinite(e).all(axis=1)
    return e, Xc[:, 2], fin, Xc, p, R


def _rho(e2, h2):
    if h2 > 0:
        with np.errstate(invalid="ignore"):
            return np.where(e2 > h2, 2.0 * np.sqrt(h2) * np.sqrt(e2) - h2, e2)
    return e2


def _cost(K, T, X, E, use, h2):
    e, _, fin, _, _, _ = _residuals(K, T, X, E["kf"], E["pt"], E["xy"])
    m = use & fin
    e2 = E["info"][m] * (e[m] ** 2).sum(axis=1)
    return float(_rho(e2, h2).sum())


def _classify(K, T, X, E, chi2):
    e, z, fin, _, _, _ = _residuals(K, T, X, E["kf"], E["pt"], E["xy"])
    with np.errstate(invalid="ignore"):
        e2 = E["info"] * (e ** 2).sum(axis=1)
        return fin & (z > 0) & (e2 <= chi2)


def lm_step(K, T, X, E, use, fidx, n_free, h2, lam):
    """one damped step from (T, X): (delta_c [6 n_free] or None when the reduced system is not positive definite, delta_p [n_local][3])"""
    ek, ep = E["kf"][use], E["pt"][use]
    e, _, fin, Xc, p, R = _residuals(K, T, X, ek, ep, E["xy"][use])
    ek, ep, e, Xc, p, R, info = ek[fin], ep[fin], e[fin], Xc[fin], p[fin], R[fin], E["info"][use][fin]
    n, nl = len(ek), len(X)
    e2 = info * (e ** 2).sum(axis=1)
    w = info * (np.where(e2 > h2, np.sqrt(h2) / np.sqrt(np.where(e2 > 0, e2, 1.0)), 1.0) if h2 > 0 else 1.0)
    # d (u, v) / d X_cam
    D = np.empty((n, 2, 3))
    for r in range(2):
        D[:, r, :] = (K[r][None, :] * p[:, 2:3] - p[:, r:r + 1] * K[2][None, :]) / (p[:, 2:3] ** 2)
    skew = np.zeros((n, 3, 3))
    skew[:, 0, 1], skew[:, 0, 2], skew[:, 1, 0], skew[:, 1, 2], skew[:, 2, 0], skew[:, 2, 1] = -Xc[:, 2], Xc[:, 1], Xc[:, 2], -Xc[:, 0], -Xc[:, 1], Xc[:, 0]
    Jc = np.concatenate([D, -np.einsum("nij,njk->nik", D, skew)], axis=2)   # [n][2][6]
    Jp = np.einsum("nij,njk->nik", D, R)                                       # [n][2][3]
    V = np.zeros((nl, 3, 3)); gp = np.zeros((nl, 3))
    np.add.at(V, ep, w[:, None, None] * np.einsum("nki,nkj->nij", Jp, Jp))
    np.add.at(gp, ep, w[:, None] * np.einsum("nki,nk->ni", Jp, e))
    V[:, [0, 1, 2], [0, 1, 2]] *= 1.0 + lam
    # positive definite: the three Cholesky pivots
    with np.errstate(all="ignore"):
        p0 = V[:, 0, 0]
        l10, l20 = V[:, 1, 0] / np.sqrt(p0), V[:, 2, 0] / np.sqrt(p0)
        p1 = V[:, 1, 1] - l10 ** 2
        l21 = (V[:, 2, 1] - l20 * l10) / np.sqrt(p1)
        p2 = V[:, 2, 2] - l20 ** 2 - l21 ** 2
        ok = (p0 > 0) & (p1 > 0) & (p2 > 0) & np.isfinite(p0) & np.isfinite(p1) & np.isfinite(p2)
    Vi = np.zeros((nl, 3, 3))
    Vi[ok] = np.linalg.inv(V[ok])
    f = fidx[ek]
    fr = f >= 0
    d = 6 * n_free
    H = np.zeros((n_free, 6, 6)); g = np.zeros((n_free, 6))
    np.add.at(H, f[fr], w[fr, None, None] * np.einsum("nki,nkj->nij", Jc[fr], Jc[fr]))
    np.add.at(g, f[fr], w[fr, None] * np.einsum("nki,nk->ni", Jc[fr], e[fr]))
    Wf = np.zeros((nl, n_free, 6, 3))
    np.add.at(Wf, (ep[fr], f[fr]), w[fr, None, None] * np.einsum("nki,nkj->nij", Jc[fr], Jp[fr]))
    Wf = Wf.reshape(nl, d, 3)
    S = np.zeros((d, d))
    for i in range(n_free):
        S[6 * i:6 * i + 6, 6 * i:6 * i + 6] = H[i] + lam * np.diag(np.diag(H[i]))
    WV = np.einsum("pik,pkl->pil", Wf, Vi)
    S -= np.einsum("pil,pjl->ij", WV, Wf)
    b = g.reshape(d) - np.einsum("pil,pl->i", WV, gp)
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return None, None
    if not np.isfinite(L).all():
        return None, None
    dc = np.linalg.solve(L.T, np.linalg.solve(L, b))
    dp = np.einsum("pkl,pl->pk", Vi, gp - np.einsum("pil,i->pl", Wf, dc))
    return dc, dp


def bundle_adjust(obs_off, obs_kf, obs_kp, counts, kf_xy, kf_oct, xyz, K, poses, window=10, scale_factor=1.2, chi2=5.991, min_inliers=50,
                  max_steps=(5, 10), trace=None):
    """kf_xy [position] -> [rows][2] f32 keypoints, kf_oct [position] -> octaves, xyz [n][3] f32, poses [n_kf][3][4].  Returns the dict
    LocalMapper.bundle_adjust's info holds (plus ok, xyz: the f32 positions after the call).  trace: a list that receives (round, cost
    before, cost of the trial, largest update) of every step, for tests that must know how close a decision was."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    n_kf, n_pts, n_obs = len(counts), len(obs_off) - 1, int(obs_off[-1]) if len(obs_off) else 0
    poses = np.array(poses, np.float64).reshape(n_kf, 3, 4)
    out = {"ok": False, "n_free": 0, "n_fixed": 0, "n_local": 0, "n_edges": 0, "n_inliers": 0, "cost": [0.0, 0.0, 0.0], "steps": [0, 0],
           "accepted": [0, 0], "free": [], "fixed": [], "edge_inlier": np.zeros(n_obs, np.uint8), "poses": poses.copy(),
           "points": np.full((n_pts, 3), np.nan), "xyz": np.array(xyz, np.float32).reshape(n_pts, 3).copy()}
    local, free, fixed, edges = problem(obs_off, obs_kf, obs_kp, counts, window)
    if n_kf == 0 or n_pts == 0 or not free or not local.any():
        return out
    lpt = np.flatnonzero(local)
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
    for rnd in range(2):
        h2 = chi2 if rnd == 0 else 0.0
        lam = 1e-4
        for _ in range(max_steps[rnd]):
            cur = _cost(K, T, X, E, use, h2)
            dc, dp = lm_step(K, T, X, E, use, fidx, len(free), h2, lam)
            if dc is None:
                break
            T2 = T.copy()
            for j, pos in enumerate(free):
                T2[pos] = pose_update(dc[6 * j:6 * j + 6], T[pos])
            X2 = X + dp
            trial = _cost(K, T2, X2, E, use, h2)
            out["steps"][rnd] += 1
            if trace is not None:
                trace.append((rnd, cur, trial, float(max(np.abs(dc).max(), np.abs(dp).max()))))
            if trial < cur:
                T, X = T2, X2
                lam /= 10.0
                out["accepted"][rnd] += 1
            else:
                lam *= 10.0
            if max(np.abs(dc).max(), np.abs(dp).max()) < 1e-10 or lam > 1e8:
                break
        inl = _classify(K, T, X, E, chi2)
        if rnd == 0:
            out["cost"][1] = _cost(K, T, X, E, np.ones(n_e, bool), chi2)
            use = inl
    out["cost"][2] = _cost(K, T, X, E, inl, 0.0)
    out["edge_inlier"][E["obs"]] = np.where(inl, 1, 2)
    out.update(n_free=len(free), n_fixed=len(fixed), n_local=len(lpt), n_edges=n_e, n_inliers=int(inl.sum()), free=free, fixed=sorted(fixed))
    out["poses"] = T
    out["points"][lpt] = X
    out["xyz"][lpt] = X.astype(np.float32)
    out["ok"] = out["n_inliers"] >= min_inliers
    return out


def add_observations(obs_off, obs_kf, obs_kp, counts, kf_pos, point, row=None):
    """the observation arrays after LocalMapper.add_observations(kf_pos, point, row): (obs_off, obs_kf, obs_kp)"""
    n_pts, n_kf = len(obs_off) - 1, len(counts)
    if not 0 <= kf_pos <= n_kf:
        raise ValueError("kf_pos")
    point = np.asarray(point).reshape(-1)
    row = np.arange(len(point)) if row is None else np.asarray(row).reshape(-1)
    edges = valid_edges(obs_off, obs_kf, obs_kp, counts)
    gain = {}
    for i, p in enumerate(point.tolist()):
        if not 0 <= p < n_pts or p in gain:
            continue
        gain[p] = i          # the lower i wins
    off, okf, okp = [0], [], []
    for p in range(n_pts):
        o0, o1 = int(obs_off[p]), int(obs_off[p + 1])
        okf += list(obs_kf[o0:o1]); okp += list(obs_kp[o0:o1])
        have = any(int(k) == kf_pos for k in obs_kf[o0:o1]) if kf_pos == n_kf else any(k == kf_pos for k, _, _ in edges[p])
        if p in gain and not have:
            okf.append(kf_pos); okp.append(int(row[gain[p]]))
        off.append(len(okf))
    return np.array(off, np.int32), np.array(okf, np.int32).reshape(-1), np.array(okp, np.int32).reshape(-1)
