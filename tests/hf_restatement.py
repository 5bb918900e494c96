"""TEST INFRASTRUCTURE ONLY: the homography branch of the two-view stage (visual-slam_amd/csrc/homography.h, twoview_h.hip,
mo_init_two_view_hf) restated in numpy f64, rule for rule: the same sampling stream (the first four indices of the oracle's sample8),
the same closed-form four-point H, the same refit rule, scores, decomposition order, CheckRT and selection.  The essential side is the
oracle's init_two_view.  Independent linear algebra: numpy's SVD (or, solver="eigh", eigh of the normal matrices - the second
formulation the parity bounds are measured with) where the device uses the sweep-operator solver and cyclic Jacobi."""
import numpy as np

from oracle import geom_oracle as G

CHI2_H, CHI2_F, COS_GOOD, COLLINEAR2 = 5.991, 3.841, 0.99998, 1e-12


def normalisation(p):
    """one image: (s, cx, cy) with x_n = s (x - c), mean distance from the centroid -> sqrt 2"""
    c = p.mean(axis=0)
    mean = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
    return (np.sqrt(2.0) / mean if mean > 1e-12 else 1.0), c[0], c[1]


def _T(nm):
    s, cx, cy = nm
    return np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1.0]])


def denormalise(Hn, n1, n2):
    return np.linalg.inv(_T(n2)) @ Hn @ _T(n1)


def _det_pts(a, b, c):
    return a[0] * (b[1] - c[1]) - a[1] * (b[0] - c[0]) + (b[0] * c[1] - b[1] * c[0])


def _spans(det, a, b, c):
    n = (a @ a + 1.0) * (b @ b + 1.0) * (c @ c + 1.0)
    return bool(det * det > COLLINEAR2 * n)


def _basis(a, b, c, d):
    l0, l1, l2, dd = _det_pts(d, b, c), _det_pts(a, d, c), _det_pts(a, b, d), _det_pts(a, b, c)
    if not (_spans(l0, d, b, c) and _spans(l1, a, d, c) and _spans(l2, a, b, d) and _spans(dd, a, b, c)):
        return None
    return np.array([[l0 * a[0], l1 * b[0], l2 * c[0]], [l0 * a[1], l1 * b[1], l2 * c[1]], [l0, l1, l2]])


def adj3(M):
    return np.array([np.cross(M[:, 1], M[:, 2]), np.cross(M[:, 2], M[:, 0]), np.cross(M[:, 0], M[:, 1])])


def homography4(x1, x2):
    """closed-form H of four correspondences (projective bases): H = B2 adj(B1), unit Frobenius norm; None = no model"""
    with np.errstate(all="ignore"):
        B1, B2 = _basis(*x1), _basis(*x2)
        if B1 is None or B2 is None:
            return None
        H = B2 @ adj3(B1)
        nn = (H * H).sum()
        if not (nn > 0 and np.isfinite(nn)):
            return None
        return H / np.sqrt(nn)


def transfer_chi(H, p1, p2, sigma):
    """CheckHomography: (chi in image 1 through adj(H), chi in image 2 through H), each (..., m)"""
    H = np.asarray(H)
    Hi = np.stack([np.cross(H[..., :, 1], H[..., :, 2]), np.cross(H[..., :, 2], H[..., :, 0]), np.cross(H[..., :, 0], H[..., :, 1])], axis=-2)
    inv = 1.0 / (sigma * sigma)
    h1 = np.concatenate([p1, np.ones((len(p1), 1))], axis=1)
    h2 = np.concatenate([p2, np.ones((len(p2), 1))], axis=1)
    with np.errstate(all="ignore"):
        q1 = np.einsum("...ij,mj->...mi", Hi, h2)
        q2 = np.einsum("...ij,mj->...mi", H, h1)
        a1, b1 = q1[..., 0] / q1[..., 2], q1[..., 1] / q1[..., 2]
        a2, b2 = q2[..., 0] / q2[..., 2], q2[..., 1] / q2[..., 2]
        c1 = ((p1[:, 0] - a1) ** 2 + (p1[:, 1] - b1) ** 2) * inv
        c2 = ((p2[:, 0] - a2) ** 2 + (p2[:, 1] - b2) ** 2) * inv
    return c1, c2


def _term(chi, th):
    with np.errstate(invalid="ignore"):
        return np.where(chi <= th, CHI2_H - chi, 0.0)


def h_cost(c1, c2):
    with np.errstate(invalid="ignore"):
        return (np.where(c1 <= CHI2_H, c1, CHI2_H) + np.where(c2 <= CHI2_H, c2, CHI2_H)).sum(axis=-1)


def h_score(c1, c2):
    with np.errstate(invalid="ignore"):
        return float((_term(c1, CHI2_H) + _term(c2, CHI2_H)).sum()), (c1 <= CHI2_H) & (c2 <= CHI2_H)


def fund_chi(F, p1, p2, sigma):
    inv = 1.0 / (sigma * sigma)
    h1 = np.concatenate([p1, np.ones((len(p1), 1))], axis=1)
    h2 = np.concatenate([p2, np.ones((len(p2), 1))], axis=1)
    l2 = h1 @ F.T   # lines in image 2: F x1
    l1 = h2 @ F     # lines in image 1: F' x2
    with np.errstate(all="ignore"):
        c1 = (l2 * h2).sum(axis=1) ** 2 / (l2[:, 0] ** 2 + l2[:, 1] ** 2) * inv
        c2 = (l1 * h1).sum(axis=1) ** 2 / (l1[:, 0] ** 2 + l1[:, 1] ** 2) * inv
    return c1, c2


def f_score(E, K, p1, p2, sigma):
    Ki = np.linalg.inv(K)
    c1, c2 = fund_chi(Ki.T @ E @ Ki, p1, p2, sigma)
    return float((_term(c1, CHI2_F) + _term(c2, CHI2_F)).sum())


def dlt_rows(x1, x2):
    z, o = np.zeros(len(x1)), np.ones(len(x1))
    r1 = np.stack([z, z, z, -x1[:, 0], -x1[:, 1], -o, x2[:, 1] * x1[:, 0], x2[:, 1] * x1[:, 1], x2[:, 1]], axis=1)
    r2 = np.stack([x1[:, 0], x1[:, 1], o, z, z, z, -x2[:, 0] * x1[:, 0], -x2[:, 0] * x1[:, 1], -x2[:, 0]], axis=1)
    return np.concatenate([r1, r2], axis=0)


def null_vector(A, solver):
    """right singular vector of the smallest singular value of A: numpy's SVD of A, or eigh of A'A"""
    if solver == "svd":
        if len(A) < A.shape[1]:
            A = np.vstack([A, np.zeros((A.shape[1] - len(A), A.shape[1]))])
        return np.linalg.svd(A)[2][-1]
    return np.linalg.eigh(A.T @ A)[1][:, 0]


def reconstruct(H, K):
    """ReconstructH: the eight (R, t, n) of Faugeras in ORB-SLAM2's order, or None (no decomposition)"""
    A = np.linalg.inv(K) @ H @ K
    if not np.isfinite(A).all():
        return None
    if np.linalg.det(A) < 0:
        A = -A
    U, d, Vt = np.linalg.svd(A)
    V = Vt.T.copy()
    # canonical signs (hg_svd3): largest component of v1 and v3 positive (the first of equals), v2 and u2 complete right-handed frames
    # (det(A) > 0, so U and V are proper together and ORB-SLAM2's s = det(U) det(V') is 1)
    for k in (0, 2):
        if V[int(np.argmax(np.abs(V[:, k]))), k] < 0:
            V[:, k] = -V[:, k]; U[:, k] = -U[:, k]
    V[:, 1] = np.cross(V[:, 2], V[:, 0]); U[:, 1] = np.cross(U[:, 2], U[:, 0])
    Vt = V.T
    d1, d2, d3 = d
    if not d3 > 0 or d1 / d2 < 1.00001 or d2 / d3 < 1.00001:
        return None
    q12, q23, q13 = d1 * d1 - d2 * d2, d2 * d2 - d3 * d3, d1 * d1 - d3 * d3
    aux1, aux3 = np.sqrt(q12 / q13), np.sqrt(q23 / q13)
    x1 = [aux1, aux1, -aux1, -aux1]
    x3 = [aux3, -aux3, aux3, -aux3]
    ss = np.sqrt(q12 * q23)
    st, ct = ss / ((d1 + d3) * d2), (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    sp, cp = ss / ((d1 - d3) * d2), (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    sgn = [1.0, -1.0, -1.0, 1.0]
    out = []
    for c in range(8):
        i = c & 3
        if c < 4:
            s = st * sgn[i]
            Rp = np.array([[ct, 0, -s], [0, 1, 0], [s, 0, ct]])
            tp = np.array([x1[i], 0, -x3[i]]) * (d1 - d3)
        else:
            s = sp * sgn[i]
            Rp = np.array([[cp, 0, s], [0, -1, 0], [s, 0, -cp]])
            tp = np.array([x1[i], 0, x3[i]]) * (d1 + d3)
        R = U @ Rp @ Vt
        t = U @ tp
        n = V @ np.array([x1[i], 0, x3[i]])
        out.append((R, t / np.linalg.norm(t), -n if n[2] < 0 else n))
    return out


def check_rt(K, R, t, p1, p2, sigma, solver):
    """CheckRT over the given correspondences -> (passed, good, cos, X): passed counts for nGood and enters the parallax list,
    good = passed with cos < COS_GOOD (a map point)"""
    P1 = K @ np.hstack([np.eye(3), np.zeros((3, 1))])
    P2 = K @ np.hstack([R, t.reshape(3, 1)])
    n = len(p1)
    A = np.empty((n, 4, 4))
    A[:, 0] = p1[:, 0:1] * P1[2] - P1[0]
    A[:, 1] = p1[:, 1:2] * P1[2] - P1[1]
    A[:, 2] = p2[:, 0:1] * P2[2] - P2[0]
    A[:, 3] = p2[:, 1:2] * P2[2] - P2[1]
    if solver == "svd":
        Q = np.linalg.svd(A)[2][:, -1, :]
    else:
        Q = np.linalg.eigh(np.einsum("nki,nkj->nij", A, A))[1][:, :, 0]
    with np.errstate(all="ignore"):
        X = Q[:, :3] / Q[:, 3:4]
        fin = np.isfinite(X).all(axis=1)
        O2 = -R.T @ t
        n2 = X - O2
        cos = (X * n2).sum(axis=1) / (np.linalg.norm(X, axis=1) * np.linalg.norm(n2, axis=1))
        low = ~(cos < COS_GOOD)
        X2 = X @ R.T + t
        ok = fin & ~((X[:, 2] <= 0) & ~low) & ~((X2[:, 2] <= 0) & ~low)
        th2 = 4.0 * sigma * sigma
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        e1 = (fx * X[:, 0] / X[:, 2] + cx - p1[:, 0]) ** 2 + (fy * X[:, 1] / X[:, 2] + cy - p1[:, 1]) ** 2
        e2 = (fx * X2[:, 0] / X2[:, 2] + cx - p2[:, 0]) ** 2 + (fy * X2[:, 1] / X2[:, 2] + cy - p2[:, 1]) ** 2
        ok &= (e1 <= th2) & (e2 <= th2)
    return ok, ok & ~low, cos, X, e1, e2


def select(n_good):
    bg = sg = 0
    bi = si = -1
    for i in range(8):
        if n_good[i] > bg:
            sg, si, bg, bi = bg, bi, n_good[i], i
        elif n_good[i] > sg:
            sg, si = n_good[i], i
    return bi, si


def hf_two_view(p1, p2, K, thr_px=3.0, n_hyp=4096, seed=4096, n_hyp_h=512, sigma=1.0, rh_threshold=0.40, min_parallax_deg=1.0,
                min_triangulated=50, pair=0, solver="svd", essential=None):
    """-> dict with the fields of Context.init_two_view_hf plus what the tests' input conditions need: cost (n_hyp_h,) float32 costs
    of the hypotheses (inf: no model), margin = the smallest relative distance of a compared error from its threshold over every
    decision the masks rest on.  essential: a precomputed G.init_two_view result for the same arguments."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    p1f = np.asarray(p1, np.float32).reshape(-1, 2); p2f = np.asarray(p2, np.float32).reshape(-1, 2)
    p1 = p1f.astype(np.float64); p2 = p2f.astype(np.float64)
    m = len(p1)
    nan33, nan31 = np.full((3, 3), np.nan), np.full((3, 1), np.nan)
    out = dict(model=-1, accepted=False, R=nan33, t=nan31, pose_mask=np.zeros(m, bool), X=np.full((m, 3), np.nan, np.float32), n_good=0,
               E=nan33, ransac_mask=np.zeros(m, bool), R_e=nan33, t_e=nan31, n_good_e=0, H=nan33, h_mask=np.zeros(m, bool), SH=0.0, SF=0.0,
               RH=0.0, n_good_h=np.zeros(8, np.int32), parallax_h=np.zeros(8), cos_h=np.full(8, 2.0), best_h=-1, second_h=-1, n_inliers_h=0,
               accepted_h=False, winner_h=-1, refits_h=0, R_h=nan33, t_h=nan31, cost=None, margin=np.inf)
    if m < 8:
        return out
    e = essential if essential is not None else G.init_two_view(p1f, p2f, K, thr_px, n_hyp, seed, pair)
    have_e = e["E"] is not None
    if have_e:
        out.update(E=e["E"], ransac_mask=e["ransac_mask"], R_e=e["R"], t_e=e["t"], n_good_e=e["n_good"])
    margins = []

    def margin_of(vals, th):
        v = np.asarray(vals, np.float64).ravel()
        v = v[np.isfinite(v)]
        if len(v):
            margins.append(float(np.abs(v - th).min() / th))

    # ---- hypotheses
    n1, n2 = normalisation(p1), normalisation(p2)
    x1 = n1[0] * (p1 - np.array(n1[1:])); x2 = n2[0] * (p2 - np.array(n2[1:]))
    Hs = np.full((n_hyp_h, 3, 3), np.nan)
    for h in range(n_hyp_h):
        idx = G.sample8(seed, h, m, pair)[:4]
        Hn = homography4(x1[idx], x2[idx])
        if Hn is not None:
            Hp = denormalise(Hn, n1, n2)
            if np.isfinite(Hp).all() and (Hp * Hp).sum() > 0:
                Hs[h] = Hp
    valid = np.isfinite(Hs[:, 0, 0])
    cost = np.full(n_hyp_h, np.inf, np.float32)
    if valid.any():
        c1, c2 = transfer_chi(Hs[valid], p1, p2, sigma)
        cost[valid] = h_cost(c1, c2).astype(np.float32)
    out["cost"] = cost
    if have_e:
        out["SF"] = f_score(e["E"], K, p1, p2, sigma)
        Ki = np.linalg.inv(K)
        for c in fund_chi(Ki.T @ e["E"] @ Ki, p1, p2, sigma):
            margin_of(c, CHI2_F)
    if valid.any():
        w = int(np.argmin(cost))  # (the first of equals: the lowest hypothesis index)
        H = Hs[w] / np.linalg.norm(Hs[w])
        out["winner_h"] = w
        # ---- a. refits
        prev, refits = None, 0
        while True:
            c1, c2 = transfer_chi(H, p1, p2, sigma)
            SH, mask = h_score(c1, c2)
            margin_of(c1, CHI2_H); margin_of(c2, CHI2_H)
            c = int(mask.sum())
            if c < 4 or (prev is not None and np.array_equal(mask, prev)) or refits == 5:
                break
            v = null_vector(dlt_rows(x1[mask], x2[mask]), solver)
            Hp = denormalise(v.reshape(3, 3), n1, n2)
            if not (np.isfinite(Hp).all() and (Hp * Hp).sum() > 0):
                break
            H = Hp / np.linalg.norm(Hp)
            prev = mask
            refits += 1
        out.update(H=H, h_mask=mask, SH=SH, n_inliers_h=c, refits_h=refits)
        # ---- c, d. decomposition and CheckRT
        cands = reconstruct(H, K)
        if cands is not None:
            q1, q2 = p1[mask], p2[mask]
            n_good = np.zeros(8, np.int32)
            res = []
            for k, (R, t, _) in enumerate(cands):
                ok, good, cos, X, e1, e2 = check_rt(K, R, t, q1, q2, sigma, solver)
                n_good[k] = int(ok.sum())
                if n_good[k]:
                    cs = np.sort(np.where(np.isnan(cos[ok]), 2.0, cos[ok]))
                    out["cos_h"][k] = cs[min(50, len(cs) - 1)]
                    out["parallax_h"][k] = np.degrees(np.arccos(np.clip(out["cos_h"][k], -1.0, 1.0)))
                res.append((ok, good, cos, X, e1, e2))
            bi, si = select(n_good)
            out.update(n_good_h=n_good, best_h=bi, second_h=si)
            if bi >= 0:
                ok, good, cos, X, e1, e2 = res[bi]
                margin_of(e1, 4.0 * sigma * sigma); margin_of(e2, 4.0 * sigma * sigma); margin_of(cos, COS_GOOD)
                cos_max = np.cos(np.radians(min_parallax_deg))
                sg = int(n_good[si]) if si >= 0 else 0
                out["accepted_h"] = bool(sg < 0.75 * n_good[bi] and out["cos_h"][bi] <= cos_max and n_good[bi] > min_triangulated and
                                         n_good[bi] > 0.9 * c)
                out.update(R_h=cands[bi][0], t_h=cands[bi][1].reshape(3, 1))
                pm = np.zeros(m, bool); pm[np.nonzero(mask)[0][good]] = True
                Xh = np.full((m, 3), np.nan, np.float32); Xh[pm] = X[good].astype(np.float32)
                out["_pose_mask_h"], out["_X_h"] = pm, Xh
    s = out["SH"] + out["SF"]
    out["RH"] = out["SH"] / s if s > 0 else 0.0
    out["margin"] = min(margins) if margins else np.inf
    if not have_e:
        return out
    if out["RH"] > rh_threshold:
        bi = out["best_h"]
        out.update(model=1, accepted=out["accepted_h"], n_good=int(out["n_good_h"][bi]) if bi >= 0 else 0, R=out["R_h"], t=out["t_h"],
                   pose_mask=out.get("_pose_mask_h", np.zeros(m, bool)), X=out.get("_X_h", np.full((m, 3), np.nan, np.float32)))
    else:
        out.update(model=0, accepted=e["n_good"] > min_triangulated, n_good=e["n_good"], R=e["R"], t=e["t"], pose_mask=e["pose_mask"], X=e["X"])
    return out
