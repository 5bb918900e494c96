"""numpy restatement of LocalMapper.create_new_map_points (mo_map_grow in include/vslam_amd.h): free rows, the geometry of every
(target, neighbour) pair, the epipolar search, claims, the base pair, the Cholesky triangulation, the gates and the appended points.
f64 in the header's operation order: the search runs one target row against a neighbour's rows as elementwise numpy expressions (the
same IEEE operations, unfused), everything behind it in Python scalars.  Exact integers given the map; every threshold decision
reports how far it was from going the other way."""
import math

import numpy as np

from tests.reloc_restatement import hamming
from tests.track_restatement import _info, _power, valid_observations

FIELDS = ("xyz", "color", "id", "obs_off", "obs_kf", "obs_kp", "dref_kf", "dref_row")
COUNTS = ("n_neighbours", "n_free", "n_epi", "n_accepted", "n_matches", "n_new", "n_obs_new", "n_points", "n_obs")
KINDS = ("den", "zone", "epi", "max_dist", "cos", "base", "chol", "z", "chi2", "dist", "ratio")


def free_rows(a, counts, lo=0):
    """per keyframe position >= lo: mask of the rows no map point validly observes (others: None)"""
    free = [None if k < lo else np.ones(int(c), bool) for k, c in enumerate(counts)]
    for v in valid_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], counts):
        for k, r in v:
            if k >= lo:
                free[k][r] = False
    return free


def camera(T):
    """(R rows, t, C) of a pose, C[i] = -(R[0][i] t[0] + R[1][i] t[1] + R[2][i] t[2])"""
    T = np.asarray(T, np.float64)
    R = [[float(T[i][j]) for j in range(3)] for i in range(3)]
    t = [float(T[i][3]) for i in range(3)]
    C = [-(R[0][i] * t[0] + R[1][i] * t[1] + R[2][i] * t[2]) for i in range(3)]
    return R, t, C


def pair_geometry(K, cam1, cam2):
    """(F rows, ex, ey) of a target cam1 and a neighbour cam2"""
    fx, fy, cx, cy = K
    (R1, t1, C1), (R2, t2, _) = cam1, cam2
    R12 = [[R1[i][0] * R2[j][0] + R1[i][1] * R2[j][1] + R1[i][2] * R2[j][2] for j in range(3)] for i in range(3)]
    t12 = [t1[i] - (R12[i][0] * t2[0] + R12[i][1] * t2[1] + R12[i][2] * t2[2]) for i in range(3)]
    E = [[t12[1] * R12[2][j] - t12[2] * R12[1][j] for j in range(3)],
         [t12[2] * R12[0][j] - t12[0] * R12[2][j] for j in range(3)],
         [t12[0] * R12[1][j] - t12[1] * R12[0][j] for j in range(3)]]
    ifx, ify = 1.0 / fx, 1.0 / fy
    G = []
    for i in range(3):
        g0, g1 = E[i][0] * ifx, E[i][1] * ify
        G.append([g0, g1, (E[i][2] - g0 * cx) - g1 * cy])
    F0 = [G[0][j] * ifx for j in range(3)]
    F1 = [G[1][j] * ify for j in range(3)]
    F2 = [(G[2][j] - F0[j] * cx) - F1[j] * cy for j in range(3)]
    c2 = [R2[i][0] * C1[0] + R2[i][1] * C1[1] + R2[i][2] * C1[2] + t2[i] for i in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        ex = float(np.float64(fx * c2[0]) / np.float64(c2[2]) + cx)
        ey = float(np.float64(fy * c2[1]) / np.float64(c2[2]) + cy)
    return [F0, F1, F2], ex, ey


def ray(cam, xn, yn):
    R = cam[0]
    return [R[0][i] * xn + R[1][i] * yn + R[2][i] for i in range(3)]


def cos_parallax(r1, r2):
    n1 = math.sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2])
    n2 = math.sqrt(r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2])
    return (r1[0] * r2[0] + r1[1] * r2[1] + r1[2] * r2[2]) / (n1 * n2)


def triangulate(cam1, xn1, yn1, cam2, xn2, yn2, note=lambda kind, v: None):
    """the header's 4 x 3 system by its normal equations and a 3 x 3 Cholesky factorisation; None when a radicand is not > 0"""
    A, a4 = [], []
    for (R, t, _), xs in ((cam1, (xn1, yn1)), (cam2, (xn2, yn2))):
        for w, x in enumerate(xs):
            A.append([x * R[2][j] - R[w][j] for j in range(3)])
            a4.append(x * t[2] - t[w])
    N = [[A[0][i] * A[0][j] + A[1][i] * A[1][j] + A[2][i] * A[2][j] + A[3][i] * A[3][j] for j in range(3)] for i in range(3)]
    g = [-(A[0][i] * a4[0] + A[1][i] * a4[1] + A[2][i] * a4[2] + A[3][i] * a4[3]) for i in range(3)]
    note("chol", N[0][0])
    if not N[0][0] > 0.0:
        return None
    l00 = math.sqrt(N[0][0]); l10 = N[1][0] / l00; l20 = N[2][0] / l00
    p1 = N[1][1] - l10 * l10
    note("chol", p1)
    if not p1 > 0.0:
        return None
    l11 = math.sqrt(p1); l21 = (N[2][1] - l20 * l10) / l11
    p2 = (N[2][2] - l20 * l20) - l21 * l21
    note("chol", p2)
    if not p2 > 0.0:
        return None
    l22 = math.sqrt(p2)
    y0 = g[0] / l00; y1 = (g[1] - l10 * y0) / l11; y2 = ((g[2] - l20 * y0) - l21 * y1) / l22
    X2 = y2 / l22
    X1 = (y1 - l21 * X2) / l11
    X0 = ((y0 - l10 * X1) - l20 * X2) / l00
    return [X0, X1, X2]


def grow(a, K, poses, kf_xy, kf_oct, kf_desc, window=10, max_dist=50, scale_factor=1.2, epi_chi2=3.84, chi2=5.991, cos_max=0.9998,
         ratio_factor=None, epipole_r2=100.0, image=None, target_slot=None, ties=1):
    """(arrays after, point [rows of the target], points [n_new][3] f64, counts, margins).  a: the map arrays (FIELDS); poses [n_kf] 4x4 or
    3x4 and kf_xy / kf_oct / kf_desc by keyframe position; image: the target's stored image (None: none); target_slot: the store slot
    of the last keyframe (None: its position).  margins: per kind of
    threshold decision (KINDS) the smallest distance of any decided value from its threshold, and "min" over the kinds.
    ties = -1 is the WRONG rule - equal distances go to the higher neighbour row and the higher target row - for the tests that show a
    tie case would notice it (tests/test_grow_cpu.py)."""
    ratio_factor = 1.5 * scale_factor if ratio_factor is None else ratio_factor
    n_kf = len(kf_desc)
    same = {f: np.array(a[f]).copy() for f in FIELDS}
    n0, o0 = len(same["id"]), len(same["obs_kf"])
    cnt = dict.fromkeys(COUNTS, 0)
    cnt["n_points"], cnt["n_obs"] = n0, o0
    margins = {k: np.inf for k in KINDS}

    def note(kind, v, thr=0.0):
        margins[kind] = min(margins[kind], abs(float(v) - thr))

    n_rows = len(kf_desc[-1]) if n_kf else 0
    point = np.full(n_rows, -1, np.int32)

    def done(arrays, pts):
        margins["min"] = min(margins.values())
        return arrays, point, np.array(pts, np.float64).reshape(-1, 3), cnt, margins
    if n_kf < 2:
        return done(same, [])
    T = n_kf - 1
    lo = T - window if 0 < window < T else 0
    cnt["n_neighbours"] = T - lo
    if n_rows == 0:
        return done(same, [])
    counts = [len(d) for d in kf_desc]
    free = free_rows(a, counts, lo)
    Kf = (float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
    fx, fy, cx, cy = Kf
    cams = [camera(poses[k]) if k >= lo else None for k in range(n_kf)]
    xy = [None if k < lo else np.asarray(kf_xy[k], np.float32).astype(np.float64).reshape(-1, 2) for k in range(n_kf)]
    rows1 = np.flatnonzero(free[T])
    cnt["n_free"] = len(rows1)
    # search and claims
    claim, accepted = {}, {}
    for k in range(lo, T):
        F, ex, ey = pair_geometry(Kf, cams[T], cams[k])
        q = np.flatnonzero(free[k])
        if not len(q):
            continue
        x2, y2 = xy[k][q, 0], xy[k][q, 1]
        o2 = [int(o) for o in np.asarray(kf_oct[k])[q]]
        zone = np.array([epipole_r2 * _power(scale_factor, o) for o in o2])
        epi = np.array([epi_chi2 * _power(scale_factor * scale_factor, o) for o in o2])
        with np.errstate(over="ignore", invalid="ignore"):   # (an epipole at infinity: ze is inf or NaN, and excludes nothing)
            dxe, dye = ex - x2, ey - y2
            ze = dxe * dxe + dye * dye
            out_zone = ~(ze < zone)
        if np.isfinite(ze).all():
            note("zone", np.abs(ze - zone).min())
        for r1 in rows1.tolist():
            x1, y1 = float(xy[T][r1, 0]), float(xy[T][r1, 1])
            la = x1 * F[0][0] + y1 * F[1][0] + F[2][0]
            lb = x1 * F[0][1] + y1 * F[1][1] + F[2][1]
            lc = x1 * F[0][2] + y1 * F[1][2] + F[2][2]
            den = la * la + lb * lb
            terms = (abs(x1 * F[0][0]) + abs(y1 * F[1][0]) + abs(F[2][0])) + (abs(x1 * F[0][1]) + abs(y1 * F[1][1]) + abs(F[2][1]))
            if terms > 0.0:   # (how far a and b are from cancelling to 0; an F of zeros is 0 on both sides)
                note("den", (abs(la) + abs(lb)) / terms)
            if den == 0.0:
                continue
            num = la * x2 + lb * y2 + lc
            with np.errstate(over="ignore", invalid="ignore"):
                e = (num * num) / den
            if out_zone.any():
                note("epi", np.abs(e - epi)[out_zone].min())
            ok = out_zone & (e < epi)
            cnt["n_epi"] += int(ok.sum())
            if not ok.any():
                continue
            qq = q[ok]
            d = hamming(kf_desc[T][r1:r1 + 1], kf_desc[k][qq])[0]
            order = np.lexsort((ties * qq, d))   # lowest distance, ties to the lower row
            bd, bq = int(d[order[0]]), int(qq[order[0]])
            note("max_dist", bd, max_dist + 0.5)
            if bd > max_dist:
                continue
            cnt["n_accepted"] += 1
            accepted[(r1, k)] = bq
            if (k, bq) not in claim or (bd, ties * r1) < (claim[(k, bq)][0], ties * claim[(k, bq)][1]):
                claim[(k, bq)] = (bd, r1)
    # points, in order of target row
    oct1 = np.asarray(kf_oct[T])
    new_xyz, new_obs, new_rows, new_X = [], [], [], []
    for r1 in rows1.tolist():
        won = [(k, accepted[(r1, k)]) for k in range(lo, T) if (r1, k) in accepted and claim[(k, accepted[(r1, k)])][1] == r1]
        cnt["n_matches"] += len(won)
        if not won:
            continue
        x1, y1, o1 = float(xy[T][r1, 0]), float(xy[T][r1, 1]), int(oct1[r1])
        xn1, yn1 = (x1 - cx) / fx, (y1 - cy) / fy
        ray1 = ray(cams[T], xn1, yn1)
        usable = []
        for k, r2 in won:
            cosp = cos_parallax(ray1, ray(cams[k], (float(xy[k][r2, 0]) - cx) / fx, (float(xy[k][r2, 1]) - cy) / fy))
            note("cos", cosp); note("cos", cosp, cos_max)
            if 0.0 < cosp < cos_max:
                usable.append((cosp, k, r2))
        if not usable:
            continue
        usable.sort()   # lowest cosp, ties to the lower position
        if len(usable) > 1:
            note("base", usable[1][0] - usable[0][0])
        _, bk, b2 = usable[0]
        x2, y2, o2 = float(xy[bk][b2, 0]), float(xy[bk][b2, 1]), int(np.asarray(kf_oct[bk])[b2])
        X = triangulate(cams[T], xn1, yn1, cams[bk], (x2 - cx) / fx, (y2 - cy) / fy, note)
        if X is None:
            continue

        def seen(cam, x, y, o):
            R, t, _ = cam
            Xc = [R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + t[i] for i in range(3)]
            note("z", Xc[2])
            if not Xc[2] > 0.0:
                return False
            u, v = (fx * Xc[0]) / Xc[2] + cx, (fy * Xc[1]) / Xc[2] + cy
            du, dv = u - x, v - y
            e2 = _info(scale_factor, o) * (du * du + dv * dv)
            note("chi2", e2, chi2)
            return e2 <= chi2
        if not seen(cams[T], x1, y1, o1) or not seen(cams[bk], x2, y2, o2):
            continue

        def dist(C):
            dx, dy, dz = X[0] - C[0], X[1] - C[1], X[2] - C[2]
            return math.sqrt(dx * dx + dy * dy + dz * dz)
        d1, d2 = dist(cams[T][2]), dist(cams[bk][2])
        note("dist", d1); note("dist", d2)
        if not (d1 > 0.0 and d2 > 0.0):
            continue
        rd, ro = d2 / d1, _power(scale_factor, o1) / _power(scale_factor, o2)
        note("ratio", rd * ratio_factor, ro); note("ratio", rd, ro * ratio_factor)
        if rd * ratio_factor < ro or rd > ro * ratio_factor:
            continue
        obs = []
        for k, r2 in won:
            if k == bk or seen(cams[k], float(xy[k][r2, 0]), float(xy[k][r2, 1]), int(np.asarray(kf_oct[k])[r2])):
                obs.append((k, r2))
        obs.append((T, r1))
        point[r1] = n0 + len(new_rows)
        new_rows.append(r1); new_obs.append(obs); new_X.append(X)
    if not new_rows:
        return done(same, [])
    n_new = len(new_rows)
    col = np.zeros((n_new, 3), np.uint8)
    col[:, 2] = 255
    if image is not None:
        img = np.asarray(image, np.uint8)
        h, w = img.shape[:2]
        for j, r1 in enumerate(new_rows):
            x, y = int(np.float32(kf_xy[T][r1][0])), int(np.float32(kf_xy[T][r1][1]))
            if 0 <= x < w and 0 <= y < h:
                px = img[y, x]
                col[j] = px if img.ndim == 3 else [px, px, px]
    out = dict(same)
    out["xyz"] = np.vstack([same["xyz"].reshape(-1, 3), np.array(new_X, np.float64).astype(np.float32)]).astype(np.float32)
    out["color"] = np.vstack([same["color"].reshape(-1, 3), col]).astype(np.uint8)
    out["id"] = np.concatenate([same["id"], n0 + np.arange(n_new)]).astype(np.int32)
    out["dref_kf"] = np.concatenate([same["dref_kf"], np.full(n_new, T if target_slot is None else target_slot)]).astype(np.int32)
    out["dref_row"] = np.concatenate([same["dref_row"], new_rows]).astype(np.int32)
    okf = [k for v in new_obs for k, _ in v]
    okp = [r for v in new_obs for _, r in v]
    off = o0 + np.cumsum([len(v) for v in new_obs])
    out["obs_off"] = np.concatenate([same["obs_off"], off]).astype(np.int32)
    out["obs_kf"] = np.concatenate([same["obs_kf"], okf]).astype(np.int32)
    out["obs_kp"] = np.concatenate([same["obs_kp"], okp]).astype(np.int32)
    cnt["n_new"], cnt["n_obs_new"] = n_new, len(okf)
    cnt["n_points"], cnt["n_obs"] = n0 + n_new, o0 + len(okf)
    return done(out, new_X)


def co_visibility_recount(a, counts, first=0):
    """{(position a < position b): points from index `first` on that validly observe both}"""
    g = {}
    sub = valid_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], counts)
    for v in sub[first:]:
        pos = sorted({k for k, _ in v})
        for i in range(len(pos)):
            for j in range(i + 1, len(pos)):
                g[(pos[i], pos[j])] = g.get((pos[i], pos[j]), 0) + 1
    return g
