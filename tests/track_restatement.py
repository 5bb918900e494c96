"""numpy restatement of LocalMapper.track_local_map (mo_map_track in include/vslam_amd.h): the local map, the representative
descriptors, the search by projection with its conflicts and the retry (exact integers given a pose), and the pose refinement (f64)."""
import numpy as np

from tests.reloc_restatement import hamming

NOT_LOCAL = None


def valid_observations(obs_off, obs_kf, obs_kp, counts):
    """per point: [(keyframe position, row)] of its valid observations in insertion order (negative values count from the end,
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
            kp = int(obs_kp[o])
            if kp < 0:
                kp += int(counts[k])
            if not 0 <= kp < counts[k]:
                continue
            v.append((k, kp))
        out.append(v)
    return out


def local_points(obs, n_kf, window):
    """mask of the points with a valid observation in the last `window` keyframe positions (0: all)"""
    lo = n_kf - window if 0 < window < n_kf else 0
    return np.array([any(k >= lo for k, _ in v) for v in obs], bool)


def representative(descs):
    """index of ComputeDistinctiveDescriptors' choice among [n][32] descriptors: smallest median distance (element (n - 1) // 2 of the
    sorted distances to all, itself included), ties to the earlier"""
    d = hamming(descs, descs)
    med = np.sort(d, axis=1)[:, (len(descs) - 1) // 2]
    return int(np.argmin(med))   # argmin: the first of equal values


def representatives(obs, kf_desc, kf_oct, local):
    """rep [n][32] and ref_octave [n] (None outside the local map)"""
    n = len(obs)
    rep = np.zeros((n, 32), np.uint8)
    ref = [None] * n
    for i, v in enumerate(obs):
        if not local[i]:
            continue
        descs = np.array([kf_desc[k][r] for k, r in v], np.uint8)
        j = representative(descs)
        k, r = v[j]
        rep[i] = kf_desc[k][r]
        ref[i] = int(kf_oct[k][r])
    return rep, ref


def _power(base, o):
    s = 1.0
    for _ in range(max(int(o), 0)):
        s *= base
    return s


def projection_matrix(K, pose):
    """P = K [R | t], each entry K[i][0] M[0][j] + K[i][1] M[1][j] + K[i][2] M[2][j] (pnp_projection)"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    M = np.asarray(pose, np.float64)[:3, :4]
    P = np.zeros((3, 4))
    for i in range(3):
        for j in range(4):
            P[i, j] = K[i, 0] * M[0, j] + K[i, 1] * M[1, j] + K[i, 2] * M[2, j]
    return P


def project(K, pose, xyz):
    """(u / z, v / z, z) of f32 points, each row of P X_h summed left to right"""
    P = projection_matrix(K, pose)
    X = np.asarray(xyz, np.float32).astype(np.float64)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    u = P[0, 0] * x + P[0, 1] * y + P[0, 2] * z + P[0, 3]
    v = P[1, 0] * x + P[1, 1] * y + P[1, 2] * z + P[1, 3]
    w = P[2, 0] * x + P[2, 1] * y + P[2, 2] * z + P[2, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        return u / w, v / w, w


def search(K, pose, xyz, rep, ref, kps, desc, w, h, radius, scale_factor=1.2, max_dist=100, ratio=0.8, octave_gate=True, scale_radius=True):
    """one attempt of a pass: (point [nq], dist [nq], candidates).  kps: KP_DTYPE records of the frame.  octave_gate=False drops the
    |octave - ref_octave| <= 1 condition, scale_radius=False searches every point at the octave-0 radius: wrong on purpose, for tests
    that must show their inputs tell the rule from its absence."""
    nq = len(kps)
    point = np.full(nq, -1, np.int64)
    dist = np.full(nq, -1, np.int64)
    u, v, z = project(K, pose, xyz)
    kx, ky = kps["x"].astype(np.float64), kps["y"].astype(np.float64)
    ko = kps["octave"].astype(np.int64)
    claim = {}
    n_cand = 0
    for i in range(len(xyz)):
        if ref[i] is None or not z[i] > 0:
            continue
        if not (u[i] >= 0 and u[i] < w and v[i] >= 0 and v[i] < h):
            continue
        n_cand += 1
        r = radius * (_power(scale_factor, ref[i]) if scale_radius else 1.0)
        q = np.flatnonzero((np.abs(kx - u[i]) < r) & (np.abs(ky - v[i]) < r) & ((np.abs(ko - ref[i]) <= 1) | (not octave_gate)))
        if len(q) == 0:
            continue
        d = hamming(rep[i:i + 1], desc[q])[0]
        order = np.lexsort((q, d))   # lowest distance, ties to the lower keypoint
        bd, bq = int(d[order[0]]), int(q[order[0]])
        if bd > max_dist:
            continue
        if len(q) > 1 and not float(bd) <= ratio * float(d[order[1]]):
            continue
        if bq not in claim or (bd, i) < claim[bq]:
            claim[bq] = (bd, i)
    for q, (d, i) in claim.items():
        point[q] = i
        dist[q] = d
    return point, dist, n_cand


def _info(scale_factor, octave):
    return 1.0 / _power(scale_factor * scale_factor, octave)


def inliers(K, pose, X, x, info, chi2):
    """z > 0 and info * squared pixel error <= chi2"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    Xc = X @ pose[:3, :3].T + pose[:3, 3]
    p = Xc @ K.T
    e2 = (p[:, 0] / p[:, 2] - x[:, 0]) ** 2 + (p[:, 1] / p[:, 2] - x[:, 1]) ** 2
    return (Xc[:, 2] > 0) & (info * e2 <= chi2)


def _exp_so3(w):
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < 1e-8:
        a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + a * W + b * (W @ W)


def refine(K, pose, X, x, octave, scale_factor=1.2, chi2=5.991, unit_information=False):
    """PoseOptimization with Gauss-Newton steps: (pose 4x4, inlier mask, inliers).  X [m][3] f64 (the map's f32 values), x [m][2] f64,
    octave [m] of the frame keypoints.  unit_information=True weighs every match with 1 (wrong on purpose, as search's switches)."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    T = np.array(pose, np.float64)
    info = np.array([1.0 if unit_information else _info(scale_factor, o) for o in octave])
    inl = np.ones(len(X), bool)
    n_inl = len(X)
    for rnd in range(4):
        huber2 = chi2 if rnd < 3 else 0.0
        for _ in range(10):
            sel = inl
            Xc = X[sel] @ T[:3, :3].T + T[:3, 3]
            p = Xc @ K.T
            iz = 1.0 / p[:, 2]
            r = np.column_stack([p[:, 0] * iz - x[sel, 0], p[:, 1] * iz - x[sel, 1]])
            du = (K[0][None, :] * p[:, 2:3] - p[:, 0:1] * K[2][None, :]) * (iz * iz)[:, None]
            dv = (K[1][None, :] * p[:, 2:3] - p[:, 1:2] * K[2][None, :]) * (iz * iz)[:, None]
            Ju = np.column_stack([du, -du[:, 1] * Xc[:, 2] + du[:, 2] * Xc[:, 1], du[:, 0] * Xc[:, 2] - du[:, 2] * Xc[:, 0],
                                  -du[:, 0] * Xc[:, 1] + du[:, 1] * Xc[:, 0]])
            Jv = np.column_stack([dv, -dv[:, 1] * Xc[:, 2] + dv[:, 2] * Xc[:, 1], dv[:, 0] * Xc[:, 2] - dv[:, 2] * Xc[:, 0],
                                  -dv[:, 0] * Xc[:, 1] + dv[:, 1] * Xc[:, 0]])
            e2 = info[sel] * (r ** 2).sum(1)
            wt = info[sel].copy()
            if huber2 > 0:
                big = e2 > huber2
                wt[big] = info[sel][big] * (np.sqrt(huber2) / np.sqrt(e2[big]))
            H = (Ju.T * wt) @ Ju + (Jv.T * wt) @ Jv
            g = (Ju.T * wt) @ r[:, 0] + (Jv.T * wt) @ r[:, 1]
            try:
                np.linalg.cholesky(H)
            except np.linalg.LinAlgError:
                break
            d = np.linalg.solve(H, -g)
            E = _exp_so3(d[3:])
            T2 = np.eye(4)
            T2[:3, :3] = E @ T[:3, :3]
            T2[:3, 3] = E @ T[:3, 3] + d[:3]
            T = T2
            if np.sqrt(d @ d) < 1e-12:
                break
        inl = inliers(K, T, X, x, info, chi2)
        n_inl = int(inl.sum())
        if n_inl < 10:
            break
    return T, inl, n_inl


def local_map(obs_off, obs_kf, obs_kp, kf_desc, kf_oct, window=10):
    """(rep, ref_octave, n_local) of the map for a window: everything track() derives before it sees the frame"""
    counts = [len(d) for d in kf_desc]
    obs = valid_observations(obs_off, obs_kf, obs_kp, counts)
    local = local_points(obs, len(counts), window)
    rep, ref = representatives(obs, kf_desc, kf_oct, local)
    return rep, ref, int(local.sum())


def track(K, pose0, xyz, obs_off, obs_kf, obs_kp, kf_desc, kf_oct, kps, desc, w, h, window=10, radii=(15.0, 4.0), scale_factor=1.2,
          max_dist=100, ratio=0.8, chi2=5.991, min_matches=20, min_inliers=30, refine_pose=True, poses=None, octave_gate=True, scale_radius=True, local_map=None):
    """the whole call: per pass the search (with its retry) and the refinement.  poses: the pose each pass projects from, in place of
    the previous pass's refinement (to restate one pass from the device's own pose).  local_map: what local_map() returned for this
    map and window, to restate several frames against one large map without deriving it again."""
    rep, ref, n_local = local_map if local_map is not None else globals()["local_map"](obs_off, obs_kf, obs_kp, kf_desc, kf_oct, window)
    xyz = np.asarray(xyz, np.float32)
    pose = np.array(pose0, np.float64)
    res = {"n_local": n_local, "passes": [], "ok": False, "pose": pose.copy()}
    for k, rad in enumerate(radii):
        if poses is not None:
            pose = np.array(poses[k], np.float64)
        point, dist, nc = search(K, pose, xyz, rep, ref, kps, desc, w, h, rad, scale_factor, max_dist, ratio, octave_gate, scale_radius)
        used = rad
        if (point >= 0).sum() < min_matches:
            used = 2.0 * rad
            point, dist, nc = search(K, pose, xyz, rep, ref, kps, desc, w, h, used, scale_factor, max_dist, ratio, octave_gate, scale_radius)
        ps = {"point": point, "dist": dist, "cand": nc, "matches": int((point >= 0).sum()), "radius": used, "from": pose.copy()}
        res["passes"].append(ps)
        if ps["matches"] < min_matches:
            return res
        if not refine_pose:
            continue
        q = np.flatnonzero(point >= 0)
        pose, inl, n_inl = refine(K, pose, xyz[point[q]].astype(np.float64), np.column_stack([kps["x"][q], kps["y"][q]]).astype(np.float64),
                                  kps["octave"][q], scale_factor, chi2)
        ps.update(pose=pose.copy(), inlier=inl, inliers=n_inl)
        res["pose"] = pose.copy()
    res["ok"] = refine_pose and res["passes"][-1]["inliers"] >= min_inliers
    return res
