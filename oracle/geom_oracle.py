"""oracle/geom_oracle.py -- TEST INFRASTRUCTURE ONLY (CPU restatement of the two-view stage, numpy f64).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.

What it restates: the geometry behind the reference's MapInitializer.initialize
  /root/reference/src/orbslam2/initializer.py:79   calculate_essential_matrix(p1, p2, K, threshold=3.0)
  /root/reference/src/orbslam2/utils.py:120-126    cv2.findEssentialMat(..., RANSAC, prob, threshold)
  /root/reference/src/orbslam2/utils.py:129-134    cv2.recoverPose(E, p1, p2, K, mask)
  /root/reference/src/orbslam2/utils.py:56-70      cv2.triangulatePoints + divide by w
The arithmetic lives in the absent, unpinned cv2 wheel.  cv2.findEssentialMat is a sequential 5-point RANSAC;
north_star prescribes an 8-point RANSAC over a fixed number of hypotheses scored in parallel, so this oracle
restates THAT algorithm (same counter-based sampling as the HIP kernels, independent linear algebra: numpy
SVDs instead of the kernels' Gauss-Jordan / Jacobi solvers).  PARITY UNPINNED against cv2: no fixture of the
reference holds E, R, t or 3-D points; results are checked against synthetic ground truth and against the
HIP path at 1e-4 relative.  recoverPose and triangulatePoints follow OpenCV's published algorithm (SVD
decomposition, W matrix, cheirality vote with depth in (0, 50), per-point 4x4 DLT null vector).
"""
import numpy as np

M64 = (1 << 64) - 1


def _splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return state, z ^ (z >> 31)


def sample8(seed, h, m, pair=0):
    """8 distinct correspondence indices of hypothesis h (same stream as twoview_kernels.hip sample8)."""
    seed = (seed + pair * 0x632BE59BD9B4E019) & M64
    s = (seed + (h + 1) * 0xD1B54A32D192ED03) & M64
    idx = []
    while len(idx) < 8:
        s, r = _splitmix64(s)
        c = r % m
        if c not in idx:
            idx.append(c)
    return idx


def normalise(p, K):
    p = np.asarray(p, np.float32).astype(np.float64)
    return np.stack([(p[:, 0] - K[0, 2]) / K[0, 0], (p[:, 1] - K[1, 2]) / K[1, 1]], axis=1)


def _design(x1, x2):
    return np.stack([x2[:, 0] * x1[:, 0], x2[:, 0] * x1[:, 1], x2[:, 0], x2[:, 1] * x1[:, 0], x2[:, 1] * x1[:, 1],
                     x2[:, 1], x1[:, 0], x1[:, 1], np.ones(len(x1))], axis=1)


def _design9(x1, x2):
    """the design matrix, padded with zero rows to 9: a reduced SVD of 8 rows has no 9th right singular vector (the null vector)"""
    A = _design(x1, x2)
    return A if len(A) >= 9 else np.vstack([A, np.zeros((9 - len(A), 9))])


def project_essential(E):
    U, s, Vt = np.linalg.svd(E)
    return U @ np.diag([1.0, 1.0, 0.0]) @ Vt


def sampson(E, x1, x2):
    """E (...,3,3), x1/x2 (M,2) -> (..., M) Sampson distance x2^T E x1 squared over the gradient norm"""
    h1 = np.concatenate([x1, np.ones((len(x1), 1))], axis=1)
    h2 = np.concatenate([x2, np.ones((len(x2), 1))], axis=1)
    Ex1 = np.einsum("...ij,mj->...mi", E, h1)
    Etx2 = np.einsum("...ji,mj->...mi", E, h2)
    num = np.einsum("...mi,mi->...m", Ex1, h2)
    den = Ex1[..., 0] ** 2 + Ex1[..., 1] ** 2 + Etx2[..., 0] ** 2 + Etx2[..., 1] ** 2
    return num * num / den


def find_essential_ransac8(p1, p2, K, thr_px=3.0, n_hyp=4096, seed=4096, pair=0, chunk=512):
    K = np.asarray(K, np.float64).reshape(3, 3)
    x1, x2 = normalise(p1, K), normalise(p2, K)
    m = len(x1)
    if m < 8:
        return None, np.zeros(m, bool)
    thr = thr_px / ((K[0, 0] + K[1, 1]) / 2.0)
    thr2 = thr * thr
    samples = np.array([sample8(seed, h, m, pair) for h in range(n_hyp)])
    A = _design(x1[samples.ravel()], x2[samples.ravel()]).reshape(n_hyp, 8, 9)
    _, _, Vt = np.linalg.svd(A)
    Es = Vt[:, -1, :].reshape(n_hyp, 3, 3)
    U, s, Vt3 = np.linalg.svd(Es)
    Es = U[:, :, :2] @ Vt3[:, :2, :]
    # MSAC score: sum of Sampson distances truncated at thr^2 (a pure inlier count would prefer slightly
    # perturbed models that catch more chance inliers); compared in float32, ties -> lowest hypothesis index
    cost = np.full(n_hyp, np.inf, np.float32)
    for a in range(0, n_hyp, chunk):
        d = sampson(Es[a:a + chunk], x1, x2)
        cost[a:a + chunk] = np.minimum(d, thr2).sum(axis=1).astype(np.float32)
    hbest = int(np.argmin(cost))
    E = Es[hbest]
    n0 = int((sampson(E, x1, x2) <= thr2).sum())
    if n0 < 8:
        return None, np.zeros(m, bool)
    # local optimisation: least-squares 8-point refits on an adaptively tightened consensus set.  The selection
    # threshold follows a 3-sigma rule on the mean Sampson residual of the previous selection (clamped to
    # [thr/64, thr]), so chance inliers of the loose RANSAC threshold do not bias the algebraic fit; a refit is
    # only accepted while at least half of the original consensus is still selected.
    lo2 = thr2 / 4096.0
    d = sampson(E, x1, x2)
    sel = d <= thr2
    tau2 = min(max(9.0 * float(d[sel].sum()) / int(sel.sum()), lo2), thr2)
    c_prev, tau2_prev = -1, -1.0
    for _ in range(5):
        d = sampson(E, x1, x2)
        sel = d <= tau2
        c = int(sel.sum())
        if c < 8 or 2 * c < n0:
            break
        if c == c_prev and tau2 == tau2_prev:  # same selection size at the same threshold: converged
            break
        c_prev, tau2_prev = c, tau2
        _, _, Vt = np.linalg.svd(_design9(x1[sel], x2[sel]), full_matrices=False)
        E = project_essential(Vt[-1].reshape(3, 3))
        tau2 = min(max(9.0 * float(d[sel].sum()) / c, lo2), thr2)
    mask = sampson(E, x1, x2) <= thr2
    return E, mask


def triangulate(P1, P2, a1, a2):
    """cv2.triangulatePoints: per point the right singular vector of the smallest singular value -> (N,4) f64"""
    n = len(a1)
    A = np.empty((n, 4, 4))
    A[:, 0] = a1[:, 0:1] * P1[2] - P1[0]
    A[:, 1] = a1[:, 1:2] * P1[2] - P1[1]
    A[:, 2] = a2[:, 0:1] * P2[2] - P2[0]
    A[:, 3] = a2[:, 1:2] * P2[2] - P2[1]
    _, _, Vt = np.linalg.svd(A)
    return Vt[:, -1, :]


def recover_pose(E, p1, p2, K, mask, dist=50.0):
    K = np.asarray(K, np.float64).reshape(3, 3)
    x1, x2 = normalise(p1, K), normalise(p2, K)
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1.0]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2:3]
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    cands = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    masks = []
    for R, tt in cands:
        P = np.hstack([R, tt])
        Q = triangulate(P0, P, x1, x2)
        ok = Q[:, 2] * Q[:, 3] > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            q = Q[:, :3] / Q[:, 3:4]
        ok &= q[:, 2] < dist
        z2 = (P @ np.concatenate([q, np.ones((len(q), 1))], axis=1).T)[2]
        ok &= (z2 > 0) & (z2 < dist)
        masks.append(ok & mask)
    good = [int(mk.sum()) for mk in masks]
    if good[0] >= good[1] and good[0] >= good[2] and good[0] >= good[3]: w = 0
    elif good[1] >= good[0] and good[1] >= good[2] and good[1] >= good[3]: w = 1
    elif good[2] >= good[0] and good[2] >= good[1] and good[2] >= good[3]: w = 2
    else: w = 3
    return good[w], cands[w][0], cands[w][1], masks[w]


def init_two_view(p1, p2, K, thr_px=3.0, n_hyp=4096, seed=4096, pair=0):
    """-> dict(E, R, t, ransac_mask, pose_mask, X (M,3) f32 with NaN outside pose_mask, n_good)"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    p1 = np.asarray(p1, np.float32); p2 = np.asarray(p2, np.float32)
    E, mask = find_essential_ransac8(p1, p2, K, thr_px, n_hyp, seed, pair)
    if E is None:
        return dict(E=None, R=None, t=None, ransac_mask=mask, pose_mask=mask, X=np.full((len(p1), 3), np.nan, np.float32), n_good=0)
    n_good, R, t, pmask = recover_pose(E, p1, p2, K, mask)
    P1 = K @ np.hstack([np.eye(3), np.zeros((3, 1))])
    P2 = K @ np.hstack([R, t])
    X = np.full((len(p1), 3), np.nan, np.float32)
    if pmask.any():
        X4 = triangulate(P1, P2, p1[pmask].astype(np.float64), p2[pmask].astype(np.float64)).astype(np.float32)
        X[pmask] = X4[:, :3] / X4[:, 3:4]
    return dict(E=E, R=R, t=t, ransac_mask=mask, pose_mask=pmask, X=X, n_good=n_good)


def rodrigues(rv):
    rv = np.asarray(rv, np.float64)
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def synthetic_two_view(seed=4096, n=2000, outlier_frac=0.3, K=None, w=640, h=480, rv=(0.02, -0.05, 0.01), t_dir=(1.0, 0.1, 0.05),
                       depth=None, noise_px=0.0, plane=None):
    """seeded two-view problem with ground truth.  X2 = R X1 + t with |t| = 1 (depths are in baselines).
    With the defaults (depth=None) the points fill the box [-4, 4]^2 x [4, 12] in front of camera 1, as this scene always did (many
    project outside the image).  depth=(lo, hi): every point is seen by both cameras - a pixel drawn uniformly in image 1 at a depth
    drawn uniformly in [lo, hi], kept only when it projects inside image 2 in front of camera 2.  noise_px: N(0, noise_px) added to
    both images' pixel coordinates of every point (drawn last, so the noise-free scene is the same).  plane=(nx, ny, nz, d, th):
    instead of a depth range, each point lies on the plane n.X = d of camera 1, its depth scaled by a factor drawn in [1 - th, 1 + th].
    -> dict(K, p1, p2 (float32 pixels), R, t (3, 1), X (n, 3) in camera 1, z1 / z2 (n,) true depths in camera 1 / 2, outlier (n,))"""
    rng = np.random.Generator(np.random.PCG64(seed))
    if K is None:
        K = np.array([[320.0, 0, 320.0], [0, 320.0, 240.0], [0, 0, 1.0]])
    K = np.asarray(K, np.float64)
    R = rodrigues(rv)
    t = np.asarray(t_dir, np.float64).copy(); t /= np.linalg.norm(t)
    if depth is None:
        X = np.stack([rng.uniform(-4, 4, n), rng.uniform(-4, 4, n), rng.uniform(4, 12, n)], axis=1)
    else:
        Ki = np.linalg.inv(K)
        X = np.empty((0, 3))
        while len(X) < n:
            k = 2 * (n - len(X)) + 64
            uv = np.stack([rng.uniform(0, w, k), rng.uniform(0, h, k), np.ones(k)], axis=1)
            ray = (Ki @ uv.T).T
            if plane is None:
                Xk = ray * rng.uniform(depth[0], depth[1], k)[:, None]
            else:
                Xk = ray * (plane[3] / (ray @ np.asarray(plane[:3], np.float64)) * rng.uniform(1 - plane[4], 1 + plane[4], k))[:, None]
            q = (K @ ((R @ Xk.T).T + t).T).T
            with np.errstate(divide="ignore", invalid="ignore"):
                ok = (q[:, 2] > 0) & (q[:, 0] >= 0) & (q[:, 0] <= w * q[:, 2]) & (q[:, 1] >= 0) & (q[:, 1] <= h * q[:, 2])
            X = np.concatenate([X, Xk[ok]])[:n]
    x1 = (K @ X.T).T; p1 = x1[:, :2] / x1[:, 2:3]
    Xc2 = (R @ X.T).T + t
    x2 = (K @ Xc2.T).T; p2 = x2[:, :2] / x2[:, 2:3]
    p1 = p1.astype(np.float32); p2 = p2.astype(np.float32)
    out = rng.random(n) < outlier_frac
    no = int(out.sum())
    p2[out] = np.stack([rng.uniform(0, w, no), rng.uniform(0, h, no)], axis=1).astype(np.float32)
    if noise_px > 0:
        p1 = (p1 + rng.normal(0, noise_px, p1.shape)).astype(np.float32)
        p2 = (p2 + rng.normal(0, noise_px, p2.shape)).astype(np.float32)
    return dict(K=K, p1=p1, p2=p2, R=R, t=t.reshape(3, 1), X=X, z1=X[:, 2].copy(), z2=Xc2[:, 2].copy(), outlier=out)


# Two-view regimes shared by tests/test_oracle_geom.py (the oracle recovers ground truth) and tests/test_gpu_geometry_regimes.py
# (every two-view entry point against the oracle): keyword arguments of synthetic_two_view.  All but "sideways" see every point in
# both images.  Disparities: sideways motion at depth z moves a point by f / z pixels.
_K320 = ((320.0, 0, 320.0), (0, 320.0, 240.0), (0, 0, 1.0))
REGIMES = {
    "sideways": dict(),                                                                  # today's scene, exactly
    "forward": dict(t_dir=(0.0, 0.0, -1.0), depth=(4, 12)),                              # camera 2 moves forward: epipole at the centre
    "backward": dict(t_dir=(0.05, -0.03, 1.0), depth=(4, 12)),                           # camera 2 moves back; epipole in the image
    "diagonal": dict(t_dir=(1.0, 1.0, 1.0), depth=(4, 12)),
    "rot15": dict(rv=tuple(np.radians(15.0) * np.array([0.2, 1.0, 0.3]) / np.linalg.norm([0.2, 1.0, 0.3])), depth=(4, 12)),
    "rot30": dict(rv=tuple(np.radians(30.0) * np.array([0.3, 0.2, 1.0]) / np.linalg.norm([0.3, 0.2, 1.0])), depth=(4, 12)),
    # f = 80: 1.8 - 3.2 px of parallax at 25 - 45 baselines, inside the depth cut of 50 (at f = 320 the same parallax lies at
    # 100 - 300 baselines, where the cheirality vote keeps nothing)
    "low_parallax": dict(K=((80.0, 0, 160.0), (0, 80.0, 120.0), (0, 0, 1.0)), w=320, h=240, depth=(25, 45), rv=(0.002, -0.005, 0.001)),
    "far": dict(depth=(4, 120)),                                                         # part of the scene beyond the depth cut
    "long_f": dict(K=((3000.0, 0, 1920.0), (0, 3000.0, 1080.0), (0, 0, 1.0)), w=3840, h=2160, depth=(4, 12)),
    "short_f": dict(K=((150.0, 0, 320.0), (0, 150.0, 240.0), (0, 0, 1.0)), w=640, h=480, depth=(4, 12)),  # |x_n| up to 2.1
    "aniso": dict(K=((300.0, 0, 448.0), (0, 345.0, 144.0), (0, 0, 1.0)), depth=(4, 12)),  # fx != fy, centre off by 20 % of w / h
    "noise05": dict(depth=(4, 12), noise_px=0.5),
    # near-planar (depths within 5 % of a tilted plane at 8 baselines), 0.5 px noise, no outliers: a plane leaves the 8-point design
    # a 3-dimensional null space, so the two smallest eigenvalues of the refits' normal matrix lie close together (ratio 0.9 here) -
    # the case wave_smallest_eigvec9's repeated squaring of the inverse exists for
    "planar": dict(depth=(0, 0), plane=(0.3, 0.2, 1.0, 8.0, 0.05), noise_px=0.5, outlier_frac=0.0),
    "min8": dict(depth=(4, 12), n=8, outlier_frac=0.0),
    "min9": dict(depth=(4, 12), n=9, outlier_frac=0.0),
    "m4097": dict(depth=(4, 12), n=4097),
}


def regime_scene(name, seed=4096, n=2000, outlier_frac=0.3):
    kw = dict(REGIMES[name])
    kw.setdefault("n", n)
    kw.setdefault("outlier_frac", outlier_frac)
    if "K" in kw:
        kw["K"] = np.array(kw["K"], np.float64)
    return synthetic_two_view(seed=seed, **kw)


# ---- tracking step (reference src/orbslam2/tracker.py:214-254) -------------------------------------------------------
def track_select(xy1, xy2, idx, dist, keep, width, height, frac=0.02):
    """The two match filters Tracker._track_from_last_frame applies between matcher.match and findEssentialMat:
      matcher.py:109-142  filter_matches_by_geometric_distance: keep hypot(pt2 - pt1) <= ((w + h) / 2) * frac   (Python floats)
      matcher.py:144-169  filter_matches_by_distance: stable sort by distance, keep distance < 2 * np.median(distances)
    xy1 / xy2: (N, 2) float32 keypoint coordinates of the previous / current frame; idx, dist, keep: knn output of
    matcher.match(prev, cur) (query = previous frame).  -> (queryIdx, trainIdx, distance) arrays in the reference's order."""
    import math
    q = np.nonzero(np.asarray(keep))[0]
    t = np.asarray(idx)[q, 0]
    d = np.asarray(dist)[q, 0]
    limit = ((width + height) / 2.0) * frac
    ok = np.array([math.hypot(float(xy2[b, 0]) - float(xy1[a, 0]), float(xy2[b, 1]) - float(xy1[a, 1])) <= limit
                   for a, b in zip(q, t)], bool)
    q, t, d = q[ok], t[ok], d[ok]
    if len(q) == 0:
        return q, t, d
    order = np.argsort(d, kind="stable")  # Python's sorted() is stable: ties stay in query order
    q, t, d = q[order], t[order], d[order]
    thr = float(np.median(d.astype(np.float64))) * 2.0
    k = d.astype(np.float64) < thr
    return q[k], t[k], d[k]


def track_pair(xy1, xy2, idx, dist, keep, K, width, height, frac=0.02, thr_px=1.0, n_hyp=4096, seed=4096, pair=0):
    """tracker.py:214-254: filters above, then E-RANSAC at 1 px and recoverPose on the selected matches (in that order)."""
    q, t, d = track_select(xy1, xy2, idx, dist, keep, width, height, frac)
    out = dict(sel_q=q, sel_t=t, sel_d=d, R=None, t=None, pose_mask=np.zeros(len(q), bool), n_good=0)
    if len(q) < 8:  # tracker.py:234
        return out
    r = init_two_view(np.asarray(xy1, np.float32)[q], np.asarray(xy2, np.float32)[t], K, thr_px, n_hyp, seed, pair)
    out.update(R=r["R"], t=r["t"], E=r["E"], pose_mask=r["pose_mask"], ransac_mask=r["ransac_mask"], n_good=r["n_good"], X=r["X"])
    return out


# ---- fundamental matrix (reference matcher.py:191, local_mapper.py:136: cv2.findFundamentalMat(p1, p2, FM_RANSAC, thr, prob)) ---
def find_fundamental_ransac8(p1, p2, thr_px=3.0, n_hyp=4096, seed=4096, pair=0, chunk=512):
    """8-point fundamental-matrix RANSAC over a fixed number of hypotheses, same structure and sampling stream as
    find_essential_ransac8 (cv2's FM_RANSAC is a sequential 7-point RANSAC: PARITY UNPINNED against cv2, pinned against the HIP
    path and synthetic ground truth).  Pixel coordinates are Hartley-normalised x_n = s (x - centroid) with ONE scale for both
    images (mean distance from the centroids -> sqrt 2), so Sampson distances scale by s^2 and the threshold is thr_px * s.
    -> (F 3x3 scaled to F[2,2] = 1, or None; mask (M,) bool)"""
    p1 = np.asarray(p1, np.float32).astype(np.float64); p2 = np.asarray(p2, np.float32).astype(np.float64)
    m = len(p1)
    if m < 8:
        return None, np.zeros(m, bool)
    c1, c2 = p1.mean(axis=0), p2.mean(axis=0)
    mean = (np.linalg.norm(p1 - c1, axis=1).sum() + np.linalg.norm(p2 - c2, axis=1).sum()) / (2.0 * m)
    s = np.sqrt(2.0) / mean if mean > 1e-12 else 1.0
    x1, x2 = s * (p1 - c1), s * (p2 - c2)
    thr2 = (thr_px * s) ** 2

    def rank2(F):
        U, sv, Vt = np.linalg.svd(F)
        sv = sv.copy(); sv[..., 2] = 0.0
        return (U * sv[..., None, :]) @ Vt

    samples = np.array([sample8(seed, h, m, pair) for h in range(n_hyp)])
    A = _design(x1[samples.ravel()], x2[samples.ravel()]).reshape(n_hyp, 8, 9)
    _, _, Vt = np.linalg.svd(A)
    Fs = rank2(Vt[:, -1, :].reshape(n_hyp, 3, 3))
    cost = np.full(n_hyp, np.inf, np.float32)
    for a in range(0, n_hyp, chunk):
        d = sampson(Fs[a:a + chunk], x1, x2)
        cost[a:a + chunk] = np.minimum(d, thr2).sum(axis=1).astype(np.float32)
    F = Fs[int(np.argmin(cost))]
    n0 = int((sampson(F, x1, x2) <= thr2).sum())
    if n0 < 8:
        return None, np.zeros(m, bool)
    lo2 = thr2 / 4096.0
    d = sampson(F, x1, x2)
    sel = d <= thr2
    tau2 = min(max(9.0 * float(d[sel].sum()) / int(sel.sum()), lo2), thr2)
    c_prev, tau2_prev = -1, -1.0
    for _ in range(5):  # same adaptive-threshold refits as the essential model
        d = sampson(F, x1, x2)
        sel = d <= tau2
        c = int(sel.sum())
        if c < 8 or 2 * c < n0:
            break
        if c == c_prev and tau2 == tau2_prev:
            break
        c_prev, tau2_prev = c, tau2
        _, _, Vt = np.linalg.svd(_design9(x1[sel], x2[sel]), full_matrices=False)
        F = rank2(Vt[-1].reshape(3, 3))
        tau2 = min(max(9.0 * float(d[sel].sum()) / c, lo2), thr2)
    mask = sampson(F, x1, x2) <= thr2
    T1 = np.array([[s, 0, -s * c1[0]], [0, s, -s * c1[1]], [0, 0, 1.0]])
    T2 = np.array([[s, 0, -s * c2[0]], [0, s, -s * c2[1]], [0, 0, 1.0]])
    Fp = T2.T @ F @ T1
    nn = np.linalg.norm(Fp)
    Fp = Fp / Fp[2, 2] if abs(Fp[2, 2]) > 1e-12 * nn else Fp / nn
    return Fp, mask


# ---- undistort (reference src/orbslam2/utils.py:40-52: cv2.undistort(image, camera_matrix, distortion)) ------------------------
def undistort(image, K, dist):
    """cv2.undistort for uint8 images restated from OpenCV's published pipeline (PARITY UNPINNED against cv2: the reference holds
    no undistorted fixture): initUndistortRectifyMap(K, dist, I, K, CV_16SC2) in double, map quantised to 1/32 px with
    round-half-even, remap(INTER_LINEAR, BORDER_CONSTANT 0) with the exact fixed-point bilinear table of 32 steps:
    out = (sum (32 - a | a)(32 - b | b) p + 512) >> 10."""
    img = np.asarray(image, np.uint8)
    h, w = img.shape[:2]
    K = np.asarray(K, np.float64).reshape(3, 3)
    d = np.zeros(5); dd = np.asarray(dist, np.float64).ravel(); d[:min(5, len(dd))] = dd[:5]
    k1, k2, p1, p2, k3 = d
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    x = (j - K[0, 2]) / K[0, 0]; y = (i - K[1, 2]) / K[1, 1]
    x2, y2 = x * x, y * y
    r2 = x2 + y2; xy2 = 2 * x * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * kr + p1 * xy2 + p2 * (r2 + 2 * x2); yd = y * kr + p1 * (r2 + 2 * y2) + p2 * xy2
    u = K[0, 0] * xd + K[0, 2]; v = K[1, 1] * yd + K[1, 2]
    iu = np.rint(np.clip(u * 32.0, -1e8, 1e8)).astype(np.int64); iv = np.rint(np.clip(v * 32.0, -1e8, 1e8)).astype(np.int64)
    sx, sy, a, b = iu >> 5, iv >> 5, iu & 31, iv & 31
    src = img.reshape(h, w, -1).astype(np.int64)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(ok[..., None], src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0)

    acc = ((32 - a) * (32 - b))[..., None] * tap(sy, sx) + (a * (32 - b))[..., None] * tap(sy, sx + 1) + \
          ((32 - a) * b)[..., None] * tap(sy + 1, sx) + (a * b)[..., None] * tap(sy + 1, sx + 1)
    return ((acc + 512) >> 10).astype(np.uint8).reshape(img.shape)
