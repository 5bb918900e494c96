"""GPU: every two-view entry point against the f64 oracle in every regime of geom_oracle.REGIMES (motion direction, rotation,
parallax, depth range, focal length, principal point, noise, minimal and odd set sizes), one stage at a time: each stage gets the
inputs the oracle had, so that an error of one stage does not flow into the next.

  mo_triangulate_points  vs G.triangulate        (ground-truth P1 / P2; pixel and normalised; P scaled; far and behind; launch tails)
  mo_recover_pose        vs G.recover_pose        (ground-truth E scaled, negated, off rank 2; with and without a mask)
  mo_init_two_view       vs G.init_two_view       (staged and plain hypothesis scoring, the oracle's seed)
  mo_find_fundamental    vs G.find_fundamental_ransac8

Tolerances are 1e-4 relative or tighter unless a derivation stands next to them.  Every test prints its worst errors (pytest -s)."""
import numpy as np
import pytest

from oracle import geom_oracle as G

pytestmark = pytest.mark.gpu

REG = list(G.REGIMES)
EPS32 = 2.0 ** -24
EPS64 = 2.0 ** -53
DIST = 50.0  # the cheirality vote's depth cut (recoverPose)


@pytest.fixture(scope="module")
def ctx():
    import vslam_amd as V
    c = V.Context(device=0, max_w=1024, max_h=1024, max_batch=1)
    yield c
    c.close()


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


def skew(t):
    t = np.asarray(t, np.float64).ravel()
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def dlt_system(P1, P2, a1, a2):
    """(n, 4, 4) f64 DLT matrices of cv2.triangulatePoints (the rows G.triangulate builds)"""
    a1 = np.asarray(a1, np.float64); a2 = np.asarray(a2, np.float64)
    A = np.empty((len(a1), 4, 4))
    A[:, 0] = a1[:, 0:1] * P1[2] - P1[0]
    A[:, 1] = a1[:, 1:2] * P1[2] - P1[1]
    A[:, 2] = a2[:, 0:1] * P2[2] - P2[0]
    A[:, 3] = a2[:, 1:2] * P2[2] - P2[1]
    return A


# ---------------------------------------------------------------- mo_triangulate_points ----------------------------------------------
def well_conditioned(sv, X):
    """Points whose dehomogenised DLT solution both sides must reproduce to 1e-5: float32 rounding of the unit X4 is relative per
    component, so it moves X = X4[:3] / X4[3] by at most 2 * 2^-24 relative per coordinate; an error of angle theta in the f64 null
    vector moves X by theta (1 + |X|) sqrt(1 + |X|^2) / |X| relative, with theta <= 16 eps64 (s1 / s3)^2 for the kernel's normal
    equations and eps64 s1 / s3 for the reference's SVD.  Well conditioned: the sum predicts <= 1e-6, a tenth of what is asserted."""
    nX = np.linalg.norm(X, axis=1)
    k = sv[:, 0] / np.maximum(sv[:, 2], 1e-300)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pred = 4 * EPS32 + (16 * EPS64 * k * k + EPS64 * k) * (1 + nX) * np.sqrt(1 + nX ** 2) / nX
    return np.isfinite(pred) & (pred <= 1e-6)


def check_triangulation(ctx, P1, P2, a1, a2, tag):
    """Kernel X4 against the SVD null vector.  Returns (well-conditioned fraction, worst relative error there)."""
    a1 = np.ascontiguousarray(a1, np.float32); a2 = np.ascontiguousarray(a2, np.float32)
    X4 = ctx.triangulate_points(P1, P2, a1, a2)
    assert X4.shape == (len(a1), 4) and X4.dtype == np.float32
    if len(a1) == 0:
        return 1.0, 0.0
    x = X4.astype(np.float64)
    assert np.isfinite(x).all(), tag
    # unit length: the kernel normalises in f64 and rounds each component to float32 (relative error <= 2^-24 each), so the norm
    # is 1 within 2^-24 plus a few f64 roundings
    nrm = np.linalg.norm(x, axis=1)
    assert np.abs(nrm - 1.0).max() <= 1.5 * EPS32, (tag, np.abs(nrm - 1.0).max())
    xh = x / nrm[:, None]
    A = dlt_system(P1, P2, a1, a2)  # the kernel's inputs are these float32 pixels, so A is the same matrix up to f64 rounding
    sv = np.linalg.svd(A, compute_uv=False)
    # A residual bound that does not depend on conditioning: the exact null direction v4 leaves |A v4| = s4.  The kernel's f64
    # vector is the smallest eigenvector of A^T A (inverse iteration, shift 1e-15 tr): its angle to v4 is at most about
    # 16 eps64 s1^2 / (s3^2 - s4^2), which moves |A x| by at most s3 times that angle, <= 16 eps64 s1^2 / s3 (for s3 >> s4), and never
    # more than sqrt(16 eps64) s1.  Rounding to float32 moves x by at most 2^-24 (|x| = 1) and |A x| by at most s1 2^-24;
    # renormalising in f64 by <= 2^-24 |A x|.  c = 2 covers the two float32 terms.
    res = np.linalg.norm(np.einsum("nij,nj->ni", A, xh), axis=1)
    f64 = np.minimum(16 * EPS64 * sv[:, 0] ** 2 / np.maximum(sv[:, 2], 1e-300), np.sqrt(16 * EPS64) * sv[:, 0])
    bound = sv[:, 3] * (1 + 1e-12) + 2 * EPS32 * sv[:, 0] + f64
    bad = res > bound
    assert not bad.any(), (tag, int(bad.sum()), (res - bound).max() / sv[bad, 0].max())
    ref = G.triangulate(P1, P2, a1.astype(np.float64), a2.astype(np.float64))
    Xr = ref[:, :3] / ref[:, 3:4]
    well = well_conditioned(sv, Xr)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.linalg.norm(x[:, :3] / x[:, 3:4] - Xr, axis=1) / np.linalg.norm(Xr, axis=1)
    worst = float(e[well].max()) if well.any() else 0.0
    assert worst <= 1e-5, (tag, worst)
    return float(well.mean()), worst


@pytest.mark.parametrize("regime", REG)
def test_triangulate_points_regimes(ctx, regime):
    s = G.regime_scene(regime, outlier_frac=0.0)
    K = s["K"]
    Rt1 = np.hstack([np.eye(3), np.zeros((3, 1))]); Rt2 = np.hstack([s["R"], s["t"]])
    n1 = G.normalise(s["p1"], K).astype(np.float32); n2 = G.normalise(s["p2"], K).astype(np.float32)
    out = []
    for tag, P1, P2, a1, a2 in [("pixel", K @ Rt1, K @ Rt2, s["p1"], s["p2"]), ("normalised", Rt1, Rt2, n1, n2),
                                ("pixel*1e-3", 1e-3 * K @ Rt1, 1e-3 * K @ Rt2, s["p1"], s["p2"]),
                                ("pixel*1e3", 1e3 * K @ Rt1, 1e3 * K @ Rt2, s["p1"], s["p2"])]:
        frac, worst = check_triangulation(ctx, P1, P2, a1, a2, "%s %s" % (regime, tag))
        out.append("%s %.2f %.1e" % (tag, frac, worst))
        # the noise-free scenes' points lie within 120 baselines: most of them are well conditioned, so the 1e-5 check is not vacuous
        # (noise05: still well conditioned - the 4x4 system does not care whether the rays meet)
        assert frac > (0.3 if regime == "far" else 0.9), (regime, tag, frac)
        if tag == "pixel" and "noise_px" not in G.REGIMES[regime]:
            X4 = ctx.triangulate_points(P1, P2, a1, a2).astype(np.float64)
            # vs ground truth: the pixels carry float32 rounding (<= 2^-24 |u|), a relative perturbation of the rays that the
            # triangulation amplifies by depth / baseline (<= 120) and 1 / sin(parallax angle); 1e-3 covers the far scene's
            # 120-baseline points and the forward scenes' points next to the epipole
            e = np.linalg.norm(X4[:, :3] / X4[:, 3:4] - s["X"], axis=1) / np.linalg.norm(s["X"], axis=1)
            assert np.median(e) < 1e-5 and np.percentile(e, 99) < 1e-3, (regime, np.median(e), np.percentile(e, 99))
    print("triangulate %s: %s" % (regime, "; ".join(out)))


def test_triangulate_points_far_and_behind(ctx):
    """points up to 1e4 baselines away, and points behind the first, the second and both cameras"""
    rng = np.random.Generator(np.random.PCG64(5))
    K = np.array([[320.0, 0, 320.0], [0, 320.0, 240.0], [0, 0, 1.0]])
    R = G.rodrigues((0.01, -0.03, 0.02)); t = np.array([[0.8], [0.0], [0.6]])
    n = 4000
    # half far (4 - 1e4 baselines, log-uniform), a quarter behind both cameras, a quarter in the slab between the two camera planes
    z = np.concatenate([np.exp(rng.uniform(np.log(4), np.log(1e4), n // 2)), -rng.uniform(1, 20, n // 4), rng.uniform(-0.7, 0.1, n // 4)])
    X = np.stack([rng.uniform(-1, 1, n) * np.maximum(np.abs(z), 1), rng.uniform(-0.7, 0.7, n) * np.maximum(np.abs(z), 1), z], axis=1)
    Xc2 = X @ R.T + t.T
    p1 = (X @ K.T)[:, :2] / X[:, 2:3]; p2 = (Xc2 @ K.T)[:, :2] / Xc2[:, 2:3]
    b1, b2 = X[:, 2] < 0, Xc2[:, 2] < 0
    assert (b1 & b2).sum() > 500 and (b1 & ~b2).sum() > 100 and (~b1 & b2).sum() + (b1 & ~b2).sum() > 200
    P1 = K @ np.hstack([np.eye(3), np.zeros((3, 1))]); P2 = K @ np.hstack([R, t])
    ok = np.isfinite(p1).all(1) & np.isfinite(p2).all(1) & (np.abs(p1).max(1) < 1e7) & (np.abs(p2).max(1) < 1e7)
    frac, worst = check_triangulation(ctx, P1, P2, p1[ok], p2[ok], "far/behind")
    assert frac > 0.4
    print("triangulate far/behind: well %.2f worst %.1e" % (frac, worst))


@pytest.mark.parametrize("n", [0, 1, 127, 128, 129, 1000000])
def test_triangulate_points_launch_tail(ctx, n):
    s = G.synthetic_two_view(seed=100 + n % 1000, n=max(n, 1), outlier_frac=0.0)
    K = s["K"]
    P1 = K @ np.hstack([np.eye(3), np.zeros((3, 1))]); P2 = K @ np.hstack([s["R"], s["t"]])
    check_triangulation(ctx, P1, P2, s["p1"][:n], s["p2"][:n], "n=%d" % n)
    if n:
        X4 = ctx.triangulate_points(P1, P2, s["p1"][:n], s["p2"][:n])
        assert np.isfinite(X4).all() and (X4[:, 3] != 0).all()  # the last point of the tail block was written


# ---------------------------------------------------------------- mo_recover_pose ---------------------------------------------------
def oracle_depths(E, p1, p2, K):
    """depths of every correspondence in both cameras under the oracle's winning candidate (all points considered), and the absolute
    error those depths may carry in the kernel's vote.  The vote's DLT is the smallest eigenvector of A^T A by at most 8 steps of
    inverse iteration from (1/2, 1/2, 1/2, 1/2): each step shrinks tan(angle to the null vector v4) by r = (s4^2 + d) / (s3^2 + d)
    (d = 1e-15 tr, the shift), so after 8 steps the angle is at most r^8 tan(angle(start, v4)) - tiny for a correspondence whose rays
    meet (r ~ 0), not for an outlier whose rays miss each other (r up to 1).  On top: the f64 angle error 16 eps64 s1^2 / (s3^2 - s4^2)
    of the normal equations and eps64 s1 / (s3 - s4) of the reference's SVD.  An angle theta of the unit 4-vector moves the point,
    and so its depths, by at most theta (1 + |X|) sqrt(1 + |X|^2)."""
    _, R, t, _ = G.recover_pose(E, p1, p2, K, np.ones(len(p1), bool))
    x1, x2 = G.normalise(p1, K), G.normalise(p2, K)
    P0, P = np.hstack([np.eye(3), np.zeros((3, 1))]), np.hstack([R, t])
    A = dlt_system(P0, P, x1, x2)
    _, sv, Vt = np.linalg.svd(A)
    Q = Vt[:, -1, :]
    d = 1e-15 * (sv ** 2).sum(axis=1)
    r = (sv[:, 3] ** 2 + d) / (sv[:, 2] ** 2 + d)
    c0 = np.abs(Q.sum(axis=1)) / 2
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        tan0 = np.sqrt(np.maximum(1 - c0 * c0, 0)) / c0
        gap2, gap = sv[:, 2] ** 2 - sv[:, 3] ** 2, sv[:, 2] - sv[:, 3]
        theta = np.minimum(r ** 8 * tan0, 1e300) + 16 * EPS64 * sv[:, 0] ** 2 / gap2 + EPS64 * sv[:, 0] / gap
        q = Q[:, :3] / Q[:, 3:4]
        nq = np.linalg.norm(q, axis=1)
        err = theta * (1 + nq) * np.sqrt(1 + nq ** 2)
    z2 = q @ R[2] + t[2, 0]
    return q[:, 2], z2, err


@pytest.mark.parametrize("regime", REG)
def test_recover_pose_regimes(ctx, regime):
    s = G.regime_scene(regime)
    K, p1, p2, inl = s["K"], s["p1"], s["p2"], ~s["outlier"]
    E0 = skew(s["t"]) @ s["R"]
    U, _, Vt = np.linalg.svd(E0)
    variants = {"gt": E0, "x1e-6": 1e-6 * E0, "x1e6": 1e6 * E0, "neg": -E0,
                "rank3": U @ np.diag([1.0, 1.0, 1e-3]) @ Vt,  # sigma3 / sigma2 = 1e-3
                "rank3b": 2.5 * U @ np.diag([1.0, 1.0 - 1e-4, 3e-4]) @ Vt}
    z1, z2, err = oracle_depths(E0, p1, p2, K)
    # exemptions: points whose depth in either camera lies within 100 x that error (at least 1e-9) of 0 or of the cut at 50 - only
    # there may the kernel's vote and the oracle's SVD disagree
    with np.errstate(invalid="ignore"):
        mg = np.maximum(100 * np.nan_to_num(err, nan=np.inf), 1e-9)
        near = (np.abs(z1) < mg) | (np.abs(z2) < mg) | (np.abs(z1 - DIST) < mg) | (np.abs(z2 - DIST) < mg) | ~np.isfinite(z1)
    n_exempt, n_exempt_inl = int(near.sum()), int((near & inl).sum())
    worst = 0.0
    for name, E in variants.items():
        for mk in (inl, None):
            r = ctx.recover_pose(E, p1, p2, K, None if mk is None else mk.astype(np.uint8))
            on, oR, ot, om = G.recover_pose(E, p1, p2, K, np.ones(len(p1), bool) if mk is None else mk)
            tag = (regime, name, mk is None)
            # the ground-truth E of a scene is exact to f64, its decomposition is unique: both land on the true pose
            assert np.linalg.norm(r["R"] - oR) < 1e-9 and np.linalg.norm(r["t"] - ot) < 1e-9, tag
            assert np.linalg.norm(r["R"] - s["R"]) < 1e-9 and np.linalg.norm(r["t"] - s["t"]) < 1e-9, tag
            worst = max(worst, np.linalg.norm(r["R"] - oR), np.linalg.norm(r["t"] - ot))
            # pose mask and n_good: exact outside the exemption band
            diff = r["mask"] != om
            assert not (diff & ~near).any(), (tag, np.flatnonzero(diff & ~near)[:8])
            assert abs(r["n_good"] - on) <= int((diff & near).sum()) and r["n_good"] == int(r["mask"].sum()), tag
            if mk is not None:
                assert not r["mask"][~mk].any(), tag
            assert np.isnan(r["X"][~r["mask"]]).all() and not np.isnan(r["X"][r["mask"]]).any(), tag
    # the map points of the winning pose against the oracle's pixel-space DLT (1e-5 where well conditioned: see well_conditioned)
    r = ctx.recover_pose(E0, p1, p2, K, inl.astype(np.uint8))
    P1 = K @ np.hstack([np.eye(3), np.zeros((3, 1))]); P2 = K @ np.hstack([s["R"], s["t"]])
    m = r["mask"]
    if m.any():
        Q = G.triangulate(P1, P2, p1[m].astype(np.float64), p2[m].astype(np.float64))
        Xo = Q[:, :3] / Q[:, 3:4]
        e = np.linalg.norm(r["X"][m] - Xo, axis=1) / np.linalg.norm(Xo, axis=1)
        sel = well_conditioned(np.linalg.svd(dlt_system(P1, P2, p1[m], p2[m]), compute_uv=False), Xo)
        assert sel.mean() > 0.5 and e[sel].max() < 1e-5 and np.median(e) < 1e-5, (regime, sel.mean(), e.max())
    print("recover_pose %s: worst R/t vs oracle %.1e, exempt near depth 0 / 50: %d (true correspondences among them: %d)"
          % (regime, worst, n_exempt, n_exempt_inl))


def test_recover_pose_empty_mask_is_well_formed(ctx):
    s = G.regime_scene("sideways")
    E = skew(s["t"]) @ s["R"]
    r = ctx.recover_pose(E, s["p1"], s["p2"], s["K"], np.zeros(len(s["p1"]), np.uint8))
    # all four candidates tie at 0: which one wins depends on the SVD basis, so only the shape of the answer is asserted
    R, t = r["R"], r["t"].ravel()
    assert r["n_good"] == 0 and not r["mask"].any() and np.isnan(r["X"]).all()
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12 and abs(np.linalg.norm(t) - 1) < 1e-12


# ---------------------------------------------------------------- mo_init_two_view --------------------------------------------------
@pytest.mark.parametrize("n_hyp", [4096, 300])  # staged scoring (f32 lower bound + f64 survivors) and plain scoring
@pytest.mark.parametrize("regime", REG)
def test_init_two_view_regimes(ctx, regime, n_hyp):
    s = G.regime_scene(regime)
    g = ctx.init_two_view(s["p1"], s["p2"], s["K"], thr_px=3.0, n_hyp=n_hyp, seed=4096)
    o = G.init_two_view(s["p1"], s["p2"], s["K"], thr_px=3.0, n_hyp=n_hyp, seed=4096)
    assert o["R"] is not None and not np.isnan(g["R"]).any(), regime
    # same samples, same exact argmin, same refits: kernel and oracle agree to 1e-4 in every regime, low parallax and noise included
    eR, et = rel(g["R"], o["R"]), rel(g["t"], o["t"])
    Eg, Eo = g["E"] / np.linalg.norm(g["E"]), o["E"] / np.linalg.norm(o["E"])
    eE = min(rel(Eg, Eo), rel(-Eg, Eo))
    fr = int((g["ransac_mask"] != o["ransac_mask"]).sum()); fp = int((g["pose_mask"] != o["pose_mask"]).sum())
    both = g["pose_mask"] & o["pose_mask"]
    eX = np.linalg.norm(g["X"][both] - o["X"][both], axis=1) / np.linalg.norm(o["X"][both], axis=1)
    eXm = float(eX.max()) if both.any() else 0.0
    print("init_two_view %s n_hyp=%d: R %.1e t %.1e E %.1e X %.1e flips %d/%d n_good %d/%d"
          % (regime, n_hyp, eR, et, eE, eXm, fr, fp, g["n_good"], o["n_good"]))
    assert eR < 1e-4 and et < 1e-4 and eE < 1e-4, (regime, eR, et, eE)
    assert fr <= 2 and fp <= 2 and abs(g["n_good"] - o["n_good"]) <= 2, (regime, fr, fp)
    assert eXm < 1e-4, (regime, eXm)
    assert np.isnan(g["X"][~g["pose_mask"]]).all() and not np.isnan(g["X"][g["pose_mask"]]).any()
    # ground truth: the noise-free regimes reach the true pose to 1e-3 (chance inliers of the 3 px threshold bias the refit: the
    # oracle's own distance on these scenes is at most 3.4e-3 on t at 1.5 px of parallax, see test_oracle_geom.py)
    if "noise_px" not in G.REGIMES[regime] and regime != "low_parallax":
        assert rel(g["R"], s["R"]) < 1e-3 and rel(g["t"], s["t"]) < 1e-3, regime


# ---------------------------------------------------------------- mo_find_fundamental -----------------------------------------------
def _epi_dist(F, p1, p2):
    h1 = np.concatenate([p1, np.ones((len(p1), 1))], 1); h2 = np.concatenate([p2, np.ones((len(p2), 1))], 1)
    l2 = h1 @ F.T; l1 = h2 @ F
    num = np.abs((h2 * l2).sum(1))
    return np.maximum(num / np.hypot(l2[:, 0], l2[:, 1]), num / np.hypot(l1[:, 0], l1[:, 1]))


@pytest.mark.parametrize("regime", REG)
def test_find_fundamental_regimes(ctx, regime):
    s = G.regime_scene(regime)
    F, mask = ctx.find_fundamental(s["p1"], s["p2"], thr_px=3.0, n_hyp=2048, seed=77)
    Fo, mo = G.find_fundamental_ransac8(s["p1"], s["p2"], thr_px=3.0, n_hyp=2048, seed=77)
    assert F is not None and Fo is not None, regime
    # compared at unit norm: F is returned scaled to F33 = 1, and F33 is a small cancellation term when the epipole sits near the
    # principal point (forward / backward motion), which would magnify the difference of two matrices 1e-8 apart
    Fu, Fou = F / np.linalg.norm(F), Fo / np.linalg.norm(Fo)
    eF = min(rel(Fu, Fou), rel(-Fu, Fou))
    flips = int((mask != mo).sum())
    inl = ~s["outlier"]
    ed = _epi_dist(F, s["p1"][inl].astype(np.float64), s["p2"][inl].astype(np.float64))
    print("find_fundamental %s: F %.1e flips %d epipolar max %.2e px" % (regime, eF, flips, ed.max()))
    assert eF < 1e-4 and flips <= 2, (regime, eF, flips)
    assert abs(np.linalg.det(F)) < 1e-9 * np.linalg.norm(F) ** 3
    if regime == "low_parallax":
        # 1.5 px of parallax under a 3 px threshold: outliers within 3 px of their epipolar line are many (about 2 % of the scene)
        # and enter the least-squares refits of BOTH implementations, tilting F; the true inliers stay within a third of the threshold
        assert ed.max() < 1.0 and mask[inl].mean() > 0.99
    elif "noise_px" in G.REGIMES[regime]:
        # N(0, 0.5) on both images: the distance of a point to its line is a difference of two noisy coordinates (sigma 0.5 sqrt 2)
        assert np.median(ed) < 0.7 and mask[inl].mean() > 0.97
    else:
        assert ed.max() < 0.05 and mask[inl].mean() > 0.99, regime
