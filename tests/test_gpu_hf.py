"""GPU tests of the homography branch of the two-view stage and the H / F model selection (mo_init_two_view_hf, twoview_h.hip)
against the numpy restatement (tests/hf_restatement.py) on the scenes of tests/hf_cases.py.

Integers (model, accepted, winning hypothesis, best and second candidate, masks, good counts) must be equal: tests/test_hf_cpu.py
asserts that no case has a compared error within 1e-9 relative of its threshold nor two best hypothesis costs within 1e-6.

Values are bounded by ten times the restatement's own SVD-versus-eigh difference on the same case PLUS a floor from the number
format, because that self-difference is often exactly 0 (both formulations round to the same bits) while the device sums in another
order (block reductions against numpy's pairwise sums) and solves with other, equally valid roundings:
  H, R, t (unit norm)   64 eps = 1.4e-14
  SH, SF                m eps relative (m non-negative terms summed in another order)
  RH                    2 m eps
  parallax (degrees)    4 ulps of its cos through acos: 4 eps / sin(parallax) in radians
  X (float32 output)    2^-23 relative: a float64 value next to a rounding boundary lands on either side
SF and RH are compared given the E the homography chain was fed, the device's own: the essential path is checked against the oracle
at 1e-4 by its own tests and is not identifiable on a plane, where two valid solvers return different members of a family.
Measured worst values and bounds: profiles/hf_parity.txt."""
import numpy as np
import pytest

from tests import hf_cases as C
from tests import hf_restatement as HR

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def ctx():
    import vslam_amd as V
    c = V.Context(device=0, max_w=1024, max_h=1024, max_batch=4)
    yield c
    c.close()


_device = {}


def device(ctx, name):
    """the device's result on a case, computed once and shared (tests do not modify it)"""
    if name not in _device:
        s = C.scene(name)
        _device[name] = ctx.init_two_view_hf(s["p1"], s["p2"], s["K"], **C.call_kw(name))
    return _device[name]


def _unit_fixed(H):
    H = np.asarray(H, np.float64) / np.linalg.norm(H)
    return H * np.sign(H.flat[int(np.argmax(np.abs(H)))])


def _same_bytes(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a)


def _assert_integers(g, r, what):
    assert g["model"] == r["model"] and g["accepted"] == r["accepted"], (what, g["model"], r["model"], g["accepted"], r["accepted"])
    assert g["winner_h"] == r["winner_h"] and g["refits_h"] == r["refits_h"], (what, g["winner_h"], r["winner_h"])
    assert g["best_h"] == r["best_h"] and g["second_h"] == r["second_h"], (what, g["best_h"], r["best_h"], g["second_h"], r["second_h"])
    assert np.array_equal(g["h_mask"], r["h_mask"]) and g["n_inliers_h"] == r["n_inliers_h"], what
    assert np.array_equal(g["n_good_h"], r["n_good_h"]), (what, g["n_good_h"], r["n_good_h"])
    assert np.array_equal(g["pose_mask"], r["pose_mask"]) and g["n_good"] == r["n_good"], what


@pytest.mark.parametrize("name", list(C.CASES))
def test_integers_equal_the_restatement(ctx, name):
    _assert_integers(device(ctx, name), C.restated(name), name)


@pytest.mark.parametrize("name", [k for k, (_, e) in C.CASES.items() if e == "H"])
def test_planes_initialise_through_the_homography(ctx, name):
    """the capability: model H, accepted, pose within the bounds tests/test_hf_cpu.py derives - where the essential path is off by
    0.1 in R and more than 0.9 in t"""
    from tests.test_hf_cpu import R_BOUND, T_BOUND
    s, g = C.scene(name), device(ctx, name)
    assert g["model"] == 1 and g["accepted"]
    clean = C.CASES[name][0].get("noise_px", 0.0) == 0.0
    eR, et = C.rel_err(g["R"], s["R"]) / np.sqrt(3.0), C.rel_err(g["t"], s["t"])
    print("%s: device R %.2e t %.2e; essential path R %.2e t %.2e" % (name, eR, et, C.rel_err(g["R_e"], s["R"]) / np.sqrt(3.0), C.rel_err(g["t_e"], s["t"])))
    assert eR < (1e-6 if clean else R_BOUND) and et < (1e-6 if clean else T_BOUND)
    assert abs(np.linalg.norm(g["t"]) - 1.0) < 1e-12 and abs(np.linalg.det(g["R"]) - 1.0) < 1e-12


@pytest.mark.parametrize("name", list(C.CASES))
def test_values_within_ten_times_the_restatements_own_spread(ctx, name):
    s, g, r, r2 = C.scene(name), device(ctx, name), C.restated(name), C.restated(name, "eigh")
    m = len(s["p1"])
    p1, p2 = s["p1"].astype(np.float64), s["p2"].astype(np.float64)
    bi = max(r["best_h"], 0)
    sf_ref = HR.f_score(g["E"], s["K"], p1, p2, 1.0) if np.isfinite(g["E"]).all() else 0.0
    rh_ref = r["SH"] / (r["SH"] + sf_ref) if r["SH"] + sf_ref > 0 else 0.0
    # per candidate: the parallax may differ by ten times the self-difference plus 4 ulps of its cos through acos (angles clipped
    # at 1e-3 degrees: the floor of a vanishing angle is the acos of 1 - 4 eps, 1.7e-6 degrees)
    th = np.radians(np.maximum(r["parallax_h"], 1e-3))
    par_dev, par_self, par_floor = np.abs(g["parallax_h"] - r["parallax_h"]), np.abs(r2["parallax_h"] - r["parallax_h"]), np.degrees(4 * EPS / np.sin(th))
    assert (par_dev <= 10 * par_self + par_floor).all(), (name, par_dev, par_self, par_floor)
    rows = [  # quantity, device - restatement, eigh - SVD, floor
        ("H", np.abs(_unit_fixed(g["H"]) - _unit_fixed(r["H"])).max(), np.abs(_unit_fixed(r2["H"]) - _unit_fixed(r["H"])).max(), 64 * EPS),
        ("SH", abs(g["SH"] - r["SH"]) / r["SH"], abs(r2["SH"] - r["SH"]) / r["SH"], m * EPS),
        ("SF", abs(g["SF"] - sf_ref) / max(sf_ref, 1e-300), 0.0, m * EPS),
        ("RH", abs(g["RH"] - rh_ref), abs(r2["RH"] - r["RH"]), 2 * m * EPS),
        ("R", np.abs(g["R_h"] - r["R_h"]).max(), np.abs(r2["R_h"] - r["R_h"]).max(), 64 * EPS),
        ("t", np.abs(g["t_h"] - r["t_h"]).max(), np.abs(r2["t_h"] - r["t_h"]).max(), 64 * EPS),
        ("parallax", par_dev[bi], par_self[bi], par_floor[bi]),
    ]
    if r["model"] == 1 and r["pose_mask"].any():
        pm = r["pose_mask"]
        nx = np.linalg.norm(r["X"][pm].astype(np.float64), axis=1)
        rows.append(("X", (np.linalg.norm(g["X"][pm].astype(np.float64) - r["X"][pm], axis=1) / nx).max(),
                     (np.linalg.norm(r2["X"][pm].astype(np.float64) - r["X"][pm], axis=1) / nx).max(), 2.0 ** -23))
        assert np.isnan(g["X"][~pm]).all()
    print(name + ": " + "; ".join("%s %.1e (self %.1e, bound %.1e)" % (q, d, sd, 10 * sd + fl) for q, d, sd, fl in rows))
    for q, d, sd, fl in rows:
        assert d <= 10 * sd + fl, (name, q, d, sd, fl)


@pytest.mark.parametrize("name", list(C.CASES))
def test_the_essential_side_is_the_existing_call(ctx, name):
    """the E block equals mo_init_two_view on the same arguments whatever the model; where F is chosen, so does the selection"""
    s, g = C.scene(name), device(ctx, name)
    e = ctx.init_two_view(s["p1"], s["p2"], s["K"], thr_px=3.0, n_hyp=C.N_HYP, seed=C.SEED)
    for a, b in (("E", "E"), ("R_e", "R"), ("t_e", "t"), ("ransac_mask", "ransac_mask")):
        assert np.array_equal(g[a], e[b], equal_nan=True), (name, a)
    assert g["n_good_e"] == e["n_good"]
    if g["model"] == 0:
        for k in ("R", "t", "pose_mask", "X", "n_good"):
            assert np.array_equal(np.asarray(g[k]), np.asarray(e[k]), equal_nan=True), (name, k)


def test_fewer_than_eight_correspondences_have_no_model(ctx):
    s = C.scene("plane_s1")
    g = ctx.init_two_view_hf(s["p1"][:7], s["p2"][:7], s["K"], **C.call_kw("plane_s1"))
    assert g["model"] == -1 and not g["accepted"] and g["n_good"] == 0 and g["winner_h"] == -1
    assert not g["pose_mask"].any() and not g["h_mask"].any() and not g["ransac_mask"].any()
    assert all(np.isnan(g[k]).all() for k in ("R", "t", "E", "H", "X", "R_h", "t_h"))


def test_forty_points_take_the_last_sorted_parallax_and_the_triangulation_minimum(ctx):
    s, r = C.scene("plane_m40"), C.restated("plane_m40")
    g50 = device(ctx, "plane_m40")
    g20 = ctx.init_two_view_hf(s["p1"], s["p2"], s["K"], **C.call_kw("plane_m40", min_triangulated=20))
    assert g50["model"] == 1 and 20 < g50["n_good"] <= 40 and not g50["accepted"] and g20["accepted"]
    _assert_integers(g20, C.restated("plane_m40", min_triangulated=20), "m40 / 20")
    assert abs(g50["parallax_h"][g50["best_h"]] - r["parallax_h"][r["best_h"]]) < 1e-9
    assert C.rel_err(g20["R"], s["R"]) < 1e-6 and C.rel_err(g20["t"], s["t"]) < 1e-5


@pytest.mark.parametrize("n_hyp_h", [1, 63, 64, 65])
def test_hypothesis_tile_tails(ctx, n_hyp_h):
    s = C.scene("plane_s1")
    kw = C.call_kw("plane_s1", n_hyp_h=n_hyp_h)
    r = C.restated("plane_s1", n_hyp_h=n_hyp_h)
    c = np.sort(r["cost"].astype(np.float64))
    assert r["margin"] > 1e-9 and (len(c) < 2 or c[1] - c[0] > 1e-6 * c[0])  # the input conditions of an integer comparison
    g = ctx.init_two_view_hf(s["p1"], s["p2"], s["K"], **kw)
    assert 0 <= g["winner_h"] < n_hyp_h
    _assert_integers(g, r, "n_hyp_h %d" % n_hyp_h)


def test_a_scene_on_one_line_has_no_homography(ctx):
    l = C.line_scene()
    g = ctx.init_two_view_hf(l["p1"], l["p2"], l["K"], **C.call_kw("line"))
    r = HR.hf_two_view(l["p1"], l["p2"], l["K"], **C.call_kw("line"))
    assert g["winner_h"] == -1 and g["SH"] == 0.0 and g["RH"] == 0.0 and np.isnan(g["H"]).all() and not g["h_mask"].any()
    assert g["model"] != 1 and (g["model"] == 0 or not g["accepted"])
    e = ctx.init_two_view(l["p1"], l["p2"], l["K"], thr_px=3.0, n_hyp=C.N_HYP, seed=C.SEED)
    assert np.array_equal(g["E"], e["E"], equal_nan=True)
    assert r["winner_h"] == -1 and r["model"] != 1


def test_non_finite_coordinates_do_what_the_existing_call_does(ctx):
    s = C.scene("plane_s1")
    p1 = s["p1"].copy()
    p1[5, 0] = np.nan
    p1[9, 1] = np.inf
    g = ctx.init_two_view_hf(p1, s["p2"], s["K"], **C.call_kw("plane_s1"))
    e = ctx.init_two_view(p1, s["p2"], s["K"], thr_px=3.0, n_hyp=C.N_HYP, seed=C.SEED)
    assert np.array_equal(g["E"], e["E"], equal_nan=True) and g["n_good_e"] == e["n_good"]
    assert g["winner_h"] == -1 and g["model"] != 1  # a non-finite centroid leaves no homography hypothesis
    if g["model"] == 0:
        assert np.array_equal(g["pose_mask"], e["pose_mask"]) and np.array_equal(g["X"], e["X"], equal_nan=True)
    assert _same_bytes(device(ctx, "plane_s1"), ctx.init_two_view_hf(s["p1"], s["p2"], s["K"], **C.call_kw("plane_s1")))  # and leaves nothing behind


def test_equal_inputs_give_equal_bytes_whatever_ran_before(ctx):
    import vslam_amd as V
    s, big, small = C.scene("plane_s2"), C.scene("plane_m4097"), C.scene("plane_m40")
    a = ctx.init_two_view_hf(s["p1"], s["p2"], s["K"], **C.call_kw("plane_s2"))
    b = ctx.init_two_view_hf(s["p1"], s["p2"], s["K"], **C.call_kw("plane_s2"))
    assert _same_bytes(a, b)
    ctx.init_two_view_hf(big["p1"], big["p2"], big["K"], **C.call_kw("plane_m4097", n_hyp_h=65))
    ctx.init_two_view_hf(small["p1"], small["p2"], small["K"], **C.call_kw("plane_m40"))
    c = ctx.init_two_view_hf(s["p1"], s["p2"], s["K"], **C.call_kw("plane_s2"))
    fresh = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    try:
        d = fresh.init_two_view_hf(s["p1"], s["p2"], s["K"], **C.call_kw("plane_s2"))
    finally:
        fresh.close()
    assert _same_bytes(a, c) and _same_bytes(a, d)


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x7F])
def test_results_do_not_depend_on_poisoned_scratch(ctx, byte):
    s = C.scene("plane_s3")
    a = device(ctx, "plane_s3")
    ctx._check(ctx.lib.mo_dbg_set_poison(ctx.h, byte))
    try:
        b = ctx.init_two_view_hf(s["p1"], s["p2"], s["K"], **C.call_kw("plane_s3"))
    finally:
        ctx._check(ctx.lib.mo_dbg_set_poison(ctx.h, -1))
    assert _same_bytes(a, b)


def test_argument_errors(ctx):
    import vslam_amd as V
    s = C.scene("plane_s1")
    for bad in (dict(sigma=0.0), dict(n_hyp_h=0), dict(n_hyp=0), dict(min_parallax_deg=-1.0), dict(min_triangulated=-1), dict(sigma=float("nan"))):
        with pytest.raises(V.NativeError):
            ctx.init_two_view_hf(s["p1"], s["p2"], s["K"], **C.call_kw("plane_s1", **bad))


# ---- drop-in -------------------------------------------------------------------------------------------------------------------------
def _warp(img, Hinv):
    """img seen through a homography: out(x2) = img(Hinv x2), bilinear, numpy only"""
    h, w = img.shape
    xx, yy = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    q = Hinv @ np.stack([xx.ravel(), yy.ravel(), np.ones(h * w)])
    x, y = np.clip(q[0] / q[2], 0, w - 1.001), np.clip(q[1] / q[2], 0, h - 1.001)
    x0, y0 = x.astype(int), y.astype(int)
    fx, fy = x - x0, y - y0
    f = img.astype(np.float64)
    out = f[y0, x0] * (1 - fx) * (1 - fy) + f[y0, x0 + 1] * fx * (1 - fy) + f[y0 + 1, x0] * (1 - fx) * fy + f[y0 + 1, x0 + 1] * fx * fy
    return np.clip(np.rint(out), 0, 255).astype(np.uint8).reshape(h, w)


def test_map_initializer_with_model_selection_on_a_textured_plane():
    """Two views of a textured plane (the second is the first warped by the plane-induced homography of a known motion): with
    model_selection=True the initializer succeeds through the homography with a pose near the truth.
    Bound: ORB keypoints sit on pyramid levels up to 1.2^7 = 3.6 px per sample and the second image is resampled, so a keypoint is
    located to about 2 px at worst; with at least 100 inliers the fitted transfer is known to 2 / sqrt(100 / 4) = 0.4 px, that is
    0.4 / 320 = 1.3e-3 rad in R and 0.4 px over the motion's signal f |t| / d = 80 px = 5e-3 in t; the bounds are five times that."""
    from orbslam2.extractor import ORBExtractor
    from orbslam2.initializer import MapInitializer
    from orbslam2.matcher import DescriptorMatcher
    from oracle.geom_oracle import rodrigues
    from tests.helpers import synthetic_frame
    K = np.array([[320.0, 0, 320.0], [0, 320.0, 240.0], [0, 0, 1.0]])
    R, t, n, d = rodrigues((0.01, -0.03, 0.02)), np.array([1.0, 0.1, 0.05]), np.array([0.1, -0.05, 1.0]), 4.0
    t, n = t / np.linalg.norm(t), n / np.linalg.norm(n)
    H = K @ (R + np.outer(t, n) / d) @ np.linalg.inv(K)
    a = synthetic_frame(77)
    b = _warp(a, np.linalg.inv(H))
    extractor = ORBExtractor(n_features=2000)
    matcher = DescriptorMatcher(matcher_type='bruteforce-hamming', ratio_threshold=0.75)
    init = MapInitializer(K, model_selection=True)
    kp0, d0 = extractor.extract_features(a, distributed=False)
    kp1, d1 = extractor.extract_features(b, distributed=False)
    init.set_first_frame(kp0, d0, a)
    ok, Rg, tg, pts, matches = init.initialize(kp1, d1, matcher, b)
    sel = init.last_selection
    print("plane drop-in:", sel, "R err", C.rel_err(Rg, R) / np.sqrt(3.0) if ok else None, "t err", C.rel_err(tg, t.reshape(3, 1)) if ok else None)
    assert ok and sel["model"] == 1 and sel["accepted"] and len(pts) == len(matches) >= 100
    assert C.rel_err(Rg, R) / np.sqrt(3.0) < 5 * 1.3e-3 and C.rel_err(tg, t.reshape(3, 1)) < 5 * 5e-3
    # the map points lie on the plane n . X = d
    X = np.array([p["position"] for p in pts], np.float64)
    assert np.median(np.abs(X @ n - d)) < 0.05 * d


def test_map_initializer_refuses_a_pure_pan_with_model_selection():
    """the np.roll pair of tests/test_gpu_dropin.py (a pure pan: planar and without a baseline to tell): model_selection=True returns
    the reference's failure tuple, the default returns what it returns today (the fused call's result)"""
    from orbslam2.extractor import ORBExtractor
    from orbslam2.initializer import MapInitializer
    from orbslam2.matcher import DescriptorMatcher
    from tests.helpers import synthetic_frame
    K = np.array([[320.0, 0, 320.0], [0, 320.0, 240.0], [0, 0, 1.0]])
    base = np.concatenate([synthetic_frame(41), synthetic_frame(42)], axis=1)
    frames = [np.ascontiguousarray(base[:, 5 * i:5 * i + 640]) for i in range(2)]
    extractor = ORBExtractor(n_features=2000)
    matcher = DescriptorMatcher(matcher_type='bruteforce-hamming', ratio_threshold=0.75)
    kp0, d0 = extractor.extract_features(frames[0], distributed=False)
    kp1, d1 = extractor.extract_features(frames[1], distributed=False)
    results = []
    for sel in (False, True):
        init = MapInitializer(K, model_selection=sel)
        init.set_first_frame(kp0, d0, frames[0])
        results.append((init.initialize(kp1, d1, matcher, frames[1]), init))
    (plain, _), (chosen, init) = results
    print("pure pan:", init.last_selection, "default ok:", plain[0])
    assert chosen[0] is False and chosen[1] is None and chosen[2] is None and chosen[3] is None and len(chosen[4]) > 300
    assert not init.last_selection["accepted"] and not init.initialization_done
    again = MapInitializer(K)  # the default path is today's code: same result as a second default initializer
    again.set_first_frame(kp0, d0, frames[0])
    ok2, R2, t2, pts2, m2 = again.initialize(kp1, d1, matcher, frames[1])
    assert ok2 == plain[0] and (not ok2 or (np.array_equal(R2, plain[1]) and np.array_equal(t2, plain[2]) and len(pts2) == len(plain[3])))
