"""The device covisibility matrix (mo_map_covisibility), the local keyframes picked from it (mo_map_local_keyframes) and tracking against
their local map (mo_map_track_covisible) against tests/covis_restatement.py: integers exactly, poses within the bounds
tests/test_gpu_map_reads.py uses for mo_map_track.  tests/test_covis_cpu.py shows on the CPU what the pan-back world tells apart."""
import ctypes as C

import numpy as np
import pytest

from tests import covis_restatement as CR
from tests import track_restatement as TR
from tests.covis_worlds import A_KF, pan_back
from tests.map_worlds import build_map, kps_array, perturbed_pose, pose_near, world

pytestmark = pytest.mark.gpu

LDS_MAX_KF = 128   # CV_LDS_MAX_KF of map_covis.hip: beyond it k_covis adds to the matrix in global memory


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _restated_W(w):
    return CR.covisibility(w.obs_off, w.obs_kf, w.obs_kp, w.counts)


def _votes(w, seeds):
    return CR.seed_votes(w.obs_off, w.obs_kf, w.obs_kp, w.counts, seeds)


def _raw_local(m, prm, out):
    return m.lib.mo_map_local_keyframes(m._h, C.byref(prm) if prm is not None else None, C.byref(out) if out is not None else None)


@pytest.mark.parametrize("name", ["clean", "stale", "ba", "ba_stale", "pan_back"])
def test_matrix_equals_restatement(name):
    """removed keyframes (position != slot), stale and negative keys, points seen twice in one keyframe; 1500 - 2000 points: several
    workgroups add into the same cells.  Twice: the matrix is recomputed, not accumulated."""
    ctx = _ctx()
    w = pan_back() if name == "pan_back" else world(name)
    m = build_map(ctx, w)
    ref = _restated_W(w)
    for _ in range(2):
        W = m.covisibility()
        assert W.dtype == np.int32 and W.shape == ref.shape
        assert np.array_equal(W, ref), int((W != ref).sum())
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_empty_map_one_keyframe_and_compute_only():
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    m = LocalMapper(np.eye(3), save_every_keyframe=False, context=ctx)
    assert m.covisibility().shape == (0, 0)
    assert m.local_keyframes() == {"local": [], "k1": [], "k2": [], "ref": -1}
    out = V.MapLocalOut(None)
    assert _raw_local(m, V.MapLocalParams(None, 0, 5, 10, 15), out) == V.MO_OK and (out.n_k1, out.n_local_kf) == (0, 0)   # (no keyframes: ref_pos is not looked at)
    rng = np.random.default_rng(1)
    m.add_keyframe(np.zeros((480, 640), np.uint8), kps_array(rng.uniform(0, 400, (6, 2))), rng.integers(0, 256, (6, 32)).astype(np.uint8), np.eye(4))
    assert np.array_equal(m.covisibility(), [[0]])   # a keyframe, no map points
    assert m.local_keyframes() == {"local": [0], "k1": [0], "k2": [], "ref": 0}
    m.update_map_points([{"id": i, "position": np.ones(3), "observed_keyframes": o} for i, o in enumerate([{0: 1}, {0: 2, -1: 3}, {1: 0}, {0: 6}])])
    assert np.array_equal(m.covisibility(), [[2]])   # (seen twice: once; a position and a row that do not exist: nothing)
    assert m.local_keyframes(seed_points=[0, 1, 2, 3]) == {"local": [0], "k1": [0], "k2": [], "ref": 0}
    m.close()
    # weights = NULL computes only; the selection that follows reads the resident matrix it computes itself
    w = pan_back()
    m = build_map(ctx, w)
    n_kf = C.c_int32(-1)
    assert m.lib.mo_map_covisibility(m._h, None, C.byref(n_kf)) == V.MO_OK and n_kf.value == len(w.counts)
    assert m.lib.mo_map_covisibility(m._h, None, None) == V.MO_ERR_ARG
    ref = CR.local_keyframes(_restated_W(w), None, 5, 10, 15)
    got = m.local_keyframes(ref=5)
    assert (got["local"], got["k1"], got["k2"], got["ref"]) == (ref["local"], ref["k1"], ref["k2"], 5)
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_global_atomics_path_beyond_the_lds_bound():
    """one keyframe more than fits the workgroups' LDS copies: six keypoints each (no growth step can find a model), 400 injected points
    with 1 - 6 observations spread over all positions, some keys negative, some naming nothing, some twice in a keyframe"""
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    n_kf, rows = LDS_MAX_KF + 1, 6
    rng = np.random.default_rng(12)
    m = LocalMapper(np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]]), save_every_keyframe=False, context=ctx)
    img = np.zeros((480, 640), np.uint8)
    for k in range(n_kf):
        m.add_keyframe(img, kps_array(rng.uniform(5, 470, (rows, 2))), rng.integers(0, 256, (rows, 32)).astype(np.uint8), np.eye(4))
        assert m.last["n_new"] == 0
    assert len(m.keyframes) == n_kf and len(m.map_points) == 0
    pts, off, okf, okp = [], [0], [], []
    for i in range(400):
        o = {}
        for k in rng.integers(-n_kf - 3, n_kf + 3, int(rng.integers(1, 7))).tolist():
            o[int(k)] = int(rng.integers(-rows - 1, rows + 2))
        if i % 7 == 0:
            k = next(iter(o))
            if 0 <= k < n_kf:
                o[k - n_kf] = int(rng.integers(0, rows))
        pts.append({"id": i, "position": rng.uniform(-1, 1, 3), "observed_keyframes": o})
        okf += list(o.keys()); okp += list(o.values()); off.append(len(okf))
    m.update_map_points(pts)
    ref = CR.covisibility(np.array(off), np.array(okf), np.array(okp), [rows] * n_kf)
    assert (ref.diagonal() > 0).all() and ref.trace() < len(okf)   # every position is seen; some keys named nothing
    for _ in range(2):
        W = m.covisibility()
        assert np.array_equal(W, ref), int((W != ref).sum())
    seeds = np.arange(0, 400, 3)
    sel = CR.local_keyframes(ref, CR.seed_votes(np.array(off), np.array(okf), np.array(okp), [rows] * n_kf, seeds), None, 3, 1)
    got = m.local_keyframes(seed_points=seeds, n_best=3, min_weight=1)
    assert (got["local"], got["k1"], got["ref"]) == (sel["local"], sel["k1"], sel["ref"])
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_selection_equals_restatement():
    import vslam_amd as V
    ctx = _ctx()
    w = pan_back()
    m = build_map(ctx, w)
    W = _restated_W(w)
    n_kf, n_pts = len(w.counts), len(w.obs)
    seeds = w.seeds()
    odd = np.concatenate([seeds, [-1, n_pts, n_pts + 7, -5, 2 ** 31 - 1], seeds[:40]]).astype(np.int32)   # entries outside the map; 40 given twice
    a_seeds = np.flatnonzero(w.a_only)[:50]
    cases = [(None, None, 10, 15), (None, 5, 10, 15), (None, 0, 2, 1), (None, 19, 0, 1), (None, 12, 10, 10 ** 6),
             (seeds, None, 10, 15), (seeds, 3, 1, 100), (seeds, None, 0, 15), (seeds, None, 25, 1), (seeds, None, 3, 10 ** 6), (seeds, None, 2, -4),
             (odd, None, 10, 15), (a_seeds, None, 1, 90), (np.full(9, -1, np.int32), 2, 10, 15), (np.zeros(0, np.int32), 7, 10, 15)]
    seen = set()
    for sp, ref, n_best, min_weight in cases:
        want = CR.local_keyframes(W, _votes(w, sp), ref, n_best, min_weight)
        got = m.local_keyframes(seed_points=sp, ref=ref, n_best=n_best, min_weight=min_weight)
        assert (got["local"], got["k1"], got["k2"], got["ref"]) == (want["local"], want["k1"], want["k2"], want["ref"]), (ref, n_best, min_weight, got, want)
        seen.add((len(got["k1"]), len(got["k2"])))
    assert len(seen) >= 6   # the cases are not one selection said fifteen times
    v, vo = _votes(w, seeds), _votes(w, odd)
    assert (vo > v).any() and vo.sum() == v.sum() + v_sum_of(w, seeds[:40])
    # the argument rules
    out = V.MapLocalOut(None)
    one = np.zeros(1, np.int32)
    ok = V.MapLocalParams(None, 0, -1, 10, 15)
    assert _raw_local(m, ok, out) == V.MO_OK and out.ref == n_kf - 1
    assert _raw_local(m, None, out) == V.MO_ERR_ARG and _raw_local(m, ok, None) == V.MO_ERR_ARG
    assert m.lib.mo_map_local_keyframes(None, C.byref(ok), C.byref(out)) == V.MO_ERR_ARG
    assert _raw_local(m, V.MapLocalParams(None, 0, -1, -1, 15), out) == V.MO_ERR_ARG           # n_best < 0
    assert _raw_local(m, V.MapLocalParams(None, 1, -1, 10, 15), out) == V.MO_ERR_ARG           # seeds announced, none given
    assert _raw_local(m, V.MapLocalParams(one.ctypes.data, 1, n_kf, 10, 15), out) == V.MO_ERR_ARG    # ref_pos == n_kf
    assert _raw_local(m, V.MapLocalParams(one.ctypes.data, 1, -2, 10, 15), out) == V.MO_ERR_ARG      # ref_pos < -1
    assert _raw_local(m, V.MapLocalParams(one.ctypes.data, 1, n_kf - 1, 10, 15), out) == V.MO_OK
    kps, desc = w.query()
    with pytest.raises(V.NativeError):
        m.track_local_map(kps, desc, w.query_pose, local="covisible", n_best=-1)
    with pytest.raises(ValueError):
        m.track_local_map(kps, desc, w.query_pose, local="recent")
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def v_sum_of(w, seeds):
    return int(_votes(w, seeds).sum())


def _same_info(a, b):
    (oa, pa, ia), (ob, pb, ib) = a, b
    assert oa == ob and pa.tobytes() == pb.tobytes()
    for f in ("point", "dist", "inlier"):
        assert np.array_equal(ia[f], ib[f]), f
    for f in ("pass_radius", "pass_cand", "pass_matches", "pass_inliers", "n_local", "n_pass_run"):
        assert ia[f] == ib[f], f
    assert len(ia["pass_pose"]) == len(ib["pass_pose"]) and all(x.tobytes() == y.tobytes() for x, y in zip(ia["pass_pose"], ib["pass_pose"]))


def _ba_query(w):
    """a frame for the consecutive-keyframe world (its observations carry random descriptors: the frame shows the representatives)"""
    rep, _ = TR.representatives(TR.valid_observations(w.obs_off, w.obs_kf, w.obs_kp, w.counts), w.kf_desc, w.kf_oct, np.ones(len(w.obs), bool))
    T = pose_near(w, 4)
    return T, w.track_query(T, point_desc=rep, octave_spread=0)


def test_every_keyframe_local_equals_the_window_of_all():
    """the same kernels on the same inputs: bit for bit, poses included"""
    ctx = _ctx()
    w = world("ba")
    m = build_map(ctx, w)
    n_kf = len(w.counts)
    T, (kps, desc) = _ba_query(w)
    pose0 = perturbed_pose(T)
    for radii in ((15.0,), (15.0, 4.0)):
        win = m.track_local_map(kps, desc, pose0, radii=radii, window=0, image_size=w.image_size)
        cov = m.track_local_map(kps, desc, pose0, radii=radii, window=3, image_size=w.image_size, local="covisible",
                                seed_points=np.arange(len(w.obs)), n_best=n_kf + 5, min_weight=1)
        assert cov[2]["local_keyframes"] == list(range(n_kf))
        assert win[2]["n_local"] == len(w.obs) and win[2]["pass_matches"][0] >= 20 and win[2]["n_pass_run"] == len(radii)
        _same_info(win, cov)
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_pan_back_tracks_what_the_window_lost():
    from tests.test_gpu_map_reads import REFINE_TOL
    ctx = _ctx()
    w = pan_back()
    m = build_map(ctx, w)
    kps, desc = w.query()
    pose0 = perturbed_pose(w.query_pose)
    W_, H_ = w.image_size
    seeds = w.seeds()
    ok, _, info = m.track_local_map(kps, desc, pose0, window=10)
    named = info["point"][info["point"] >= 0]
    assert not ok and not w.a_only[named].any() and info["n_local"] == int(TR.local_points(w.valid, len(w.counts), 10).sum())
    args = (w.K, pose0, w.xyz, w.obs_off, w.obs_kf, w.obs_kp, w.kf_desc, w.kf_oct, kps, desc, W_, H_)
    # pass 1 alone: integers from pose0
    ok1, _, i1 = m.track_local_map(kps, desc, pose0, radii=(15.0,), local="covisible", seed_points=seeds)
    r1, sel = CR.track_covisible(*args, seed_points=seeds, radii=(15.0,), refine_pose=False)
    p1 = r1["passes"][0]
    assert i1["local_keyframes"] == sel["local"] and i1["ref_keyframe"] == sel["ref"] and i1["n_local"] == r1["n_local"]
    assert np.array_equal(i1["point"], p1["point"]) and np.array_equal(i1["dist"], p1["dist"])
    assert (i1["pass_cand"][0], i1["pass_matches"][0], i1["pass_radius"][0]) == (p1["cand"], p1["matches"], p1["radius"])
    # the call as its defaults run it, against the restatement of the whole call
    ok, pose, info = m.track_local_map(kps, desc, pose0, local="covisible", seed_points=seeds)
    res, sel = CR.track_covisible(*args, seed_points=seeds)
    last = res["passes"][-1]
    assert all(k in info["local_keyframes"] for k in A_KF) and info["local_keyframes"] == sel["local"]
    assert ok and res["ok"] and info["n_pass_run"] == 2 and info["n_local"] == res["n_local"]
    assert np.array_equal(info["point"], last["point"]) and np.array_equal(info["dist"], last["dist"])
    q = np.flatnonzero(info["point"] >= 0)
    assert np.array_equal(info["inlier"][q], last["inlier"]) and not info["inlier"][info["point"] < 0].any()
    assert info["pass_matches"] == [p["matches"] for p in res["passes"]] and info["pass_inliers"] == [p["inliers"] for p in res["passes"]]
    assert int(w.a_only[info["point"][q]].sum()) >= 100 and info["pass_inliers"][-1] >= 30
    print("pan-back: %d matches, %d on points of A, largest |pose - restated pose| %.3g, |pose - truth| %.3g"
          % (len(q), int(w.a_only[info["point"][q]].sum()), np.abs(pose - res["pose"]).max(), np.abs(pose - w.query_pose).max()))
    assert np.allclose(pose, res["pose"], **REFINE_TOL), pose - res["pose"]
    # seeds on A alone and a tight selection: B is not local, and the local map is the restatement's
    a_seeds = np.flatnonzero(w.a_only)[:50]
    ok, pose, info = m.track_local_map(kps, desc, pose0, radii=(15.0,), local="covisible", seed_points=a_seeds, n_best=1, min_weight=90)
    r, sel = CR.track_covisible(*args, seed_points=a_seeds, n_best=1, min_weight=90, radii=(15.0,), refine_pose=False)
    assert info["local_keyframes"] == sel["local"] and max(sel["local"]) < 9 and info["n_local"] == r["n_local"] < len(w.obs)
    assert np.array_equal(info["point"], r["passes"][0]["point"])
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_window_paths_unchanged_by_covisible_calls():
    """k_trk_rep serves mo_map_track, mo_map_fuse and mo_map_track_covisible: a map that ran the covisible calls tracks and fuses like
    its twin that never did"""
    ctx = _ctx()
    w = world("ba")
    a, b = build_map(ctx, w), build_map(ctx, w)
    T, (kps, desc) = _ba_query(w)
    pose0 = perturbed_pose(T)
    b.covisibility()
    b.local_keyframes(seed_points=np.arange(0, len(w.obs), 2), n_best=2)
    b.track_local_map(kps, desc, pose0, image_size=w.image_size, local="covisible", seed_points=np.arange(50), n_best=1, min_weight=40)
    for window in (4, 0):
        _same_info(a.track_local_map(kps, desc, pose0, window=window, image_size=w.image_size),
                   b.track_local_map(kps, desc, pose0, window=window, image_size=w.image_size))
    fa, fb = a.fuse_map_points(window=5, image_size=w.image_size), b.fuse_map_points(window=5, image_size=w.image_size)
    assert fa["n_local"] > 0 and fa["n_pairs"] > 0
    for k in fa:
        assert np.array_equal(np.asarray(fa[k]), np.asarray(fb[k])), k
    xa, xb = a.arrays(), b.arrays()
    assert all(np.array_equal(xa[f], xb[f]) for f in xa)
    assert ctx.dev_status() == 0
    a.close(); b.close(); ctx.close()
