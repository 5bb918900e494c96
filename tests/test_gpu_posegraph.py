"""LocalMapper.optimize_essential_graph (mo_map_pose_graph) on the device: the edge set against tests/posegraph_restatement.py, the exact
cases against their truth and the drift cases against the host replay (tests/native/posegraph_replay.cpp) under the bounds measured on
the host (tests/posegraph_cases.py), the point rule, the calls that write nothing, and detect_loop(..., optimize=True) on the loop world."""
import ctypes as C

import numpy as np
import pytest

from tests import posegraph_cases as PC
from tests import posegraph_restatement as PR

pytestmark = pytest.mark.gpu

EXACT = {c.name: c for c in PC.exact_cases()}
DRIFT = {c.name: c for c in PC.drift_cases()}
EDGES = {c.name: c for c in PC.edge_cases()}
INTS = ("steps", "accepted", "cg_iters", "n_free", "n_fixed", "n_edges", "n_extra_used", "n_moved", "ok")


@pytest.fixture(scope="module")
def ctx():
    import vslam_amd as V
    c = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    d = tmp_path_factory.mktemp("posegraph_replay")
    return PC.build_native(d, "posegraph_replay"), d


def _xyz(m):
    m._cache = None
    return m.arrays()["xyz"].copy()


def _kp(m):
    """the integers of a fuse_map_points over all keyframes: a reader of the store's kP"""
    info = m.fuse_map_points(window=0, image_size=(PC.W_IMG, PC.H_IMG))
    return {k: v for k, v in info.items() if k != "into"}


def call(m, case, edge_cap=None, guard=0, **over):
    """mo_map_pose_graph called directly on the case's inputs: (rc, dict of every output).  guard: entries behind edge_cap that must stay"""
    import vslam_amd as V
    n, n_pts = case.n_kf, len(case.xyz)
    prm = dict(case.solver, min_weight=case.min_weight, fixed=case.fixed, extra=case.extra, poses=case.poses, init=case.init)
    prm.update(over)
    fixed = np.ascontiguousarray(prm["fixed"], np.uint8)
    xa = np.array([a for a, _ in prm["extra"]] or [0], np.int32)
    xb = np.array([b for _, b in prm["extra"]] or [0], np.int32)
    cap = n * (n - 1) // 2 if edge_cap is None else edge_cap
    ea, eb = np.full(cap + guard + 1, -7, np.int32), np.full(cap + guard + 1, -7, np.int32)
    ek = np.full(cap + guard + 1, 77, np.uint8)
    poses_out, sim3_out = np.full((n, 12), np.nan), np.full((n, 13), np.nan)
    moved = np.full(max(n_pts, 1), 9, np.uint8)
    p = V.MapPgParams(fixed.ctypes.data, xa.ctypes.data, xb.ctypes.data, len(prm["extra"]), int(prm["min_weight"]), int(prm["max_steps"]), int(prm["max_cg"]),
                      float(prm["cg_tol"]), float(prm["step_tol"]), (C.c_double * 9)(*np.asarray(prm.get("K", PC.K), np.float64).reshape(9)))
    o = V.MapPgOut(poses_out.ctypes.data, sim3_out.ctypes.data, ea.ctypes.data, eb.ctypes.data, ek.ctypes.data, moved.ctypes.data, cap)
    P, S0 = np.ascontiguousarray(prm["poses"], np.float64), np.ascontiguousarray(prm["init"], np.float64)
    rc = m.lib.mo_map_pose_graph(m._h, V._ptr(P), V._ptr(S0), C.byref(p), C.byref(o))
    out = {k: int(getattr(o, k)) for k in INTS}
    out.update(cost=(float(o.cost[0]), float(o.cost[1])), lam=float(o.lambda_), poses=poses_out, sim3=sim3_out, edge_a=ea, edge_b=eb, edge_kind=ek,
               moved=moved[:n_pts], cap=cap)
    return rc, out


def _edges_equal(case, out):
    a, b, k = case.edges()
    ne = len(a)
    assert out["n_edges"] == ne and out["n_free"] == int((case.fixed == 0).sum()) and out["n_fixed"] == int((case.fixed != 0).sum()), case.name
    assert np.array_equal(out["edge_a"][:ne], a) and np.array_equal(out["edge_b"][:ne], b) and np.array_equal(out["edge_kind"][:ne], k), case.name
    assert out["n_extra_used"] == int((k == PR.EXTRA).sum())
    assert (out["edge_a"][ne:] == -7).all() and (out["edge_kind"][ne:] == 77).all()   # nothing behind the edges is written


def _points_follow(case, before, after, out):
    """rule 4 for the points: from the returned sim3_out in numpy f64, to one f32 rounding; the rest keep their bytes"""
    want, moved = PR.moved_points(dict(case.arrays(), xyz=before), case.counts(), case.fixed, case.init, out["sim3"])
    if not out["ok"]:
        moved[:] = False
    assert np.array_equal(out["moved"].astype(bool), moved) and out["n_moved"] == int(moved.sum()), case.name
    assert after[~moved].tobytes() == before[~moved].tobytes(), case.name
    if moved.any():
        w32 = want[moved].astype(np.float32)
        ulp = np.spacing(np.abs(w32))
        assert (np.abs(after[moved].astype(np.float64) - want[moved]) <= ulp).all(), case.name
        assert moved.any() and (after[moved] != before[moved]).any()


@pytest.mark.parametrize("name", list(EDGES))
def test_edges_and_counts_equal_the_restatement(name, ctx):
    from tests.test_gpu_scratch_poison import _flat
    case = EDGES[name]
    got = []
    for other in (False, True):
        m = case.build_map(ctx)
        if other:   # another call in between leaves its own scratch behind
            x = EDGES["edges:thresholds"].build_map(ctx)
            call(x, EDGES["edges:thresholds"])
            x.close()
        before = _xyz(m)
        rc, out = call(m, case)
        assert rc == 0
        _edges_equal(case, out)
        after = _xyz(m)
        _points_follow(case, before, after, out)
        kp_reader = _kp(m)
        got.append(_flat((out, after, kp_reader)))
        m.close()
    assert got[0] == got[1], name


@pytest.mark.parametrize("name", list(EXACT))
def test_exact_cases_reach_the_truth(name, ctx):
    case = EXACT[name]
    m = case.build_map(ctx)
    before = _xyz(m)
    rc, out = call(m, case)
    assert rc == 0
    after = _xyz(m)
    e = PC.truth_error(case, out["sim3"])
    print("%s: %d edges, %d steps (%d accepted), %d cg iterations, cost %.3g -> %.3g, error to the truth %.3g (bound %.3g)"
          % (name, out["n_edges"], out["steps"], out["accepted"], out["cg_iters"], out["cost"][0], out["cost"][1], e, PC.TRUTH_BOUND))
    _edges_equal(case, out)
    assert out["ok"] and out["cost"][1] < out["cost"][0]
    assert e <= PC.TRUTH_BOUND, (name, e)
    assert out["sim3"][0].tobytes() == case.init[0].tobytes() and out["poses"][0].tobytes() == PR.pose_of(case.init[0]).tobytes()
    assert np.array_equal(out["poses"], np.array([PR.pose_of(S).reshape(12) for S in out["sim3"]]))
    _points_follow(case, before, after, out)
    if name == "exact:12":   # the store's kP follows the poses: fuse_map_points reads it, its restatement reads K [R | t] of the returned poses
        from tests import fuse_restatement as FR
        rows = case.kf_rows()
        poses = []
        for P in out["poses"]:
            T = np.eye(4)
            T[:3, :4] = P.reshape(3, 4)
            poses.append(T)
        want = FR.fuse(dict(case.arrays(), xyz=after), FR.store_P(PC.K, poses), [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows],
                       PC.W_IMG, PC.H_IMG, window=0)
        info = m.fuse_map_points(window=0, image_size=(PC.W_IMG, PC.H_IMG))
        assert want[3]["min"] > 1e-6 and want[2]["n_cand"] > 20 and all(info[c] == want[2][c] for c in FR.COUNTS), (info, want[2])
    m.close()


@pytest.mark.parametrize("name", list(DRIFT))
def test_drift_cases_equal_the_replay(name, ctx, replay):
    exe, d = replay
    case = DRIFT[name]
    r = PC.run_replay(exe, case, d)
    m = case.build_map(ctx)
    before = _xyz(m)
    rc, out = call(m, case)
    assert rc == 0
    after = _xyz(m)
    sp = PC.spread(case, out["sim3"], r["sim3"])
    bound = PC.SPREAD_FACTOR * PC.LIBM_SPREAD[name]
    r0, r1 = PC.consecutive_residual(case, case.init), PC.consecutive_residual(case, out["sim3"])
    print("%s: device %d steps (%d accepted, %d cg iterations), replay %d (%d, %d); cost %.9g -> %.9g (replay %.9g -> %.9g); |device - replay| %.3g (bound %.3g); "
          "largest consecutive residual %.3g -> %.3g" % (name, out["steps"], out["accepted"], out["cg_iters"], r["steps"], r["accepted"], r["cg_iters"],
                                                          out["cost"][0], out["cost"][1], r["cost"][0], r["cost"][1], sp, bound, r0, r1))
    _edges_equal(case, out)
    assert out["ok"] and out["cost"][1] < out["cost"][0] and r1 < r0
    assert out["sim3"][0].tobytes() == case.init[0].tobytes()
    assert sp <= bound, (name, sp, bound)
    assert (out["steps"], out["accepted"]) == (r["steps"], r["accepted"])   # (both cases are decisive: tests/test_posegraph_cpu.py)
    _points_follow(case, before, after, out)
    m.close()


def test_calls_that_write_nothing(ctx):
    case = DRIFT["drift:12"]
    m = case.build_map(ctx)
    before = _xyz(m)
    kp0 = _kp(m)
    assert kp0["n_cand"] > 20 and kp0["n_proposals"] == 0 and _xyz(m).tobytes() == before.tobytes()   # (the reader changes nothing itself)
    rc, out = call(m, case, max_steps=0)
    assert rc == 0 and not out["ok"] and out["steps"] == 0 and out["n_moved"] == 0 and not out["moved"].any()
    _edges_equal(case, out)
    assert out["sim3"].tobytes() == case.init.tobytes()
    assert _xyz(m).tobytes() == before.tobytes() and _kp(m) == kp0
    rc, out = call(m, case, fixed=np.ones(case.n_kf, np.uint8))
    assert rc == 0 and not out["ok"] and all(out[k] == 0 for k in INTS) and np.isnan(out["sim3"]).all() and (out["edge_a"] == -7).all()
    assert _xyz(m).tobytes() == before.tobytes() and _kp(m) == kp0
    m.close()
    # one keyframe; no keyframe
    from vslam_amd.mapper import LocalMapper
    one = PC.Case("one", 1)
    m = one.build_map(ctx)
    rc, out = call(m, one)
    assert rc == 0 and all(out[k] == 0 for k in INTS)
    m.close()
    empty = LocalMapper(PC.K, save_every_keyframe=False, context=ctx)
    rc, out = call(empty, PC.Case("none", 0), fixed=np.zeros(1, np.uint8), poses=np.zeros((1, 12)), init=np.zeros((1, 13)))
    assert rc == 0 and all(out[k] == 0 for k in INTS)
    empty.close()


def test_short_edge_outputs(ctx):
    case = EDGES["edges:thresholds"]
    a, b, k = case.edges()
    for cap in (0, 4, len(a)):
        m = case.build_map(ctx)
        rc, out = call(m, case, edge_cap=cap, guard=16)
        assert rc == 0 and out["n_edges"] == len(a) and out["ok"]
        assert np.array_equal(out["edge_a"][:cap], a[:cap]) and np.array_equal(out["edge_b"][:cap], b[:cap]) and np.array_equal(out["edge_kind"][:cap], k[:cap])
        assert (out["edge_a"][cap:] == -7).all() and (out["edge_b"][cap:] == -7).all() and (out["edge_kind"][cap:] == 77).all()
        m.close()


def test_errors_leave_the_map_alone(ctx):
    import vslam_amd as V
    case = DRIFT["drift:12"]
    m = case.build_map(ctx)
    before = _xyz(m)
    bad_init, bad_scale, bad_poses = case.init.copy(), case.init.copy(), case.poses.copy()
    bad_init[3, 5] = np.nan; bad_scale[4, 0] = 0.0; bad_poses[2, 7] = np.inf
    Kn = PC.K.copy(); Kn[0, 0] = np.nan
    for over in (dict(fixed=np.zeros(case.n_kf, np.uint8)), dict(init=bad_init), dict(init=bad_scale), dict(poses=bad_poses), dict(K=Kn),
                 dict(extra=[(0, case.n_kf)]), dict(extra=[(-1, 3)]), dict(extra=[(4, 4)]), dict(max_steps=-1), dict(max_steps=101), dict(max_cg=0),
                 dict(cg_tol=-1.0), dict(step_tol=np.nan)):
        rc, out = call(m, case, **over)
        assert rc == V.MO_ERR_ARG, over
    assert _xyz(m).tobytes() == before.tobytes()
    m.close()


def test_scratch_poison():
    """the 12-keyframe drift case on a rebuilt map under two poison bytes gives the outputs and the map of the unpoisoned run"""
    from tests.test_gpu_scratch_poison import _checked, _ctx, _flat, _map_state, _same, _set
    case = DRIFT["drift:12"]
    c = _ctx()
    try:
        def run(poisoned):
            m = _checked(c, lambda: case.build_map(c), poisoned)
            rc, out = _checked(c, lambda: call(m, case), poisoned)
            assert rc == 0 and out["accepted"] == 3 and out["n_moved"] > 0   # the call finds what it looks for: nothing compares empty results
            kp = _checked(c, lambda: _kp(m), poisoned)
            got = _flat((out, _map_state(m), kp))
            m.close()
            return got
        want = run(False)
        for byte in (255, 90):
            _set(c, byte)
            _same(run(True), want, (byte, "pose graph"))
            assert c.dev_status() == 0
    finally:
        c.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
FACTOR = 1.3
CHI2 = 5.991


def _inlier_observations(m, w):
    """the observations whose point reprojects within the chi2 gate under its keyframe's kf["pose"] (every keypoint of the loop world is of
    octave 0: information 1)"""
    from tests.track_restatement import valid_observations
    m._cache = None
    a = m.arrays()
    n = 0
    for i, v in enumerate(valid_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], w.counts)):
        X = a["xyz"][i].astype(np.float64)
        for k, row in v:
            T = np.asarray(m.keyframes[k]["pose"], np.float64)
            x = w.K @ (T[:3, :3] @ X + T[:3, 3])
            d = x[:2] / x[2] - np.asarray(w.kf_xy[k][row], np.float64)
            n += bool(x[2] > 0 and d @ d <= CHI2)
    return n


def test_detect_loop_with_optimisation_on_the_rescaled_loop_world():
    """detect_loop(26, sim3=True, confirm=True, correct=True, optimize=True) on the loop world with its return side drifted by a scale of
    1.3, the old side (the winning candidate's group) fixed: the optimisation accepts a step, the cost does not rise, the old side's
    poses keep their bytes, the return side stays at the unscaled world, and no observation stops reprojecting within the chi2 gate.
    On a second map the loop is corrected without the keyword and then optimised from correct_loop's info alone - the poses before it
    reconstructed from A, the fixed set the default, the winning candidate: that keyframe keeps its bytes.  The keyword's own default is
    the same: run once on a third map."""
    import vslam_amd as V
    from tests import correct_worlds as CW
    from tests import loop_worlds as LW
    from tests.test_gpu_sim3 import _rescaled
    c = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    base = LW.loop_world()
    w = _rescaled(base, FACTOR)
    words, weights = LW.loop_vocabulary()
    voc = V.Vocabulary.from_arrays(words, weights, context=c)
    group = CW.restated(w, FACTOR)["group"]   # (on the CPU: the old side the correction will name)
    assert 3 in group and len(group) > 1
    for keyword in (True, False):
        m = w.build(c)
        m.set_vocabulary(voc)
        if keyword:
            with pytest.raises(ValueError):
                m.detect_loop(26, sim3=True, confirm=True, optimize=True)
        n0 = _inlier_observations(m, w)
        poses0 = [np.asarray(kf["pose"], np.float64).copy() for kf in m.keyframes]
        m._loop_consistency = None
        got = [m.detect_loop(p, sim3=True, confirm=True, correct=(p == 26), optimize=(keyword and p == 26), optimize_kw=dict(fixed=group), seed=11)
               for p in LW.RETURN_POS[:-1]]
        if keyword:   # the keyword's own default first, on a map of its own: the winning candidate alone stays
            x = w.build(c)
            x.set_vocabulary(voc)
            x._loop_consistency = None
            d = [x.detect_loop(p, sim3=True, confirm=True, correct=(p == 26), optimize=(p == 26), seed=11) for p in LW.RETURN_POS][-1][1]["accepted"]
            assert d["optimize"]["ok"] and d["optimize"]["fixed"] == [d["pos"]] == [3]
            x.close()
        got.append(m.detect_loop(26, sim3=True, confirm=True, correct=True, optimize=keyword, optimize_kw=dict(fixed=group), seed=11))
        assert [f for f, _ in got] == [p == 26 for p in LW.RETURN_POS]
        a = got[-1][1]["accepted"]
        co = a["correct"]
        assert co["group"] == list(group) and a["pos"] == 3
        n1 = _inlier_observations(m, w)
        og = a["optimize"] if keyword else m.optimize_essential_graph(a)
        n2 = _inlier_observations(m, w)
        print("optimize=%s: %s; cost %.6g -> %.6g; inlier observations %d before the call, %d corrected, %d optimised"
              % (keyword, {k: og[k] for k in INTS}, og["cost"][0], og["cost"][1], n0, n1, n2))
        assert og["ok"] and og["accepted"] > 0 and og["cost"][1] <= og["cost"][0]
        assert og["fixed"] == (list(group) if keyword else [3]) and og["n_free"] == LW.N_KF - len(og["fixed"]) and og["n_extra_used"] > 0
        assert n2 >= n0, (n0, n1, n2)
        rest = ret = 0.0
        for k, kf in enumerate(m.keyframes):
            T = np.asarray(kf["pose"], np.float64)
            assert np.array_equal(T[:3, :4], og["poses"][k])
            if k in og["fixed"]:
                assert T.tobytes() == poses0[k].tobytes(), k
            elif k in group:
                rest = max(rest, np.abs(T - poses0[k]).max())
            elif k in LW.RETURN_POS:
                ret = max(ret, np.abs(T[:3, :4] - np.asarray(base.kf_poses[k], np.float64)[:3, :4]).max())
        # (printed, not bounded: the optimum of this graph is not known in closed form - the filler keyframes hang on the return side by
        # odometry measured before the correction, and are carried along)
        print("the free part of the old side moved by %.3g; the return side is %.3g from the unscaled world (the correction alone: %.3g)" % (rest, ret, CW.TRUTH_BOUND))
        m.close()
    voc.close(); c.close()
