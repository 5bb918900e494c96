"""LocalMapper.correct_loop (mo_map_loop_correct) on the device against tests/correct_restatement.py on the constructed cases of
tests/correct_cases.py, and detect_loop(sim3=True, confirm=True, correct=True) on the loop worlds.  Every integer, `into`, `moved` and the
observation arrays must be equal; xyz must hold the bytes the restatement gets from the call's own A; the projections are restated under
the call's own poses_out.  A and poses_out themselves are held to ten times the largest difference to the f64 restatement measured over
all cases (A_POSE_MEASURED)."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import correct_cases as CC
from tests import correct_restatement as CR
from tests import correct_worlds as CW

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in CC.all_cases()}
STAGES = ["correct_move", "correct_search", "correct_merge"]
# The largest |device - restatement| over A, A_scale and poses_out of every case, measured on one MI355X: 0 on all 27 cases - the host side of
# the library forms them in the restatement's operation order and neither compiler reorders or fuses.  The bound is ten times the
# measurement, so the values must be equal; a build that rounds otherwise has to measure again and write its number here.
A_POSE_MEASURED = 0.0
A_POSE_BOUND = 10 * A_POSE_MEASURED


@pytest.fixture(scope="module")
def ctx():
    import vslam_amd as V
    c = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    yield c
    c.close()


def _state(m):
    m._cache = None
    return {f: v.copy() for f, v in m.arrays().items()}


def _compare(case, before, info, after, m):
    """device against the restatement of `before` under the call's own A and poses_out; returns the largest difference of A / poses"""
    own = case.restate(before, A=info["A"], poses_out=info["poses"])
    pure = case.restate(before)
    for k in CR.COUNTS:
        assert info[k] == own["counts"][k] == pure["counts"][k], (case.name, k, info[k], own["counts"][k], pure["counts"][k])
    assert np.array_equal(info["into"], own["into"]) and np.array_equal(info["moved"], own["moved"]), case.name
    for f in ("id", "color", "obs_off", "obs_kf", "obs_kp", "dref_kf", "dref_row"):
        assert np.array_equal(after[f], own["arrays"][f]), (case.name, f)
    assert after["xyz"].tobytes() == own["arrays"]["xyz"].tobytes(), (case.name, np.flatnonzero((after["xyz"] != own["arrays"]["xyz"]).any(axis=1)))
    assert info["corrected"] == np.flatnonzero(case.masks()[0]).tolist() and info["group"] == np.flatnonzero(case.masks()[1]).tolist()
    d = max(np.abs(info["A"] - pure["A"]).max(), abs(info["A_scale"] - pure["A_scale"]), np.abs(info["poses"] - pure["poses_out"]).max())
    for k, kf in enumerate(m.keyframes):   # the host poses follow
        assert np.array_equal(np.asarray(kf["pose"], np.float64)[:3, :4], info["poses"][k]), (case.name, k)
    return d, own


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_restatement(name, ctx):
    case = CASES[name]
    CC.check(case)   # the case's conditions, before any device is asked
    t0 = time.perf_counter()
    m = case.build_map(ctx)
    before = _state(m)
    t1 = time.perf_counter()
    info = case.call(m)
    t2 = time.perf_counter()
    after = _state(m)
    d, own = _compare(case, before, info, after, m)
    CC.check(case, own)   # what the case was built to show holds of the device's result too
    print("%s: largest difference of A / poses_out to the f64 restatement %.3g (bound %.3g); error to the true world %.3g; map %.3f s, call %.3f s"
          % (name, d, A_POSE_BOUND, CC.truth_error(case, own), t1 - t0, t2 - t1))
    assert d <= A_POSE_BOUND, (name, d)
    if own["fused"]:
        assert len(after["id"]) == info["n_points"] < len(before["id"]) or info["n_absorbed"] == 0
    else:
        assert info["n_points"] == len(before["id"]) and np.array_equal(info["into"], np.arange(len(before["id"])))
    m.close()


def test_two_calls_give_equal_bytes(ctx):
    from tests.test_gpu_scratch_poison import _flat
    for name in ("points:257", "rows:1025", "stale_observations"):
        case = CASES[name]
        got = []
        for other in (False, True):
            m = case.build_map(ctx)
            if other:   # another call in between leaves its own scratch behind
                x = CASES["chain"].build_map(ctx)
                CASES["chain"].call(x)
                x.close()
            info = case.call(m)
            got.append(_flat((info, _state(m))))
            m.close()
        assert got[0] == got[1], name


def test_stage_names(ctx):
    case = CASES["scale:1.3"]
    m = case.build_map(ctx)
    ctx.set_host_timing(True)
    info = case.call(m)
    names = [n for n, _ in ctx.stage_times()]
    ctx.set_host_timing(False)
    m.close()
    assert info["n_absorbed"] > 0 and names == STAGES


def _raw(m, case, **over):
    """mo_map_loop_correct called directly with every output array NULL: (rc, MapCorrectOut)"""
    import vslam_amd as V
    case.finish()
    n_kf = len(case.kf)
    Ka = np.ascontiguousarray(CC.K, np.float64).reshape(9)
    Pa = np.ascontiguousarray(np.stack([T[:3, :4] for T in case.poses()]), np.float64).reshape(n_kf, 12)
    cm, gm = case.masks()
    cm, gm = cm.copy(), gm.copy()
    if over.pop("drop_p", False):
        cm[case.p] = 0
    if over.pop("both", False):
        gm[np.flatnonzero(cm)[0]] = 1
    s, R, t = case.model()
    R, t = np.array(R, np.float64).reshape(9), np.array(t, np.float64)
    if "R0" in over:
        R[0] = over.pop("R0")
    if "t0" in over:
        t[0] = over.pop("t0")
    lp = case.loop_point()
    f = dict(kf_pos=case.p, cand_pos=case.q, scale=s, w=CC.W_IMG, h=CC.H_IMG, **CC.PRM)
    f.update(over)
    p = V.MapCorrectParams(f["kf_pos"], f["cand_pos"], f["scale"], (C.c_double * 9)(*R), (C.c_double * 3)(*t), cm.ctypes.data, gm.ctypes.data,
                           None if lp is None else lp.ctypes.data, f["w"], f["h"], f["radius"], f["scale_factor"], f["max_dist"], f["chi2"])
    o = V.MapCorrectOut()
    rc = m.lib.mo_map_loop_correct(m._h, V._ptr(Ka), V._ptr(Pa), C.byref(p), C.byref(o))
    return rc, o


def test_errors_and_empties(ctx):
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    case = CASES["scale:1.3"]
    m = case.build_map(ctx)
    before = _state(m)
    for bad, code in CC.error_calls(len(case.kf)):
        assert _raw(m, case, **dict(bad))[0] == getattr(V, "MO_ERR_" + code), bad
    assert all(np.array_equal(before[f], x) for f, x in _state(m).items())   # a refused call leaves the map alone
    rc, o = _raw(m, case)                                                   # every output array NULL: legal
    want = case.restate(before)["counts"]
    assert rc == V.MO_OK and all(getattr(o, k) == want[k] for k in CR.COUNTS)
    empty = LocalMapper(CC.K, save_every_keyframe=False, context=ctx)
    rc, o = _raw(empty, case)
    assert rc == V.MO_OK and all(getattr(o, k) == 0 for k in CR.COUNTS) and o.A_scale == 1.0
    with pytest.raises(ValueError):
        m.detect_loop(correct=True, sim3=True)
    with pytest.raises(ValueError):
        m.correct_loop({"win": -1, "candidates": []})
    m.close(); empty.close()


def test_poison():
    """the call on a rebuilt map under the poison bytes 255, 0 and 90 gives the bytes of the unpoisoned run, and the fill totals grow"""
    from tests.test_gpu_scratch_poison import _map_state, _write_sweep
    cases = [CASES[n] for n in ("points:257", "stale_observations", "empty_group", "search_on_given_row")]

    def run(ctx, call):
        out = []
        for case in cases:
            m = call(lambda: case.build_map(ctx))
            info = call(lambda: case.call(m))
            out.append((info, _map_state(m)))
            m.close()
        assert out[0][0]["n_absorbed"] == 6 and out[2][0]["n_moved"] == 6   # the calls find what they look for: nothing compares empty results
        return out
    _write_sweep(run)


def test_the_corrected_map_serves_its_readers(ctx):
    """kP, xyz and the host poses agree with one another after a correction: track_local_map from the true pose of p finds every loop
    point of its rows as an inlier and returns that pose; fuse_map_points - which reads the store's own kP - equals its restatement
    under P = K [R | t] of the host poses; bundle_adjust runs on the corrected keyframes."""
    from tests import fuse_restatement as FR
    from tests.map_worlds import kps_array
    case = CASES["tracking"]
    m = case.build_map(ctx)
    info = case.call(m)
    assert info["n_absorbed"] == 40 and info["n_moved"] == 40
    k = case.kf[case.p]
    T_true = case.true_pose[case.p]
    assert np.abs(np.asarray(m.keyframes[case.p]["pose"])[:3, :4] - T_true[:3, :4]).max() < 1e-12
    ok, T, tr = m.track_local_map(kps_array(np.array(k["xy"]), np.array(k["oct"], np.int32)), np.array(k["desc"], np.uint8), T_true, window=0, radii=(4.0,),
                                  image_size=(CC.W_IMG, CC.H_IMG))
    print("tracking: %d matches, %d inliers, pose off by %.3g" % (tr["pass_matches"][-1], tr["pass_inliers"][-1], np.abs(T - T_true).max()))
    assert ok and tr["pass_inliers"][-1] >= 40 and np.abs(T - T_true).max() < 1e-5
    rows = [fe["row"][case.p] for fe in case.f_dup]
    assert np.array_equal(tr["point"][rows], info["into"][[fe["L"] for fe in case.f_dup]]) and tr["inlier"][rows].all()
    before = _state(m)
    poses = [np.asarray(kf["pose"], np.float64) for kf in m.keyframes]
    want = FR.fuse(before, FR.store_P(CC.K, poses), [q["xy"] for q in case.kf], [q["oct"] for q in case.kf],
                   [np.array(q["desc"], np.uint8).reshape(-1, 32) for q in case.kf], CC.W_IMG, CC.H_IMG, window=0)
    assert want[3]["min"] >= CC.MARGIN
    got = m.fuse_map_points(window=0, image_size=(CC.W_IMG, CC.H_IMG))
    assert all(got[c] == want[2][c] for c in FR.COUNTS), (got, want[2])
    assert got["n_cand"] > 0 and got["n_absorbed"] == 0   # (the correction left no duplicate behind)
    ok, ba = m.bundle_adjust(window=0, min_inliers=10)
    assert ba["n_free"] > 0 and ba["n_edges"] > 0 and np.isfinite(ba["poses"]).all()
    m.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
FACTOR = 1.3


def test_detect_loop_with_correction_on_the_loop_worlds():
    """The loop world plain and with its return side rescaled by 1.3 (drifted): detect_loop(26, sim3=True, confirm=True, correct=True)
    absorbs every duplicate confirm's loop_point names into the old point of the same world id, moves no old point, and puts the poses
    20, 22, 24, 26 and the surviving duplicates back at the unscaled world within CW.TRUTH_BOUND; the filler keyframes and every point
    outside the two sides keep their bytes; the co-visibility graph gains edges across the loop."""
    import vslam_amd as V
    from tests import loop_worlds as LW
    from tests.test_gpu_sim3 import _rescaled
    c = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    base = LW.loop_world()
    words, weights = LW.loop_vocabulary()
    voc = V.Vocabulary.from_arrays(words, weights, context=c)
    # on the CPU first: the corrected set is exactly the return keyframes and at least 40 loop points exist
    pre = CW.restated(_rescaled(base, FACTOR), FACTOR)
    assert pre["corrected"] == list(LW.RETURN_POS) and int((pre["loop_point"] >= 0).sum()) >= 40 and pre["res"]["counts"]["n_absorbed"] >= 40
    for tag, w, factor in (("plain", base, 1.0), ("rescaled", _rescaled(base, FACTOR), FACTOR)):
        m = w.build(c)
        m.set_vocabulary(voc)
        before = _state(m)
        poses0 = [np.asarray(kf["pose"], np.float64).copy() for kf in m.keyframes]
        graph0 = {a: dict(b) for a, b in m.co_visibility_graph.items()}
        m._loop_consistency = None
        got = [m.detect_loop(p, sim3=True, confirm=True, correct=(p == 26), seed=11) for p in LW.RETURN_POS]
        assert [f for f, _ in got] == [p == 26 for p in LW.RETURN_POS], tag
        a = got[-1][1]["accepted"]
        cf, co = a["confirm"], a["correct"]
        after = _state(m)
        assert co["corrected"] == list(LW.RETURN_POS) and a["pos"] == 3 and not set(co["group"]) & set(co["corrected"])
        lpt = cf["loop_point"]
        named, wrong, old_moved, e = CW.facts(w, base, {"into": co["into"], "moved": co["moved"], "xyz": after["xyz"], "ids": after["id"],
                                                          "poses": co["poses"], "loop_point": lpt})
        print("%s: %s; %d named duplicates absorbed; error to the unscaled world %.3g (bound %.3g, restated %.3g)"
              % (tag, {k: co[k] for k in CR.COUNTS}, named, e, CW.TRUTH_BOUND, CW.TRUTH_RESTATED))
        assert int((lpt >= 0).sum()) >= 40 and named >= 40 and wrong == [] and old_moved == 0
        assert co["n_absorbed"] >= named and co["n_points"] == len(after["id"]) == len(before["id"]) - co["n_absorbed"]
        assert e <= CW.TRUTH_BOUND, (tag, e)
        for k, kf in enumerate(m.keyframes):
            T = np.asarray(kf["pose"], np.float64)
            if k in LW.RETURN_POS:
                assert np.abs(T[:3, :4] - np.asarray(base.kf_poses[k], np.float64)[:3, :4]).max() <= CW.TRUTH_BOUND
            else:
                assert T.tobytes() == poses0[k].tobytes(), (tag, k)
        # every old point keeps its bytes; points seen by fillers only (none here) and by the old side only do too
        old = np.arange(w.n_old)
        assert np.array_equal(after["xyz"][co["into"][old]], before["xyz"][old]) and np.array_equal(after["id"][co["into"][old]], before["id"][old])
        ret_ids, old_ids = [m.keyframes[k]["id"] for k in LW.RETURN_POS], {m.keyframes[k]["id"] for k in co["group"]}
        gained = [(x, y) for x in ret_ids for y in old_ids if m.co_visibility_graph[x].get(y, 0) > graph0.get(x, {}).get(y, 0)]
        assert gained and co["loop_connections"] and set(co["loop_connections"]) == set(ret_ids)
        assert any(set(v) & old_ids for v in co["loop_connections"].values()) and not any(set(v) & set(ret_ids) for v in co["loop_connections"].values())
        m.close()
    voc.close(); c.close()
