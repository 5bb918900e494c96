"""LocalMapper.global_bundle_adjust (mo_map_global_ba) on the device against the numpy restatement with its dense solve
(tests/gba_restatement.py) and against the known poses and points of the long-trajectory scenes (tests/gba_cases.py)."""
import copy

import numpy as np
import pytest

from tests.ba_scene import H_IMG, W_IMG
from tests.gba_cases import case, scale_normalised_errors
from tests.test_gba_cpu import MOVED_SEED, NOISE, NOISE_SEED, RECOVERY_A, RECOVERY_A_FREE_SCALE, RECOVERY_B, RECOVERY_STEPS
from tests.test_gpu_bundle_adjust import _ctx, _mapper

pytestmark = pytest.mark.gpu

INT_KEYS = ("n_free", "n_fixed", "n_points", "n_edges", "steps", "accepted", "free", "fixed")
# largest |device - restatement| over the pose entries and the f64 points, as measured on an MI355X (profiles/gba_parity.txt): after one
# step with the solve run to cg_tol 1e-12 (cases A, B, C, D), and after the full run with the defaults (noise and moved edges, cases A and
# C).  The assertions are 100 x that, never looser than 1e-6.
PARITY_MEASURED = 5.33e-10
PARITY_BOUND = min(100 * PARITY_MEASURED, 1e-6)
FULL_MEASURED = 1.93e-12
FULL_BOUND = min(100 * FULL_MEASURED, 1e-6)


def _same_integers(info, ref):
    for k in INT_KEYS:
        assert info[k] == ref[k], (k, info[k], ref[k])
    state = np.zeros(len(ref["kf_state"]), np.int32)
    state[info["free"]] = 2
    state[info["fixed"]] = 1
    assert np.array_equal(state, ref["kf_state"])


def _diff(info, ref):
    loc = ~np.isnan(ref["points"][:, 0])
    assert np.array_equal(loc, ~np.isnan(info["points"][:, 0]))
    return max(float(np.abs(info["poses"] - ref["poses"]).max()), float(np.abs(info["points"][loc] - ref["points"][loc]).max()))


def test_case_a_runs_past_the_limit_of_the_local_solver():
    import vslam_amd as V
    ctx = _ctx()
    s = case("A")
    poses, xyz = s.perturbed()
    m = _mapper(ctx, s, poses, xyz)
    with pytest.raises(V.NativeError):
        m.bundle_adjust(window=0)
    ok, info = m.global_bundle_adjust(fixed=[0, 1])
    print("case A: %d free keyframes, %d points, %d edges; steps %d accepted %d, %d conjugate-gradient iterations; cost %.6g -> %.6g"
          % (info["n_free"], info["n_points"], info["n_edges"], info["steps"], info["accepted"], info["cg_iters"], info["cost"][0], info["cost"][1]))
    assert ok and info["n_free"] == 22 > 16 and info["fixed"] == [0, 1] and info["accepted"] > 0 and info["cost"][1] < 1e-6 * info["cost"][0]
    m.close(); ctx.close()


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_one_step_against_the_restatement(name):
    ctx = _ctx()
    s = case(name)
    poses, xyz = s.perturbed()
    ref = s.restate(poses, xyz, fixed=[0, 1], max_steps=1)
    m = _mapper(ctx, s, poses, xyz)
    ok, info = m.global_bundle_adjust(fixed=[0, 1], max_steps=1, cg_tol=1e-12, max_cg=2000, want_points=True)
    d = _diff(info, ref)
    print("case %s, one step: %d conjugate-gradient iterations; largest difference to the restatement %.3g (bound %.3g); cost %s for %s"
          % (name, info["cg_iters"], d, PARITY_BOUND, info["cost"], ref["cost"]))
    _same_integers(info, ref)
    assert ref["steps"] == 1 and ref["accepted"] == 1
    np.testing.assert_allclose(info["cost"], ref["cost"], rtol=1e-9)
    assert d <= PARITY_BOUND
    m.close(); ctx.close()


@pytest.mark.parametrize("name", ["A", "C"])
def test_full_run_with_noise_and_moved_edges_against_the_restatement(name):
    ctx = _ctx()
    s = case(name, pixel_noise=NOISE, seed=NOISE_SEED)
    poses, xyz = s.perturbed()
    moved = s.move_edges(seed=MOVED_SEED)
    ref = s.restate(poses, xyz, fixed=[0, 1])
    m = _mapper(ctx, s, poses, xyz)
    ok, info = m.global_bundle_adjust(fixed=[0, 1], want_points=True)
    d = _diff(info, ref)
    ei = info["edge_inlier"]
    print("case %s, full run: steps %d accepted %d (restatement %d %d), %d conjugate-gradient iterations; %d of %d moved edges flagged; "
          "largest difference to the restatement %.3g (bound %.3g)"
          % (name, info["steps"], info["accepted"], ref["steps"], ref["accepted"], info["cg_iters"], (ei[moved] == 2).sum(), moved.sum(), d, FULL_BOUND))
    _same_integers(info, ref)
    assert ok == ref["ok"] and info["n_inliers"] == ref["n_inliers"] and np.array_equal(ei, ref["edge_inlier"])
    assert (ei[moved] == 2).all()
    assert d <= FULL_BOUND
    m.close(); ctx.close()


def test_recovery_of_the_truth():
    ctx = _ctx()
    a = case("A")
    poses, xyz = a.perturbed(first_free=1)
    m = _mapper(ctx, a, poses, xyz)
    ok, info = m.global_bundle_adjust(want_points=True, max_steps=RECOVERY_STEPS)   # fixed=None: position 0 alone, the scale free
    loc = ~np.isnan(info["points"][:, 0])
    e_pose, e_pt = scale_normalised_errors(a, info["poses"], info["points"], loc)
    print("case A, position 0 fixed: cost %s, steps %d; after normalising the scale: pose error %.3g, point error %.3g"
          % (info["cost"], info["steps"], e_pose, e_pt))
    assert ok and info["fixed"] == [0] and info["n_free"] == 23 and not (info["edge_inlier"] == 2).any()
    assert e_pose < RECOVERY_A_FREE_SCALE[0] and e_pt < RECOVERY_A_FREE_SCALE[1]
    m.close()
    for s, bound in ((a, RECOVERY_A), (case("B"), RECOVERY_B)):
        poses, xyz = s.perturbed()
        m = _mapper(ctx, s, poses, xyz)
        ok, info = m.global_bundle_adjust(fixed=[0, 1], want_points=True, max_steps=RECOVERY_STEPS)
        loc = ~np.isnan(info["points"][:, 0])
        e_pose, e_pt = s.pose_error(info["poses"]), float(np.abs(info["points"][loc] - s.X[loc]).max())
        print("%d keyframes, positions 0 and 1 fixed: cost %s, steps %d accepted %d, %d iterations; pose error %.3g -> %.3g, point error %.3g"
              % (s.n_kf, info["cost"], info["steps"], info["accepted"], info["cg_iters"], s.pose_error(poses), e_pose, e_pt))
        assert ok and not (info["edge_inlier"] == 2).any()
        assert e_pose < bound[0] and e_pt < bound[1]
        m.close()
    ctx.close()


def test_what_is_written_and_determinism():
    ctx = _ctx()
    s = case("A")
    poses, xyz = s.perturbed()
    lone = np.diff(s.obs_off) < 2
    assert lone.any()
    m = _mapper(ctx, s, poses, xyz)
    before = {k: v.copy() for k, v in m.arrays().items()}
    lists = [a.copy() for a in m.list_arrays()]
    kf_poses = [kf["pose"].copy() for kf in m.keyframes]
    # max_steps = 0: nothing runs, nothing is written
    ok, info = m.global_bundle_adjust(fixed=[0, 1], max_steps=0, want_points=True)
    assert not ok and info["n_free"] == info["n_points"] == info["steps"] == 0 and np.isnan(info["points"]).all()
    m._cache = None
    for k, v in m.arrays().items():
        assert np.array_equal(v, before[k]), k
    ok, info = m.global_bundle_adjust(fixed=[0, 1], want_points=True)
    assert ok and info["accepted"] > 0
    m._cache = None
    after = m.arrays()
    loc = ~np.isnan(info["points"][:, 0])
    assert loc.sum() == info["n_points"] and np.array_equal(loc, ~lone)
    assert np.array_equal(after["xyz"][loc], info["points"][loc].astype(np.float32))
    assert np.array_equal(after["xyz"][~loc], before["xyz"][~loc])          # fewer than two edges: the bytes of before
    assert not np.array_equal(after["xyz"][loc], before["xyz"][loc])
    for k in before:
        if k != "xyz":
            assert np.array_equal(after[k], before[k]), k
    for a, b in zip(lists, m.list_arrays()):
        assert np.array_equal(a, b)
    for k, kf in enumerate(m.keyframes):
        if k in info["free"]:
            assert np.array_equal(kf["pose"][:3, :4], info["poses"][k]) and not np.array_equal(kf["pose"], kf_poses[k])
        else:
            assert np.array_equal(kf["pose"], kf_poses[k])
    # two maps built alike (the second with tiny capacities: every buffer regrown): the same bytes
    m2 = _mapper(ctx, s, poses, xyz, capacity=(2, 16, 16, 32))
    ok2, info2 = m2.global_bundle_adjust(fixed=[0, 1], want_points=True)
    assert ok2 == ok
    for k in info:
        assert np.array_equal(np.asarray(info[k]), np.asarray(info2[k]), equal_nan=True), k
    m2._cache = None
    for k, v in m2.arrays().items():
        assert np.array_equal(v, after[k]), k
    # kP of the free keyframes is K [R | t] of poses_out: a map whose keyframes were STORED at the refined poses, holding the refined
    # points, answers a reader of kP alike (under the stale kP of the perturbed poses the projections are pixels off)
    s3 = copy.copy(s)
    s3.poses = [np.vstack([T, [0.0, 0.0, 0.0, 1.0]]) for T in info["poses"]]
    m3 = _mapper(ctx, s3, s3.poses, after["xyz"])
    s4 = copy.copy(s)
    s4.poses = poses
    stale = _mapper(ctx, s4, poses, after["xyz"])    # keyframes stored at the perturbed poses: the kP a call that wrote none would leave
    r1, r3, r0 = _kp(m), _kp(m3), _kp(stale)
    print("a reader of kP: refined %s, stored at the refined poses %s, at the perturbed poses %s" % (r1, r3, r0))
    assert r1 == r3 and r1 != r0
    m.close(); m2.close(); m3.close(); stale.close(); ctx.close()


def _kp(m):
    """the integers of a fuse_map_points over all keyframes: a reader of the store's kP (it changes the map: the last thing a test does)"""
    info = m.fuse_map_points(window=0, image_size=(W_IMG, H_IMG))
    return {k: v for k, v in info.items() if k != "into"}


def test_a_keyframe_outside_the_problem_keeps_its_bytes():
    """case A with a 25th keyframe of random keypoints that no point observes: outside the problem, its pose stays, and so does every
    result of the call on the 24"""
    ctx = _ctx()
    s = case("A")
    poses, xyz = s.perturbed()
    rng = np.random.default_rng(5)
    s5 = copy.copy(s)
    s5.n_kf = s.n_kf + 1
    s5.kxy = s.kxy + [np.column_stack([rng.uniform(0, W_IMG, 40), rng.uniform(0, H_IMG, 40)]).astype(np.float32)]
    s5.octave = s.octave + [np.zeros(40, np.int32)]
    s5.poses = s.poses + [s.poses[-1]]
    m = _mapper(ctx, s5, poses + [s.poses[-1]], xyz)
    assert len(m.keyframes) == s.n_kf + 1 and len(m.map_points) == len(s.X)
    pose0 = m.keyframes[-1]["pose"].copy()
    ok, info = m.global_bundle_adjust(fixed=[0, 1], want_points=True)
    assert ok and info["n_free"] == 22 and s.n_kf not in info["free"] and s.n_kf not in info["fixed"]
    assert np.array_equal(m.keyframes[-1]["pose"], pose0) and np.array_equal(info["poses"][-1], pose0[:3, :4])
    m24 = _mapper(ctx, s, poses, xyz)
    ok24, info24 = m24.global_bundle_adjust(fixed=[0, 1], want_points=True)
    assert ok24 == ok and np.array_equal(info24["poses"], info["poses"][:-1]) and np.array_equal(info24["points"], info["points"], equal_nan=True)
    m.close(); m24.close(); ctx.close()


def test_tracking_after_global_bundle_adjust_lands_on_the_refined_map():
    """keyframe 5's own keypoints tracked from a pose 0.5 degree / 2 cm off its true one, before and after the call (the local solver's
    test of the same name states why the points outside the problem are kept exact)"""
    from tests.ba_scene import rot
    ctx = _ctx()
    s = case("A")
    poses, xyz = s.perturbed()
    xyz[~s.problem] = s.X[~s.problem]
    m = _mapper(ctx, s, poses, xyz)
    kf = m.keyframes[5]
    kps, desc = np.array(kf["keypoints"]).copy(), np.array(kf["descriptors"]).copy()
    P = np.eye(4)
    P[:3, :3] = rot([0.0, np.deg2rad(0.5), 0.0]); P[:3, 3] = [0.02, 0.0, 0.0]
    pred = P @ s.poses[5]

    def err(T):
        return float(np.abs(T[:3, :4] - s.poses[5][:3, :4]).max())
    ok0, T0, i0 = m.track_local_map(kps, desc, pred, window=0, image_size=(W_IMG, H_IMG))
    okb, info = m.global_bundle_adjust(fixed=[0, 1], max_steps=RECOVERY_STEPS)
    ok1, T1, i1 = m.track_local_map(kps, desc, pred, window=0, image_size=(W_IMG, H_IMG))
    print("tracked pose error: before %.3g (ok %s), after %.3g (ok %s); refined keyframe pose %.3g" % (err(T0), ok0, err(T1), ok1, err(m.keyframes[5]["pose"])))
    assert okb and ok1 and err(T1) <= err(T0)
    assert err(T1) < 10 * RECOVERY_A[0] + 1e-6   # (tracking's own bound on exact data, < 1e-6, on top of the map's)
    m.close(); ctx.close()


def test_argument_and_empty_cases():
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    from tests.ba_scene import K
    ctx = _ctx()
    s = case("A")
    poses, xyz = s.perturbed()
    m = _mapper(ctx, s, poses, xyz)
    before = {k: v.copy() for k, v in m.arrays().items()}
    bad = [dict(max_steps=-1), dict(max_steps=101), dict(max_cg=0), dict(cg_tol=-1.0), dict(cg_tol=float("nan")), dict(step_tol=-1.0),
           dict(step_tol=float("inf")), dict(scale_factor=0.0), dict(scale_factor=float("nan")), dict(chi2=-1.0), dict(chi2=float("inf")),
           dict(fixed=[]), dict(fixed=[s.n_kf + 3])]   # (the last two: no fixed position takes part)
    for kw in bad:
        with pytest.raises(V.NativeError):
            m.global_bundle_adjust(**kw)
    m.keyframes[3]["pose"][0, 3] = np.nan
    with pytest.raises(V.NativeError):
        m.global_bundle_adjust()
    m.keyframes[3]["pose"][:] = poses[3]
    m._cache = None
    for k, v in m.arrays().items():
        assert np.array_equal(v, before[k]), k
    # every participant fixed: nothing runs, not an error
    ok, info = m.global_bundle_adjust(fixed=range(s.n_kf))
    assert not ok and info["n_free"] == info["n_fixed"] == info["n_points"] == info["n_edges"] == info["steps"] == 0 and info["free"] == []
    m._cache = None
    for k, v in m.arrays().items():
        assert np.array_equal(v, before[k]), k
    empty = LocalMapper(K, save_every_keyframe=False, context=ctx)
    ok, info = empty.global_bundle_adjust()
    assert not ok and info["n_free"] == 0 and info["steps"] == 0
    with pytest.raises(ValueError):
        empty.detect_loop(sim3=True, confirm=True, correct=True, global_ba=True)
    m.close(); empty.close(); ctx.close()


def test_scratch_poison():
    """case A on a rebuilt map under two poison bytes gives the outputs and the map of the unpoisoned run"""
    from tests.test_gpu_scratch_poison import _checked, _ctx as pctx, _flat, _map_state, _same, _set
    s = case("A")
    poses, xyz = s.perturbed()
    c = pctx()
    try:
        def run(poisoned):
            m = _checked(c, lambda: _mapper(c, s, poses, xyz), poisoned)
            ok, info = _checked(c, lambda: m.global_bundle_adjust(fixed=[0, 1], want_points=True), poisoned)
            assert ok and info["accepted"] > 0
            got = _flat((info, _map_state(m), _kp(m)))
            m.close()
            return got
        want = run(False)
        for byte in (255, 90):
            _set(c, byte)
            _same(run(True), want, (byte, "global bundle adjustment"))
            assert c.dev_status() == 0
    finally:
        c.close()


def _problem_inliers(m, w, chi2=5.991):
    """the observations of the points with at least two valid ones - the edges of the global problem - whose point reprojects within the
    chi2 gate under its keyframe's kf["pose"] (every keypoint of the loop world is of octave 0: information 1)"""
    from tests.track_restatement import valid_observations
    m._cache = None
    a = m.arrays()
    n = tot = 0
    for i, v in enumerate(valid_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], w.counts)):
        if len(v) < 2:
            continue
        X = a["xyz"][i].astype(np.float64)
        for k, row in v:
            T = np.asarray(m.keyframes[k]["pose"], np.float64)
            x = w.K @ (T[:3, :3] @ X + T[:3, 3])
            d = x[:2] / x[2] - np.asarray(w.kf_xy[k][row], np.float64)
            n += bool(x[2] > 0 and d @ d <= chi2)
            tot += 1
    return n, tot


def test_detect_loop_with_global_ba_on_the_noisy_rescaled_loop_world():
    """detect_loop(26, sim3=True, confirm=True, correct=True, optimize=True, global_ba=True) on the loop world with its return side drifted
    by a scale of 1.3 and 0.5 px of noise on every keypoint: the global bundle adjustment behind the essential graph is ok, its robust
    cost does not rise, and of the problem's edges (the observations of the points with two or more: a point with one observation is
    outside the problem and keeps its bytes while its keyframe moves) no fewer reproject within the chi2 gate than before the call"""
    import vslam_amd as V
    from tests import loop_worlds as LW
    from tests.test_gpu_posegraph import FACTOR
    from tests.test_gpu_sim3 import _rescaled
    c = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    w = copy.copy(_rescaled(LW.loop_world(), FACTOR))
    rng = np.random.default_rng(3)
    w.kf_xy = [(xy + rng.normal(0, 0.5, xy.shape)).astype(np.float32) for xy in w.kf_xy]
    words, weights = LW.loop_vocabulary()
    voc = V.Vocabulary.from_arrays(words, weights, context=c)
    m = w.build(c)
    m.set_vocabulary(voc)
    n0, tot0 = _problem_inliers(m, w)
    m._loop_consistency = None
    got = [m.detect_loop(p, sim3=True, confirm=True, correct=(p == 26), optimize=(p == 26), global_ba=(p == 26), seed=11) for p in LW.RETURN_POS]
    assert [f for f, _ in got] == [p == 26 for p in LW.RETURN_POS]
    a = got[-1][1]["accepted"]
    g = a["global_ba"]
    n1, tot1 = _problem_inliers(m, w)
    print("global BA behind the loop: %s; cost %.6g -> %.6g; inlier edges %d of %d before the call, %d of %d after (the call's own count: %d of %d)"
          % ({k: g[k] for k in ("n_free", "n_fixed", "n_points", "n_edges", "steps", "accepted", "cg_iters")}, g["cost"][0], g["cost"][1], n0, tot0, n1, tot1,
             g["n_inliers"], g["n_edges"]))
    assert a["optimize"]["ok"] and g["ok"] and g["accepted"] > 0 and g["fixed"] == [0]
    assert g["cost"][1] <= g["cost"][0] and n1 >= n0 and g["n_inliers"] >= n0
    for k, kf in enumerate(m.keyframes):
        assert np.array_equal(np.asarray(kf["pose"], np.float64)[:3, :4], g["poses"][k])
    m.close(); voc.close(); c.close()
