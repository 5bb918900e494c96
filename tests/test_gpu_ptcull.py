"""The life of a map point on the device map (mo_map_point_life, mo_map_note_tracking, mo_map_points_bad, mo_map_erase_points,
mo_map_cull_points; LocalMapper's point_life / note_tracking / cull_map_points / erase_map_points) against tests/ptcull_restatement.py on
the worlds of tests/ptcull_worlds.py: everything is integers and must be equal.  tests/test_ptcull_cpu.py shows what each world is there
to exclude."""
import copy
import ctypes as C

import numpy as np
import pytest

from tests import ptcull_restatement as PR
from tests import ptcull_worlds as PW
from tests import track_restatement as TR
from tests.fuse_worlds import map_inputs
from tests.map_worlds import BA_STEPS, BA_WINDOW, build_map, perturbed, perturbed_pose, pose_near, world

pytestmark = pytest.mark.gpu

TINY = (2, 16, 16, 32)


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _snap(m):
    m._cache = None
    return {k: v.copy() for k, v in m.arrays().items()}


def _life(m):
    p = m.point_life()
    return np.column_stack([p["visible"], p["found"], p["born"]]).astype(np.int32), p["now"]


def _same_bytes(a, b, fields=None):
    for f in fields or a:
        assert a[f].dtype == b[f].dtype and a[f].tobytes() == b[f].tobytes(), f


def _equals(removed, info, r):
    assert info["reason"].tolist() == r["reason"].tolist() and info["removed"].tolist() == r["removed"].tolist()
    assert removed == r["removed_indices"] and info["n_removed"] == r["n_removed"] and info["n_tested"] == r["n_tested"]
    assert info["n_reason"] == r["n_reason"] and info["now"] == r["now"]


def _vary(m, seed=5):
    """a note_tracking call with an empty local map and a made-up match list: the records differ from point to point"""
    rng = np.random.default_rng(seed)
    n = len(m.map_points)
    pt = rng.integers(0, n, n).astype(np.int32)
    inl = rng.random(n) < 0.4
    before, _ = _life(m)
    a = m.arrays()
    m.note_tracking(np.eye(4), {"point": pt, "inlier": inl}, local_keyframes=[])
    want, _ = PR.note(before, a["xyz"], a["obs_off"], a["obs_kf"], a["obs_kp"], [kf._rows for kf in m.keyframes], m.camera_matrix, np.eye(4), 640, 480,
                      pt, inl, local_keyframes=[])
    got, _ = _life(m)
    assert np.array_equal(got, want) and len(set(map(tuple, got.tolist()))) > 2
    return got


# ---- 1. the decision; 3. the records through add_keyframe's cull, add_observations, erase_keyframes, capacity growth -------------------------
@pytest.mark.parametrize("name", list(PW.CASES))
def test_decision_equals_the_restatement(name):
    ctx = _ctx()
    w = PW.case(name)
    m = PW.build(ctx, w)
    before = _snap(m)
    for f, want in w.arrays().items():
        assert before[f].tobytes() == want.tobytes(), f
    life, now = _life(m)
    assert np.array_equal(life, w.life) and now == w.now   # born through every rebuild of the script, the counters through the notes
    r = PW.decide(w)
    kw = dict(w.kw)
    for _ in range(2):
        _equals(*m.cull_map_points(erase=False, **kw), r)
    _same_bytes(before, _snap(m))
    assert np.array_equal(_life(m)[0], life)
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_records_survive_capacity_growth():
    ctx = _ctx()
    w = PW.case("age_window")
    m = PW.build(ctx, w, capacity=TINY)   # 16 points, 32 observations: every injection regrows the store
    life, now = _life(m)
    assert np.array_equal(life, w.life) and now == w.now
    _equals(*m.cull_map_points(erase=False), PW.decide(w))
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


# ---- 2. the erase --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["large", "age_window", "invalid_entry", "protect"])
def test_erase_equals_the_restatement_and_cull_erases_what_it_decides(name):
    ctx = _ctx()
    w = PW.case(name)
    r = PW.decide(w)
    want, want_life, want_remap = PR.erase(w.arrays(), w.life, r["removed"])
    maps = []
    for how in ("erase", "cull"):
        m = PW.build(ctx, w)
        a0 = _snap(m)
        if how == "erase":
            remap = m.erase_map_points(r["removed"]) if name != "age_window" else m.erase_map_points(r["removed_indices"])
        else:
            removed, info = m.cull_map_points(**w.kw)
            _equals(removed, info, r)
            remap = info["remap"]
            assert info["n_points"] == len(want["id"]) and info["n_obs"] == len(want["obs_kf"])
        assert np.array_equal(remap, want_remap)
        a = _snap(m)
        for f in want:
            assert a[f].tobytes() == want[f].tobytes(), (how, f)
        keep = ~r["removed"]
        for f in ("color", "dref_kf", "dref_row"):
            assert a[f].tobytes() == a0[f][keep].tobytes(), (how, f)
        assert np.array_equal(_life(m)[0], want_life) and len(m.map_points) == len(want["id"])
        maps.append(m)
    _same_bytes(_snap(maps[0]), _snap(maps[1]))
    # what is left decides as the restatement says, and erasing nothing changes no byte
    m = maps[0]
    r2 = PR.decide(want_life, w.now, want["obs_off"], want["obs_kf"], want["obs_kp"], w.counts,
                   **{k: (v[~r["removed"]] if k == "protect" else v) for k, v in w.kw.items()})
    kw2 = {k: (v[~r["removed"]] if k == "protect" else v) for k, v in w.kw.items()}
    _equals(*m.cull_map_points(erase=False, **kw2), r2)
    snap, version = _snap(m), m._version
    assert np.array_equal(m.erase_map_points([]), np.arange(len(want["id"])))
    assert np.array_equal(m.erase_map_points(np.zeros(len(want["id"]), bool)), np.arange(len(want["id"])))
    if not r2["n_removed"]:
        removed, info = m.cull_map_points(**kw2)
        assert removed == [] and np.array_equal(info["remap"], np.arange(len(want["id"])))
    _same_bytes(snap, _snap(m))
    assert m._version == version and np.array_equal(_life(m)[0], want_life)
    assert ctx.dev_status() == 0
    for m in maps:
        m.close()
    ctx.close()


def test_erased_map_equals_its_twin():
    """the consecutive-keyframe world (positions 1 and 5 removed earlier: position != slot): every point that at most two keyframes observe
    is culled (every age tested, no minimum age); the map then is the map built from the survivors alone, and serves its readers like it"""
    from tests.test_gpu_map_reads import _same_track
    from tests.covis_restatement import covisibility as covis_restated
    ctx = _ctx()
    w = world("ba")
    poses, xyz = perturbed(w, first_free=4)
    m = build_map(ctx, w, poses=poses, xyz=xyz)
    a0 = _snap(m)
    life0, now = _life(m)
    assert (life0 == [1, 1, now]).all() and now == w.n_kf0 - 1
    kw = dict(max_age=-1, min_age=0)
    r = PR.decide(life0, now, w.obs_off, w.obs_kf, w.obs_kp, w.counts, **kw)
    removed, info = m.cull_map_points(**kw)
    _equals(removed, info, r)
    keep = ~r["removed"]
    assert 100 < r["n_removed"] < len(keep) - 100 and r["n_reason"][2] == r["n_removed"]
    want, want_life, want_remap = PR.erase(a0, life0, r["removed"])
    assert np.array_equal(info["remap"], want_remap)
    w2 = copy.copy(w)
    w2.obs = [o for o, k in zip(w.obs, keep) if k]
    w2.ids = w.ids[keep]
    twin = build_map(ctx, w2, poses=poses, xyz=xyz[keep])
    after = _snap(m)
    _same_bytes(after, want)
    # (dref_kf of an injected point is its index among the dicts the host was given: the twin was given fewer, the restatement has it)
    shared = [f for f in after if f != "dref_kf"]
    _same_bytes(after, _snap(twin), shared)
    assert [p["id"] for p in m.map_points[:50]] == [p["id"] for p in twin.map_points[:50]]
    assert np.array_equal(_life(m)[0], _life(twin)[0]) and np.array_equal(_life(m)[0], want_life)
    W = covis_restated(want["obs_off"], want["obs_kf"], want["obs_kp"], w.counts)
    assert np.array_equal(m.covisibility(), W) and np.array_equal(twin.covisibility(), W)
    T = pose_near(w, 7)
    kps, desc = w.track_query(T, octave_spread=1)
    pose0 = perturbed_pose(T)
    ta, tb = m.track_local_map(kps, desc, pose0), twin.track_local_map(kps, desc, pose0)
    assert ta[2]["n_local"] > 0 and ta[2]["pass_matches"][0] >= 20
    _same_track(ta, tb)
    oka, ia = m.bundle_adjust(window=BA_WINDOW, max_steps=BA_STEPS, want_points=True)
    okb, ib = twin.bundle_adjust(window=BA_WINDOW, max_steps=BA_STEPS, want_points=True)
    assert oka == okb and ia["n_edges"] > 0
    for k in ia:
        assert np.array_equal(np.asarray(ia[k]), np.asarray(ib[k]), equal_nan=True), k
    _same_bytes(_snap(m), _snap(twin), shared)
    assert ctx.dev_status() == 0
    m.close(); twin.close(); ctx.close()


# ---- 3. carried and merged: the calls that create points or merge them ---------------------------------------------------------------------
def test_created_points_are_born_now():
    from tests import grow_worlds as GW
    ctx = _ctx()
    w, held = GW.withheld_points_world()
    m = build_map(ctx, w)
    before = _vary(m)
    now = _life(m)[1]
    info = m.create_new_map_points(window=0)
    assert info["n_new"] > 20 and info["n_points"] == len(before) + info["n_new"]
    got, now2 = _life(m)
    assert np.array_equal(got, PR.appended(before, info["n_new"], now)) and now2 == now == len(w.slot_poses) - 1
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_fused_points_take_the_sums():
    from tests import fuse_worlds as FW
    ctx = _ctx()
    w, unsplit, n_split = FW.split_world()
    m = build_map(ctx, w)
    before = _vary(m)
    a = _snap(m)
    n_valid = [len(v) for v in TR.valid_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], w.counts)]
    info = m.fuse_map_points(window=0, image_size=w.image_size)
    assert info["n_absorbed"] == n_split > 100
    want = PR.merged(before, info["into"], n_obs_valid=n_valid)
    got, _ = _life(m)
    assert np.array_equal(got, want)
    members = np.bincount(info["into"])
    assert (got[members == 2, 0] >= 2).all() and got[:, 0].sum() == before[:, 0].sum() and got[:, 1].sum() == before[:, 1].sum()
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_loop_correction_merges_the_records():
    from tests import correct_cases as CC
    ctx = _ctx()
    case = {c.name: c for c in CC.all_cases()}["points:257"]
    m = case.build_map(ctx)
    before = _vary(m)
    a0 = _snap(m)
    info = case.call(m)
    a1 = _snap(m)
    assert info["n_absorbed"] > 0
    into = np.asarray(info["into"])
    survivors = []
    for r in range(info["n_points"]):   # the member whose identity the new point carries
        mem = np.flatnonzero(into == r)
        s = [i for i in mem if a0["id"][i] == a1["id"][r] and a0["dref_kf"][i] == a1["dref_kf"][r] and a0["dref_row"][i] == a1["dref_row"][r]]
        assert len(s) == 1, (r, mem)
        survivors.append(s[0])
    got, _ = _life(m)
    assert np.array_equal(got, PR.merged(before, into, survivors=survivors))
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


# ---- 4. note_tracking ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("local", ["window", "covisible"])
def test_note_tracking_sees_what_tracking_searches(local):
    from tests import view_worlds as VW
    ctx = _ctx()
    c = VW.track_case("track")
    w = c["w"]
    kps, desc, pose0 = c["kps"], c["desc"], c["pose0"]
    maps = [w.build(ctx), w.build(ctx)]
    lives = []
    for m in maps:
        a, P, _, octv, dsc = map_inputs(m)
        counts = [len(d) for d in dsc]
        life, now = _life(m)
        for frustum in (True, False):
            ok, _, info = m.track_local_map(kps, desc, pose0, radii=(15.0,), window=5, local=local, frustum=frustum)
            assert info["pass_matches"][0] >= 20 and 0 < info["n_local"] < len(a["xyz"])
            cnt = m.note_tracking(pose0, info, window=5, frustum=frustum)
            assert cnt["n_seen"] == info["pass_cand"][0] and cnt["n_local"] == info["n_local"]
            if frustum:
                assert cnt["n_seen"] < info["pass_in_image"][0]
            fr = dict(kf_oct=octv, kf_P=P) if frustum else None
            life, want = PR.note(life, a["xyz"], a["obs_off"], a["obs_kf"], a["obs_kp"], counts, VW.K, pose0, VW.W_IMG, VW.H_IMG, info["point"],
                                 info["inlier"], window=5, local_keyframes=info.get("local_keyframes"), frustum=fr)
            assert cnt == want and cnt["n_matched"] == info["pass_matches"][0] and cnt["n_found"] == info["pass_inliers"][0]
            assert np.array_equal(_life(m)[0], life)
        # a point that two keypoints name is counted once; entries out of range are ignored
        p = int(info["point"][info["point"] >= 0][0])
        pt = np.array([p, p, p, -1, len(a["xyz"]), 2 ** 31 - 1], np.int32)
        inl = np.array([0, 1, 1, 1, 1, 1], bool)
        cnt = m.note_tracking(pose0, {"point": pt, "inlier": inl}, local_keyframes=[])
        assert cnt == dict(n_local=0, n_seen=0, n_matched=1, n_found=1)
        life[p, :2] += 1
        assert np.array_equal(_life(m)[0], life)
        assert (life[:, 1] <= life[:, 0]).all() and life[:, 0].max() >= 3 and (life[:, 2] == now).all()
        lives.append(m.point_life())
    for f in ("visible", "found", "born"):
        assert lives[0][f].tobytes() == lives[1][f].tobytes(), f   # equal maps, equal calls: equal bytes
    assert ctx.dev_status() == 0
    for m in maps:
        m.close()
    ctx.close()


# ---- 5. one sequence -----------------------------------------------------------------------------------------------------------------------
def test_wrong_points_leave_and_true_points_stay():
    """tests/ptcull_worlds.sequence(): fifty points from wrong matches among the true ones.  Four keyframes, each behind two tracked
    frames that are noted, each followed by the cull: exactly the fifty leave (never found again, their ratio falls below 0.25 at the
    second keyframe), and every record is what the restatement derives from the tracking results"""
    from tests import view_worlds as VW
    ctx = _ctx()
    s = PW.sequence()
    w, wrong = s["w"], s["wrong"]
    m = w.build(ctx)
    n = len(w.obs)
    assert 150 <= n <= 400 and len(wrong) == PW.N_WRONG
    ids = np.arange(n)
    life, now = _life(m)
    assert now == VW.N_KF - 1 and (life == [1, 1, now]).all()
    gone = []
    img = np.zeros((VW.H_IMG, VW.W_IMG), np.uint8)
    for j, (Tk, frames) in enumerate(s["steps"]):
        for T, kps, desc in frames:
            ok, pose, info = m.track_local_map(kps, desc, VW.perturbed(T), window=0, frustum=True)
            assert ok and info["pass_inliers"][-1] >= 30
            a, P, _, octv, dsc = map_inputs(m)
            cnt = m.note_tracking(pose, info, window=0, frustum=True)
            life, want = PR.note(life, a["xyz"], a["obs_off"], a["obs_kf"], a["obs_kp"], [len(d) for d in dsc], VW.K, pose, VW.W_IMG, VW.H_IMG,
                                 info["point"], info["inlier"], window=0, frustum=dict(kf_oct=octv, kf_P=P))
            assert cnt == want and np.array_equal(_life(m)[0], life)
            assert not np.isin(ids[info["point"][info["point"] >= 0]], wrong).any()   # never found again
        kp, d = PW.empty_keyframe(j)
        m.add_keyframe(img, kp, d, Tk)
        assert m.last["n_new"] == 0 and len(m.map_points) == len(ids)   # (the keyframe's own cull keeps all of them, the wrong ones too)
        a = _snap(m)
        r = PR.decide(life, now + 1 + j, a["obs_off"], a["obs_kf"], a["obs_kp"], [kf._rows for kf in m.keyframes])
        removed, info = m.cull_map_points()
        _equals(removed, info, r)
        gone += ids[removed].tolist()
        _, life, _ = PR.erase(a, life, r["removed"])
        ids = ids[~r["removed"]]
        assert np.array_equal(_life(m)[0], life)
    assert sorted(gone) == wrong and len(m.map_points) == n - PW.N_WRONG
    assert (4 * life[:, 1] >= life[:, 0]).all() and life[:, 0].max() >= 8
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


# ---- 6. empty maps and argument errors -----------------------------------------------------------------------------------------------------
def test_empty_maps():
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    m = LocalMapper(PW.BASE_K, save_every_keyframe=False, context=ctx)
    for erase in (False, True):
        removed, info = m.cull_map_points(erase=erase)
        assert removed == [] and info["n_removed"] == 0 and info["n_tested"] == 0 and info["now"] == 0 and len(info["reason"]) == 0
    assert len(m.erase_map_points([])) == 0
    assert m.note_tracking(np.eye(4), {"point": [3, -1], "inlier": [1, 0]}) == dict(n_local=0, n_seen=0, n_matched=0, n_found=0)
    p = m.point_life()
    assert p["now"] == 0 and len(p["visible"]) == 0
    # points without keyframes: nothing is noted, every point is an orphan
    m.update_map_points([{"id": i, "position": np.array([0.0, 0.0, 5.0]), "observed_keyframes": {0: i}} for i in range(3)])
    assert m.note_tracking(np.eye(4), {"point": [0, 1], "inlier": [1, 1]}, window=0) == dict(n_local=0, n_seen=0, n_matched=0, n_found=0)
    assert _life(m)[0].tolist() == [[1, 1, 0]] * 3
    removed, info = m.cull_map_points(erase=False)
    assert removed == [0, 1, 2] and info["n_reason"] == [0, 0, 0, 3] and info["n_tested"] == 3
    assert m.cull_map_points(erase=False, orphan_obs=-1)[0] == []
    removed, info = m.cull_map_points()
    assert removed == [0, 1, 2] and len(m.map_points) == 0 and info["n_points"] == 0 and info["n_obs"] == 0 and info["remap"].tolist() == [-1] * 3
    assert len(m.arrays()["obs_kf"]) == 0 and m.arrays()["obs_off"].tolist() == [0]
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_errors_leave_the_map_unchanged():
    import vslam_amd as V
    ctx = _ctx()
    w = PW.case("duplicate_position")
    m = PW.build(ctx, w)
    before, life = _snap(m), _life(m)[0]
    out, nout, eout = V.MapPtCullOut(), V.MapNoteOut(), V.MapPtEraseOut()

    def prm(ratio=0.25, min_age=2):
        return V.MapPtCullParams(ratio, min_age, 3, 2, 1, None, 1)
    for fn in (m.lib.mo_map_cull_points, m.lib.mo_map_points_bad):
        for p in (prm(ratio=float("nan")), prm(ratio=float("inf")), prm(min_age=-1)):
            assert fn(m._h, C.byref(p), C.byref(out)) == V.MO_ERR_ARG
        assert fn(m._h, None, C.byref(out)) == V.MO_ERR_ARG and fn(m._h, C.byref(prm()), None) == V.MO_ERR_ARG
        assert fn(None, C.byref(prm()), C.byref(out)) == V.MO_ERR_ARG
    K = np.ascontiguousarray(PW.BASE_K, np.float64).reshape(9)
    pose = np.ascontiguousarray(np.eye(4)[:3], np.float64).reshape(12)
    pt, inl = np.zeros(4, np.int32), np.ones(4, np.uint8)

    def note(K=K, pose=pose, n=4, pt=pt, inl=inl, out=nout, handle=m._h, **kw):
        f = dict(w=640, h=480, window=10, scale_factor=1.2, local_mask=None, frustum=None)
        f.update(kw)
        p = V.MapNoteParams(f["w"], f["h"], f["window"], f["scale_factor"], f["local_mask"], f["frustum"])
        return m.lib.mo_map_note_tracking(handle, V._ptr(K) if K is not None else None, V._ptr(pose) if pose is not None else None, C.byref(p), n,
                                          V._ptr(pt) if pt is not None else None, V._ptr(inl) if inl is not None else None,
                                          C.byref(out) if out is not None else None)
    bad_K, bad_pose = K.copy(), pose.copy()
    bad_K[4] = np.nan; bad_pose[11] = np.inf
    bad_fr = V.MapFrustumParams(0, 0.8, 1.2, 0.5)
    for kw in (dict(K=None), dict(pose=None), dict(pt=None), dict(inl=None), dict(out=None), dict(K=bad_K), dict(pose=bad_pose), dict(n=-1), dict(w=0),
               dict(h=-3), dict(window=-1), dict(scale_factor=0.0), dict(scale_factor=float("nan")), dict(frustum=C.addressof(bad_fr)), dict(handle=None)):
        assert note(**kw) == V.MO_ERR_ARG, kw
    assert m.lib.mo_map_note_tracking(m._h, V._ptr(K), V._ptr(pose), None, 0, None, None, C.byref(nout)) == V.MO_ERR_ARG
    assert m.lib.mo_map_erase_points(m._h, None, None, C.byref(eout)) == V.MO_ERR_ARG
    assert m.lib.mo_map_erase_points(m._h, V._ptr(np.zeros(len(w.ids), np.uint8)), None, None) == V.MO_ERR_ARG
    assert m.lib.mo_map_erase_points(None, None, None, C.byref(eout)) == V.MO_ERR_ARG
    assert m.lib.mo_map_point_life(m._h, None, None) == V.MO_ERR_ARG and m.lib.mo_map_point_life(None, None, None) == V.MO_ERR_ARG
    with pytest.raises(ValueError):
        m.cull_map_points(protect=[0, 1])
    with pytest.raises(ValueError):
        m.erase_map_points(np.zeros(3, bool))
    with pytest.raises(IndexError):
        m.erase_map_points([len(w.ids)])
    _same_bytes(before, _snap(m))
    assert np.array_equal(_life(m)[0], life)
    _equals(*m.cull_map_points(erase=False), PW.decide(w))   # and the map still answers
    none = np.zeros(len(w.counts), np.uint8)
    assert note(n=0, pt=None, inl=None, local_mask=none.ctypes.data) == V.MO_OK and np.array_equal(_life(m)[0], life)   # (no keypoints, no local keyframe)
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


# ---- 8. poison -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x5A])
def test_no_result_depends_on_stale_scratch(byte):
    """every scratch buffer filled with `byte` in front of each call: the notes, the decision and the erase are what they were"""
    from tests import view_worlds as VW
    ctx = _ctx()
    w = PW.case("large")
    m = PW.build(ctx, w)
    r = PW.decide(w)
    _equals(*m.cull_map_points(erase=False), r)   # (the feature's buffers exist)
    c = VW.track_case("track")
    v = c["w"].build(ctx)
    ok, _, info = v.track_local_map(c["kps"], c["desc"], c["pose0"], radii=(15.0,), window=5, frustum=True)
    a, P, _, octv, dsc = map_inputs(v)
    life0 = _life(v)[0]
    want_life, want_cnt = PR.note(life0, a["xyz"], a["obs_off"], a["obs_kf"], a["obs_kp"], [len(d) for d in dsc], VW.K, c["pose0"], VW.W_IMG, VW.H_IMG,
                                  info["point"], info["inlier"], window=5, frustum=dict(kf_oct=octv, kf_P=P))
    v.note_tracking(c["pose0"], {"point": [], "inlier": []}, local_keyframes=[])   # (the feature's buffers exist; nothing is noted)
    ctx._check(ctx.lib.mo_dbg_set_poison(ctx.h, byte))
    try:
        assert v.note_tracking(c["pose0"], info, window=5, frustum=True) == want_cnt
        assert np.array_equal(_life(v)[0], want_life)
        _equals(*m.cull_map_points(erase=False), r)
        removed, cinfo = m.cull_map_points()
        _equals(removed, cinfo, r)
        want, life, remap = PR.erase(w.arrays(), w.life, r["removed"])
        got = _snap(m)
        for f in want:
            assert got[f].tobytes() == want[f].tobytes(), f
        assert np.array_equal(cinfo["remap"], remap) and np.array_equal(_life(m)[0], life)
    finally:
        ctx._check(ctx.lib.mo_dbg_set_poison(ctx.h, -1))
    assert ctx.dev_status() == 0
    m.close(); v.close(); ctx.close()
