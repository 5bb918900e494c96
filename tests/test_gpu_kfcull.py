"""The keyframe cull by ORB-SLAM2's rule on the device map (mo_map_kf_redundancy, mo_map_erase_keyframes, mo_map_cull_keyframes; LocalMapper's
cull_keyframes / erase_keyframes): the decision equals tests/kfcull_restatement.py integer for integer on every world of
tests/kfcull_worlds.py and on the existing worlds of tests/map_worlds.py, whichever way the candidates are walked; the erase leaves the
restated arrays byte for byte, and the map then behaves like the twin that never had the keyframes.  tests/test_kfcull_cpu.py shows what
each world is there to exclude."""
import ctypes as C

import numpy as np
import pytest

from tests import kfcull_restatement as KR
from tests import kfcull_worlds as KW
from tests.covis_restatement import covisibility as covis_restated
from tests.map_worlds import BA_STEPS, BA_WINDOW, build_map, kps_array, perturbed, perturbed_pose, pose_near, world

pytestmark = pytest.mark.gpu

OBS = ("obs_off", "obs_kf", "obs_kp")
POINTS = ("xyz", "color", "id", "dref_kf", "dref_row")


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _snap(m):
    m._cache = None
    return {k: v.copy() for k, v in m.arrays().items()}


def _same_bytes(a, b, fields=None):
    for f in fields or a:
        assert a[f].dtype == b[f].dtype and a[f].tobytes() == b[f].tobytes(), f


def _call_kw(kw):
    kw = dict(kw)
    if "kf_pos" in kw:
        kw["kf_position"] = kw.pop("kf_pos")
    return kw


def _equals(removed, info, r):
    for k in ("pos", "weight", "n_points", "n_redundant"):
        assert info[k].tolist() == r[k], (k, info[k].tolist(), r[k])
    assert info["removed"].tolist() == r["removed"] and removed == r["removed_positions"]
    assert info["n_local"] == len(r["pos"]) and info["n_removed"] == len(removed)


def _other(ctx):
    """a map of another size, culled once: what the next call on the first map must not see"""
    w, kw = KW.case("mutual")
    m = build_map(ctx, w)
    _equals(*m.cull_keyframes(erase=False, **_call_kw(kw)), KW.decide(w, **kw))
    return m


@pytest.mark.parametrize("name", KW.ALL)
def test_decision_equals_the_restatement(name):
    ctx = _ctx()
    w, kw = KW.any_world(name)
    m = build_map(ctx, w)
    before = _snap(m)
    r = KW.decide(w, **kw)
    for walk in (1, 2, 0, 1):   # one workgroup, a launch per candidate, the library's choice, and the first again
        _equals(*m.cull_keyframes(erase=False, walk=walk, **_call_kw(kw)), r)
    other = _other(ctx)
    for walk in (2, 1):
        _equals(*m.cull_keyframes(erase=False, walk=walk, **_call_kw(kw)), r)
    _same_bytes(before, _snap(m))
    assert len(m.keyframes) == len(w.counts)
    assert ctx.dev_status() == 0
    other.close(); m.close(); ctx.close()


def test_empty_maps():
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    m = LocalMapper(KW.BASE_K, save_every_keyframe=False, context=ctx)
    for erase in (False, True):
        removed, info = m.cull_keyframes(erase=erase)
        assert removed == [] and info["n_local"] == 0 and info["n_removed"] == 0 and len(info["pos"]) == 0
    out = V.MapKfCullOut()
    assert m.lib.mo_map_kf_redundancy(m._h, C.byref(V.MapKfCullParams(7, 15, 3, 1, 0.9, None, 0, 0)), C.byref(out)) == V.MO_OK   # (no keyframes: kf_pos is not looked at)
    m.erase_keyframes([])
    m.close()
    for name in ("one_keyframe", "no_points"):
        w, kw = KW.case(name)
        m = build_map(ctx, w)
        for erase in (False, True):
            removed, info = m.cull_keyframes(erase=erase)
            assert removed == [] and info["n_local"] == 0 and info["n_removed"] == 0 and len(m.keyframes) == len(w.counts)
        m.close()
    # keyframes without points can still be erased: the position table alone
    w, _ = KW.case("no_points")
    m = build_map(ctx, w)
    m.erase_keyframes([1, 1, 2])
    assert len(m.keyframes) == 2 and [kf["id"] for kf in m.keyframes] == [0, 1] and m.covisibility().shape == (2, 2)
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def _twin(ctx, w, poses, xyz, gone):
    """the map that never had the keyframes at `gone`: the surviving keyframes in order, the restated erased observations"""
    from vslam_amd.mapper import LocalMapper
    off, okf, okp, counts = KR.erase(w.obs_off, w.obs_kf, w.obs_kp, w.counts, gone)
    m = LocalMapper(w.K, save_every_keyframe=False, context=ctx)
    img = np.zeros((w.image_size[1], w.image_size[0]), np.uint8)
    for q in range(len(w.counts)):
        if q in gone:
            continue
        m.add_keyframe(img, kps_array(w.kf_xy[q], w.kf_oct[q]), w.kf_desc[q], np.asarray(poses[q], np.float64))
        assert m.last["n_new"] == 0 and len(m.map_points) == 0
    dicts = []
    for i in range(len(off) - 1):
        o = dict(zip(okf[off[i]:off[i + 1]].tolist(), okp[off[i]:off[i + 1]].tolist()))
        assert len(o) == off[i + 1] - off[i]
        dicts.append({"id": int(w.ids[i]), "position": xyz[i], "color": np.zeros(3, np.uint8), "observed_keyframes": o})
    m.update_map_points(dicts)
    return m, (off, okf, okp, counts)


@pytest.mark.parametrize("how", ["erase", "cull"])
def test_erased_map_equals_its_twin(how):
    """the consecutive-keyframe world (positions 1 and 5 removed earlier: position != slot), keyframes 2 and 6 erased - by erase_keyframes,
    or by a cull that protects everything else at a ratio every candidate passes.  Observation arrays equal to the restatement, point
    arrays untouched, covisibility, tracking, bundle adjustment and place recognition as on the twin."""
    from tests.test_gpu_map_reads import _same_track
    ctx = _ctx()
    w = world("ba")
    n_kf = len(w.counts)
    gone = [2, 6]
    poses, xyz = perturbed(w, first_free=4)
    m = build_map(ctx, w, poses=poses, xyz=xyz)
    voc = m.train_vocabulary(64, 5)
    T = pose_near(w, 7)
    kps, desc = w.track_query(T, octave_spread=1)
    m.query_keyframes(kps, desc, 5)   # (the keyframe database exists before the erase)
    before = _snap(m)
    if how == "erase":
        m.erase_keyframes(gone)
    else:
        protect = np.ones(n_kf, np.uint8); protect[gone] = 0
        removed, info = m.cull_keyframes(kf_position=4, min_weight=1, ratio=-1.0, protect=protect)   # (4 shares points with both)
        r = KW.decide(w, kf_pos=4, min_weight=1, ratio=-1.0, protect=protect)
        _equals(removed, info, r)
        assert removed == gone
    twin, (off, okf, okp, counts) = _twin(ctx, w, poses, xyz, gone)
    after = _snap(m)
    for f, want in zip(OBS, (off, okf, okp)):
        assert after[f].dtype == want.dtype and after[f].tobytes() == want.tobytes(), f
    _same_bytes(before, after, POINTS)
    _same_bytes(after, _snap(twin))
    assert len(okf) < len(w.obs_kf) and (np.diff(off) <= 1).any()           # points left with one observation or none stay
    assert len(m.keyframes) == n_kf - 2 == len(twin.keyframes)
    W = covis_restated(off, okf, okp, counts)
    assert np.array_equal(m.covisibility(), W) and np.array_equal(twin.covisibility(), W)
    pose0 = perturbed_pose(T)
    a, b = m.track_local_map(kps, desc, pose0), twin.track_local_map(kps, desc, pose0)
    assert a[2]["n_local"] > 0 and a[2]["pass_matches"][0] >= 20
    _same_track(a, b)
    twin.set_vocabulary(voc)
    (pa, sa), (pb, sb) = m.query_keyframes(kps, desc, 5), twin.query_keyframes(kps, desc, 5)
    assert len(pa) and pa.tolist() == pb.tolist() and sa.tobytes() == sb.tobytes()
    oka, ia = m.bundle_adjust(window=BA_WINDOW, max_steps=BA_STEPS, want_points=True)
    okb, ib = twin.bundle_adjust(window=BA_WINDOW, max_steps=BA_STEPS, want_points=True)
    assert oka == okb and ia["n_edges"] > 0
    for k in ia:
        assert np.array_equal(np.asarray(ia[k]), np.asarray(ib[k]), equal_nan=True), k
    _same_bytes(_snap(m), _snap(twin))
    assert ctx.dev_status() == 0
    m.close(); twin.close(); ctx.close()


@pytest.mark.parametrize("name", ["plain", "mutual", "negative_keys", "earlier_removals", "tall", "many", "ba_stale"])
def test_cull_erases_what_it_decides_and_culls_again(name):
    ctx = _ctx()
    w, kw = KW.any_world(name)
    m = build_map(ctx, w)
    before = _snap(m)
    # (tests.map_worlds.remove_keyframes, which built the worlds with earlier removals, leaves the serials of the removed keyframes in)
    m._kf_serials = [s for q, s in enumerate(m._kf_serials) if q not in getattr(w, "removed", ())]
    serials = list(m._kf_serials)
    assert len(serials) == len(m.keyframes)
    r = KW.decide(w, **kw)
    removed, info = m.cull_keyframes(**_call_kw(kw))
    _equals(removed, info, r)
    after = _snap(m)
    _same_bytes(before, after, POINTS)
    if removed:
        off, okf, okp, counts = KR.erase(w.obs_off, w.obs_kf, w.obs_kp, w.counts, removed)
        for f, want in zip(OBS, (off, okf, okp)):
            assert after[f].tobytes() == want.tobytes(), f
    else:   # nothing removed: the map keeps its bytes, stale keys included
        off, okf, okp, counts = w.obs_off, w.obs_kf, w.obs_kp, w.counts
        _same_bytes(before, after)
    assert info["n_obs"] == len(okf)
    keep = [q for q in range(len(w.counts)) if q not in removed]
    assert [kf["id"] for kf in m.keyframes] == list(range(len(keep))) and m._kf_serials == [serials[q] for q in keep]
    assert np.array_equal(m.covisibility(), covis_restated(off, okf, okp, counts))
    # the second cull, on the erased map: asked from where the same keyframe now stands
    kw2 = dict(kw)
    p = kw.get("kf_pos", -1)
    if p >= 0:
        kw2["kf_pos"] = keep.index(p)
    if "protect" in kw2:
        kw2["protect"] = [kw["protect"][q] for q in keep]
    oct2 = [w.kf_oct[q] for q in keep]
    r2 = KR.decide(off, okf, okp, counts, oct2, **kw2)
    removed2, info2 = m.cull_keyframes(**_call_kw(kw2))
    _equals(removed2, info2, r2)
    if removed2:
        o2 = KR.erase(off, okf, okp, counts, removed2)
        a2 = _snap(m)
        for f, want in zip(OBS, o2[:3]):
            assert a2[f].tobytes() == want.tobytes(), f
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_host_bookkeeping_and_what_follows():
    """after a cull the keyframe list, the ids, the co-visibility graph's keys and the serials agree; a tracked keyframe and a loop
    detection run on the map"""
    ctx = _ctx()
    w, kw = KW.case("plain")
    m = build_map(ctx, w)
    n_kf = len(w.counts)
    for a in range(n_kf):
        for b in range(n_kf):
            if a != b:
                m.co_visibility_graph[a][b] = 1 + a + b
    kept_dicts = [kf for q, kf in enumerate(m.keyframes) if q != 2]
    serials = [s for q, s in enumerate(m._kf_serials) if q != 2]
    version = m._version
    removed, info = m.cull_keyframes()
    assert removed == [2]
    assert all(a is b for a, b in zip(m.keyframes, kept_dicts)) and len(m.keyframes) == n_kf - 1
    assert [kf["id"] for kf in m.keyframes] == list(range(n_kf - 1)) and m._kf_serials == serials and len(m._list_rows) == n_kf - 1
    g = m.co_visibility_graph
    assert 2 not in g and all(2 not in g[a] for a in list(g)) and sorted(g) == [0, 1, 3, 4, 5]
    assert m._version > version and len(m.map_points) == len(w.obs)
    assert len(m.arrays()["obs_kf"]) == info["n_obs"] == m._n_obs
    # what follows: a keyframe with tracked observations, a loop detection
    m.train_vocabulary(32, 3)
    rng = np.random.default_rng(3)
    n = 120
    kp = kps_array(np.column_stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)]))
    d = np.repeat(rng.integers(0, 256, (n // 2, 32)).astype(np.uint8), 2, axis=0)
    pt = np.full(n, -1, np.int32); pt[:40] = np.arange(40)
    inl = np.zeros(n, bool); inl[:40:2] = True
    m.add_keyframe(np.zeros((480, 640), np.uint8), kp, d, w.kf_poses[-1], tracked=(pt, inl))
    assert len(m.keyframes) == n_kf and [kf["id"] for kf in m.keyframes] == list(range(n_kf))
    found, linfo = m.detect_loop()
    assert found in (True, False) and "candidates" in linfo
    removed, info = m.cull_keyframes(erase=False)
    a = m.arrays()
    counts = [kf._rows for kf in m.keyframes]
    octs = [np.asarray(kf["keypoints"]["octave"]) for kf in m.keyframes]
    _equals(removed, info, KR.decide(a["obs_off"], a["obs_kf"], a["obs_kp"], counts, octs))
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_errors_leave_the_map_unchanged():
    import vslam_amd as V
    ctx = _ctx()
    w, _ = KW.case("plain")
    m = build_map(ctx, w)
    n_kf = len(w.counts)
    before = _snap(m)
    out = V.MapKfCullOut()

    def prm(kf_pos=-1, min_observers=3, ratio=0.9, walk=0, erase=1):
        return V.MapKfCullParams(kf_pos, 15, min_observers, 1, ratio, None, erase, walk)
    bad = [prm(kf_pos=n_kf), prm(kf_pos=-2), prm(min_observers=0), prm(ratio=float("nan")), prm(ratio=float("inf")), prm(walk=3), prm(walk=-1)]
    for fn in (m.lib.mo_map_cull_keyframes, m.lib.mo_map_kf_redundancy):
        for p in bad:
            assert fn(m._h, C.byref(p), C.byref(out)) == V.MO_ERR_ARG
        assert fn(m._h, None, C.byref(out)) == V.MO_ERR_ARG and fn(m._h, C.byref(prm()), None) == V.MO_ERR_ARG
        assert fn(None, C.byref(prm()), C.byref(out)) == V.MO_ERR_ARG
    for pos in ([n_kf], [-1], [2, n_kf], [2, -1, 3]):
        a = np.array(pos, np.int32)
        assert m.lib.mo_map_erase_keyframes(m._h, V._ptr(a), len(a)) == V.MO_ERR_ARG
    assert m.lib.mo_map_erase_keyframes(m._h, None, 2) == V.MO_ERR_ARG and m.lib.mo_map_erase_keyframes(m._h, None, -1) == V.MO_ERR_ARG
    assert m.lib.mo_map_erase_keyframes(None, None, 0) == V.MO_ERR_ARG
    with pytest.raises(V.NativeError):
        m.erase_keyframes([n_kf])
    with pytest.raises(ValueError):
        m.cull_keyframes(protect=[0, 1])
    _same_bytes(before, _snap(m))
    assert len(m.keyframes) == n_kf and m.covisibility().shape == (n_kf, n_kf)
    _equals(*m.cull_keyframes(erase=False), KW.decide(w))   # and the map still answers
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x5A])
def test_no_result_depends_on_stale_scratch(byte):
    """every scratch buffer of the feature filled with `byte` in front of each call: the decision and the erase are what they were"""
    ctx = _ctx()
    w, kw = KW.case("many")
    m = build_map(ctx, w)
    r = KW.decide(w, **kw)
    _equals(*m.cull_keyframes(erase=False, **kw), r)   # (the feature's buffers exist)
    ctx._check(ctx.lib.mo_dbg_set_poison(ctx.h, byte))
    try:
        for walk in (1, 2):
            _equals(*m.cull_keyframes(erase=False, walk=walk, **kw), r)
        removed, info = m.cull_keyframes(**kw)
        _equals(removed, info, r)
        off, okf, okp, _ = KR.erase(w.obs_off, w.obs_kf, w.obs_kp, w.counts, removed)
        a = _snap(m)
        for f, want in zip(OBS, (off, okf, okp)):
            assert a[f].tobytes() == want.tobytes(), f
    finally:
        ctx._check(ctx.lib.mo_dbg_set_poison(ctx.h, -1))
    assert ctx.dev_status() == 0
    m.close(); ctx.close()
