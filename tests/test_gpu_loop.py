"""mo_map_loop_candidates on the device against its numpy restatement (tests/loop_restatement.py) on every world of
tests/loop_worlds.py: positions, counts, flags and correspondences equal as lists, the f64 values equal with ==.  The restatement is fed
from the map as downloaded, so whatever a growth step did is in both."""
import numpy as np
import pytest

from tests import loop_restatement as LR
from tests import loop_worlds as LW
from tests.map_worlds import kps_array, remove_keyframes

pytestmark = pytest.mark.gpu

STAGES = ["bow_quantise", "bow_hist", "covis", "loop_score", "loop_select", "loop_match", "loop_gather"]


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _voc(ctx, words, weights):
    import vslam_amd as V
    return V.Vocabulary.from_arrays(words, weights, context=ctx)


def _prepared(m, kf_desc, words):
    a = m.arrays()
    return a, LR.prepared(kf_desc, a["obs_off"], a["obs_kf"], a["obs_kp"], words)


def _equals_restatement(m, kf_desc, words, weights, p, prep=None, min_weight=15, n_best=10, max_cand=4, ratio=0.75):
    a, (kc, W, tab) = prep if prep is not None else _prepared(m, kf_desc, words)
    r = LR.loop_candidates(kf_desc, a["obs_off"], a["obs_kf"], a["obs_kp"], words, weights, p, min_weight, n_best, max_cand, ratio, kc, W, tab)
    d = m.loop_candidates(p, min_weight, n_best, max_cand, ratio)
    c = d["candidates"]
    assert [x["pos"] for x in c] == r["cand"], (p, [x["pos"] for x in c], r["cand"])
    assert (d["n_found"], d["n_connected"], d["max_common"], d["n_scored"], d["n_passed"]) == \
        (r["n_found"], r["n_connected"], r["max_common"], r["n_scored"], r["n_passed"]), (p, d, r)
    assert d["connected"] == r["connected"] and [x["group"] for x in c] == r["group"]
    assert d["min_score"] == r["min_score"]                                        # == on the f64 values
    assert [x["acc"] for x in c] == r["acc"] and [x["score"] for x in c] == r["score"], (p, [x["acc"] for x in c], r["acc"])
    assert [x["n_match"] for x in c] == r["n_match"]
    assert d["cur_point"].tolist() == r["cur_point"].tolist()                      # (with or without a candidate)
    for x, mp, mr in zip(c, r["match_point"], r["match_row"]):
        assert x["cur_point"].tolist() == r["cur_point"].tolist()
        assert x["match_point"].tolist() == mp.tolist() and x["match_row"].tolist() == mr.tolist()
    return d, r


def _same(a, b):
    assert {k: v for k, v in a.items() if k not in ("candidates", "cur_point")} == {k: v for k, v in b.items() if k not in ("candidates", "cur_point")}
    assert np.array_equal(a["cur_point"], b["cur_point"])
    assert len(a["candidates"]) == len(b["candidates"])
    for x, y in zip(a["candidates"], b["candidates"]):
        assert all(np.array_equal(x[k], y[k]) for k in x)


def test_loop_world():
    import vslam_amd as V
    ctx = _ctx()
    w = LW.loop_world()
    words, weights = LW.loop_vocabulary()
    m = w.build(ctx)
    with pytest.raises(V.NativeError) as e:
        m.loop_candidates()                                                       # no vocabulary attached
    assert e.value.code == V.MO_ERR_ARG
    m.set_vocabulary(_voc(ctx, words, weights))                                   # attached after the keyframes
    before = {f: x.copy() for f, x in m.arrays().items()}
    prep = _prepared(m, w.kf_desc, words)
    res = {p: _equals_restatement(m, w.kf_desc, words, weights, p, prep) for p in (19,) + LW.RETURN_POS}
    assert res[19][0]["candidates"] == [] and res[19][0]["n_scored"] > 0 and res[19][0]["n_passed"] == 0
    assert all(x["pos"] in range(0, 6) for p in LW.RETURN_POS for x in res[p][0]["candidates"])
    _equals_restatement(m, w.kf_desc, words, weights, -1, prep)                   # the last keyframe, a filler: nothing in common
    # the same call twice; a query and a tracking call in between (they share the spare database row and the resident W)
    first = m.loop_candidates(26)
    _same(first, m.loop_candidates(26))
    kps, qd = kps_array(w.kf_xy[3]), w.kf_desc[3]
    m.query_keyframes(kps, qd, 5)
    _same(first, m.loop_candidates(26))
    m.track_local_map(kps, qd, w.kf_poses[3], local="covisible")
    _same(first, m.loop_candidates(26))
    ctx.set_host_timing(True)
    m.loop_candidates(26)
    assert [n for n, _ in ctx.stage_times()] == STAGES
    ctx.set_host_timing(False)
    # detect_loop at its default threshold of 3 on the finished map: the four return keyframes in turn, detection at the fourth alone
    found = {}
    for p in LW.RETURN_POS:
        found[p], info = m.detect_loop(p)
        assert [x["pos"] for x in info["candidates"]] == res[p][1]["cand"]
    assert [p for p in LW.RETURN_POS if found[p]] == [26], found
    acc = info["accepted"]
    assert acc["consistency"] == 3 and acc["n_match"] >= 20 and acc["pos"] in range(0, 6)
    m._cache = None
    assert all(np.array_equal(before[f], x) for f, x in m.arrays().items())       # the map is read, not changed
    m.close(); ctx.close()


@pytest.mark.parametrize("n_kf", sorted(LW.TINY))
def test_tiny_maps(n_kf):
    ctx = _ctx()
    w = LW.tiny_world(n_kf)
    m = w.build(ctx)
    m.set_vocabulary(_voc(ctx, w.words, w.weights))
    prep = _prepared(m, w.kf_desc, w.words)
    n_cand = 0
    for p in w.asking():
        for n_best, max_cand in ((10, 4), (2, 16), (0, 1)):
            d, _ = _equals_restatement(m, w.kf_desc, w.words, w.weights, p, prep, LW.TINY_MIN_WEIGHT, n_best, max_cand)
            n_cand += len(d["candidates"])
    assert n_cand > 0
    if n_kf == 70:
        # keyframes removed (position != slot): equal to the restatement on the survivors, the stored observation keys read as they are
        gone = [3, 20, 41]
        remove_keyframes(m, gone)
        kept = [d for k, d in enumerate(w.kf_desc) if k not in gone]
        m._cache = None
        for p in (-1, 0, 30):
            _equals_restatement(m, kept, w.words, w.weights, p, None, LW.TINY_MIN_WEIGHT, 10, 4)
    m.close(); ctx.close()


def test_hand_cases():
    ctx = _ctx()
    for i, (name, (w, kw)) in enumerate(LW.hand_cases().items()):
        v = _voc(ctx, w.words, w.weights)
        m = w.build(ctx, vocabulary=v if i % 2 else None)                        # attached before the keyframes, or after them
        m.set_vocabulary(v)
        _equals_restatement(m, w.kf_desc, w.words, w.weights, -1, None, **kw)
        m.close()
    ctx.close()


def test_errors_and_empty_map():
    import ctypes as C
    import vslam_amd as V
    ctx = _ctx()
    w, kw = LW.hand_cases()["groups"]
    v = _voc(ctx, w.words, w.weights)
    m = w.build(ctx, vocabulary=v)
    for bad in (dict(kf_position=5), dict(kf_position=-2), dict(n_best=-1), dict(max_candidates=17), dict(max_candidates=-1), dict(ratio=0.0),
                dict(ratio=1.5), dict(ratio=float("nan"))):
        with pytest.raises(V.NativeError) as e:
            m.loop_candidates(**bad)
        assert e.value.code == V.MO_ERR_ARG, bad
    assert m.lib.mo_map_loop_candidates(m._h, None, None) == V.MO_ERR_ARG
    assert m.loop_candidates(ratio=1.0, min_weight=1)["n_found"] == 1             # the bounds that are legal
    prm, out = V.MapLoopParams(-1, 1, 10, 4, 0.75), V.MapLoopOut()               # every output array NULL
    assert m.lib.mo_map_loop_candidates(m._h, C.byref(prm), C.byref(out)) == V.MO_OK and out.n_found == 1 and out.n_cand == 1
    empty = LW.new_mapper(ctx, w.K, (8, 16, 64, 256), v)
    r = empty.loop_candidates()
    assert r["candidates"] == [] and r["connected"] == [] and r["min_score"] == 1.0
    assert (r["n_found"], r["n_connected"], r["max_common"], r["n_scored"], r["n_passed"]) == (0, 0, 0, 0, 0)
    with pytest.raises(V.NativeError):
        empty.loop_candidates(kf_position=0)
    m.close(); empty.close(); ctx.close()


def test_detect_loop_while_the_map_is_built():
    """keyframe by keyframe (tests/loop_worlds.LoopWorld.steps): the device equals the restatement on the map as it stands behind every
    return keyframe; the first of them has no connected keyframe yet and so no candidate, the chain of consistent groups starts at
    keyframe 22 and a consistency of 2 is reached at keyframe 26, and only there"""
    ctx = _ctx()
    w = LW.loop_world()
    words, weights = LW.loop_vocabulary()
    m = LW.new_mapper(ctx, w.K, (32, 512, 4096, 16384), _voc(ctx, words, weights))
    found = {}
    for add, inject, ask in w.steps():
        for k in add:
            LW.add_keyframe(m, w, k)
        m.update_map_points(inject)
        _equals_restatement(m, w.kf_desc[:len(m.keyframes)], words, weights, ask)
        found[ask], info = m.detect_loop(ask, consistency=2)
        if ask != 26:
            assert info["accepted"] is None
    assert [p for p in found if found[p]] == [26], found
    acc = info["accepted"]
    assert acc["pos"] in range(0, 6) and acc["consistent"] and acc["n_match"] >= 20 and acc["serial"] == acc["pos"]
    rows = np.flatnonzero(acc["match_point"] >= 0)
    ids = m.arrays()["id"].astype(np.int64)
    assert len(rows) == acc["n_match"] and (ids[acc["cur_point"][rows]] - LW.DUP_ID == ids[acc["match_point"][rows]]).all()
    m.close(); ctx.close()
