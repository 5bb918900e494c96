"""What the context's buffer owners guard: every growth and rebuild path of a context walked once, the context destroyed, and all of
it again in the same process.  The second pass equals the first bit for bit and no call leaves an error behind: nothing is freed twice
or too early, nothing a rebuilt plan dropped is read afterwards, and a refused call leaves the context as it was."""
import numpy as np
import pytest

import vslam_amd as V
from vslam_amd.stream import FrameStream
from tests.helpers import synthetic_frame

pytestmark = pytest.mark.gpu

W, H = 96, 80   # (at the default edge_threshold of 31 levels 0 and 1 hold keypoints; level 2, 67 x 56, has no border region: a level
                #  without strips is part of every plan here)
K = np.array([[90.0, 0, W / 2], [0, 90.0, H / 2], [0, 0, 1.0]])


@pytest.fixture(scope="module")
def frames():
    """smooth-textured frames from fixed seeds: eight of 96 x 80 (consecutive ones a two-pixel pan of one wide frame, so that pairs
    match) and one of 160 x 120"""
    wide = synthetic_frame(20251017, W + 16, H)
    small = np.stack([np.ascontiguousarray(wide[:, 2 * i:2 * i + W]) for i in range(8)])
    return small, synthetic_frame(20251018, 160, 120)


def _bytes_of(x):
    """every array and number below x, in order, as bytes"""
    if isinstance(x, dict):
        return [(k, _bytes_of(v)) for k, v in sorted(x.items())]
    if isinstance(x, (list, tuple)):
        return [_bytes_of(v) for v in x]
    return None if x is None else np.asarray(x).tobytes()


def _clean(ctx):
    assert ctx.lib.mo_last_error(ctx.h).decode() == ""
    assert ctx.dev_status() == 0


def _lifetime_pass(small, large):
    ctx = V.Context(max_w=256, max_h=256, max_batch=4)
    prm = V.orb_params(nfeatures=100, nlevels=3)
    out = {}
    out["first_plan"] = ctx.orb_detect_compute(small[0], prm)           # the first plan
    out["other_size"] = ctx.orb_detect_compute(large, prm)              # rebuilt for another size
    out["batch"] = ctx.orb_detect_compute(small[:4], prm)               # rebuilt for a larger batch; the output staging grows
    assert all(len(k) > 0 for k, _ in out["first_plan"] + out["other_size"] + out["batch"])
    out["grid"] = ctx.grid_detect_compute(small[1], prm, 128)
    rng = np.random.default_rng(5)
    d = rng.integers(0, 256, (400, 32), dtype=np.uint8)
    out["match50"] = ctx.match_knn2_ratio(d[:50], d[25:75], 0.75)
    out["match400"] = ctx.match_knn2_ratio(d, d[::-1], 0.75)            # the matcher staging grows
    (k0, d0), = ctx.orb_detect_compute(small[0], prm)
    (k1, d1), = ctx.orb_detect_compute(small[1], prm)
    t0, t1 = V.resident_token(ctx, d0, k0), V.resident_token(ctx, d1, k1)
    assert t0 and t1
    pair = ctx.pair_frontend(k0, d0, k1, d1, V.MODE_INIT, K, n_hyp=64)
    assert (pair["token1"], pair["token2"]) == (t0, t1)                 # both frames were resident: nothing uploaded
    out["pair_resident"] = pair
    out["more_features"] = ctx.orb_detect_compute(small[2], V.orb_params(nfeatures=600, nlevels=3))   # 1624 rows per slot: the slot arrays grow
    again = ctx.pair_frontend(k0, d0, k1, d1, V.MODE_INIT, K, n_hyp=64)
    assert again["token1"] not in (0, t0) and again["token2"] not in (0, t1)   # the tokens died with the old arrays: uploaded again
    for name in ("idx", "dist", "keep"):
        assert np.array_equal(again[name], pair[name])
    out["pair_uploaded"] = again
    resp = rng.integers(0, 40, 300).astype(np.float32)                  # (few distinct values: ties at the boundary)
    out["retain"] = ctx.dbg_retain_best(resp, 120, V.ORDER_LIBSTDCXX)
    assert len(out["retain"]) >= 120
    _clean(ctx)
    ctx.close()

    fs = FrameStream(K, width=W, height=H, chunk=4, prm=prm, n_hyp=64)
    out["stream"] = [(r.keypoints, r.descriptors) + (() if r.pair is None else (r.pair.sel, r.pair.sel_dist, r.pair.R, r.pair.t, r.pair.n_inliers))
                     for r in fs.run(small)]
    assert [len(x) for x in out["stream"]] == [2] + [7] * 7
    _clean(fs.ctx)
    fs.close()
    return _bytes_of(out)


def test_context_lifetime_twice_in_one_process(frames):
    small, large = frames
    first = _lifetime_pass(small, large)
    second = _lifetime_pass(small, large)
    assert first == second


def test_refused_calls_leave_the_context_usable(frames):
    small, _ = frames
    ctx = V.Context(max_w=128, max_h=128, max_batch=2)
    prm = V.orb_params(nfeatures=100, nlevels=3)
    before = _bytes_of(ctx.orb_detect_compute(small[0], prm))
    last_error = lambda: ctx.lib.mo_last_error(ctx.h).decode()
    assert last_error() == ""
    with pytest.raises(V.NativeError, match="max_w/max_h"):
        ctx.orb_detect_compute(synthetic_frame(3, 160, 120), prm)       # wider than max_w
    refused = last_error()
    assert _bytes_of(ctx.orb_detect_compute(small[0], prm)) == before
    assert last_error() == refused                                      # (a message stays until the next failure: the valid call added none)
    with pytest.raises(V.NativeError, match="max_batch"):
        ctx.orb_detect_compute(small[:3], prm)                          # more frames than max_batch
    refused = last_error()
    assert "max_batch" in refused
    assert _bytes_of(ctx.orb_detect_compute(small[0], prm)) == before
    assert last_error() == refused
    assert ctx.dev_status() == 0
    ctx.close()


def _reloc_last(m):
    """(rc, everything mo_dbg_map_reloc_last wrote)"""
    import ctypes as C
    n = C.c_int32(-7)
    cand, ncorr, ninl = (np.full(64, -7, np.int32) for _ in range(3))
    best = np.full(64, 7, np.uint64)
    pose = np.full((64, 12), 7.0)
    rc = m.lib.mo_dbg_map_reloc_last(m._h, C.byref(n), V._ptr(cand), V._ptr(best), V._ptr(ncorr), V._ptr(ninl), V._ptr(pose))
    return rc, _bytes_of([n.value, cand, best, ncorr, ninl, pose])


def test_map_features_live_and_die_with_their_map(frames):
    """every feature has run on one map; the vocabulary is replaced and the query answers against the new one; the last relocalization
    stays readable; the map goes, and the context extracts what it extracted before the map existed; a map that has run nothing has no
    relocalization to report"""
    from tests import bow_restatement as B
    from tests import loop_worlds as LW
    from tests.map_worlds import kps_array
    small, _ = frames
    ctx = V.Context(max_w=128, max_h=128, max_batch=1)
    prm = V.orb_params(nfeatures=100, nlevels=3)
    before = _bytes_of(ctx.orb_detect_compute(small[0], prm))
    w = LW.feature_world()
    m = w.build(ctx)
    voc = V.Vocabulary.from_arrays(w.words, w.weights, context=ctx)
    for name, fn in LW.feature_steps(m, w, voc):
        fn()
    rc, last = _reloc_last(m)
    assert rc == V.MO_OK
    # another vocabulary: the words in reverse order, the weights 1, 2, 3, ...
    words2 = np.ascontiguousarray(w.words[::-1])
    weights2 = np.arange(1, len(words2) + 1, dtype=np.int32)
    voc2 = V.Vocabulary.from_arrays(words2, weights2, context=ctx)
    m.set_vocabulary(voc2)
    kps, desc = kps_array(w.kf_xy[1]), w.kf_desc[1]
    pos, score = m.query_keyframes(kps, desc, 4)
    want_pos, want_score = B.query(desc, w.kf_desc, words2, weights2, 4)
    assert len(pos) > 0 and pos.tolist() == list(want_pos) and np.array_equal(score, np.asarray(want_score, np.float64))
    assert _reloc_last(m) == (V.MO_OK, last)
    _clean(ctx)
    m.close()
    assert _bytes_of(ctx.orb_detect_compute(small[0], prm)) == before
    m2 = LW.new_mapper(ctx, w.K, (8, 16, 16, 32))
    assert _reloc_last(m2)[0] == V.MO_ERR_ARG
    m2.close(); voc.close(); voc2.close()
    ctx.close()
