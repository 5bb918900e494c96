"""Place recognition on the device (bow.hip) against its numpy restatement (tests/bow_restatement.py): trained vocabularies byte for
byte, query positions equal and scores bit-equal, and relocalization with preselection against the plain call."""
import numpy as np
import pytest

from tests import bow_restatement as B
from tests import bow_worlds as BW
from tests.covis_worlds import pan_back
from tests.map_worlds import build_map, flip, kps_array, remove_keyframes
from tests.test_bow_cpu import PAN_FIRST, PAN_WORDS, RELOC_PRE, RELOC_WORDS

pytestmark = pytest.mark.gpu

SMALL_IMG = np.zeros((32, 32), np.uint8)


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _split(desc, off):
    return [desc[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _train_equals_restatement(ctx, arrays, W, iters=10, want=None):
    import vslam_amd as V
    desc, off = BW.rows_of(arrays)
    words, weights, ran = want if want is not None else B.train(desc, off, W, iters)
    v = V.Vocabulary.train(arrays, W, iters, context=ctx)
    assert v.words.tobytes() == words.tobytes() and v.weights.tobytes() == weights.tobytes() and v.iterations == ran, (W, v.iterations, ran)
    assert len(v) == W
    return v


def test_training_hand_cases():
    import vslam_amd as V
    ctx = _ctx()
    desc, off, W = BW.hand_split()
    v = _train_equals_restatement(ctx, _split(desc, off), W)
    assert v.iterations == 2                                  # the last iteration changed nothing
    assert _train_equals_restatement(ctx, _split(desc, off), W, iters=1).iterations == 1
    _train_equals_restatement(ctx, _split(desc, off), W, iters=0)
    _train_equals_restatement(ctx, _split(desc, off), 8)      # as many words as rows
    desc, off, W = BW.hand_duplicates()
    v = _train_equals_restatement(ctx, _split(desc, off), W)
    assert np.array_equal(v.words[1], desc[2]) and np.array_equal(v.words[2], desc[5])
    with pytest.raises(V.NativeError) as e:
        V.Vocabulary.train(_split(*BW.hand_split()[:2]), 9, context=ctx)   # n < W
    assert e.value.code == V.MO_ERR_ARG
    with pytest.raises(V.NativeError):
        V.Vocabulary.train([], 2, context=ctx)                              # no image
    ctx.close()


@pytest.mark.parametrize("W", [100, PAN_WORDS])
def test_training_on_the_pan_back_rows(W, tmp_path):
    import vslam_amd as V
    ctx = _ctx()
    v = _train_equals_restatement(ctx, pan_back().kf_desc, W, want=BW.vocabulary("pan", W))
    v.save(tmp_path / "voc.npz")
    v2 = V.Vocabulary.load(tmp_path / "voc.npz", context=ctx)
    assert np.array_equal(v2.words, v.words) and np.array_equal(v2.weights, v.weights)
    with pytest.raises(V.NativeError):
        V.Vocabulary.from_arrays(v.words, np.full(W, 14 * 1024 + 1, np.int32), context=ctx)
    ctx.close()


def _mapper(ctx, frames, capacity=None, vocabulary=None):
    from vslam_amd.mapper import LocalMapper
    kw = {"capacity": capacity} if capacity else {}
    m = LocalMapper(BW.K, save_every_keyframe=False, context=ctx, n_hyp=8, **kw)
    if vocabulary is not None:
        m.set_vocabulary(vocabulary)
    for d in frames:
        _add(m, d)
    return m


def _add(m, d):
    rng = np.random.default_rng(len(m.keyframes))
    m.add_keyframe(SMALL_IMG, kps_array(rng.uniform(0, 32, (len(d), 2))), d, np.eye(4))


def _query_equals_restatement(m, frames, qd, words, weights, n_best):
    pos, sc = m.query_keyframes(kps_array(np.zeros((len(qd), 2))), qd, n_best)
    rpos, rsc = B.query(qd, frames, words, weights, n_best)
    assert pos.tolist() == rpos, (pos.tolist()[:10], rpos[:10])
    assert sc.tolist() == rsc      # == on the f64 values
    return rpos, rsc


def test_query_on_the_pan_back_world():
    import vslam_amd as V
    ctx = _ctx()
    w = pan_back()
    words, weights, _ = BW.vocabulary("pan", PAN_WORDS)
    v = V.Vocabulary.from_arrays(words, weights, context=ctx)
    m = build_map(ctx, w)
    with pytest.raises(V.NativeError) as e:
        m.query_keyframes(*w.query())                          # no vocabulary attached
    assert e.value.code == V.MO_ERR_ARG
    m.set_vocabulary(v)
    kps, qd = w.query()
    before = {f: a.copy() for f, a in m.arrays().items()}
    pos, sc = m.query_keyframes(kps, qd, 20)
    rpos, rsc = B.query(qd, w.kf_desc, words, weights, 20)
    assert pos.tolist() == rpos and sc.tolist() == rsc
    assert all(p in range(0, 6) for p in pos[:PAN_FIRST])
    ctx.set_host_timing(True)
    m.query_keyframes(kps, qd, 20)
    assert [n for n, _ in ctx.stage_times()] == ["bow_quantise", "bow_hist", "bow_score", "bow_rank"]
    ctx.set_host_timing(False)
    m._cache = None
    assert all(np.array_equal(before[f], a) for f, a in m.arrays().items())   # the map is read, not changed
    # edge cases: none is an error
    assert m.query_keyframes(kps, qd, 0)[0].tolist() == []
    assert m.query_keyframes(np.zeros(0, V.KP_DTYPE), np.zeros((0, 32), np.uint8), 5)[0].tolist() == []
    pos, sc = m.query_keyframes(kps, qd, 50)                   # more places than keyframes
    rpos, rsc = B.query(qd, w.kf_desc, words, weights, 50)
    assert pos.tolist() == rpos and sc.tolist() == rsc and len(rpos) <= 20
    m.set_vocabulary(None)
    with pytest.raises(V.NativeError):
        m.query_keyframes(kps, qd)
    from vslam_amd.mapper import LocalMapper
    empty = LocalMapper(BW.K, save_every_keyframe=False, context=ctx)
    empty.set_vocabulary(v)
    assert empty.query_keyframes(kps, qd)[0].tolist() == []     # a map without keyframes
    m.close(); empty.close(); ctx.close()


@pytest.mark.parametrize("W", [64, 100])
def test_database_follows_the_keyframe_store(W):
    """keyframes of 60 to 500 rows; the vocabulary attached before and after the keyframes, a removal followed by a new keyframe, a
    restride forced by a wide query frame, a frame of zero-weight words"""
    import vslam_amd as V
    ctx = _ctx()
    rng = np.random.default_rng(W)
    base = rng.integers(0, 256, (300, 32)).astype(np.uint8)
    sizes = [60, 173, 500, 64, 257, 65, 128, 311, 90, 449]
    # (neighbouring keyframes draw from different halves of the base descriptors: no growth step finds a model, the map stays empty)
    frames = [flip(rng, base[150 * (k % 2) + rng.integers(0, 150, n)], 6) for k, n in enumerate(sizes)]
    words, weights, _ = B.train(*BW.rows_of(frames), W, 10)
    assert (weights > 0).any()
    v = V.Vocabulary.from_arrays(words, weights, context=ctx)
    qd = flip(rng, base[rng.integers(60, 260, 200)], 8)
    after = _mapper(ctx, frames, capacity=(4, 512, 16, 32))
    after.set_vocabulary(v)                                                     # attached after the keyframes
    before = _mapper(ctx, frames, capacity=(4, 512, 16, 32), vocabulary=v)      # ... and before them
    for m in (after, before):
        _query_equals_restatement(m, frames, qd, words, weights, 10)
        _query_equals_restatement(m, frames, qd, words, weights, 3)
    # two positions removed, then a keyframe added: the rows follow the slots, the new keyframe is counted by the next query
    m = before
    remove_keyframes(m, [2, 5])
    kept = [f for k, f in enumerate(frames) if k not in (2, 5)]
    _query_equals_restatement(m, kept, qd, words, weights, 10)
    new = flip(rng, base[rng.integers(0, 150, 333)], 6)
    _add(m, new)
    assert len(m.map_points) == 0
    kept.append(new)
    _query_equals_restatement(m, kept, qd, words, weights, 10)
    # a query frame wider than the row capacity restrides the store between two queries
    wide = flip(rng, base[rng.integers(0, 300, 700)], 8)
    _query_equals_restatement(m, kept, wide, words, weights, 10)
    _query_equals_restatement(m, kept, qd, words, weights, 10)
    # every word of the frame has weight 0: nothing scores
    zero = np.flatnonzero(weights == 0)
    if len(zero):
        pos, sc = m.query_keyframes(kps_array(np.zeros((len(zero), 2))), words[zero], 10)
        assert pos.tolist() == [] and B.query(words[zero], kept, words, weights, 10)[0] == []
    wz = weights.copy()
    wz[:] = 0
    m.set_vocabulary(V.Vocabulary.from_arrays(words, wz, context=ctx))          # another vocabulary: the database starts again
    assert m.query_keyframes(kps_array(np.zeros((len(qd), 2))), qd, 10)[0].tolist() == []
    m.set_vocabulary(v)
    _query_equals_restatement(m, kept, qd, words, weights, 10)
    after.close(); before.close(); ctx.close()


def test_equidistant_descriptor_on_the_device():
    import vslam_amd as V
    ctx = _ctx()
    d, words = BW.hand_equidistant()
    weights = np.array([1024, 1024, 1024], np.int32)
    v = V.Vocabulary.from_arrays(words, weights, context=ctx)
    frames = [words[2:3].copy(), words[1:2].copy()]
    m = _mapper(ctx, frames, vocabulary=v)
    pos, sc = m.query_keyframes(kps_array(np.zeros((1, 2))), d[None], 5)
    assert pos.tolist() == [1] and sc.tolist() == [1.0]        # word 1, the lower of the two equidistant words
    m.close(); ctx.close()


@pytest.mark.parametrize("n_kf", [70, 1100])
def test_rank_beyond_a_wave_and_beyond_a_workgroup(n_kf):
    import vslam_amd as V
    ctx = _ctx()
    frames, base = BW.tiny_map_frames(n_kf)
    words, weights, _ = B.train(*BW.rows_of(frames[:64]), 64, 10)
    weights = np.maximum(weights, 1).astype(np.int32)          # (every word counts: more distinct scores, still many ties)
    v = V.Vocabulary.from_arrays(words, weights, context=ctx)
    m = _mapper(ctx, frames, capacity=(4, 16, 16, 32), vocabulary=v)
    qd = flip(np.random.default_rng(1), base[:12], 3)
    kc = [B.counts(d, words) for d in frames]
    for n_best in (10, n_kf, n_kf + 7):
        pos, sc = m.query_keyframes(kps_array(np.zeros((len(qd), 2))), qd, n_best)
        rpos, rsc = B.query(qd, frames, words, weights, n_best, kf_counts=kc)
        assert pos.tolist() == rpos and sc.tolist() == rsc
    assert len(rpos) > min(n_kf, 1024) - 64 and len(set(rsc)) < len(rsc)   # the ranking reaches past the widths, and scores tie
    m.close(); ctx.close()


def _same(a, b):
    (oa, pa, ia), (ob, pb, ib) = a, b
    assert oa == ob and ia["candidates"] == ib["candidates"] and ia["kf_pos"] == ib["kf_pos"]
    assert ia["n_corr"] == ib["n_corr"] and ia["n_inliers"] == ib["n_inliers"]
    assert np.array_equal(ia["point"], ib["point"]) and np.array_equal(ia["inlier"], ib["inlier"])
    assert (pa is None and pb is None) or pa.tobytes() == pb.tobytes()


def test_relocalize_with_preselection():
    import vslam_amd as V
    ctx = _ctx()
    w = BW.reloc_world()
    m = w.build(ctx)
    k = 5
    xy, qd = w.query(k, w.query_pose(k))
    kps = kps_array(xy)
    plain = m.relocalize(kps, qd)
    assert plain[0] and plain[2]["kf_pos"] == k
    with pytest.raises(V.NativeError) as e:
        m.relocalize(kps, qd, preselect=3)                     # no vocabulary
    assert e.value.code == V.MO_ERR_ARG
    v = m.train_vocabulary(RELOC_WORDS, 10)
    words, weights, ran = BW.vocabulary("reloc", RELOC_WORDS)
    assert v.words.tobytes() == words.tobytes() and v.weights.tobytes() == weights.tobytes() and v.iterations == ran
    _same(plain, m.relocalize(kps, qd))                        # the plain call is unchanged by the vocabulary
    _same(plain, m.relocalize(kps, qd, preselect=w.n_kf))      # every keyframe preselected: the plain call's bytes
    _same(plain, m.relocalize(kps, qd, preselect=100))
    first = m.query_keyframes(kps, qd, RELOC_PRE)[0].tolist()
    assert first == B.query(qd, w.kf_desc, words, weights, RELOC_PRE)[0] and k in first
    ok, pose, info = m.relocalize(kps, qd, preselect=RELOC_PRE)
    assert ok and info["kf_pos"] == plain[2]["kf_pos"] and info["n_inliers"] == plain[2]["n_inliers"] and info["n_corr"] == plain[2]["n_corr"]
    assert pose.tobytes() == plain[1].tobytes()
    assert np.array_equal(info["point"], plain[2]["point"]) and np.array_equal(info["inlier"], plain[2]["inlier"])
    cand = [c[0] for c in info["candidates"]]
    assert cand and set(cand) <= set(first)
    by_pos = {c[0]: c for c in plain[2]["candidates"]}
    assert all(c == by_pos[c[0]] for c in info["candidates"] if c[0] in by_pos)   # score and inliers of a candidate do not depend on the others
    # a frame no keyframe shares a word weight with: nothing is selected, nothing is matched
    with pytest.raises(V.NativeError):
        m.relocalize(kps, qd, preselect=0)
    ok, pose, info = m.relocalize(kps_array(np.zeros((1, 2))), words[np.argmin(weights)][None], preselect=2)
    assert not ok and info["candidates"] == []
    m.close(); ctx.close()
