"""LocalMapper.relocalize_batch (mo_map_relocalize_batch) and query_keyframes_batch (mo_map_query_keyframes_batch): every frame of a
batch gets what relocalize / query_keyframes returns for it alone on the same map - integers equal, doubles equal bit for bit - whatever
the order, the company and the grouping; the scores also against the numpy restatements, the first frame against its known pose."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bow_restatement as B
from tests import bow_worlds as BW
from tests.map_worlds import flip, kps_array
from tests.test_bow_cpu import RELOC_PRE, RELOC_WORDS
from tests.test_gpu_relocalize import _World, _ctx, _kps, _pose, _rot

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["candidates", "from_token", "inlier", "kf_id", "kf_pos", "n_corr", "n_inliers", "point"]

_SMALL = {}


def _small_world():
    """RelocWorld with keyframes under 1024 rows (one trip of the gather's block)"""
    if "w" not in _SMALL:
        _SMALL["w"] = BW.RelocWorld(n_w=1200)
        assert max(len(d) for d in _SMALL["w"].kf_desc) < 1024
    return _SMALL["w"]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def _equal(one, batch, i, tag=""):
    """(ok, pose, info) of relocalize against frame i of (ok, poses, infos) of relocalize_batch: every array and scalar"""
    (o1, p1, i1), (ob, pb, ib) = one, batch
    pb, ib = pb[i], ib[i]
    assert bool(o1) == bool(ob[i]), (tag, i, "ok")
    assert (p1 is None) == (pb is None), (tag, i, "pose")
    if p1 is not None:
        assert np.array_equal(_bits(p1), _bits(pb)), (tag, i, "pose", p1 - pb)
    assert sorted(i1) == sorted(ib) == KEYS, (tag, i, sorted(i1), sorted(ib))
    assert i1["candidates"] == ib["candidates"], (tag, i, i1["candidates"], ib["candidates"])
    for f in ("kf_pos", "kf_id", "n_corr", "n_inliers", "from_token"):
        assert type(i1[f]) is type(ib[f]) and i1[f] == ib[f], (tag, i, f, i1[f], ib[f])
    for f in ("point", "inlier"):
        assert i1[f].dtype == ib[f].dtype and i1[f].shape == ib[f].shape and np.array_equal(i1[f], ib[f]), (tag, i, f)


def _singles(m, frames, **kw):
    return [m.relocalize(k, d, **kw) for k, d in frames]


def _all_equal(m, frames, tag, **kw):
    """the batch against the singles; returns (singles, batch)"""
    batch_kw = dict(kw)
    one = _singles(m, frames, **{k: v for k, v in kw.items() if k != "max_pairs"})
    batch = m.relocalize_batch(frames, **batch_kw)
    assert len(batch[0]) == len(batch[1]) == len(batch[2]) == len(frames)
    for i in range(len(frames)):
        _equal(one[i], batch, i, tag)
    return one, batch


def _empty():
    import vslam_amd as V
    return np.zeros(0, V.KP_DTYPE), np.zeros((0, 32), np.uint8)


def _random(n, seed):
    rng = np.random.default_rng(seed)
    return (_kps(np.column_stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)]).astype(np.float32)),
            rng.integers(0, 256, (n, 32)).astype(np.uint8))


def _cut(frame, n):
    return np.ascontiguousarray(frame[0][:n]), np.ascontiguousarray(frame[1][:n])


def _bw_query(w, k, seed=5, noise=0.0):
    xy, d = w.query(k, w.query_pose(k), seed=seed)
    if noise:
        xy = (xy + np.random.default_rng(seed + 100).normal(0, noise, xy.shape)).astype(np.float32)
    return kps_array(xy), d


def _seven(w):
    """the mixed batch of the group, map and poison tests on a RelocWorld: two real queries, nothing to find, an empty frame, an odd cut,
    a repeated frame, a third query"""
    q5, q2, q7 = _bw_query(w, 5), _bw_query(w, 2, seed=9, noise=0.5), _bw_query(w, 7, seed=11)
    n_odd = (len(q5[0]) * 2 // 3) | 1
    return [q5, q2, _random(301, 3), _empty(), _cut(q5, n_odd), q5, q7]


def test_equal_to_the_single_call_order_and_company():
    ctx = _ctx()
    w = _World(ctx)
    T5 = w.poses[5] @ _pose(_rot([0.02, -0.03, 0.01]), np.array([0.08, -0.05, 0.1]))
    T2 = w.poses[2] @ _pose(_rot([-0.01, 0.02, 0.0]), np.array([-0.05, 0.04, 0.06]))
    clean = w.query(5, T5)
    noisy = w.query(2, T2, noise=0.5, seed=9)
    n_odd = (len(clean[0]) * 2 // 3) | 1
    assert n_odd % 64 and len(clean[0]) > 1024   # (past the gather's block of 1024 rows)
    frames = [clean, noisy, _random(500, 8), _empty(), _cut(clean, 1), _cut(clean, 2), _cut(clean, 3), _cut(clean, n_odd), clean]
    one, batch = _all_equal(w.m, frames, "as given")
    ok, poses, infos = batch
    print("ok %s, kf_pos %s, n_inliers %s, candidates %s" % (ok.tolist(), [x["kf_pos"] for x in infos], [x["n_inliers"] for x in infos],
                                                             [len(x["candidates"]) for x in infos]))
    assert ok[0] and ok[8] and infos[0]["kf_pos"] == 5 and not ok[2:7].any()
    assert np.abs(poses[0][:3, :3] - T5[:3, :3]).max() < 1e-6 and np.abs(poses[0][:3, 3] - T5[:3, 3]).max() < 1e-6, poses[0] - T5
    for i in (2, 3, 4, 5, 6):   # nothing to find, no keypoints, fewer than a P3P sample: no candidate, no pose
        assert infos[i]["candidates"] == [] and poses[i] is None and infos[i]["kf_pos"] == -1 and (infos[i]["point"] == -1).all()
    assert [len(infos[i]["point"]) for i in (3, 4, 5, 6)] == [0, 1, 2, 3]
    rev = w.m.relocalize_batch(frames[::-1])
    for i in range(len(frames)):
        _equal(one[i], rev, len(frames) - 1 - i, "reversed")
    for i in range(len(frames)):
        _equal(one[i], w.m.relocalize_batch([frames[i]]), 0, "alone")
    from tests.test_gpu_scratch_poison import _flat
    assert _flat(w.m.relocalize_batch(frames)) == _flat(batch)   # a batch run twice gives equal bytes
    # other parameters reach every frame: fewer candidates and hypotheses, another seed and threshold
    _all_equal(w.m, frames[:3], "parameters", max_candidates=2, n_hyp=37, seed=77, threshold=2.0, ratio_threshold=0.8, min_inliers=20)
    assert w.m.relocalize_batch([])[1:] == ([], []) and w.m.last_reloc_groups == 0
    assert ctx.dev_status() == 0
    w.m.close(); ctx.close()


def test_a_candidate_at_the_score_gate():
    """queries cut to 14 and to 15 rows of keyframe 7 that only keyframe 7 observes, plus random rows: |C_7| is exactly 14 (no candidate)
    and exactly 15 (RL_MIN_SCORE: a candidate)"""
    ctx = _ctx()
    w = BW.reloc_world()
    m = w.build(ctx)
    k = w.n_kf - 1
    rows = np.array([o[k] for o in w.obs if list(o) == [k]])
    assert len(rows) >= 15
    rnd = _random(60, 17)
    frames = []
    for n in (14, 15):
        xy = np.vstack([w.kf_xy[k][rows[:n]], np.column_stack([rnd[0]["x"], rnd[0]["y"]])]).astype(np.float32)
        frames.append((kps_array(xy), np.vstack([w.kf_desc[k][rows[:n]], rnd[1]])))
    want = [B.brute_force_candidates(d, w.kf_desc, w.obs_off, w.obs_kf, w.obs_kp)[:2] for _, d in frames]
    assert want[0][1][k] == 14 and want[1][1][k] == 15 and max(s for j, s in enumerate(want[1][1]) if j != k) < 14, want
    one, batch = _all_equal(m, frames + frames[::-1], "gate")
    infos = batch[2]
    # the device's scores first: below the gate no candidate, at the gate keyframe 7 with its 15 correspondences
    assert infos[0]["candidates"] == [] and infos[3]["candidates"] == []
    for i in (1, 2):
        assert [c[:2] for c in infos[i]["candidates"]] == [(k, 15)] and infos[i]["n_corr"] == 15 and infos[i]["kf_pos"] == k
        assert (infos[i]["point"][:15] >= 0).all() and (infos[i]["point"][15:] == -1).all()
        assert infos[i]["n_inliers"] == 15 and not batch[0][i]     # exact rows of the keyframe: all inliers, fewer than min_inliers
    assert batch[0].tolist() == [False] * 4
    assert m.relocalize_batch(frames, min_inliers=15)[0].tolist() == [False, True]
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_preselection():
    import vslam_amd as V
    from tests.test_gpu_scratch_poison import _flat
    ctx = _ctx()
    w = BW.reloc_world()
    m = w.build(ctx)
    q5, q2 = _bw_query(w, 5), _bw_query(w, 2, seed=9, noise=0.5)
    with pytest.raises(V.NativeError) as e:
        m.relocalize_batch([q5], preselect=3)                      # no vocabulary
    assert e.value.code == V.MO_ERR_ARG
    with pytest.raises(V.NativeError) as e:
        m.query_keyframes_batch([q5])
    assert e.value.code == V.MO_ERR_ARG
    m.train_vocabulary(RELOC_WORDS, 10)
    words, weights, _ = BW.vocabulary("reloc", RELOC_WORDS)
    nothing = (kps_array(np.zeros((1, 2))), words[np.argmin(weights)][None])   # the least-weight word's descriptor: selects nothing
    frames = [q5, nothing, q2, _empty(), _random(301, 3), q5]
    plain = m.relocalize_batch(frames)
    for pre in (1, RELOC_PRE, w.n_kf, 100):
        one, batch = _all_equal(m, frames, "preselect %d" % pre, preselect=pre)
        assert batch[2][1]["candidates"] == [] and not batch[0][1]
        if pre >= w.n_kf:
            assert _flat(batch) == _flat(plain), pre
    one, batch = _all_equal(m, frames, "preselect, one frame per group", preselect=RELOC_PRE, max_pairs=RELOC_PRE)
    assert m.last_reloc_groups == len(frames)
    assert batch[0][0] and batch[2][0]["kf_pos"] == 5
    with pytest.raises(V.NativeError) as e:
        m.relocalize_batch(frames, preselect=0)
    assert e.value.code == V.MO_ERR_ARG
    # the query alone: per frame query_keyframes', and the restatement's on the host
    kc = [B.counts(d, words) for d in w.kf_desc]
    for nb in (RELOC_PRE, w.n_kf + 2, 0):
        got = m.query_keyframes_batch(frames, nb)
        assert len(got) == len(frames)
        for (kps, d), (pos, sc) in zip(frames, got):
            p1, s1 = m.query_keyframes(kps, d, nb)
            rpos, rsc = B.query(d, w.kf_desc, words, weights, nb, kf_counts=kc)
            assert pos.tolist() == p1.tolist() == rpos and sc.tolist() == s1.tolist() == rsc, (nb, pos, p1, rpos)
    assert got[1][0].tolist() == [] and m.query_keyframes_batch([], 5) == []
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_query_batch_ranks_beyond_a_workgroup():
    """1100 keyframes of 8 rows: the ranking workgroup of every frame walks more positions than it has threads"""
    import vslam_amd as V
    from tests.test_gpu_bow import _mapper
    ctx = _ctx()
    n_kf = 1100
    frames, base = BW.tiny_map_frames(n_kf)
    words, weights, _ = B.train(*BW.rows_of(frames[:64]), 64, 10)
    weights = np.maximum(weights, 1).astype(np.int32)
    v = V.Vocabulary.from_arrays(words, weights, context=ctx)
    m = _mapper(ctx, frames, capacity=(4, 16, 16, 32), vocabulary=v)
    rng = np.random.default_rng(1)
    qs = [flip(rng, base[:12], 3), flip(rng, base[5:36], 2), flip(rng, base[20:23], 3)]
    batch = [(kps_array(np.zeros((len(q), 2))), q) for q in qs]
    kc = [B.counts(d, words) for d in frames]
    for n_best in (10, n_kf + 7):
        got = m.query_keyframes_batch(batch, n_best)
        for q, (pos, sc) in zip(qs, got):
            rpos, rsc = B.query(q, frames, words, weights, n_best, kf_counts=kc)
            assert pos.tolist() == rpos and sc.tolist() == rsc
    rpos, rsc = B.query(qs[0], frames, words, weights, n_kf + 7, kf_counts=kc)
    assert len(rpos) > 1024 - 64 and len(set(rsc)) < len(rsc)   # the ranking reaches past the width, and scores tie
    assert ctx.dev_status() == 0
    m.close(); v.close(); ctx.close()


def test_groups():
    from tests.test_gpu_scratch_poison import _flat
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    w = BW.reloc_world()
    m = w.build(ctx)
    frames = _seven(w)
    one, ref = _all_equal(m, frames, "default budget")
    assert m.last_reloc_groups == 1 == LocalMapper.reloc_batch_plan(7, w.n_kf, 4096)[1]
    assert ref[0][0] and ref[0][5] and not ref[0][2] and not ref[0][3], ref[0]
    want = _flat(ref)
    # one frame per group; boundaries that do not divide the batch (2 + 2 + 2 + 1); a budget below one frame's pairs
    for max_pairs, groups in ((w.n_kf, 7), (3 * w.n_kf - 1, 4), (1, 7), (7 * w.n_kf, 1), (4 * w.n_kf, 2)):
        assert LocalMapper.reloc_batch_plan(7, w.n_kf, 4096, max_pairs)[1] == groups
        got = m.relocalize_batch(frames, max_pairs=max_pairs)
        assert m.last_reloc_groups == groups, (max_pairs, m.last_reloc_groups)
        assert _flat(got) == want, max_pairs
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def _call(m, frames, stride, nf=None, n_pre=-1, max_pairs=0, nc=4, null=None, fill=-7):
    """mo_map_relocalize_batch through the C boundary on arrays filled with `fill`; null: the name of an array passed as NULL"""
    import vslam_amd as V
    n = len(frames)
    refs = (V.FrameRef * max(n, 1))()
    keep = []
    for i, (k, d) in enumerate(frames):
        refs[i], _, arrays = m._frame_ref(k, d)
        keep.append(arrays)
    a = {"point": np.full((n, stride), fill, np.int32), "inlier": np.full((n, stride), 7, np.uint8), "cand_pos": np.full((n, nc), fill, np.int32),
         "cand_score": np.full((n, nc), fill, np.int32), "cand_inliers": np.full((n, nc), fill, np.int32), "pose": np.full((n, 12), float(fill))}
    for f in ("ok", "kf_pos", "n_cand", "n_corr", "n_inliers", "from_token"):
        a[f] = np.full(n, fill, np.int32)
    order = ["point", "inlier", "cand_pos", "cand_score", "cand_inliers", "pose", "ok", "kf_pos", "n_cand", "n_corr", "n_inliers", "from_token"]
    out = V.MapRelocBatchOut(stride, *[None if f == null else a[f].ctypes.data for f in order])
    out.n_ok, out.n_groups = fill, fill
    prm = V.MapRelocBatchParams(V.MapRelocParams(0.75, 3.0, 50, nc, 512, m.seed), n_pre, max_pairs)
    Kc = np.ascontiguousarray(m.camera_matrix, np.float64).reshape(9)
    rc = m.lib.mo_map_relocalize_batch(m._h, refs, n if nf is None else nf, V._ptr(Kc), C.byref(prm), C.byref(out))
    return rc, out, a


def _untouched(a, fill=-7):
    return all((v == (7 if f == "inlier" else fill)).all() for f, v in a.items())


def test_sources_and_strides():
    import vslam_amd as V
    from tests.helpers import synthetic_frame
    ctx = _ctx()
    w = _small_world()
    m = w.build(ctx)
    prm = V.orb_params(nfeatures=500)
    (ka, da), = ctx.orb_detect_compute(synthetic_frame(20250523), prm)
    for s in range(4):   # four more extractions: the first result's slot is taken over, its token goes stale
        (kb, db), = ctx.orb_detect_compute(synthetic_frame(20250524 + s), prm)
    assert V.resident_token(ctx, db, kb) and V.resident_token(ctx, da, ka) and len(ka) > 0 and len(kb) > 0
    host = _bw_query(w, 5)
    frames = [(kb, db), host, (ka, da)]
    one, batch = _all_equal(m, frames, "mixed sources")
    assert [x["from_token"] for x in batch[2]] == [True, False, False] and batch[0][1] and batch[2][1]["kf_pos"] == 5
    # stride larger than every n: each frame's rows as the tight call gave them, the rows past n untouched
    ns = [len(k) for k, _ in frames]
    stride = max(ns) + 77
    rc, out, a = _call(m, frames, stride)
    assert rc == 0 and out.n_ok == int(batch[0].sum()) and out.n_groups == 1
    for i, n in enumerate(ns):
        info = batch[2][i]
        assert np.array_equal(a["point"][i, :n], info["point"]) and np.array_equal(a["inlier"][i, :n].astype(bool), info["inlier"])
        assert (a["point"][i, n:] == -7).all() and (a["inlier"][i, n:] == 7).all()
        assert a["kf_pos"][i] == info["kf_pos"] and a["n_corr"][i] == info["n_corr"] and a["n_inliers"][i] == info["n_inliers"]
        assert [tuple(int(a[f][i, j]) for f in ("cand_pos", "cand_score", "cand_inliers")) for j in range(a["n_cand"][i])] == info["candidates"]
        assert (a["cand_pos"][i, a["n_cand"][i]:] == -1).all()
        if batch[1][i] is not None:
            assert np.array_equal(_bits(a["pose"][i]), _bits(batch[1][i][:3, :].reshape(12)))
        else:
            assert np.isnan(a["pose"][i]).all()
    # the stated errors, each with nothing written
    for kw in ({"stride": max(ns) - 1}, {"stride": stride, "nf": V.RELOC_BATCH_MAX + 1}, {"stride": stride, "nf": -1}, {"stride": stride, "n_pre": 0},
               {"stride": stride, "n_pre": 3}, {"stride": stride, "null": "pose"}, {"stride": stride, "null": "from_token"}, {"stride": stride, "max_pairs": -1},
               {"stride": stride, "nc": 65}):
        rc, out, a = _call(m, frames, **kw)
        assert rc == V.MO_ERR_ARG and _untouched(a) and out.n_ok == -7 and out.n_groups == -7, kw
    rc, out, a = _call(m, frames, stride, nf=0)   # no frame: nothing runs, nothing is touched but the two counts
    assert rc == 0 and _untouched(a) and out.n_ok == 0 and out.n_groups == 0
    # a map without keyframes: every frame its defaults
    from vslam_amd.mapper import LocalMapper
    empty = LocalMapper(BW.K, save_every_keyframe=False, context=ctx)
    e = empty.relocalize_batch(frames)
    for i, fr in enumerate(frames):
        _equal(empty.relocalize(*fr), e, i, "empty map")
        assert not e[0][i] and e[1][i] is None and e[2][i]["candidates"] == []
    assert empty.last_reloc_groups == 0
    assert ctx.dev_status() == 0
    empty.close(); m.close(); ctx.close()


def test_a_frame_wider_than_the_store_comes_first():
    """the store's row stride is grown before anything is staged: the batch on a fresh map equals the single calls on another fresh map"""
    ctx = _ctx()
    w = _small_world()
    rows = max(len(d) for d in w.kf_desc)
    q5 = _bw_query(w, 5)
    rnd = _random(rows + 300 - len(q5[0]), 4)
    wide = (np.concatenate([q5[0], rnd[0]]), np.vstack([q5[1], rnd[1]]))
    assert len(wide[0]) == rows + 300 and len(q5[0]) < rows
    frames = [wide, q5, _bw_query(w, 2, seed=9)]
    cap = (16, ((rows + 63) // 64) * 64, 1 << 12, 1 << 13)
    m1, m2 = w.build(ctx, capacity=cap), w.build(ctx, capacity=cap)
    batch = m1.relocalize_batch(frames)
    one = _singles(m2, frames)
    for i in range(3):
        _equal(one[i], batch, i, "restride")
    assert batch[0][0] and batch[0][1] and batch[2][0]["kf_pos"] == 5 and batch[2][1]["kf_pos"] == 5
    _all_equal(m1, frames, "after the restride")
    assert ctx.dev_status() == 0
    m1.close(); m2.close(); ctx.close()


def test_maps_that_changed(tmp_path):
    """after erase_keyframes (positions no longer equal slots), after erase_map_points, and on a mapper loaded from a saved state"""
    from tests.test_gpu_scratch_poison import _flat
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    w = _small_world()
    m = w.build(ctx)
    frames = _seven(w)
    _all_equal(m, frames, "as built")
    m.erase_keyframes([1, 4])
    m._cache = None
    before = {f: a.copy() for f, a in m.arrays().items()}
    one, batch = _all_equal(m, frames, "keyframes erased")
    assert batch[0][0] and batch[2][0]["kf_pos"] == 3   # keyframe 5 at its new position
    m._cache = None
    assert all(a.tobytes() == before[f].tobytes() for f, a in m.arrays().items())     # the map is read, not changed
    a = m.arrays()
    gone = np.flatnonzero(np.arange(len(a["id"])) % 3 == 0)
    m.erase_map_points(gone)
    one, batch = _all_equal(m, frames, "points erased")
    assert batch[0][0]
    path = tmp_path / "state.npz"
    m.save_state(path)
    m2 = LocalMapper.load_state(path, context=ctx)
    one2, batch2 = _all_equal(m2, frames, "loaded")
    assert _flat(batch2) == _flat(batch)
    m2._cache = None
    m._cache = None
    assert all(x.tobytes() == m.arrays()[f].tobytes() for f, x in m2.arrays().items())
    assert ctx.dev_status() == 0
    m2.close(); m.close(); ctx.close()


def test_poison():
    """the mixed batch, plain and preselected, under two poison bytes, a fresh context and map each: the unpoisoned bytes; the fill
    counters grow by the batch's own buffers"""
    from tests.test_gpu_scratch_poison import _checked, _filled, _flat, _same, _set
    w = _small_world()
    frames = _seven(w)
    want = None
    for byte in (None, 255, 90):
        ctx = _ctx()
        if byte is not None:
            _set(ctx, byte)
        m = w.build(ctx)
        m.train_vocabulary(64, 3)
        m.relocalize(*frames[0])
        m.relocalize(*frames[0])
        f0 = _filled(ctx)[0]
        m.relocalize(*frames[0])
        d0 = _filled(ctx)[0] - f0                        # buffers one call fills before the batch's feature exists
        got = [_flat(_checked(ctx, lambda: m.relocalize_batch(frames), byte is not None)),
               _flat(_checked(ctx, lambda: m.relocalize_batch(frames, max_pairs=2 * w.n_kf), byte is not None))]
        f1 = _filled(ctx)[0]
        m.relocalize(*frames[0])
        d1 = _filled(ctx)[0] - f1
        # the staged rows, the counts, point_of, the pair list (2), the matcher's outputs (3), the scores, C_k (3), the per-keypoint
        # outputs (2) and the result blocks
        assert d1 - d0 == (16 if byte is not None else 0), (d0, d1)
        got.append(_flat(_checked(ctx, lambda: m.relocalize_batch(frames, preselect=2), byte is not None)))
        got.append(_flat(_checked(ctx, lambda: m.query_keyframes_batch(frames, 3), byte is not None)))
        assert got[0] == got[1]
        if want is None:
            want = got
        else:
            for g, x, tag in zip(got, want, ("plain", "groups", "preselect", "query")):
                _same(g, x, (byte, tag))
            _same(_flat(_checked(ctx, lambda: m.relocalize_batch(frames), True)), want[0], (byte, "again"))
        assert ctx.dev_status() == 0
        m.close(); ctx.close()


def test_run_frames_localizes_in_a_loaded_map(tmp_path, capsys):
    """run_frames.py --load-state ... --localize --batch 4 prints, per frame, what relocalize of that frame on the loaded mapper returns"""
    import vslam_amd as V
    from tests.test_gpu_dropin import _run_frames_module
    from vslam_amd.mapper import LocalMapper
    from vslam_amd.stream import FrameStream
    mod = _run_frames_module()
    state = str(tmp_path / "state.npz")
    mod.main(["--max-frames", "14", "--keyframe-every", "4", "--map", str(tmp_path / "map.ply"), "--save-state", state])
    assert "state saved to " + state in capsys.readouterr().out
    r = subprocess.run([sys.executable, os.path.join(ROOT, "visual-slam_amd", "examples", "run_frames.py"), "--max-frames", "14", "--load-state", state,
                        "--localize", "--batch", "4"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ": localize " in ln]
    print("\n".join(ln[:110] for ln in lines))
    # the same extraction (chunks of 4: three whole ones and a part), then the single call per frame on the loaded mapper
    frames = np.stack(list(mod.synthetic_sequence(14)))
    orb = mod.DEFAULTS["orb"]
    prm = V.orb_params(nfeatures=orb["n_features"], scale_factor=orb["scale_factor"], nlevels=orb["n_levels"], fast_threshold=orb["min_threshold"])
    Kd = np.array(mod.DEFAULTS["camera"]["camera_matrix"], np.float64).reshape(3, 3)
    m = LocalMapper.load_state(state)
    fs = FrameStream(Kd, width=frames.shape[2], height=frames.shape[1], channels=1, chunk=4, prm=prm, copy=True)
    try:
        want = [mod.localize_line(x.index, *m.relocalize(x.keypoints, x.descriptors)) for x in fs.run(frames)]
    finally:
        fs.close()
    assert len(lines) == 14 and lines == want
    assert m.ctx.dev_status() == 0
    m.close()
