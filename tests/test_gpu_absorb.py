"""mo_map_absorb and mo_map_loop_candidates_among on the GPU: the export of the absorbing map equals the numpy restatement
(tests/absorb_restatement.py) applied to the two exports, byte for byte, with and without the poison fill, over keyframe counts, row
counts on both copy paths, a forced restride, dead slots, stale entries and injected points; an absorbed mapper has the future of a
mapper imported from the restated snapshot; every refusal leaves the map unchanged; the masked loop candidates equal their restatement
bit for bit and the unmasked forms give the bytes of the plain call."""
import ctypes as C

import numpy as np
import pytest

from tests import absorb_restatement as AR
from tests import loop_restatement as LR
from tests import loop_worlds as LW
from tests import merge_worlds as MW

pytestmark = pytest.mark.gpu

INT32_MIN = -2 ** 31
K = np.array([[50.0, 0, 32.0], [0, 50.0, 24.0], [0, 0, 1.0]])


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _same(a, b, tag):
    from tests.test_gpu_scratch_poison import _flat, _same as same
    same(_flat(a), _flat(b), tag)


def _add_points(m, rng, n, id_hi=5000):
    """n points given to the library as they are: 0 .. 3 entries each, keys and rows valid from the front, valid from the end, one past
    the end, far out of range or INT32_MIN; dref_kf an ordinal for every second point, an injected reference for the others"""
    if n == 0:
        return
    from tests.test_gpu_snapshot import _sizes
    import vslam_amd as V
    n_kf = _sizes(m.lib, m._h)[0]
    counts = [kf._rows for kf in m.keyframes]
    off = np.concatenate([[0], np.cumsum(rng.integers(0, 4, n))]).astype(np.int32)
    no = int(off[-1])
    kind = rng.integers(0, 10, no)
    okf, okp = np.zeros(max(no, 1), np.int32), np.zeros(max(no, 1), np.int32)
    for e in range(no):
        k = int(rng.integers(0, max(n_kf, 1)))
        c = counts[k] if n_kf else 0
        r = int(rng.integers(0, max(c, 1)))
        okf[e], okp[e] = {0: (k, r), 1: (k, r), 2: (k, r), 3: (k - n_kf, r), 4: (k, r - c), 5: (-1, r), 6: (n_kf, r), 7: (k, c),
                          8: (INT32_MIN, r), 9: (k + 70000, INT32_MIN)}[int(kind[e])]
    xyz = rng.normal(0, 3, (n, 3)).astype(np.float32)
    col = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    ids = rng.integers(0, id_hi, n).astype(np.int32)
    dkf = np.where(np.arange(n) % 2 == 0, rng.integers(0, max(n_kf, 1), n), -(np.arange(n) + 1)).astype(np.int32)
    drow = rng.integers(0, 40, n).astype(np.int32)
    m._check(m.lib.mo_map_add_points(m._h, n, V._ptr(xyz), V._ptr(col), V._ptr(ids), V._ptr(off), V._ptr(okf), V._ptr(okp), V._ptr(dkf), V._ptr(drow)))
    m._cache = None
    m._sync_size()


def _build(ctx, seed, rows, n_points, erase=None, stride=16):
    """a map of len(rows) random keyframes (no two share a descriptor: no growth step finds a model), position `erase` erased (a dead
    slot: slot != position behind it), then the points"""
    from tests.test_gpu_snapshot import _rand_kf
    from vslam_amd.mapper import LocalMapper
    rng = np.random.default_rng(seed)
    m = LocalMapper(K, save_every_keyframe=False, context=ctx, n_hyp=8, capacity=(2, stride, 16, 32))
    for r in rows:
        _rand_kf(m, rng, r)
    if erase is not None:
        m.erase_keyframes([erase])
    _add_points(m, rng, n_points)
    return m


def _absorb_raw(dst, src, shift):
    import vslam_amd as V
    prm, out = V.MapAbsorbParams(shift), V.MapAbsorbOut()
    rc = dst.lib.mo_map_absorb(dst._h, src._h, C.byref(prm), C.byref(out))
    return rc, out


# (rows of dst's keyframes, dst's erased position, dst's points, rows of src's keyframes, src's erased position, src's points)
SHAPES = {
    "both_empty": ([], None, 0, [], None, 0),
    "empty_src": ([5, 5, 5], None, 3, [], None, 0),
    "empty_dst": ([], None, 0, [3, 5, 4], None, 257),
    "restride_one_each": ([4], None, 1, [33], None, 255),
    "dead_slots_every_row_count": ([0, 1, 3, 4], 1, 257, [5, 33, 0, 1, 0, 3], 4, 1025),
    "five_into_five_no_src_points": ([3, 4, 5, 33, 1, 5], 4, 1025, [1, 0, 4, 4, 3], None, 0),
    "src_points_without_keyframes": ([4, 4], None, 5, [], None, 7),
    "one_into_three_odd_stride": ([3, 1, 5], None, 255, [5], None, 1),
}
_EXPORTS = {}


@pytest.mark.parametrize("poison", [-1, 171])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_absorb_equals_the_restatement(shape, poison):
    from tests.test_gpu_snapshot import _sizes
    from vslam_amd import snapshot as S
    d_rows, d_erase, d_pts, s_rows, s_erase, s_pts = SHAPES[shape]
    ctx = _ctx()
    try:
        ctx._check(ctx.lib.mo_dbg_set_poison(ctx.h, poison))
        dst = _build(ctx, 11, d_rows, d_pts, d_erase, stride=21 if "odd_stride" in shape else 16)
        src = _build(ctx, 12, s_rows, s_pts, s_erase, stride=40)
        a, b = dst.export_state(), src.export_state()
        slots0 = _sizes(dst.lib, dst._h)[5]
        want = AR.absorb(a, b, 7)
        rc, out = _absorb_raw(dst, src, 7)
        assert rc == 0, ctx.lib.mo_last_error(ctx.h)
        dst._cache = None
        dst._sync_size()
        got = S.export_map(dst.lib, dst._h, dst._check)
        _same(got, want, (shape, poison))
        _same(src.export_state(), b, (shape, poison, "src is only read"))
        da, db, dw = AR.dims_of(a), AR.dims_of(b), AR.dims_of(want)
        assert (out.kf_offset, out.slot_offset, out.point_offset, out.obs_offset, out.id_offset, out.ordinal_offset) == \
            (da["n_kf"], slots0, da["n_pts"], da["n_obs"], da["id_bound"], da["kf_stored"])
        noop = db["n_kf"] == 0 and db["n_pts"] == 0
        assert (out.n_kf, out.n_pts, out.n_obs, out.id_bound, out.kf_stored) == (dw["n_kf"], dw["n_pts"], dw["n_obs"], dw["id_bound"], dw["kf_stored"])
        assert out.n_slots == slots0 + (0 if noop else db["n_kf"]) == _sizes(dst.lib, dst._h)[5]   # src's dead slots are shed, dst's stay
        if noop:
            _same(got, a, (shape, "no change"))
        if d_erase is not None:
            assert slots0 == da["n_kf"] + 1
        if shape == "restride_one_each":
            assert max(b["kf_cnt"]) > 16   # wider than dst's stride was
        # the restated snapshot obeys every rule of an import (snapshot_violation), and the absorbed map still answers
        h = S.import_map(dst.lib, ctx.h, want, (0, 0, 0, 0), dst._check)
        dst.lib.mo_map_destroy(h)
        if dw["n_kf"]:   # (through the library: the raw absorb left the mapper's own keyframe list behind)
            import vslam_amd as V
            from tests import covis_restatement as CR
            W, nk = np.zeros((dw["n_kf"], dw["n_kf"]), np.int32), C.c_int32(0)
            assert dst.lib.mo_map_covisibility(dst._h, V._ptr(W), C.byref(nk)) == 0 and nk.value == dw["n_kf"]
            assert np.array_equal(W, np.asarray(CR.covisibility(want["obs_off"], want["obs_kf"], want["obs_kp"], want["kf_cnt"].tolist())))
        assert ctx.dev_status() == 0
        _EXPORTS[(shape, poison)] = got
        if (shape, -1) in _EXPORTS and (shape, 171) in _EXPORTS:
            _same(_EXPORTS[(shape, 171)], _EXPORTS[(shape, -1)], (shape, "poisoned"))
        dst.close(); src.close()
    finally:
        ctx._check(ctx.lib.mo_dbg_set_poison(ctx.h, -1))
        ctx.close()


def test_absorb_stage_names_and_two_absorbs_in_a_row():
    ctx = _ctx()
    dst, src = _build(ctx, 3, [5, 4], 9), _build(ctx, 4, [3, 33, 1], 300, erase=1)
    a, b = dst.export_state(), src.export_state()
    ctx.set_host_timing(True)
    assert _absorb_raw(dst, src, 0)[0] == 0
    assert [n for n, _ in ctx.stage_times()] == ["absorb_rows", "absorb_points", "absorb_obs"]
    ctx.set_host_timing(False)
    assert _absorb_raw(dst, src, 2)[0] == 0   # the same src again: it is only read
    dst._cache = None
    dst._sync_size()
    _same(dst.export_state(), AR.absorb(AR.absorb(a, b, 0), b, 2), "twice")
    dst.close(); src.close(); ctx.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_map_unchanged():
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    ctx, ctx2 = _ctx(), _ctx()
    dst, src = _build(ctx, 5, [4, 3], 20), _build(ctx, 6, [5], 10)
    far = _build(ctx2, 7, [5], 10)
    before = dst.export_state()
    prm, out = V.MapAbsorbParams(0), V.MapAbsorbOut()
    lib = dst.lib

    def refused(rc, code, text):
        assert rc == code and text in lib.mo_last_error(ctx.h).decode(), (rc, lib.mo_last_error(ctx.h))
        _same(dst.export_state(), before, text)
    refused(lib.mo_map_absorb(dst._h, None, C.byref(prm), C.byref(out)), V.MO_ERR_ARG, "NULL argument")
    refused(lib.mo_map_absorb(dst._h, src._h, None, C.byref(out)), V.MO_ERR_ARG, "NULL argument")
    refused(lib.mo_map_absorb(dst._h, src._h, C.byref(prm), None), V.MO_ERR_ARG, "NULL argument")
    assert lib.mo_map_absorb(None, src._h, C.byref(prm), C.byref(out)) == V.MO_ERR_ARG
    refused(lib.mo_map_absorb(dst._h, dst._h, C.byref(prm), C.byref(out)), V.MO_ERR_ARG, "cannot absorb itself")
    refused(lib.mo_map_absorb(dst._h, far._h, C.byref(prm), C.byref(out)), V.MO_ERR_ARG, "different contexts")
    neg = V.MapAbsorbParams(-1)
    refused(lib.mo_map_absorb(dst._h, src._h, C.byref(neg), C.byref(out)), V.MO_ERR_ARG, "dref_injected_shift")
    # a sum past int32: two maps whose id bounds add up past 2^31 (one point each with an id just under 2^31 / 2 ... and above)
    big_a, big_b = _build(ctx, 8, [3], 0), _build(ctx, 9, [3], 0)
    _add_points(big_a, np.random.default_rng(1), 4, id_hi=5)
    _add_points(big_b, np.random.default_rng(2), 4, id_hi=5)
    for m, top in ((big_a, 2 ** 30 + 5), (big_b, 2 ** 30)):
        one = np.array([top], np.int32)
        z3, c3, z1, o2 = np.zeros(3, np.float32), np.zeros(3, np.uint8), np.zeros(1, np.int32), np.zeros(2, np.int32)
        m._check(lib.mo_map_add_points(m._h, 1, V._ptr(z3), V._ptr(c3), V._ptr(one), V._ptr(o2), V._ptr(z1), V._ptr(z1), V._ptr(z1), V._ptr(z1)))
        m._cache = None
        m._sync_size()
    ea = big_a.export_state()
    assert AR.dims_of(ea)["id_bound"] + AR.dims_of(big_b.export_state())["id_bound"] > 2 ** 31
    rc = lib.mo_map_absorb(big_a._h, big_b._h, C.byref(prm), C.byref(out))
    assert rc == V.MO_ERR_CAPACITY and "beyond int32 indexing" in lib.mo_last_error(ctx.h).decode()
    _same(big_a.export_state(), ea, "int32")
    # LocalMapper.absorb refuses another context and another camera matrix before the library is touched
    with pytest.raises(ValueError, match="context"):
        dst.absorb(far)
    other = LocalMapper(K + np.array([[1e-12, 0, 0], [0, 0, 0], [0, 0, 0]]), save_every_keyframe=False, context=ctx, n_hyp=8, capacity=(2, 16, 16, 32))
    with pytest.raises(ValueError, match="camera matrix"):
        dst.absorb(other)
    with pytest.raises(V.NativeError):
        dst.absorb(dst)
    _same(dst.export_state(), before, "python refusals")
    assert len(dst.keyframes) == 2 and ctx.dev_status() == 0
    # ... and the next valid absorb works
    off = dst.absorb(src)
    assert off["kf_offset"] == 2 and off["n_kf"] == 3 and [kf["id"] for kf in dst.keyframes] == [0, 1, 2] and dst._kf_serials == [0, 1, 2]
    for m in (dst, src, far, big_a, big_b, other):
        m.close()
    ctx.close(); ctx2.close()


# ---- same future ---------------------------------------------------------------------------------------------------------------------------
def _future(m, w, rng_seed=31):
    """what a mapper answers from here on, each call on the map the one before left"""
    from tests.map_worlds import kps_array
    rng = np.random.default_rng(rng_seed)
    kps, qd = kps_array(w.kf_xy[3]), w.kf_desc[3]
    out = {"covisibility": m.covisibility(), "track": m.track_local_map(kps, qd, w.kf_poses[3], window=0),
           "track_covisible": m.track_local_map(kps, qd, w.kf_poses[3], local="covisible"),
           "fuse": m.fuse_map_points(image_size=w.image_size, window=0)}
    m.erase_keyframes([5, 22])
    out["erased"] = m.export_state()
    n = 90
    xy = np.column_stack([rng.uniform(0, w.image_size[0], n), rng.uniform(0, w.image_size[1], n)])
    m.add_keyframe(np.zeros((w.image_size[1], w.image_size[0]), np.uint8), kps_array(xy), rng.integers(0, 256, (n, 32)).astype(np.uint8), np.eye(4))
    out["added"] = {"last": {k: v for k, v in m.last.items()}, "ids": [kf["id"] for kf in m.keyframes], "serials": list(m._kf_serials),
                    "lists": m.list_arrays(), "life": m.point_life()}
    out["state"] = m.export_state()
    return out


def test_an_absorbed_mapper_has_the_future_of_one_imported_from_the_restated_snapshot(tmp_path):
    from vslam_amd import snapshot as S
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    w = LW.loop_world()
    A, B = MW.split(w)
    mA, mB = A.build(ctx), B.build(ctx)
    a, b = mA.export_state(), mB.export_state()
    off = mA.absorb(mB)
    want = AR.absorb(a, b, len(A.points))
    _same(mA.export_state(), want, "absorbed loop world")
    assert off["kf_offset"] == 20 and off["point_offset"] == w.n_old and off["injected_offset"] == w.n_old and off["n_kf"] == 28
    # key for key the one-session world
    arr = mA.arrays()
    assert np.array_equal(arr["obs_kf"], w.obs_kf) and np.array_equal(arr["obs_kp"], w.obs_kp) and np.array_equal(arr["obs_off"], w.obs_off)
    assert [kf["id"] for kf in mA.keyframes] == list(range(28)) and mA._kf_serials == list(range(28)) and mA._next_serial == 28
    assert len(mA.map_points) == len(w.points) and mA.map_points[w.n_old + 3]["id"] == w.points[w.n_old + 3]["id"]
    _same(mB.export_state(), b, "src")
    # the twin: the absorbed mapper's host side from its file, the device map imported from the restated snapshot
    path = str(tmp_path / "absorbed.npz")
    mA.save_state(path)
    twin = LocalMapper.load_state(path, context=ctx)
    twin.lib.mo_map_destroy(twin._h)
    twin._h = S.import_map(twin.lib, ctx.h, want, (0, 0, 0, 0), twin._check)
    twin._cache = None
    twin._sync_size()
    _same(_future(twin, w), _future(mA, w), "future")
    assert ctx.dev_status() == 0
    for m in (mA, mB, twin):
        m.close()
    ctx.close()


# ---- loop candidates among a keyframe set ------------------------------------------------------------------------------------------------------
def _voc(ctx, words, weights):
    import vslam_amd as V
    return V.Vocabulary.from_arrays(words, weights, context=ctx)


def _equals_masked_restatement(m, kf_desc, words, weights, p, among, prep, a, **kw):
    r = AR.loop_candidates_among(kf_desc, a["obs_off"], a["obs_kf"], a["obs_kp"], words, weights, among, p, prepared=prep, **kw)
    d = m.loop_candidates(p, kw.get("min_weight", 15), kw.get("n_best", 10), kw.get("max_cand", 4), kw.get("ratio", 0.75),
                          among=None if among is None else np.asarray(among) != 0)
    c = d["candidates"]
    assert [x["pos"] for x in c] == r["cand"], (p, [x["pos"] for x in c], r["cand"])
    assert (d["n_found"], d["n_connected"], d["max_common"], d["n_scored"], d["n_passed"]) == \
        (r["n_found"], r["n_connected"], r["max_common"], r["n_scored"], r["n_passed"]), (p, d, r)
    assert d["connected"] == r["connected"] and [x["group"] for x in c] == r["group"]
    assert d["min_score"] == r["min_score"]                                        # == on the f64 values
    assert [x["acc"] for x in c] == r["acc"] and [x["score"] for x in c] == r["score"], (p, [x["acc"] for x in c], r["acc"])
    assert [x["n_match"] for x in c] == r["n_match"] and d["cur_point"].tolist() == r["cur_point"].tolist()
    for x, mp, mr in zip(c, r["match_point"], r["match_row"]):
        assert x["match_point"].tolist() == mp.tolist() and x["match_row"].tolist() == mr.tolist()
    return d, r


@pytest.mark.parametrize("n_kf", sorted(LW.TINY))
def test_masked_candidates_on_the_tiny_worlds(n_kf):
    from tests.test_gpu_loop import _same as same_answer
    ctx = _ctx()
    w = LW.tiny_world(n_kf)
    m = w.build(ctx)
    m.set_vocabulary(_voc(ctx, w.words, w.weights))
    a = m.arrays()
    prep = LR.prepared(w.kf_desc, a["obs_off"], a["obs_kf"], a["obs_kp"], w.words)
    rng = np.random.default_rng(n_kf)
    n_cand, n_changed = 0, 0
    for p in w.asking():
        plain = m.loop_candidates(p, LW.TINY_MIN_WEIGHT, 10, 4)
        same_answer(m.loop_candidates(p, LW.TINY_MIN_WEIGHT, 10, 4, among=None), plain)
        same_answer(m.loop_candidates(p, LW.TINY_MIN_WEIGHT, 10, 4, among=np.ones(n_kf, bool)), plain)
        same_answer(m.loop_candidates(p, LW.TINY_MIN_WEIGHT, 10, 4, among=np.arange(n_kf)), plain)
        for among, (n_best, max_cand) in ((rng.integers(0, 2, n_kf), (10, 4)), ((np.arange(n_kf) < n_kf // 2).astype(np.int64), (2, 16)),
                                          (rng.integers(0, 4, n_kf) == 0, (0, 1))):
            d, _ = _equals_masked_restatement(m, w.kf_desc, w.words, w.weights, p, np.asarray(among).astype(np.uint8), prep, a,
                                              min_weight=LW.TINY_MIN_WEIGHT, n_best=n_best, max_cand=max_cand)
            n_cand += len(d["candidates"])
            assert all(among[x["pos"]] for x in d["candidates"])
        n_changed += [x["pos"] for x in plain["candidates"]] != [x["pos"] for x in m.loop_candidates(p, LW.TINY_MIN_WEIGHT, 10, 4, among=rng.integers(0, 2, n_kf) == 1)["candidates"]]
    assert n_cand > 0 and n_changed > 0
    same_answer(m.loop_candidates(w.asking()[0], LW.TINY_MIN_WEIGHT, 10, 4), m.loop_candidates(w.asking()[0], LW.TINY_MIN_WEIGHT, 10, 4))   # a masked call leaves nothing behind
    with pytest.raises(ValueError):
        m.loop_candidates(0, among=np.ones(n_kf + 1, bool))
    with pytest.raises(IndexError):
        m.loop_candidates(0, among=[n_kf])
    m.close(); ctx.close()


def test_masked_candidates_on_the_loop_world_and_the_same_side_world():
    from tests.test_gpu_loop import STAGES, _same as same_answer
    ctx = _ctx()
    w = LW.loop_world()
    words, weights = LW.loop_vocabulary()
    m = w.build(ctx)
    m.set_vocabulary(_voc(ctx, words, weights))
    a = m.arrays()
    prep = LR.prepared(w.kf_desc, a["obs_off"], a["obs_kf"], a["obs_kp"], words)
    own = (np.arange(LW.N_KF) < MW.SPLIT).astype(np.uint8)
    for p in LW.RETURN_POS:
        plain = m.loop_candidates(p)
        same_answer(m.loop_candidates(p, among=np.ones(LW.N_KF, bool)), plain)
        d, _ = _equals_masked_restatement(m, w.kf_desc, words, weights, p, own, prep, a)
        assert d["candidates"] and all(x["pos"] < MW.SPLIT for x in d["candidates"])
        d, _ = _equals_masked_restatement(m, w.kf_desc, words, weights, p, 1 - own, prep, a)
        assert all(x["pos"] >= MW.SPLIT for x in d["candidates"])
    ctx.set_host_timing(True)
    m.loop_candidates(26, among=own != 0)
    i = STAGES.index("loop_select")
    assert [n for n, _ in ctx.stage_times()] == STAGES[:i] + ["loop_among"] + STAGES[i:]
    m.loop_candidates(26)
    assert [n for n, _ in ctx.stage_times()] == STAGES
    ctx.set_host_timing(False)
    m.close()
    # a same-side keyframe wins unmasked; the mask names the other side's keyframe
    hw = MW.same_side_world()
    hm = hw.build(ctx, _voc(ctx, hw.words, hw.weights))
    ha = hm.arrays()
    hp = LR.prepared(hw.kf_desc, ha["obs_off"], ha["obs_kf"], ha["obs_kp"], hw.words)
    d, _ = _equals_masked_restatement(hm, hw.kf_desc, hw.words, hw.weights, 3, None, hp, ha, **MW.SAME_SIDE_KW)
    assert [x["pos"] for x in d["candidates"]] == [2]
    d, _ = _equals_masked_restatement(hm, hw.kf_desc, hw.words, hw.weights, 3, np.array(MW.SAME_SIDE_AMONG, np.uint8), hp, ha, **MW.SAME_SIDE_KW)
    assert [x["pos"] for x in d["candidates"]] == [0]
    hm.close(); ctx.close()
