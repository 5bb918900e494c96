"""The snapshot of the device map on the GPU: export -> import -> export gives equal bytes, a loaded mapper answers every call with the
bytes the original answers with and has the same future, a loaded map has shed its dead slots, a broken snapshot is refused, and the
file carries the vocabulary and the images."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _same(a, b, tag):
    from tests.test_gpu_scratch_poison import _flat, _same as same
    same(_flat(a), _flat(b), tag)


def _sizes(lib, h):
    s = (C.c_int64 * 6)()
    assert lib.mo_map_sizes(h, s) == 0
    return [int(v) for v in s]


def _round_trip(m, capacity=(0, 0, 0, 0), tag=""):
    """export -> import at `capacity` -> export: equal bytes in every array and in the dims; slots == keyframes on the imported map.
    Returns the first export."""
    from vslam_amd import snapshot as S
    a = m.export_state()
    h = S.import_map(m.lib, m.ctx.h, a, capacity, m._check)
    try:
        b = S.export_map(m.lib, h, m._check)
        sz = _sizes(m.lib, h)
    finally:
        m.lib.mo_map_destroy(h)
    _same(b, a, ("round trip", tag, capacity))
    assert sz[5] == sz[0] == len(m.keyframes) and sz[1] == len(m.map_points)
    assert m.ctx.dev_status() == 0
    return a


def _rand_kf(m, rng, rows, size=(64, 48)):
    from tests.map_worlds import kps_array
    img = rng.integers(0, 256, (size[1], size[0], 3)).astype(np.uint8)
    xy = np.column_stack([rng.uniform(0, size[0], rows), rng.uniform(0, size[1], rows)])
    m.add_keyframe(img, kps_array(xy), rng.integers(0, 256, (rows, 32)).astype(np.uint8), np.eye(4))


def _points(m):
    """every map_points[i] dict, its descriptor among the fields, in one form for a dict the mapper made and one a caller injected"""
    out = []
    for p in m.map_points:
        d = p.get("descriptor")
        out.append({"id": int(p.get("id", 0)), "position": np.asarray(p["position"], np.float64).reshape(3),
                    "color": np.asarray(p.get("color", (0, 0, 0))).reshape(-1)[:3].astype(np.uint8),
                    "observed_keyframes": sorted((int(k), int(v)) for k, v in p.get("observed_keyframes", {}).items()),
                    "descriptor": None if d is None else np.asarray(d, np.uint8).reshape(32)})
    return out


# ---- round trip --------------------------------------------------------------------------------------------------------------------------
_FEATURE_EXPORTS = {}


@pytest.mark.parametrize("poison", [-1, 171])
def test_round_trip_of_the_feature_world_after_every_feature_step(poison):
    """... and once more with the poison byte set: the same exports, byte for byte"""
    import vslam_amd as V
    from tests import loop_worlds as LW
    from vslam_amd import snapshot as S
    ctx = _ctx()
    try:
        ctx._check(ctx.lib.mo_dbg_set_poison(ctx.h, poison))
        w = LW.feature_world()
        m = w.build(ctx)
        voc = V.Vocabulary.from_arrays(w.words, w.weights, context=ctx)
        exports = [_round_trip(m, tag="built")]
        for name, fn in LW.feature_steps(m, w, voc):
            fn()
            exports.append(_round_trip(m, tag=name))
        d = dict(zip(S.DIM_NAMES, exports[-1]["dims"].tolist()))
        assert d["n_kf"] == 4 and d["kf_rows"] == 32 and d["n_pts"] > 0 and d["kf_stored"] == 4
        _FEATURE_EXPORTS[poison] = exports
        if len(_FEATURE_EXPORTS) == 2:
            _same(_FEATURE_EXPORTS[171], _FEATURE_EXPORTS[-1], "poisoned exports")
    finally:
        ctx._check(ctx.lib.mo_dbg_set_poison(ctx.h, -1))
        ctx.close()


def _dead_slot_map(ctx):
    """the stale world of tests/map_worlds (10 keyframes, two removed by mo_map_remove_keyframes behind the injected points: stale and
    negative keys), then one more erased by erase_keyframes (renumbered keys), life records moved by note_tracking, a device-trained
    vocabulary.  7 keyframes in 10 slots."""
    from tests.map_worlds import build_map, world
    w = world("stale")
    m = build_map(ctx, w)
    m._kf_serials = [s for i, s in enumerate(m._kf_serials) if i not in w.removed]   # (build_map's removal leaves the serials to the mapper)
    m.erase_keyframes([2])
    # (the erase rewrote every key: points whose keys are negative, name no keyframe or no row are injected behind it)
    m.update_map_points([{"id": 5000 + i, "position": np.array([0.1 * i, 0.0, 5.0]), "color": np.full(3, i, np.uint8),
                          "descriptor": np.full(32, i, np.uint8), "observed_keyframes": {-1: 3, 99: 0, 2: 100000, -9: 1, i % 7: i}} for i in range(9)])
    n = len(m.map_points)
    m.note_tracking(w.kf_poses[4], {"point": np.arange(0, n, 3), "inlier": np.arange(0, n, 3) % 2 == 0}, window=0, image_size=w.image_size)
    m.train_vocabulary(1024, iters=3)
    return w, m


def test_round_trip_with_dead_slots_stale_keys_injected_points_and_moved_life_records():
    ctx = _ctx()
    w, m = _dead_slot_map(ctx)
    life = m.point_life()
    a = m.arrays()
    assert _sizes(m.lib, m._h)[5] == 10 and len(m.keyframes) == 7
    assert (a["dref_kf"] < 0).all() and (a["obs_kf"] < 0).any() and (life["visible"] > 1).any() and (life["found"] > 1).any()
    for cap in ((0, 0, 0, 0), (64, 2048, 1 << 16, 1 << 17), (9, 333, 2001, 7000)):
        e = _round_trip(m, cap, "dead slots")
    assert e["kf_ord"].tolist() == [k for k in w.survivors if k != w.survivors[2]] and int(e["dims"][6]) == 10
    m.close(); ctx.close()


def test_round_trip_of_an_empty_map_one_keyframe_a_keyframe_of_0_rows_and_one_of_1100_rows():
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    rng = np.random.default_rng(5)
    K = np.array([[50.0, 0, 32.0], [0, 50.0, 24.0], [0, 0, 1.0]])
    m = LocalMapper(K, save_every_keyframe=False, context=ctx, n_hyp=8, capacity=(2, 16, 16, 32))
    e = _round_trip(m, tag="empty")
    assert e["dims"][:8].tolist() == [0] * 8 and e["obs_off"].tolist() == [0]
    _rand_kf(m, rng, 8)
    e = _round_trip(m, tag="one keyframe")
    assert e["kf_cnt"].tolist() == [8] and e["img1"].size == 64 * 48 * 3
    _rand_kf(m, rng, 0)
    _round_trip(m, tag="0 rows")
    _rand_kf(m, rng, 1100)
    for cap in ((0, 0, 0, 0), (5, 1500, 100, 100)):
        e = _round_trip(m, cap, "1100 rows")
    assert e["kf_cnt"].tolist() == [8, 0, 1100] and e["kf_kps"].shape == (1108,)
    m.close(); ctx.close()


# ---- refusal -----------------------------------------------------------------------------------------------------------------------------
def test_import_refuses_a_broken_snapshot_and_the_context_stays_usable():
    import vslam_amd as V
    from tests import loop_worlds as LW
    from vslam_amd import snapshot as S
    ctx = _ctx()
    w = LW.feature_world()
    m = w.build(ctx)
    good = m.export_state()

    def broken(edit):
        a = {k: v.copy() for k, v in good.items()}
        edit(a)
        s = S._struct_of(a)
        h = C.c_void_p(12345)
        rc = ctx.lib.mo_map_import(ctx.h, C.byref(s), 0, 0, 0, 0, C.byref(h))
        return rc, h.value, ctx.lib.mo_last_error(ctx.h).decode()

    def off_end(a):
        a["obs_off"][-1] += 1

    def id_at_bound(a):
        a["id"][3] = a["dims"][7]

    def negative_count(a):
        a["kf_cnt"][1] = -8
    for edit, text in ((off_end, "obs_off must start at 0"), (id_at_bound, "every id must lie in"), (negative_count, "kf_cnt must be >= 0")):
        rc, h, err = broken(edit)
        assert rc == V.MO_ERR_ARG and h is None and text in err, (rc, h, err)
    _round_trip(m, tag="behind the refusals")   # the next valid import on the same context works
    m.close(); ctx.close()


# ---- same answers, compaction, same future --------------------------------------------------------------------------------------------------
def _answers(m, w, tmp_path, name):
    from tests.map_worlds import perturbed_pose, stale_queries
    T, (kps, desc), pos, (qk, qd) = stale_queries(w)
    pose0 = perturbed_pose(T)
    m.set_output_path(str(tmp_path / (name + ".ply")))
    m.save_map()
    out = {"arrays": m.arrays(), "lists": m.list_arrays(), "life": m.point_life(), "points": _points(m),
           "keyframes": [{k: kf[k] for k in ("id", "keypoints", "descriptors", "pose", "map_points")} for kf in m.keyframes],
           "statistics": m.get_map_statistics(), "ply": np.frombuffer((tmp_path / (name + ".ply")).read_bytes(), np.uint8),
           "covisibility": m.covisibility(), "views": m.point_views(), "query": m.query_keyframes(qk, qd, 5),
           "relocalize": m.relocalize(qk, qd), "relocalize_pre": m.relocalize(qk, qd, preselect=3),
           "track": m.track_local_map(kps, desc, pose0, window=3), "track_all": m.track_local_map(kps, desc, pose0, window=0),
           "track_covisible": m.track_local_map(kps, desc, pose0, local="covisible", min_weight=1),
           "track_reference": m.track_reference_keyframe(kps, desc, kf_position=4, pose=pose0)}
    loop = m.loop_candidates(len(m.keyframes) - 1, min_weight=5, n_best=3, max_candidates=3)
    out["loop"] = loop
    out["sim3"] = m.compute_sim3(loop, n_hyp=32)
    return out


def test_a_loaded_mapper_gives_the_same_answers_has_no_dead_slots_and_the_same_future(tmp_path):
    from tests.map_worlds import kps_array
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    w, m = _dead_slot_map(ctx)
    path = str(tmp_path / "state.npz")
    m.save_state(path)
    l = LocalMapper.load_state(path, context=ctx)
    # compaction: slots == keyframes, the ordinal is the original's
    assert _sizes(m.lib, m._h)[5] == 10 and _sizes(l.lib, l._h)[5] == _sizes(l.lib, l._h)[0] == 7
    assert l.point_life()["now"] == m.point_life()["now"] == 9
    _same(l.export_state(), m.export_state(), "loaded export")
    # the vocabulary came with the file
    assert l.vocabulary is not None and np.array_equal(l.vocabulary.words, m.vocabulary.words) and np.array_equal(l.vocabulary.weights, m.vocabulary.weights)
    want = _answers(m, w, tmp_path, "original")
    assert want["track_all"][2]["pass_cand"][0] > 0 and len(want["query"][0]) > 0   # (the reads have something to read)
    _same(_answers(l, w, tmp_path, "loaded"), want, "same answers")
    assert l.keyframes[-1]["image"].tobytes() == m.keyframes[-1]["image"].tobytes() and all(kf["image"] is None for kf in l.keyframes[:-1])
    # the same future on both: a keyframe (no model on this world), the edits, a keyframe cull; then equal exports
    rng = np.random.default_rng(3)
    xy = np.column_stack([rng.uniform(5, 630, 120), rng.uniform(5, 470, 120)])
    desc = rng.integers(0, 256, (120, 32)).astype(np.uint8)
    img = rng.integers(0, 256, (480, 640), dtype=np.uint8)
    T = w.kf_poses[-1].copy()
    futures = []
    for x in (m, l):
        x.add_keyframe(img, kps_array(xy), desc, T)
        f = {"ba": x.bundle_adjust(window=4), "fuse": x.fuse_map_points(window=0), "grow": x.create_new_map_points(window=3),
             "cull_points": x.cull_map_points(), "cull_keyframes": x.cull_keyframes(min_weight=5),
             "life": x.point_life(), "covis_graph": sorted((p, q, n) for p, r in x.co_visibility_graph.items() for q, n in r.items() if n),
             "serials": list(x._kf_serials), "ids": [kf["id"] for kf in x.keyframes], "export": x.export_state(),
             "points": _points(x)}
        futures.append(f)
    _same(futures[1], futures[0], "same future")
    assert futures[0]["life"]["now"] == 10
    l.close(); m.close(); ctx.close()


def test_the_same_future_of_a_growing_map_with_a_dead_slot_and_every_image_in_the_file(tmp_path):
    """four keyframes of a camera moving sideways past a two-depth scene, whose growth steps find models (points coloured from the
    previous keyframe's BGR image); the second is erased, so the saved map has a dead slot and the loaded one has slot != ordinal from
    there on.  Saved with images="all".  On both, create_new_map_points and a fifth keyframe grow the same points: the pair's sampling
    stream, the colours, id_bound and born continue, and the new points' dref_kf is the ordinal of the keyframe their descriptor
    came from (3), which on the loaded map is not its slot (2)."""
    import vslam_amd as V
    from tests.helpers import parallax_frames
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    K = np.array([[320.0, 0, 320.0], [0, 320.0, 240.0], [0, 0, 1.0]])
    gray = parallax_frames(5, seed=31, bg_step=4, fg_step=8)   # 0.1 per frame along x: the layers stand at depths 8 and 4
    frames = [np.stack([g, 255 - g, g // 2], -1) for g in gray]
    poses = []
    for i in range(5):
        T = np.eye(4); T[0, 3] = -0.1 * i
        poses.append(T)
    prm = V.orb_params(nfeatures=1000)
    m = LocalMapper(K, save_every_keyframe=False, context=ctx, pair_index_base=5)
    feats = []
    for g in gray:
        (kps, desc), = ctx.orb_detect_compute(g, prm)
        feats.append((np.array(kps), np.array(desc)))
    for (kps, desc), fr, T in zip(feats[:4], frames, poses):
        m.add_keyframe(fr, kps, desc, T)
    assert len(m.map_points) > 20
    m.erase_keyframes([1])
    _round_trip(m, tag="grown")
    path = str(tmp_path / "all.npz")
    m.save_state(path, images="all", compressed=True)
    l = LocalMapper.load_state(path, context=ctx, capacity=(4, 100, 10, 10))
    assert _sizes(m.lib, m._h)[5] == 4 and _sizes(l.lib, l._h)[5] == 3 and l.export_state()["kf_ord"].tolist() == [0, 2, 3]
    assert all(a["image"].tobytes() == b["image"].tobytes() and a["image"].shape == b["image"].shape for a, b in zip(l.keyframes, m.keyframes))
    _same(_points(l), _points(m), "points of the grown map")
    out = []
    for x in (m, l):
        n0 = len(x.map_points)
        grow = x.create_new_map_points(window=0)
        grown_dref = x.arrays()["dref_kf"][n0:].copy()   # (the call appends its points behind the map's)
        x.add_keyframe(frames[4], feats[4][0], feats[4][1], poses[4])
        print("create_new_map_points made %d points, add_keyframe %d" % (grow["n_new"], x.last["n_new"]))
        out.append({"grow": grow, "grown_dref": grown_dref, "last": dict(x.last), "export": x.export_state(), "points": _points(x),
                    "life": x.point_life(),
                    "graph": sorted((p, q, n) for p, r in x.co_visibility_graph.items() for q, n in r.items() if n)})
    for o in out:   # on the original and on the loaded map alike: the ordinal, not the slot
        assert o["grow"]["n_new"] > 0 and len(o["grown_dref"]) == o["grow"]["n_new"] and (o["grown_dref"] == 3).all()
        assert o["last"]["n_new"] > 20 and (o["life"]["born"] == 4).any() and o["export"]["col"].any()
        assert (o["export"]["dref_kf"][o["export"]["life"][:, 2] == 4] == 3).all()   # born with keyframe 4: grown from keyframe 3's rows
    _same(out[1], out[0], "same future of the grown map")
    l.close(); m.close(); ctx.close()


def test_the_last_keyframe_dict_keeps_its_own_image_when_the_last_stored_keyframe_is_gone(tmp_path):
    """the device's current image belongs to the last keyframe ever stored; with that one erased, the loaded last keyframe dict still
    carries its own image, and the default image size survives the loss of every image"""
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    rng = np.random.default_rng(9)
    m = LocalMapper(np.array([[50.0, 0, 32.0], [0, 50.0, 24.0], [0, 0, 1.0]]), save_every_keyframe=False, context=ctx, n_hyp=8)
    for _ in range(3):
        _rand_kf(m, rng, 8)
    m.erase_keyframes([2])
    path = str(tmp_path / "s.npz")
    m.save_state(path)
    l = LocalMapper.load_state(path, context=ctx)
    e = m.export_state()
    assert e["img%d" % int(e["dims"][14])].tobytes() != m.keyframes[-1]["image"].tobytes()   # (the device's image is the erased keyframe's)
    assert l.keyframes[-1]["image"].tobytes() == m.keyframes[-1]["image"].tobytes()
    assert l.keyframes[0]["image"] is None and l._default_image_size() == m._default_image_size() == (64, 48)
    for x in (m, l):
        x.erase_keyframes([1])
    assert l.keyframes[-1]["image"] is None and l._default_image_size() == m._default_image_size() == (64, 48)
    _same(l.fuse_map_points(window=0), m.fuse_map_points(window=0), "fuse at the default image size")
    l.close(); m.close(); ctx.close()


def test_the_driver_saves_a_run_and_localises_the_next_in_it(tmp_path, capsys):
    """examples/run_frames.py --map --save-state, then a second run with --load-state --relocalize on the same sequence: it starts
    tracking without initialising and relocalises its first frame against the saved map"""
    from tests.test_gpu_dropin import _run_frames_module
    mod = _run_frames_module()
    state_file = str(tmp_path / "run.npz")
    state, poses, n_map = mod.main(["--max-frames", "14", "--keyframe-every", "4", "--map", str(tmp_path / "a.ply"), "--save-state", state_file])
    first = capsys.readouterr().out
    assert state == "TRACKING" and "state saved to " + state_file in first
    state, poses2, _ = mod.main(["--max-frames", "6", "--keyframe-every", "4", "--map", str(tmp_path / "b.ply"), "--load-state", state_file, "--relocalize"])
    second = capsys.readouterr().out
    assert state == "TRACKING" and "loaded " + state_file in second and "initialised" not in second
    assert "frame 0: relocalize " in second and len(poses2) >= 4, second


def test_detect_loop_continues_its_consistency_count_across_a_save(tmp_path):
    """the loop world asked at the first two return keyframes, saved, loaded; the other two asked on both: the loop is found at the last,
    which needs the groups remembered from before the save"""
    import vslam_amd as V
    from tests import loop_worlds as LW
    from tests.map_worlds import kps_array
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    lw = LW.loop_world()
    words, weights = LW.loop_vocabulary()
    m = lw.build(ctx)
    m.set_vocabulary(V.Vocabulary.from_arrays(words, weights, context=ctx))
    for p in LW.RETURN_POS[:2]:
        assert not m.detect_loop(p)[0]
    path = str(tmp_path / "loop.npz")
    m.save_state(path)
    l = LocalMapper.load_state(path, context=ctx)
    got = [[x.detect_loop(p) for p in LW.RETURN_POS[2:]] for x in (m, l)]
    assert [f for f, _ in got[0]] == [False, True]
    _same(got[1], got[0], "detect_loop behind a save")
    _same(l.query_keyframes(kps_array(lw.kf_xy[3]), lw.kf_desc[3], 5), m.query_keyframes(kps_array(lw.kf_xy[3]), lw.kf_desc[3], 5), "query")
    fresh = LocalMapper.load_state(path, context=ctx)
    fresh._loop_consistency = None
    assert [fresh.detect_loop(p)[0] for p in LW.RETURN_POS[2:]] == [False, False]   # (without the remembered groups the count starts again)
    fresh.close(); l.close(); m.close(); ctx.close()
