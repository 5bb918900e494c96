"""No result may depend on stale device memory.  mo_dbg_set_poison(ctx, byte) fills every block the library allocates and, at the start
of every entry point, every buffer the audit in NOTES.md classifies as scratch; every family of entry points is run once with poison
off on a fresh context and then under the bytes 255 (-1 as an int32, NaN as a float), 0 and 90, and every array and scalar it returns -
and, where a map is involved, every array of m.arrays() and m.list_arrays() - must keep its bytes.  No tolerance anywhere: the suite
already asserts run-to-run byte equality of these calls.  After every poisoned call mo_dbg_poison_filled must have grown: the poison
really got there.

Calls that only read a map reuse one context and one map for all four runs, so the poisoned calls also follow one another, a large
call in front of a small one; calls that change the map rebuild it from its world for each byte, under the poison.  The shapes are the
smallest of the existing tests that still reach each path."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests.helpers import parallax_frames, synthetic_frame

pytestmark = pytest.mark.gpu
BYTES = (255, 0, 90)
K_VGA = np.array([[320.0, 0, 320.0], [0, 320.0, 240.0], [0, 0, 1.0]])


def _ctx(w=640, h=480, batch=1):
    import vslam_amd as V
    return V.Context(device=0, max_w=w, max_h=h, max_batch=batch)


def _set(ctx, byte):
    ctx._check(ctx.lib.mo_dbg_set_poison(ctx.h, int(byte)))


def _filled(ctx):
    n, b = C.c_int64(-1), C.c_int64(-1)
    ctx._check(ctx.lib.mo_dbg_poison_filled(ctx.h, C.byref(n), C.byref(b)))
    return n.value, b.value


def _flat(x, path="r", out=None):
    """a result - nested dicts, lists, tuples, arrays, scalars - as a list of (path, bytes or value)"""
    out = [] if out is None else out
    if isinstance(x, dict):
        for k in sorted(x, key=str):
            _flat(x[k], "%s[%r]" % (path, k), out)
    elif isinstance(x, (list, tuple)):
        out.append((path + ".len", len(x)))
        for i, v in enumerate(x):
            _flat(v, "%s[%d]" % (path, i), out)
    elif isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        out.append((path, (str(a.dtype), a.shape, a.tobytes())))
    elif isinstance(x, (float, np.floating)):
        out.append((path, struct.pack("<d", float(x))))
    elif isinstance(x, np.generic):
        out.append((path, x.item()))
    else:
        out.append((path, x))
    return out


def _same(got, want, tag):
    assert [p for p, _ in got] == [p for p, _ in want], (tag, "the results differ in structure")
    for (p, a), (_, b) in zip(got, want):
        if a != b:
            where = ""
            if isinstance(a, tuple) and isinstance(b, tuple) and a[:2] == b[:2]:
                x, y = np.frombuffer(a[2], np.uint8), np.frombuffer(b[2], np.uint8)
                d = np.flatnonzero(x != y)
                where = "%d of %d bytes differ, the first at %d: %s for %s" % (len(d), len(x), d[0], x[d[:8]].tolist(), y[d[:8]].tolist())
            raise AssertionError("poison %r: %s moved (%s)" % (tag, p, where or "%r for %r" % (a, b)))


def _checked(ctx, fn, poisoned):
    """fn() with the fill totals read around it: they grow under poison and stay at zero without"""
    before = _filled(ctx)
    r = fn()
    after = _filled(ctx)
    if poisoned:
        assert after[0] > before[0] and after[1] > before[1], (before, after)
    else:
        assert before == after == (0, 0), (before, after)
    return r


def _sweep(make_ctx, calls, fresh):
    """calls [(name, fn(ctx))] in order on a fresh context with poison off, then under every byte: on a fresh context each (the plan and
    every work buffer are then allocated under the poison) or all on the first one (the buffers keep what the last call left)"""
    ctx = make_ctx()
    try:
        ref = [_flat(_checked(ctx, lambda: f(ctx), False)) for _, f in calls]
        for byte in BYTES:
            if fresh:
                ctx.close()
                ctx = make_ctx()
            _set(ctx, byte)
            for (name, f), want in zip(calls, ref):
                _same(_flat(_checked(ctx, lambda: f(ctx), True)), want, (byte, name))
            assert ctx.dev_status() == 0
    finally:
        ctx.close()


def _noised(frames, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.clip(frames.astype(np.float32) + rng.normal(0, 2.0, frames.shape), 0, 255).round().astype(np.uint8)


def _map_state(m):
    m._cache = None; m._lists = None
    return {"arrays": {f: v.copy() for f, v in m.arrays().items()}, "lists": [x.copy() for x in m.list_arrays()]}


# ---- the extractor ----------------------------------------------------------------------------------------------------------------------
def test_extractor_vga_both_select_orders():
    import vslam_amd as V
    frame = synthetic_frame(20250523)
    calls = [("nfeatures %d order %d" % (nf, order),
              lambda c, nf=nf, order=order: c.orb_detect_compute(frame, V.orb_params(nfeatures=nf, select_order=order)))
             for nf in (2000, 500) for order in (V.ORDER_LIBSTDCXX, V.ORDER_MSVC)]
    _sweep(_ctx, calls, fresh=True)


def test_extractor_noise_frame_dense_fallback():
    """the 320 x 200 noise frame of test_fast_nms_on_noise_uses_the_dense_fallback at threshold 0"""
    import vslam_amd as V
    rng = np.random.Generator(np.random.PCG64(99))
    img = rng.integers(0, 256, size=(200, 320), dtype=np.uint8)
    img[40:90, 100:260] = rng.integers(100, 104, size=(50, 160), dtype=np.uint8)
    p = V.orb_params(select_order=V.ORDER_LIBSTDCXX, fast_threshold=0, nlevels=3)
    calls = [("fast level %d" % L, lambda c, L=L: c.dbg_fast_level(img, p, L)) for L in range(3)]
    calls.append(("extract", lambda c: c.orb_detect_compute(img, p)))
    _sweep(_ctx, calls, fresh=True)


def test_extractor_full_hd_selection_in_hbm_scratch():
    """1920 x 1080 at (nfeatures, fast threshold) = (5000, 3): the one size whose selection replay leaves LDS for d_scratch"""
    import vslam_amd as V
    img = synthetic_frame(77, 1920, 1080)
    p = V.orb_params(nfeatures=5000, fast_threshold=3)
    _sweep(lambda: _ctx(1920, 1080), [("full hd", lambda c: c.orb_detect_compute(img, p))], fresh=False)


def _dev_extract(c, frames, prm, cap):
    import torch
    dev = torch.device("cuda", 0)
    fr = torch.from_numpy(frames).to(dev)
    nb, h, w = frames.shape
    kps = torch.zeros((nb, cap, 7), dtype=torch.float32, device=dev)
    desc = torch.zeros((nb, cap, 32), dtype=torch.uint8, device=dev)
    counts = torch.zeros(nb, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    c._check(c.lib.mo_dev_orb_detect_compute(c.h, C.byref(prm), fr.data_ptr(), w, h, nb, kps.data_ptr(), desc.data_ptr(), cap, counts.data_ptr()))
    torch.cuda.synchronize()
    assert c.dev_status() == 0
    n = counts.cpu().numpy()
    assert (n > 300).all() and (n <= cap).all(), n
    # (the rows behind a frame's count are the caller's own zeros: whatever the library wrote there would show too)
    return n, kps.cpu().numpy(), desc.cpu().numpy()


def test_extractor_other_routes():
    """the grid detector on the 3-px checkerboard (cells with more local maxima than one sort holds), descriptors at caller keypoints,
    a batch of three frames resident on the device, undistort"""
    import vslam_amd as V
    yy, xx = np.mgrid[0:236, 0:663]
    checker3 = (((yy // 3 + xx // 3) & 1) * 255).astype(np.uint8)
    frame = synthetic_frame(20250523)
    frames3 = parallax_frames(3, seed=5, w=320, h=240)
    prm = V.orb_params(nfeatures=500)
    given = _ctx()
    (k0, _), = given.orb_detect_compute(frame, prm)
    k0 = np.ascontiguousarray(k0[::3]).copy()
    given.close()
    assert len(k0) > 100 and len(set(k0["octave"].tolist())) > 3
    dist = np.array([-0.28, 0.07, 0.0008, -0.0004, 0.0])
    calls = [("grid detector", lambda c: c.grid_detect_compute(checker3, V.orb_params(nfeatures=2000), 2000, records=True)),
             ("grid corners", lambda c: c.grid_good_features(checker3, 2000)),
             ("compute at caller keypoints", lambda c: c.orb_compute(frame, prm, k0)),
             ("device batch of three", lambda c: _dev_extract(c, frames3, prm, 576)),
             ("undistort", lambda c: c.undistort(frame, K_VGA, dist))]
    _sweep(lambda: _ctx(672, 480, 3), calls, fresh=True)


# ---- the matcher ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["valu", "mfma"])
def test_matcher_sliced_unsliced_tiny_and_batched(kernel, monkeypatch):
    """(700, 1000) and (513, 129): few workgroups, the train set sliced through d_match_part; (17000, 300): not sliced; (5, 1); batched"""
    monkeypatch.setenv("VSLAM_AMD_MATCHER", kernel)
    rng = np.random.default_rng(17)
    sets = [(rng.integers(0, 256, (nq, 32), dtype=np.uint8), rng.integers(0, 256, (nt, 32), dtype=np.uint8))
            for nq, nt in ((700, 1000), (513, 129), (17000, 300), (5, 1))]
    sets.append((rng.integers(0, 256, (3, 300, 32), dtype=np.uint8), rng.integers(0, 256, (3, 200, 32), dtype=np.uint8)))
    calls = [("%s x %s" % (q.shape[:-1], t.shape[:-1]), lambda c, q=q, t=t: c.match_knn2_ratio(q, t, 0.75)) for q, t in sets]
    _sweep(_ctx, calls, fresh=True)


# ---- two-view stage and geometry --------------------------------------------------------------------------------------------------------
def test_two_view_and_geometry():
    import vslam_amd as V
    from oracle import geom_oracle as G
    s = G.synthetic_two_view(seed=4096, n=600)
    s20, s7 = G.synthetic_two_view(seed=11, n=20), G.synthetic_two_view(seed=12, n=7)
    t = s["t"].reshape(3)
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ s["R"]
    P1 = s["K"] @ np.hstack([np.eye(3), np.zeros((3, 1))])
    P2 = s["K"] @ np.hstack([s["R"], s["t"].reshape(3, 1)])
    a, b = _noised(parallax_frames(2, seed=31), 3)   # (two depths: the essential matrix of the pair is well posed)
    prm = V.orb_params(nfeatures=1000)

    def pair_steps(c):
        (k0, d0), = c.orb_detect_compute(a, prm)
        (k1, d1), = c.orb_detect_compute(b, prm)
        out = {"init": c.pair_frontend(k0, d0, k1, d1, V.MODE_INIT, K_VGA, 640, 480, n_hyp=256),                      # by tokens
               "track": c.pair_frontend(k0, d0, k1, d1, V.MODE_TRACK, K_VGA, 640, 480, n_hyp=256, want_matches=True),
               "track_pair": c.track_pair(k0.copy(), d0.copy(), k1.copy(), d1.copy(), 640, 480, K_VGA, n_hyp=256)}      # uploaded
        assert out["init"]["keep"].sum() >= 300 and len(out["track"]["sel"]) >= 100 and len(out["track_pair"]["sel"]) >= 100   # (no call compares empty lists)
        return {k: {f: v for f, v in r.items() if f not in ("token1", "token2")} for k, r in out.items()}   # (tokens count calls)

    calls = [("two-view (600, 512) staged", lambda c: c.init_two_view(s["p1"], s["p2"], s["K"], n_hyp=512, seed=77)),
             ("two-view (600, 300) plain", lambda c: c.init_two_view(s["p1"], s["p2"], s["K"], n_hyp=300, seed=77)),
             ("two-view (20, 1024)", lambda c: c.init_two_view(s20["p1"], s20["p2"], s20["K"], n_hyp=1024, seed=77)),
             ("two-view n = 7", lambda c: c.init_two_view(s7["p1"], s7["p2"], s7["K"], n_hyp=64, seed=77)),
             ("find_fundamental", lambda c: c.find_fundamental(s["p1"], s["p2"], n_hyp=512, seed=77)),
             ("recover_pose", lambda c: c.recover_pose(E, s["p1"], s["p2"], s["K"])),
             ("triangulate_points", lambda c: c.triangulate_points(P1, P2, s["p1"], s["p2"])),
             ("pair steps", pair_steps)]
    _sweep(_ctx, calls, fresh=True)


# ---- the frame stream and the batched front end -----------------------------------------------------------------------------------------
def test_frame_stream_track_mode():
    """6 frames of 320 x 240 in chunks of 4 (4 + 2 behind its halo) with want_points: the lanes' slabs are poisoned with the rest"""
    import vslam_amd as V
    from vslam_amd.stream import FrameStream
    frames = _noised(parallax_frames(6, seed=5, w=320, h=240, bg_step=2, fg_step=4), 3)
    Kq = np.array([[160.0, 0, 160.0], [0, 160.0, 120.0], [0, 0, 1.0]])

    def run(byte):
        fs = FrameStream(Kq, width=320, height=240, chunk=4, n_features=500, mode=V.MODE_TRACK, n_hyp=256, want_points=True)
        try:
            if byte is not None:
                _set(fs.ctx, byte)
            got = _checked(fs.ctx, lambda: list(fs.run(frames)), byte is not None)
            out = []
            for g in got:
                p = g.pair
                r = {"index": g.index, "keypoints": g.keypoints, "descriptors": g.descriptors}
                if p is not None:
                    r.update({k: p[k] for k in ("ok", "R", "t", "n_inliers", "pair_index", "sel", "sel_dist", "inlier", "X")})
                out.append(r)
            assert len(out) == 6 and all(r["ok"] and r["n_inliers"] >= 20 and len(r["sel"]) >= 100 for r in out[1:])
            return _flat(out)
        finally:
            fs.close()
    want = run(None)
    for byte in BYTES:
        _same(run(byte), want, (byte, "stream"))


def test_dev_frontend_batch():
    """one mo_dev_frontend_batch call on 4 frames in MODE_TRACK; every output array whole (rows nobody wrote are the caller's zeros)"""
    import torch
    import vslam_amd as V
    from tests.test_gpu_frame_api import _batch
    frames = _noised(parallax_frames(4, seed=5, w=320, h=240, bg_step=2, fg_step=4), 3)
    Kq = np.array([[160.0, 0, 160.0], [0, 160.0, 120.0], [0, 0, 1.0]])
    prm = V.orb_params(nfeatures=500)

    def run(c):
        dev = torch.device("cuda", 0)
        o, b = _batch(torch, V, dev, frames, 576, 256, Kq, 320, 240, 0.75)
        b["mask"] = torch.zeros((3, 576), dtype=torch.uint8, device=dev)
        o.mode = V.MODE_TRACK; o.thr_px = 1.0; o.disp_frac = 0.02; o.pair_index_base = 0
        o.d_sel_idx = b["sel"].data_ptr(); o.d_sel_dist = b["seld"].data_ptr(); o.d_sel_n = b["seln"].data_ptr(); o.d_pose_mask = b["mask"].data_ptr()
        torch.cuda.synchronize()
        c._check(c.lib.mo_dev_frontend_batch(c.h, C.byref(prm), C.byref(o)))
        torch.cuda.synchronize()
        assert c.dev_status() == 0
        r = {k: v.cpu().numpy() for k, v in b.items() if k != "fr"}
        assert (r["seln"] >= 100).all() and (r["npts"] >= 8).all(), (r["seln"], r["npts"])
        return r
    _sweep(lambda: _ctx(320, 240, 4), [("batch of four", run)], fresh=True)


# ---- map reads: one context, one map, four runs -------------------------------------------------------------------------------------------
def _read_sweep(ctx, maps, calls):
    """calls [(name, fn())] on maps that must not change: reference, then the three bytes, all on this context and these maps"""
    before = [_flat(_map_state(m)) for m in maps]
    ref = [_flat(_checked(ctx, f, False)) for _, f in calls]
    for byte in BYTES:
        _set(ctx, byte)
        for (name, f), want in zip(calls, ref):
            _same(_flat(_checked(ctx, f, True)), want, (byte, name))
        for m, b in zip(maps, before):
            _same(_flat(_checked(ctx, lambda: _map_state(m), True)), b, (byte, "the map itself"))
        assert ctx.dev_status() == 0
    _set(ctx, -1)


def test_map_reads_track_relocalize_query_covisibility():
    from tests.map_worlds import PRE_N, PRE_WORDS, build_map, clean_reloc_query, perturbed_pose, pose_near, world
    ctx = _ctx()
    w = world("clean")
    m = build_map(ctx, w)
    m.train_vocabulary(PRE_WORDS, 10)
    T = pose_near(w, 4)
    kps, desc = w.track_query(T)
    pose0 = perturbed_pose(T)
    small = np.arange(0, len(kps), len(kps) // 60)[:60]
    ks, ds = np.ascontiguousarray(kps[small]), np.ascontiguousarray(desc[small])
    rk, rd, _ = clean_reloc_query(3)
    seeds = np.arange(0, len(w.obs), 7)
    print("track queries of %d and %d keypoints, relocalization query of %d" % (len(kps), len(ks), len(rk)))
    assert len(kps) >= 1800 and len(ks) == 60
    calls = [("track %d keypoints, window 5" % len(kps), lambda: m.track_local_map(kps, desc, pose0, window=5)),
             ("track 60 keypoints, window 5", lambda: m.track_local_map(ks, ds, pose0, window=5, min_matches=5)),
             ("track %d keypoints, covisible" % len(kps), lambda: m.track_local_map(kps, desc, pose0, local="covisible")),
             ("track 60 keypoints, covisible", lambda: m.track_local_map(ks, ds, pose0, local="covisible", min_matches=5)),
             ("relocalize", lambda: m.relocalize(rk, rd)),
             ("relocalize preselected", lambda: m.relocalize(rk, rd, preselect=PRE_N)),
             ("query_keyframes", lambda: m.query_keyframes(rk, rd, PRE_N)),
             ("covisibility", lambda: m.covisibility()),
             ("local_keyframes", lambda: m.local_keyframes(seed_points=seeds, n_best=3, min_weight=1))]
    r = calls[0][1]()
    assert r[0] and r[2]["pass_inliers"][-1] >= 30 and calls[4][1]()[0]   # the reads find what they look for: nothing below compares empty results
    _read_sweep(ctx, [m], calls)
    m.close(); ctx.close()


def test_map_reads_covisibility_beyond_the_lds_bound():
    """the world of test_global_atomics_path_beyond_the_lds_bound: 129 keyframes, k_covis adds into the matrix in global memory"""
    from tests.map_worlds import kps_array
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    n_kf, rows = 129, 6
    rng = np.random.default_rng(12)
    m = LocalMapper(np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]]), save_every_keyframe=False, context=ctx)
    img = np.zeros((480, 640), np.uint8)
    for k in range(n_kf):
        m.add_keyframe(img, kps_array(rng.uniform(5, 470, (rows, 2))), rng.integers(0, 256, (rows, 32)).astype(np.uint8), np.eye(4))
    pts = []
    for i in range(400):
        o = {int(k): int(rng.integers(-rows - 1, rows + 2)) for k in rng.integers(-n_kf - 3, n_kf + 3, int(rng.integers(1, 7))).tolist()}
        pts.append({"id": i, "position": rng.uniform(-1, 1, 3), "observed_keyframes": o})
    m.update_map_points(pts)
    seeds = np.arange(0, 400, 3)
    calls = [("covisibility", lambda: m.covisibility()),
             ("local_keyframes", lambda: m.local_keyframes(seed_points=seeds, n_best=3, min_weight=1))]
    assert calls[0][1]().trace() > 400
    _read_sweep(ctx, [m], calls)
    m.close(); ctx.close()


def test_map_reads_loop_candidates_and_detect_loop():
    import vslam_amd as V
    from tests import loop_worlds as LW
    ctx = _ctx()
    tw = LW.tiny_world(70)
    tm = tw.build(ctx)
    tm.set_vocabulary(V.Vocabulary.from_arrays(tw.words, tw.weights, context=ctx))
    lw = LW.loop_world()
    words, weights = LW.loop_vocabulary()
    lm = lw.build(ctx)
    lm.set_vocabulary(V.Vocabulary.from_arrays(words, weights, context=ctx))

    def detect():
        lm._loop_consistency = None   # (the consistency bookkeeping is the mapper's own host state: every run starts it again)
        return [lm.detect_loop(p) for p in LW.RETURN_POS]
    calls = []
    for p in (69, 35):
        calls += [("tiny world %d (2, 16)" % p, lambda p=p: tm.loop_candidates(p, LW.TINY_MIN_WEIGHT, 2, 16)),
                  ("tiny world %d (0, 1)" % p, lambda p=p: tm.loop_candidates(p, LW.TINY_MIN_WEIGHT, 0, 1))]
    calls += [("loop world 26", lambda: lm.loop_candidates(26)), ("detect_loop", detect)]
    assert len(calls[4][1]()["candidates"]) > 0
    assert [f for f, _ in detect()] == [p == 26 for p in LW.RETURN_POS]
    _read_sweep(ctx, [tm, lm], calls)
    tm.close(); lm.close(); ctx.close()


# ---- map writes: the map rebuilt from its world for every byte, under the poison ---------------------------------------------------------
def _write_sweep(run):
    """run(ctx, call) builds the map and returns everything the calls returned and left; call(fn) wraps every library call"""
    ctx = _ctx()
    try:
        want = _flat(run(ctx, lambda fn: _checked(ctx, fn, False)))
        for byte in BYTES:
            _set(ctx, byte)
            _same(_flat(run(ctx, lambda fn: _checked(ctx, fn, True))), want, (byte, "map"))
            assert ctx.dev_status() == 0
    finally:
        ctx.close()


def test_map_writes_add_keyframe_growth_cull_removal_and_ply(tmp_path):
    """the first four survey keyframes from capacities (2, 16, 16, 32): every store regrows, under the poison; then the PLY, a keyframe
    removed, and the readers of the position table behind it"""
    import vslam_amd as V
    from tests.map_worlds import remove_keyframes
    from tests.test_gpu_mapper import K, _sequence
    from vslam_amd.mapper import LocalMapper
    frames, poses = _sequence()
    prm = V.orb_params(nfeatures=2000)

    def run(ctx, call):
        m = call(lambda: LocalMapper(K, output_path=str(tmp_path / "map.ply"), save_every_keyframe=False, context=ctx, capacity=(2, 16, 16, 32)))
        out = []
        for fr, T in zip(frames[:4], poses[:4]):
            (kps, desc), = call(lambda: ctx.orb_detect_compute(fr, prm))
            call(lambda: m.add_keyframe(fr, kps, desc, T))
            out.append({"last": dict(m.last), "map": _map_state(m)})
        assert len(m.map_points) > 20 and out[1]["last"]["n_new"] > 20
        call(m.save_map)
        out.append((tmp_path / "map.ply").read_bytes())
        remove_keyframes(m, [1])
        out.append({"covisibility": call(m.covisibility), "map": call(lambda: _map_state(m))})
        m.close()
        return out
    _write_sweep(run)


def test_map_writes_create_new_map_points():
    from tests import grow_worlds as GW
    from tests.map_worlds import build_map
    w, held = GW.withheld_points_world()

    def run(ctx, call):
        m = call(lambda: build_map(ctx, w))
        info = call(lambda: m.create_new_map_points(want_points=True, window=0))
        assert info["n_new"] > 20
        again = call(lambda: m.create_new_map_points(want_points=True, window=3))
        out = {"info": info, "again": again, "map": _map_state(m)}
        m.close()
        return out
    _write_sweep(run)


def test_map_writes_fuse_map_points():
    from tests import fuse_worlds as FW
    from tests.map_worlds import build_map
    w, unsplit, n_split = FW.split_world()

    def run(ctx, call):
        m = call(lambda: build_map(ctx, w))
        info = call(lambda: m.fuse_map_points(image_size=w.image_size, window=0))
        assert info["n_absorbed"] == n_split > 100
        again = call(lambda: m.fuse_map_points(image_size=w.image_size, window=0))   # nothing left to fuse: the call that writes nothing
        out = {"info": info, "again": again, "map": _map_state(m)}
        m.close()
        return out
    _write_sweep(run)


def test_map_writes_bundle_adjust_and_add_observations():
    from tests.ba_scene import Scene
    from tests.test_gpu_bundle_adjust import _mapper
    s = Scene()
    poses, xyz = s.perturbed()
    rng = np.random.default_rng(4)
    point = rng.integers(-5, len(s.X) + 5, 300).astype(np.int32)
    row = rng.integers(0, 50, 300).astype(np.int32)

    def run(ctx, call):
        m = call(lambda: _mapper(ctx, s, poses, xyz))
        ok, info = call(lambda: m.bundle_adjust(window=6, want_points=True))
        assert ok and info["n_free"] > 0 and sum(info["accepted"]) > 0
        out = {"ba": (ok, info), "kf_poses": [kf["pose"].copy() for kf in m.keyframes], "after ba": _map_state(m)}
        out["ba (0, 0)"] = call(lambda: m.bundle_adjust(window=6, max_steps=(0, 0), want_points=True))
        call(lambda: m.add_observations(4, point, row))
        call(lambda: m.add_observations(s.n_kf, point[::-1].copy(), row))
        out["after add_observations"] = _map_state(m)
        m.close()
        return out
    _write_sweep(run)


# ---- vocabulary training ------------------------------------------------------------------------------------------------------------------
def test_vocabulary_training_hand_cases():
    import vslam_amd as V
    from tests import bow_worlds as BW

    def train(c, case, W=None, iters=10):
        desc, off, W0 = case
        v = V.Vocabulary.train([desc[off[i]:off[i + 1]] for i in range(len(off) - 1)], W or W0, iters, context=c)
        r = (v.words.copy(), v.weights.copy(), v.iterations)
        v.close()
        return r
    calls = [("split", lambda c: train(c, BW.hand_split())), ("split, one iteration", lambda c: train(c, BW.hand_split(), iters=1)),
             ("split, none", lambda c: train(c, BW.hand_split(), iters=0)), ("as many words as rows", lambda c: train(c, BW.hand_split(), W=8)),
             ("duplicates", lambda c: train(c, BW.hand_duplicates()))]
    _sweep(_ctx, calls, fresh=False)


# ---- no map feature leaves the audit ------------------------------------------------------------------------------------------------------
# What one covisibility() fills under a poison byte on loop_worlds.feature_world: after covisibility alone, then after each further
# feature of feature_steps has run once.  Measured on the commit before the features registered themselves with the map (its library
# through VSLAM_AMD_LIB, this test printing the sequence); a feature that registers nothing, or one the fill walks past, changes a count.
# That sequence was [18, 30, 41, 68, 85, 94, 102, 120].  The step of bundle_adjust(window=4) was 27 buffers, all of BaBufs: 25 problem
# arrays (pout is not reserved without want_points), S and the result block.  Since the local and the global solver share one problem
# (BaProblem of csrc/ba_problem.h) it is 28, in two features: 25 - lpt (written and never read: deleted) + e_pt + fpos (the global
# solver's, which the one reserve of the problem brings; fpos is also where the free positions moved from the local result block) = 26
# in BaProblem, and S and the result block in BaBufs.  The observation edits left BaBufs for a feature of their own (map_obs.hip) that
# no step here calls.  So every count from the bundle adjustment on is one higher.
# The rebuilds share map_rebuild.h since: KfCullBufs lost ecnt and ebase (15 buffers -> 13), ObsEditBufs ao_cnt, ao_base and ao_total (10 -> 7);
# the map's kobs / obase and a word of the feature's result block stand in.  Neither feature is among the eight steps (the observation
# edits as said above, the keyframe cull never was), and the four arrays of the map were already filled from the first step on, so the
# list stands as it is: 18 + 0, 30 + 0, ... - measured again with the buffers gone, the same eight numbers.
FEATURE_FILLS = [18, 30, 41, 69, 86, 95, 103, 121]


def test_every_map_feature_joins_the_poison_fill():
    import vslam_amd as V
    from tests import loop_worlds as LW
    ctx = _ctx()
    w = LW.feature_world()
    m = w.build(ctx)
    voc = V.Vocabulary.from_arrays(w.words, w.weights, context=ctx)
    _set(ctx, 90)
    steps = LW.feature_steps(m, w, voc)
    assert [name for name, _ in steps][0] == "covisibility" and len(steps) == 8
    fills = []
    for name, fn in steps:
        fn()
        before = _filled(ctx)[0]
        m.covisibility()
        fills.append(_filled(ctx)[0] - before)
    print("buffers one covisibility() fills after each feature:", fills)
    assert all(b > a for a, b in zip(fills, fills[1:])), fills   # every feature added at least one buffer
    assert fills == FEATURE_FILLS
    assert ctx.dev_status() == 0
    m.close(); voc.close(); ctx.close()
