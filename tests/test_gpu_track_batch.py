"""LocalMapper.track_local_map_batch (mo_map_track_batch): every frame of a batch gets what track_local_map (mo_map_track) returns for it
alone on the same map - integers equal, doubles equal bit for bit - whatever the order and the company; the first frames also against
the numpy restatement (tests/track_restatement.py) and against known poses.

n_local is the one shared result: the batch forms one local map.  track_local_map reports n_local = 0 for a frame without keypoints
(it forms no local map for it), so that key is compared on the frames that have keypoints."""
import ctypes as C

import numpy as np
import pytest

from tests import track_restatement as TR
from tests.test_gpu_relocalize import K, _World, _ctx, _kps, _pose, _rot
from tests.test_gpu_track_map import _perturbed, _query, _restate, _same_pass

pytestmark = pytest.mark.gpu

RETRY_RADII = (1.0, 4.0, 4.0)   # test_retry_then_refine_over_three_passes' radii: a first pass at 1 px


def _odd(kps, desc):
    """the frame with a keypoint count that is no multiple of 64"""
    if len(kps) % 64 == 0:
        kps, desc = kps[:-1], desc[:-1]
    return np.ascontiguousarray(kps), np.ascontiguousarray(desc)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def _equal(one, batch, i, tag=""):
    """(ok, pose, info) of track_local_map against frame i of (ok, poses, infos) of track_local_map_batch: every array and scalar"""
    (o1, p1, i1), (ob, pb, ib) = one, batch
    ib = ib[i]
    assert bool(o1) == bool(ob[i]), (tag, i, "ok")
    assert np.array_equal(_bits(p1), _bits(pb[i])), (tag, i, "pose")
    assert sorted(i1) == sorted(ib), (tag, i, sorted(i1), sorted(ib))
    for f in ("point", "dist", "inlier"):
        assert i1[f].dtype == ib[f].dtype and np.array_equal(i1[f], ib[f]), (tag, i, f)
    for f in ("pass_radius", "pass_cand", "pass_matches", "pass_inliers", "n_pass_run", "from_token"):
        assert type(i1[f]) is type(ib[f]) and i1[f] == ib[f], (tag, i, f, i1[f], ib[f])
    assert np.array_equal(_bits(i1["pass_radius"]), _bits(ib["pass_radius"])), (tag, i, "pass_radius")
    assert len(i1["pass_pose"]) == len(ib["pass_pose"])
    for a, b in zip(i1["pass_pose"], ib["pass_pose"]):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (tag, i, "pass_pose")   # (NaN compares by its bits)
    if len(i1["point"]):
        assert i1["n_local"] == ib["n_local"], (tag, i, "n_local")


def _three(w, noise):
    """three frames at different poses, with different keypoint counts"""
    Ts = [w.poses[6] @ _pose(_rot([0.01, -0.02, 0.01]), np.array([0.1, -0.05, 0.05])),
          w.poses[3] @ _pose(_rot([-0.02, 0.01, 0.0]), np.array([-0.08, 0.03, 0.1])),
          w.poses[1] @ _pose(_rot([0.0, 0.02, -0.015]), np.array([0.05, 0.06, -0.04]))]
    frames = [_odd(*_query(w, T, noise=noise, seed=5 + 3 * i)) for i, T in enumerate(Ts)]
    ns = [len(k) for k, _ in frames]
    assert len(set(ns)) == 3 and all(n % 64 for n in ns), ns
    return Ts, frames, [_perturbed(T) for T in Ts]


def _five(w):
    """(frames, poses, roles) of the mixed batch, for RETRY_RADII: an empty frame, pure distractors, a frame whose first pass needs the
    retry (test_retry_then_refine_over_three_passes'), two ordinary frames that pass at the first radius"""
    import vslam_amd as V
    rng = np.random.default_rng(31)
    T_r = w.poses[4] @ _pose(_rot([0.01, 0.02, -0.01]), np.array([-0.05, 0.04, 0.06]))
    T_a = w.poses[6] @ _pose(_rot([0.01, -0.02, 0.01]), np.array([0.1, -0.05, 0.05]))
    T_b = w.poses[2] @ _pose(_rot([-0.01, 0.01, 0.02]), np.array([0.02, 0.05, -0.03]))
    n_d = 301
    distract = (_kps(np.column_stack([rng.uniform(0, 640, n_d), rng.uniform(0, 480, n_d)]).astype(np.float32)),
                rng.integers(0, 256, (n_d, 32)).astype(np.uint8))
    frames = [(np.zeros(0, V.KP_DTYPE), np.zeros((0, 32), np.uint8)),
              distract,
              _odd(*_query(w, T_r, seed=13)),
              _odd(*_query(w, T_a, seed=7)),
              _odd(*_query(w, T_b, noise=0.1, seed=17))]
    poses = [w.poses[0], w.poses[5],
             _pose(_rot([0.0, 0.003, 0.0]), np.zeros(3)) @ T_r,     # every projection ~1.5 px off: nothing within 1 px
             T_a,                                                    # exact: every true match within 1 px
             _pose(_rot([0.0, 0.0005, 0.0]), np.zeros(3)) @ T_b]    # ~0.25 px off
    assert len({len(k) for k, _ in frames}) == 5
    return frames, poses, ("empty", "distractors", "retry", "ordinary", "ordinary")


def _singles(m, frames, poses, **kw):
    return [m.track_local_map(k, d, T, **kw) for (k, d), T in zip(frames, poses)]


def _check_five(one, batch, poses):
    ok, Ts, infos = batch
    for i in range(5):
        _equal(one[i], batch, i, "five")
    print("n_pass_run %s, pass_radius %s, pass_matches %s, pass_inliers %s"
          % ([x["n_pass_run"] for x in infos], [x["pass_radius"] for x in infos], [x["pass_matches"] for x in infos],
             [x["pass_inliers"] for x in infos]))
    assert infos[0]["n_pass_run"] == 0 and not ok[0] and len(infos[0]["point"]) == 0
    assert infos[1]["n_pass_run"] == 1 and infos[1]["pass_radius"] == [2.0] and not ok[1]           # ended after the retry ...
    assert np.array_equal(_bits(Ts[1]), _bits(poses[1])) and np.array_equal(_bits(Ts[0]), _bits(poses[0]))   # ... and returned its pose0
    assert infos[2]["n_pass_run"] == 3 and infos[2]["pass_radius"] == [2.0, 4.0, 4.0] and ok[2]
    for i in (3, 4):                                                                                # its neighbours are ok
        assert ok[i] and infos[i]["pass_radius"] == [1.0, 4.0, 4.0], (i, infos[i]["pass_radius"])
    assert infos[0]["n_local"] == infos[3]["n_local"] > 0


def test_equal_to_the_restatement_and_the_truth():
    ctx = _ctx()
    w = _World(ctx)
    Ts, frames, pose0 = _three(w, noise=0.5)
    ok1, _, i1 = w.m.track_local_map_batch(frames, pose0, radii=(15.0,))
    ok2, P2, i2 = w.m.track_local_map_batch(frames, pose0)
    a = w.m.arrays()
    for i, (kps, desc) in enumerate(frames):
        r1 = _restate(w.m, kps, desc, pose0[i], radii=(15.0,), refine_pose=False)
        assert i1[i]["n_local"] == r1["n_local"]
        assert np.array_equal(i1[i]["point"], r1["passes"][0]["point"]) and np.array_equal(i1[i]["dist"], r1["passes"][0]["dist"])
        _same_pass(i1[i], r1["passes"][0], 0)
        info = i2[i]
        assert info["n_pass_run"] == 2 and np.array_equal(_bits(info["pass_pose"][0]), _bits(i1[i]["pass_pose"][0]))
        q = np.flatnonzero(info["point"] >= 0)
        ref, inl, n_inl = TR.refine(K, info["pass_pose"][0], a["xyz"][info["point"][q]].astype(np.float64),
                                    np.column_stack([kps["x"][q], kps["y"][q]]).astype(np.float64), kps["octave"][q])
        assert np.allclose(P2[i], ref, rtol=1e-9, atol=1e-9), P2[i] - ref
        assert np.array_equal(info["inlier"][q], inl) and info["pass_inliers"][1] == n_inl and ok2[i]
    _, clean, _ = _three(w, noise=0.0)
    ok0, P0, _ = w.m.track_local_map_batch(clean, pose0)
    for i in range(3):
        assert ok0[i] and np.abs(P0[i] - Ts[i]).max() < 1e-6, P0[i] - Ts[i]
    assert ctx.dev_status() == 0
    w.m.close(); ctx.close()


def test_equal_to_the_per_frame_call_order_and_company():
    ctx = _ctx()
    w = _World(ctx)
    frames, poses, _ = _five(w)
    one = _singles(w.m, frames, poses, radii=RETRY_RADII)
    batch = w.m.track_local_map_batch(frames, poses, radii=RETRY_RADII)
    _check_five(one, batch, poses)
    # the same frames reversed give the reversed results; a batch of one gives the per-frame result; a batch run twice gives equal bytes
    rev = w.m.track_local_map_batch(frames[::-1], poses[::-1], radii=RETRY_RADII)
    for i in range(5):
        _equal(one[i], rev, 4 - i, "reversed")
    for i in range(5):
        _equal(one[i], w.m.track_local_map_batch([frames[i]], [poses[i]], radii=RETRY_RADII), 0, "alone")
    again = w.m.track_local_map_batch(frames, poses, radii=RETRY_RADII)
    from tests.test_gpu_scratch_poison import _flat
    assert _flat(again) == _flat(batch)
    # [n][3][4] poses are the same call
    assert _flat(w.m.track_local_map_batch(frames, np.array(poses)[:, :3, :], radii=RETRY_RADII)) == _flat(batch)
    assert ctx.dev_status() == 0
    w.m.close(); ctx.close()


def test_mixed_sources():
    """one frame by the token of a resident extraction, one by host arrays"""
    import vslam_amd as V
    from tests.helpers import synthetic_frame
    ctx = _ctx()
    w = _World(ctx)
    T = w.poses[5] @ _pose(_rot([0.01, 0.0, -0.01]), np.array([0.03, 0.02, 0.04]))
    host = _odd(*_query(w, T, seed=23))
    (kps, desc), = ctx.orb_detect_compute(synthetic_frame(20250523), V.orb_params(nfeatures=500))
    assert V.resident_token(ctx, desc, kps) and len(kps) > 0
    frames, poses = [(kps, desc), host], [w.poses[2], _perturbed(T)]
    batch = w.m.track_local_map_batch(frames, poses)
    assert [x["from_token"] for x in batch[2]] == [True, False] and batch[0][1]
    one = _singles(w.m, frames, poses)
    assert one[0][2]["from_token"] and not one[1][2]["from_token"]
    for i in range(2):
        _equal(one[i], batch, i, "mixed")
    # the token frame by its host copies: the same bytes but for from_token
    kh, dh = np.array(kps).copy(), np.array(desc).copy()
    hb = w.m.track_local_map_batch([(kh, dh), host], poses)
    assert [x["from_token"] for x in hb[2]] == [False, False]
    assert np.array_equal(hb[2][0]["point"], batch[2][0]["point"]) and np.array_equal(_bits(hb[1]), _bits(batch[1]))
    assert ctx.dev_status() == 0
    w.m.close(); ctx.close()


def test_stride_and_bounds():
    import vslam_amd as V
    ctx = _ctx()
    w = _World(ctx)
    Ts, frames, pose0 = _three(w, noise=0.0)
    ref = w.m.track_local_map_batch(frames, pose0)
    nf, ns = 3, [len(k) for k, _ in frames]
    stride = max(ns) + 77

    def call(stride, nf=nf):
        refs = (V.FrameRef * 3)()
        keep = []
        for i, (k, d) in enumerate(frames):
            refs[i], _, arrays = w.m._frame_ref(k, d)
            keep.append(arrays)
        point = np.full((3, stride), -7, np.int32); dist = np.full((3, stride), -7, np.int32); inlier = np.full((3, stride), 7, np.uint8)
        pose = np.zeros((3, 12)); pass_pose = np.zeros((3, 4, 12)); pass_radius = np.zeros((3, 4))
        cand, matches, inliers = (np.zeros((3, 4), np.int32) for _ in range(3))
        n_run, ok, tok = (np.full(3, -7, np.int32) for _ in range(3))
        prm = V.MapTrackParams(640, 480, 10, 2, (C.c_double * 4)(15.0, 4.0, 0.0, 0.0), 1.2, 0.8, 5.991, 100, 20, 30)
        out = V.MapTrackBatchOut(stride, *[a.ctypes.data for a in (point, dist, inlier, pose, pass_pose, pass_radius, cand, matches, inliers, n_run,
                                                                   ok, tok)])
        Kc = np.ascontiguousarray(K, np.float64).reshape(9)
        p0 = np.ascontiguousarray(np.array(pose0)[:, :3, :]).reshape(3, 12)
        rc = w.m.lib.mo_map_track_batch(w.m._h, refs, nf, V._ptr(Kc), V._ptr(p0), C.byref(prm), C.byref(out))
        return rc, out, point, dist, inlier, pose, ok, n_run
    rc, out, point, dist, inlier, pose, ok, n_run = call(stride)
    assert rc == 0 and out.n_ok == 3 and out.n_local == ref[2][0]["n_local"]
    for i, n in enumerate(ns):   # the rows of each frame as the tight call gave them, the rows past n untouched
        assert np.array_equal(point[i, :n], ref[2][i]["point"]) and np.array_equal(dist[i, :n], ref[2][i]["dist"])
        assert np.array_equal(inlier[i, :n].astype(bool), ref[2][i]["inlier"])
        assert (point[i, n:] == -7).all() and (dist[i, n:] == -7).all() and (inlier[i, n:] == 7).all()
        assert np.array_equal(_bits(pose[i]), _bits(ref[1][i][:3, :].reshape(12)))
    # a frame of more rows than stride is refused and nothing is written; so is a batch beyond the maximum
    rc, out, point, dist, inlier, pose, ok, n_run = call(max(ns) - 1)
    assert rc == V.MO_ERR_ARG and (point == -7).all() and (ok == -7).all() and (n_run == -7).all()
    assert call(stride, nf=V.TRACK_BATCH_MAX + 1)[0] == V.MO_ERR_ARG and call(stride, nf=-1)[0] == V.MO_ERR_ARG
    bad = [p.copy() for p in pose0]; bad[1][0, 3] = np.inf
    with pytest.raises(V.NativeError):
        w.m.track_local_map_batch(frames, bad)
    with pytest.raises(V.NativeError):
        w.m.track_local_map_batch(frames, pose0, window=-1)
    # n_frames = 0: empty results, and through the C call nothing is touched
    rc, out, point, dist, inlier, pose, ok, n_run = call(stride, nf=0)
    assert rc == 0 and out.n_ok == 0 and out.n_local == 0 and (point == -7).all() and (ok == -7).all()
    ok0, P0, infos0 = w.m.track_local_map_batch([], [])
    assert ok0.shape == (0,) and P0.shape == (0, 4, 4) and infos0 == []
    # a map without keyframes, and one without points: no pass for any frame, not an error
    from vslam_amd.mapper import LocalMapper
    empty = LocalMapper(K, save_every_keyframe=False, context=ctx)
    for _ in range(2):
        e = empty.track_local_map_batch(frames[:2], pose0[:2])
        for i in range(2):
            _equal(empty.track_local_map(frames[i][0], frames[i][1], pose0[i]), e, i, "empty map")
            assert not e[0][i] and e[2][i]["n_pass_run"] == 0 and (e[2][i]["point"] == -1).all() and e[2][i]["n_local"] == 0
        empty.add_keyframe(np.zeros((480, 640), np.uint8), frames[0][0], frames[0][1], pose0[0])   # one keyframe, no map point
    assert ctx.dev_status() == 0
    empty.close(); w.m.close(); ctx.close()


def test_maps_that_changed():
    """a stale world with removed keyframes, then erase_keyframes: the batch reads the store's current copy"""
    from tests.map_worlds import build_map, perturbed_pose, pose_near, world
    ctx = _ctx()
    w = world("stale")
    m = build_map(ctx, w)
    Ts = [pose_near(w, 4), pose_near(w, 2, (0.0, 0.01, -0.01), (-0.05, 0.02, 0.03))]
    frames = [_odd(*w.track_query(T, seed=5 + i)) for i, T in enumerate(Ts)]
    pose0 = [perturbed_pose(T) for T in Ts]
    before = m.track_local_map_batch(frames, pose0)
    for i, one in enumerate(_singles(m, frames, pose0)):
        _equal(one, before, i, "stale")
    m.erase_keyframes([1])
    after = m.track_local_map_batch(frames, pose0)
    one = _singles(m, frames, pose0)
    for i in range(2):
        _equal(one[i], after, i, "erased")
    print("n_local %d -> %d, matches %s -> %s" % (before[2][0]["n_local"], after[2][0]["n_local"], [x["pass_matches"] for x in before[2]],
                                                  [x["pass_matches"] for x in after[2]]))
    assert all(x["pass_matches"][0] >= 20 for x in after[2])   # (nothing above compares empty results)
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_poison():
    """the mixed batch under two poison bytes, a fresh context and map each: the unpoisoned bytes, and the fill counters grow"""
    from tests.test_gpu_scratch_poison import _checked, _flat, _same, _set
    want = None
    for byte in (None, 255, 90):
        ctx = _ctx()
        if byte is not None:
            _set(ctx, byte)
        w = _World(ctx)
        frames, poses, _ = _five(w)
        got = _flat(_checked(ctx, lambda: w.m.track_local_map_batch(frames, poses, radii=RETRY_RADII), byte is not None))
        if want is None:
            want = got
        else:
            _same(got, want, (byte, "batch of five"))
            _same(_flat(_checked(ctx, lambda: w.m.track_local_map_batch(frames, poses, radii=RETRY_RADII), True)), want, (byte, "again"))
        assert ctx.dev_status() == 0
        w.m.close(); ctx.close()
