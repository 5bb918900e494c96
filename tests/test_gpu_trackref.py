"""Tracking against the reference keyframe on the device (map_trackref.hip) against its numpy restatement
(tests/trackref_restatement.py): every integer equal, the refined pose at the bound the tracker's refinement is held to."""
import numpy as np
import pytest

from tests import bow_restatement as B
from tests import bow_worlds as BW
from tests import track_restatement as TR
from tests import trackref_worlds as TW
from tests.map_worlds import flip, kps_array

pytestmark = pytest.mark.gpu

INTS = ("n_cand", "n_claims", "n_matches_raw", "n_matches", "n_inliers")


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _vocab(ctx, words, weights):
    import vslam_amd as V
    return V.Vocabulary.from_arrays(words, np.maximum(weights, 0).astype(np.int32), context=ctx)


def _integers_equal(res, r, tag=""):
    ok, pose, info = res
    for f in INTS:
        print(tag, f, info[f], r[f])
    for f in INTS:
        assert info[f] == r[f], (tag, f, info[f], r[f])
    for f in ("point", "dist", "kf_row"):
        assert np.array_equal(info[f], r[f]), (tag, f, np.flatnonzero(info[f] != r[f])[:8])
    assert info["hist"].tolist() == list(r["hist"]) and info["kept_bin"].tolist() == list(r["kept_bin"]), (tag, info["hist"], r["hist"], info["kept_bin"])
    assert np.array_equal(info["inlier"], r["inlier"]) and ok == r["ok"], (tag, ok, r["ok"])


def _bytes(res):
    ok, pose, info = res
    return (ok, pose.tobytes()) + tuple(np.asarray(info[f]).tobytes() for f in sorted(info) if f != "from_token")


def test_parity_on_the_reloc_world():
    ctx = _ctx()
    w = BW.reloc_world()
    m = TW.build_reloc(ctx)
    words, weights, _ = BW.vocabulary("reloc", 256)
    m.set_vocabulary(_vocab(ctx, words, weights))
    kps, d, T = TW.reloc_frame("near")
    r = TW.reloc_restated("near", 256)
    res = m.track_reference_keyframe(kps, d, kf_position=TW.KF)
    ok, pose, info = res
    _integers_equal(res, r, "reloc 256")
    q = np.flatnonzero(info["point"] >= 0)
    xyz = m.arrays()["xyz"]
    rp, rinl, rn = TR.refine(BW.K, w.poses[TW.KF], xyz[info["point"][q]].astype(np.float64), np.column_stack([kps["x"][q], kps["y"][q]]).astype(np.float64),
                             kps["octave"][q])
    assert np.array_equal(info["inlier"][q], rinl) and info["n_inliers"] == rn and not info["inlier"][info["point"] < 0].any()
    print("pose against the restatement", np.abs(pose - rp).max(), "against the truth", np.abs(pose - T).max())
    assert np.allclose(pose, rp, rtol=1e-9, atol=1e-9)
    assert np.abs(pose - T).max() < 1e-6
    assert ok and not info["from_token"]
    assert _bytes(res) == _bytes(m.track_reference_keyframe(kps, d, kf_position=TW.KF))
    ctx.set_host_timing(True)
    m.track_reference_keyframe(kps, d, kf_position=TW.KF)
    assert [n for n, _ in ctx.stage_times()] == ["trackref_words", "trackref_prep", "trackref_search", "trackref_orient", "trackref_refine"]
    ctx.set_host_timing(False)
    m.close(); ctx.close()


def test_a_resident_frame_gives_the_bytes_of_its_host_copies():
    """a frame extracted on the device against a one-keyframe map of its own rows: by its token and by host copies"""
    import vslam_amd as V
    from tests.helpers import synthetic_frame
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    img = synthetic_frame(20250523)
    (kps, desc), = ctx.orb_detect_compute(img, V.orb_params(nfeatures=500))
    kh, dh = np.array(kps).copy(), np.array(desc).copy()
    n = len(kh)
    assert n > 100
    m = LocalMapper(BW.K, save_every_keyframe=False, context=ctx, n_hyp=8)
    m.add_keyframe(img, kh, dh, np.eye(4))
    rng = np.random.default_rng(3)
    rows = np.arange(0, n, 2)
    z = rng.uniform(3.0, 8.0, len(rows))
    X = np.column_stack([(kh["x"][rows] - BW.K[0, 2]) / BW.K[0, 0] * z, (kh["y"][rows] - BW.K[1, 2]) / BW.K[1, 1] * z, z]).astype(np.float32)
    m.update_map_points([{"id": int(i), "position": X[i], "color": np.zeros(3, np.uint8), "observed_keyframes": {0: int(r)}} for i, r in enumerate(rows)])
    words, weights, _ = B.train(dh, np.array([0, n]), 32, 5)
    m.set_vocabulary(_vocab(ctx, words, np.full(32, 1024, np.int32)))
    assert V.resident_token(ctx, desc, kps)
    by_token = m.track_reference_keyframe(kps, desc, pose=BW.pose(BW.rot([0.0, 0.02, 0.0]), np.array([0.05, 0.0, 0.0])))
    by_host = m.track_reference_keyframe(kh, dh, pose=BW.pose(BW.rot([0.0, 0.02, 0.0]), np.array([0.05, 0.0, 0.0])))
    assert by_token[2]["from_token"] and not by_host[2]["from_token"]
    assert _bytes(by_token) == _bytes(by_host)
    _integers_equal(by_host, TW.restate_on_map(m, words, -1, kh, dh, pose0=BW.pose(BW.rot([0.0, 0.02, 0.0]), np.array([0.05, 0.0, 0.0]))), "resident")
    assert by_host[0] and by_host[2]["n_cand"] == len(rows) and by_host[2]["kept_bin"].tolist() == [0, -1, -1]
    assert np.abs(by_host[1] - np.eye(4)).max() < 1e-4   # (f32 points under an exact pose)
    m.close(); ctx.close()


def test_contrast_with_the_projection_tracker():
    ctx = _ctx()
    w = BW.reloc_world()
    m = TW.build_reloc(ctx)
    words, weights, _ = BW.vocabulary("reloc", 256)
    m.set_vocabulary(_vocab(ctx, words, weights))
    kps, d, T = TW.reloc_frame("far")
    ok, _, info = m.track_local_map(kps, d, w.poses[TW.KF])
    print("projection tracker from the keyframe's pose:", ok, info["pass_matches"])
    assert not ok
    res = m.track_reference_keyframe(kps, d, kf_position=TW.KF)
    _integers_equal(res, TW.reloc_restated("far", 256), "far")
    ok, pose, info = res
    print("reference keyframe:", ok, info["n_matches"], info["n_inliers"], np.abs(pose - T).max())
    assert ok and info["n_inliers"] >= 800 and np.abs(pose - T).max() < 1e-6
    ok2, pose2, info2 = m.track_local_map(kps, d, pose)
    print("projection tracker from that pose:", ok2, info2["pass_matches"], info2["pass_inliers"])
    assert ok2
    m.close(); ctx.close()


@pytest.mark.parametrize("n_words,rows,n_extra", [(2, 70, 110), (100, 70, 10), (64, 1100, -1)])
def test_small_shapes_equal_the_restatement(n_words, rows, n_extra):
    """W = 2: buckets longer than a wavefront; W = 100: no multiple of 64, empty words; 1100 rows against 1100: more than one round of
    1024 in the sort and the compaction.  Then the edges of the call on the same map."""
    import vslam_amd as V
    ctx = _ctx()
    w = TW.SmallWorld(3, rows, seed=rows + n_words, bare=True)
    words, weights, _ = w.vocabulary(n_words)
    m = w.build(ctx, capacity=(4, 64, 16, 32))
    m.set_vocabulary(_vocab(ctx, words, weights))
    for k in (1, 0):
        T = w.poses[k] @ BW.pose(BW.rot([0.01, -0.02, 0.4]), np.array([0.05, 0.02, -0.03]))
        kps, d = w.query(k, T, n_extra=n_extra)
        lengths = np.bincount(B.quantise(d, words), minlength=n_words)
        print("frame rows %d, longest bucket %d, empty words %d" % (len(d), lengths.max(), (lengths == 0).sum()))
        assert (n_words != 2 or lengths.max() > 64) and (n_words != 100 or (lengths == 0).any()) and (rows < 1024 or len(d) == rows)
        r = TW.restate_on_map(m, words, k, kps, d)
        res = m.track_reference_keyframe(kps, d, kf_position=k)
        _integers_equal(res, r, "W %d rows %d kf %d" % (n_words, rows, k))
        assert r["n_matches_raw"] > 10 and np.allclose(res[1], r["pose"], rtol=1e-9, atol=1e-9)
        if r["ok"]:
            assert np.abs(res[1] - T).max() < 1e-5
        # the same call by the position counted from the end
        assert _bytes(res) == _bytes(m.track_reference_keyframe(kps, d, kf_position=k - w.n_kf))
        # without the orientation stage
        r0 = TW.restate_on_map(m, words, k, kps, d, check_orientation=False)
        res0 = m.track_reference_keyframe(kps, d, kf_position=k, check_orientation=False)
        _integers_equal(res0, r0, "no orientation")
        assert res0[2]["n_matches"] == res0[2]["n_matches_raw"] and res0[2]["hist"].sum() == 0 and res0[2]["kept_bin"].tolist() == [-1, -1, -1]
    if rows == 1100:
        assert (res[2]["point"][1024:] >= 0).any()
    # the last keyframe observes nothing: no candidate, not ok, not an error
    ok, pose, info = m.track_reference_keyframe(kps, d, kf_position=-1)
    assert not ok and info["n_cand"] == 0 and info["n_matches"] == 0 and (info["point"] == -1).all() and (info["kf_row"] == -1).all()
    assert pose.tobytes() == np.asarray(m.keyframes[-1]["pose"], np.float64).tobytes()
    # an empty frame
    ok, pose, info = m.track_reference_keyframe(np.zeros(0, V.KP_DTYPE), np.zeros((0, 32), np.uint8), kf_position=0)
    assert not ok and info["n_cand"] == 0 and len(info["point"]) == 0
    # positions out of range
    for bad in (w.n_kf, -w.n_kf - 1):
        with pytest.raises(IndexError):
            m.track_reference_keyframe(kps, d, kf_position=bad, pose=np.eye(4))
    with pytest.raises(V.NativeError) as e:
        m.track_reference_keyframe(kps, d, kf_position=0, scale_factor=0.0)
    assert e.value.code == V.MO_ERR_ARG
    m.close(); ctx.close()


def test_keypoints_without_angles():
    ctx = _ctx()
    w = TW.SmallWorld(3, 70, seed=11)
    words, weights, _ = w.vocabulary(16)
    m = w.build(ctx, angles=False)
    m.set_vocabulary(_vocab(ctx, words, weights))
    T = w.poses[2] @ BW.pose(BW.rot([0.01, -0.02, 0.4]), np.array([0.05, 0.02, -0.03]))
    kps, d = w.query(2, T, angles=False)
    assert (kps["angle"] == -1).all() and (m.keyframes[2]["keypoints"]["angle"] == -1).all()
    res = m.track_reference_keyframe(kps, d, check_orientation=False)
    _integers_equal(res, TW.restate_on_map(m, words, -1, kps, d, check_orientation=False), "angle -1")
    assert res[0] and res[2]["n_matches"] == res[2]["n_matches_raw"] > 15
    m.close(); ctx.close()


def test_words_are_kept_by_slot():
    """a keyframe wider than the store's stride, then erase_keyframes([1]): the words of every keyframe equal the quantisation, and a call
    against the last keyframe equals the restatement on the map as it stands"""
    ctx = _ctx()
    w = TW.SmallWorld(3, 70, seed=7)
    words, weights, _ = w.vocabulary(100)
    m = w.build(ctx, capacity=(2, 80, 16, 32))
    m.set_vocabulary(_vocab(ctx, words, weights))

    def words_equal(tag):
        for k, kf in enumerate(m.keyframes):
            got = m.keyframe_words(k)
            assert got.dtype == np.int32 and np.array_equal(got, B.quantise(kf["descriptors"], words)), (tag, k)
        assert np.array_equal(m.keyframe_words(-1), m.keyframe_words(len(m.keyframes) - 1))

    words_equal("built")
    T = w.poses[2] @ BW.pose(BW.rot([0.01, -0.02, 0.4]), np.array([0.05, 0.02, -0.03]))
    kps, d = w.query(2, T)
    first = m.track_reference_keyframe(kps, d, kf_position=2)
    _integers_equal(first, TW.restate_on_map(m, words, 2, kps, d), "before")
    rng = np.random.default_rng(4)
    wide = rng.integers(0, 256, (200, 32)).astype(np.uint8)      # 200 rows > the stride of 80: the store is restrided
    img = np.zeros((BW.H_IMG, BW.W_IMG), np.uint8)
    m.add_keyframe(img, TW.with_angles(rng.uniform(0, 400, (200, 2)), TW.uniform_angles(rng, 200)), wide, np.eye(4))
    words_equal("restrided")
    more = rng.integers(0, 256, (50, 32)).astype(np.uint8)       # a fifth keyframe: the store gains slots, the database regrows
    m.add_keyframe(img, TW.with_angles(rng.uniform(0, 400, (50, 2)), TW.uniform_angles(rng, 50)), more, np.eye(4))
    words_equal("regrown")
    assert len(m.map_points) == len(w.obs)                       # (the keyframes' culls kept every point)
    assert _bytes(first) == _bytes(m.track_reference_keyframe(kps, d, kf_position=2))
    m.erase_keyframes([1])
    words_equal("erased")
    after = m.track_reference_keyframe(kps, d, kf_position=1)     # keyframe 2 moved to position 1; its points lost keyframe 1's observations
    _integers_equal(after, TW.restate_on_map(m, words, 1, kps, d), "after the erase")
    assert np.array_equal(after[2]["point"], first[2]["point"])
    last = m.track_reference_keyframe(kps, d, kf_position=-1)
    _integers_equal(last, TW.restate_on_map(m, words, -1, kps, d), "the last keyframe")
    with pytest.raises(IndexError):
        m.keyframe_words(len(m.keyframes))
    m.close(); ctx.close()


def test_scratch_poison_and_a_map_left_alone():
    from tests.test_gpu_scratch_poison import _map_state, _set
    ctx = _ctx()
    w = TW.SmallWorld(3, 300, seed=13)
    words, weights, _ = w.vocabulary(64)
    m = w.build(ctx)
    m.set_vocabulary(_vocab(ctx, words, weights))
    T = w.poses[1] @ BW.pose(BW.rot([0.01, -0.02, 0.4]), np.array([0.05, 0.02, -0.03]))
    kps, d = w.query(1, T, n_extra=40)
    before = _map_state(m)
    ref = m.track_reference_keyframe(kps, d, kf_position=1)
    assert ref[0] and _bytes(ref) == _bytes(m.track_reference_keyframe(kps, d, kf_position=1))
    for byte in (0x00, 0xA5, 0xFF):
        _set(ctx, byte)
        assert _bytes(ref) == _bytes(m.track_reference_keyframe(kps, d, kf_position=1)), byte
        assert _bytes(ref) == _bytes(m.track_reference_keyframe(kps, d, kf_position=1)), byte
        assert np.array_equal(m.keyframe_words(1), B.quantise(w.kf_desc[1], words))
    _set(ctx, -1)
    after = _map_state(m)
    assert all(np.array_equal(before["arrays"][f], after["arrays"][f]) for f in before["arrays"])
    assert all(np.array_equal(a, b) for a, b in zip(before["lists"], after["lists"]))
    m.close(); ctx.close()


def test_no_vocabulary_is_an_argument_error():
    import vslam_amd as V
    ctx = _ctx()
    w = TW.SmallWorld(3, 70, seed=7)
    m = w.build(ctx)
    kps, d = w.query(2, w.poses[2])
    for call in (lambda: m.track_reference_keyframe(kps, d), lambda: m.keyframe_words(0)):
        with pytest.raises(V.NativeError) as e:
            call()
        assert e.value.code == V.MO_ERR_ARG and "no vocabulary attached to the map" in str(e.value)
    m.close(); ctx.close()
