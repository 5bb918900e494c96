"""GPU tests of the result routes the benchmark does not take: the frame stream (stream.hip) in MODE_INIT, with want_matches / want_points,
with BGR and strided input, with a pair_index_base and with a final chunk of ONE frame behind its halo; the pair call (mo_pair_frontend)
on an empty frame and on a single train descriptor; the matcher once the caller has dropped the keypoints.  Every array a route hands
out is pinned to the per-pair device call, to the CPU oracle, or (MODE_TRACK map points, which no per-pair call returns) to one batched
call on the whole sequence; the map points are rebuilt in f64 from the stream's own pose as well.

The scene is small (7 frames of 320 x 240, ~ 475 keypoints each, n_hyp 256) and the CPU oracle alone clears the floors asserted per pair
(>= 333 ratio survivors, >= 292 kept tracking matches, >= 37 pose inliers in both modes on every one of the six pairs): no comparison
below can pass on empty arrays.  chunk = 3 cuts the sequence into 3 + 3 + 1 frames."""
import ctypes as C
import gc
from unittest import mock

import numpy as np
import pytest

from tests.helpers import parallax_frames

pytestmark = pytest.mark.gpu
W, H, NFR, CHUNK, NFEAT, N_HYP = 320, 240, 7, 3, 500, 256
K = np.array([[160.0, 0, 160.0], [0, 160.0, 120.0], [0, 0, 1.0]])
TOL = 1e-4          # the project's bound on a map point against the f64 SVD (test_gpu_twoview.test_triangulate_points_matches_svd)
I32MAX = np.iinfo(np.int32).max


def _xy(k):
    return np.stack([k["x"], k["y"]], 1)


def _noised(frames, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.clip(frames.astype(np.float32) + rng.normal(0, 2.0, frames.shape), 0, 255).round().astype(np.uint8)


def _same(a, b):
    """bit-identical, NaN positions included"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@pytest.fixture(scope="module")
def scene():
    """frames + the CPU oracle's extraction, knn lists, ratio test and tracking filters of every consecutive pair (computed once)"""
    from oracle import geom_oracle as G
    from oracle import orb_oracle as O
    O.lib().orc_set_variant(0, 0)   # libstdc++ selection order, the device's default
    frames = _noised(parallax_frames(NFR, seed=5, w=W, h=H, bg_step=2, fg_step=4), 3)
    ext = [O.detect_and_compute(f, O.params(nfeatures=NFEAT)) for f in frames]
    pairs = []
    for i in range(NFR - 1):
        (k0, d0), (k1, d1) = ext[i], ext[i + 1]
        idx, dist = O.match_knn2(d0, d1)
        keep = O.ratio_test(idx, dist, 0.75)
        sq, st, sd = G.track_select(_xy(k0), _xy(k1), idx, dist, keep, W, H)
        assert keep.sum() >= 300 and len(sq) >= 250, i            # the floors are the oracle's own before they are anyone else's
        pairs.append(dict(idx=idx, dist=dist, keep=keep, sel=np.stack([sq, st], 1).astype(np.int32), sel_dist=sd.astype(np.int32)))
    return dict(frames=frames, ext=ext, pairs=pairs)


@pytest.fixture(scope="module")
def per_pair(scene):
    """reference 1: every frame through the single-frame call, every pair through ctx.pair_frontend(pair_index=i) in both modes"""
    import vslam_amd as V
    ctx = V.Context(device=0, max_w=W, max_h=H, max_batch=1)
    prm = V.orb_params(nfeatures=NFEAT)
    try:
        ext = [tuple(np.array(a) for a in ctx.orb_detect_compute(f, prm)[0]) for f in scene["frames"]]
        out = {}
        for mode in (V.MODE_INIT, V.MODE_TRACK):
            out[mode] = [ctx.pair_frontend(*ext[i], *ext[i + 1], mode, K, W, H, n_hyp=N_HYP, pair_index=i, want_matches=True)
                         for i in range(NFR - 1)]
    finally:
        ctx.close()
    out["ext"] = ext           # keys: MODE_INIT, MODE_TRACK -> the six pair results; "ext" -> the seven (keypoints, descriptors)
    return out


@pytest.fixture(scope="module")
def batched_track(scene):
    """reference 3: ONE mo_dev_frontend_batch call on all 7 frames in MODE_TRACK with d_points set -> points (6, cap, 3), pose mask (6, cap)"""
    import torch
    import vslam_amd as V
    from tests.test_gpu_frame_api import _batch     # the one place that fills a BatchIO for the tests
    cap = (NFEAT + 48 + 63) // 64 * 64      # FrameStream's default
    dev = torch.device("cuda", 0)
    nb = NFR
    o, b = _batch(torch, V, dev, scene["frames"], cap, N_HYP, K, W, H, 0.75)
    b["mask"] = torch.zeros((nb - 1, cap), dtype=torch.uint8, device=dev)
    o.mode = V.MODE_TRACK; o.thr_px = 1.0; o.disp_frac = 0.02; o.pair_index_base = 0      # the stream's MODE_TRACK defaults
    o.d_sel_idx = b["sel"].data_ptr(); o.d_sel_dist = b["seld"].data_ptr(); o.d_sel_n = b["seln"].data_ptr(); o.d_pose_mask = b["mask"].data_ptr()
    ctx = V.Context(device=0, max_w=W, max_h=H, max_batch=nb)
    try:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        prm = V.orb_params(nfeatures=NFEAT)
        ctx._check(ctx.lib.mo_dev_frontend_batch(ctx.h, C.byref(prm), C.byref(o)))
        torch.cuda.synchronize()
        assert ctx.dev_status() == 0
        return dict(counts=b["counts"].cpu().numpy(), pts=b["pts"].cpu().numpy(), mask=b["mask"].cpu().numpy().astype(bool))
    finally:
        ctx.close()


def _stream(mode, want_matches=False, want_points=False, copy=True, **kw):
    from vslam_amd.stream import FrameStream
    kw.setdefault("width", W); kw.setdefault("height", H)
    return FrameStream(K, chunk=CHUNK, n_features=NFEAT, mode=mode, n_hyp=N_HYP, want_matches=want_matches, want_points=want_points, copy=copy, **kw)


_runs = {}


def _full_run(scene, mode, want_matches, want_points):
    """the 7 frames through a copy=True stream, once per flag combination (the results are the caller's own and outlive the stream)"""
    key = (mode, bool(want_matches), bool(want_points))
    if key not in _runs:
        fs = _stream(mode, want_matches, want_points)
        try:
            _runs[key] = list(fs.run(scene["frames"]))
        finally:
            fs.close()
    return _runs[key]


def _raises_attr(p, name):
    with pytest.raises(AttributeError):
        getattr(p, name)
    assert name not in p


def _check_pair(i, p, kq, kt, mode, wm, wp, scene, per_pair, batched):
    """pair i = (frame i, frame i + 1) of a stream against the three references, the shape invariants and the f64 triangulation"""
    import vslam_amd as V
    from oracle import geom_oracle as G
    track = mode == V.MODE_TRACK
    have_knn = wm or not track
    ref, orc = per_pair[mode][i], scene["pairs"][i]
    nq = len(kq)
    assert p.pair_index == i and p.ok and p.n_inliers >= 20, i
    assert np.isfinite(p.R).all() and np.isfinite(p.t).all() and abs(np.linalg.det(p.R) - 1.0) < 1e-9
    assert ref["keep"].sum() >= 300 and len(ref["idx"]) == nq
    # ---- the knn lists: per-pair call and oracle, or absent
    if have_knn:
        assert p.keep.sum() >= 300, i
        for name in ("idx", "dist", "keep"):
            assert _same(p[name], ref[name]), (i, name, "per-pair call")
            assert _same(p[name], orc[name]), (i, name, "oracle")
    else:
        for name in ("idx", "dist", "keep"):
            _raises_attr(p, name)
    # ---- the mode's own results against the per-pair call (and the oracle's filters)
    assert _same(p.R, ref["R"]) and _same(p.t, ref["t"]), i
    if track:
        assert len(p.sel) >= 250, i
        for name in ("sel", "sel_dist", "inlier"):
            assert _same(p[name], ref[name]), (i, name, "per-pair call")
        assert _same(p.sel, orc["sel"]) and _same(p.sel_dist, orc["sel_dist"]), (i, "oracle filters")
        assert p.n_inliers == ref["n_inliers"] == int(p.inlier.sum())
        _raises_attr(p, "pose_mask")
        mask = np.zeros(nq, bool)
        mask[p.sel[p.inlier, 0]] = True                     # the recoverPose mask per QUERY keypoint
        assert _same(p._c.mask[p._j, :nq].view(bool), mask) and not p._c.mask[p._j, nq:].any(), (i, "the chunk's mask row")
        q, t = p.sel[p.inlier, 0], p.sel[p.inlier, 1]
    else:
        assert _same(p.pose_mask, ref["pose_mask"]) and p.n_inliers == ref["n_good"], i
        _raises_attr(p, "sel")
        mask = p.pose_mask
        assert not mask[~p.keep].any()
        q = np.flatnonzero(mask)
        t = p.idx[q, 0]
    assert int(mask.sum()) == p.n_inliers >= 20, i
    # ---- the map points
    if not wp:
        _raises_attr(p, "X")
        return None
    X = p.X
    assert X.shape == (nq, 3) and X.dtype == np.float32
    fin = np.isfinite(X).all(axis=1)
    assert _same(fin, mask) and np.isnan(X[~fin]).all() and int(fin.sum()) == p.n_inliers, (i, "finite exactly on the pose mask")
    if track:
        assert batched["counts"][i] == nq
        assert _same(X, batched["pts"][i, :nq]) and _same(batched["mask"][i, :nq], mask), (i, "batched call")
    else:
        assert _same(X, ref["X"]), (i, "per-pair call")
    # rebuilt in f64 from the stream's own pose (the pose is the SAME one: no conditioning tail of a pose difference enters)
    P1 = K @ np.hstack([np.eye(3), np.zeros((3, 1))])
    P2 = K @ np.hstack([p.R, p.t])
    X4 = G.triangulate(P1, P2, _xy(kq)[q].astype(np.float64), _xy(kt)[t].astype(np.float64))
    Xr = X4[:, :3] / X4[:, 3:4]
    err = np.linalg.norm(X[q].astype(np.float64) - Xr, axis=1) / np.linalg.norm(Xr, axis=1)
    print("pair %d mode %d: %d map points, depth %.2f .. %.2f, triangulation error max %.3e median %.3e"
          % (i, mode, len(q), Xr[:, 2].min(), Xr[:, 2].max(), err.max(), np.median(err)))
    assert err.max() < TOL, (i, float(err.max()))
    return float(err.max())


def _check_frames(got, per_pair, scene):
    assert [g.index for g in got] == list(range(NFR)) and got[0].pair is None
    for i, g in enumerate(got):
        assert len(g.keypoints) >= 400
        assert _same(g.keypoints, per_pair["ext"][i][0]) and _same(g.descriptors, per_pair["ext"][i][1]), i
        assert _same(g.keypoints, scene["ext"][i][0]) and _same(g.descriptors, scene["ext"][i][1]), (i, "oracle")


# ---- A. stream results against per-pair calls, the oracle and the batched call ------------------------------------------------------
CASES = [("track", 0, 1), ("track", 1, 0), ("track", 1, 1), ("init", 1, 1)]


@pytest.mark.parametrize("mode,wm,wp", CASES)
def test_stream_results_equal_per_pair_calls_oracle_and_batch(mode, wm, wp, scene, per_pair, batched_track):
    """copy=True: every result array of every pair of the stream - knn lists, ratio test, kept matches, pose, masks, map points - against
    ctx.pair_frontend(pair_index=i) bit for bit, against the oracle's matcher and filters bit for bit, MODE_TRACK map points against the
    batched call bit for bit; map points finite exactly on the recoverPose mask and within 1e-4 of the f64 SVD triangulation; the
    arrays that were not asked for are absent.  The last chunk is one frame behind its halo."""
    import vslam_amd as V
    m = V.MODE_TRACK if mode == "track" else V.MODE_INIT
    got = _full_run(scene, m, wm, wp)
    _check_frames(got, per_pair, scene)
    assert got[-1]._c.first_frame == NFR - 1 and len(got[-1]._c.npts) == 1        # 3 + 3 + 1: n_pairs == 1 in the last chunk
    for i in range(NFR - 1):
        _check_pair(i, got[i + 1].pair, got[i].keypoints, got[i + 1].keypoints, m, wm, wp, scene, per_pair, batched_track)


def test_stream_views_read_while_iterating(scene, per_pair, batched_track):
    """copy=False, MODE_TRACK without want_matches and with want_points: the arrays are views of the pinned result buffer, read while
    iterating - the map points must have been downloaded although the knn lists in front of which they once lay are not"""
    import vslam_amd as V
    fs = _stream(V.MODE_TRACK, 0, 1, copy=False)
    seen, last = 0, None
    try:
        for g in fs.run(scene["frames"]):
            k = np.array(g.keypoints)
            assert _same(k, per_pair["ext"][g.index][0]) and _same(g.descriptors, per_pair["ext"][g.index][1])
            if g.index:
                _check_pair(g.index - 1, g.pair, last, k, V.MODE_TRACK, 0, 1, scene, per_pair, batched_track)
            else:
                assert g.pair is None
            last = k
            seen += 1
    finally:
        fs.close()
    assert seen == NFR


# ---- B. input routes of the stream --------------------------------------------------------------------------------------------------
def _equal_track_runs(got, want, pairs):
    """keypoints, descriptors and every MODE_TRACK pair field of `got` == `want` (lists of FrameResult); pairs: [(row in got, row in want)]"""
    for a, b in pairs:
        assert _same(got[a].keypoints, want[b].keypoints) and _same(got[a].descriptors, want[b].descriptors), (a, b)
        p, r = got[a].pair, want[b].pair
        assert (p is None) == (r is None), (a, b)
        if r is None:
            continue
        assert p.ok and r.ok and len(p.sel) >= 250 and p.n_inliers == r.n_inliers >= 20
        for name in ("sel", "sel_dist", "inlier", "R", "t", "idx", "dist", "keep"):
            assert _same(p[name], r[name]), (a, b, name)


@pytest.fixture(scope="module")
def bgr_scene():
    """three differently noised copies of the scene as B, G, R (their gray is no single channel), and the dense channels=3 run on them"""
    import vslam_amd as V
    clean = parallax_frames(NFR, seed=5, w=W, h=H, bg_step=2, fg_step=4)
    bgr = np.stack([_noised(clean, 11 + c) for c in range(3)], axis=-1)
    fs = _stream(V.MODE_TRACK, 1, 0, channels=3)
    try:
        got = list(fs.run(bgr))
    finally:
        fs.close()
    return dict(frames=bgr, run=got)


def test_stream_bgr_frames_equal_the_per_frame_loop_on_gray(bgr_scene):
    """channels=3: the device's BGR -> gray in front of the batch; reference: the per-frame loop on the oracle's bgr2gray."""
    import vslam_amd as V
    from oracle import orb_oracle as O
    bgr, got = bgr_scene["frames"], bgr_scene["run"]
    gray = np.stack([O.bgr2gray(f) for f in bgr])
    assert all((gray != bgr[..., c]).mean() > 0.3 for c in range(3))
    assert [g.index for g in got] == list(range(NFR))
    ctx = V.Context(device=0, max_w=W, max_h=H, max_batch=1)
    prm = V.orb_params(nfeatures=NFEAT)
    try:
        last = None
        for i in range(NFR):
            (k, d), = ctx.orb_detect_compute(gray[i], prm)
            assert len(k) >= 400 and _same(got[i].keypoints, k) and _same(got[i].descriptors, d), i
            if last is not None:
                r = ctx.track_pair(last[0], last[1], k, d, W, H, K, n_hyp=N_HYP, pair_index=i - 1)
                p = got[i].pair
                assert p.ok and len(p.sel) >= 250 and p.n_inliers == r["n_inliers"] >= 20, i
                for name in ("sel", "sel_dist", "inlier", "R", "t"):
                    assert _same(p[name], r[name]), (i, name)
            last = (k, d)
    finally:
        ctx.close()


@pytest.mark.parametrize("form", ["array", "array_bgr", "iterator", "pixel_stride"])
def test_stream_strided_frames_equal_the_dense_run(form, scene, bgr_scene):
    """frames cut out of a (7, 250, 352[, 3]) parent that is 255 outside the window: a row or a frame read at the wrong stride puts
    white into the image and moves the corners.  array / array_bgr: chunks are slices of the view and reach mo_stream_submit with the
    view's own strides, uncopied - the only two forms that take submit's strided branch (one channel / three).  iterator: run() copies
    frame by frame into its own dense block, so submit sees a dense chunk; what is pinned is that the strided frames are READ rightly.
    pixel_stride: every second pixel of a double-width parent, which mo_stream_submit cannot describe - submit makes it contiguous.
    All equal the dense run bit for bit."""
    import vslam_amd as V
    bgr = form == "array_bgr"
    frames = bgr_scene["frames"] if bgr else scene["frames"]
    want = bgr_scene["run"] if bgr else _full_run(scene, V.MODE_TRACK, 1, 0)
    if bgr:
        parent = np.full((NFR, 250, 352, 3), 255, np.uint8)
        view = parent[:, 5:5 + H, 16:16 + W]
    elif form == "pixel_stride":
        parent = np.full((NFR, 250, 2 * 352), 255, np.uint8)
        view = parent[:, 5:5 + H, 32:32 + 2 * W:2]
    else:
        parent = np.full((NFR, 250, 352), 255, np.uint8)
        view = parent[:, 5:5 + H, 16:16 + W]
    view[...] = frames
    assert not view.flags.c_contiguous and np.array_equal(view, frames)
    fs = _stream(V.MODE_TRACK, 1, 0, channels=3 if bgr else 1)
    try:
        lib = fs.ctx.lib
        with mock.patch.object(lib, "mo_stream_submit", wraps=lib.mo_stream_submit) as spy:
            got = list(fs.run(iter(view) if form == "iterator" else view))
        strides = [(c.args[2], c.args[3], c.args[4]) for c in spy.call_args_list]
    finally:
        fs.close()
    if form == "array":          # (n, row stride, frame stride): the view's own; a chunk of one frame needs no frame stride
        assert strides == [(3, 352, 250 * 352), (3, 352, 250 * 352), (1, 352, 0)]
    elif bgr:
        assert strides == [(3, 3 * 352, 250 * 3 * 352), (3, 3 * 352, 250 * 3 * 352), (1, 3 * 352, 0)]
    else:
        assert strides == [(3, 0, 0), (3, 0, 0), (1, 0, 0)]
    assert [g.index for g in got] == list(range(NFR))
    _equal_track_runs(got, want, [(i, i) for i in range(NFR)])


def test_stream_pair_index_base(scene):
    """a stream that takes the sequence up at frame 2 with pair_index_base=2 equals pairs 2..5 of the full run bit for bit (the sampler is
    keyed by the global pair index), pair_index included; with base 0 the same frames count their pairs from 0"""
    import vslam_amd as V
    want = _full_run(scene, V.MODE_TRACK, 1, 0)
    got = {}
    for base in (2, 0):
        fs = _stream(V.MODE_TRACK, 1, 0, pair_index_base=base)
        try:
            got[base] = list(fs.run(scene["frames"][2:]))
        finally:
            fs.close()
        assert [g.index for g in got[base]] == list(range(NFR - 2)) and got[base][0].pair is None
        assert [g.pair.pair_index for g in got[base][1:]] == [base + j for j in range(NFR - 3)]
    assert [g.pair.pair_index for g in got[2][1:]] == [g.pair.pair_index for g in want[3:]] == [2, 3, 4, 5]
    _equal_track_runs(got[2], want, [(j, j + 2) for j in range(1, NFR - 2)])
    assert _same(got[2][0].keypoints, want[2].keypoints)
    for j in range(1, NFR - 2):   # base 0: other sampling streams, the same matches
        assert _same(got[0][j].pair.sel, want[j + 2].pair.sel) and got[0][j].pair.ok


# ---- C. pair and matcher routes -----------------------------------------------------------------------------------------------------
def test_matcher_after_the_keypoints_were_dropped(scene):
    """`_, des = orb.detect_and_compute(img)`: the descriptors still carry their token, the keypoint records are gone.  The matcher
    then takes the upload path: same matches as on copies, and the knn lists of the oracle."""
    import vslam_amd as V
    from orbslam2.extractor import ORBExtractor
    from orbslam2.matcher import DescriptorMatcher
    ex = ORBExtractor(n_features=NFEAT)
    kps, des1 = ex.detect_and_compute(scene["frames"][0])
    _, des2 = ex.detect_and_compute(scene["frames"][1])
    ctx = V.default_context()
    assert V.resident_token(ctx, des1, kps.array) and V.resident_token(ctx, des2)
    del kps, _
    gc.collect()
    assert V.resident_token(ctx, des1) and V.resident_token(ctx, des2)            # the descriptors are resident ...
    assert V._resident_kps(des1) is None and V._resident_kps(des2) is None        # ... their keypoint arrays are dead
    mt = DescriptorMatcher()
    a = [(m.queryIdx, m.trainIdx, m.distance) for m in mt.match(des1, des2)]
    b = [(m.queryIdx, m.trainIdx, m.distance) for m in mt.match(des1.copy(), des2.copy())]
    assert a == b and len(a) >= 300
    idx, dist, keep = ctx.match_knn2_ratio(des1, des2, 0.75)
    orc = scene["pairs"][0]
    assert _same(idx, orc["idx"]) and _same(dist, orc["dist"]) and _same(keep, orc["keep"])
    assert a == [(int(q), int(orc["idx"][q, 0]), float(orc["dist"][q, 0])) for q in np.flatnonzero(orc["keep"])]


@pytest.mark.parametrize("mode", ["init", "track"])
@pytest.mark.parametrize("empty", [(False, True), (True, False), (True, True)], ids=["n2=0", "n1=0", "both=0"])
def test_pair_frontend_on_an_empty_frame_returns_defined_arrays(mode, empty, per_pair):
    """matcher.py:57-61: an empty frame gives no matches.  Every array the pair call returns is then fully defined: no neighbour (-1 at
    INT32_MAX, what the matcher's own entry point gives), nothing kept, no map point, no pose."""
    import vslam_amd as V
    m = V.MODE_TRACK if mode == "track" else V.MODE_INIT
    none = (np.zeros(0, V.KP_DTYPE), np.zeros((0, 32), np.uint8))
    f1 = none if empty[0] else per_pair["ext"][0]
    f2 = none if empty[1] else per_pair["ext"][1]
    n1 = len(f1[0])
    assert n1 == 0 or n1 >= 400
    ctx = V.Context(device=0, max_w=W, max_h=H, max_batch=1)
    try:
        tok = (0, 0)
        for _ in range(2):   # (uploaded, then by the tokens under which the first call left the two frames resident)
            r = ctx.pair_frontend(*f1, *f2, m, K, W, H, n_hyp=N_HYP, want_matches=True, token1=tok[0], token2=tok[1])
            tok = (r["token1"], r["token2"])
            assert tok[0] and tok[1] and tok[0] != tok[1]
            assert r["idx"].shape == (n1, 2) and (r["idx"] == -1).all()
            assert r["dist"].shape == (n1, 2) and (r["dist"] == I32MAX).all()
            assert r["keep"].shape == (n1,) and r["keep"].dtype == bool and not r["keep"].any()
            assert np.isnan(r["R"]).all() and np.isnan(r["t"]).all()
            if mode == "init":
                assert r["X"].shape == (n1, 3) and np.isnan(r["X"]).all()
                assert r["pose_mask"].shape == (n1,) and not r["pose_mask"].any() and not r["ransac_mask"].any()
                assert r["n_good"] == 0
            else:
                assert len(r["sel"]) == 0 and len(r["sel_dist"]) == 0 and len(r["inlier"]) == 0 and r["n_inliers"] == 0
        if n1:   # the same through the matcher's own entry point
            idx, dist, keep = ctx.match_knn2_ratio(f1[1], np.zeros((0, 32), np.uint8), 0.75)
            assert _same(idx, r["idx"]) and _same(dist, r["dist"]) and _same(keep, r["keep"])
    finally:
        ctx.close()


def test_pair_frontend_matcher_only_on_one_train_descriptor(per_pair):
    """n2 == 1 through pair_frontend(MODE_INIT, n_hyp=0): no second neighbour (-1), every query kept as the ratio test of the reference
    keeps it; no two-view stage ran, so no map point: X all NaN, masks empty, no pose"""
    import vslam_amd as V
    from oracle import orb_oracle as O
    (k1, d1), (k2, d2) = per_pair["ext"][0], per_pair["ext"][1]
    eidx, edist = O.match_knn2(d1, d2[:1])
    ekeep = O.ratio_test(eidx, edist, 0.75)
    assert (eidx[:, 1] == -1).all() and (eidx[:, 0] == 0).all() and ekeep.all() and len(eidx) >= 400
    ctx = V.Context(device=0, max_w=W, max_h=H, max_batch=1)
    try:
        r = ctx.pair_frontend(k1, d1, k2[:1], d2[:1], V.MODE_INIT, K, W, H, n_hyp=0)
    finally:
        ctx.close()
    assert _same(r["idx"], eidx) and _same(r["dist"], edist) and _same(r["keep"], ekeep)
    assert r["X"].shape == (len(k1), 3) and np.isnan(r["X"]).all()
    assert not r["pose_mask"].any() and not r["ransac_mask"].any() and r["n_good"] == 0
    assert np.isnan(r["R"]).all() and np.isnan(r["t"]).all()
