"""The device map's read paths - relocalize, track_local_map, bundle_adjust, add_observations - on maps whose keyframe position -> slot
table is not the identity (keyframes removed), with stale and negative observation keys, across octaves, image sizes and block
boundaries; each against its numpy restatement and, where the header defines the result by positions alone, byte for byte against the
twin map that never had the removed keyframes.  tests/test_map_worlds_cpu.py shows on the CPU that these worlds tell a kernel that
skips the table (or the octave gate, the radius scaling, the information weights, the tie rule) from one that does not.
Bounds: those of tests/test_gpu_relocalize.py, tests/test_gpu_track_map.py and tests/test_gpu_bundle_adjust.py for the same quantities;
the agreement measured on an MI355X is recorded in profiles/map_reads_parity.txt."""
import numpy as np
import pytest

from tests import track_restatement as TR
from tests.ba_restatement import add_observations as restate_add
from tests.map_worlds import (BA_STEPS, BA_WINDOW, PRE_N, PRE_QUERIES, PRE_WORDS, STALE_BA_STEPS, MapWorld, ba_case, ba_restated, build_map,
                              clean_reloc_query, clean_vocabulary, cull_after_ba, flip, kps_array, perturbed, perturbed_pose, pose_near, project,
                              stale_queries, track, world)
from tests.reloc_restatement import restate

pytestmark = pytest.mark.gpu

POSE_TRUTH = 1e-6            # noise-free pose against the truth: test_constructed_map of both the relocalization and the track tests
REFINE_TOL = dict(rtol=1e-9, atol=1e-9)   # device pose against TR.refine: tests/test_gpu_track_map.py


def _ctx(w=640, h=480):
    import vslam_amd as V
    return V.Context(device=0, max_w=max(w, 640), max_h=max(h, 480), max_batch=1)


def _map_is_the_world(m, w):
    a = m.arrays()
    for f in ("xyz", "obs_off", "obs_kf", "obs_kp"):
        assert np.array_equal(a[f], getattr(w, f)), f
    assert np.array_equal(a["id"], w.ids)
    assert all(np.array_equal(np.asarray(kf["descriptors"]), d) for kf, d in zip(m.keyframes, w.kf_desc))


def _snapshot(m):
    m._cache = None; m._lists = None
    return {f: v.copy() for f, v in m.arrays().items()}, [x.copy() for x in m.list_arrays()]


def _unchanged(m, snap):
    a, lists = _snapshot(m)
    assert all(np.array_equal(a[f], snap[0][f]) for f in a) and all(np.array_equal(x, y) for x, y in zip(lists, snap[1]))


def _reloc_equals_restatement(m, desc, info):
    a = m.arrays()
    r = restate(desc, [np.asarray(kf["descriptors"]) for kf in m.keyframes], a["obs_off"], a["obs_kf"], a["obs_kp"], 0.75, 4)
    assert [c[0] for c in info["candidates"]] == r["candidates"]
    assert [c[1] for c in info["candidates"]] == [r["scores"][p] for p in r["candidates"]]
    if info["kf_pos"] >= 0:
        qi, pi = r["C"][info["kf_pos"]]
        assert np.array_equal(np.flatnonzero(info["point"] >= 0), qi) and np.array_equal(info["point"][qi], pi)
        assert info["n_corr"] == len(qi)
    return r


def _same_reloc(a, b):
    from tests.test_gpu_relocalize import _same
    _same(a, b)
    assert a[2]["n_corr"] == b[2]["n_corr"] and a[2]["n_inliers"] == b[2]["n_inliers"]
    assert a[1] is None or a[1].tobytes() == b[1].tobytes()


def _same_track(a, b):
    from tests.test_gpu_track_map import _same
    _same(a, b)
    assert a[1].tobytes() == b[1].tobytes()


def _pass_equals(info, ps, k=0):
    assert info["pass_cand"][k] == ps["cand"] and info["pass_matches"][k] == ps["matches"] and info["pass_radius"][k] == ps["radius"], \
        (info["pass_cand"], ps["cand"], info["pass_matches"], ps["matches"], info["pass_radius"], ps["radius"])


def _track_checks(m, w, kps, desc, pose0, truth=None, first=(15.0,), **kw):
    """pass 1 alone and then the two default passes, as test_constructed_map of tests/test_gpu_track_map.py: integers equal to the
    restatement (pass 2 restated from the device's pass-1 pose), the final pose equal to the restated refinement of the device's
    matches.  Returns the two device results and the largest |pose - restated pose|."""
    size = w.image_size
    res1 = m.track_local_map(kps, desc, pose0, radii=first, image_size=size, **kw)
    i1 = res1[2]
    r1 = track(w, kps, desc, pose0, radii=first, refine_pose=False, **kw)
    assert i1["n_local"] == r1["n_local"]
    p1 = r1["passes"][0]
    assert np.array_equal(i1["point"], p1["point"]), int((i1["point"] != p1["point"]).sum())
    assert np.array_equal(i1["dist"], p1["dist"])
    _pass_equals(i1, p1)
    res = m.track_local_map(kps, desc, pose0, image_size=size, **kw)
    ok, pose, info = res
    mm = kw.get("min_matches", 20)
    assert info["pass_matches"][0] >= mm, info["pass_matches"]   # the call went on to pass 2: what follows is checked, never skipped
    assert info["n_pass_run"] == 2 and (first != (15.0,) or np.array_equal(info["pass_pose"][0], i1["pass_pose"][0]))
    r2 = track(w, kps, desc, pose0, poses=[pose0, info["pass_pose"][0]], refine_pose=False, **kw)
    p2 = r2["passes"][1]
    assert np.array_equal(info["point"], p2["point"]) and np.array_equal(info["dist"], p2["dist"])
    _pass_equals(info, p2, 1)
    assert p2["matches"] >= mm, p2["matches"]
    q = np.flatnonzero(info["point"] >= 0)
    ref, inl, n_inl = TR.refine(w.K, info["pass_pose"][0], w.xyz[info["point"][q]].astype(np.float64),
                                np.column_stack([kps["x"][q], kps["y"][q]]).astype(np.float64), kps["octave"][q],
                                scale_factor=kw.get("scale_factor", 1.2))
    d = float(np.abs(pose - ref).max())
    assert np.allclose(pose, ref, **REFINE_TOL), pose - ref
    assert np.array_equal(info["inlier"][q], inl) and not info["inlier"][info["point"] < 0].any()
    assert info["pass_inliers"][1] == n_inl == int(info["inlier"].sum())
    if truth is not None:
        assert ok and np.abs(pose - truth).max() < POSE_TRUTH, pose - truth
    return res1, res, d


def test_relocalize_after_removal():
    """(a) clean world, positions (1, 4) removed.  The header seeds the P3P sampling stream by (seed, keyframe POSITION, h) and
    k_reloc_hyp / k_reloc_refine pass the position: everything is defined by positions, so the twin must give the same bytes."""
    from tests.test_gpu_relocalize import _recheck
    ctx = _ctx()
    w = world("clean")
    m, twin = build_map(ctx, w), build_map(ctx, w, twin=True)
    _map_is_the_world(m, w); _map_is_the_world(twin, w)
    worst = 0.0
    for pos in (3, 6, 0):   # slots 5, 8, 0
        T = pose_near(w, pos, (0.02, -0.03, 0.01), (0.08, -0.05, 0.1))
        kps, desc = w.reloc_query(pos, T)
        snap = _snapshot(m)
        res = m.relocalize(kps, desc)
        ok, pose, info = res
        _reloc_equals_restatement(m, desc, info)
        assert ok and info["kf_pos"] == pos and info["kf_id"] == m.keyframes[pos]["id"] == pos, info["candidates"]
        worst = max(worst, float(np.abs(pose[:3] - T[:3]).max()))
        assert np.abs(pose[:3, :3] - T[:3, :3]).max() < POSE_TRUTH and np.abs(pose[:3, 3] - T[:3, 3]).max() < POSE_TRUTH, pose - T
        _recheck(type("W", (), {"m": m}), kps, info, pose)
        assert info["n_inliers"] == int(info["inlier"].sum()) >= 50
        _same_reloc(res, twin.relocalize(kps, desc))
        _unchanged(m, snap)
    print("relocalize after removal: largest |pose - truth| %.3g (bound %.3g)" % (worst, POSE_TRUTH))
    assert ctx.dev_status() == 0
    m.close(); twin.close(); ctx.close()


def test_relocalize_preselected_after_removal():
    """(a') the same world and queries with relocalize(preselect=3): the point_of table is indexed by POSITION and only the preselected
    keyframes are matched, on a map whose position -> slot table is not the identity.  The vocabulary (256 words: the true position
    ranks first, tests/test_map_worlds_cpu.py) is byte-equal on the map and its twin and equal to the restatement's; per query the
    ranking equals the restatement on both maps, the preselected call gives the same bytes on the map and on its twin, and its winner,
    counts, pose bytes and per-keypoint arrays are the plain call's, which still equals the relocalization's restatement."""
    from tests import bow_restatement as B
    ctx = _ctx()
    w = world("clean")
    m, twin = build_map(ctx, w), build_map(ctx, w, twin=True)
    v, vt = m.train_vocabulary(PRE_WORDS, 10), twin.train_vocabulary(PRE_WORDS, 10)
    words, weights, ran = clean_vocabulary()
    assert v.words.tobytes() == vt.words.tobytes() and v.weights.tobytes() == vt.weights.tobytes() and v.iterations == vt.iterations
    assert v.words.tobytes() == words.tobytes() and v.weights.tobytes() == weights.tobytes() and v.iterations == ran
    for pos in PRE_QUERIES:   # slots 5, 8, 0
        kps, desc, T = clean_reloc_query(pos)
        rpos, rsc = B.query(desc, w.kf_desc, words, weights, PRE_N)
        for mm in (m, twin):
            qp, qs = mm.query_keyframes(kps, desc, PRE_N)
            assert qp.tolist() == rpos and qs.tolist() == rsc, (qp.tolist(), rpos)
        assert pos in rpos
        snap = _snapshot(m)
        pre = m.relocalize(kps, desc, preselect=PRE_N)
        _same_reloc(pre, twin.relocalize(kps, desc, preselect=PRE_N))
        plain = m.relocalize(kps, desc)
        (ok, pose, info), (okp, posep, infop) = plain, pre
        assert ok and okp and infop["kf_pos"] == info["kf_pos"] == pos
        assert infop["n_corr"] == info["n_corr"] and infop["n_inliers"] == info["n_inliers"] and posep.tobytes() == pose.tobytes()
        assert np.array_equal(infop["point"], info["point"]) and np.array_equal(infop["inlier"], info["inlier"])
        assert set(c[0] for c in infop["candidates"]) <= set(rpos)
        _reloc_equals_restatement(m, desc, info)
        _unchanged(m, snap)
    assert ctx.dev_status() == 0
    m.close(); twin.close(); ctx.close()


def test_track_after_removal():
    """(b) the same world; windows 3 and 5 start between the removed slots and the end, 0 takes every position"""
    ctx = _ctx()
    w = world("clean")
    m, twin = build_map(ctx, w), build_map(ctx, w, twin=True)
    worst = 0.0
    for window, pos in ((3, 6), (5, 4), (0, 4)):
        T = pose_near(w, pos)
        kps, desc = w.track_query(T, wrong=0.0 if window else 0.1)
        pose0 = perturbed_pose(T)
        r1, r2, d = _track_checks(m, w, kps, desc, pose0, truth=T if window else None, window=window)
        worst = max(worst, d)
        assert r2[0] and r2[2]["pass_inliers"][1] >= 30
        _same_track(r1, twin.track_local_map(kps, desc, pose0, radii=(15.0,), window=window))
        _same_track(r2, twin.track_local_map(kps, desc, pose0, window=window))
    print("track after removal: largest |pose - restated refinement| %.3g" % worst)
    assert ctx.dev_status() == 0
    m.close(); twin.close(); ctx.close()


def test_bundle_adjust_after_removal_and_its_write_back():
    """(c) consecutive-keyframe world, positions (1, 5) removed, window 6: the fixed keyframes 1 - 3 and the free ones 4 - 9 all sit in
    slots that are not their positions.  The keyframe added afterwards culls with the P the bundle adjustment wrote: the survivors are
    those of the cull in numpy under the refined P of the free keyframes and the stored P of the rest."""
    from tests.test_gpu_bundle_adjust import PARITY_BOUND, _diff, _same_integers
    c = ba_case()
    w, poses, xyz, ref = c["w"], c["poses"], c["xyz"], c["ref"]
    ctx = _ctx()
    m, twin = build_map(ctx, w, poses=poses, xyz=xyz), build_map(ctx, w, twin=True, poses=poses, xyz=xyz)
    ok, info = m.bundle_adjust(window=BA_WINDOW, max_steps=BA_STEPS, want_points=True)
    _same_integers(info, ok, ref)
    d = _diff(info, ref)
    print("bundle adjustment after removal: steps %s accepted %s, largest difference to the restatement %.3g (bound %.3g)"
          % (info["steps"], info["accepted"], d, PARITY_BOUND))
    assert d <= PARITY_BOUND
    assert ok and info["free"] == ref["free"] and info["fixed"] == ref["fixed"]
    assert any(w.survivors[p] != p for p in info["free"]) and any(w.survivors[p] != p for p in info["fixed"])
    ok2, info2 = twin.bundle_adjust(window=BA_WINDOW, max_steps=BA_STEPS, want_points=True)
    assert ok2 == ok
    for k in info:
        assert np.array_equal(np.asarray(info[k]), np.asarray(info2[k]), equal_nan=True), k
    a, b = m.arrays(), twin.arrays()
    assert all(np.array_equal(a[f], b[f]) for f in a)
    for kf, kt in zip(m.keyframes, twin.keyframes):
        assert np.array_equal(kf["pose"], kt["pose"])
    # the write-back, through the next keyframe's cull
    dev = {"free": info["free"], "poses": info["poses"], "xyz": a["xyz"].copy()}
    keep, near = cull_after_ba(w, poses, dev, "slot")
    keep_none, _ = cull_after_ba(w, poses, dev, "none")
    keep_pos, _ = cull_after_ba(w, poses, dev, "position")
    assert near.sum() < 10 and (keep != keep_none).any() and (keep != keep_pos).any()
    rng = np.random.default_rng(3)
    W, H = w.image_size
    kp = kps_array(np.column_stack([rng.uniform(0, W, 200), rng.uniform(0, H, 200)]))
    for mm in (m, twin):
        mm.add_keyframe(np.zeros((H, W), np.uint8), kp, rng.integers(0, 256, (200, 32)).astype(np.uint8), w.kf_poses[-1])
        assert mm.last["n_new"] == 0
        got = np.isin(w.ids, mm.arrays()["id"])
        assert np.array_equal(got[~near], keep[~near]), int((got != keep).sum())
    print("cull after the write-back: %d of %d points kept (%d under the stored poses, %d with the write at kP[position])"
          % (keep.sum(), len(keep), keep_none.sum(), keep_pos.sum()))
    assert ctx.dev_status() == 0
    m.close(); twin.close(); ctx.close()


def test_add_observations_and_tracked_keyframe_after_removal():
    """(d) position 4 sits in slot 6; position n_kf names the next keyframe"""
    ctx = _ctx()
    w = world("ba")
    n, n_kf = len(w.obs), len(w.survivors)
    assert w.survivors[4] != 4
    rng = np.random.default_rng(4)
    point = rng.integers(-5, n + 5, 400).astype(np.int32)
    point[10] = point[3]
    have = np.array([i for i, o in enumerate(w.obs) if 4 in o][:40], np.int32)   # already observed at position 4: skipped
    point[50:50 + len(have)] = have
    row = rng.integers(0, 50, 400).astype(np.int32)
    for kf_pos in (4, n_kf):
        m = build_map(ctx, w)
        before = {k: v.copy() for k, v in m.arrays().items()}
        m.add_observations(kf_pos, point, row)
        off, okf, okp = restate_add(w.obs_off, w.obs_kf, w.obs_kp, w.counts, kf_pos, point, row)
        b = m.arrays()
        assert np.array_equal(b["obs_off"], off) and np.array_equal(b["obs_kf"], okf) and np.array_equal(b["obs_kp"], okp)
        assert len(okf) > len(w.obs_kf)
        if kf_pos == 4:
            assert all(np.diff(off)[i] == len(w.obs[i]) for i in have.tolist())
        for k in ("xyz", "color", "id", "dref_kf", "dref_row"):
            assert np.array_equal(before[k], b[k]), k
        m.close()
    # a tracked frame becomes keyframe n_kf: its inlier matches are observations, the co-visibility counts go to the renumbered ids
    m, plain = build_map(ctx, w), build_map(ctx, w)
    T = w.kf_poses[-1].copy()
    T[:3, 3] -= T[:3, :3] @ np.array([0.2, 0.0, 0.0])
    pts = np.array([i for i, o in enumerate(w.obs) if n_kf - 1 in o and len(o) >= 2])
    xy, _ = project(w.K, T, w.xyz[pts])
    kp = kps_array(np.vstack([xy, np.zeros((20, 2))]))
    pt = np.full(len(kp), -1, np.int32); pt[:len(pts)] = pts
    inl = np.zeros(len(kp), bool); inl[:len(pts):2] = True
    desc = np.random.default_rng(5).integers(0, 256, (len(kp), 32)).astype(np.uint8)
    img = np.zeros((w.image_size[1], w.image_size[0]), np.uint8)
    m.add_keyframe(img, kp, desc, T, tracked=(pt, inl))
    plain.add_keyframe(img, kp, desc, T)
    gained = pts[::2]
    a = m.arrays()
    at = {int(i): k for k, i in enumerate(a["id"])}
    for i in gained.tolist():
        k = at[int(w.ids[i])]
        assert a["obs_off"][k + 1] - a["obs_off"][k] == len(w.obs[i]) + 1 and a["obs_kf"][a["obs_off"][k + 1] - 1] == n_kf
    want = {}
    for i in gained.tolist():
        for k in w.obs[i]:
            want[k] = want.get(k, 0) + 1
    assert [kf["id"] for kf in m.keyframes][:n_kf] == list(range(n_kf))
    for k, cnt in want.items():
        assert m.co_visibility_graph[n_kf][k] - plain.co_visibility_graph[n_kf][k] == cnt
        assert m.co_visibility_graph[k][n_kf] - plain.co_visibility_graph[k][n_kf] == cnt
    assert ctx.dev_status() == 0
    m.close(); plain.close(); ctx.close()


def test_stale_and_negative_keys_in_every_read_path():
    """(e) keys left in the positions of before the removal: they name other keyframes, rows beyond a keyframe's keypoints, no keyframe
    at all, or count from the end.  Integers equal the restatements, floats within the bounds above, nothing is written by the two
    read-only calls.  The map is nonsense on purpose: no accuracy is asserted."""
    from tests.test_gpu_bundle_adjust import PARITY_BOUND, _diff, _same_integers
    ctx = _ctx()
    w = world("stale")
    m, twin = build_map(ctx, w), build_map(ctx, w, twin=True)
    _map_is_the_world(m, w)
    T, (kps, desc), pos, (qk, qd) = stale_queries(w)
    snap = _snapshot(m)
    res = m.relocalize(qk, qd)
    r = _reloc_equals_restatement(m, qd, res[2])
    assert r["candidates"] and res[2]["kf_pos"] >= 0
    _same_reloc(res, twin.relocalize(qk, qd))
    _unchanged(m, snap)
    pose0 = perturbed_pose(T)
    for window in (3, 0):
        r1, r2, d = _track_checks(m, w, kps, desc, pose0, window=window)
        assert r1[2]["pass_matches"][0] >= 20
        _same_track(r2, twin.track_local_map(kps, desc, pose0, window=window))
    _unchanged(m, snap)
    m.close(); twin.close()
    # bundle adjustment and add_observations on the consecutive-keyframe world with stale keys
    b = world("ba_stale")
    poses, xyz = perturbed(b, first_free=4)
    ref = ba_restated(b, poses, xyz, max_steps=STALE_BA_STEPS)
    m, twin = build_map(ctx, b, poses=poses, xyz=xyz), build_map(ctx, b, twin=True, poses=poses, xyz=xyz)
    ok, info = m.bundle_adjust(window=BA_WINDOW, max_steps=STALE_BA_STEPS, want_points=True)
    _same_integers(info, ok, ref)
    dd = _diff(info, ref)
    print("stale keys: bundle adjustment %d edges, steps %s, largest difference to the restatement %.3g" % (info["n_edges"], info["steps"], dd))
    assert info["n_edges"] >= 50 and dd <= PARITY_BOUND
    ok2, info2 = twin.bundle_adjust(window=BA_WINDOW, max_steps=STALE_BA_STEPS, want_points=True)
    for k in info:
        assert np.array_equal(np.asarray(info[k]), np.asarray(info2[k]), equal_nan=True), k
    a0 = {k: v.copy() for k, v in m.arrays().items()}
    rng = np.random.default_rng(6)
    point = rng.integers(-5, len(b.obs) + 5, 400).astype(np.int32)
    row = rng.integers(0, 50, 400).astype(np.int32)
    m.add_observations(4, point, row)
    off, okf, okp = restate_add(a0["obs_off"], a0["obs_kf"], a0["obs_kp"], b.counts, 4, point, row)
    a1 = m.arrays()
    assert np.array_equal(a1["obs_off"], off) and np.array_equal(a1["obs_kf"], okf) and np.array_equal(a1["obs_kp"], okp)
    assert ctx.dev_status() == 0
    m.close(); twin.close(); ctx.close()


def test_track_across_octaves():
    """(f) reference octaves 0 .. 7, keyframe keypoints at +/- 1, frame keypoints at -2 .. 2 around the reference: the gate rejects, the
    radius and the information scale.  Scale factors 1.2 and 1.5.  The world's descriptors are code words 128 bits apart (a point
    whose own keypoint the gate rejects would otherwise take a random keypoint at distance <= 100 now and then, and at octave 9 the
    information 1 / sf^18 keeps such a match an inlier up to 12 px off), so the noise-free runs recover the truth at the default max_dist."""
    ctx = _ctx()
    w = world("octave")
    m = build_map(ctx, w)
    T = pose_near(w, 4)
    pose0 = perturbed_pose(T)
    for sf, wrong, seed in ((1.2, 0.0, 6), (1.2, 0.1, 7), (1.5, 0.0, 6)):
        kps, desc = w.track_query(T, octave_spread=2, seed=seed, wrong=wrong, noise=0.5 if wrong else 0.0)
        assert len(np.unique(kps["octave"])) >= 9
        kw = {}
        # (pass 1 alone at radius 6: pose0 puts the projections up to 13 px off, so the octave scaling of the radius decides)
        r1, r2, d = _track_checks(m, w, kps, desc, pose0, truth=None if wrong else T, first=(6.0,), scale_factor=sf, **kw)
        assert r2[0]
        # the gate rejected and the scaling mattered in this very call
        g = track(w, kps, desc, pose0, radii=(6.0,), refine_pose=False, scale_factor=sf, octave_gate=False, **kw)["passes"][0]
        s = track(w, kps, desc, pose0, radii=(6.0,), refine_pose=False, scale_factor=sf, scale_radius=False, **kw)["passes"][0]
        n_g, n_s = int((g["point"] != r1[2]["point"]).sum()), int((s["point"] != r1[2]["point"]).sum())
        assert n_g > 0 and n_s > 0, (n_g, n_s)
        print("octaves, scale factor %.1f, wrong %.1f: matches %s inliers %s, |pose - restated refinement| %.3g, |pose - truth| %.3g"
              % (sf, wrong, r2[2]["pass_matches"], r2[2]["pass_inliers"], d, np.abs(r2[1] - T).max()))
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def _grid_query(w, T, n, seed):
    """n keypoints: the visible points at their projections, keypoints on and beyond every border (x = 0, w - 2^-10, w, beyond, negative;
    the same in y) carrying the descriptor of the nearest projected point, 1500 keypoints inside one grid cell (n = 5000), random ones
    up to n; shuffled"""
    rng = np.random.default_rng(seed)
    W, H = w.image_size
    kps, desc = w.track_query(T, wrong=0.0, extra=0.0, seed=seed)
    xy = np.column_stack([kps["x"], kps["y"]]).astype(np.float64)
    if n == 1:
        return kps[:1].copy(), desc[:1].copy()
    pxy, z = project(w.K, T, w.xyz)
    pxy[~(z > 0)] = 1e9
    sx, sd = [], []
    for v, size, axis in [(0.0, W, 0), (W - 2.0 ** -10, W, 0), (float(W), W, 0), (W + 7.5, W, 0), (-3.25, W, 0),
                          (0.0, H, 1), (H - 2.0 ** -10, H, 1), (float(H), H, 1), (H + 7.5, H, 1), (-3.25, H, 1)]:
        for _ in range(6):
            p = np.array([rng.uniform(0, W), rng.uniform(0, H)])
            p[axis] = v
            near = int(np.argmin(np.abs(pxy - p).max(axis=1)))
            sx.append(p); sd.append(flip(rng, w.base[w.world[near]][None], 4)[0])
    sx, sd = np.array(sx), np.array(sd, np.uint8)
    parts_xy, parts_d = [sx, xy], [sd, desc]
    if n >= 5000:
        c = xy[len(xy) // 2]
        cx, cy = int(c[0] * 64 / W), int(c[1] * 48 / H)
        lo = np.array([cx * W / 64.0, cy * H / 48.0]); hi = np.array([(cx + 1) * W / 64.0, (cy + 1) * H / 48.0])
        inside = lo + (hi - lo) * rng.uniform(0.01, 0.99, (1500, 2))
        parts_xy.append(inside); parts_d.append(rng.integers(0, 256, (1500, 32)).astype(np.uint8))
    axy, ad = np.vstack(parts_xy), np.vstack(parts_d)
    if len(axy) < n:
        k = n - len(axy)
        axy = np.vstack([axy, np.column_stack([rng.uniform(0, W, k), rng.uniform(0, H, k)])])
        ad = np.vstack([ad, rng.integers(0, 256, (k, 32)).astype(np.uint8)])
    if len(axy) > n:   # the border keypoints stay, then the one-cell run (last part), the rest as far as n allows
        keep = np.r_[np.arange(len(sx)), np.arange(len(sx) + len(xy), len(axy)), np.arange(len(sx), len(sx) + len(xy))][:n]
        axy, ad = axy[keep], ad[keep]
    perm = rng.permutation(n)
    return kps_array(axy[perm].astype(np.float32)), ad[perm]


GRID = [((752, 480), 255, 600, 0), ((1241, 376), 256, 600, 0), ((333, 251), 257, 600, 0), ((64, 48), 256, 600, 0),
        ((752, 480), 66000, 80000, 1)]


@pytest.mark.parametrize("image_size,n_points,n_w,window", GRID, ids=["752x480", "1241x376", "333x251", "64x48", "752x480-66000"])
def test_track_grid_geometry(image_size, n_points, n_w, window):
    """(g) image sizes whose 64 x 48 cells are not whole pixels (and 64 x 48 itself: cells of one pixel), keypoints on and outside every
    border, 1500 keypoints in one cell, keypoint counts around the 1024 of k_trk_grid / k_trk_compact, map sizes around the 256 of
    k_trk_rep / k_trk_search and one beyond 65 536; every map with every keypoint count.  The large map is searched with window = 1:
    k_trk_rep still reads all 66 000 points, the local ones (those the last keyframe sees, indices up to the last) are searched, and
    the restatement, which loops over the local points in Python, stays affordable.  The cell table is not exported: point and dist
    over windows that straddle cells are the check."""
    W, H = image_size
    ctx = _ctx(W, H)
    w = MapWorld(image_size=image_size, removed=(1, 4), n_w=n_w, n_points=n_points, n_rand=40, seed=31)
    assert len(w.obs) == n_points
    m = build_map(ctx, w)
    T = pose_near(w, 7 if window else 4)
    pose0 = perturbed_pose(T)
    lm = TR.local_map(w.obs_off, w.obs_kf, w.obs_kp, w.kf_desc, w.kf_oct, window)
    for n in (1, 1023, 1024, 1025, 5000):
        kps, desc = _grid_query(w, T, n, seed=n)
        assert len(kps) == n
        ok, pose, info = m.track_local_map(kps, desc, pose0, radii=(15.0,), image_size=image_size, window=window)
        r = track(w, kps, desc, pose0, radii=(15.0,), refine_pose=False, window=window, local_map=lm)
        ps = r["passes"][0]
        assert info["n_local"] == r["n_local"] and (window or r["n_local"] == n_points)
        if n == 5000:
            assert ps["matches"] >= 20 and (ps["point"].max() > 65536 or n_points < 65536)
        assert np.array_equal(info["point"], ps["point"]), (n, int((info["point"] != ps["point"]).sum()))
        assert np.array_equal(info["dist"], ps["dist"])
        _pass_equals(info, ps)
        out = (kps["x"] < 0) | (kps["x"] >= W) | (kps["y"] < 0) | (kps["y"] >= H)
        print("%dx%d, %d points, %d keypoints: %d candidates, %d matches (%d on keypoints outside the image), radius %s"
              % (W, H, n_points, n, ps["cand"], ps["matches"], int((ps["point"][out] >= 0).sum()), ps["radius"]))
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


@pytest.mark.parametrize("name", ["clean", "ba"])
def test_representative_ties_go_to_the_earlier_observation(name):
    """(h) points whose observations tie on the median distance (three at equal pairwise distance 12; four as D0, D1, D0, D1): the
    frame carries the earlier observation's descriptor exactly, so dist is 0 under the rule and 12 (40) under a later-wins rule"""
    ctx = _ctx()
    w = world(name)
    m = build_map(ctx, w)
    counts = [len(d) for d in w.kf_desc]
    obs = TR.valid_observations(w.obs_off, w.obs_kf, w.obs_kp, counts)
    _, ref = TR.representatives(obs, w.kf_desc, w.kf_oct, np.ones(len(obs), bool))
    hit = 0
    for pos in (2, 5, len(w.survivors) - 2):
        T = w.kf_poses[pos]
        idx = np.array([w.index_of[j] for j, _, _ in w.ties])
        xy, z = project(w.K, T, w.xyz[idx])
        vis = np.flatnonzero((z > 0) & (xy[:, 0] > 1) & (xy[:, 0] < w.image_size[0] - 1) & (xy[:, 1] > 1) & (xy[:, 1] < w.image_size[1] - 1))
        if len(vis) == 0:
            continue
        kps = kps_array(xy[vis].astype(np.float32), [ref[i] for i in idx[vis]])
        desc = np.stack([w.ties[t][1] for t in vis])
        later = np.stack([w.ties[t][2] for t in vis])
        ok, pose, info = m.track_local_map(kps, desc, T, radii=(2.0,), window=0, min_matches=1, image_size=w.image_size)
        r = track(w, kps, desc, T, radii=(2.0,), window=0, min_matches=1, refine_pose=False)["passes"][0]
        assert np.array_equal(info["point"], r["point"]) and np.array_equal(info["dist"], r["dist"])
        own = info["point"] == idx[vis]
        assert (info["dist"][own] == 0).all() and (TR.hamming(desc, later).diagonal() >= 12).all()
        hit += int(own.sum())
    print("%s world: %d tie points matched at distance 0" % (name, hit))
    assert hit >= 10
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


TINY = (2, 16, 16, 32)   # keyframe slots, rows per keyframe, map points, observations: the capacities of tests/test_gpu_mapper.py's tiny run


def _bytes_of(x):
    """every array and number below x, in order, as bytes"""
    if isinstance(x, dict):
        return [(k, _bytes_of(v)) for k, v in sorted(x.items())]
    if isinstance(x, (list, tuple)):
        return [_bytes_of(v) for v in x]
    return None if x is None else np.asarray(x).tobytes()


def _lifetime_pass(ctx, w, poses, xyz, frames):
    """a map at tiny capacities, one call of each feature that keeps scratch of its own, the map destroyed; every output"""
    m = build_map(ctx, w, poses=poses, xyz=xyz, capacity=TINY)
    sizes = (w.n_kf0, max(len(d) for d in w.slot_desc), len(m.map_points), len(m.arrays()["obs_kf"]))
    assert all(a > b for a, b in zip(sizes, TINY)), sizes   # every store outgrew what it was made with
    (tk, td, pose0), (rk, rd), (point, row) = frames
    out = {"track": m.track_local_map(tk, td, pose0, image_size=w.image_size), "reloc": m.relocalize(rk, rd)}
    assert out["track"][2]["n_local"] > 0
    out["ba"] = m.bundle_adjust(window=BA_WINDOW, max_steps=BA_STEPS, want_points=True)
    assert out["ba"][1]["n_edges"] > 0
    m._cache = None
    out["after_ba"] = {k: v.copy() for k, v in m.arrays().items()}
    m.add_observations(3, point, row)
    out["after_add"] = {k: v.copy() for k, v in m.arrays().items()}
    assert len(out["after_add"]["obs_kf"]) > len(out["after_ba"]["obs_kf"])
    out["poses"] = [np.asarray(kf["pose"]).copy() for kf in m.keyframes]
    m.close()
    return _bytes_of(out)


def test_map_lifetime_twice_in_one_context():
    """(i) what the buffers' owners guard: the smallest world (448 points, 8 keyframes after the removal) built at capacities every store
    outgrows, track, relocalize, bundle_adjust and add_observations once each (the three scratch structs made on first use), the map
    destroyed - and all of it again in the same process and context.  The second pass equals the first bit for bit and the context
    holds no error: nothing freed twice or too early, nothing of the first map read by the second."""
    ctx = _ctx()
    w = world("octave")
    poses, xyz = perturbed(w)
    T = pose_near(w, 4)
    tk, td = w.track_query(T, octave_spread=2, seed=6, wrong=0.0)
    rng = np.random.default_rng(8)
    frames = ((tk, td, perturbed_pose(T)), w.reloc_query(3, pose_near(w, 3)),
              (rng.integers(-5, len(w.obs) + 5, 300).astype(np.int32), rng.integers(0, 50, 300).astype(np.int32)))
    first = _lifetime_pass(ctx, w, poses, xyz, frames)
    second = _lifetime_pass(ctx, w, poses, xyz, frames)
    assert first == second
    assert ctx.lib.mo_last_error(ctx.h).decode() == ""
    assert ctx.dev_status() == 0
    ctx.close()
