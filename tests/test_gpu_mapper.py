"""The device LocalMapper (vslam_amd.mapper) against the numpy restatement of the reference's bookkeeping (tests/map_restatement.py)."""
import ctypes as C

import numpy as np
import pytest

from tests.map_restatement import RefMapper, cull_arrays

pytestmark = pytest.mark.gpu

K = np.array([[320.0, 0, 320.0], [0, 320.0, 240.0], [0, 0, 1.0]])


def _rz(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _state(m):
    a = m.arrays()
    lo, ids = m.list_arrays()
    return {k: v.copy() for k, v in a.items()}, lo.copy(), ids.copy(), [kf["map_points"] for kf in m.keyframes]


def test_cull_kernel_on_a_large_synthetic_map():
    """10^6 points with 1 - 4 observations over 8 keyframes (two of them removed and the rest renumbered, negative positions among
    the observation keys): keep mask, compacted order, observations, per-keyframe lists and keyframe counts equal numpy's"""
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    rng = np.random.default_rng(11)
    ctx = _ctx()
    m = LocalMapper(K, save_every_keyframe=False, context=ctx)
    n_kf0, nkp = 10, 512
    W = np.column_stack([rng.uniform(-2, 2, nkp), rng.uniform(-1.5, 1.5, nkp), rng.uniform(3, 6, nkp)])
    poses, xys = [], []
    for k in range(n_kf0):
        T = np.eye(4)
        T[:3, :3] = _rz(rng.uniform(-0.05, 0.05)); T[:3, 3] = [rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1), 0]
        x = (K @ (T[:3, :3] @ W.T + T[:3, 3:4])).T
        xy = (x[:, :2] / x[:, 2:3] + rng.normal(0, 1.5, (nkp, 2))).astype(np.float32)
        kps = np.zeros(nkp, V.KP_DTYPE); kps["x"] = xy[:, 0]; kps["y"] = xy[:, 1]
        # identical descriptors: no ratio-test survivor, so add_keyframe grows nothing
        m.add_keyframe(np.zeros((480, 640), np.uint8), kps, np.zeros((nkp, 32), np.uint8), T)
        poses.append(T); xys.append(xy)
    assert len(m.map_points) == 0
    # _cull_keyframes' outcome: positions 3 and 6 go, the rest are renumbered
    m._check(m.lib.mo_map_remove_keyframes(m._h, np.array([6, 3], np.int32).ctypes.data_as(C.c_void_p), 2))
    for i in (6, 3):
        m.keyframes.pop(i); poses.pop(i); xys.pop(i); m._list_rows.pop(i)
    for i, kf in enumerate(m.keyframes):
        kf["id"] = i
    n_kf = len(m.keyframes)  # 8, and the next keyframe makes 9
    T = poses[-1].copy()
    x = (K @ (T[:3, :3] @ W.T + T[:3, 3:4])).T
    xy_last = (x[:, :2] / x[:, 2:3]).astype(np.float32)
    poses.append(T); xys.append(xy_last)
    n = 10 ** 6
    cnt = rng.integers(1, 5, n)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    no = int(off[-1])
    key = np.argsort(rng.random((n, n_kf + 1)), axis=1)[:, :4]       # distinct keyframe positions per point
    okf = key[np.repeat(np.arange(n), cnt), np.concatenate([np.arange(c) for c in cnt])].astype(np.int32)
    neg = rng.random(no) < 0.2
    okf[neg] -= n_kf + 1
    j = rng.integers(0, nkp, n)
    okp = np.repeat(j, cnt).astype(np.int32)
    other = rng.random(no) < 0.05
    okp[other] = rng.integers(0, nkp, other.sum())
    xyz = (W[j] + rng.normal(0, 0.01, (n, 3))).astype(np.float32)
    ids = rng.permutation(n).astype(np.int32) // 2          # duplicate ids
    zeros = np.zeros(n, np.int32)
    col = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    src = np.arange(n, dtype=np.int32)   # carried through the compaction as the (opaque) descriptor row: each survivor's input index
    m._check(m.lib.mo_map_add_points(m._h, n, *[V._ptr(a) for a in (xyz, col, ids, off, okf, okp)], V._ptr(zeros - 1), V._ptr(src)))
    m._sync_size()
    kps = np.zeros(nkp, V.KP_DTYPE); kps["x"] = xy_last[:, 0]; kps["y"] = xy_last[:, 1]
    m.add_keyframe(np.zeros((480, 640), np.uint8), kps, np.zeros((nkp, 32), np.uint8), T)
    Ps = [K @ np.hstack((p[:3, :3], p[:3, 3:4])) for p in poses]
    keep, near = cull_arrays(Ps, xys, xyz, off, okf, okp)
    got = m.arrays()
    # the device's survivors in order, matched against numpy's keep mask (points within 1e-9 px of 5.0 excepted)
    assert 0.1 * n < keep.sum() < 0.9 * n
    exp_idx = np.flatnonzero(keep)
    assert near.sum() < 10
    # survivors: exactly numpy's keep mask outside the points within 1e-9 px of the threshold, those may go either way
    g = got["dref_row"]
    dev_keep = np.zeros(n, bool); dev_keep[g] = True
    assert np.all(np.diff(g) > 0)   # compaction keeps map order
    assert np.array_equal(dev_keep[~near], keep[~near])
    assert np.array_equal(got["id"], ids[g]) and np.array_equal(got["xyz"], xyz[g]) and np.array_equal(got["color"], col[g])
    assert np.array_equal(np.diff(got["obs_off"]), cnt[g])
    sel = np.repeat(dev_keep, cnt)
    assert np.array_equal(got["obs_kf"], okf[sel]) and np.array_equal(got["obs_kp"], okp[sel])
    del exp_idx
    # lists: stable by keyframe, in map order
    nk = len(m.keyframes)
    eid = np.repeat(got["id"], np.diff(got["obs_off"]))
    k = got["obs_kf"]
    ok = (k >= 0) & (k < nk)
    order = np.argsort(k[ok], kind="stable")
    lo, lids = m.list_arrays()
    assert np.array_equal(lids, eid[ok][order])
    assert np.array_equal(np.diff(lo), np.bincount(k[ok], minlength=nk))
    # keyframe counts: the first point with each id, its keys other than the keyframe's own
    first = {}
    for i, v in enumerate(got["id"].tolist()):
        first.setdefault(v, i)
    red = np.zeros(nk, np.int64)
    offs = got["obs_off"]
    for r in range(nk):
        for v in lids[lo[r]:lo[r + 1]].tolist():
            p = first[v]
            red[r] += int((got["obs_kf"][offs[p]:offs[p + 1]] != r).sum()) >= 3
    assert np.array_equal(m.last["kf_redundant"][:nk], red)
    m.close(); ctx.close()


_SEQ = {}


def _sequence():
    """twelve keyframes of the survey8d scene (every second frame), ground-truth absolute poses; keyframe 5's pose perturbed so the
    cull has points to remove"""
    if not _SEQ:
        import torch
        from vslam_amd.synth import Survey8dScene, frame_roll_deg
        sc = Survey8dScene(torch, "cpu")
        frames, poses = [], []
        for k in range(12):
            g = 2 * k
            frames.append(sc.frame(g).numpy())
            R = _rz(np.deg2rad(frame_roll_deg(sc.seed, g)))
            T = np.eye(4); T[:3, :3] = R; T[:3, 3] = -R @ np.array([g * 0.05, 0.0, 0.0])
            if k == 5:
                T[:3, :3] = _rz(0.004) @ T[:3, :3]
            poses.append(T)
        _SEQ["frames"], _SEQ["poses"] = frames, poses
    return _SEQ["frames"], _SEQ["poses"]


def _run(ctx, tmp_path=None, copy=False, capacity=None, check=None):
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    frames, poses = _sequence()
    kw = {"capacity": capacity} if capacity else {}
    m = LocalMapper(K, output_path=str(tmp_path / "map.ply") if tmp_path else None, save_every_keyframe=tmp_path is not None, context=ctx, **kw)
    prm = V.orb_params(nfeatures=2000)
    states = []
    for k, (fr, T) in enumerate(zip(frames, poses)):
        (kps, desc), = ctx.orb_detect_compute(fr, prm)
        if copy:
            kps, desc = kps.copy(), desc.copy()
        m.add_keyframe(fr, kps, desc, T)
        assert m.last["from_token"] == (not copy)
        if check:
            check(k, m, kps, desc)
        states.append(_state(m))
    return m, states


def test_twelve_keyframes_against_the_restatement(tmp_path):
    """after every add_keyframe: match lists equal the host matcher, the F mask the oracle's (same sampling stream), positions the
    oracle's DLT; ids, colours, observations, per-keyframe lists, co-visibility and the cull equal the restatement fed the device's
    positions; the PLY is byte-identical to the restatement's writer"""
    from oracle import geom_oracle as G
    ctx = _ctx()
    ref = RefMapper(K)
    frames, poses = _sequence()
    prev = {}
    totals = {"grown": 0}

    def check(k, m, kps, desc):
        xy = np.stack([kps["x"], kps["y"]], 1).astype(np.float32)
        growth = None
        if k >= 1:
            idx, dist, keep = ctx.match_knn2_ratio(prev["desc"], desc, 0.8)
            last = m.last
            assert np.array_equal(last["match_idx"], idx) and np.array_equal(last["match_pass"], keep)
            sel = np.flatnonzero(keep & (idx[:, 1] >= 0))
            p1, p2 = prev["xy"][sel], xy[idx[sel, 0]]
            Fo, mo = G.find_fundamental_ransac8(p1, p2, thr_px=3.0, n_hyp=1024, seed=4096, pair=k - 1)
            inl = last["inlier"]
            assert Fo is not None and (inl[sel] != mo).sum() <= 2 and not np.delete(inl, sel).any()
            q = np.flatnonzero(inl)
            X = last["points"][q]
            P1 = ref.keyframes[-1]["P"]; P2 = K @ np.hstack((poses[k][:3, :3], poses[k][:3, 3:4]))
            X4 = G.triangulate(P1, P2, prev["xy"][q].astype(np.float64), xy[idx[q, 0]].astype(np.float64))
            well = np.abs(X4[:, 3]) > 1e-2
            Xo = X4[:, :3] / X4[:, 3:4]
            e = np.linalg.norm(X - Xo, axis=1) / np.maximum(np.linalg.norm(Xo, axis=1), 1e-9)
            assert well.mean() > 0.9 and np.median(e) < 1e-5 and e[well].max() < 1e-4
            growth = (q, idx[q, 0], X)
            assert last["n_new"] == len(q)
            totals["grown"] += len(q)
        ref.add_keyframe(fr_of[k], xy, poses[k], growth)
        a = m.arrays()
        assert not ref.near
        assert a["id"].tolist() == [p["id"] for p in ref.map_points]
        assert np.array_equal(a["xyz"], np.array([p["position"] for p in ref.map_points], np.float32).reshape(-1, 3))
        assert np.array_equal(a["color"], np.array([p["color"] for p in ref.map_points], np.uint8).reshape(-1, 3))
        assert [m.map_points[i]["observed_keyframes"] for i in range(0, len(m.map_points), 97)] == \
            [p["observed_keyframes"] for p in ref.map_points[::97]]
        assert [kf["map_points"] for kf in m.keyframes] == [kf["map_points"] for kf in ref.keyframes]
        assert {a: dict(b) for a, b in m.co_visibility_graph.items()} == {a: dict(b) for a, b in ref.co_visibility_graph.items()}
        prev["desc"], prev["xy"] = desc, xy

    fr_of = frames
    m, _ = _run(ctx, tmp_path=tmp_path, check=check)
    assert 0 < len(m.map_points) < totals["grown"], (len(m.map_points), totals["grown"])
    assert (tmp_path / "map.ply").read_bytes() == ref.ply_text().encode()
    st = m.get_map_statistics()
    assert st["num_keyframes"] == 12 and st["num_map_points"] == len(ref.map_points) and st["avg_observations_per_point"] == 2.0
    mp = m.get_map_point_by_id(ref.map_points[3]["id"])
    assert np.array_equal(mp["descriptor"], m._records[m.arrays()["dref_kf"][3]]["descriptors"][m.arrays()["dref_row"][3]])
    m.close(); ctx.close()


def test_token_path_upload_path_and_tiny_capacities_give_the_same_map():
    ctx = _ctx()
    _, s_tok = _run(ctx)
    _, s_up = _run(ctx, copy=True)
    _, s_tiny = _run(ctx, capacity=(2, 16, 16, 32))
    for a, b, c in zip(s_tok, s_up, s_tiny):
        for x in (b, c):
            assert all(np.array_equal(a[0][f], x[0][f]) for f in a[0])
            assert np.array_equal(a[1], x[1]) and np.array_equal(a[2], x[2]) and a[3] == x[3]
    ctx.close()


def test_update_map_points_and_keyframe_culling():
    """the initializer's dicts (no 'observed_keyframes') are culled at the next keyframe; injected points seen by >= 3 other keyframes
    make _cull_keyframes fire, and the mapper then equals the restatement (renumbered ids, stale observation keys, co-visibility)"""
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    rng = np.random.default_rng(5)
    ctx = _ctx()
    m = LocalMapper(K, save_every_keyframe=False, context=ctx)
    ref = RefMapper(K)
    nkp = 64
    W = np.column_stack([rng.uniform(-1, 1, nkp), rng.uniform(-1, 1, nkp), rng.uniform(3, 5, nkp)])
    T = np.eye(4)
    x = (K @ W.T).T
    xy = (x[:, :2] / x[:, 2:3]).astype(np.float32)
    kps = np.zeros(nkp, V.KP_DTYPE); kps["x"] = xy[:, 0]; kps["y"] = xy[:, 1]
    img = rng.integers(0, 256, (480, 640, 3)).astype(np.uint8)
    init = [{"position": W[i], "color": np.array([1, 2, 3]), "keypoint_references": {0: i, 1: i}, "observed_frames": [0, 1]} for i in range(10)]
    m.update_map_points(init); ref.map_points.extend(init)
    assert len(m.map_points) == 10 and m.get_map_statistics()["num_filtered_points"] == 0
    inj = [{"id": 100 + i, "position": W[i].astype(np.float32), "color": np.array([4, 5, 6], np.uint8),
            "observed_keyframes": {0: i, 1: i, 2: i, 3: i}} for i in range(30)]
    for k in range(5):
        if k == 3:
            m.update_map_points(inj); ref.map_points.extend(inj)
        m.add_keyframe(img, kps, np.zeros((nkp, 32), np.uint8), T)
        ref.add_keyframe(img, xy, T, None)
        assert [p.get("id") for p in m.map_points] == [p.get("id") for p in ref.map_points]
        assert [kf["id"] for kf in m.keyframes] == [kf["id"] for kf in ref.keyframes]
        assert [kf["map_points"] for kf in m.keyframes] == [kf["map_points"] for kf in ref.keyframes]
    # keyframes 1.. were redundant: popped, the rest renumbered; the observation keys stay stale
    assert len(ref.keyframes) < 5 and len(m.keyframes) == len(ref.keyframes)
    assert m.map_points[0] is inj[0] and m.map_points[0]["observed_keyframes"] == {0: 0, 1: 0, 2: 0, 3: 0}
    assert {a: dict(b) for a, b in m.co_visibility_graph.items()} == {a: dict(b) for a, b in ref.co_visibility_graph.items()}
    # a key beyond the renumbered keyframes: the next keyframe's cull raises IndexError, as the reference's
    bad = [{"id": 999, "position": W[0].astype(np.float32), "color": np.array([0, 0, 0], np.uint8), "observed_keyframes": {0: 0, 7: 0}}]
    m.update_map_points(bad); ref.map_points.extend(bad)
    with pytest.raises(IndexError):
        ref.add_keyframe(img, xy, T, None)
    with pytest.raises(IndexError):
        m.add_keyframe(img, kps, np.zeros((nkp, 32), np.uint8), T)
    m.close(); ctx.close()


def test_per_keyframe_growth_equals_the_batched_keyframe_mode():
    """the mapper's growth of keyframe pair k (sampling stream pair_index = k) equals MO_MODE_KEYFRAME on the same twelve keyframes
    with pair_index_base = 0 (pair k = keyframes k, k + 1) bit for bit: match lists, ratio flags, F, the inlier mask and the points"""
    import torch
    import vslam_amd as V
    from tests.test_gpu_dropin import _batch_io
    from vslam_amd.mapper import LocalMapper
    frames, poses = _sequence()
    nb, cap = len(frames), 2048
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    try:
        ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=nb)
        ctx.set_stream(st.cuda_stream)
        prm = V.orb_params(nfeatures=2000)
        d_fr = torch.from_numpy(np.stack(frames)).to(dev)
        io, b, _ = _batch_io(torch, V, dev, d_fr, nb, cap, 1024, want_mask=True)
        pairs = [(k, k + 1) for k in range(nb - 1)]
        P = [K @ np.hstack((T[:3, :3], T[:3, 3:4])) for T in poses]
        d_q = torch.tensor([q for q, _ in pairs], dtype=torch.int32, device=dev)
        d_t = torch.tensor([t for _, t in pairs], dtype=torch.int32, device=dev)
        d_P1 = torch.from_numpy(np.stack([P[q].reshape(12) for q, _ in pairs])).to(dev)
        d_P2 = torch.from_numpy(np.stack([P[t].reshape(12) for _, t in pairs])).to(dev)
        d_F = torch.zeros((len(pairs), 9), dtype=torch.float64, device=dev)
        io.mode = V.MODE_KEYFRAME; io.ratio = 0.8; io.thr_px = 3.0; io.n_kf_pairs = len(pairs); io.pair_index_base = 0
        io.d_kf_query = d_q.data_ptr(); io.d_kf_train = d_t.data_ptr(); io.d_kf_P1 = d_P1.data_ptr(); io.d_kf_P2 = d_P2.data_ptr()
        io.d_kf_F = d_F.data_ptr()
        ctx._check(ctx.lib.mo_dev_frontend_batch(ctx.h, C.byref(prm), C.byref(io)))
        st.synchronize()
        assert ctx.dev_status() == 0
        cn = b["counts"].cpu().numpy()
        kps = b["kps"].cpu().numpy()
        desc = b["desc"].cpu().numpy()
        m = LocalMapper(K, save_every_keyframe=False, context=ctx)
        grown = 0
        for k in range(nb):
            kp = np.ascontiguousarray(kps[k, :cn[k]]).view(V.KP_DTYPE).reshape(-1)
            m.add_keyframe(frames[k], kp, desc[k, :cn[k]].copy(), poses[k])
            if k == 0:
                continue
            p, nq = k - 1, cn[k - 1]
            last = m.last
            assert np.array_equal(last["match_idx"], b["midx"][p, :nq].cpu().numpy()), k
            assert np.array_equal(last["match_pass"], b["mpass"][p, :nq].cpu().numpy().astype(bool)), k
            assert np.array_equal(last["F"].reshape(9), d_F[p].cpu().numpy(), equal_nan=True), k
            assert np.array_equal(last["inlier"], b["pmask"][p, :nq].cpu().numpy().astype(bool)), k
            assert np.array_equal(last["points"], b["pts"][p, :nq].cpu().numpy(), equal_nan=True), k
            assert last["n_new"] == int(b["npts"][p].item())
            grown += last["n_new"]
        assert grown > 1000
        m.close(); ctx.close()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream(dev))


def test_run_frames_with_a_map(tmp_path):
    """examples/run_frames.py --map on the synthetic sequence: keyframes into the device mapper, a PLY written, a non-empty map"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "map.ply"
    r = subprocess.run([sys.executable, os.path.join(root, "visual-slam_amd", "examples", "run_frames.py"), "--max-frames", "40",
                        "--keyframe-every", "5", "--map", str(out)], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    stats = [ln for ln in r.stdout.splitlines() if ln.startswith("map statistics: ")]
    assert stats and "'num_map_points': 0," not in stats[-1], r.stdout[-2000:]
    text = out.read_text()
    assert text.startswith("ply\nformat ascii 1.0\nelement vertex ") and int(text.split("\n")[2].split()[-1]) > 0
