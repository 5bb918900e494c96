"""LocalMapper.track_local_map_batch (mo_map_track_batch, csrc/map_track_batch.hip) at the sizes where its own code runs, on the worlds of
tests/track_batch_worlds.py: the strided walk of k_tb_search over a local list longer than two rounds, the compaction of a list that
is far from dense, k_tb_scan across its chunks of 1024 blocks and a partial last block, the early return behind the workgroup remap,
the frame indexing up to the maximum batch, and the keypoint-count regimes of k_trk_grid / k_trk_compact that test_track_grid_geometry
(tests/test_gpu_map_reads.py) checks for the per-frame kernels.

The rule under test is the header's: every frame of a batch gets what track_local_map returns for it alone - integers equal, doubles
equal bit for bit (_equal of tests/test_gpu_track_batch.py).  Named frames are also compared with the numpy restatement of pass 1
(integers only; the refined pose against the restatement is tests/test_gpu_track_batch.py's).  No tolerance anywhere in this file.
tests/test_track_batch_worlds_cpu.py shows on the CPU that the worlds reach what is claimed here."""
import numpy as np
import pytest

from tests import track_batch_worlds as TB
from tests.test_gpu_track_batch import _bits, _equal, _singles

pytestmark = pytest.mark.gpu


def _ctx(w=640, h=480):
    import vslam_amd as V
    return V.Context(device=0, max_w=max(w, 640), max_h=max(h, 480), max_batch=1)


@pytest.fixture(scope="module")
def grid_map():
    """(context, world, device map, 19 frames, poses, index of each named frame) of the grid world, built once for this module"""
    from tests.map_worlds import build_map
    w = TB.grid_world()
    ctx = _ctx(*w.image_size)
    m = build_map(ctx, w)
    frames, pose0, at = TB.grid_batch()
    yield ctx, w, m, frames, pose0, at
    m.close(); ctx.close()


@pytest.fixture(scope="module")
def scan_map():
    w = TB.scan_world()
    ctx = _ctx()
    m = TB.build_scan_map(ctx, w)
    yield ctx, w, m
    m.close(); ctx.close()


def _first(infos):
    """matches of pass 1 of every frame (0 for a frame no pass ran for)"""
    return [x["pass_matches"][0] if x["pass_matches"] else 0 for x in infos]


def _restated_pass(info, r, tag):
    """the integers of pass 1 against TR.track's"""
    ps = r["passes"][0]
    assert info["n_local"] == r["n_local"], (tag, info["n_local"], r["n_local"])
    assert np.array_equal(info["point"], ps["point"]), (tag, int((info["point"] != ps["point"]).sum()))
    assert np.array_equal(info["dist"], ps["dist"]), tag
    assert info["pass_cand"][0] == ps["cand"] and info["pass_matches"][0] == ps["matches"], (tag, info["pass_cand"], ps["cand"], info["pass_matches"], ps["matches"])


def test_stride_rounds_and_frame_shape_edges(grid_map):
    """19 frames on the grid world, window 3.  pblocks = ceil(100000 / 256) = 391, lb_per_frame = min(391, max(TB_MIN_LB = 128,
    ceil(TB_SEARCH_WGS = 2048 / 19) = 108)) = 128, n_local = 66481 = 259 * 256 + 177 list entries: workgroup lb of a frame walks the list
    blocks lb, lb + 128 and (lb < 4) lb + 256, the last of them partial; 128 * 19 = 8 * 304, so no workgroup of this launch returns
    early.  The frames are test_track_grid_geometry's keypoint counts around the 1024 of k_trk_grid / k_trk_compact (1, 1023, 1024, 1025,
    5000 with 1500 keypoints in one cell, keypoints on and beyond every border), 13 frames of 200 .. 900 rows from other poses and one
    empty frame, at stride 5000.  The n = 1025 frame's matches stand in all three rounds (343 / 340 / 9 in the restatement)."""
    ctx, w, m, frames, pose0, at = grid_map
    nf = len(frames)
    kw = dict(image_size=w.image_size, window=TB.GRID_WINDOW)
    one = _singles(m, frames, pose0, radii=(15.0,), **kw)
    batch = m.track_local_map_batch(frames, pose0, radii=(15.0,), **kw)
    n_local = batch[2][0]["n_local"]
    assert n_local > 65536 and nf >= 17 and max(len(k) for k, _ in frames) == TB.GRID_STRIDE
    for i in range(nf):
        _equal(one[i], batch, i, "one pass")
    r = TB.grid_restated(1025)
    info = batch[2][at[1025]]
    _restated_pass(info, r, "n = 1025")
    per_round, _ = TB.matches_per_round(info["point"], TB.list_positions(TB.grid_local_map()[1]))
    print("n_local %d; n = 1025: %d candidates, %d matches, %s in the three rounds; matches of all frames %s"
          % (n_local, info["pass_cand"][0], info["pass_matches"][0], per_round, _first(batch[2])))
    assert min(per_round) >= 1
    assert batch[2][at[5000]]["pass_matches"][0] >= 20 and batch[2][at[5000]]["point"].max() >= 65536
    assert sum(n >= 20 for n in _first(batch[2])) >= 16   # (nothing above compares empty results)
    # the default two passes
    one2 = _singles(m, frames, pose0, **kw)
    batch2 = m.track_local_map_batch(frames, pose0, **kw)
    for i in range(nf):
        _equal(one2[i], batch2, i, "two passes")
    assert sum(x["n_pass_run"] == 2 for x in batch2[2]) >= 16 and batch2[0].sum() >= 12, (batch2[0], [x["n_pass_run"] for x in batch2[2]])
    # the same batch reversed gives the reversed results
    rev = m.track_local_map_batch(frames[::-1], pose0[::-1], **kw)
    for i in range(nf):
        _equal(one2[i], rev, nf - 1 - i, "reversed")
    assert np.array_equal(_bits(rev[1][::-1]), _bits(batch2[1])) and np.array_equal(rev[0][::-1], batch2[0])
    assert ctx.dev_status() == 0


def _ranges_and_ties(w, info, marks, tag):
    """matches in each of the four index ranges; the lower of the duplicate points and the lower of the duplicate keypoints win"""
    matched = info["point"][info["point"] >= 0]
    in_range = np.bincount(w.range_of(matched) + 1, minlength=5)
    assert in_range[0] == 0 and (in_range[1:] >= 1).all(), (tag, in_range)
    lo, hi = w.dup_points
    q = marks["dup_points"]
    assert info["point"][q] == lo and info["dist"][q] == 0 and not (info["point"] == hi).any(), (tag, info["point"][q], lo, hi)
    q1, q2 = marks["dup_kp"]
    assert q1 < q2 and info["point"][q1] == w.dup_kp_point and info["dist"][q1] == 0 and info["point"][q2] == -1, (tag, info["point"][[q1, q2]])
    return in_range[1:].tolist()


def test_scan_across_chunks_partial_last_block_and_remap_tail(scan_map):
    """The scan world, window 3: pblocks = 1027, so k_tb_scan carries its running total from the chunk of blocks 0 .. 1023 into the chunk
    of blocks 1024 .. 1026, the last of them of 37 points; the local list has 178284 of the 262693 points (697 list blocks).
      1 frame:  lb_per_frame = min(1027, max(128, 2048)) = 1027, the launch is 8 * ceil(1027 / 8) = 1032 workgroups: five return early.
      2 frames: lb_per_frame = min(1027, max(128, 1024)) = 1024, 2048 workgroups, none returns early.
      3 frames: lb_per_frame = min(1027, max(128, 683)) = 683, 2049 pairs in a launch of 2056: seven return early, and the list blocks
                683 .. 696 - where every match of the three upper index ranges stands - are reached in a second round only.
    With window 0 the list is all 262693 points (1027 list blocks): at 2 frames the blocks 1024 .. 1026 are a second round.
    Every frame equals its single call; the first frame equals the restatement through the vectorised local map; matches exist in block
    0, on both sides of point 262144 and in the last partial block; the duplicate point pair and the duplicate keypoint pair resolve to
    the lower index."""
    ctx, w, m = scan_map
    for window in (TB.SCAN_WINDOW, 0):
        frames, pose0, marks, lm, r = TB.scan_case(window)
        kw = dict(radii=(15.0,), window=window)
        one = _singles(m, frames, pose0, **kw)
        assert all(x[2]["pass_matches"][0] >= 20 for x in one)
        for nf in (1, 2, 3) if window else (2,):
            batch = m.track_local_map_batch(frames[:nf], pose0[:nf], **kw)
            for i in range(nf):
                _equal(one[i], batch, i, "window %d, %d frames" % (window, nf))
            _restated_pass(batch[2][0], r, (window, nf))
            per = _ranges_and_ties(w, batch[2][0], marks, (window, nf))
            print("window %d, %d frames: n_local %d, matches %s, first frame per range %s"
                  % (window, nf, batch[2][0]["n_local"], [x["pass_matches"][0] for x in batch[2]], per))
        # the two default passes, three frames
        one2 = _singles(m, frames, pose0, window=window)
        batch2 = m.track_local_map_batch(frames, pose0, window=window)
        for i in range(3):
            _equal(one2[i], batch2, i, "window %d, two passes" % window)
        assert batch2[0].all()
    assert ctx.dev_status() == 0


def _sixteen(w):
    """16 distinct (frame, pose) pairs on _World of at most 300 rows each, with different row counts: one empty, one of distractors
    alone, 14 cuts of _query frames from different poses"""
    import vslam_amd as V
    from tests.test_gpu_relocalize import _kps, _pose, _rot
    from tests.test_gpu_track_map import _perturbed, _query
    rng = np.random.default_rng(91)
    frames, poses = [], []
    for j in range(14):
        T = w.poses[1 + j % 6] @ _pose(_rot(rng.uniform(-0.02, 0.02, 3)), rng.uniform(-0.1, 0.1, 3))
        kps, desc = _query(w, T, noise=0.3 * (j % 2), seed=40 + j)
        n = 300 - 11 * j
        assert len(kps) >= n
        frames.append((np.ascontiguousarray(kps[:n]), np.ascontiguousarray(desc[:n]))); poses.append(_perturbed(T))
    n_d = 97
    frames.insert(4, (np.zeros(0, V.KP_DTYPE), np.zeros((0, 32), np.uint8))); poses.insert(4, w.poses[0])
    frames.insert(11, (_kps(np.column_stack([rng.uniform(0, 640, n_d), rng.uniform(0, 480, n_d)]).astype(np.float32)),
                       rng.integers(0, 256, (n_d, 32)).astype(np.uint8))); poses.insert(11, w.poses[5])
    assert len(frames) == 16 and len({len(k) for k, _ in frames}) == 16 and max(len(k) for k, _ in frames) <= 300
    return frames, poses


def _sequence(n, seed=5):
    """n indices into the 16 pairs: seeded permutations of all 16 one after the other, no two neighbours equal"""
    rng = np.random.default_rng(seed)
    seq = []
    while len(seq) < n:
        p = rng.permutation(16).tolist()
        if seq and p[0] == seq[-1]:
            p[0], p[1] = p[1], p[0]
        seq += p
    seq = seq[:n]
    assert all(a != b for a, b in zip(seq, seq[1:])) and len(set(seq[:16])) == 16
    return seq


def test_the_maximum_batch_and_batches_with_a_remap_tail():
    """V.TRACK_BATCH_MAX = 1024 frames of 16 distinct (frame, pose) pairs on _World (4507 points, pblocks = 18 = lb_per_frame): res_all + f,
    f * stride and f * (TK_CELLS + 1) up to the last frame.  Then 17 and 23 frames: 18 * 17 = 306 and 18 * 23 = 414 pairs in launches of
    312 and 416 workgroups, of which six and two return early."""
    import vslam_amd as V
    from tests.test_gpu_relocalize import _World
    ctx = _ctx()
    w = _World(ctx)
    frames, poses = _sixteen(w)
    one = _singles(w.m, frames, poses)
    roles = [(len(frames[i][0]), one[i][2]["n_pass_run"], bool(one[i][0])) for i in range(16)]
    print("(rows, passes run, ok) of the 16 pairs:", roles)
    assert one[4][2]["n_pass_run"] == 0 and one[11][2]["n_pass_run"] == 1 and not one[11][0] and sum(x[0] for x in one) >= 12
    pblocks = (w.m._n_points + 255) // 256
    assert pblocks == 18
    for n in (V.TRACK_BATCH_MAX, 17, 23):
        assert (pblocks * n) % 8 == {V.TRACK_BATCH_MAX: 0, 17: 2, 23: 6}[n]
        seq = _sequence(n)
        batch = w.m.track_local_map_batch([frames[j] for j in seq], [poses[j] for j in seq])
        assert len(batch[2]) == n
        for i, j in enumerate(seq):
            _equal(one[j], batch, i, "%d frames" % n)
    assert ctx.dev_status() == 0
    w.m.close(); ctx.close()


def test_poison(grid_map, scan_map):
    """the 19-frame grid batch and the 2-frame scan batch under poison byte 255, on the maps the tests above read: the unpoisoned bytes"""
    from tests.test_gpu_scratch_poison import _checked, _flat, _same, _set
    ctx, w, m, frames, pose0, at = grid_map
    sctx, sw, sm = scan_map
    sframes, spose0 = TB.scan_case()[:2]
    calls = [(ctx, "grid batch of 19", lambda: m.track_local_map_batch(frames, pose0, image_size=w.image_size, window=TB.GRID_WINDOW)),
             (sctx, "scan batch of 2", lambda: sm.track_local_map_batch(sframes[:2], spose0[:2], window=TB.SCAN_WINDOW))]
    for c, name, fn in calls:
        want = _flat(_checked(c, fn, False))
        _set(c, 255)
        try:
            _same(_flat(_checked(c, fn, True)), want, (255, name))
        finally:
            _set(c, -1)
        assert c.dev_status() == 0
