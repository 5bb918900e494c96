"""Worlds for the batched map tracker (mo_map_track_batch, csrc/map_track_batch.hip) at the sizes where its own code runs: the compacted
local list, the strided walk of k_tb_search over list blocks, k_tb_scan across its chunks of 1024, the tail of the workgroup remap.
Plain numpy; the device maps are built by build_map (tests/map_worlds.py) and build_scan_map, which import the library when called.
tests/test_track_batch_worlds_cpu.py checks on the restatement alone that these worlds reach what tests/test_gpu_track_batch_regimes.py
relies on.

The shapes derive from three constants of map_track_batch.hip (NOTES.md names them too; whoever moves one moves the shapes):
  TB_SEARCH_WGS = 2048, TB_MIN_LB = 128:  lb_per_frame = min(pblocks, max(TB_MIN_LB, ceil(TB_SEARCH_WGS / n_frames))), pblocks =
                ceil(map points / 256).  A workgroup of k_tb_search walks the list blocks lb, lb + lb_per_frame, ...: it makes a second
                round only when the local list has more than lb_per_frame * 256 entries.
  the 1024 of k_tb_scan:  the per-block counts are scanned in chunks of 1024 blocks; the running total is carried into a second chunk
                only on a map of more than 1024 * 256 points.

The grid world: the large world of test_track_grid_geometry (tests/test_gpu_map_reads.py) grown to 100 000 points.  With window = 3 its
local list has 66 481 entries (> 2 * 128 * 256), a third of the map is not local, and with 17 frames or more (lb_per_frame = 128) a
workgroup makes three rounds, the last one partial.

The scan world: 1024 * 256 + 2 * 256 + 37 points (pblocks = 1027) injected through one mo_map_add_points call, six keyframes of 2000
random rows, two valid observations per point.  About a third of the points, by a seeded mask, are observed by the two oldest
keyframes alone and fall outside window = 3: the per-block counts differ and the list is not the identity.  Almost all points lie
behind the camera (local and listed, never candidates: the Python restatement skips them at once); the points in view of the query
poses sit in four index ranges - block 0, the last 300 indices below 262 144, the first 300 from 262 144 on, the last partial block
(893 points, about 600 of them local).  Two of them are exact duplicates (same xyz, first observations on rows with identical
descriptors and octaves, the lower one in block 0, the higher one in the last block), and the first query frame carries one keypoint
twice (same position, the descriptor of its point exactly)."""
import numpy as np

from tests import track_restatement as TR
from tests.ba_scene import pose, rot
from tests.map_worlds import BASE_K, MapWorld, flip, kps_array, perturbed_pose, pose_near, project, track

# ---- the grid world -------------------------------------------------------------------------------------------------------------------
GRID_SIZE = (752, 480)
GRID_WINDOW = 3
GRID_NS = (1, 1023, 1024, 1025, 5000)   # the keypoint counts of test_track_grid_geometry; 5000 carries the 1500-keypoint cell
GRID_STRIDE = 5000
ROUND = 128 * 256                       # list entries one round of the 128 workgroups of a frame covers (TB_MIN_LB * 256)
_G = {}


def grid_world():
    if "w" not in _G:
        _G["w"] = MapWorld(image_size=GRID_SIZE, removed=(1, 4), n_w=120000, n_points=100000, n_rand=40, seed=31)
    return _G["w"]


def grid_local_map():
    """TR.local_map of the grid world at GRID_WINDOW, derived once"""
    if "lm" not in _G:
        w = grid_world()
        _G["lm"] = TR.local_map(w.obs_off, w.obs_kf, w.obs_kp, w.kf_desc, w.kf_oct, GRID_WINDOW)
    return _G["lm"]


def list_positions(ref):
    """position of every local point in the ascending local list (-1: not local), from the ref_octave list of a local map"""
    local = np.array([r is not None for r in ref], bool)
    return np.where(local, np.cumsum(local) - 1, -1)


def grid_batch():
    """(frames, pose0, at): the 19 frames of the stride test and the index of each GRID_NS frame among them.  The five GRID_NS frames
    are test_track_grid_geometry's (_grid_query from pose_near(w, 7), seed = n); 13 more _grid_query frames of 200 .. 900 rows from
    different poses near positions 5 .. 7, and one empty frame."""
    if "batch" not in _G:
        from tests.test_gpu_map_reads import _grid_query
        import vslam_amd as V
        w = grid_world()
        rng = np.random.default_rng(77)
        frames, poses = [], []
        rows = rng.permutation(np.arange(200, 851, 50))[:13] + rng.integers(0, 50, 13)
        for j, n in enumerate(rows.tolist()):
            T = pose_near(w, 5 + j % 3, rng.uniform(-0.02, 0.02, 3).tolist(), rng.uniform(-0.1, 0.1, 3).tolist())
            frames.append(_grid_query(w, T, n, seed=100 + j)); poses.append(perturbed_pose(T))
        frames.insert(6, (np.zeros(0, V.KP_DTYPE), np.zeros((0, 32), np.uint8))); poses.insert(6, perturbed_pose(pose_near(w, 6)))
        T7 = pose_near(w, 7)
        at = {}
        for n, i in zip(GRID_NS, (2, 5, 9, 13, 17)):   # among the others, none first, none last
            frames.insert(i, _grid_query(w, T7, n, seed=n)); poses.insert(i, perturbed_pose(T7))
        for n in GRID_NS:
            at[n] = [i for i, (k, _) in enumerate(frames) if len(k) == n][0]
        assert len(frames) == 19 and sorted(at.values()) == [2, 5, 9, 13, 17] and len({len(k) for k, _ in frames}) == 19
        _G["batch"] = (frames, poses, at)
    return _G["batch"]


def grid_restated(n):
    """pass 1 at radius 15 of the GRID_NS frame of n keypoints, restated in numpy: TR.track's result"""
    if ("r", n) not in _G:
        frames, poses, at = grid_batch()
        kps, desc = frames[at[n]]
        _G["r", n] = track(grid_world(), kps, desc, poses[at[n]], radii=(15.0,), refine_pose=False, window=GRID_WINDOW, local_map=grid_local_map())
    return _G["r", n]


def matches_per_round(point, list_pos, rnd=ROUND):
    """how many matched points of `point` stand in each round of the list ([0, rnd), [rnd, 2 rnd), ...), and their list positions"""
    p = point[point >= 0]
    pos = list_pos[p]
    assert (pos >= 0).all()
    return np.bincount(pos // rnd, minlength=3).tolist(), pos


# ---- the scan world -------------------------------------------------------------------------------------------------------------------
SCAN_SPLIT = 1024 * 256                   # the first point of k_tb_scan's second chunk
SCAN_N = SCAN_SPLIT + 2 * 256 + 37        # pblocks = 1027, the last block partial
SCAN_WINDOW = 3
SCAN_SIZE = (640, 480)


class ScanWorld:
    """kf_desc / kf_oct / kf_poses per keyframe, xyz f32, obs_off / obs_kf / obs_kp, ranges (the four index ranges in view), in_view,
    dup_points (lower, higher), dup_kp_point (the point whose keypoint a frame may carry twice)"""

    def __init__(self, n_pts=SCAN_N, split=SCAN_SPLIT, edge=300, rows=2000, n_kf=6, not_local_share=0.32, seed=41):
        rng = np.random.default_rng(seed)
        self.K, self.image_size, self.n_kf, self.rows = BASE_K.copy(), SCAN_SIZE, n_kf, rows
        last = (n_pts - 1) // 256 * 256
        self.ranges = [(0, 256), (split - edge, split), (split, split + edge), (last, n_pts)]
        assert 256 <= split - edge and split + edge <= last < n_pts
        self.kf_desc = [rng.integers(0, 256, (rows, 32)).astype(np.uint8) for _ in range(n_kf)]
        self.kf_oct = [rng.integers(0, 3, rows).astype(np.int32) for _ in range(n_kf)]
        self.kf_poses = [pose(np.eye(3), np.array([0.01 * k, 0.0, 0.0])) for k in range(n_kf)]
        # behind the camera, but for the four ranges
        xyz = np.column_stack([rng.uniform(-3, 3, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(-10, -4, n_pts)])
        self.in_view = np.concatenate([np.arange(a, b) for a, b in self.ranges])
        nv = len(self.in_view)
        xyz[self.in_view] = np.column_stack([rng.uniform(-1.8, 1.8, nv), rng.uniform(-1.3, 1.3, nv), rng.uniform(4, 10, nv)])
        # two observations each: (0, 1) in either order for the points outside every window < n_kf - 1; else one keyframe of the last
        # three and one other, in either order
        out = rng.random(n_pts) < not_local_share
        b = rng.integers(n_kf - 3, n_kf, n_pts)
        a = (b + rng.integers(1, n_kf, n_pts)) % n_kf
        a[out], b[out] = 0, 1
        swap = rng.random(n_pts) < 0.5
        kf = np.where(swap[:, None], np.column_stack([b, a]), np.column_stack([a, b]))
        row = rng.integers(0, rows, (n_pts, 2))
        # the points in view name rows of their own in the first observation: no two of them share a representative by chance
        nxt = [iter(rng.permutation(rows).tolist()) for _ in range(n_kf)]
        for i in self.in_view.tolist():
            row[i, 0] = next(nxt[kf[i, 0]])
            if row[i, 1] == row[i, 0] and kf[i, 1] == kf[i, 0]:
                raise AssertionError("an observation twice")
        assert (kf[:, 0] != kf[:, 1]).all()
        self.not_local = out
        # the duplicate pair: local points in block 0 and in the last block
        local_view = [[i for i in range(a_, b_) if not out[i]] for a_, b_ in self.ranges]
        lo, hi = local_view[0][len(local_view[0]) // 2], local_view[3][len(local_view[3]) // 2]
        xyz[hi] = xyz[lo]
        self.kf_desc[kf[hi, 0]][row[hi, 0]] = self.kf_desc[kf[lo, 0]][row[lo, 0]]
        self.kf_oct[kf[hi, 0]][row[hi, 0]] = self.kf_oct[kf[lo, 0]][row[lo, 0]]
        self.dup_points = (lo, hi)
        self.dup_kp_point = local_view[2][len(local_view[2]) // 3]
        self.xyz = xyz.astype(np.float32)
        self.obs_off = (np.arange(n_pts + 1) * 2).astype(np.int32)
        self.obs_kf = np.ascontiguousarray(kf.reshape(-1), np.int32)
        self.obs_kp = np.ascontiguousarray(row.reshape(-1), np.int32)

    def range_of(self, point):
        """index of the range each point index lies in (-1: none)"""
        point = np.asarray(point)
        r = np.full(point.shape, -1)
        for j, (a, b) in enumerate(self.ranges):
            r[(point >= a) & (point < b)] = j
        return r

    def frame(self, T, seed, keep=1.0, dup_kp=False):
        """(keypoints, descriptors, marks): the points in view - local or not - seen from T, each a keypoint at its projection with the
        descriptor and the octave of its first observation (up to 6 bits flipped), a share `keep` of them; 30 % random keypoints on
        top.  The higher duplicate point has no keypoint of its own; the lower one's carries its descriptor exactly.  dup_kp: the
        keypoint of dup_kp_point stands twice, with that point's descriptor exactly.  marks: {"dup_points": q, "dup_kp": (q1, q2)}."""
        rng = np.random.default_rng(seed)
        W, H = self.image_size
        lo, hi = self.dup_points
        pts = self.in_view[self.in_view != hi]
        xy, z = project(self.K, T, self.xyz[pts])
        vis = (z > 0) & (xy[:, 0] > 0) & (xy[:, 0] < W) & (xy[:, 1] > 0) & (xy[:, 1] < H)
        special = (pts == lo) | (pts == self.dup_kp_point)
        assert vis[special].all()
        use = vis & ((rng.random(len(pts)) < keep) | special)
        pts, xy = pts[use], xy[use]
        kf0, row0 = self.obs_kf[2 * pts], self.obs_kp[2 * pts]
        exact = np.stack([self.kf_desc[k][r] for k, r in zip(kf0, row0)])
        d = flip(rng, exact, 6)
        octv = np.array([self.kf_oct[k][r] for k, r in zip(kf0, row0)], np.int32)
        keep_exact = (pts == lo) | (pts == self.dup_kp_point)
        d[keep_exact] = exact[keep_exact]
        tag = np.where(pts == lo, 1, np.where(pts == self.dup_kp_point, 2, 0))
        if dup_kp:
            j = int(np.flatnonzero(pts == self.dup_kp_point)[0])
            xy, d, octv, tag = np.vstack([xy, xy[j:j + 1]]), np.vstack([d, d[j:j + 1]]), np.r_[octv, octv[j]], np.r_[tag, 2]
        n_extra = int(0.3 * len(xy))
        xy = np.vstack([xy, np.column_stack([rng.uniform(0, W, n_extra), rng.uniform(0, H, n_extra)])]).astype(np.float32)
        d = np.vstack([d, rng.integers(0, 256, (n_extra, 32)).astype(np.uint8)])
        octv = np.r_[octv, rng.integers(0, 4, n_extra)].astype(np.int32)
        tag = np.r_[tag, np.zeros(n_extra, np.int64)]
        perm = rng.permutation(len(xy))
        tag = tag[perm]
        marks = {"dup_points": int(np.flatnonzero(tag == 1)[0]), "dup_kp": tuple(np.flatnonzero(tag == 2).tolist())}
        return kps_array(xy[perm], octv[perm]), np.ascontiguousarray(d[perm]), marks

    def queries(self):
        """(frames, pose0, marks of the first frame): three frames from different poses with different keypoint counts; the first one
        carries the duplicated keypoint"""
        Ts = [pose(rot([0.01, -0.02, 0.01]), np.array([0.1, -0.05, 0.05])), pose(rot([-0.02, 0.01, 0.0]), np.array([-0.08, 0.03, 0.1])),
              pose(rot([0.0, 0.02, -0.015]), np.array([0.05, 0.06, -0.04]))]
        off = pose(rot([0.002, -0.001, 0.004]), np.array([0.01, -0.01, 0.01]))   # a few pixels
        got = [self.frame(T, seed=60 + i, keep=(1.0, 0.8, 0.6)[i], dup_kp=i == 0) for i, T in enumerate(Ts)]
        frames = [(k, d) for k, d, _ in got]
        assert len({len(k) for k, _ in frames}) == 3
        return frames, [off @ T for T in Ts], got[0][2]

    def restated(self, kps, desc, pose0, window=SCAN_WINDOW, local_map=None, **kw):
        """pass 1 at radius 15 in numpy, through the vectorised local map unless another is given"""
        lm = scan_local_map(self, window) if local_map is None else local_map
        W, H = self.image_size
        return TR.track(self.K, pose0, self.xyz, self.obs_off, self.obs_kf, self.obs_kp, self.kf_desc, self.kf_oct, kps, desc, W, H,
                        window=window, radii=(15.0,), refine_pose=False, local_map=lm, **kw)


def scan_local_map(w, window):
    """TR.local_map for a scan world, vectorised.  It states the rule these maps make simple: every key is valid and every point has
    two observations in different keyframes, so a point is local if either lies in the window; the representative is the first (both
    medians are 0, ties go to the earlier) and ref_octave is that row's octave.  Returns (rep, ref_octave list, n_local) as
    TR.local_map does."""
    n_kf = len(w.kf_desc)
    lo = n_kf - window if 0 < window < n_kf else 0
    kf, row = w.obs_kf.reshape(-1, 2), w.obs_kp.reshape(-1, 2)
    local = (kf >= lo).any(axis=1)
    D, O = np.stack(w.kf_desc), np.stack(w.kf_oct)
    rep = np.zeros((len(kf), 32), np.uint8)
    rep[local] = D[kf[local, 0], row[local, 0]]
    octv = O[kf[:, 0], row[:, 0]].tolist()
    ref = [o if l else None for o, l in zip(octv, local.tolist())]
    return rep, ref, int(local.sum())


_S = {}


def scan_world():
    if "w" not in _S:
        _S["w"] = ScanWorld()
    return _S["w"]


def small_scan_world():
    """the same construction at 3000 points, for comparing scan_local_map with TR.local_map"""
    if "small" not in _S:
        _S["small"] = ScanWorld(n_pts=3000, split=1024, edge=100, rows=200, seed=42)
    return _S["small"]


def scan_case(window=SCAN_WINDOW):
    """(frames, pose0, marks, local map, restated first frame) of the scan world for a window, derived once"""
    if ("case", window) not in _S:
        w = scan_world()
        if "q" not in _S:
            _S["q"] = w.queries()
        frames, pose0, marks = _S["q"]
        lm = scan_local_map(w, window)
        _S["case", window] = (frames, pose0, marks, lm, w.restated(frames[0][0], frames[0][1], pose0[0], window=window, local_map=lm))
    return _S["case", window]


def build_scan_map(ctx, w):
    """the scan world as a device map: the keyframes through add_keyframe (random descriptors: no growth step finds a model), the points
    through one mo_map_add_points call on the arrays"""
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    n = len(w.xyz)
    m = LocalMapper(w.K, save_every_keyframe=False, context=ctx, capacity=(max(w.n_kf, 2), w.rows, n, 2 * n))
    img = np.zeros((w.image_size[1], w.image_size[0]), np.uint8)
    for k in range(w.n_kf):
        m.add_keyframe(img, kps_array(np.zeros((w.rows, 2)), w.kf_oct[k]), w.kf_desc[k], w.kf_poses[k])
        assert m.last["n_new"] == 0
    z = np.zeros(n, np.int32)
    arrays = (np.ascontiguousarray(w.xyz), np.zeros((n, 3), np.uint8), np.arange(n, dtype=np.int32), w.obs_off, w.obs_kf, w.obs_kp)
    m._check(m.lib.mo_map_add_points(m._h, n, *[V._ptr(a) for a in arrays], V._ptr(z - 1), V._ptr(z)))
    m._sync_size()
    assert len(m.keyframes) == w.n_kf and m._n_points == n
    return m
