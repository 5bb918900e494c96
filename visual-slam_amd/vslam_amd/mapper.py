"""LocalMapper on the device: the reference's orbslam2.local_mapper.LocalMapper (local_mapper.py) with its map held in HBM.

The keyframe store, the map points (positions, colours, ids, observations in CSR form) and the per-keyframe lists live in the
library's mo_map (map_kernels.hip).  One add_keyframe is one native call with one synchronisation: store -> growth of the
(previous, new) keyframe pair (ratio-0.8 knn match, fundamental-matrix RANSAC at 3 px, triangulation) -> cull of every map point ->
per-keyframe lists and the counts _cull_keyframes reads.  The host keeps what the reference's callers see: the keyframe dicts, a lazy
sequence of map-point dicts, the co-visibility graph.

Attach it to the reference's Tracker without editing the reference:
    Tracker(K, local_mapper=vslam_amd.mapper.LocalMapper(K, "map.ply"))
"""
from collections import defaultdict
from collections.abc import Sequence

import ctypes as C
import weakref

import numpy as np

import vslam_amd as V

_N_HYP = 1024
_SEED = 4096


def predict_pose(prev, last):
    """constant-velocity prediction of the next pose from the two before it (4x4, X_cam = R X + t): the motion prev -> last applied
    once more, (last @ inv(prev)) @ last"""
    prev, last = np.asarray(prev, np.float64), np.asarray(last, np.float64)
    return (last @ np.linalg.inv(prev)) @ last


def positions_sharing_points(a, counts, positions):
    """{position: set of the keyframe positions that validly observe a map point the position validly observes} (itself included once it
    observes anything) on the map arrays a; counts: rows per keyframe position.  An observation is read as the library reads it:
    negative positions and rows count from the end, entries that name nothing are skipped."""
    counts = np.asarray(counts, np.int64)
    n_kf, n = len(counts), len(a["obs_off"]) - 1
    if n_kf == 0 or n == 0:
        return {int(i): set() for i in positions}
    k, r = np.asarray(a["obs_kf"], np.int64), np.asarray(a["obs_kp"], np.int64)
    k = np.where(k < 0, k + n_kf, k)
    ok = (k >= 0) & (k < n_kf)
    kc = np.clip(k, 0, n_kf - 1)
    r = np.where(r < 0, r + counts[kc], r)
    ok &= (r >= 0) & (r < counts[kc])
    pt = np.repeat(np.arange(n), np.diff(np.asarray(a["obs_off"], np.int64)))[ok]
    k = k[ok]
    out = {}
    for i in positions:
        sees = np.zeros(n, bool)
        sees[pt[k == i]] = True
        out[int(i)] = set(np.unique(k[sees[pt]]).tolist())
    return out


class _Keyframe(dict):
    """a keyframe dict whose 'map_points' is read from the mapper's per-keyframe lists when asked for"""
    __slots__ = ("_mapper", "_extra", "_rows")

    def __getitem__(self, key):
        if key == "map_points" and not dict.__contains__(self, "map_points"):
            return self._mapper._kf_list(self)
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        return self[key] if key in self else default

    def __contains__(self, key):
        return key == "map_points" or dict.__contains__(self, key)


class _MapPoints(Sequence):
    """LocalMapper.map_points: a Sequence of dicts materialised from the device map on access (one download per map version)"""

    def __init__(self, mapper):
        self._m = mapper

    def __len__(self):
        return self._m._n_points

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("map point index out of range")
        return self._m._point(i)

    def __iter__(self):
        for i in range(len(self)):
            yield self._m._point(i)

    def __bool__(self):
        return len(self) > 0


class LocalMapper:
    """Same public methods and attributes as the reference's LocalMapper, with the same results.  Differences: map_points is a lazy
    sequence (the dicts are built when read), get_map_statistics also works between update_map_points and the next keyframe (the
    reference raises KeyError there on points without 'observed_keyframes'), positions of injected points are stored as float32."""

    def __init__(self, camera_matrix, output_path=None, save_every_keyframe=True, context=None, n_hyp=_N_HYP, seed=_SEED,
                 pair_index_base=0, capacity=(64, 2048, 1 << 16, 1 << 17)):
        self._init_host_state(camera_matrix, output_path, save_every_keyframe, context, n_hyp, seed, pair_index_base)
        kf_slots, rows, pts, obs = capacity
        h = self.lib.mo_map_create(self.ctx.h, int(kf_slots), int(rows), int(pts), int(obs))
        if not h:
            raise V.NativeError(V.MO_ERR_HIP, self.lib.mo_last_error(self.ctx.h).decode())
        self._adopt(h)

    def _init_host_state(self, camera_matrix, output_path, save_every_keyframe, context, n_hyp, seed, pair_index_base):
        """every host attribute of a mapper without a device map yet (the constructor and load_state both start here)"""
        self.camera_matrix = camera_matrix
        self.keyframes = []
        self.output_path = output_path if output_path else "map.ply"
        self.co_visibility_graph = defaultdict(lambda: defaultdict(int))
        self.redundancy_threshold = 0.9
        self.min_observations = 2
        self.culling_threshold = 0.05
        self.save_every_keyframe = save_every_keyframe
        self.n_hyp, self.seed, self.pair_index_base = int(n_hyp), int(seed), int(pair_index_base)
        self.ctx = context if context is not None else V.default_context()
        self.lib = self.ctx.lib
        self._h = None
        self._records = []        # every keyframe dict ever added, by ordinal (the descriptor references; on a loaded mapper a removed keyframe's entry is None or holds the rows points still name)
        self._rec_n = []          # their keypoint counts
        self._injected = []       # the dicts given to update_map_points (dref_kf = -(j + 1))
        self._n_points = 0
        self._list_rows = []      # keyframe position -> row of the per-keyframe lists (None: empty list)
        self._kf_serials = []     # keyframe position -> creation serial (positions are renumbered by every keyframe cull, serials never)
        self._next_serial = 0
        self._loop_consistency = None
        self._version = 0
        self._cache = None
        self._lists = None
        self._image_size = None   # load_state: (w, h) of the saved last keyframe's image, for when no keyframe dict carries one
        self.last = None          # the growth step of the last add_keyframe (match lists, inlier mask, F, new points)
        self.map_points = _MapPoints(self)
        self.vocabulary = None

    def _adopt(self, handle):
        """the device map of this mapper; closing the context closes it first"""
        self._h = handle
        if not hasattr(self.ctx, "_maps"):
            self.ctx._maps = weakref.WeakSet()
        self.ctx._maps.add(self)

    def _default_image_size(self):
        """(w, h) a projection must land in when the caller names none: the last keyframe's image (on a loaded mapper the latest
        keyframe that carries one, else the saved one's size), else twice the principal point"""
        for kf in reversed(self.keyframes):
            if kf["image"] is not None:
                return kf["image"].shape[1::-1]
        if self._image_size is not None:
            return self._image_size
        Km = np.asarray(self.camera_matrix, np.float64)
        return (max(int(round(2 * Km[0, 2])), 1), max(int(round(2 * Km[1, 2])), 1))

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "h", None):
            self.lib.mo_map_destroy(self._h)
        self._h = None
        self.vocabulary = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc == V.MO_ERR_INDEX:
            raise IndexError(self.lib.mo_last_error(self.ctx.h).decode())
        if rc != V.MO_OK:
            raise V.NativeError(rc, self.lib.mo_last_error(self.ctx.h).decode())

    def set_output_path(self, output_path):
        self.output_path = output_path

    # ---- the reference's per-keyframe step ------------------------------------------------------------------------------------
    def add_keyframe(self, image, keypoints, descriptors, pose, tracked=None):
        """tracked: (point, inlier) as track_local_map returned them for this very frame against the map as it stands; the inlier
        matches become observations of their map points in this keyframe (add_observations) before the growth step and the cull, and
        the co-visibility graph gets the shared-point counts.  None: the reference's step alone."""
        from orbslam2.types import keypoints_to_array
        from orbslam2.utils import compute_projection_matrix
        kf = _Keyframe({"id": len(self.keyframes), "image": image.copy(), "keypoints": keypoints, "descriptors": descriptors,
                        "pose": pose.copy()})
        kf._mapper = self
        kf._extra = []   # ids appended by a growth step whose cull raised (the reference's lists at that point)
        kf._rows = 0     # its keypoint rows in the store (set below)
        slot = len(self._records)
        token = V.resident_token(self.ctx, descriptors) if descriptors is not None else 0
        kps_arr = V._resident_kps(descriptors) if token else None
        if kps_arr is None or len(kps_arr) != len(keypoints):
            token = 0
            if isinstance(keypoints, np.ndarray) and keypoints.dtype == V.KP_DTYPE:
                kps_arr = keypoints
            else:
                kps_arr = keypoints_to_array(keypoints) if len(keypoints) else np.zeros(0, V.KP_DTYPE)
        kps_arr = np.ascontiguousarray(kps_arr, V.KP_DTYPE).reshape(-1)
        desc = np.ascontiguousarray(descriptors if descriptors is not None else np.zeros((0, 32), np.uint8), np.uint8).reshape(-1, 32)
        n = len(kps_arr) if token else min(len(kps_arr), len(desc))
        ref = V.FrameRef(token, V._ptr(kps_arr), V._ptr(desc), n)
        kf._rows = n
        P = np.ascontiguousarray(compute_projection_matrix(pose[:3, :3], pose[:3, 3], self.camera_matrix), np.float64).reshape(12)
        img = np.ascontiguousarray(image, np.uint8)
        ch = 1 if img.ndim == 2 else img.shape[2]
        n_prev = self.keyframes[-1]._rows if self.keyframes else 0   # (the last keyframe in the map, which an absorb or an erase may leave different from the last record)
        n_kf = len(self.keyframes) + 1
        midx = np.full((max(n_prev, 1), 2), -1, np.int32)
        mpass = np.zeros(max(n_prev, 1), np.uint8)
        inl = np.zeros(max(n_prev, 1), np.uint8)
        gpts = np.full((max(n_prev, 1), 3), np.nan, np.float32)
        kf_len = np.zeros(n_kf, np.int32)
        kf_red = np.zeros(n_kf, np.int32)
        prm = V.MapKfParams(0.8, 3.0, self.n_hyp, self.seed, self.pair_index_base + max(slot - 1, 0))
        out = V.MapKfOut(midx.ctypes.data, mpass.ctypes.data, inl.ctypes.data, gpts.ctypes.data, kf_len.ctypes.data, kf_red.ctypes.data)
        self.keyframes.append(kf)
        self._kf_serials.append(self._next_serial)
        self._next_serial += 1
        self._records.append(kf)
        self._version += 1
        self._cache = None
        self._lists = None
        shared = self._add_tracked(n_kf - 1, tracked) if tracked is not None else None
        rc = self.lib.mo_map_add_keyframe(self._h, C.byref(ref), V._ptr(P), V._ptr(img), img.shape[1], img.shape[0], ch, C.byref(prm), C.byref(out))
        self._rec_n.append(n)
        if shared and rc == V.MO_OK:
            for other_id, cnt in shared.items():
                self.co_visibility_graph[other_id][kf["id"]] += cnt
                self.co_visibility_graph[kf["id"]][other_id] += cnt
        n_before = self._n_points
        self._sync_size()
        if rc == V.MO_ERR_INDEX:
            # the reference raises inside _cull_map_points: the grown points, their list entries and the co-visibility increments
            # are already there (local_mapper.py:171-187); the lists of the previous cull stay as they were
            new = list(range(n_before, n_before + int(out.n_new)))
            if new:
                self.keyframes[-2]._extra.extend(new); kf._extra.extend(new)
                self.co_visibility_graph[self.keyframes[-2]["id"]][kf["id"]] += len(new)
                self.co_visibility_graph[kf["id"]][self.keyframes[-2]["id"]] += len(new)
            self._list_rows.append(None)
        self._check(rc)
        self.last = {"match_idx": midx[:n_prev], "match_pass": mpass[:n_prev].astype(bool), "inlier": inl[:n_prev].astype(bool),
                     "points": gpts[:n_prev], "kf_len": kf_len, "kf_redundant": kf_red,
                     "F": np.array(out.F).reshape(3, 3), "n_new": int(out.n_new), "from_token": bool(out.from_token)}
        if n_kf >= 2 and out.n_new > 0:
            prev_id, cur_id = self.keyframes[-2]["id"], kf["id"]
            self.co_visibility_graph[prev_id][cur_id] += int(out.n_new)
            self.co_visibility_graph[cur_id][prev_id] += int(out.n_new)
        if n_kf < 2:   # (local_mapper.py:75: no map update, no save, before the second keyframe)
            self._list_rows = [None]
            return
        self._list_rows = list(range(n_kf))
        for k in self.keyframes:
            k._extra = []
        if len(self.keyframes) > 3:
            self._cull_keyframes(kf_len, kf_red)
        if self.save_every_keyframe:
            self._save_map()

    # ---- tracked observations and bundle adjustment ---------------------------------------------------------------------------------
    def _add_tracked(self, kf_pos, tracked):
        """the inlier matches of a tracked frame as observations of keyframe position kf_pos (the keyframe being added); returns
        {keyframe id: points shared with it} over the keyframes (positions before this one) the gaining points are observed in"""
        point, inlier = tracked
        point = np.asarray(point, np.int64).reshape(-1)
        inlier = np.asarray(inlier).reshape(-1).astype(bool)
        if len(point) != len(inlier):
            raise ValueError("tracked: point and inlier must have one entry per keypoint")
        pt = np.where(inlier, point, -1).astype(np.int32)
        if not (pt >= 0).any() or self._n_points == 0:
            return {}
        a = self.arrays()
        rows = np.flatnonzero((pt >= 0) & (pt < self._n_points))
        gained = np.unique(pt[rows])                      # (the new keyframe holds no observation yet: every named point gains one)
        self.add_observations(kf_pos, pt)
        n_before = kf_pos                                 # keyframes in the store
        off, okf = a["obs_off"], a["obs_kf"]
        ent = np.concatenate([np.arange(off[i], off[i + 1]) for i in gained.tolist()]) if len(gained) else np.zeros(0, np.int64)
        pos = okf[ent.astype(np.int64)].astype(np.int64)
        pos = np.where(pos < 0, pos + n_before, pos)
        pos = pos[(pos >= 0) & (pos < n_before)]
        shared = {}
        for p_, cnt in zip(*np.unique(pos, return_counts=True)):
            shared[self.keyframes[int(p_)]["id"]] = int(cnt)
        return shared

    def add_observations(self, kf_position, point, row=None):
        """Appends the observation (kf_position, row[i]) to map point point[i] (index into the map as it stands); row defaults to
        0, 1, 2, ... (point has one entry per keypoint of that keyframe, -1: none).  Skipped: point < 0 or out of range, a point that
        already has a valid observation in that keyframe; of two entries naming one point the first wins (mo_map_add_observations).
        kf_position == len(keyframes) names the keyframe the next add_keyframe stores."""
        pt = np.ascontiguousarray(np.asarray(point).reshape(-1), np.int32)
        rw = np.arange(len(pt), dtype=np.int32) if row is None else np.ascontiguousarray(np.asarray(row).reshape(-1), np.int32)
        if len(rw) != len(pt):
            raise ValueError("point and row must have the same length")
        self._check(self.lib.mo_map_add_observations(self._h, int(kf_position), len(pt), V._ptr(pt), V._ptr(rw)))
        self._version += 1
        self._cache = None
        self._sync_size()

    def bundle_adjust(self, window=10, scale_factor=1.2, chi2=5.991, min_inliers=50, max_steps=(5, 10), want_points=False, local="window",
                      kf_position=-1, n_best=15, min_weight=15, free=None, erase_outliers=False):
        """Local bundle adjustment on the map as it stands (ORB-SLAM2's LocalBundleAdjustment; mo_map_bundle_adjust in
        include/vslam_amd.h states the rules): the poses of the last `window` keyframes (0: all, at most 16, never the first) and the
        positions of the points they see are refined together, the other keyframes seeing those points held fixed.  The refined poses
        are written into kf["pose"] of the free keyframes (into the array), the map points move on the device.
        Returns (ok, info): info holds n_free, n_fixed, n_local, n_edges, n_inliers, cost (3), steps / accepted per round, `free` and
        `fixed` position lists, `edge_inlier` per observation entry (0 outside, 1 inlier, 2 outlier), `poses` [n_kf][3][4] and, with
        want_points, `points` [n_points][3] f64 (NaN for points outside the problem).
        The set form (mo_map_bundle_adjust_local; `window` is then not used): local="covisible" frees keyframe `kf_position` (-1: the
        last) and its `n_best` (0 .. 15) heaviest covisible neighbours sharing at least `min_weight` points with it, selected on the
        device; free= (positions, or a bool mask with one entry per keyframe; at most 16 besides position 0) frees exactly those.
        Position 0 is never free.  erase_outliers=True erases the observation entries the adjustment ended with as outliers
        (edge_inlier == 2) in the same device chain, when the adjustment is ok; points left with fewer than two entries stay and are
        counted (cull_map_points' orphan rule removes them).  With any of these info also holds `candidates` (the positions of the
        set, before the gauge), `n_erased` and `n_under`; edge_inlier is indexed by the entries as they were before the erase."""
        if local not in ("window", "covisible"):
            raise ValueError("local must be 'window' or 'covisible'")
        set_form = local == "covisible" or free is not None or bool(erase_outliers)
        n_kf = len(self.keyframes)
        poses = np.zeros((max(n_kf, 1), 12), np.float64)
        for i, kf in enumerate(self.keyframes):
            poses[i] = np.asarray(kf["pose"], np.float64)[:3, :4].reshape(12)
        K = np.ascontiguousarray(self.camera_matrix, np.float64).reshape(9)
        poses_out = poses.copy()
        state = np.zeros(max(n_kf, 1), np.int32)
        n_obs_before = self._n_obs if self._n_points else 0
        einl = np.zeros(max(n_obs_before, 1), np.uint8)
        pts = np.full((max(self._n_points, 1), 3), np.nan, np.float64) if want_points else None
        ms = [int(v) for v in max_steps]
        if len(ms) != 2:
            raise ValueError("max_steps: one count per round")
        prm = V.MapBaParams(int(window), int(min_inliers), (C.c_int32 * 2)(*ms), float(scale_factor), float(chi2))
        out = V.MapBaOut(poses_out.ctypes.data, state.ctypes.data, einl.ctypes.data, pts.ctypes.data if want_points else None)
        if set_form:
            fmask = None
            if free is not None:
                sel = np.asarray(free)
                if sel.dtype == np.bool_:
                    if sel.shape != (n_kf,):
                        raise ValueError("a mask must have one entry per keyframe")
                    fmask = np.ascontiguousarray(sel, np.uint8)
                else:
                    idx = sel.astype(np.int64).reshape(-1)
                    if len(idx) and (idx.min() < 0 or idx.max() >= n_kf):
                        raise IndexError("keyframe position out of range")
                    fmask = np.zeros(n_kf, np.uint8)
                    fmask[idx] = 1
                fmask = np.concatenate([fmask, np.zeros(1, np.uint8)])   # (never empty)
            elif local == "window":   # erase_outliers alone: the window's own set
                lo = n_kf - int(window) if 0 < int(window) < n_kf else 0
                fmask = np.zeros(n_kf + 1, np.uint8)
                fmask[lo:n_kf] = 1
            cand = np.zeros(max(n_kf, 1), np.uint8)
            lprm = V.MapBaLocalParams(fmask.ctypes.data if fmask is not None else None, int(kf_position), int(n_best), int(min_weight),
                                      1 if erase_outliers else 0)
            lout = V.MapBaLocalOut(cand.ctypes.data)
            self._check(self.lib.mo_map_bundle_adjust_local(self._h, V._ptr(K), V._ptr(poses), C.byref(prm), C.byref(lprm), C.byref(out), C.byref(lout)))
        else:
            self._check(self.lib.mo_map_bundle_adjust(self._h, V._ptr(K), V._ptr(poses), C.byref(prm), C.byref(out)))
        state = state[:n_kf]
        free = np.flatnonzero(state == 2).tolist()
        if out.n_free:
            for i in free:
                self.keyframes[i]["pose"][:3, :4] = poses_out[i].reshape(3, 4)
            self._version += 1
            self._cache = None
        info = {"n_free": int(out.n_free), "n_fixed": int(out.n_fixed), "n_local": int(out.n_local), "n_edges": int(out.n_edges),
                "n_inliers": int(out.n_inliers), "cost": [float(v) for v in out.cost], "steps": [int(v) for v in out.steps],
                "accepted": [int(v) for v in out.accepted], "lambda": float(out.lambda_), "free": free,
                "fixed": np.flatnonzero(state == 1).tolist(), "edge_inlier": einl[:n_obs_before],
                "poses": poses_out[:n_kf].reshape(n_kf, 3, 4)}
        if want_points:
            info["points"] = pts[:self._n_points]
        if set_form:
            info.update(candidates=np.flatnonzero(cand[:n_kf]).tolist(), n_erased=int(lout.n_erased), n_under=int(lout.n_under))
            if info["n_erased"]:
                self._version += 1
                self._cache = None
                self._sync_size()
        return bool(out.ok), info

    def erase_observations(self, entries_or_mask):
        """Removes single entries of the observation arrays on the device (mo_map_erase_observations): every point keeps its index, its
        fields and its life record, the surviving entries their order and bytes; a point may end with no entries.  entries_or_mask: entry
        indices into obs_kf / obs_kp, or a bool mask with one entry per observation entry.  Returns {"n_erased", "n_under" (the points
        that lost an entry and now hold fewer than two), "n_obs"}."""
        n = self._n_obs if self._n_points else 0
        sel = np.asarray(entries_or_mask)
        if sel.dtype == np.bool_:
            if sel.shape != (n,):
                raise ValueError("a mask must have one entry per observation entry")
            mask = np.ascontiguousarray(sel, np.uint8)
        else:
            idx = sel.astype(np.int64).reshape(-1)
            if len(idx) and (idx.min() < 0 or idx.max() >= n):
                raise IndexError("observation entry out of range")
            mask = np.zeros(n, np.uint8)
            mask[idx] = 1
        out = V.MapObsEraseOut()
        self._check(self.lib.mo_map_erase_observations(self._h, V._ptr(mask) if n else None, C.byref(out)))
        if int(out.n_erased):
            self._version += 1
            self._cache = None
            self._sync_size()
        return {"n_erased": int(out.n_erased), "n_under": int(out.n_under), "n_obs": int(out.n_obs)}

    def global_bundle_adjust(self, fixed=None, max_steps=10, max_cg=200, cg_tol=1e-8, step_tol=1e-10, min_inliers=50, scale_factor=1.2,
                             chi2=5.991, want_points=False):
        """Global bundle adjustment on the map as it stands (ORB-SLAM2's GlobalBundleAdjustemnt, the step behind a loop correction and
        optimize_essential_graph; mo_map_global_ba in include/vslam_amd.h states the rules): the poses of all keyframes that are not
        held fixed and every point with at least two observations are refined together, with no limit on the number of keyframes: the
        reduced camera system is solved matrix-free by a preconditioned conjugate gradient.  `fixed`: the positions that stay; None:
        position 0 only (the scale is then held by the damping alone).  One robust round of at most max_steps steps; no observation is
        erased.  The refined poses are written into kf["pose"] of the free keyframes when a step was accepted, the points move on the
        device.
        Returns (ok, info): info holds n_free, n_fixed, n_points, n_edges, n_inliers, cost (start, end), lambda, steps, accepted,
        cg_iters, `free` and `fixed` position lists, `edge_inlier` per observation entry (0 outside, 1 inlier, 2 outlier), `poses`
        [n_kf][3][4] and, with want_points, `points` [n_points][3] f64 (NaN for points outside the problem)."""
        n_kf = len(self.keyframes)
        poses = np.zeros((max(n_kf, 1), 12), np.float64)
        for i, kf in enumerate(self.keyframes):
            poses[i] = np.asarray(kf["pose"], np.float64)[:3, :4].reshape(12)
        K = np.ascontiguousarray(self.camera_matrix, np.float64).reshape(9)
        fmask = None
        if fixed is not None:
            fmask = np.zeros(max(n_kf, 1), np.uint8)
            for k in fixed:
                if 0 <= int(k) < n_kf:
                    fmask[int(k)] = 1
        poses_out = poses.copy()
        state = np.zeros(max(n_kf, 1), np.int32)
        n_obs = self._n_obs if self._n_points else 0
        einl = np.zeros(max(n_obs, 1), np.uint8)
        pts = np.full((max(self._n_points, 1), 3), np.nan, np.float64) if want_points else None
        prm = V.MapGbaParams(fmask.ctypes.data if fmask is not None else None, int(max_steps), int(max_cg), float(cg_tol), float(step_tol),
                             int(min_inliers), float(scale_factor), float(chi2))
        out = V.MapGbaOut(poses_out.ctypes.data, state.ctypes.data, einl.ctypes.data, pts.ctypes.data if want_points else None)
        self._check(self.lib.mo_map_global_ba(self._h, V._ptr(K), V._ptr(poses), C.byref(prm), C.byref(out)))
        state = state[:n_kf]
        free = np.flatnonzero(state == 2).tolist()
        if out.accepted:
            for i in free:
                self.keyframes[i]["pose"][:3, :4] = poses_out[i].reshape(3, 4)
            self._version += 1
            self._cache = None
        info = {k: int(getattr(out, k)) for k in ("n_free", "n_fixed", "n_points", "n_edges", "n_inliers", "steps", "accepted", "cg_iters")}
        info.update(cost=[float(v) for v in out.cost], free=free, fixed=np.flatnonzero(state == 1).tolist(), edge_inlier=einl[:n_obs],
                    poses=poses_out[:n_kf].reshape(n_kf, 3, 4))
        info["lambda"] = float(out.lambda_)
        if want_points:
            info["points"] = pts[:self._n_points]
        return bool(out.ok), info

    # ---- fusion of duplicate map points ---------------------------------------------------------------------------------------------
    def _valid_positions(self, a, i, counts):
        """the keyframe positions map point i of the arrays a validly observes (the library's reading of an observation)"""
        n_kf = len(counts)
        out = set()
        for o in range(int(a["obs_off"][i]), int(a["obs_off"][i + 1])):
            k, r = int(a["obs_kf"][o]), int(a["obs_kp"][o])
            k = k + n_kf if k < 0 else k
            if not 0 <= k < n_kf:
                continue
            r = r + counts[k] if r < 0 else r
            if 0 <= r < counts[k]:
                out.add(k)
        return out

    def fuse_map_points(self, window=10, radius=3.0, scale_factor=1.2, max_dist=50, chi2=5.991, image_size=None, frustum=False, n_levels=8,
                        view_range=(0.8, 1.2), min_cos=0.5):
        """Merges map points that are the same 3D feature and gives points the observations they lack (ORB-SLAM2's SearchInNeighbors /
        Fuse / Replace; mo_map_fuse in include/vslam_amd.h states the rules): every point the last `window` keyframes (0: all) see is
        projected, under the store's own projection matrices, into each of those keyframes that does not observe it; a keypoint it
        matches within `radius` (at octave 0), `chi2` and `max_dist` either belongs to another point - the two are merged, the one with
        more observations survives and takes the other's - or to none, and becomes an observation of the point.  image_size as in
        track_local_map.  The co-visibility graph follows: per changed point, the keyframe pairs that observe it after the call less
        those that observed its parts before.
        frustum=True (mo_map_fuse_frustum): a point is projected into a keyframe only when that keyframe's centre lies within view_range
        of the point's scale-invariance range and within acos(min_cos) of its mean viewing direction (point_views), and it is searched at
        the pyramid level L its distance predicts, against keypoints of octave L - 1 or L; n_cand then counts those.  n_levels: the
        extractor's pyramid levels.
        Returns info: n_targets, n_local, n_pairs, n_cand, n_proposals, n_gained, n_edges, n_absorbed, n_points, n_obs and `into`
        (the new index of the point each old point now is)."""
        if image_size is None:
            image_size = self._default_image_size()
        n0 = self._n_points
        before = self.arrays() if n0 else None
        into = np.arange(max(n0, 1), dtype=np.int32)
        prm = V.MapFuseParams(int(image_size[0]), int(image_size[1]), int(window), float(radius), float(scale_factor), int(max_dist), float(chi2))
        out = V.MapFuseOut(into.ctypes.data)
        if frustum:
            fprm = V.MapFrustumParams(int(n_levels), float(view_range[0]), float(view_range[1]), float(min_cos))
            self._check(self.lib.mo_map_fuse_frustum(self._h, C.byref(prm), C.byref(fprm), C.byref(out)))
        else:
            self._check(self.lib.mo_map_fuse(self._h, C.byref(prm), C.byref(out)))
        into = into[:n0]
        self._version += 1
        self._cache = None
        self._sync_size()
        info = {k: int(getattr(out, k)) for k in ("n_targets", "n_local", "n_pairs", "n_cand", "n_proposals", "n_gained", "n_edges", "n_absorbed",
                                                  "n_points", "n_obs")}
        info["into"] = into
        if info["n_proposals"]:
            self._fuse_co_visibility(before, self.arrays(), into)
        return info

    def _fuse_co_visibility(self, before, after, into):
        slot_of = {id(r): s for s, r in enumerate(self._records)}
        counts = [self._rec_n[slot_of[id(kf)]] for kf in self.keyframes]
        members = np.bincount(into, minlength=len(after["id"]))
        n_before, n_after = np.diff(before["obs_off"]), np.diff(after["obs_off"])
        changed = np.unique(into[(members[into] > 1) | (n_before != n_after[into])])
        if not len(changed):
            return
        order = np.argsort(into, kind="stable")
        first = np.searchsorted(into[order], changed)
        delta = defaultdict(int)

        def pairs(pos, sign):
            pos = sorted(pos)
            for x in range(len(pos)):
                for y in range(x + 1, len(pos)):
                    delta[(pos[x], pos[y])] += sign
        for j, f in zip(changed.tolist(), first.tolist()):
            pairs(self._valid_positions(after, j, counts), 1)
            for i in order[f:f + members[j]].tolist():
                pairs(self._valid_positions(before, i, counts), -1)
        g = self.co_visibility_graph
        for (p, q), d in delta.items():
            if d:
                a, b = self.keyframes[p]["id"], self.keyframes[q]["id"]
                g[a][b] = max(0, g[a][b] + d)
                g[b][a] = max(0, g[b][a] + d)

    # ---- new map points from neighbour keyframes ------------------------------------------------------------------------------------
    def create_new_map_points(self, window=10, max_dist=50, scale_factor=1.2, epi_chi2=3.84, chi2=5.991, cos_max=0.9998, want_points=False,
                              ratio_factor=None, epipole_r2=100.0):
        """New map points for the last keyframe from its `window` neighbours (0: every earlier keyframe; ORB-SLAM2's CreateNewMapPoints /
        SearchForTriangulation; mo_map_grow in include/vslam_amd.h states the rules): every keypoint of the last keyframe that no map
        point observes is searched along its epipolar line among the unobserved keypoints of each neighbour (`epi_chi2`, `max_dist`),
        triangulated from the match with the most parallax (`cos_max`) and kept when depth, reprojection error (`chi2`) and scale
        consistency (ratio_factor, by default 1.5 * scale_factor) hold; its other matches become observations.  The poses are the
        keyframes' kf["pose"].  The co-visibility graph gains 1 for every pair of keyframes in each new point's observations.
        Returns info: n_neighbours, n_free, n_epi, n_accepted, n_matches, n_new, n_obs_new, n_points, n_obs, `point` (per keypoint of
        the last keyframe the index of the map point it created, -1: none) and, with want_points, `points` [n_new][3] f64."""
        n_kf = len(self.keyframes)
        poses = np.zeros((max(n_kf, 1), 12), np.float64)
        for i, kf in enumerate(self.keyframes):
            poses[i] = np.asarray(kf["pose"], np.float64)[:3, :4].reshape(12)
        K = np.ascontiguousarray(self.camera_matrix, np.float64).reshape(9)
        n_rows = self._rec_n[next(s for s, r in enumerate(self._records) if r is self.keyframes[-1])] if n_kf else 0
        point = np.full(max(n_rows, 1), -1, np.int32)
        pts = np.full((max(n_rows, 1), 3), np.nan, np.float64) if want_points else None
        rf = 1.5 * float(scale_factor) if ratio_factor is None else float(ratio_factor)
        prm = V.MapGrowParams(int(window), int(max_dist), float(scale_factor), float(epi_chi2), float(chi2), float(cos_max), rf, float(epipole_r2))
        out = V.MapGrowOut(point.ctypes.data, pts.ctypes.data if want_points else None)
        n0 = self._n_points   # (the map before the call: the new points are appended behind it)
        self._check(self.lib.mo_map_grow(self._h, V._ptr(K), V._ptr(poses), C.byref(prm), C.byref(out)))
        self._version += 1
        self._cache = None
        self._sync_size()
        info = {k: int(getattr(out, k)) for k in ("n_neighbours", "n_free", "n_epi", "n_accepted", "n_matches", "n_new", "n_obs_new", "n_points",
                                                  "n_obs")}
        info["point"] = point[:n_rows]
        if want_points:
            info["points"] = pts[:info["n_new"]]
        if info["n_new"]:
            a = self.arrays()
            g = self.co_visibility_graph
            for i in range(n0, self._n_points):   # (written non-negative, one entry per position)
                pos = a["obs_kf"][a["obs_off"][i]:a["obs_off"][i + 1]].tolist()
                for x in range(len(pos)):
                    for y in range(x + 1, len(pos)):
                        p, q = self.keyframes[pos[x]]["id"], self.keyframes[pos[y]]["id"]
                        g[p][q] += 1
                        g[q][p] += 1
        return info

    def _cull_keyframes(self, kf_len, kf_red):
        """local_mapper.py:253-315 on the counts the device produced: list length and the listed ids whose first map point with
        that id has >= 3 observations in other keyframes"""
        remove = []
        for i in range(1, len(self.keyframes) - 2):
            if kf_len[i] < 20:
                continue
            if kf_red[i] / kf_len[i] > self.redundancy_threshold:
                remove.append(i)
        if not remove:
            for i, kf in enumerate(self.keyframes):
                kf["id"] = i
            return
        self._forget_keyframes(remove)
        pos = np.array(sorted(remove), np.int32)
        self._check(self.lib.mo_map_remove_keyframes(self._h, V._ptr(pos), len(pos)))
        for i, kf in enumerate(self.keyframes):
            kf["id"] = i

    def _forget_keyframes(self, remove):
        """the host's part of removing the keyframes at the positions `remove` (the loop that ends the reference's _cull_keyframes):
        their co-visibility entries, their dicts, list rows and serials; the caller renumbers the ids"""
        for idx in sorted(remove, reverse=True):
            kf_id = self.keyframes[idx]["id"]
            for other in self.co_visibility_graph[kf_id]:
                if other != kf_id:
                    del self.co_visibility_graph[other][kf_id]
            del self.co_visibility_graph[kf_id]
            self.keyframes.pop(idx)
            self._list_rows.pop(idx)
            self._kf_serials.pop(idx)

    # ---- keyframe culling by ORB-SLAM2's rule ---------------------------------------------------------------------------------------
    def _keyframes_erased(self, removed):
        """behind a device erase: _cull_keyframes' bookkeeping, and every cached view of the map dropped"""
        self._forget_keyframes(removed)
        for i, kf in enumerate(self.keyframes):
            kf["id"] = i
        self._version += 1
        self._cache = None
        self._lists = None
        self._sync_size()

    def cull_keyframes(self, kf_position=-1, min_weight=15, min_observers=3, ratio=0.9, scale_gap=1, protect=None, erase=True, walk=0):
        """ORB-SLAM2's KeyFrameCulling asked from keyframe `kf_position` (-1: the last), decided on the device from the map as it stands
        (mo_map_kf_redundancy / mo_map_cull_keyframes in include/vslam_amd.h state the rules): the candidates are the positions sharing
        at least max(min_weight, 1) map points with it, most shared points first; one is removed when more than `ratio` of the points it
        observes are observed by at least `min_observers` other keyframes at an octave no coarser than its own + `scale_gap`, keyframes
        removed earlier in the same call not counting.  Position 0 and the positions where `protect` ([n_kf], non-zero) is set stay.
        erase=True removes them from the map (erase_keyframes' rewrite, in the same device chain) and from the host's lists; erase=False
        only reports.  Returns (removed_positions, info): positions ascending, as they were before the call; info holds `pos`, `weight`,
        `n_points`, `n_redundant`, `removed` per candidate in candidate order, `n_local`, `n_removed` and `n_obs`."""
        n_kf = len(self.keyframes)
        names = ("pos", "weight", "n_points", "n_redundant", "removed")
        arr = {k: np.zeros(max(n_kf, 1), np.int32) for k in names}
        prot = None
        if protect is not None:
            prot = np.ascontiguousarray(np.asarray(protect).reshape(-1) != 0, np.uint8)
            if len(prot) != n_kf:
                raise ValueError("protect must have one entry per keyframe")
        prm = V.MapKfCullParams(int(kf_position), int(min_weight), int(min_observers), int(scale_gap), float(ratio),
                                prot.ctypes.data if prot is not None and n_kf else None, 1 if erase else 0, int(walk))
        out = V.MapKfCullOut(*[arr[k].ctypes.data for k in names])
        self._check(self.lib.mo_map_cull_keyframes(self._h, C.byref(prm), C.byref(out)))
        n_local = int(out.n_local)
        info = {k: arr[k][:n_local].copy() for k in names}
        info["removed"] = info["removed"].astype(bool)
        info.update(n_local=n_local, n_removed=int(out.n_removed), n_obs=int(out.n_obs))
        removed = sorted(info["pos"][info["removed"]].tolist())
        assert len(removed) == info["n_removed"]
        if erase and removed:
            self._keyframes_erased(removed)
        return removed, info

    def erase_keyframes(self, positions):
        """Removes the keyframes at `positions` so that the map is the map that never had them (mo_map_erase_keyframes): every point
        keeps its valid observations at the surviving keyframes, keyed by the positions after the removal; the points themselves, and
        their indices, stay - also one left with a single observation or none.  The host's lists follow as after _cull_keyframes."""
        pos = np.ascontiguousarray(np.asarray(positions, np.int64).reshape(-1), np.int32)
        self._check(self.lib.mo_map_erase_keyframes(self._h, V._ptr(pos) if len(pos) else None, len(pos)))
        if len(pos):
            self._keyframes_erased(sorted(set(pos.tolist())))

    # ---- the life of a map point: found / visible counters, culling by ORB-SLAM2's rule -----------------------------------------------
    def point_life(self):
        """The life records of the map points (mo_map_point_life; include/vslam_amd.h states their rules): a dict of `visible` and
        `found` (ORB-SLAM2's mnVisible / mnFound), `born` (the ordinal of the last stored keyframe when the point was made), each (n,)
        int32, and `now` (that ordinal today).  Ordinals count the keyframes ever stored and never shift."""
        n = self._n_points
        life = np.zeros((max(n, 1), 4), np.int32)
        now = C.c_int64(0)
        self._check(self.lib.mo_map_point_life(self._h, V._ptr(life), C.byref(now)))
        life = life[:n]
        return {"visible": life[:, 0].copy(), "found": life[:, 1].copy(), "born": life[:, 2].copy(), "now": int(now.value)}

    def note_tracking(self, pose, info, window=10, local_keyframes=None, frustum=False, n_levels=8, view_range=(0.8, 1.2), min_cos=0.5,
                      scale_factor=1.2, image_size=None):
        """Records one tracked frame in the life records (mo_map_note_tracking): `visible` grows by one for every local point that the
        frame at `pose` (4x4) sees - its projection lies in the image and, with frustum=True, it passes track_local_map's frustum test
        with the same parameters - or that a keypoint was matched to; `found` by one for every point an inlier match names.  info:
        track_local_map's dict (`point`, `inlier`; its `local_keyframes`, when there, are the local map unless local_keyframes names
        positions itself; else the last `window` keyframes, 0: all).  Returns n_local, n_seen, n_matched, n_found."""
        if image_size is None:
            image_size = self._default_image_size()
        n_kf = len(self.keyframes)
        if local_keyframes is None:
            local_keyframes = info.get("local_keyframes")
        mask = None
        if local_keyframes is not None:
            mask = np.zeros(max(n_kf, 1), np.uint8)
            mask[np.asarray(local_keyframes, np.int64).reshape(-1)] = 1
        point = np.ascontiguousarray(np.asarray(info["point"]).reshape(-1), np.int32)
        inlier = np.ascontiguousarray(np.asarray(info["inlier"]).reshape(-1) != 0, np.uint8)
        if len(point) != len(inlier):
            raise ValueError("info: point and inlier must have one entry per keypoint")
        K = np.ascontiguousarray(self.camera_matrix, np.float64).reshape(9)
        pose12 = np.ascontiguousarray(np.asarray(pose, np.float64)[:3, :4]).reshape(12)
        fprm = V.MapFrustumParams(int(n_levels), float(view_range[0]), float(view_range[1]), float(min_cos)) if frustum else None
        prm = V.MapNoteParams(int(image_size[0]), int(image_size[1]), int(window), float(scale_factor), mask.ctypes.data if mask is not None else None,
                              C.addressof(fprm) if fprm is not None else None)
        out = V.MapNoteOut()
        self._check(self.lib.mo_map_note_tracking(self._h, V._ptr(K), V._ptr(pose12), C.byref(prm), len(point), V._ptr(point) if len(point) else None,
                                                  V._ptr(inlier) if len(point) else None, C.byref(out)))
        return {k: int(getattr(out, k)) for k in ("n_local", "n_seen", "n_matched", "n_found")}

    def _points_erased(self):
        """behind a device erase of map points: what add_keyframe does after its own compaction.  Nothing on the host is keyed by point
        index but the cached arrays (injected dicts are found through dref_kf, the per-keyframe lists hold ids and stay those of the last
        cull); the co-visibility graph keeps the reference's increments, as after add_keyframe's cull."""
        self._version += 1
        self._cache = None
        self._sync_size()

    def cull_map_points(self, ratio=0.25, min_age=2, max_age=3, max_obs=2, orphan_obs=1, protect=None, erase=True):
        """ORB-SLAM2's MapPointCulling decided on the device from the life records (mo_map_points_bad / mo_map_cull_points in
        include/vslam_amd.h state the rules).  With age = now - born, a point of age <= max_age (max_age < 0: any) is removed when
        found < ratio * visible (reason 1), or else when age >= min_age and at most max_obs keyframes observe it (reason 2); a point of
        any age when at most orphan_obs keyframes observe it (reason 3; -1: off).  Points where `protect` ([n], non-zero) is set report
        their reason and stay.  erase=True removes them in the same device chain (erase_map_points' rebuild); erase=False only reports.
        Returns (removed_indices, info): indices ascending, as before the call; info holds `reason` and `removed` per point, `n_tested`,
        `n_removed`, `n_reason` (4), `now`, `n_points`, `n_obs` and, when erasing, `remap` (new index per old point, -1: removed)."""
        n = self._n_points
        reason = np.zeros(max(n, 1), np.uint8)
        removed = np.zeros(max(n, 1), np.uint8)
        remap = np.arange(max(n, 1), dtype=np.int32)
        prot = None
        if protect is not None:
            prot = np.ascontiguousarray(np.asarray(protect).reshape(-1) != 0, np.uint8)
            if len(prot) != n:
                raise ValueError("protect must have one entry per map point")
        prm = V.MapPtCullParams(float(ratio), int(min_age), int(max_age), int(max_obs), int(orphan_obs),
                                prot.ctypes.data if prot is not None and n else None, 1 if erase else 0)
        out = V.MapPtCullOut(reason.ctypes.data, removed.ctypes.data, remap.ctypes.data)
        self._check(self.lib.mo_map_cull_points(self._h, C.byref(prm), C.byref(out)))
        info = {"reason": reason[:n], "removed": removed[:n].astype(bool), "n_tested": int(out.n_tested), "n_removed": int(out.n_removed),
                "n_reason": [int(x) for x in out.n_reason], "now": int(out.now), "n_points": int(out.n_points), "n_obs": int(out.n_obs)}
        gone = np.flatnonzero(info["removed"]).tolist()
        assert len(gone) == info["n_removed"]
        if erase:
            info["remap"] = remap[:n]
            if gone:
                self._points_erased()
        return gone, info

    def erase_map_points(self, indices_or_mask):
        """Removes map points so that the map is the map the others alone would have built (mo_map_erase_points): the survivors keep their
        order, every field, their life records and their observation entries as stored.  indices_or_mask: point indices, or a bool mask
        with one entry per point.  Returns remap (n,) int32: the new index of every old point, -1: removed."""
        n = self._n_points
        sel = np.asarray(indices_or_mask)
        if sel.dtype == np.bool_:
            if sel.shape != (n,):
                raise ValueError("a mask must have one entry per map point")
            mask = np.ascontiguousarray(sel, np.uint8)
        else:
            idx = sel.astype(np.int64).reshape(-1)
            if len(idx) and (idx.min() < 0 or idx.max() >= n):
                raise IndexError("map point index out of range")
            mask = np.zeros(n, np.uint8)
            mask[idx] = 1
        remap = np.arange(max(n, 1), dtype=np.int32)
        out = V.MapPtEraseOut()
        self._check(self.lib.mo_map_erase_points(self._h, V._ptr(mask) if n else None, V._ptr(remap), C.byref(out)))
        if int(out.n_removed):
            self._points_erased()
        return remap[:n]

    def update_map_points(self, new_map_points):
        """Appends the points as given.  Points without 'observed_keyframes' (the initializer's carry 'observed_frames') count as
        0 observations: the next keyframe culls them, as in the reference."""
        pts = list(new_map_points)
        if not pts:
            return
        n = len(pts)
        xyz = np.zeros((n, 3), np.float32)
        col = np.zeros((n, 3), np.uint8)
        ids = np.zeros(n, np.int32)
        off = np.zeros(n + 1, np.int32)
        okf, okp = [], []
        dkf = np.zeros(n, np.int32)
        drow = np.zeros(n, np.int32)
        for i, mp in enumerate(pts):
            xyz[i] = np.asarray(mp["position"], np.float64).reshape(3)
            c = np.asarray(mp.get("color", (0, 0, 0))).reshape(-1)
            col[i] = c[:3] if c.size >= 3 else np.repeat(c[:1], 3)
            ids[i] = int(mp.get("id", 0))
            obs = mp.get("observed_keyframes", {})
            for k, v in obs.items():
                okf.append(int(k)); okp.append(int(v))
            off[i + 1] = len(okf)
            self._injected.append(mp)
            dkf[i] = -len(self._injected)
        okf = np.array(okf if okf else [0], np.int32)
        okp = np.array(okp if okp else [0], np.int32)
        self._check(self.lib.mo_map_add_points(self._h, n, V._ptr(xyz), V._ptr(col), V._ptr(ids), V._ptr(off), V._ptr(okf), V._ptr(okp),
                                               V._ptr(dkf), V._ptr(drow)))
        self._version += 1
        self._cache = None
        self._sync_size()

    # ---- relocalization -----------------------------------------------------------------------------------------------------------
    # ---- place recognition ----------------------------------------------------------------------------------------------------------
    def set_vocabulary(self, vocabulary):
        """Attaches a vslam_amd.Vocabulary (None detaches): the map then keeps a database of term counts per keyframe, made lazily by
        the next query_keyframes or relocalize(preselect=...).  The mapper keeps the vocabulary alive while it is attached."""
        if vocabulary is not None and vocabulary.h is None:
            raise ValueError("the vocabulary is closed")
        self._check(self.lib.mo_map_set_vocabulary(self._h, vocabulary.h if vocabulary is not None else None))
        self.vocabulary = vocabulary

    def train_vocabulary(self, words, iters=10):
        """A vocabulary trained on the descriptors of this map's keyframes (one image per keyframe), attached and returned"""
        v = V.Vocabulary.train([kf["descriptors"] for kf in self.keyframes if kf["descriptors"] is not None], words, iters, context=self.ctx)
        self.set_vocabulary(v)
        return v

    def query_keyframes(self, keypoints, descriptors, n_best=10):
        """The keyframes that look like the frame (mo_map_query_keyframes in include/vslam_amd.h states the rules): DBoW2's L1 score of
        the frame's and each keyframe's tf-idf vector over the attached vocabulary.  The frame is given like relocalize's; the map is
        not changed.  Returns (positions, scores): the keyframe positions with a score > 0, highest first, at most n_best."""
        ref, n, _keep = self._frame_ref(keypoints, descriptors)
        nb = int(n_best)
        pos = np.full(max(nb, 1), -1, np.int32)
        score = np.zeros(max(nb, 1), np.float64)
        prm = V.MapQueryParams(nb)
        out = V.MapQueryOut(pos.ctypes.data, score.ctypes.data)
        self._check(self.lib.mo_map_query_keyframes(self._h, C.byref(ref), C.byref(prm), C.byref(out)))
        return pos[:int(out.n)].copy(), score[:int(out.n)].copy()

    def relocalize(self, keypoints, descriptors, ratio_threshold=0.75, threshold=3.0, min_inliers=50, max_candidates=4, n_hyp=512, seed=None,
                   preselect=None):
        """The pose of a lost frame against the map as it stands (the map is not changed): the frame is matched against every keyframe
        (knn-2, Lowe ratio), the matches become 2D-3D correspondences through the map's observations, and a P3P RANSAC with Gauss-Newton
        refinement runs on the best-scoring keyframes (mo_map_relocalize in include/vslam_amd.h states the rules).  The frame is given
        like add_keyframe's: the arrays a detect_and_compute returned (resident on the device: nothing is uploaded) or host arrays.
        Returns (ok, pose, info): pose 4x4 (X_cam = R X + t, the convention add_keyframe takes; None without a winner); info holds
        kf_pos / kf_id of the winner, the candidates [(position, score, inliers)], and per query keypoint `point` (map point index,
        -1: none) and `inlier` of the winner.
        preselect=N: the frame is matched only against the N keyframes query_keyframes ranks first (selected on the device, no host
        round trip; mo_map_relocalize_pre); needs a vocabulary.  N >= the number of keyframes gives the plain call's result."""
        seed = self.seed if seed is None else int(seed)
        ref, n, _keep = self._frame_ref(keypoints, descriptors)
        K = np.ascontiguousarray(self.camera_matrix, np.float64).reshape(9)
        nc = int(max_candidates)
        point = np.full(max(n, 1), -1, np.int32)
        inlier = np.zeros(max(n, 1), np.uint8)
        cpos = np.full(max(nc, 1), -1, np.int32)
        cscore = np.zeros(max(nc, 1), np.int32)
        cinl = np.zeros(max(nc, 1), np.int32)
        prm = V.MapRelocParams(float(ratio_threshold), float(threshold), int(min_inliers), nc, int(n_hyp), seed)
        out = V.MapRelocOut(point.ctypes.data, inlier.ctypes.data, cpos.ctypes.data, cscore.ctypes.data, cinl.ctypes.data)
        if preselect is None:
            self._check(self.lib.mo_map_relocalize(self._h, C.byref(ref), V._ptr(K), C.byref(prm), C.byref(out)))
        else:
            self._check(self.lib.mo_map_relocalize_pre(self._h, C.byref(ref), V._ptr(K), C.byref(prm), int(preselect), C.byref(out)))
        kf_pos = int(out.kf_pos)
        pose = None
        if kf_pos >= 0:
            pose = np.eye(4)
            pose[:3, :] = np.array(out.pose).reshape(3, 4)
        nk = int(out.n_cand)
        info = {"kf_pos": kf_pos, "kf_id": self.keyframes[kf_pos]["id"] if kf_pos >= 0 else None,
                "candidates": [(int(cpos[i]), int(cscore[i]), int(cinl[i])) for i in range(nk)],
                "n_corr": int(out.n_corr), "n_inliers": int(out.n_inliers), "point": point[:n], "inlier": inlier[:n].astype(bool),
                "from_token": bool(out.from_token)}
        return bool(out.ok), pose, info

    @staticmethod
    def _batch_frames(frames, limit):
        """the (keypoints, descriptors) pairs of a batch call as a list, checked before anything touches the map"""
        frames = list(frames)
        if len(frames) > limit:
            raise ValueError("at most %d frames in a batch" % limit)
        for fr in frames:
            if not isinstance(fr, (tuple, list)) or len(fr) != 2:
                raise ValueError("frames: a sequence of (keypoints, descriptors) pairs")
        return frames

    def _batch_refs(self, frames):
        """(FrameRef array, row counts, the arrays they point into) of the frames of a batch call"""
        refs = (V.FrameRef * max(len(frames), 1))()
        ns, keep = [], []
        for i, (kp, de) in enumerate(frames):
            refs[i], n, arrays = self._frame_ref(kp, de)
            ns.append(n)
            keep.append(arrays)
        return refs, ns, keep

    @staticmethod
    def reloc_batch_plan(n_frames, pairs_per_frame, row, max_pairs=None):
        """(frames per group, groups) of relocalize_batch (mo_map_reloc_batch_plan): whole frames under the pair budget - max_pairs,
        by default 1 GiB of matcher output at `row` rows per frame, never more than 65535 pairs -, at least one frame per group.
        pairs_per_frame: the keyframes matched per frame.  Runs on the host."""
        fpg, ng = C.c_int32(0), C.c_int32(0)
        rc = V.load_library().mo_map_reloc_batch_plan(int(n_frames), int(pairs_per_frame), int(row), int(max_pairs or 0), C.byref(fpg), C.byref(ng))
        if rc != 0:
            raise ValueError("reloc_batch_plan: negative argument")
        return fpg.value, ng.value

    def relocalize_batch(self, frames, ratio_threshold=0.75, threshold=3.0, min_inliers=50, max_candidates=4, n_hyp=512, seed=None,
                         preselect=None, max_pairs=None):
        """relocalize for many frames in one device chain (mo_map_relocalize_batch in include/vslam_amd.h states the rules): a directory
        of query images against a saved map, the cameras of a rig after a tracking loss, the frames of a stream chunk behind a break.
        frames: a sequence of (keypoints, descriptors) as relocalize takes them (arrays that still carry a token are used resident).
        One camera matrix and one parameter set serve every frame.  max_pairs: the most (frame, keyframe) pairs matched per group of
        frames (None: 1 GiB of matcher output); the grouping changes no result.
        Returns (ok [n] bool, poses, infos): every frame's results are what relocalize (with the same preselect) returns for it alone on
        the same map, bit for bit, whatever the order and the company; poses[i] is None without a winner; infos[i] has the keys of
        relocalize's info.  The groups the call ran in are kept in `last_reloc_groups`."""
        frames = self._batch_frames(frames, V.RELOC_BATCH_MAX)
        nf = len(frames)
        if max_pairs is not None and int(max_pairs) < 1:
            raise ValueError("max_pairs: at least one pair, or None")
        nc = int(max_candidates)
        if not 1 <= nc <= 64:
            raise ValueError("max_candidates must be in 1 .. 64")
        seed = self.seed if seed is None else int(seed)
        refs, ns, _keep = self._batch_refs(frames)
        stride = max(ns + [1])
        m = max(nf, 1)
        point = np.full((m, stride), -1, np.int32)
        inlier = np.zeros((m, stride), np.uint8)
        cpos = np.full((m, nc), -1, np.int32)
        cscore, cinl = np.zeros((m, nc), np.int32), np.zeros((m, nc), np.int32)
        pose = np.full((m, 12), np.nan)
        ok, kf_pos, n_cand, n_corr, n_inl, tok = (np.zeros(m, np.int32) for _ in range(6))
        K = np.ascontiguousarray(self.camera_matrix, np.float64).reshape(9)
        prm = V.MapRelocBatchParams(V.MapRelocParams(float(ratio_threshold), float(threshold), int(min_inliers), nc, int(n_hyp), seed),
                                    -1 if preselect is None else int(preselect), int(max_pairs or 0))
        out = V.MapRelocBatchOut(stride, *[a.ctypes.data for a in (point, inlier, cpos, cscore, cinl, pose, ok, kf_pos, n_cand, n_corr, n_inl, tok)])
        self._check(self.lib.mo_map_relocalize_batch(self._h, refs, nf, V._ptr(K), C.byref(prm), C.byref(out)))
        self.last_reloc_groups = int(out.n_groups)
        poses, infos = [], []
        for i in range(nf):
            kp = int(kf_pos[i])
            T = None
            if kp >= 0:
                T = np.eye(4)
                T[:3, :] = pose[i].reshape(3, 4)
            poses.append(T)
            infos.append({"kf_pos": kp, "kf_id": self.keyframes[kp]["id"] if kp >= 0 else None,
                          "candidates": [(int(cpos[i, j]), int(cscore[i, j]), int(cinl[i, j])) for j in range(int(n_cand[i]))],
                          "n_corr": int(n_corr[i]), "n_inliers": int(n_inl[i]), "point": point[i, :ns[i]].copy(),
                          "inlier": inlier[i, :ns[i]].astype(bool), "from_token": bool(tok[i])})
        return ok[:nf].astype(bool), poses, infos

    def query_keyframes_batch(self, frames, n_best=10):
        """query_keyframes for many frames in one device chain (mo_map_query_keyframes_batch): a list of (positions, scores), frame i's
        what query_keyframes returns for it alone.  frames are given like relocalize_batch's; the map is not changed."""
        frames = self._batch_frames(frames, V.RELOC_BATCH_MAX)
        nf, nb = len(frames), int(n_best)
        if nb < 0:
            raise ValueError("n_best must be >= 0")
        refs, _ns, _keep = self._batch_refs(frames)
        pos = np.full((max(nf, 1), max(nb, 1)), -1, np.int32)
        score = np.zeros((max(nf, 1), max(nb, 1)), np.float64)
        n, tok = np.zeros(max(nf, 1), np.int32), np.zeros(max(nf, 1), np.int32)
        prm = V.MapQueryParams(nb)
        if nb == 0:   # (the places are [n][n_best]: with none asked for there is no row to address)
            pos, score = pos[:, :0], score[:, :0]
        self._check(self.lib.mo_map_query_keyframes_batch(self._h, refs, nf, C.byref(prm), pos.ctypes.data if nb else None,
                                                          score.ctypes.data if nb else None, n.ctypes.data, tok.ctypes.data))
        return [(pos[i, :int(n[i])].copy(), score[i, :int(n[i])].copy()) for i in range(nf)]

    def _frame_ref(self, keypoints, descriptors):
        """(FrameRef, n, arrays it points into) of a query frame: by token when the arrays are a resident detect_and_compute result,
        else the host arrays"""
        from orbslam2.types import keypoints_to_array
        token = V.resident_token(self.ctx, descriptors) if descriptors is not None else 0
        kps_arr = V._resident_kps(descriptors) if token else None
        if kps_arr is None or len(kps_arr) != len(keypoints):
            token = 0
            if isinstance(keypoints, np.ndarray) and keypoints.dtype == V.KP_DTYPE:
                kps_arr = keypoints
            else:
                kps_arr = keypoints_to_array(keypoints) if len(keypoints) else np.zeros(0, V.KP_DTYPE)
        kps_arr = np.ascontiguousarray(kps_arr, V.KP_DTYPE).reshape(-1)
        desc = np.ascontiguousarray(descriptors if descriptors is not None else np.zeros((0, 32), np.uint8), np.uint8).reshape(-1, 32)
        n = len(kps_arr) if token else min(len(kps_arr), len(desc))
        return V.FrameRef(token, V._ptr(kps_arr), V._ptr(desc), n), n, (kps_arr, desc)

    # ---- tracking against the map -------------------------------------------------------------------------------------------------
    def _track_params(self, window, radii, scale_factor, max_dist, ratio, chi2, min_matches, min_inliers, image_size):
        """MapTrackParams of track_local_map and track_local_map_batch: the radii checked, image_size defaulted to the last keyframe's image"""
        radii = [float(r) for r in radii]
        if not 1 <= len(radii) <= 4:
            raise ValueError("radii: one to four passes")
        if image_size is None:
            image_size = self._default_image_size()
        return V.MapTrackParams(int(image_size[0]), int(image_size[1]), int(window), len(radii), (C.c_double * 4)(*(radii + [0.0] * (4 - len(radii)))),
                                float(scale_factor), float(ratio), float(chi2), int(max_dist), int(min_matches), int(min_inliers))

    @staticmethod
    def _track_info(n, point, dist, inlier, nr, pass_pose, pass_radius, pass_cand, pass_matches, pass_inliers, n_local, from_token):
        """the info dict of one tracked frame from its per-keypoint rows and per-pass arrays (nr passes ran)"""
        nr = int(nr)
        return {"point": point[:n], "dist": dist[:n], "inlier": inlier[:n].astype(bool),
                "pass_pose": [np.vstack([np.array(pass_pose[k]).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]]) for k in range(nr)],
                "pass_radius": [float(pass_radius[k]) for k in range(nr)], "pass_cand": [int(pass_cand[k]) for k in range(nr)],
                "pass_matches": [int(pass_matches[k]) for k in range(nr)], "pass_inliers": [int(pass_inliers[k]) for k in range(nr)],
                "n_pass_run": nr, "n_local": int(n_local), "from_token": bool(from_token)}

    def track_local_map(self, keypoints, descriptors, pose, window=10, radii=(15.0, 4.0), scale_factor=1.2, max_dist=100, ratio=0.8,
                        chi2=5.991, min_matches=20, min_inliers=30, image_size=None, local="window", seed_points=None, n_best=10, min_weight=15,
                        frustum=False, n_levels=8, view_range=(0.8, 1.2), min_cos=0.5):
        """The pose of a tracked frame in the map's frame and scale, from a predicted pose (ORB-SLAM2's TrackLocalMap: search by projection
        of the local map, then pose-only optimisation; mo_map_track in include/vslam_amd.h states the rules).  The map is not changed.
        pose: the predicted 4x4 (X_cam = R X + t; predict_pose gives the constant-velocity one).  window: keyframe positions of the
        local map, counted from the last (0: all).  radii: one search half-width per pass (1 to 4 passes), at octave 0.  image_size:
        (w, h) a projection must land in, by default the last keyframe's image.  The frame is given like relocalize's.
        Returns (ok, pose, info): pose 4x4 of the last pass that finished (the given pose when none did); info holds per keypoint
        `point` (map point index, -1: none), `dist` (Hamming distance, -1: none) and `inlier` of the last pass searched, per pass
        `pass_pose`, `pass_radius`, `pass_cand`, `pass_matches`, `pass_inliers` (lists over the passes that ran), `n_local` and
        `from_token`.
        local: "window" - the local map is what the last `window` keyframes see; "covisible" - what the local keyframes of
        local_keyframes(seed_points, None, n_best, min_weight) see (mo_map_track_covisible; `window` is not used): seed_points is the
        `point` array a previous track_local_map on this map returned (-1 entries are skipped; None: the last keyframe and its
        neighbours).  info then also holds `local_keyframes` (positions) and `ref_keyframe`.
        frustum=True (mo_map_track_frustum, with either local map): ORB-SLAM2's isInFrustum and PredictScale - a point is searched only
        when the pass camera stands within view_range = (0.8, 1.2) of its scale-invariance range [min_dist, max_dist] and within
        acos(min_cos) of its mean viewing direction (point_views gives both), at the pyramid level L its distance predicts and against
        keypoints of octave L - 1 or L, in place of the representative observation's octave +- 1.  n_levels: the extractor's pyramid
        levels.  pass_cand then counts the points that passed; info also holds `pass_in_image` (the plain candidates) and per keypoint
        `level` (the predicted level of its point, -1: none)."""
        if local not in ("window", "covisible"):
            raise ValueError("local: \"window\" or \"covisible\"")
        prm = self._track_params(window, radii, scale_factor, max_dist, ratio, chi2, min_matches, min_inliers, image_size)
        ref, n, _keep = self._frame_ref(keypoints, descriptors)
        K = np.ascontiguousarray(self.camera_matrix, np.float64).reshape(9)
        pose0 = np.ascontiguousarray(np.asarray(pose, np.float64)[:3, :4]).reshape(12)
        point = np.full(max(n, 1), -1, np.int32)
        dist = np.full(max(n, 1), -1, np.int32)
        inlier = np.zeros(max(n, 1), np.uint8)
        out = V.MapTrackOut(point.ctypes.data, dist.ctypes.data, inlier.ctypes.data)
        if frustum:
            level = np.full(max(n, 1), -1, np.int32)
            fprm = V.MapFrustumParams(int(n_levels), float(view_range[0]), float(view_range[1]), float(min_cos))
            fout = V.MapFrustumOut(level.ctypes.data)
            lprm = lout = None
            if local == "covisible":
                lprm, lout, mask, _seeds = self._local_args(seed_points, None, n_best, min_weight)
            self._check(self.lib.mo_map_track_frustum(self._h, C.byref(ref), V._ptr(K), V._ptr(pose0), C.byref(prm), C.byref(lprm) if lprm else None,
                                                      C.byref(fprm), C.byref(out), C.byref(lout) if lout else None, C.byref(fout)))
        elif local == "covisible":
            lprm, lout, mask, _seeds = self._local_args(seed_points, None, n_best, min_weight)
            self._check(self.lib.mo_map_track_covisible(self._h, C.byref(ref), V._ptr(K), V._ptr(pose0), C.byref(prm), C.byref(lprm), C.byref(lout),
                                                        C.byref(out)))
        else:
            self._check(self.lib.mo_map_track(self._h, C.byref(ref), V._ptr(K), V._ptr(pose0), C.byref(prm), C.byref(out)))
        T = np.eye(4)
        T[:3, :] = np.array(out.pose).reshape(3, 4)
        nr = int(out.n_pass_run)
        info = self._track_info(n, point, dist, inlier, nr, out.pass_pose, out.pass_radius, out.pass_cand, out.pass_matches, out.pass_inliers,
                                out.n_local, out.from_token)
        if frustum:
            info["level"] = level[:n]
            info["pass_in_image"] = [int(fout.pass_in_image[k]) for k in range(nr)]
        if local == "covisible":
            info["local_keyframes"] = np.flatnonzero(mask[:len(self.keyframes)]).tolist()
            info["ref_keyframe"] = int(lout.ref)
        return bool(out.ok), T, info

    def keyframe_words(self, kf_position):
        """The vocabulary word of every row of the keyframe at kf_position (negative: from the end), int32 [rows], as the keyframe
        database holds them (mo_map_keyframe_words: stale keyframes are quantised first).  Needs a vocabulary."""
        n_kf = len(self.keyframes)
        pos = int(kf_position) + n_kf if int(kf_position) < 0 else int(kf_position)
        if not 0 <= pos < n_kf:
            raise IndexError("keyframe position out of range")
        rows = int(self.keyframes[pos]._rows)
        out = np.zeros(max(rows, 1), np.int32)
        self._check(self.lib.mo_map_keyframe_words(self._h, pos, V._ptr(out)))
        return out[:rows]

    def track_reference_keyframe(self, keypoints, descriptors, kf_position=-1, pose=None, max_dist=50, ratio=0.7, check_orientation=True,
                                 scale_factor=1.2, chi2=5.991, min_matches=15, min_inliers=10):
        """The pose of a frame from its matches by appearance to one keyframe (ORB-SLAM2's TrackReferenceKeyFrame;
        mo_map_track_reference in include/vslam_amd.h states the rules): the keyframe rows that have a map point are matched to the
        frame rows of the same vocabulary word, the matches are checked for a consistent rotation, and the pose is refined from them.
        The step between track_local_map, which needs a good predicted pose, and relocalize, which matches against many keyframes: it
        needs no good prior and costs what a tracking call costs.  Needs a vocabulary; the map is not changed.
        kf_position: the reference keyframe (negative: from the end).  pose: the 4x4 the refinement starts from, by default the
        keyframe's stored pose.  check_orientation=False for keypoints without angles (angle -1).  The frame is given like relocalize's.
        Returns (ok, pose, info) shaped like track_local_map's: info holds per keypoint `point`, `dist`, `inlier` and `kf_row` (the
        keyframe row of the match, -1: none), the counts `n_cand`, `n_claims`, `n_matches_raw`, `n_matches`, `n_inliers`, the
        orientation histogram `hist` [30] with `kept_bin` [3] (-1: none), and `from_token`; `point` and `inlier` feed
        add_keyframe(..., tracked=) and note_tracking as track_local_map's do."""
        n_kf = len(self.keyframes)
        pos = int(kf_position)
        if pose is None:
            at = pos + n_kf if pos < 0 else pos
            pose = self.keyframes[at]["pose"] if 0 <= at < n_kf else np.eye(4)
        ref, n, _keep = self._frame_ref(keypoints, descriptors)
        K = np.ascontiguousarray(self.camera_matrix, np.float64).reshape(9)
        pose0 = np.ascontiguousarray(np.asarray(pose, np.float64)[:3, :4]).reshape(12)
        point = np.full(max(n, 1), -1, np.int32)
        dist = np.full(max(n, 1), -1, np.int32)
        inlier = np.zeros(max(n, 1), np.uint8)
        kf_row = np.full(max(n, 1), -1, np.int32)
        prm = V.MapTrackRefParams(pos, int(bool(check_orientation)), float(scale_factor), float(ratio), float(chi2), int(max_dist), int(min_matches),
                                  int(min_inliers))
        out = V.MapTrackRefOut(point.ctypes.data, dist.ctypes.data, inlier.ctypes.data, kf_row.ctypes.data)
        self._check(self.lib.mo_map_track_reference(self._h, C.byref(ref), V._ptr(K), V._ptr(pose0), C.byref(prm), C.byref(out)))
        T = np.eye(4)
        T[:3, :] = np.array(out.pose).reshape(3, 4)
        info = {"point": point[:n], "dist": dist[:n], "inlier": inlier[:n].astype(bool), "kf_row": kf_row[:n],
                "n_cand": int(out.n_cand), "n_claims": int(out.n_claims), "n_matches_raw": int(out.n_matches_raw), "n_matches": int(out.n_matches),
                "n_inliers": int(out.n_inliers), "hist": np.array(out.hist, np.int32), "kept_bin": np.array(out.kept_bin, np.int32),
                "from_token": bool(out.from_token)}
        return bool(out.ok), T, info

    def track_local_map_batch(self, frames, poses, window=10, radii=(15.0, 4.0), scale_factor=1.2, max_dist=100, ratio=0.8, chi2=5.991,
                              min_matches=20, min_inliers=30, image_size=None):
        """track_local_map for many frames in one device chain (mo_map_track_batch in include/vslam_amd.h states the rules): the cameras
        of a rig, a recorded sequence with odometry priors, a set of relocalised frames, the frames of one stream chunk.  frames: a
        sequence of (keypoints, descriptors) as track_local_map takes them (arrays that still carry a token are used resident); poses:
        [n][4][4] or [n][3][4] predicted poses.  One camera matrix, image size and parameter set serve every frame; the local map is
        the window's ("covisible" and the frustum mode are not offered here).
        Returns (ok [n] bool, poses [n][4][4], infos): every frame's results are what track_local_map returns for it alone on the same
        map, bit for bit, whatever the order and the company; infos[i] has the keys of track_local_map's info (`n_local` is the
        batch's: the local map is formed once)."""
        frames = list(frames)
        nf = len(frames)
        if nf > V.TRACK_BATCH_MAX:
            raise ValueError("at most %d frames in a batch" % V.TRACK_BATCH_MAX)
        for fr in frames:
            if not isinstance(fr, (tuple, list)) or len(fr) != 2:
                raise ValueError("frames: a sequence of (keypoints, descriptors) pairs")
        poses = np.asarray(poses, np.float64)
        if poses.size == 0 and nf == 0:
            poses = np.zeros((0, 3, 4))
        if poses.ndim != 3 or poses.shape[0] != nf or poses.shape[1:] not in ((4, 4), (3, 4)):
            raise ValueError("poses: [n][4][4] or [n][3][4], one per frame")
        pose0 = np.ascontiguousarray(poses[:, :3, :4]).reshape(nf, 12)
        prm = self._track_params(window, radii, scale_factor, max_dist, ratio, chi2, min_matches, min_inliers, image_size)
        refs = (V.FrameRef * max(nf, 1))()
        ns, keep = [], []
        for i, (kp, de) in enumerate(frames):
            ref, n, arrays = self._frame_ref(kp, de)
            refs[i] = ref
            ns.append(n)
            keep.append(arrays)
        stride = max(ns + [1])
        m = max(nf, 1)
        point = np.full((m, stride), -1, np.int32)
        dist = np.full((m, stride), -1, np.int32)
        inlier = np.zeros((m, stride), np.uint8)
        pose = np.zeros((m, 12))
        pass_pose = np.zeros((m, 4, 12))
        pass_radius = np.zeros((m, 4))
        pass_cand, pass_matches, pass_inliers = (np.zeros((m, 4), np.int32) for _ in range(3))
        n_run, ok, from_token = (np.zeros(m, np.int32) for _ in range(3))
        K = np.ascontiguousarray(self.camera_matrix, np.float64).reshape(9)
        out = V.MapTrackBatchOut(stride, *[a.ctypes.data for a in (point, dist, inlier, pose, pass_pose, pass_radius, pass_cand, pass_matches,
                                                                   pass_inliers, n_run, ok, from_token)])
        self._check(self.lib.mo_map_track_batch(self._h, refs, nf, V._ptr(K), pose0.ctypes.data if nf else None, C.byref(prm), C.byref(out)))
        Ts = np.tile(np.eye(4), (nf, 1, 1))
        Ts[:, :3, :] = pose[:nf].reshape(nf, 3, 4)
        infos = [self._track_info(ns[i], point[i], dist[i], inlier[i], n_run[i], pass_pose[i], pass_radius[i], pass_cand[i], pass_matches[i],
                                  pass_inliers[i], out.n_local, from_token[i]) for i in range(nf)]
        return ok[:nf].astype(bool), Ts, infos

    def point_views(self, scale_factor=1.2, n_levels=8):
        """Where every map point was seen from (ORB-SLAM2's UpdateNormalAndDepth; mo_map_point_views in include/vslam_amd.h states the
        rules), computed on the device from the map as it stands and the store's own projection matrices; the map is not changed.
        Returns a dict of arrays: `normal` (n, 3) f32 the mean unit viewing direction (not renormalised), `min_dist` / `max_dist` (n,)
        f32 the scale-invariance range, `ref_pos` (n,) the keyframe position of the reference observation (-1: none), `ref_octave`,
        `n_valid` (the observations in the mean) and `centre` (n_kf, 3) f64 the camera centres by position (NaN: none)."""
        n, n_kf = self._n_points, len(self.keyframes)
        res = {"normal": np.zeros((n, 3), np.float32), "min_dist": np.zeros(n, np.float32), "max_dist": np.zeros(n, np.float32),
               "ref_pos": np.full(n, -1, np.int32), "ref_octave": np.zeros(n, np.int32), "n_valid": np.zeros(n, np.int32),
               "centre": np.full((n_kf, 3), np.nan)}
        prm = V.MapViewParams(float(scale_factor), int(n_levels))
        out = V.MapViewOut(*[res[f].ctypes.data if res[f].size else None for f in ("normal", "min_dist", "max_dist", "ref_pos", "ref_octave", "n_valid",
                                                                                    "centre")])
        self._check(self.lib.mo_map_point_views(self._h, C.byref(prm), C.byref(out)))
        assert int(out.n_points) == n and int(out.n_kf) == n_kf
        return res

    # ---- covisibility ---------------------------------------------------------------------------------------------------------------
    def covisibility(self):
        """W (n_kf, n_kf) int32 by keyframe position, computed on the device from the map as it stands (mo_map_covisibility in
        include/vslam_amd.h states the rules): W[p][q] = the map points with a valid observation at both positions, W[p][p] = those
        with one at p.  The true shared-point counts: co_visibility_graph keeps the reference's increments instead."""
        n = len(self.keyframes)
        W = np.zeros((n, n), np.int32)
        n_kf = C.c_int32(0)
        self._check(self.lib.mo_map_covisibility(self._h, V._ptr(W) if n else None, C.byref(n_kf)))
        assert n_kf.value == n
        return W

    def _local_args(self, seed_points, ref, n_best, min_weight):
        seeds = None if seed_points is None else np.ascontiguousarray(np.asarray(seed_points).reshape(-1), np.int32)
        mask = np.zeros(max(len(self.keyframes), 1), np.uint8)
        prm = V.MapLocalParams(seeds.ctypes.data if seeds is not None and len(seeds) else None, 0 if seeds is None else len(seeds),
                               -1 if ref is None else int(ref), int(n_best), int(min_weight))
        return prm, V.MapLocalOut(mask.ctypes.data), mask, seeds

    def local_keyframes(self, seed_points=None, ref=None, n_best=10, min_weight=15):
        """The local keyframes of ORB-SLAM2's UpdateLocalKeyFrames on the device covisibility matrix (mo_map_local_keyframes states the
        rules): K1 = the positions observing the map points in seed_points (indices; -1 and out-of-range entries are skipped), or
        {ref} (None: the last keyframe) when nothing votes; K2 = per K1 keyframe its n_best neighbours by shared points, each with at
        least max(min_weight, 1).  Returns {"local", "k1", "k2", "ref"}: position lists (k2: those not in k1) and the K1 position with
        the most votes."""
        prm, out, mask, _seeds = self._local_args(seed_points, ref, n_best, min_weight)
        self._check(self.lib.mo_map_local_keyframes(self._h, C.byref(prm), C.byref(out)))
        mask = mask[:len(self.keyframes)]
        assert int(out.n_k1) == int((mask == 1).sum()) and int(out.n_local_kf) == int((mask != 0).sum())
        return {"local": np.flatnonzero(mask).tolist(), "k1": np.flatnonzero(mask == 1).tolist(), "k2": np.flatnonzero(mask == 2).tolist(),
                "ref": int(out.ref)}

    # ---- loop detection --------------------------------------------------------------------------------------------------------------
    def loop_candidates(self, kf_position=-1, min_weight=15, n_best=10, max_candidates=4, ratio=0.75, among=None):
        """The old keyframes keyframe `kf_position` (-1: the last) may close a loop with, and the map points of the two that correspond
        (ORB-SLAM2's DetectLoopCandidates and the matching that opens ComputeSim3; mo_map_loop_candidates in include/vslam_amd.h states
        the rules).  Needs a vocabulary; stateless; the map is not changed.  Returns a dict: `candidates`, a list of dicts in rank order
        with `pos`, `acc` (accumulated group score), `score` (its own), `group` (the positions of the candidate and the keyframes
        connected to it), `n_match`, `cur_point` (the asking keyframe's map point per keypoint row, -1: none), `match_point` (the
        candidate's map point matched to that row, -1) and `match_row` (its keypoint row in the candidate, -1); `cur_point` once more at the top (also there
        without a candidate); `connected` (positions connected to the asking keyframe, itself included), `min_score`, `max_common`, `n_scored`, `n_passed`, `n_found` (candidates
        before the cut at max_candidates) and `n_connected`.
        among: keyframe positions, or a bool mask with one entry per keyframe: only these can be candidates or add to a group's score
        (mo_map_loop_candidates_among; merge_map asks the absorbed side about the absorbing one).  None: every keyframe."""
        n_kf, mc = len(self.keyframes), int(max_candidates)
        amask = None
        if among is not None:
            sel = np.asarray(among)
            if sel.dtype == np.bool_:
                if sel.shape != (n_kf,):
                    raise ValueError("a mask must have one entry per keyframe")
                amask = np.ascontiguousarray(sel, np.uint8)
            else:
                idx = sel.astype(np.int64).reshape(-1)
                if len(idx) and (idx.min() < 0 or idx.max() >= n_kf):
                    raise IndexError("keyframe position out of range")
                amask = np.zeros(n_kf, np.uint8)
                amask[idx] = 1
            amask = np.concatenate([amask, np.zeros(1, np.uint8)])   # (never empty)
        p = n_kf - 1 if int(kf_position) < 0 else int(kf_position)
        n_p = self.keyframes[p]._rows if 0 <= p < n_kf else 0
        m1 = max(mc, 1)
        cand = np.full(m1, -1, np.int32)
        acc, score = np.zeros(m1, np.float64), np.zeros(m1, np.float64)
        connected = np.zeros(max(n_kf, 1), np.uint8)
        group = np.zeros((m1, max(n_kf, 1)), np.uint8)
        cur = np.full(max(n_p, 1), -1, np.int32)
        mpt, mrow = np.full((m1, max(n_p, 1)), -1, np.int32), np.full((m1, max(n_p, 1)), -1, np.int32)
        n_match = np.zeros(m1, np.int32)
        prm = V.MapLoopParams(int(kf_position), int(min_weight), int(n_best), mc, float(ratio))
        out = V.MapLoopOut(cand.ctypes.data, acc.ctypes.data, score.ctypes.data, connected.ctypes.data, group.ctypes.data, cur.ctypes.data,
                           mpt.ctypes.data, mrow.ctypes.data, n_match.ctypes.data)
        if amask is None:
            self._check(self.lib.mo_map_loop_candidates(self._h, C.byref(prm), C.byref(out)))
        else:
            self._check(self.lib.mo_map_loop_candidates_among(self._h, C.byref(prm), V._ptr(amask), C.byref(out)))
        # (the device writes the arrays packed: [max_cand][n_kf] and [max_cand][rows], which is their shape whenever they hold anything)
        cur = cur[:n_p]
        cands = [{"pos": int(cand[i]), "acc": float(acc[i]), "score": float(score[i]), "group": np.flatnonzero(group[i, :n_kf]).tolist(),
                  "n_match": int(n_match[i]), "cur_point": cur, "match_point": mpt[i, :n_p], "match_row": mrow[i, :n_p]}
                 for i in range(int(out.n_cand))]
        return {"candidates": cands, "cur_point": cur, "connected": np.flatnonzero(connected[:n_kf]).tolist(), "min_score": float(out.min_score),
                "max_common": int(out.max_common), "n_scored": int(out.n_scored), "n_passed": int(out.n_passed), "n_found": int(out.n_found),
                "n_connected": int(out.n_connected), "kf_pos": p}

    def compute_sim3(self, info_or_candidates, n_hyp=300, seed=0, chi2=9.210, scale_factor=1.2, min_inliers=20, kf_position=None):
        """The similarity that aligns the asking keyframe with its loop candidates (ORB-SLAM2's ComputeSim3; mo_map_loop_sim3 in
        include/vslam_amd.h states the rules): per candidate a 3-point RANSAC over Horn's closed form on the matched map points, scored
        by reprojection into both keyframes, then Gauss-Newton on sim(3).  The map is not changed.  Takes loop_candidates()'s dict, or a
        list of its candidate dicts such as [info["accepted"]] (then the asking keyframe is kf_position, by default the last).  Poses
        come from kf["pose"], K from camera_matrix.
        Returns (ok, info): ok when the winner - the candidate with the most final inliers - has at least min_inliers.  info holds
        `candidates`, a list of dicts with `pos`, `scale`, `R` (3, 3), `t` (3), `n_corr`, `n_inliers` and `inlier` (bool per keypoint row
        of the asking keyframe); `win` (index into that list, -1: none), `n_inliers` of the winner, `kf_pos`, and `world`: the 4x4
        similarity in the map frame that takes the candidate's side onto the asking side, T1^-1 S12 T2 (None without a winner).
        X1 = scale R X2 + t takes a point of the candidate's camera frame into the asking keyframe's."""
        n_kf = len(self.keyframes)
        if isinstance(info_or_candidates, dict):
            cands = list(info_or_candidates["candidates"])
            p = info_or_candidates.get("kf_pos") if kf_position is None else kf_position
            cur = info_or_candidates.get("cur_point")
        else:
            cands = list(info_or_candidates)
            p, cur = kf_position, None
        p = n_kf - 1 if p is None or int(p) < 0 else int(p)
        nc = len(cands)
        n_p = self.keyframes[p]._rows if 0 <= p < n_kf else 0
        if cur is None and nc:
            cur = cands[0]["cur_point"]
        w = max(n_p, 1)   # (the library reads the lists packed [n_cand][rows of p]: the arrays' shape whenever they hold anything)
        cur_a = np.full(w, -1, np.int32)
        mpt, mrow = np.full((max(nc, 1), w), -1, np.int32), np.full((max(nc, 1), w), -1, np.int32)
        if nc and n_p:
            cur_a[:n_p] = np.asarray(cur, np.int32).reshape(-1)[:n_p]
            for i, cd in enumerate(cands):
                mpt[i, :n_p] = np.asarray(cd["match_point"], np.int32).reshape(-1)[:n_p]
                mrow[i, :n_p] = np.asarray(cd["match_row"], np.int32).reshape(-1)[:n_p]
        pos = np.array([int(cd["pos"]) for cd in cands] or [0], np.int32)
        poses = np.zeros((max(n_kf, 1), 12), np.float64)
        for i, kf in enumerate(self.keyframes):
            poses[i] = np.asarray(kf["pose"], np.float64)[:3, :4].reshape(12)
        K = np.ascontiguousarray(self.camera_matrix, np.float64).reshape(9)
        m1 = max(nc, 1)
        scale, R, t = np.full(m1, np.nan), np.full((m1, 9), np.nan), np.full((m1, 3), np.nan)
        n_corr, n_inl = np.zeros(m1, np.int32), np.zeros(m1, np.int32)
        inl = np.zeros((m1, w), np.uint8)
        prm = V.MapSim3Params(p, nc, pos.ctypes.data, cur_a.ctypes.data, mpt.ctypes.data, mrow.ctypes.data, int(n_hyp), int(min_inliers),
                              int(seed), float(chi2), float(scale_factor))
        out = V.MapSim3Out(scale.ctypes.data, R.ctypes.data, t.ctypes.data, n_corr.ctypes.data, n_inl.ctypes.data, inl.ctypes.data)
        self._check(self.lib.mo_map_loop_sim3(self._h, V._ptr(K), V._ptr(poses), C.byref(prm), C.byref(out)))
        inl = inl[:nc, :n_p].astype(bool)
        res = [{"pos": int(pos[i]), "scale": float(scale[i]), "R": R[i].reshape(3, 3).copy(), "t": t[i].copy(), "n_corr": int(n_corr[i]),
                "n_inliers": int(n_inl[i]), "inlier": inl[i]} for i in range(nc)]
        win = int(out.win)
        world = None
        if win >= 0:
            S = np.eye(4)
            S[:3, :3] = res[win]["scale"] * res[win]["R"]
            S[:3, 3] = res[win]["t"]
            T1, T2 = np.eye(4), np.eye(4)
            T1[:3, :] = poses[p].reshape(3, 4)
            T2[:3, :] = poses[res[win]["pos"]].reshape(3, 4)
            world = np.linalg.inv(T1) @ S @ T2
        return bool(out.ok), {"candidates": res, "win": win, "n_inliers": int(out.win_inliers), "kf_pos": p, "world": world}

    def confirm_loop(self, candidates, sim3, group=None, kf_position=None, image_size=None, radius_guided=7.5, radius_proj=10.0, max_dist=50,
                     chi2=9.210, scale_factor=1.2, min_inliers=20, min_matches=40):
        """Confirms a loop whose candidates compute_sim3 aligned (the second half of ORB-SLAM2's ComputeSim3; mo_map_loop_confirm in
        include/vslam_amd.h states the rules): both keyframes are searched again guided by the similarity, the similarity is refitted on
        the seeds (the alignment's inliers) and the guided matches, and the points the winner's group observes are projected into the
        asking keyframe.  The map is not changed.  `candidates` are loop_candidates' candidate dicts (or its whole dict), `sim3` is
        compute_sim3's info or its list of per-candidate dicts, in the same order.  `group`: per candidate the keyframe positions whose
        points are projected; by default each candidate dict's `group` when it has one, else the candidate alone.  The asking keyframe is
        kf_position, by default sim3's `kf_pos`, else the last.  image_size (w, h) defaults to twice the principal point of K, rounded up.
        Returns (ok, info): ok when a candidate with at least min_inliers final inliers won and n_total >= min_matches.  info holds
        `candidates`, a list of dicts with `pos`, the refined `scale`, `R`, `t`, `n_pairs`, `n_guided`, `n_inliers`, `inlier` (bool per
        row of the asking keyframe), `fwd` (per row of the asking keyframe the candidate row the guided search found, -1) and `bwd` (per
        candidate row the asking row, -1); `win`, `loop_point` (per row of the asking keyframe the loop-side map point, -1: none), `source`
        (0 none, 1 seed, 2 guided, 3 projection), `n_total`, `n_proj`, `n_proj_cand`, `n_loop_points`, `n_inliers` of the winner, `kf_pos`,
        and `world` as in compute_sim3, from the refined model."""
        n_kf = len(self.keyframes)
        if isinstance(candidates, dict):
            cands = list(candidates["candidates"])
            cur = candidates.get("cur_point")
        else:
            cands, cur = list(candidates), None
        p = kf_position
        if isinstance(sim3, dict):
            models = list(sim3["candidates"])
            p = sim3.get("kf_pos") if p is None else p
        else:
            models = list(sim3)
        if len(models) != len(cands):
            raise ValueError("confirm_loop needs one alignment per candidate")
        p = n_kf - 1 if p is None or int(p) < 0 else int(p)
        nc = len(cands)
        n_p = self.keyframes[p]._rows if 0 <= p < n_kf else 0
        if cur is None and nc:
            cur = cands[0]["cur_point"]
        w = max(n_p, 1)
        m1 = max(nc, 1)
        cur_a = np.full(w, -1, np.int32)
        mpt, mrow = np.full((m1, w), -1, np.int32), np.full((m1, w), -1, np.int32)
        seed = np.ones((m1, w), np.uint8)
        if nc and n_p:
            cur_a[:n_p] = np.asarray(cur, np.int32).reshape(-1)[:n_p]
            for i, (cd, md) in enumerate(zip(cands, models)):
                mpt[i, :n_p] = np.asarray(cd["match_point"], np.int32).reshape(-1)[:n_p]
                mrow[i, :n_p] = np.asarray(cd["match_row"], np.int32).reshape(-1)[:n_p]
                if md.get("inlier") is not None:
                    seed[i, :n_p] = np.asarray(md["inlier"]).reshape(-1)[:n_p] != 0
        pos = np.array([int(cd["pos"]) for cd in cands] or [0], np.int32)
        s_in = np.array([float(md["scale"]) for md in models] or [np.nan], np.float64)
        R_in = np.array([np.asarray(md["R"], np.float64).reshape(9) for md in models] or [np.full(9, np.nan)], np.float64)
        t_in = np.array([np.asarray(md["t"], np.float64).reshape(3) for md in models] or [np.full(3, np.nan)], np.float64)
        gmask = np.zeros((m1, max(n_kf, 1)), np.uint8)
        for i, cd in enumerate(cands):
            g = group[i] if group is not None else cd.get("group")
            for q in ([int(cd["pos"])] if g is None else g):
                if 0 <= int(q) < n_kf:
                    gmask[i, int(q)] = 1
        rows2 = max([self.keyframes[int(k)]._rows if 0 <= int(k) < n_kf else 0 for k in pos[:nc]] + [1])
        poses = np.zeros((max(n_kf, 1), 12), np.float64)
        for i, kf in enumerate(self.keyframes):
            poses[i] = np.asarray(kf["pose"], np.float64)[:3, :4].reshape(12)
        K = np.ascontiguousarray(self.camera_matrix, np.float64).reshape(9)
        if image_size is None:
            image_size = (max(int(np.ceil(2 * K[2])), 1), max(int(np.ceil(2 * K[5])), 1))
        scale, R, t = np.full(m1, np.nan), np.full((m1, 9), np.nan), np.full((m1, 3), np.nan)
        n_pairs, n_guided, n_inl = np.zeros(m1, np.int32), np.zeros(m1, np.int32), np.zeros(m1, np.int32)
        inl = np.zeros((m1, w), np.uint8)
        fwd, bwd = np.full((m1, w), -1, np.int32), np.full((m1, rows2), -1, np.int32)
        lpt, src = np.full(w, -1, np.int32), np.zeros(w, np.uint8)
        flagged = any(md.get("inlier") is not None for md in models)   # (no flags at all: NULL, every listed row is a seed)
        prm = V.MapConfirmParams(p, nc, pos.ctypes.data, cur_a.ctypes.data, mpt.ctypes.data, mrow.ctypes.data, seed.ctypes.data if flagged else None, s_in.ctypes.data,
                                 R_in.ctypes.data, t_in.ctypes.data, gmask.ctypes.data, int(image_size[0]), int(image_size[1]), int(max_dist),
                                 int(min_inliers), int(min_matches), float(radius_guided), float(radius_proj), float(chi2), float(scale_factor))
        out = V.MapConfirmOut(scale.ctypes.data, R.ctypes.data, t.ctypes.data, n_pairs.ctypes.data, n_guided.ctypes.data, n_inl.ctypes.data,
                              inl.ctypes.data, fwd.ctypes.data, bwd.ctypes.data, lpt.ctypes.data, src.ctypes.data)
        self._check(self.lib.mo_map_loop_confirm(self._h, V._ptr(K), V._ptr(poses), C.byref(prm), C.byref(out)))
        # (the library writes the arrays packed: [n_cand][rows of p] and [n_cand][R2], which is their shape whenever they hold anything)
        res = []
        for i in range(nc):
            n2 = self.keyframes[int(pos[i])]._rows
            res.append({"pos": int(pos[i]), "scale": float(scale[i]), "R": R[i].reshape(3, 3).copy(), "t": t[i].copy(), "n_pairs": int(n_pairs[i]),
                        "n_guided": int(n_guided[i]), "n_inliers": int(n_inl[i]), "inlier": inl[i, :n_p].astype(bool), "fwd": fwd[i, :n_p].copy(),
                        "bwd": bwd[i, :n2].copy()})
        win = int(out.win)
        world = None
        if win >= 0:
            S = np.eye(4)
            S[:3, :3] = res[win]["scale"] * res[win]["R"]
            S[:3, 3] = res[win]["t"]
            T1, T2 = np.eye(4), np.eye(4)
            T1[:3, :] = poses[p].reshape(3, 4)
            T2[:3, :] = poses[res[win]["pos"]].reshape(3, 4)
            world = np.linalg.inv(T1) @ S @ T2
        return bool(out.ok), {"candidates": res, "win": win, "n_inliers": int(out.win_inliers), "loop_point": lpt[:n_p].copy(), "source": src[:n_p].copy(),
                              "n_total": int(out.n_total), "n_proj": int(out.n_proj), "n_proj_cand": int(out.n_proj_cand),
                              "n_loop_points": int(out.n_loop_points), "kf_pos": p, "world": world}

    def correct_loop(self, confirm, kf_position=None, corrected=None, group=None, min_weight=15, image_size=None, radius=4.0, scale_factor=1.2,
                     max_dist=50, chi2=5.991):
        """Corrects a confirmed loop on the map (the first half of ORB-SLAM2's CorrectLoop; mo_map_loop_correct in include/vslam_amd.h
        states the rules): the similarity is carried to the asking keyframe's neighbourhood, whose keyframes and points move onto the old
        side, and the old side's points replace and absorb the neighbourhood's duplicates - confirm's loop points directly, the rest of
        the group's points by fuse_map_points' search under the corrected poses.  The essential-graph optimisation is
        optimize_essential_graph, a call of its own, and so is the global bundle adjustment behind it, global_bundle_adjust.  `confirm` is confirm_loop's info, or an `accepted` candidate of detect_loop(confirm=True) (its
        `confirm` entry is used, its `group` is the default group).  The asking keyframe is kf_position, by default confirm's `kf_pos`.
        `corrected`: the positions that move; by default p and the positions whose covisibility() weight with p is at least min_weight,
        less the group's.  `group`: the old side's positions; by default the winning candidate's group, else the candidate alone.
        image_size as in confirm_loop.  kf["pose"] of the corrected keyframes is rewritten and the co-visibility graph follows the
        fusion as in fuse_map_points.
        Returns info: the counts n_corrected, n_moved, n_loop_points, n_direct_edges, n_direct_gained, n_pairs, n_cand, n_proposals,
        n_gained, n_edges, n_absorbed, n_points, n_obs; `into` (the new index of the point each old point now is), `moved` (bool per
        old point), `A` (3, 4) and `A_scale`: the map-frame transform the moved points took, `corrected` and `group` (position lists),
        `poses` [n_kf][3][4] and `loop_connections`: {corrected keyframe id: sorted ids of the keyframes, not corrected ones, it shares
        a point with after the call and shared none with before} (ORB-SLAM2's LoopConnections)."""
        n_kf = len(self.keyframes)
        acc = confirm if "confirm" in confirm else None
        cf = confirm["confirm"] if acc is not None else confirm
        win = int(cf["win"])
        if win < 0:
            raise ValueError("correct_loop needs a confirmation with a winner")
        model = cf["candidates"][win]
        p = cf.get("kf_pos") if kf_position is None else kf_position
        p = n_kf - 1 if p is None or int(p) < 0 else int(p)
        q = int(model["pos"])
        if group is None:
            group = acc.get("group") if acc is not None and acc.get("group") is not None else [q]
        gmask = np.zeros(max(n_kf, 1), np.uint8)
        for k in group:
            if 0 <= int(k) < n_kf:
                gmask[int(k)] = 1
        cmask = np.zeros(max(n_kf, 1), np.uint8)
        if corrected is None:
            W = self.covisibility()
            if 0 <= p < n_kf:
                cmask[:n_kf] = (W[p] >= max(int(min_weight), 1)) & (gmask[:n_kf] == 0)
                cmask[p] = 1
        else:
            for k in corrected:
                if 0 <= int(k) < n_kf:
                    cmask[int(k)] = 1
        n_p = self.keyframes[p]._rows if 0 <= p < n_kf else 0
        lpt = np.full(max(n_p, 1), -1, np.int32)
        if cf.get("loop_point") is not None and n_p:
            lpt[:n_p] = np.asarray(cf["loop_point"], np.int32).reshape(-1)[:n_p]
        poses = np.zeros((max(n_kf, 1), 12), np.float64)
        for i, kf in enumerate(self.keyframes):
            poses[i] = np.asarray(kf["pose"], np.float64)[:3, :4].reshape(12)
        K = np.ascontiguousarray(self.camera_matrix, np.float64).reshape(9)
        if image_size is None:
            image_size = (max(int(np.ceil(2 * K[2])), 1), max(int(np.ceil(2 * K[5])), 1))
        n0 = self._n_points
        before = self.arrays() if n0 else None
        into = np.arange(max(n0, 1), dtype=np.int32)
        moved = np.zeros(max(n0, 1), np.uint8)
        poses_out = poses.copy()
        prm = V.MapCorrectParams(p, q, float(model["scale"]), (C.c_double * 9)(*np.asarray(model["R"], np.float64).reshape(9)),
                                 (C.c_double * 3)(*np.asarray(model["t"], np.float64).reshape(3)), cmask.ctypes.data, gmask.ctypes.data, lpt.ctypes.data,
                                 int(image_size[0]), int(image_size[1]), float(radius), float(scale_factor), int(max_dist), float(chi2))
        out = V.MapCorrectOut(poses_out.ctypes.data, into.ctypes.data, moved.ctypes.data)
        self._check(self.lib.mo_map_loop_correct(self._h, V._ptr(K), V._ptr(poses), C.byref(prm), C.byref(out)))
        into = into[:n0]
        cpos = np.flatnonzero(cmask[:n_kf]).tolist() if out.n_corrected else []
        for i in cpos:
            self.keyframes[i]["pose"][:3, :4] = poses_out[i].reshape(3, 4)
        self._version += 1
        self._cache = None
        self._sync_size()
        info = {k: int(getattr(out, k)) for k in ("n_corrected", "n_moved", "n_loop_points", "n_direct_edges", "n_direct_gained", "n_pairs", "n_cand",
                                                  "n_proposals", "n_gained", "n_edges", "n_absorbed", "n_points", "n_obs")}
        info.update(into=into, moved=moved[:n0].astype(bool), A=np.array(out.A, np.float64).reshape(3, 4), A_scale=float(out.A_scale), corrected=cpos,
                    group=np.flatnonzero(gmask[:n_kf]).tolist(), poses=poses_out[:n_kf].reshape(n_kf, 3, 4), kf_pos=p, loop_connections={})
        if info["n_proposals"] or info["n_direct_edges"] or info["n_direct_gained"]:
            after = self.arrays()
            self._fuse_co_visibility(before, after, into)
            slot_of = {id(r): s for s, r in enumerate(self._records)}
            counts = np.array([self._rec_n[slot_of[id(kf)]] for kf in self.keyframes], np.int64)
            nb0, nb1 = positions_sharing_points(before, counts, cpos), positions_sharing_points(after, counts, cpos)
            cset = set(cpos)
            info["loop_connections"] = {self.keyframes[i]["id"]: sorted(self.keyframes[k]["id"] for k in nb1[i] - nb0[i] - cset) for i in cpos}
        return info

    def optimize_essential_graph(self, correct, poses_before=None, fixed=None, min_weight=100, extra_edges=None, max_steps=20, max_cg=200,
                                 cg_tol=1e-8, step_tol=1e-10, want_edges=True):
        """Optimises the essential graph behind a loop correction (the second half of ORB-SLAM2's CorrectLoop, OptimizeEssentialGraph;
        mo_map_pose_graph in include/vslam_amd.h states the rules): a Sim(3) pose graph over all keyframes whose edges come from the
        covisibility matrix (a parent per keyframe, the pairs of at least min_weight common points) and from the loop; the error the
        correction left at the edge of the corrected set is spread along the trajectory, and every point follows its reference keyframe.
        `correct` is correct_loop's info, or an `accepted` candidate of detect_loop(correct=True) (its `correct` entry is used and its
        `pos` is the winning candidate).  poses_before: the [R | t] of every keyframe before that correction (n_kf arrays of at least
        3 x 4); by default they are reconstructed in f64 from correct["poses"], A and A_scale (R_i = R_i' RA, t_i = s t_pose + R_i' tA
        with s = 1 / A_scale, RA | tA = s A).  `fixed`: the positions that stay; by default the winning candidate's (given correct_loop's info alone,
        which does not name it, the lowest position of its group).  correct["loop_connections"] (keyframe ids) become position pairs and join extra_edges (position pairs).
        kf["pose"] of the free keyframes is rewritten when a step was accepted.
        Returns info: ok, cost (start, end), lambda, steps, accepted, cg_iters, n_free, n_fixed, n_edges, n_extra_used, n_moved, `poses`
        [n_kf][3][4], `sim3` [n_kf][13] (s, R, t), `moved` (bool per point), `fixed` (positions) and `edges`: (a, b, kind) arrays."""
        n_kf = len(self.keyframes)
        winner = None
        if "correct" in correct:
            winner, correct = int(correct["pos"]), correct["correct"]
        cpos = [int(k) for k in correct["corrected"]]
        s = 1.0 / float(correct["A_scale"])
        A = np.asarray(correct["A"], np.float64).reshape(3, 4)
        RA, tA = s * A[:, :3], s * A[:, 3]
        after = np.asarray(correct["poses"], np.float64).reshape(-1, 3, 4) if n_kf else np.zeros((0, 3, 4))
        poses = np.zeros((max(n_kf, 1), 12), np.float64)
        init = np.zeros((max(n_kf, 1), 13), np.float64)
        cset = set(cpos)
        for i in range(n_kf):
            if poses_before is not None:
                T = np.asarray(poses_before[i], np.float64)[:3, :4]
            elif i in cset:
                Ri = after[i][:, :3] @ RA
                T = np.hstack([Ri, (s * after[i][:, 3] + after[i][:, :3] @ tA).reshape(3, 1)])
            else:
                T = after[i]
            poses[i] = T.reshape(12)
            if i in cset:   # S_iw' = T_i o A^-1: the corrected pose with its translation back at scale s
                init[i, 0] = s
                init[i, 1:10] = after[i][:, :3].reshape(9)
                init[i, 10:] = s * after[i][:, 3]
            else:
                init[i, 0] = 1.0
                init[i, 1:10] = T[:, :3].reshape(9)
                init[i, 10:] = T[:, 3]
        if fixed is None:
            fixed = [winner] if winner is not None else sorted(correct["group"])[:1]
        fmask = np.zeros(max(n_kf, 1), np.uint8)
        for k in fixed:
            if 0 <= int(k) < n_kf:
                fmask[int(k)] = 1
        pos_of = {kf["id"]: i for i, kf in enumerate(self.keyframes)}
        pairs = [(int(a), int(b)) for a, b in (extra_edges or [])]
        for a, others in (correct.get("loop_connections") or {}).items():
            pairs += [(pos_of[a], pos_of[b]) for b in others if a in pos_of and b in pos_of]
        xa = np.array([a for a, _ in pairs] or [0], np.int32)
        xb = np.array([b for _, b in pairs] or [0], np.int32)
        cap = max(n_kf * (n_kf - 1) // 2, 1) if want_edges else 0
        ea, eb, ek = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.uint8)
        n0 = self._n_points
        moved = np.zeros(max(n0, 1), np.uint8)
        poses_out = np.zeros((max(n_kf, 1), 12), np.float64)
        sim3_out = init.copy()
        for i in range(n_kf):
            poses_out[i] = np.hstack([init[i, 1:10].reshape(3, 3), (init[i, 10:] / init[i, 0]).reshape(3, 1)]).reshape(12)
        K = np.ascontiguousarray(self.camera_matrix, np.float64).reshape(9)
        prm = V.MapPgParams(fmask.ctypes.data, xa.ctypes.data, xb.ctypes.data, len(pairs), int(min_weight), int(max_steps), int(max_cg), float(cg_tol),
                            float(step_tol), (C.c_double * 9)(*K))
        out = V.MapPgOut(poses_out.ctypes.data, sim3_out.ctypes.data, ea.ctypes.data, eb.ctypes.data, ek.ctypes.data, moved.ctypes.data, cap)
        self._check(self.lib.mo_map_pose_graph(self._h, V._ptr(poses), V._ptr(init), C.byref(prm), C.byref(out)))
        ok = bool(out.ok)
        if ok:
            for i in range(n_kf):
                if not fmask[i]:
                    self.keyframes[i]["pose"][:3, :4] = poses_out[i].reshape(3, 4)
        self._version += 1
        self._cache = None
        info = {k: int(getattr(out, k)) for k in ("steps", "accepted", "cg_iters", "n_free", "n_fixed", "n_edges", "n_extra_used", "n_moved")}
        ne = min(info["n_edges"], cap)
        info.update(ok=ok, cost=(float(out.cost[0]), float(out.cost[1])), poses=poses_out[:n_kf].reshape(n_kf, 3, 4), sim3=sim3_out[:n_kf],
                    moved=moved[:n0].astype(bool), fixed=np.flatnonzero(fmask[:n_kf]).tolist(), edges=(ea[:ne].copy(), eb[:ne].copy(), ek[:ne].copy()))
        info["lambda"] = float(out.lambda_)
        return info

    def detect_loop(self, kf_position=-1, min_weight=15, n_best=10, max_candidates=4, ratio=0.75, min_matches=20, consistency=3, sim3=False,
                    confirm=False, confirm_kw=None, correct=False, correct_kw=None, optimize=False, optimize_kw=None, global_ba=False,
                    global_ba_kw=None, **sim3_kw):
        """ORB-SLAM2's DetectLoop up to the point correspondences: loop_candidates for the keyframe, the consistent-group bookkeeping
        (vslam_amd.loop.LoopConsistency, kept on the mapper from call to call on keyframe serials; call it once per new keyframe), and
        the match count.  Returns (found, info): found when a candidate whose group was consistent `consistency` times in a row has
        n_match >= min_matches; info is loop_candidates' dict, each candidate also with `serial`, `consistency`, `consistent` and
        `enough_matches`, and `accepted`: the first candidate in order with both flags (None: no loop), with its correspondence arrays.
        sim3=True: such a candidate is accepted only when compute_sim3 on it (keyword arguments in sim3_kw) is ok; `accepted` then also
        holds `sim3`: that candidate's alignment (scale, R, t, n_corr, n_inliers, inlier) with `world`, and every candidate that was
        tried holds `sim3_ok`.
        confirm=True (needs sim3=True): an aligned candidate is accepted only when confirm_loop on it (keyword arguments in confirm_kw) is ok
        too; `accepted` then also holds `confirm`: confirm_loop's info, and every candidate that was aligned holds `confirm_ok`.
        correct=True (needs confirm=True): an accepted loop is corrected by correct_loop (keyword arguments in correct_kw): the map
        changes, and `accepted` also holds `correct`: correct_loop's info.
        optimize=True (needs correct=True): the essential graph is optimised behind the correction by optimize_essential_graph (keyword
        arguments in optimize_kw) from the poses as they were before it, and `accepted` also holds `optimize`: its info.
        global_ba=True (needs optimize=True): global_bundle_adjust (keyword arguments in global_ba_kw) runs behind the essential graph,
        and `accepted` also holds `global_ba`: its info with `ok`."""
        from vslam_amd.loop import LoopConsistency
        if global_ba and not optimize:
            raise ValueError("global_ba=True needs optimize=True")
        if confirm and not sim3:
            raise ValueError("confirm=True needs sim3=True")
        if correct and not confirm:
            raise ValueError("correct=True needs confirm=True")
        if optimize and not correct:
            raise ValueError("optimize=True needs correct=True")
        if self._loop_consistency is None or self._loop_consistency.threshold != int(consistency):
            self._loop_consistency = LoopConsistency(consistency)
        info = self.loop_candidates(kf_position, min_weight, n_best, max_candidates, ratio)
        cands = info["candidates"]
        ser = self._kf_serials
        reported, cons = self._loop_consistency.update([(ser[c["pos"]], [ser[q] for q in c["group"]]) for c in cands])
        for c, n in zip(cands, cons):
            c["serial"] = ser[c["pos"]]
            c["consistency"] = n
            c["consistent"] = c["serial"] in reported
            c["enough_matches"] = c["n_match"] >= int(min_matches)
        if not sim3:
            info["accepted"] = next((c for c in cands if c["consistent"] and c["enough_matches"]), None)
            return info["accepted"] is not None, info
        info["accepted"] = None
        for c in cands:
            if not (c["consistent"] and c["enough_matches"]):
                continue
            ok, al = self.compute_sim3([c], kf_position=info["kf_pos"], **sim3_kw)
            c["sim3_ok"] = ok
            if ok and confirm:
                ok, cf = self.confirm_loop([c], al, kf_position=info["kf_pos"], **(confirm_kw or {}))
                c["confirm_ok"] = ok
                if ok:
                    c["confirm"] = cf
            if ok:
                c["sim3"] = dict(al["candidates"][0], world=al["world"])
                info["accepted"] = c
                if correct:
                    before = [np.asarray(kf["pose"], np.float64)[:3, :4].copy() for kf in self.keyframes] if optimize else None
                    c["correct"] = self.correct_loop(c, kf_position=info["kf_pos"], min_weight=min_weight, **(correct_kw or {}))
                    if optimize:
                        c["optimize"] = self.optimize_essential_graph(c, poses_before=before, **(optimize_kw or {}))
                    if global_ba:
                        gok, ginfo = self.global_bundle_adjust(**(global_ba_kw or {}))
                        c["global_ba"] = dict(ginfo, ok=gok)
                break
        return info["accepted"] is not None, info

    # ---- two maps into one --------------------------------------------------------------------------------------------------------------
    def absorb(self, other):
        """Appends the map of `other` - a LocalMapper on this context, or the path of a file save_state wrote, which is loaded on this
        context - to this one on the device (mo_map_absorb in include/vslam_amd.h states the rules): its keyframes become the last
        positions, its points the last indices, every key, id, ordinal and offset relocated.  Nothing aligns the two frames (merge_map
        does).  `other` is only read and stays usable.  Both must have the same context and bit-equal camera matrices: ValueError
        otherwise, before the library is touched.
        The host's bookkeeping is spliced: the absorbed keyframe dicts are appended (copies; their ids shifted by 1 + the largest id
        here), the keyframe records and injected dicts concatenated, the serials shifted by this mapper's next serial, the co-visibility
        graph re-keyed by the shifted ids.  Absorbed keyframes have no per-keyframe list until the next cull.  This mapper's
        loop-consistency state, vocabulary, settings and sampling parameters stay.
        Returns the offsets: kf_offset, slot_offset, point_offset, obs_offset, id_offset, ordinal_offset (the library's), kf_id_offset,
        serial_offset, injected_offset, and n_kf / n_points / n_obs after the call."""
        loaded = None
        if not isinstance(other, LocalMapper):
            other = loaded = LocalMapper.load_state(other, context=self.ctx)
        try:
            if other.ctx is not self.ctx:
                raise ValueError("absorb: the two mappers must share one context")
            Ka, Kb = np.asarray(self.camera_matrix, np.float64), np.asarray(other.camera_matrix, np.float64)
            if Ka.shape != Kb.shape or Ka.tobytes() != Kb.tobytes():
                raise ValueError("absorb: the two mappers must have the same camera matrix, bit for bit")
            shift = len(self._injected)
            prm = V.MapAbsorbParams(shift)
            out = V.MapAbsorbOut()
            self._check(self.lib.mo_map_absorb(self._h, other._h, C.byref(prm), C.byref(out)))
            id_base = 1 + max([int(kf["id"]) for kf in self.keyframes], default=-1)
            off = {k: int(getattr(out, k)) for k in ("kf_offset", "slot_offset", "point_offset", "obs_offset", "id_offset", "ordinal_offset")}
            off.update(kf_id_offset=id_base, serial_offset=self._next_serial, injected_offset=shift)
            if other.keyframes or other._n_points:   # (else the library's no-op: no counter moved)
                ordinal = off["ordinal_offset"]
                self._records += [None] * (ordinal - len(self._records))
                self._rec_n += [0] * (ordinal - len(self._rec_n))
                copy_of = {}
                for kf in other.keyframes:
                    k2 = _Keyframe({k: v for k, v in dict.items(kf)})
                    k2["id"] = int(kf["id"]) + id_base
                    k2["pose"] = np.array(kf["pose"], np.float64)
                    k2._mapper, k2._rows = self, kf._rows
                    k2._extra = [int(i) + off["id_offset"] for i in kf._extra]
                    copy_of[id(kf)] = k2
                    self.keyframes.append(k2)
                self._records += [copy_of.get(id(r), r) for r in other._records]
                self._rec_n += list(other._rec_n) + [0] * (len(other._records) - len(other._rec_n))
                self._injected += list(other._injected)
                self._kf_serials += [int(s) + self._next_serial for s in other._kf_serials]
                self._next_serial += other._next_serial
                self._list_rows += [None] * len(other.keyframes)
                for p, row in other.co_visibility_graph.items():
                    for q, n in row.items():
                        self.co_visibility_graph[int(p) + id_base][int(q) + id_base] = n
                self._version += 1
                self._cache = None
            self._sync_size()
            off.update(n_kf=len(self.keyframes), n_points=self._n_points, n_obs=self._n_obs)
            return off
        finally:
            if loaded is not None:
                loaded.close()

    def merge_map(self, other, max_tries=3, keep_unaligned=False, global_ba=False, min_weight=15, n_best=10, max_candidates=4, ratio=0.75,
                  sim3_kw=None, confirm_kw=None, correct_kw=None, global_ba_kw=None):
        """Two maps of one place into one (ORB-SLAM3's Atlas merge on this library's loop calls): absorb(other), then the absorbed side is
        aligned onto this one.  The absorbed keyframes that have map points are walked from the last backwards, at most max_tries of
        them: loop_candidates(kf_position=p, among=this mapper's own positions; min_weight, n_best, max_candidates, ratio), compute_sim3
        (sim3_kw), confirm_loop (confirm_kw).  On the first confirmed candidate correct_loop(corrected=every absorbed position, group=the
        candidate's group; correct_kw) moves the absorbed keyframes and points onto this map's frame and fuses the duplicates;
        global_ba=True then runs global_bundle_adjust (global_ba_kw).  Needs a vocabulary (this mapper's is used; the database
        recounts the absorbed keyframes lazily).
        When nothing confirms and keep_unaligned is false, the absorbed points and keyframes are taken out again by erase_map_points and
        erase_keyframes: arrays() and the keyframe list are those of before the call.  As after any erase, nothing is rewound: ordinals,
        the id bound, serials, the keyframe records and the injected dicts keep the absorbed side's share.
        Returns a dict: `aligned`, `kf_pos` and `cand_pos` (the asking absorbed position and the winning position of this side, -1), `scale`,
        `R`, `t` and `world` of the confirmed similarity (None), `tries`, `offsets` (absorb's), `kept` (the absorbed side is still in the
        map), `correct` (correct_loop's info, its counts among it; None) and `global_ba` ((ok, info); None)."""
        if self.vocabulary is None:
            raise ValueError("merge_map needs a vocabulary (set_vocabulary or train_vocabulary)")
        off = self.absorb(other)
        n0, n_kf = off["kf_offset"], len(self.keyframes)
        absorbed = list(range(n0, n_kf))
        res = {"aligned": False, "kf_pos": -1, "cand_pos": -1, "scale": None, "R": None, "t": None, "world": None, "tries": 0, "offsets": off,
               "kept": True, "correct": None, "global_ba": None}
        own = np.zeros(n_kf, bool)
        own[:n0] = True
        seen = np.zeros(n_kf, bool)
        if self._n_points and n_kf:
            k = self.arrays()["obs_kf"].astype(np.int64)
            k = np.where(k < 0, k + n_kf, k)
            seen[k[(k >= 0) & (k < n_kf)]] = True
        if n0:
            for p in reversed(absorbed):
                if res["tries"] >= int(max_tries):
                    break
                if not seen[p]:
                    continue
                res["tries"] += 1
                info = self.loop_candidates(p, min_weight, n_best, max_candidates, ratio, among=own)
                if not info["candidates"]:
                    continue
                ok, al = self.compute_sim3(info, **(sim3_kw or {}))
                if not ok:
                    continue
                ok, cf = self.confirm_loop(info, al, **(confirm_kw or {}))
                if not ok:
                    continue
                win = cf["candidates"][int(cf["win"])]
                group = info["candidates"][int(cf["win"])]["group"]
                res["correct"] = self.correct_loop(cf, kf_position=p, corrected=absorbed, group=group, **(correct_kw or {}))
                res.update(aligned=True, kf_pos=p, cand_pos=int(win["pos"]), scale=float(win["scale"]), R=win["R"].copy(), t=win["t"].copy(),
                           world=cf["world"])
                break
        if res["aligned"]:
            if global_ba:
                res["global_ba"] = self.global_bundle_adjust(**(global_ba_kw or {}))
        elif not keep_unaligned:
            if self._n_points > off["point_offset"]:
                self.erase_map_points(np.arange(off["point_offset"], self._n_points))
            if absorbed:
                self.erase_keyframes(absorbed)
            res["kept"] = False
        return res

    # ---- device map -> host -----------------------------------------------------------------------------------------------------
    def _sync_size(self):
        s = (C.c_int64 * 6)()
        self._check(self.lib.mo_map_sizes(self._h, s))
        self._n_points = int(s[1])
        self._n_obs = int(s[2])
        self._list_n = int(s[3])

    def _download(self, field, dtype, count, shape=None):
        a = np.empty(count, dtype)
        self._check(self.lib.mo_map_download(self._h, field, V._ptr(a) if count else None, a.nbytes))
        return a.reshape(shape) if shape else a

    def arrays(self):
        """the map as arrays: xyz [n][3] f32, color [n][3] u8, id, obs_off [n + 1], obs_kf, obs_kp, dref_kf, dref_row"""
        if self._cache is None:
            n, no = self._n_points, self._n_obs
            self._cache = {"xyz": self._download(0, np.float32, n * 3, (n, 3)), "color": self._download(1, np.uint8, n * 3, (n, 3)),
                           "id": self._download(2, np.int32, n), "obs_off": self._download(3, np.int32, n + 1),
                           "obs_kf": self._download(4, np.int32, no), "obs_kp": self._download(5, np.int32, no),
                           "dref_kf": self._download(6, np.int32, n), "dref_row": self._download(7, np.int32, n)}
        return self._cache

    def list_arrays(self):
        """per-keyframe lists of the last cull: offsets [rows + 1], ids (rows in the keyframe positions of that cull)"""
        if self._lists is None:
            rows = self._list_n
            if rows == 0:
                self._lists = (np.zeros(1, np.int32), np.zeros(0, np.int32))
            else:
                lo = self._download(8, np.int32, rows + 1)
                self._lists = (lo, self._download(9, np.int32, int(lo[-1])))
        return self._lists

    def _kf_list(self, kf):
        pos = next((i for i, k in enumerate(self.keyframes) if k is kf), None)
        if pos is None or pos >= len(self._list_rows) or self._list_rows[pos] is None:
            return list(kf._extra)
        lo, ids = self.list_arrays()
        r = self._list_rows[pos]
        if r + 1 >= len(lo):
            return list(kf._extra)
        return ids[lo[r]:lo[r + 1]].tolist() + kf._extra

    def _point(self, i):
        a = self.arrays()
        d = int(a["dref_kf"][i])
        if d < 0:
            return self._injected[-d - 1]
        o0, o1 = int(a["obs_off"][i]), int(a["obs_off"][i + 1])
        return {"id": int(a["id"][i]), "position": a["xyz"][i].copy(), "color": a["color"][i].copy(),
                "observed_keyframes": dict(zip(a["obs_kf"][o0:o1].tolist(), a["obs_kp"][o0:o1].tolist())),
                "descriptor": self._records[d]["descriptors"][int(a["dref_row"][i])]}

    def _obs_counts(self):
        off = self.arrays()["obs_off"]
        return np.diff(off)

    # ---- output ------------------------------------------------------------------------------------------------------------------
    def _save_map(self):
        if self._n_points == 0:
            return
        nw = C.c_int64(0)
        self._check(self.lib.mo_map_write_ply(self._h, str(self.output_path).encode(), self.min_observations, C.byref(nw)))
        if nw.value:
            print(f"Saved map with {nw.value} points to {self.output_path}")

    def save_map(self):
        """writes the PLY now (for save_every_keyframe=False)"""
        self._save_map()

    # ---- the whole state in one file ------------------------------------------------------------------------------------------------
    def export_state(self):
        """The device map's snapshot as a dict of numpy arrays (mo_map_export in include/vslam_amd.h states the canonical form):
        `dims` (int64, vslam_amd.snapshot.DIM_NAMES) and the arrays vslam_amd.snapshot.array_specs names.  The map is not changed."""
        from vslam_amd import snapshot as S
        return S.export_map(self.lib, self._h, self._check)

    def save_state(self, path, images="last", compressed=False):
        """Writes the mapper - the device map's snapshot, the camera matrix and the host's bookkeeping - to one .npz at `path` (the path
        as given), from which load_state makes a mapper that returns the bytes this one returns, for every call and every later edit.
        images="last": the file holds the image the next add_keyframe colours its points from (the device's copy) and the last
        keyframe dict's own image; the loaded keyframe dicts of earlier keyframes carry image=None; "all": every keyframe's image as
        well.  An attached vocabulary's two arrays are embedded.  Of a dict given to update_map_points the keys id, position, color,
        descriptor and observed_keyframes are kept.  No call may be in flight on the map."""
        from vslam_amd import snapshot as S
        if images not in ("last", "all"):
            raise ValueError("images: \"last\" or \"all\"")
        a = self.export_state()
        out = {"format_version": np.array(S.FORMAT_VERSION, np.int64), "dims": a["dims"]}
        out.update({"map_" + k: v for k, v in a.items() if k != "dims"})
        n_kf = len(self.keyframes)
        out["camera_matrix"] = np.asarray(self.camera_matrix, np.float64).reshape(3, 3)
        out["settings"] = np.array([self.redundancy_threshold, self.min_observations, self.culling_threshold, float(bool(self.save_every_keyframe))],
                                   np.float64)
        out["sampling"] = np.array([self.n_hyp, self.seed, self.pair_index_base], np.uint64)
        out["kf_ids"] = np.array([int(kf["id"]) for kf in self.keyframes], np.int64)
        out["kf_poses"] = np.array([np.asarray(kf["pose"], np.float64).reshape(4, 4) for kf in self.keyframes], np.float64).reshape(n_kf, 4, 4)
        out["kf_serials"] = np.array(self._kf_serials, np.int64)
        out["next_serial"] = np.array(self._next_serial, np.int64)
        out["list_rows"] = np.array([-1 if r is None else int(r) for r in self._list_rows], np.int64)
        out["covis"] = np.array([(int(p), int(q), int(n)) for p, row in self.co_visibility_graph.items() for q, n in row.items()],
                                np.int64).reshape(-1, 3)
        rec_n = list(self._rec_n) + [0] * (len(self._records) - len(self._rec_n))
        out["rec_n"] = np.array(rec_n, np.int64)
        # the descriptor rows that points name in keyframes no longer in the map
        ref, row = a["dref_kf"].astype(np.int64), a["dref_row"].astype(np.int64)
        live = np.zeros(len(self._records) + 1, bool)
        live[a["kf_ord"]] = True
        dead = np.unique(np.stack([ref, row], 1)[(ref >= 0) & ~live[np.clip(ref, 0, len(self._records))]], axis=0) if len(ref) else np.zeros((0, 2), np.int64)
        out["dead_ref"] = dead.reshape(-1, 2)
        out["dead_desc"] = np.array([np.asarray(self._records[int(k)]["descriptors"][int(r)], np.uint8).reshape(32) for k, r in dead.tolist()],
                                    np.uint8).reshape(-1, 32)
        # the injected dicts that points still name
        inj = np.unique(-ref[ref < 0] - 1) if len(ref) else np.zeros(0, np.int64)
        nj = len(inj)
        flags, col, desc = np.zeros((nj, 3), np.uint8), np.zeros((nj, 3), np.uint8), np.zeros((nj, 32), np.uint8)
        ids, pos, obs, obs_off = np.zeros(nj, np.int64), np.zeros((nj, 3), np.float64), [], np.zeros(nj + 1, np.int64)
        for x, j in enumerate(inj.tolist()):
            mp = self._injected[j]
            ids[x] = int(mp.get("id", 0))
            pos[x] = np.asarray(mp["position"], np.float64).reshape(3)
            if "color" in mp:
                c = np.asarray(mp["color"]).reshape(-1)
                flags[x, 0], col[x] = 1, (c[:3] if c.size >= 3 else np.repeat(c[:1], 3))
            if mp.get("descriptor") is not None:
                flags[x, 1], desc[x] = 1, np.asarray(mp["descriptor"], np.uint8).reshape(32)
            if "observed_keyframes" in mp:
                flags[x, 2] = 1
                obs += [(int(k), int(v)) for k, v in mp["observed_keyframes"].items()]
            obs_off[x + 1] = len(obs)
        out.update(n_injected=np.array(len(self._injected), np.int64), inj_index=inj.astype(np.int64), inj_id=ids, inj_pos=pos, inj_flags=flags,
                   inj_color=col, inj_desc=desc, inj_obs_off=obs_off, inj_obs=np.array(obs, np.int64).reshape(-1, 2))
        lc = self._loop_consistency
        groups = lc.groups if lc is not None else []
        out["lc_threshold"] = np.array(lc.threshold if lc is not None else -1, np.int64)
        out["lc_counts"] = np.array([int(n) for _, n in groups], np.int64)
        out["lc_off"] = np.concatenate([[0], np.cumsum([len(g) for g, _ in groups])]).astype(np.int64)
        out["lc_serials"] = np.array([s for g, _ in groups for s in sorted(g)], np.int64)
        voc = self.vocabulary
        out["vocab_words"] = np.array(voc.words, np.uint8).reshape(-1, 32) if voc is not None else np.zeros((0, 32), np.uint8)
        out["vocab_weights"] = np.array(voc.weights, np.int32).reshape(-1) if voc is not None else np.zeros(0, np.int32)
        out["images_all"] = np.array(1 if images == "all" else 0, np.int64)
        shapes = []
        if images == "all":
            for k, kf in enumerate(self.keyframes):
                img = np.ascontiguousarray(kf["image"], np.uint8) if kf["image"] is not None else np.zeros((0, 0), np.uint8)
                shapes.append((img.shape[0], img.shape[1], 0 if img.ndim == 2 else img.shape[2]))
                out["kf_image_%d" % k] = img
        out["image_shapes"] = np.array(shapes, np.int64).reshape(-1, 3)
        # the last keyframe dict's own image: the device's current image is that of the last keyframe ever stored, which may be gone
        last = self.keyframes[-1]["image"] if self.keyframes else None
        last = np.ascontiguousarray(last, np.uint8) if last is not None else np.zeros((0, 0), np.uint8)
        out["last_image"] = last
        out["last_image_size"] = np.array(self._default_image_size() if self.keyframes else (0, 0), np.int64)
        with open(path, "wb") as fh:   # (the path as given: np.savez would append .npz to a name without it)
            (np.savez_compressed if compressed else np.savez)(fh, **out)

    @classmethod
    def load_state(cls, path, context=None, capacity=None, output_path=None):
        """A mapper from a file save_state wrote.  The file is checked completely - version, presence, dtype, shape and mutual
        consistency of every array (vslam_amd.snapshot.check_file) - before a context is created or the library touched; a bad file
        raises ValueError naming the array.  capacity: as the constructor's, by default what the snapshot needs (the library takes the
        larger of the two anyway).  The loaded map has no dead keyframe slots; keyframe ordinals, serials, ids and the sampling stream of
        the next keyframe pair continue.  Keyframe dicts carry the stored rows as `keypoints` (vslam_amd.KP_DTYPE) and `descriptors`."""
        from vslam_amd import snapshot as S
        from vslam_amd.loop import LoopConsistency
        with np.load(path, allow_pickle=False) as z:
            f = S.check_file(z)
        d = dict(zip(S.DIM_NAMES, (int(x) for x in f["dims"])))
        self = cls.__new__(cls)
        n_hyp, seed, base = (int(v) for v in f["sampling"])
        self._init_host_state(f["camera_matrix"].copy(), output_path, bool(f["settings"][3]), context, n_hyp, seed, base)
        self.redundancy_threshold, self.culling_threshold = float(f["settings"][0]), float(f["settings"][2])
        self.min_observations = int(f["settings"][1])
        ctx = self.ctx
        cap = capacity if capacity is not None else (0, 0, 0, 0)

        def check(rc):
            if rc != V.MO_OK:
                err = self.lib.mo_last_error(ctx.h).decode()
                raise (ValueError("state file: the library refuses the snapshot: " + err) if rc == V.MO_ERR_ARG else V.NativeError(rc, err))
        self._adopt(S.import_map(self.lib, ctx.h, f, cap, check))
        # the keyframes: the stored rows by position
        n_kf = d["n_kf"]
        off = np.concatenate([[0], np.cumsum(f["kf_cnt"], dtype=np.int64)])
        last_img = f["last_image"].copy() if f["last_image"].size else None
        if n_kf:
            self._image_size = tuple(int(v) for v in f["last_image_size"])
        self._records = [None] * len(f["rec_n"])
        self._rec_n = [int(v) for v in f["rec_n"]]
        for k in range(n_kf):
            img = f["kf_image_%d" % k].copy() if int(f["images_all"]) else (last_img if k == n_kf - 1 else None)
            kf = _Keyframe({"id": int(f["kf_ids"][k]), "image": img, "keypoints": f["kf_kps"][off[k]:off[k + 1]].copy(),
                            "descriptors": f["kf_desc"][off[k]:off[k + 1]].copy(), "pose": f["kf_poses"][k].copy()})
            kf._mapper, kf._extra, kf._rows = self, [], int(f["kf_cnt"][k])
            self.keyframes.append(kf)
            self._records[int(f["kf_ord"][k])] = kf
        # the descriptor rows of removed keyframes that points still name: a record of those rows alone
        for (k, r), desc in zip(f["dead_ref"].tolist(), f["dead_desc"]):
            if self._records[k] is None:
                self._records[k] = {"descriptors": {}}
            self._records[k]["descriptors"][r] = desc.copy()
        self._injected = [None] * int(f["n_injected"])
        for x, j in enumerate(f["inj_index"].tolist()):
            mp = {"id": int(f["inj_id"][x]), "position": f["inj_pos"][x].copy()}
            if f["inj_flags"][x, 0]:
                mp["color"] = f["inj_color"][x].copy()
            if f["inj_flags"][x, 1]:
                mp["descriptor"] = f["inj_desc"][x].copy()
            if f["inj_flags"][x, 2]:
                mp["observed_keyframes"] = {int(a): int(b) for a, b in f["inj_obs"][f["inj_obs_off"][x]:f["inj_obs_off"][x + 1]].tolist()}
            self._injected[j] = mp
        for p, q, n in f["covis"].tolist():
            self.co_visibility_graph[p][q] = n
        self._list_rows = [None if r < 0 else int(r) for r in f["list_rows"].tolist()]
        self._kf_serials = [int(v) for v in f["kf_serials"]]
        self._next_serial = int(f["next_serial"])
        if int(f["lc_threshold"]) >= 0:
            self._loop_consistency = LoopConsistency(int(f["lc_threshold"]))
            lo = f["lc_off"]
            self._loop_consistency.groups = [(frozenset(f["lc_serials"][lo[g]:lo[g + 1]].tolist()), int(n)) for g, n in enumerate(f["lc_counts"].tolist())]
        self._sync_size()
        if len(f["vocab_weights"]):
            self.set_vocabulary(V.Vocabulary.from_arrays(f["vocab_words"], f["vocab_weights"], context=ctx))
        return self

    def _filter_map_points(self):
        a = self.arrays()
        keep = self._obs_counts() >= self.min_observations
        return a["xyz"][keep], a["color"][keep]

    def get_map_statistics(self):
        n = self._n_points
        cnt = self._obs_counts() if n else np.zeros(0)
        return {"num_keyframes": len(self.keyframes), "num_map_points": n,
                "num_filtered_points": int((cnt >= self.min_observations).sum()),
                "avg_observations_per_point": np.mean(cnt) if n else 0,
                "map_density": n / len(self.keyframes) if len(self.keyframes) > 0 else 0}

    def visualize_map(self, width=800, height=600):
        """top-down (x, z) drawing of the filtered points and the keyframe trajectory; needs cv2 (drawing is not ported)"""
        try:
            import cv2
        except ImportError as e:
            raise ImportError("LocalMapper.visualize_map draws with cv2, which is not installed") from e
        canvas = np.zeros((height, width, 3), np.uint8)
        pts, cols = self._filter_map_points()
        if len(pts) == 0:
            return canvas
        lo, ext = pts.min(0), pts.max(0) - pts.min(0)
        m = 50
        sx = (width - 2 * m) / ext[0] if ext[0] > 0 else 1
        sz = (height - 2 * m) / ext[2] if ext[2] > 0 else 1
        sc = min(sx, sz)

        def to_px(p):
            return int(m + (p[0] - lo[0]) * sc), int(m + (p[2] - lo[2]) * sc)
        for p, c in zip(pts, cols):
            cv2.circle(canvas, to_px(p), 1, c.tolist(), -1)
        centres = self.get_camera_trajectory()
        if len(self.keyframes) > 1:
            for a, b in zip(centres[:-1], centres[1:]):
                cv2.line(canvas, to_px(a), to_px(b), (0, 255, 0), 2)
            cv2.circle(canvas, to_px(centres[-1]), 5, (0, 0, 255), -1)
        font = cv2.FONT_HERSHEY_SIMPLEX
        cv2.putText(canvas, f"Map Points: {len(pts)}", (10, 20), font, 0.5, (255, 255, 255), 1)
        cv2.putText(canvas, f"Keyframes: {len(self.keyframes)}", (10, 40), font, 0.5, (255, 255, 255), 1)
        return canvas

    def get_camera_trajectory(self):
        cs = [-kf["pose"][:3, :3].T @ kf["pose"][:3, 3] for kf in self.keyframes]
        return np.array(cs) if cs else np.array([])

    def get_keyframe_by_id(self, keyframe_id):
        return next((kf for kf in self.keyframes if kf["id"] == keyframe_id), None)

    def get_map_point_by_id(self, map_point_id):
        hit = np.flatnonzero(self.arrays()["id"] == map_point_id) if self._n_points else []
        return self._point(int(hit[0])) if len(hit) else None

    def find_connected_keyframes(self, keyframe_id, min_connections=15):
        if keyframe_id not in self.co_visibility_graph:
            return []
        return [k for k, n in self.co_visibility_graph[keyframe_id].items() if n >= min_connections]
