"""Worlds for the absorb and merge tests (mo_map_absorb, LocalMapper.merge_map), in numpy alone.

split(w): tests/loop_worlds.LoopWorld mapped in two sessions.  Map A holds the positions 0 .. 19 with the old points, map B the
positions 20 .. 27 - the return keyframes and their fillers - with the duplicates, its observation keys shifted by -20: B's own
positions.  B absorbed into A is the one-session world again, key for key.  Given a world whose return side was rescaled
(tests/test_gpu_sim3._rescaled), B is a map in a frame of its own.

snapshot_of(half): the snapshot dict of such a map written by hand, for the restatement on the CPU.

same_side_world(): four keyframes, two per side, on which a keyframe of the asking side outscores the true match of the other side."""
import numpy as np

from tests import loop_worlds as LW

SPLIT = 20


class Half:
    """a run of keyframes of a world with a run of its points, as a world of its own (the attributes LoopWorld.build reads)"""

    def __init__(self, w, kf, points, shift):
        self.K, self.image_size = w.K, w.image_size
        self.kf_xy, self.kf_desc, self.kf_poses = list(w.kf_xy[kf]), list(w.kf_desc[kf]), [np.array(T, np.float64) for T in w.kf_poses[kf]]
        self.counts = np.array([len(d) for d in self.kf_desc], np.int32)
        self.points = [dict(q, observed_keyframes={k - shift: r for k, r in q["observed_keyframes"].items()}) for q in points]
        self.obs_off, self.obs_kf, self.obs_kp = LW.obs_arrays(self.points)
        self.ids = np.array([q["id"] for q in self.points], np.int64)

    def build(self, ctx, capacity=(32, 512, 4096, 16384), vocabulary=None):
        m = LW.new_mapper(ctx, self.K, capacity, vocabulary)
        for k in range(len(self.kf_desc)):
            LW.add_keyframe(m, self, k)
        m.update_map_points(self.points)
        return m


def split(w, at=SPLIT):
    """(A, B): the keyframes before `at` with the old points, the keyframes from `at` on with the duplicates keyed by B's positions"""
    assert all(max(q["observed_keyframes"]) < at for q in w.points[:w.n_old])
    assert all(min(q["observed_keyframes"]) >= at for q in w.points[w.n_old:])
    return Half(w, slice(0, at), w.points[:w.n_old], 0), Half(w, slice(at, None), w.points[w.n_old:], at)


def snapshot_of(h):
    """the snapshot dict (LocalMapper.export_state's form) of a half built by Half.build, written by hand: the points as
    update_map_points injects them (dref_kf = -(j + 1), life {1, 1, now, 0}), no lists, no images"""
    from tests.absorb_restatement import DIM_NAMES
    from tests.map_worlds import kps_array
    n_kf, n = len(h.kf_desc), len(h.points)
    K = np.asarray(h.K, np.float64)
    d = dict.fromkeys(DIM_NAMES, 0)
    d.update(n_kf=n_kf, kf_rows=int(h.counts.sum()), n_pts=n, n_obs=len(h.obs_kf), kf_stored=n_kf, id_bound=int(h.ids.max()) + 1 if n else 0,
             st_live0=n, st_live1=len(h.obs_kf), img_ch0=1, img_ch1=1)
    life = np.zeros((n, 4), np.int32)
    life[:, :2] = 1
    life[:, 2] = max(n_kf - 1, 0)
    return {"dims": np.array([d[k] for k in DIM_NAMES], np.int64), "kf_cnt": h.counts.copy(), "kf_ord": np.arange(n_kf, dtype=np.int32),
            "kf_kps": np.concatenate([kps_array(np.zeros((0, 2)))] + [kps_array(xy) for xy in h.kf_xy]),
            "kf_desc": np.concatenate([np.zeros((0, 32), np.uint8)] + h.kf_desc).astype(np.uint8),
            "kf_P": np.array([(K @ T[:3, :4]).reshape(12) for T in h.kf_poses], np.float64).reshape(n_kf, 12),
            "xyz": np.array([np.asarray(q["position"], np.float64) for q in h.points], np.float32).reshape(n, 3), "col": np.zeros((n, 3), np.uint8),
            "id": h.ids.astype(np.int32), "dref_kf": -(np.arange(n, dtype=np.int32) + 1), "dref_row": np.zeros(n, np.int32),
            "obs_off": h.obs_off.copy(), "obs_kf": h.obs_kf.copy(), "obs_kp": h.obs_kp.copy(), "life": life,
            "list_off": np.zeros(0, np.int32), "list_ids": np.zeros(0, np.int32), "kf_red": np.zeros(0, np.int32),
            "img0": np.zeros(0, np.uint8), "img1": np.zeros(0, np.uint8)}


# ---- a same-side keyframe that wins unmasked -------------------------------------------------------------------------------------------
SAME_SIDE_AMONG = [1, 1, 0, 0]
SAME_SIDE_KW = dict(min_weight=1)


def same_side_world():
    """Positions 0, 1: the absorbing side; 2, 3: the absorbed side; 3 asks.  3 is connected to 1 alone (one shared point), which shares
    no word with it: min_score 0.  Keyframe 2 has 3's four words and nothing else: score 1.0; keyframe 0 has them and two rows of a
    fifth word: score 2 / 3 (loop_worlds.hand_cases' "groups").  Both have four common words: S = M = {0, 2}, nobody is connected to
    either: acc = score.  Unmasked 0.75 * 1.0 retains 2 alone; with among = the absorbing side, 2 takes no part and 0 is the candidate."""
    frames = [LW._rows(0, 1, 2, 3, 5, 5), LW._rows(5, 6), LW._rows(0, 1, 2, 3), LW._rows(0, 1, 2, 3)]
    return LW.HandWorld(frames, [{3: 0, 1: 0}])
