"""The loop world of tests/loop_worlds.py as the loop confirmation reads it, for the end-to-end tests of LocalMapper.detect_loop(sim3=True,
confirm=True): the restatement's inputs at an asking position, with the true similarity of the world (the rigid motion between the two
cameras, times the factor the return side was rescaled by) in place of the alignment's result.  Plain numpy."""
import numpy as np

from tests import confirm_restatement as CR
from tests import loop_restatement as LR
from tests import loop_worlds as LW


def true_model(w, p, k, factor=1.0):
    """X1 = factor R1 R2^T X2 + (t1 - factor R t2): the same physical point seen from keyframe k (old side) and p (return side, whose
    translations already carry the factor)"""
    T1, T2 = np.asarray(w.kf_poses[p], np.float64), np.asarray(w.kf_poses[k], np.float64)
    R = T1[:3, :3] @ T2[:3, :3].T
    return (float(factor), R, T1[:3, 3] - factor * R @ T2[:3, 3])


def candidates_at(w, p, words, weights):
    """loop_restatement's result for asking position p"""
    return LR.loop_candidates(w.kf_desc, w.obs_off, w.obs_kf, w.obs_kp, words, weights, p)


def inputs_at(w, res, c, p, factor=1.0, **prm):
    """the confirmation's inputs for candidate c of res (every match a seed, the candidate's group, the true model)"""
    k = res["cand"][c]
    n_kf = len(w.kf_desc)
    group = np.zeros((1, n_kf), bool)
    group[0, list(res["group"][c])] = True
    group[0, k] = True
    xyz = np.array([np.asarray(q["position"], np.float64) for q in w.points], np.float32)
    return CR.Inputs(w.K, w.kf_poses, w.kf_xy, [np.zeros(len(a), np.int64) for a in w.kf_xy], w.kf_desc, xyz, w.obs_off, w.obs_kf, w.obs_kp, p, [k],
                     res["cur_point"], [res["match_point"][c]], [res["match_row"][c]], None, [true_model(w, p, k, factor)], group,
                     w.image_size[0], w.image_size[1], **prm)


def true_loop_point(w, p, cur_point, kf_xy_p, lpt, factor=1.0, tol=1.0):
    """the rows of p whose loop_point is not true.  True: the old point j for a row whose own point is DUP_ID + j; for a row without a
    point of its own, the row's keypoint lies within tol pixels of the old point's projection into the asking keyframe (under the pose
    of the world before its return side was rescaled by factor: the translation divided by it)"""
    from tests.map_worlds import project
    T = np.array(w.kf_poses[p], np.float64)
    T[:3, 3] /= factor
    bad = []
    for i in np.flatnonzero(np.asarray(lpt) >= 0):
        x, a = int(lpt[i]), int(cur_point[i])
        if a >= 0:
            ok = w.ids[a] == LW.DUP_ID + w.ids[x]
        else:
            xy, z = project(w.K, T, np.asarray(w.points[x]["position"], np.float64)[None])
            ok = w.ids[x] < LW.DUP_ID and z[0] > 0 and np.abs(xy[0] - np.asarray(kf_xy_p[i], np.float64)).max() < tol
        if not ok:
            bad.append(int(i))
    return bad


class LookAlikeWorld(LW.LoopWorld):
    """The loop world with look-alike rows: each of the keyframes `positions` gains, for every third row that observes a map point, a row without a point
    that holds the same descriptor with one bit flipped, 80 pixels away.  The ratio test of the loop matching refuses these rows' matches
    (two neighbours one bit apart), so the alignment never sees them; the guided search finds them, its window being 7.5 pixels."""

    def __init__(self, positions=(0, 1, 2, 3, 4, 5, 6), every=3):
        super().__init__()
        Wd, Hd = self.image_size
        self.n_alike = {}
        for pos in positions:
            owned = sorted({r for q in self.points for k, r in q["observed_keyframes"].items() if k == pos})
            xy, desc = [self.kf_xy[pos]], [self.kf_desc[pos]]
            for r in owned[::every]:
                d = self.kf_desc[pos][r].copy()
                d[5] ^= np.uint8(4)
                x = self.kf_xy[pos][r] + np.float32([80.0, 0.0])
                if x[0] >= Wd:
                    x = self.kf_xy[pos][r] - np.float32([80.0, 0.0])
                xy.append(x[None]); desc.append(d[None])
            self.kf_xy[pos] = np.vstack(xy).astype(np.float32)
            self.kf_desc[pos] = np.vstack(desc).astype(np.uint8)
            self.n_alike[pos] = len(owned[::every])
        self.counts = np.array([len(d) for d in self.kf_desc], np.int32)


_W = {}


def look_alike_world():
    if "alike" not in _W:
        _W["alike"] = LookAlikeWorld()
    return _W["alike"]
