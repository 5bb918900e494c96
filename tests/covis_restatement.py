"""numpy restatement of the device covisibility (mo_map_covisibility, mo_map_local_keyframes, mo_map_track_covisible in
include/vslam_amd.h): the matrix of shared points, the K1 / K2 selection with its tie rules, and tracking against the local map of a
keyframe set.  Observations are read by tests/track_restatement.valid_observations; the tracking itself is track_restatement.track."""
import numpy as np

from tests import track_restatement as TR


def positions(obs):
    """per point the sorted distinct keyframe positions of its valid observations (a point seen twice in a keyframe: once)"""
    return [sorted({k for k, _ in v}) for v in obs]


def covisibility(obs_off, obs_kf, obs_kp, counts):
    """W [n_kf][n_kf] int32: W[p][q] = points with a valid observation at p and at q, W[p][p] = points with one at p"""
    n = len(counts)
    W = np.zeros((n, n), np.int32)
    for ks in positions(TR.valid_observations(obs_off, obs_kf, obs_kp, counts)):
        for a in ks:
            for b in ks:
                W[a, b] += 1
    return W


def seed_votes(obs_off, obs_kf, obs_kp, counts, seed_points):
    """votes [n_kf]: every seed entry inside the map votes once for each position its point validly observes"""
    pos = positions(TR.valid_observations(obs_off, obs_kf, obs_kp, counts))
    votes = np.zeros(len(counts), np.int64)
    for i in ([] if seed_points is None else np.asarray(seed_points).reshape(-1).tolist()):
        if 0 <= i < len(pos):
            for k in pos[i]:
                votes[k] += 1
    return votes


def local_keyframes(W, votes=None, ref=None, n_best=10, min_weight=15):
    """{"mask" [n_kf] uint8 (1 = K1, 2 = K2 only), "k1", "k2", "local" (position lists), "ref"}.  ref: the position used when nothing
    votes (None: the last).  Ties, of ref on the votes and of a neighbour on the weight, go to the later position."""
    W = np.asarray(W)
    n = len(W)
    mask = np.zeros(n, np.uint8)
    if n == 0:
        return {"mask": mask, "k1": [], "k2": [], "local": [], "ref": -1}
    votes = np.zeros(n, np.int64) if votes is None else np.asarray(votes)
    if (votes > 0).any():
        k1 = np.flatnonzero(votes > 0).tolist()
        r = max(k1, key=lambda k: (votes[k], k))
    else:
        r = n - 1 if ref is None or ref < 0 else int(ref)
        k1 = [r]
    mask[k1] = 1
    floor = max(int(min_weight), 1)
    for p in k1:
        cand = sorted((q for q in range(n) if q != p and W[p, q] >= floor), key=lambda q: (W[p, q], q), reverse=True)
        for q in cand[:n_best]:
            if mask[q] == 0:
                mask[q] = 2
    return {"mask": mask, "k1": k1, "k2": np.flatnonzero(mask == 2).tolist(), "local": np.flatnonzero(mask).tolist(), "ref": int(r)}


def local_point_mask(obs, kf_mask):
    """the points with a valid observation at a keyframe of the set"""
    return np.array([any(kf_mask[k] for k, _ in v) for v in obs], bool)


def track_covisible(K, pose0, xyz, obs_off, obs_kf, obs_kp, kf_desc, kf_oct, kps, desc, w, h, seed_points=None, ref=None, n_best=10, min_weight=15,
                    **kw):
    """(track_restatement.track's result on the local map of the selected keyframes, the selection)"""
    counts = [len(d) for d in kf_desc]
    obs = TR.valid_observations(obs_off, obs_kf, obs_kp, counts)
    sel = local_keyframes(covisibility(obs_off, obs_kf, obs_kp, counts), seed_votes(obs_off, obs_kf, obs_kp, counts, seed_points), ref, n_best,
                          min_weight)
    local = local_point_mask(obs, sel["mask"])
    rep, ref_oct = TR.representatives(obs, kf_desc, kf_oct, local)
    res = TR.track(K, pose0, xyz, obs_off, obs_kf, obs_kp, kf_desc, kf_oct, kps, desc, w, h, local_map=(rep, ref_oct, int(local.sum())), **kw)
    return res, sel
