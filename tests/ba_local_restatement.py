"""numpy restatement of the set form of the local bundle adjustment (mo_map_bundle_adjust_local in include/vslam_amd.h) and of the
observation erase (mo_map_erase_observations).  The candidate rule and the set form of problem() are restated here; the steps are
tests/ba_restatement's own (lm_step, the costs, the classification), run through its bundle_adjust with the set rule in problem()'s
place."""
import numpy as np

from tests import ba_restatement as BR


def covisibility(obs_off, obs_kf, obs_kp, counts):
    """W [n_kf][n_kf]: the points with a valid observation at p and at q (a point seen twice in a keyframe counts once)"""
    n = len(counts)
    W = np.zeros((n, n), np.int32)
    for v in BR.valid_edges(obs_off, obs_kf, obs_kp, counts):
        ks = sorted({k for k, _, _ in v})
        for a in ks:
            for b in ks:
                W[a, b] += 1
    return W


def candidates(W, kf_pos=-1, n_best=15, min_weight=15):
    """C of the covisible form: kf_pos (-1: the last) and its n_best heaviest neighbours q with W[kf_pos][q] >= max(min_weight, 1),
    heaviest first, ties to the later position; position 0 dropped.  Sorted positions."""
    n = len(W)
    if n == 0:
        return []
    if not 0 <= n_best <= 15:
        raise ValueError("n_best must be in 0 .. 15")
    p = n - 1 if kf_pos < 0 else int(kf_pos)
    floor = max(int(min_weight), 1)
    nb = sorted((q for q in range(n) if q != p and W[p][q] >= floor), key=lambda q: (W[p][q], q), reverse=True)[:n_best]
    return sorted(q for q in set([p] + nb) if q != 0)


def mask_candidates(free, n_kf):
    """C of the mask form: the named positions (a bool mask or a position list) without position 0; ValueError for more than 16"""
    sel = np.asarray(free)
    pos = np.flatnonzero(sel).tolist() if sel.dtype == np.bool_ else sorted(set(int(k) for k in sel.reshape(-1)))
    pos = [k for k in pos if k != 0]
    if len(pos) > 16:
        raise ValueError("more than 16 free keyframes")
    return pos


def problem_set(obs_off, obs_kf, obs_kp, counts, cand):
    """problem() of tests/ba_restatement over the set `cand` (positions, 0 not among them): (local mask, free, fixed, per-point edges)"""
    n_kf = len(counts)
    C = set(int(k) for k in cand)
    assert 0 not in C and len(C) <= 16
    edges = BR.valid_edges(obs_off, obs_kf, obs_kp, counts)
    local = np.array([len(v) >= 2 and any(k in C for k, _, _ in v) for v in edges], bool)
    seen = set(k for v, l in zip(edges, local) if l for k, _, _ in v)
    fixed = [p for p in range(n_kf) if p in seen and p not in C]
    free = []
    for p in sorted(C):
        if p not in seen:
            continue               # a candidate without an edge to a local point is outside the problem
        if len(fixed) < 2:
            fixed.append(p)        # the gauge
        else:
            free.append(p)
    return local, free, fixed, edges


def bundle_adjust_set(obs_off, obs_kf, obs_kp, counts, kf_xy, kf_oct, xyz, K, poses, cand, **kw):
    """ba_restatement.bundle_adjust over the set `cand`; the result gains "candidates" """
    saved = BR.problem
    BR.problem = lambda off, okf, okp, cnt, window: problem_set(off, okf, okp, cnt, cand)
    try:
        r = BR.bundle_adjust(obs_off, obs_kf, obs_kp, counts, kf_xy, kf_oct, xyz, K, poses, **kw)
    finally:
        BR.problem = saved
    r["candidates"] = sorted(int(k) for k in cand)
    return r


def restate_set(s, poses, xyz, cand, **kw):
    """bundle_adjust_set on a tests/ba_scene.Scene-like world"""
    from tests.ba_scene import K
    return bundle_adjust_set(s.obs_off, s.obs_kf, s.obs_kp, s.counts, s.kxy, s.octave, xyz, K, np.array([np.asarray(T)[:3, :4] for T in poses]), cand, **kw)


def erase_entries(obs_off, obs_kf, obs_kp, flags):
    """the observation arrays without the flagged entries: (obs_off, obs_kf, obs_kp, n_erased, n_under).  The survivors keep order and
    bytes; n_under counts the points that lost an entry and now hold fewer than two."""
    obs_off = np.asarray(obs_off)
    keep = np.asarray(flags).reshape(-1) == 0
    assert len(keep) == len(obs_kf) == int(obs_off[-1])
    S = np.concatenate([[0], np.cumsum(keep)]).astype(np.int32)
    off = S[obs_off]
    before, after = np.diff(obs_off), np.diff(off)
    return off.astype(np.int32), np.asarray(obs_kf)[keep], np.asarray(obs_kp)[keep], int((~keep).sum()), int(((after < before) & (after < 2)).sum())


def outlier_flags(r, min_inliers=50):
    """the entries erase_outliers removes behind the restated adjustment r: class 2, when the problem ran (a free keyframe and a local
    point) and ended with >= min_inliers inliers"""
    ran = r["n_free"] > 0 and r["n_local"] > 0
    return (r["edge_inlier"] == 2) & bool(ran and r["n_inliers"] >= min_inliers)
