"""numpy restatement of the keyframe cull by ORB-SLAM2's rule and of the erase that goes with it (mo_map_kf_redundancy,
mo_map_erase_keyframes, mo_map_cull_keyframes in include/vslam_amd.h): plain Python over obs_off / obs_kf / obs_kp, the keyframe row counts
and the per-keyframe octaves.  decide() takes four switches, each the rule a kernel could get wrong; tests/test_kfcull_cpu.py shows that
every constructed world of tests/kfcull_worlds.py decides differently under the switch it is there for."""
import numpy as np


def valid_observations(obs_off, obs_kf, obs_kp, counts):
    """per point the valid observations [(position, row)] in entry order, both non-negative: negative keys and rows count from the end,
    entries that name nothing are skipped (map_obs of csrc/map_store.h)"""
    n_kf = len(counts)
    out = []
    for i in range(len(obs_off) - 1):
        v = []
        for o in range(int(obs_off[i]), int(obs_off[i + 1])):
            k, r = int(obs_kf[o]), int(obs_kp[o])
            if k < 0:
                k += n_kf
            if not 0 <= k < n_kf:
                continue
            if r < 0:
                r += int(counts[k])
            if not 0 <= r < int(counts[k]):
                continue
            v.append((k, r))
        out.append(v)
    return out


def keyframe_observations(valid, kf_oct, later_duplicate=False):
    """per point {position: octave of its observation there}: the first valid observation in entry order (later_duplicate: the last), a
    negative octave as 0; the dict keeps the positions in the order they first appear"""
    out = []
    for v in valid:
        d = {}
        for k, r in v:
            if k in d and not later_duplicate:
                continue
            d[k] = max(int(kf_oct[k][r]), 0)
        out.append(d)
    return out


def covisibility(valid, n_kf):
    W = np.zeros((n_kf, n_kf), np.int32)
    for v in valid:
        pos = sorted({k for k, _ in v})
        for a in pos:
            for b in pos:
                W[a, b] += 1
    return W


def decide(obs_off, obs_kf, obs_kp, counts, kf_oct, kf_pos=-1, min_weight=15, min_observers=3, ratio=0.9, scale_gap=1, protect=None,
           scale_test=True, one_pass=False, later_duplicate=False, ties_earlier=False):
    """the candidates of keyframe kf_pos in order and the decision for each: dict of pos, weight, n_points, n_redundant, removed (lists in
    candidate order) and removed_positions (ascending).  The switches: scale_test=False drops the octave condition; one_pass=True decides
    every candidate on the map as it stands; later_duplicate=True takes the last of several observations in one keyframe; ties_earlier=True
    orders equal weights by the earlier position."""
    n_kf = len(counts)
    res = {"pos": [], "weight": [], "n_points": [], "n_redundant": [], "removed": [], "removed_positions": []}
    if n_kf < 2 or len(obs_off) < 2:
        return res
    valid = valid_observations(obs_off, obs_kf, obs_kp, counts)
    seen = keyframe_observations(valid, kf_oct, later_duplicate)
    W = covisibility(valid, n_kf)
    p = n_kf - 1 if kf_pos < 0 else kf_pos
    cand = [q for q in range(n_kf) if q != p and W[p, q] >= max(min_weight, 1)]
    cand.sort(key=lambda q: (-int(W[p, q]), q if ties_earlier else -q))
    gone = set()
    for c in cand:
        n_points = n_red = 0
        for d in seen:
            if c not in d:
                continue
            n_points += 1
            lim = d[c] + scale_gap
            n = sum(1 for q, o in d.items() if q != c and q not in gone and (not scale_test or o <= lim))
            n_red += n >= min_observers
        rm = c != 0 and not (protect is not None and protect[c]) and float(n_red) > ratio * float(n_points)
        if rm and not one_pass:
            gone.add(c)
        res["pos"].append(c); res["weight"].append(int(W[p, c])); res["n_points"].append(n_points); res["n_redundant"].append(n_red)
        res["removed"].append(bool(rm))
    res["removed_positions"] = sorted(c for c, r in zip(res["pos"], res["removed"]) if r)
    return res


def erase(obs_off, obs_kf, obs_kp, counts, positions):
    """(obs_off, obs_kf, obs_kp, counts) of the map without the keyframes at `positions`: every point keeps, in entry order, its valid
    observations at surviving positions as (position after the removal, non-negative row)"""
    n_kf = len(counts)
    gone = {int(q) for q in positions}
    assert all(0 <= q < n_kf for q in gone)
    new_pos, k = {}, 0
    for q in range(n_kf):
        if q not in gone:
            new_pos[q] = k
            k += 1
    off, okf, okp = [0], [], []
    for v in valid_observations(obs_off, obs_kf, obs_kp, counts):
        for q, r in v:
            if q in new_pos:
                okf.append(new_pos[q]); okp.append(r)
        off.append(len(okf))
    return (np.array(off, np.int32), np.array(okf, np.int32), np.array(okp, np.int32),
            np.array([c for q, c in enumerate(counts) if q not in gone], np.int32))
