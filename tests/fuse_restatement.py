"""numpy restatement of LocalMapper.fuse_map_points (mo_map_fuse in include/vslam_amd.h): targets, local points and their representative
descriptors, the search by projection under the store's own P, claims, owners, merge components, survivors and the merged observation
lists.  Exact integers given the map; every floating-point threshold decision reports how far it was from going the other way."""
import numpy as np

from tests.reloc_restatement import hamming
from tests.track_restatement import _info, _power, local_points, projection_matrix, representatives, valid_observations

FIELDS = ("xyz", "color", "id", "obs_off", "obs_kf", "obs_kp", "dref_kf", "dref_row")
COUNTS = ("n_targets", "n_local", "n_pairs", "n_cand", "n_proposals", "n_gained", "n_edges", "n_absorbed", "n_points", "n_obs")


def store_P(K, poses):
    """P = K [R | t] per keyframe position from 4x4 poses, as projection_matrix forms it (hand-made maps; a device map's P is what the
    mapper stored)"""
    return [projection_matrix(K, T) for T in poses]


def as_arrays(xyz, obs, ids=None, color=None):
    """map arrays from positions and per-point [(key, row)] lists as stored (keys may be stale or negative)"""
    n = len(obs)
    off = np.zeros(n + 1, np.int32)
    okf, okp = [], []
    for i, v in enumerate(obs):
        okf += [k for k, _ in v]; okp += [r for _, r in v]
        off[i + 1] = len(okf)
    return {"xyz": np.asarray(xyz, np.float32).reshape(n, 3), "color": np.zeros((n, 3), np.uint8) if color is None else np.asarray(color, np.uint8),
            "id": np.arange(n, dtype=np.int32) if ids is None else np.asarray(ids, np.int32), "obs_off": off,
            "obs_kf": np.array(okf, np.int32), "obs_kp": np.array(okp, np.int32), "dref_kf": np.zeros(n, np.int32), "dref_row": np.zeros(n, np.int32)}


def lists_of(a):
    """per point [(key, row)] as stored"""
    return [list(zip(a["obs_kf"][a["obs_off"][i]:a["obs_off"][i + 1]].tolist(), a["obs_kp"][a["obs_off"][i]:a["obs_off"][i + 1]].tolist()))
            for i in range(len(a["obs_off"]) - 1)]


def fuse(a, kf_P, kf_xy, kf_oct, kf_desc, w, h, window=10, radius=3.0, scale_factor=1.2, max_dist=50, chi2=5.991, ties=1):
    """(fused arrays, into, counts, margins).  a: the map arrays (FIELDS); kf_P / kf_xy / kf_oct / kf_desc by keyframe position.
    margins: per kind of threshold decision ("z", "border", "r", "chi2", "max_dist") the smallest distance of any decided value from its
    threshold over all pairs, and "min" over the kinds.  ties = -1 is the WRONG rule - equal distances go to the higher keypoint row - for
    the tests that show a tie case would notice it (tests/test_fuse_cpu.py)."""
    off, okf, okp = a["obs_off"], a["obs_kf"], a["obs_kp"]
    n, n_kf = len(off) - 1, len(kf_desc)
    cnt = dict.fromkeys(COUNTS, 0)
    cnt["n_points"], cnt["n_obs"] = n, int(off[-1]) if n else 0
    margins = {k: np.inf for k in ("z", "border", "r", "chi2", "max_dist")}
    same = {f: np.array(a[f]).copy() for f in FIELDS}
    into = np.arange(n, dtype=np.int32)

    def done(arrays, into):
        margins["min"] = min(margins.values())
        return arrays, into, cnt, margins
    if n == 0 or n_kf == 0:
        return done(same, into)
    counts = [len(d) for d in kf_desc]
    obs = valid_observations(off, okf, okp, counts)
    lo = n_kf - window if 0 < window < n_kf else 0
    local = local_points(obs, n_kf, window)
    rep, ref = representatives(obs, kf_desc, kf_oct, local)
    cnt["n_targets"], cnt["n_local"] = n_kf - lo, int(local.sum())
    owner = {}
    for i, v in enumerate(obs):
        for k, r in v:
            owner.setdefault((k, r), i)   # ascending i: the lowest point
    X = np.asarray(a["xyz"], np.float32).astype(np.float64)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    claim, proposal = {}, {}
    for k in range(lo, n_kf):
        P = np.asarray(kf_P[k], np.float64).reshape(3, 4)
        pu = P[0, 0] * x + P[0, 1] * y + P[0, 2] * z + P[0, 3]
        pv = P[1, 0] * x + P[1, 1] * y + P[1, 2] * z + P[1, 3]
        pz = P[2, 0] * x + P[2, 1] * y + P[2, 2] * z + P[2, 3]
        kx, ky = np.asarray(kf_xy[k], np.float32)[:, 0].astype(np.float64), np.asarray(kf_xy[k], np.float32)[:, 1].astype(np.float64)
        ko = np.asarray(kf_oct[k], np.int64)
        info = np.array([_info(scale_factor, o) for o in ko])
        for i in np.flatnonzero(local).tolist():
            if any(kk == k for kk, _ in obs[i]):
                continue
            cnt["n_pairs"] += 1
            margins["z"] = min(margins["z"], abs(pz[i]))
            if not pz[i] > 0:
                continue
            u, v = pu[i] / pz[i], pv[i] / pz[i]
            margins["border"] = min(margins["border"], abs(u), abs(u - w), abs(v), abs(v - h))
            if not (u >= 0 and u < w and v >= 0 and v < h):
                continue
            cnt["n_cand"] += 1
            r = radius * _power(scale_factor, ref[i])
            dx, dy = kx - u, ky - v
            gate = np.abs(ko - ref[i]) <= 1
            if gate.any():
                margins["r"] = min(margins["r"], np.abs(np.abs(dx[gate]) - r).min(), np.abs(np.abs(dy[gate]) - r).min())
            near = gate & (np.abs(dx) < r) & (np.abs(dy) < r)
            e = info * (dx * dx + dy * dy)
            if near.any():
                margins["chi2"] = min(margins["chi2"], np.abs(e[near] - chi2).min())
            q = np.flatnonzero(near & (e <= chi2))
            if len(q) == 0:
                continue
            d = hamming(rep[i:i + 1], kf_desc[k][q])[0]
            order = np.lexsort((ties * q, d))   # lowest distance, ties to the lower row
            bd, bq = int(d[order[0]]), int(q[order[0]])
            margins["max_dist"] = min(margins["max_dist"], abs(bd - (max_dist + 0.5)))
            if bd > max_dist:
                continue
            cnt["n_proposals"] += 1
            proposal[(i, k)] = bq
            if (k, bq) not in claim or (bd, i) < claim[(k, bq)]:
                claim[(k, bq)] = (bd, i)
    if not cnt["n_proposals"]:
        return done(same, into)
    # winners: merge edges and gained observations
    parent = list(range(n))

    def find(p):
        while parent[p] != p:
            p = parent[p]
        return p
    gained = [[] for _ in range(n)]
    for (k, row), (_, i) in sorted(claim.items()):
        if (k, row) in owner:
            cnt["n_edges"] += 1
            ra, rb = find(i), find(owner[(k, row)])
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        else:
            cnt["n_gained"] += 1
            gained[i].append((k, row))
    comp = {}
    for i in range(n):
        comp.setdefault(find(i), []).append(i)
    survivor = {}
    for root, mem in comp.items():
        survivor[root] = min(mem, key=lambda j: (-len(obs[j]), j))
    stored = lists_of(a)
    new_list = {}
    for root, mem in comp.items():
        s = survivor[root]
        lst = list(stored[s])
        held = {k for k, _ in obs[s]}
        extra = [e for j in mem if j != s for e in obs[j]] + [e for j in mem for e in sorted(gained[j])]
        for k, row in extra:
            if k not in held:
                held.add(k)
                lst.append((k, row))
        new_list[s] = lst
    keep = sorted(new_list)
    rank = {s: r for r, s in enumerate(keep)}
    into = np.array([rank[survivor[find(i)]] for i in range(n)], np.int32)
    out = {f: np.array(a[f])[keep] for f in ("xyz", "color", "id", "dref_kf", "dref_row")}
    noff = np.zeros(len(keep) + 1, np.int32)
    nkf, nkp = [], []
    for r, s in enumerate(keep):
        nkf += [k for k, _ in new_list[s]]; nkp += [p for _, p in new_list[s]]
        noff[r + 1] = len(nkf)
    out.update(obs_off=noff, obs_kf=np.array(nkf, np.int32), obs_kp=np.array(nkp, np.int32))
    cnt["n_absorbed"] = n - len(keep)
    cnt["n_points"], cnt["n_obs"] = len(keep), len(nkf)
    return done(out, into)


def co_visibility_delta(before, after, into, counts):
    """{(position a < position b): change} of the co-visibility counts: per changed component, the pairs of positions validly observing
    the survivor after, less the same over its members before"""
    ob = valid_observations(before["obs_off"], before["obs_kf"], before["obs_kp"], counts)
    oa = valid_observations(after["obs_off"], after["obs_kf"], after["obs_kp"], counts)
    delta = {}

    def add(v, sign):
        pos = sorted({k for k, _ in v})
        for i in range(len(pos)):
            for j in range(i + 1, len(pos)):
                delta[(pos[i], pos[j])] = delta.get((pos[i], pos[j]), 0) + sign
    for j in range(len(oa)):
        mem = np.flatnonzero(into == j)
        if len(mem) == 1 and len(lists_of_point(before, mem[0])) == len(lists_of_point(after, j)):
            continue
        add(oa[j], 1)
        for i in mem.tolist():
            add(ob[i], -1)
    return {k: d for k, d in delta.items() if d}


def lists_of_point(a, i):
    return a["obs_kf"][a["obs_off"][i]:a["obs_off"][i + 1]]
