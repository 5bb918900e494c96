"""numpy restatement of LocalMapper.correct_loop (mo_map_loop_correct in include/vslam_amd.h), rule by rule in the header's order: the
transform A and the corrected poses in the library's operation order (f64), the moved points, the direct replacements, the search of the
loop points in the corrected keyframes, components, survivors and merged lists.  The pieces mo_map_fuse shares with this call are taken
from tests/fuse_restatement.py and tests/track_restatement.py (observation reading, representatives, projection matrices, distances,
array helpers); fuse() itself searches a recency window of contiguous targets with the points of that window, so the search loop is
written out here over the loop points and a position list, with the same margins."""
import numpy as np

from tests.fuse_restatement import FIELDS, lists_of
from tests.reloc_restatement import hamming
from tests.track_restatement import _info, _power, projection_matrix, representatives, valid_observations

COUNTS = ("n_corrected", "n_moved", "n_loop_points", "n_direct_edges", "n_direct_gained", "n_pairs", "n_cand", "n_proposals", "n_gained", "n_edges",
          "n_absorbed", "n_points", "n_obs")


def transform(poses, p, q, s, R, t):
    """(A [3][4], A_scale, RA, tA): rule 1 in the library's order, every sum left to right"""
    Tp, Tc = np.asarray(poses[p], np.float64), np.asarray(poses[q], np.float64)
    Rp, tp, Rc, tc = Tp[:3, :3], Tp[:3, 3], Tc[:3, :3], Tc[:3, 3]
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    s = float(s)
    Rq, d = np.zeros((3, 3)), np.zeros(3)
    for i in range(3):
        for j in range(3):
            Rq[i, j] = R[i, 0] * Rc[0, j] + R[i, 1] * Rc[1, j] + R[i, 2] * Rc[2, j]
        u = R[i, 0] * tc[0] + R[i, 1] * tc[1] + R[i, 2] * tc[2]
        d[i] = tp[i] - (s * u + t[i])
    inv = 1.0 / s
    RA, tA, A = np.zeros((3, 3)), np.zeros(3), np.zeros((3, 4))
    for i in range(3):
        for j in range(3):
            RA[i, j] = Rq[0, i] * Rp[0, j] + Rq[1, i] * Rp[1, j] + Rq[2, i] * Rp[2, j]
            A[i, j] = inv * RA[i, j]
        tA[i] = Rq[0, i] * d[0] + Rq[1, i] * d[1] + Rq[2, i] * d[2]
        A[i, 3] = inv * tA[i]
    return A, inv, RA, tA


def corrected_poses(poses, cpos, s, RA, tA):
    """rule 2: [n_kf][3][4], the corrected positions rewritten"""
    out = np.array([np.asarray(T, np.float64)[:3, :4] for T in poses]).reshape(len(poses), 3, 4).copy()
    for k in cpos:
        Ri, ti = out[k, :, :3].copy(), out[k, :, 3].copy()
        for i in range(3):
            for j in range(3):
                out[k, i, j] = Ri[i, 0] * RA[j, 0] + Ri[i, 1] * RA[j, 1] + Ri[i, 2] * RA[j, 2]
            v = out[k, i, 0] * tA[0] + out[k, i, 1] * tA[1] + out[k, i, 2] * tA[2]
            out[k, i, 3] = (ti[i] - v) / float(s)
    return out


def move(xyz, A):
    """rule 3's arithmetic: A (X, 1) in f64 from f32, rounded once"""
    X = np.asarray(xyz, np.float32).astype(np.float64)
    A = np.asarray(A, np.float64).reshape(3, 4)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return np.stack([A[d, 0] * x + A[d, 1] * y + A[d, 2] * z + A[d, 3] for d in range(3)], axis=1).astype(np.float32)


def correct(a, K, poses, kf_xy, kf_oct, kf_desc, p, q, model, corrected, group, loop_point, w, h, radius=4.0, scale_factor=1.2, max_dist=50,
            chi2=5.991, A=None, poses_out=None):
    """dict: arrays (the map after the call), into, moved, counts, A, A_scale, poses_out, margins, fused.  a: the map arrays (FIELDS);
    poses: 4x4 per position; model = (s, R, t); corrected / group: masks [n_kf] (group may be None); loop_point: per row of p or None.
    A / poses_out: the call's own, to restate what follows from them (the moved xyz, the projections)."""
    off, okf, okp = a["obs_off"], a["obs_kf"], a["obs_kp"]
    n, n_kf = len(off) - 1, len(kf_desc)
    cnt = dict.fromkeys(COUNTS, 0)
    cnt["n_points"], cnt["n_obs"] = n, int(off[-1]) if n else 0
    margins = {k: np.inf for k in ("z", "border", "r", "chi2", "max_dist")}
    arrays = {f: np.array(a[f]).copy() for f in FIELDS}
    res = {"arrays": arrays, "into": np.arange(n, dtype=np.int32), "moved": np.zeros(n, bool), "counts": cnt, "A": np.eye(4)[:3], "A_scale": 1.0,
           "poses_out": np.array([np.asarray(T, np.float64)[:3, :4] for T in poses]).reshape(n_kf, 3, 4), "margins": margins, "fused": False}

    def done():
        margins["min"] = min(margins.values())
        return res
    if n == 0 or n_kf == 0:
        return done()
    s, R, t = model
    cmask = np.asarray(corrected).astype(bool)
    gmask = np.zeros(n_kf, bool) if group is None else np.asarray(group).astype(bool)
    assert cmask[p] and not (cmask & gmask).any()
    cpos = np.flatnonzero(cmask).tolist()
    cnt["n_corrected"] = len(cpos)
    A0, inv, RA, tA = transform(poses, p, q, s, R, t)
    P0 = corrected_poses(poses, cpos, s, RA, tA)
    res["A"], res["A_scale"], res["poses_out"] = A0, inv, P0
    A_used = A0 if A is None else np.asarray(A, np.float64).reshape(3, 4)
    P_used = P0 if poses_out is None else np.asarray(poses_out, np.float64).reshape(n_kf, 3, 4)
    counts = [len(d) for d in kf_desc]
    obs = valid_observations(off, okf, okp, counts)
    # rule 3
    loop = np.array([any(gmask[k] for k, _ in v) for v in obs], bool)
    moved = np.array([any(cmask[k] for k, _ in v) for v in obs], bool) & ~loop
    res["moved"] = moved
    cnt["n_moved"], cnt["n_loop_points"] = int(moved.sum()), int(loop.sum())
    arrays["xyz"][moved] = move(arrays["xyz"], A_used)[moved]
    owner = {}
    for i, v in enumerate(obs):
        for k, r in v:
            owner.setdefault((k, r), i)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    def unite(x, y):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    # rule 4
    drow = {}
    n_p = counts[p]
    lp = np.full(n_p, -1, np.int64) if loop_point is None else np.asarray(loop_point, np.int64).reshape(-1)[:n_p]
    for r in range(len(lp)):
        L = int(lp[r])
        if not 0 <= L < n:
            continue
        o = owner.get((p, r))
        if o is not None:
            if o != L:
                cnt["n_direct_edges"] += 1
                unite(o, L)
        elif not any(k == p for k, _ in obs[L]) and L not in drow:
            drow[L] = r
            cnt["n_direct_gained"] += 1
    given = {(p, r): L for L, r in drow.items()}
    # rule 5
    rep, ref = representatives(obs, kf_desc, kf_oct, loop)
    X = arrays["xyz"].astype(np.float64)   # (loop points are not moved)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    claim, proposal = {}, {}
    for k in cpos:
        T = np.eye(4)
        T[:3, :4] = P_used[k]
        P = projection_matrix(K, T)
        pu = P[0, 0] * x + P[0, 1] * y + P[0, 2] * z + P[0, 3]
        pv = P[1, 0] * x + P[1, 1] * y + P[1, 2] * z + P[1, 3]
        pz = P[2, 0] * x + P[2, 1] * y + P[2, 2] * z + P[2, 3]
        kx, ky = np.asarray(kf_xy[k], np.float32).reshape(-1, 2)[:, 0].astype(np.float64), np.asarray(kf_xy[k], np.float32).reshape(-1, 2)[:, 1].astype(np.float64)
        ko = np.asarray(kf_oct[k], np.int64)
        info = np.array([_info(scale_factor, o) for o in ko])
        for i in np.flatnonzero(loop).tolist():
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
            qs = np.flatnonzero(near & (e <= chi2))
            if len(qs) == 0:
                continue
            d = hamming(rep[i:i + 1], np.asarray(kf_desc[k], np.uint8)[qs])[0]
            order = np.lexsort((qs, d))
            bd, bq = int(d[order[0]]), int(qs[order[0]])
            margins["max_dist"] = min(margins["max_dist"], abs(bd - (max_dist + 0.5)))
            if bd > max_dist:
                continue
            cnt["n_proposals"] += 1
            proposal[(i, k)] = bq
            if (k, bq) not in claim or (bd, i) < claim[(k, bq)]:
                claim[(k, bq)] = (bd, i)
    res["proposal"], res["claim"], res["drow"] = proposal, claim, drow
    if not (cnt["n_proposals"] or cnt["n_direct_edges"] or cnt["n_direct_gained"]):
        return done()
    res["fused"] = True
    gained = [[] for _ in range(n)]
    for (k, row), (_, i) in sorted(claim.items()):
        o = owner.get((k, row), given.get((k, row)))
        if o is not None:
            cnt["n_edges"] += 1
            unite(i, o)
        else:
            cnt["n_gained"] += 1
            gained[i].append((k, row))
    # rule 6
    comp = {}
    for i in range(n):
        comp.setdefault(find(i), []).append(i)
    stored = lists_of(a)
    new_list, survivor = {}, {}
    for root, mem in comp.items():
        sv = min(mem, key=lambda j: (not loop[j], -len(obs[j]), j))
        survivor[root] = sv
        lst = list(stored[sv])
        held = {k for k, _ in obs[sv]}
        extra = [e for j in mem if j != sv for e in obs[j]]
        for j in mem:
            extra += ([(p, drow[j])] if j in drow else []) + sorted(gained[j])
        for k, row in extra:
            if k not in held:
                held.add(k)
                lst.append((k, row))
        new_list[sv] = lst
    keep = sorted(new_list)
    rank = {sv: r for r, sv in enumerate(keep)}
    res["into"] = np.array([rank[survivor[find(i)]] for i in range(n)], np.int32)
    out = {f: arrays[f][keep] for f in ("xyz", "color", "id", "dref_kf", "dref_row")}
    noff = np.zeros(len(keep) + 1, np.int32)
    nkf, nkp = [], []
    for r, sv in enumerate(keep):
        nkf += [k for k, _ in new_list[sv]]; nkp += [row for _, row in new_list[sv]]
        noff[r + 1] = len(nkf)
    out.update(obs_off=noff, obs_kf=np.array(nkf, np.int32), obs_kp=np.array(nkp, np.int32))
    res["arrays"] = out
    res["survivor"] = {i: survivor[find(i)] for i in range(n)}
    cnt["n_absorbed"] = n - len(keep)
    cnt["n_points"], cnt["n_obs"] = len(keep), len(nkf)
    return done()
