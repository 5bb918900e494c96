"""numpy restatement of the point views and of the frustum mode of the searches (mo_map_point_views, mo_map_track_frustum and
mo_map_fuse_frustum in include/vslam_amd.h), in the header's operation order: the camera centres from the store's P, the viewing
direction and scale-invariance range of every point, the frustum test with the predicted level, one attempt of a tracking pass under it,
and fusion under it.  Exact integers given the map; every floating-point gate also reports its margin - the relative distance of the
tested quantity from its threshold - so that a test can require inputs on which a last-bit difference cannot flip a decision."""
import numpy as np

from tests.fuse_restatement import COUNTS, FIELDS, lists_of
from tests.reloc_restatement import hamming
from tests.track_restatement import _info, _power, local_points, project, refine, representatives, valid_observations

GATES = ("z", "border", "range_lo", "range_hi", "min_cos", "level", "box", "chi2", "max_dist")


def new_margins():
    return {g: np.inf for g in GATES}


def _note(margins, gate, value, threshold, scale=None):
    """relative distance of value from threshold (relative to `scale`, by default the threshold)"""
    if margins is None:
        return
    s = abs(threshold) if scale is None else abs(scale)
    m = abs(value - threshold) / s if s > 0 else abs(value - threshold)
    if m < margins[gate]:
        margins[gate] = m


def min_margin(margins):
    return min(margins[g] for g in GATES)


def centres(kf_P):
    """[n_kf][3] camera centres C = -M^-1 p by cofactors (NaN: none), from P = [M | p] per keyframe position"""
    out = np.full((len(kf_P), 3), np.nan)
    for k, P in enumerate(kf_P):
        P = np.asarray(P, np.float64).reshape(3, 4)
        (m00, m01, m02, p0), (m10, m11, m12, p1), (m20, m21, m22, p2) = P.tolist()
        a00 = m11 * m22 - m12 * m21; a01 = m02 * m21 - m01 * m22; a02 = m01 * m12 - m02 * m11
        a10 = m12 * m20 - m10 * m22; a11 = m00 * m22 - m02 * m20; a12 = m02 * m10 - m00 * m12
        a20 = m10 * m21 - m11 * m20; a21 = m01 * m20 - m00 * m21; a22 = m00 * m11 - m01 * m10
        det = m00 * a00 + m01 * a10 + m02 * a20
        if det == 0.0:
            continue
        with np.errstate(all="ignore"):
            c = np.array([-(np.float64(a00 * p0 + a01 * p1 + a02 * p2) / det), -(np.float64(a10 * p0 + a11 * p1 + a12 * p2) / det),
                          -(np.float64(a20 * p0 + a21 * p1 + a22 * p2) / det)])
        if np.isfinite(c).all():
            out[k] = c
    return out


def point_views(xyz, obs, kf_oct, C, scale_factor=1.2, n_levels=8, only=None):
    """the views of the points (those of the mask `only`, when given; the others report "none"): dict of normal [n][3] f32, max_dist and
    min_dist [n] f32, ref_pos, ref_octave, n_valid [n] int32.  obs: valid_observations' lists; C: centres()"""
    n = len(obs)
    X = np.asarray(xyz, np.float32).astype(np.float64).reshape(n, 3)
    res = {"normal": np.zeros((n, 3), np.float32), "min_dist": np.zeros(n, np.float32), "max_dist": np.zeros(n, np.float32),
           "ref_pos": np.full(n, -1, np.int32), "ref_octave": np.zeros(n, np.int32), "n_valid": np.zeros(n, np.int32)}
    top = _power(scale_factor, n_levels - 1)
    for i, v in enumerate(obs):
        if only is not None and not only[i]:
            continue
        s = [0.0, 0.0, 0.0]
        cnt, rp, ro, d_ref = 0, -1, 0, 0.0
        for k, row in v:
            c = C[k]
            if np.isnan(c[0]):
                continue
            dx, dy, dz = X[i, 0] - c[0], X[i, 1] - c[1], X[i, 2] - c[2]
            d = float(np.sqrt(dx * dx + dy * dy + dz * dz))
            if rp < 0:
                rp, ro, d_ref = k, int(kf_oct[k][row]), d
            if not d > 0.0:
                continue
            s[0] += dx / d; s[1] += dy / d; s[2] += dz / d
            cnt += 1
        if cnt:
            res["normal"][i] = [np.float32(s[0] / cnt), np.float32(s[1] / cnt), np.float32(s[2] / cnt)]
        with np.errstate(over="ignore"):
            res["max_dist"][i] = np.float32(d_ref * _power(scale_factor, ro))
            res["min_dist"][i] = np.float32(float(res["max_dist"][i]) / top)
        res["ref_pos"][i], res["ref_octave"][i], res["n_valid"][i] = rp, ro, cnt
    return res


def frustum(X, normal, max_dist, C, scale_factor=1.2, n_levels=8, range_lo=0.8, range_hi=1.2, min_cos=0.5, margins=None):
    """(the point is searched, its predicted level L) for the f64 position X [3], the f32 record (normal [3], max_dist) and the camera
    centre C [3]; `margins` (new_margins()) takes the margins of the gates decided"""
    px, py, pz = float(X[0]) - float(C[0]), float(X[1]) - float(C[1]), float(X[2]) - float(C[2])
    dist = float(np.sqrt(px * px + py * py + pz * pz))
    mx = float(np.float32(max_dist))
    if not dist > 0.0 or not mx > 0.0:
        return False, 0
    mn = mx / _power(scale_factor, n_levels - 1)
    _note(margins, "range_lo", dist, range_lo * mn)
    if dist < range_lo * mn:
        return False, 0
    _note(margins, "range_hi", dist, range_hi * mx)
    if dist > range_hi * mx:
        return False, 0
    dot = px * float(normal[0]) + py * float(normal[1]) + pz * float(normal[2])
    _note(margins, "min_cos", dot, min_cos * dist, dist)
    if dot < min_cos * dist:
        return False, 0
    s, L = 1.0, 0
    while L < n_levels - 1:
        _note(margins, "level", dist * s, mx)
        if not dist * s < mx:
            break
        s *= scale_factor
        L += 1
    return True, L


def camera_centre(pose):
    """-R^T t of a 4x4 or 3x4 pose, C_j = -(R[0][j] t0 + R[1][j] t1 + R[2][j] t2)"""
    T = np.asarray(pose, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    return np.array([-(R[0, j] * t[0] + R[1, j] * t[1] + R[2, j] * t[2]) for j in range(3)])


def level_by_log(dist, max_dist, scale_factor=1.2, n_levels=8):
    """ORB-SLAM2's PredictScale: ceil(log(max / dist) / log(scale_factor)) clamped to [0, n_levels - 1]"""
    return int(min(max(np.ceil(np.log(max_dist / dist) / np.log(scale_factor)), 0), n_levels - 1))


def search_frustum(K, pose, xyz, rep, ref, views, kps, desc, w, h, radius, scale_factor=1.2, max_dist=100, ratio=0.8, n_levels=8,
                   view_range=(0.8, 1.2), min_cos=0.5, margins=None):
    """one attempt of a pass of mo_map_track_frustum: (point [nq], dist [nq], level [nq], in_image, candidates).  ref: the local map's
    ref_octave list (None outside it); views: point_views() of at least the local points"""
    nq = len(kps)
    point = np.full(nq, -1, np.int64)
    dist = np.full(nq, -1, np.int64)
    level = np.full(nq, -1, np.int64)
    X = np.asarray(xyz, np.float32).astype(np.float64)
    u, v, z = project(K, pose, xyz)
    C = camera_centre(pose)
    kx, ky = kps["x"].astype(np.float64), kps["y"].astype(np.float64)
    ko = kps["octave"].astype(np.int64)
    claim = {}
    n_img = n_cand = 0
    for i in range(len(X)):
        if ref[i] is None:
            continue
        _note(margins, "z", z[i], 0.0)
        if not z[i] > 0:
            continue
        for val, thr in ((u[i], 0.0), (u[i], float(w)), (v[i], 0.0), (v[i], float(h))):
            _note(margins, "border", val, thr, w)
        if not (u[i] >= 0 and u[i] < w and v[i] >= 0 and v[i] < h):
            continue
        n_img += 1
        ok, L = frustum(X[i], views["normal"][i], views["max_dist"][i], C, scale_factor, n_levels, view_range[0], view_range[1], min_cos, margins)
        if not ok:
            continue
        n_cand += 1
        r = radius * _power(scale_factor, L)
        dx, dy = np.abs(kx - u[i]), np.abs(ky - v[i])
        gate = (ko >= L - 1) & (ko <= L)
        if margins is not None and gate.any() and r > 0:
            margins["box"] = min(margins["box"], float(np.abs(dx[gate] - r).min() / r), float(np.abs(dy[gate] - r).min() / r))
        q = np.flatnonzero(gate & (dx < r) & (dy < r))
        if len(q) == 0:
            continue
        d = hamming(rep[i:i + 1], desc[q])[0]
        order = np.lexsort((q, d))
        bd, bq = int(d[order[0]]), int(q[order[0]])
        _note(margins, "max_dist", bd, max_dist + 0.5)
        if bd > max_dist:
            continue
        if len(q) > 1 and not float(bd) <= ratio * float(d[order[1]]):
            continue
        if bq not in claim or (bd, i) < claim[bq][:2]:
            claim[bq] = (bd, i, L)
    for q, (d, i, L) in claim.items():
        point[q], dist[q], level[q] = i, d, L
    return point, dist, level, n_img, n_cand


def local_views(xyz, obs_off, obs_kf, obs_kp, kf_desc, kf_oct, kf_P, window=10, scale_factor=1.2, n_levels=8, local=None):
    """what a frustum call derives from the map before it searches: (obs, local mask, rep, ref, views of the local points, centres).
    local: the mask of a covisible local map in place of the window's"""
    counts = [len(d) for d in kf_desc]
    obs = valid_observations(obs_off, obs_kf, obs_kp, counts)
    if local is None:
        local = local_points(obs, len(counts), window)
    rep, ref = representatives(obs, kf_desc, kf_oct, local)
    C = centres(kf_P)
    return obs, local, rep, ref, point_views(xyz, obs, kf_oct, C, scale_factor, n_levels, only=local), C


def track_frustum(K, pose0, xyz, lv, kps, desc, w, h, radii=(15.0, 4.0), scale_factor=1.2, max_dist=100, ratio=0.8, chi2=5.991,
                  min_matches=20, n_levels=8, view_range=(0.8, 1.2), min_cos=0.5, poses=None, refine_pose=False, margins=None):
    """tests.track_restatement.track under the frustum: per pass the search with its retry.  lv: local_views(); poses: the pose each
    pass projects from (the device's own), in place of the restated refinement"""
    _, local, rep, ref, views, _ = lv
    pose = np.array(pose0, np.float64)
    res = {"n_local": int(np.sum(local)), "passes": []}
    kw = dict(scale_factor=scale_factor, max_dist=max_dist, ratio=ratio, n_levels=n_levels, view_range=view_range, min_cos=min_cos, margins=margins)
    for k, rad in enumerate(radii):
        if poses is not None:
            pose = np.array(poses[k], np.float64)
        used = rad
        point, dist, level, n_img, nc = search_frustum(K, pose, xyz, rep, ref, views, kps, desc, w, h, used, **kw)
        if (point >= 0).sum() < min_matches:
            used = 2.0 * rad
            point, dist, level, n_img, nc = search_frustum(K, pose, xyz, rep, ref, views, kps, desc, w, h, used, **kw)
        ps = {"point": point, "dist": dist, "level": level, "in_image": n_img, "cand": nc, "matches": int((point >= 0).sum()), "radius": used,
              "from": pose.copy()}
        res["passes"].append(ps)
        if ps["matches"] < min_matches:
            return res
        if refine_pose:
            q = np.flatnonzero(point >= 0)
            pose, inl, n_inl = refine(K, pose, np.asarray(xyz, np.float32)[point[q]].astype(np.float64),
                                      np.column_stack([kps["x"][q], kps["y"][q]]).astype(np.float64), kps["octave"][q], scale_factor, chi2)
            ps.update(pose=pose.copy(), inliers=n_inl)
    return res


def fuse_frustum(a, kf_P, kf_xy, kf_oct, kf_desc, w, h, window=10, radius=3.0, scale_factor=1.2, max_dist=50, chi2=5.991, n_levels=8,
                 view_range=(0.8, 1.2), min_cos=0.5):
    """tests.fuse_restatement.fuse under the frustum: (fused arrays, into, counts, margins).  The proposals are restated here; claims,
    owners, components, survivors and merged lists follow mo_map_fuse's rules unchanged."""
    off, okf, okp = a["obs_off"], a["obs_kf"], a["obs_kp"]
    n, n_kf = len(off) - 1, len(kf_desc)
    cnt = dict.fromkeys(COUNTS, 0)
    cnt["n_points"], cnt["n_obs"] = n, int(off[-1]) if n else 0
    margins = new_margins()
    same = {f: np.array(a[f]).copy() for f in FIELDS}
    into = np.arange(n, dtype=np.int32)
    if n == 0 or n_kf == 0:
        return same, into, cnt, margins
    obs, local, rep, ref, views, C = local_views(a["xyz"], off, okf, okp, kf_desc, kf_oct, kf_P, window, scale_factor, n_levels)
    lo = n_kf - window if 0 < window < n_kf else 0
    cnt["n_targets"], cnt["n_local"] = n_kf - lo, int(local.sum())
    owner = {}
    for i, v in enumerate(obs):
        for k, r in v:
            owner.setdefault((k, r), i)
    X = np.asarray(a["xyz"], np.float32).astype(np.float64)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    claim = {}
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
            _note(margins, "z", pz[i], 0.0)
            if not pz[i] > 0:
                continue
            u, v = pu[i] / pz[i], pv[i] / pz[i]
            for val, thr in ((u, 0.0), (u, float(w)), (v, 0.0), (v, float(h))):
                _note(margins, "border", val, thr, w)
            if not (u >= 0 and u < w and v >= 0 and v < h):
                continue
            if np.isnan(C[k][0]):
                continue
            ok, L = frustum(X[i], views["normal"][i], views["max_dist"][i], C[k], scale_factor, n_levels, view_range[0], view_range[1], min_cos,
                            margins)
            if not ok:
                continue
            cnt["n_cand"] += 1
            r = radius * _power(scale_factor, L)
            dx, dy = kx - u, ky - v
            gate = (ko >= L - 1) & (ko <= L)
            if gate.any() and r > 0:
                margins["box"] = min(margins["box"], float(np.abs(np.abs(dx[gate]) - r).min() / r), float(np.abs(np.abs(dy[gate]) - r).min() / r))
            near = gate & (np.abs(dx) < r) & (np.abs(dy) < r)
            e = info * (dx * dx + dy * dy)
            if near.any() and chi2 > 0:
                margins["chi2"] = min(margins["chi2"], float(np.abs(e[near] - chi2).min() / chi2))
            q = np.flatnonzero(near & (e <= chi2))
            if len(q) == 0:
                continue
            d = hamming(rep[i:i + 1], kf_desc[k][q])[0]
            order = np.lexsort((q, d))
            bd, bq = int(d[order[0]]), int(q[order[0]])
            _note(margins, "max_dist", bd, max_dist + 0.5)
            if bd > max_dist:
                continue
            cnt["n_proposals"] += 1
            if (k, bq) not in claim or (bd, i) < claim[(k, bq)]:
                claim[(k, bq)] = (bd, i)
    if not cnt["n_proposals"]:
        return same, into, cnt, margins
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
    stored = lists_of(a)
    new_list = {}
    survivor = {}
    for root, mem in comp.items():
        s = survivor[root] = min(mem, key=lambda j: (-len(obs[j]), j))
        lst = list(stored[s])
        held = {k for k, _ in obs[s]}
        for k, row in [e for j in mem if j != s for e in obs[j]] + [e for j in mem for e in sorted(gained[j])]:
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
    return out, into, cnt, margins
