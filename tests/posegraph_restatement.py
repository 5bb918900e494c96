"""numpy restatement of rule 1 of mo_map_pose_graph (include/vslam_amd.h): the covisibility weights of a map's observation lists, the
parent of every keyframe position, and the edge set with its kinds in the order the library returns it.  Plain integers: the device
must return exactly these.  Also the f64 similarity helpers the pose-graph tests share (composition, inverse, the retraction, the
residual of an edge, the point rule)."""
import numpy as np

from tests.track_restatement import valid_observations

EXTRA, TREE, COVIS = 0, 1, 2


def covisibility(arrays, counts):
    """W [n_kf][n_kf] of mo_map_covisibility: the points with a valid observation at both positions (a point counts once per pair)"""
    n = len(counts)
    W = np.zeros((n, n), np.int32)
    for v in valid_observations(arrays["obs_off"], arrays["obs_kf"], arrays["obs_kp"], counts):
        pos = sorted({k for k, _ in v})
        for a in pos:
            for b in pos:
                W[a, b] += 1
    return W


def parents(W):
    """parent[b], b >= 1: the position a < b of the largest weight, ties to the lowest; b - 1 when that weight is 0.  parent[0] = -1."""
    n = len(W)
    par = np.full(n, -1, np.int32)
    for b in range(1, n):
        col = np.asarray(W[:b, b])
        par[b] = int(np.argmax(col)) if col.max() > 0 else b - 1   # (argmax: the first of equal values)
    return par


def edges(W, extra, fixed, min_weight):
    """(a [n], b [n], kind [n]) ordered by (a, b): the union of the extra pairs, {parent[b], b} and the pairs of weight >= min_weight
    (below 1: 1), each once with the first kind that applies, less the pairs of two fixed positions"""
    n = len(W)
    par = parents(W)
    ex = {(min(int(a), int(b)), max(int(a), int(b))) for a, b in extra}
    mw = max(int(min_weight), 1)
    out = []
    for a in range(n):
        for b in range(a + 1, n):
            if fixed[a] and fixed[b]:
                continue
            if (a, b) in ex:
                out.append((a, b, EXTRA))
            elif par[b] == a:
                out.append((a, b, TREE))
            elif W[a, b] >= mw:
                out.append((a, b, COVIS))
    e = np.array(out, np.int32).reshape(-1, 3)
    return e[:, 0].copy(), e[:, 1].copy(), e[:, 2].astype(np.uint8)


# ---- similarities as rows of 13: s, R (row-major), t ----------------------------------------------------------------------------------------
def sim(s, R, t):
    return np.concatenate([[float(s)], np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def parts(S):
    S = np.asarray(S, np.float64)
    return float(S[0]), S[1:10].reshape(3, 3), S[10:13]


def compose(A, B):
    sa, Ra, ta = parts(A)
    sb, Rb, tb = parts(B)
    return sim(sa * sb, Ra @ Rb, sa * (Ra @ tb) + ta)


def inverse(S):
    s, R, t = parts(S)
    return sim(1.0 / s, R.T, -(R.T @ t) / s)


def apply(S, X):
    s, R, t = parts(S)
    return s * (R @ np.asarray(X, np.float64)) + t


def exp_so3(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-8:
        return np.eye(3) + Wx + 0.5 * Wx @ Wx
    return np.eye(3) + np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * Wx @ Wx


def log_so3(R):
    """for the moderate angles of the tests (well below pi)"""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn, c = np.linalg.norm(v), 0.5 * (np.trace(R) - 1.0)
    if sn < 1e-6:
        return v * (1.0 + sn * sn / 6.0)
    return v * (np.arctan2(sn, c) / sn)


def retract(d, S):
    """D(d) o S, d = (rho, w, lambda)"""
    s, R, t = parts(S)
    E, el = exp_so3(d[3:6]), np.exp(d[6])
    return sim(el * s, E @ R, el * (E @ t) + np.asarray(d[:3], np.float64))


def residual(M, Sa, Sb):
    s, R, t = parts(compose(M, compose(Sa, inverse(Sb))))
    return np.concatenate([t, log_so3(R), [np.log(s)]])


def pose_of(S):
    """[R | t / s], 3 x 4"""
    s, R, t = parts(S)
    return np.hstack([R, (t / s).reshape(3, 1)])


def moved_points(arrays, counts, fixed, init, final):
    """rule 4 for the points in f64: (X' [n][3] f64, moved [n]): a point whose reference - the position of its first valid observation - is
    free becomes S_r,final^-1 (S_r,init X); every other point stays"""
    xyz = np.asarray(arrays["xyz"], np.float32)
    out = xyz.astype(np.float64)
    moved = np.zeros(len(xyz), bool)
    for i, v in enumerate(valid_observations(arrays["obs_off"], arrays["obs_kf"], arrays["obs_kp"], counts)):
        if not v or fixed[v[0][0]]:
            continue
        r = v[0][0]
        out[i] = apply(inverse(final[r]), apply(init[r], xyz[i].astype(np.float64)))
        moved[i] = True
    return out, moved
