"""numpy restatement of LocalMapper.relocalize's integer steps (mo_map_relocalize in include/vslam_amd.h): knn-2 matching of the frame
against every keyframe with the Lowe ratio, the keypoint -> map point table, the correspondence sets C_k and the candidate ranking."""
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
MIN_SCORE = 15


def hamming(qd, td):
    """[nq][nt] Hamming distances of 32-byte descriptors"""
    qd, td = np.asarray(qd, np.uint8), np.asarray(td, np.uint8)
    out = np.zeros((len(qd), len(td)), np.int32)
    for b in range(0, len(qd), 256):
        out[b:b + 256] = _POP[qd[b:b + 256, None, :] ^ td[None, :, :]].sum(2)
    return out


def knn2_ratio(qd, td, ratio):
    """(idx [nq][2], dist [nq][2], keep [nq]) like the matcher: smallest (distance, train index) first; a missing neighbour is -1;
    one neighbour only -> kept; two -> d0 < ratio * d1"""
    nq, nt = len(qd), len(td)
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), np.iinfo(np.int32).max, np.int32)
    keep = np.zeros(nq, bool)
    if nq == 0 or nt == 0:
        return idx, dist, keep
    d = hamming(qd, td)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]   # stable: ties to the lower train index
    r = np.arange(nq)
    idx[:, 0] = order[:, 0]; dist[:, 0] = d[r, order[:, 0]]
    if nt >= 2:
        idx[:, 1] = order[:, 1]; dist[:, 1] = d[r, order[:, 1]]
        keep = dist[:, 0].astype(np.float64) < ratio * dist[:, 1].astype(np.float64)
    else:
        keep[:] = True
    return idx, dist, keep


def point_of(obs_off, obs_kf, obs_kp, counts):
    """per keyframe position k: [counts[k]] lowest map point observing (k, row), -1 for none; observations read like the cull reads
    them (negative values count from the end), entries naming nothing skipped"""
    n_kf = len(counts)
    tab = [np.full(int(c), -1, np.int64) for c in counts]
    n = len(obs_off) - 1
    for i in range(n - 1, -1, -1):   # descending, so the lowest index is written last
        for o in range(int(obs_off[i]), int(obs_off[i + 1])):
            k = int(obs_kf[o])
            if k < 0:
                k += n_kf
            if not 0 <= k < n_kf:
                continue
            kp = int(obs_kp[o])
            if kp < 0:
                kp += int(counts[k])
            if not 0 <= kp < counts[k]:
                continue
            tab[k][kp] = i
    return tab


def correspondences(idx, keep, tab_k):
    """C_k: (query indices, map points) of the ratio-test survivors whose best neighbour has a map point, in query order"""
    q = np.flatnonzero(keep & (idx[:, 0] >= 0))
    p = tab_k[idx[q, 0]] if len(tab_k) else np.zeros(0, np.int64)
    sel = p >= 0
    return q[sel], p[sel]


def rank(scores, max_candidates):
    """positions with score >= 15, highest first, ties to the lower position"""
    pos = [k for k in range(len(scores)) if scores[k] >= MIN_SCORE]
    pos.sort(key=lambda k: (-scores[k], k))
    return pos[:max_candidates]


def restate(query_desc, kf_desc, obs_off, obs_kf, obs_kp, ratio=0.75, max_candidates=4):
    """everything relocalize decides before the geometry: per-keyframe C_k, scores, the candidate list"""
    counts = [len(d) for d in kf_desc]
    tab = point_of(obs_off, obs_kf, obs_kp, counts)
    C = []
    for k, td in enumerate(kf_desc):
        idx, _, keep = knn2_ratio(query_desc, td, ratio)
        C.append(correspondences(idx, keep, tab[k]))
    scores = [len(c[0]) for c in C]
    return {"C": C, "scores": scores, "candidates": rank(scores, max_candidates), "point_of": tab}
