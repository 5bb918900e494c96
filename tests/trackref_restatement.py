"""numpy restatement of LocalMapper.track_reference_keyframe (mo_map_track_reference in include/vslam_amd.h), rule by rule: the buckets
of the frame's rows by word, the search of every keyframe row that has a point inside the bucket of its word, the keyframe row of
each match, the orientation stage and the one refinement pass.  The per-row words are tests/bow_restatement.quantise's, the point_of
table is tests/reloc_restatement.point_of's and the refinement is tests/track_restatement.refine: nothing of those is restated here.
Everything in front of the refinement is integer work."""
import numpy as np

from tests import bow_restatement as B
from tests import track_restatement as TR

N_BINS = 30


def buckets(f_words, n_words):
    """(woff [W + 1], wrows [n]): the frame's rows grouped by word, ascending row order within a word"""
    f_words = np.asarray(f_words, np.int64)
    wrows = np.argsort(f_words, kind="stable")
    woff = np.zeros(n_words + 1, np.int64)
    woff[1:] = np.cumsum(np.bincount(f_words, minlength=n_words))
    return woff, wrows


def search(kf_desc, kf_words, tab, f_desc, woff, wrows, max_dist=50, ratio=0.7):
    """(key {frame row: (dist, point)}, cq [rows], cd [rows], n_cand, n_claims): candidate r (tab[r] >= 0) walks the bucket of its word
    with its own descriptor: the best distance (ties to the lower frame row), the second distance, the two gates, the claim"""
    kf_desc = np.asarray(kf_desc, np.uint8).reshape(-1, 32)
    n = len(kf_desc)
    cq = np.full(n, -1, np.int64)
    cd = np.full(n, -1, np.int64)
    key = {}
    cand = np.flatnonzero(np.asarray(tab) >= 0)
    d_all = B.hamming(kf_desc, f_desc) if len(f_desc) and n else np.zeros((n, 0), np.int32)
    for r in cand:
        w = int(kf_words[r])
        rows = wrows[woff[w]:woff[w + 1]]
        if len(rows) == 0:
            continue
        d = d_all[r, rows]
        j = int(np.argmin(d))               # the first minimum: rows ascend, so ties go to the lower frame row
        bd, bq = int(d[j]), int(rows[j])
        if bd > max_dist:
            continue
        if len(rows) > 1:
            sd = int(np.sort(d)[1])
            if not float(bd) <= ratio * float(sd):
                continue
        cq[r], cd[r] = bq, bd
        p = int(tab[r])
        if bq not in key or (bd, p) < key[bq]:
            key[bq] = (bd, p)
    return key, cq, cd, len(cand), int((cq >= 0).sum())


def keyframe_rows(key, cq, cd, tab, n_frame):
    """kf_row [n_frame]: the lowest candidate row whose claim stands on the frame row, -1 without a claim"""
    kf_row = np.full(n_frame, -1, np.int64)
    for r in range(len(cq) - 1, -1, -1):    # descending, so the lowest row is written last
        q = int(cq[r])
        if q >= 0 and key[q] == (int(cd[r]), int(tab[r])):
            kf_row[q] = r
    return kf_row


def rotation_bin(kf_angle, f_angle):
    """the bin of one match from the two f32 angles; -1 outside 0 .. 29"""
    rot = float(np.float64(np.float32(kf_angle)) - np.float64(np.float32(f_angle)))
    if rot < 0:
        rot += 360.0
    b = np.rint(np.float64(rot) / np.float64(12.0))
    if not (b >= 0.0 and b < 2.0 * N_BINS):
        return -1
    b = int(b)
    return b - N_BINS if b >= N_BINS else b


def three_maxima(hist):
    """kept_bin [3] (-1: none): the three highest bins, ties to the lower bin; the second iff 10 * c2 >= c1, the third iff the second is
    kept and 10 * c3 >= c1; a bin of count 0 is never kept"""
    order = sorted(range(len(hist)), key=lambda i: (-int(hist[i]), i))[:3]
    c = [int(hist[i]) for i in order]
    kept = [-1, -1, -1]
    if c[0] > 0:
        kept[0] = order[0]
        if c[1] > 0 and 10 * c[1] >= c[0]:
            kept[1] = order[1]
            if c[2] > 0 and 10 * c[2] >= c[0]:
                kept[2] = order[2]
    return kept


def orientation(key, kf_row, kf_angle, f_angle):
    """(hist [30], kept_bin [3], the claims that stay)"""
    hist = np.zeros(N_BINS, np.int64)
    bins = {q: rotation_bin(kf_angle[kf_row[q]], f_angle[q]) for q in key}
    for b in bins.values():
        if b >= 0:
            hist[b] += 1
    kept = three_maxima(hist)
    return hist, kept, {q: v for q, v in key.items() if bins[q] >= 0 and bins[q] in kept}


def track_reference(K, pose0, xyz, tab, kf_kps, kf_desc, kf_words, f_kps, f_desc, f_words, n_words, max_dist=50, ratio=0.7, check_orientation=True,
                    scale_factor=1.2, chi2=5.991, min_matches=15, min_inliers=10):
    """the whole call on one keyframe: tab = point_of of the reference keyframe (-1: no point), kf_kps / f_kps KP_DTYPE-like records
    (angle, x, y, octave), the words of both sides under one vocabulary of n_words words"""
    n = len(f_desc)
    woff, wrows = buckets(f_words, n_words)
    key, cq, cd, n_cand, n_claims = search(kf_desc, kf_words, tab, f_desc, woff, wrows, max_dist, ratio)
    kf_row = keyframe_rows(key, cq, cd, tab, n)
    res = {"woff": woff, "wrows": wrows, "cq": cq, "cd": cd, "n_cand": n_cand, "n_claims": n_claims, "n_matches_raw": len(key),
           "hist": np.zeros(N_BINS, np.int64), "kept_bin": [-1, -1, -1]}
    if check_orientation:
        res["hist"], res["kept_bin"], key = orientation(key, kf_row, kf_kps["angle"], f_kps["angle"])
    point = np.full(n, -1, np.int64)
    dist = np.full(n, -1, np.int64)
    for q, (d, p) in key.items():
        point[q], dist[q] = p, d
    kf_row[point < 0] = -1
    q = np.flatnonzero(point >= 0)
    res.update(point=point, dist=dist, kf_row=kf_row, n_matches=len(q), inlier=np.zeros(n, bool), n_inliers=0, ok=False,
               pose=np.array(pose0, np.float64), refined=False)
    if len(q) < min_matches:
        return res
    xyz = np.asarray(xyz, np.float32)
    pose, inl, n_inl = TR.refine(K, pose0, xyz[point[q]].astype(np.float64), np.column_stack([f_kps["x"][q], f_kps["y"][q]]).astype(np.float64),
                                 f_kps["octave"][q], scale_factor, chi2)
    res["inlier"][q] = inl
    res.update(pose=pose, n_inliers=n_inl, ok=n_inl >= min_inliers, refined=True)
    return res
