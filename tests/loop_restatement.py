"""numpy restatement of mo_map_loop_candidates (include/vslam_amd.h), rule for rule: connected keyframes on the covisibility matrix,
the scores of tests/bow_restatement.py with a keyframe's own counts as the query, min_score, common words, the sets S and M, the group
accumulation with its tie rules, the 0.75 retain test, the candidates, their groups and the map-point matching.  Integer work and Python
floats (IEEE f64) in the order the header states."""
import numpy as np

from tests import bow_restatement as B
from tests import covis_restatement as CR
from tests import reloc_restatement as RR

MAX_CAND = 16


def connected(W, k, min_weight):
    floor = max(int(min_weight), 1)
    return [q for q in range(len(W)) if q != k and W[k][q] >= floor]


def neighbours(W, k, min_weight, n_best):
    """N_k in rank order: the largest weight first, ties to the later position"""
    return sorted(connected(W, k, min_weight), key=lambda q: (W[k][q], q), reverse=True)[:max(int(n_best), 0)]


def common_words(cp, ck, weights):
    return int(((np.asarray(weights) > 0) & (np.asarray(cp) > 0) & (np.asarray(ck) > 0)).sum())


def select(W, kc, weights, p, min_weight=15, n_best=10, max_cand=4):
    """everything up to the candidates, from the covisibility matrix W and the term counts kc [n_kf][words]"""
    n = len(W)
    res = {"cand": [], "acc": [], "score": [], "n_found": 0, "connected": [], "n_connected": 0, "min_score": 1.0, "max_common": 0,
           "n_scored": 0, "n_passed": 0, "group": [], "S": [], "M": [], "retained": [], "scores": [], "common": [], "acc_of": {},
           "best_of": {}}
    if n == 0:
        return res
    score = [B.score(kc[p], kc[k], weights) for k in range(n)]
    conn = connected(W, p, min_weight)
    min_score = min([score[q] for q in conn], default=1.0)
    common = [0 if k == p or k in set(conn) else common_words(kc[p], kc[k], weights) for k in range(n)]
    max_common = max(common)
    S = [k for k in range(n) if common[k] > (4 * max_common) // 5]
    M = [k for k in S if score[k] >= min_score]
    in_s = set(S)
    acc, best = {}, {}
    for k in M:
        a, bs, b = score[k], score[k], k
        for q in neighbours(W, k, min_weight, n_best):
            if q not in in_s:
                continue
            a = a + score[q]
            if score[q] > bs:
                bs, b = score[q], q
        acc[k], best[k] = a, b
    top = max(acc.values(), default=0.0)
    retained = [k for k in M if acc[k] > 0.75 * top]
    cacc = {}
    for k in retained:
        cacc[best[k]] = max(cacc.get(best[k], 0.0), acc[k])
    order = sorted(cacc, key=lambda k: (-cacc[k], k))
    cand = order[:max_cand]
    res.update({"cand": cand, "acc": [cacc[k] for k in cand], "score": [score[k] for k in cand], "n_found": len(order),
                "connected": sorted(conn + [p]), "n_connected": len(conn), "min_score": min_score, "max_common": max_common,
                "n_scored": len(S), "n_passed": len(M), "group": [sorted(connected(W, k, min_weight) + [k]) for k in cand], "S": S, "M": M,
                "retained": retained, "scores": score, "common": common, "acc_of": acc, "best_of": best})
    return res


def match(qd, td, tab_p, tab_c, ratio):
    """(match_point, match_row, n_match) of one candidate: the matcher's knn-2 with the ratio test, the two point_of lookups, a != b,
    and per train row the query row with the lowest (distance, row)"""
    nq = len(qd)
    mpt, mrow = np.full(nq, -1, np.int64), np.full(nq, -1, np.int64)
    idx, dist, keep = RR.knn2_ratio(qd, td, ratio)
    claim = {}
    for i in range(nq):
        j = int(idx[i, 0])
        if not keep[i] or j < 0:
            continue
        a, b = int(tab_p[i]), int(tab_c[j])
        if a < 0 or b < 0 or a == b:
            continue
        key = (int(dist[i, 0]), i)
        if j not in claim or key < claim[j][0]:
            claim[j] = (key, b)
    for j, ((_, i), b) in claim.items():
        mpt[i], mrow[i] = b, j
    return mpt, mrow, len(claim)


def loop_candidates(kf_desc, obs_off, obs_kf, obs_kp, words, weights, p=-1, min_weight=15, n_best=10, max_cand=4, ratio=0.75, kf_counts=None,
                    W=None, tab=None):
    """the whole call.  kf_counts / W / tab: term counts, covisibility matrix and point_of table made before (they do not depend on p)"""
    n = len(kf_desc)
    counts = [len(d) for d in kf_desc]
    if n == 0:
        return select([], [], weights, 0)
    p = n - 1 if p < 0 else int(p)
    W = CR.covisibility(obs_off, obs_kf, obs_kp, counts) if W is None else W
    kc = [B.counts(d, words) for d in kf_desc] if kf_counts is None else kf_counts
    res = select(W, kc, weights, p, min_weight, n_best, max_cand)
    tab = RR.point_of(obs_off, obs_kf, obs_kp, counts) if tab is None else tab
    res["cur_point"] = np.asarray(tab[p], np.int64)
    res["match_point"], res["match_row"], res["n_match"] = [], [], []
    for c in res["cand"]:
        mpt, mrow, nm = match(kf_desc[p], kf_desc[c], tab[p], tab[c], ratio)
        res["match_point"].append(mpt); res["match_row"].append(mrow); res["n_match"].append(nm)
    return res


def prepared(kf_desc, obs_off, obs_kf, obs_kp, words):
    """(kf_counts, W, tab) for loop_candidates calls on the same map with several asking keyframes"""
    counts = [len(d) for d in kf_desc]
    return ([B.counts(d, words) for d in kf_desc], CR.covisibility(obs_off, obs_kf, obs_kp, counts),
            RR.point_of(obs_off, obs_kf, obs_kp, counts))
