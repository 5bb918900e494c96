"""numpy restatement of mo_map_absorb (include/vslam_amd.h, rules A1 - A6) on snapshot dicts - the dicts LocalMapper.export_state
returns: `dims` (an int64 vector in DIM_NAMES order) and the snapshot arrays - and of the one rule mo_map_loop_candidates_among adds to
tests/loop_restatement.select.  Plain numpy, int64 arithmetic cast back to the arrays' types."""
import numpy as np

from tests import bow_restatement as B
from tests import loop_restatement as LR

# vslam_amd.snapshot.DIM_NAMES (tests/test_absorb_cpu.py asserts they are the same)
DIM_NAMES = ("n_kf", "list_rows", "kf_rows", "n_pts", "n_obs", "list_ids", "kf_stored", "id_bound", "img_w0", "img_w1", "img_h0", "img_h1",
             "img_ch0", "img_ch1", "img_cur", "st_live0", "st_live1", "st_live2", "img_bytes0", "img_bytes1")
INT32_MIN = -2 ** 31


def dims_of(a):
    return dict(zip(DIM_NAMES, (int(x) for x in a["dims"])))


def entry_keys(obs_kf, obs_kp, kf_cnt, kf_offset):
    """A3 on src's entries: (obs_kf, obs_kp) as they are written into dst.  An entry names a row as every reader reads it: negative
    values count from the end.  One that does is written normalised behind dst's positions; one that names nothing becomes
    (INT32_MIN, its row value unchanged)."""
    k, r = np.asarray(obs_kf, np.int64), np.asarray(obs_kp, np.int64)
    cnt = np.asarray(kf_cnt, np.int64)
    n_kf = len(cnt)
    k = np.where(k < 0, k + n_kf, k)
    ok = (k >= 0) & (k < n_kf)
    nk = cnt[np.clip(k, 0, max(n_kf - 1, 0))] if n_kf else np.zeros(len(k), np.int64)
    rr = np.where(r < 0, r + nk, r)
    ok &= (rr >= 0) & (rr < nk)
    return np.where(ok, k + kf_offset, INT32_MIN).astype(np.int32), np.where(ok, rr, r).astype(np.int32)


def absorb(dst, src, dref_injected_shift=0):
    """the snapshot of dst after mo_map_absorb(dst, src): src appended as dst's tail"""
    d, s = dims_of(dst), dims_of(src)
    out = {k: np.array(v, copy=True) for k, v in dst.items()}
    if s["n_kf"] == 0 and s["n_pts"] == 0:   # nothing to append: a complete no-op, counters included
        return out
    cat = lambda k: np.concatenate([dst[k], src[k]])
    # A1: positions behind dst's, ordinals behind dst's history; counts, rows and projection matrices as they are
    for k in ("kf_cnt", "kf_kps", "kf_desc", "kf_P"):
        out[k] = cat(k)
    out["kf_ord"] = np.concatenate([dst["kf_ord"], (src["kf_ord"].astype(np.int64) + d["kf_stored"]).astype(np.int32)])
    # A2
    for k in ("xyz", "col", "dref_row"):
        out[k] = cat(k)
    out["id"] = np.concatenate([dst["id"], (src["id"].astype(np.int64) + d["id_bound"]).astype(np.int32)])
    ref = src["dref_kf"].astype(np.int64)
    out["dref_kf"] = np.concatenate([dst["dref_kf"], np.where(ref >= 0, ref + d["kf_stored"], ref - int(dref_injected_shift)).astype(np.int32)])
    life = src["life"].astype(np.int64).reshape(-1, 4).copy()
    life[:, 2] = np.minimum(life[:, 2] + d["kf_stored"], max(d["kf_stored"] + s["kf_stored"] - 1, 0))   # (held at the new now: binds for a src without history)
    life[:, 3] = 0
    out["life"] = np.concatenate([dst["life"].reshape(-1, 4), life.astype(np.int32)])
    # A3
    out["obs_off"] = np.concatenate([dst["obs_off"], (src["obs_off"][1:].astype(np.int64) + d["n_obs"]).astype(np.int32)])
    okf, okp = entry_keys(src["obs_kf"], src["obs_kp"], src["kf_cnt"], d["n_kf"])
    out["obs_kf"], out["obs_kp"] = np.concatenate([dst["obs_kf"], okf]), np.concatenate([dst["obs_kp"], okp])
    # A4: the sums; the third live word (new points of the last growth step) stays dst's.  A6: the lists stay dst's (copied above)
    o = dict(d)
    for k in ("n_kf", "kf_rows", "n_pts", "n_obs", "kf_stored", "id_bound", "st_live0", "st_live1"):
        o[k] = d[k] + s[k]
    # A5: the tail's images
    if s["n_kf"] > 0:
        for k in ("img_w0", "img_w1", "img_h0", "img_h1", "img_ch0", "img_ch1", "img_cur", "img_bytes0", "img_bytes1"):
            o[k] = s[k]
        out["img0"], out["img1"] = src["img0"].copy(), src["img1"].copy()
    out["dims"] = np.array([o[k] for k in DIM_NAMES], np.int64)
    return out


def select_among(W, kc, weights, p, among, min_weight=15, n_best=10, max_cand=4):
    """tests/loop_restatement.select with mo_map_loop_candidates_among's rule: common_k = 0 where among[k] == 0, and from there on the
    same S, M, groups, retain test and candidates.  among None: select itself."""
    if among is None or len(W) == 0:
        return LR.select(W, kc, weights, p, min_weight, n_best, max_cand)
    n = len(W)
    score = [B.score(kc[p], kc[k], weights) for k in range(n)]
    conn = LR.connected(W, p, min_weight)
    min_score = min([score[q] for q in conn], default=1.0)
    common = [0 if k == p or k in set(conn) or not among[k] else LR.common_words(kc[p], kc[k], weights) for k in range(n)]
    max_common = max(common)
    S = [k for k in range(n) if common[k] > (4 * max_common) // 5]
    M = [k for k in S if score[k] >= min_score]
    in_s = set(S)
    acc, best = {}, {}
    for k in M:
        a, bs, b = score[k], score[k], k
        for q in LR.neighbours(W, k, min_weight, n_best):
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
    return {"cand": cand, "acc": [cacc[k] for k in cand], "score": [score[k] for k in cand], "n_found": len(order),
            "connected": sorted(conn + [p]), "n_connected": len(conn), "min_score": min_score, "max_common": max_common,
            "n_scored": len(S), "n_passed": len(M), "group": [sorted(LR.connected(W, k, min_weight) + [k]) for k in cand], "S": S, "M": M,
            "retained": retained, "scores": score, "common": common, "acc_of": acc, "best_of": best}


def loop_candidates_among(kf_desc, obs_off, obs_kf, obs_kp, words, weights, among, p=-1, min_weight=15, n_best=10, max_cand=4, ratio=0.75,
                          prepared=None):
    """tests/loop_restatement.loop_candidates with the masked selection; prepared: LR.prepared's (kf_counts, W, tab)"""
    n = len(kf_desc)
    p = n - 1 if p < 0 else int(p)
    kc, W, tab = prepared if prepared is not None else LR.prepared(kf_desc, obs_off, obs_kf, obs_kp, words)
    res = select_among(W, kc, weights, p, among, min_weight, n_best, max_cand)
    res["cur_point"] = np.asarray(tab[p], np.int64)
    res["match_point"], res["match_row"], res["n_match"] = [], [], []
    for c in res["cand"]:
        mpt, mrow, nm = LR.match(kf_desc[p], kf_desc[c], tab[p], tab[c], ratio)
        res["match_point"].append(mpt); res["match_row"].append(mrow); res["n_match"].append(nm)
    return res
