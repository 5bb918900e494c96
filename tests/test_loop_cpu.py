"""Loop candidates without a GPU: the numpy restatement (tests/loop_restatement.py) against brute-force Python loops on the tiny maps,
the facts of the loop world that tests/test_gpu_loop.py relies on, LoopConsistency on hand sequences, and the ctypes mirrors of the two
new structs against the header as gcc lays it out."""
import os

import numpy as np
import pytest

from tests import loop_restatement as LR
from tests import loop_worlds as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A_KEYFRAMES = range(0, 6)


# ---- brute force: every rule once more, with plain loops and nothing shared with the restatement but the inputs ------------------------
def _popcount(a, b):
    return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))


def _brute(w, p, min_weight, n_best, max_cand, ratio=0.75):
    n = w.n_kf
    rows = [len(d) for d in w.kf_desc]
    valid = []   # per point the (position, row) pairs that name something
    for q in w.points:
        v = []
        for k, r in q["observed_keyframes"].items():
            k = k + n if k < 0 else k
            if 0 <= k < n:
                r = r + rows[k] if r < 0 else r
                if 0 <= r < rows[k]:
                    v.append((k, r))
        valid.append(v)
    Wm = [[0] * n for _ in range(n)]
    for v in valid:
        ks = sorted({k for k, _ in v})
        for a in ks:
            for b in ks:
                Wm[a][b] += 1
    cnt = []
    for d in w.kf_desc:
        c = [0] * len(w.words)
        for row in d:
            dist = [_popcount(row, wd) for wd in w.words]
            c[dist.index(min(dist))] += 1
        cnt.append(c)
    wt = [int(x) for x in w.weights]

    def score(a, b):
        qa, qb = [x * y for x, y in zip(cnt[a], wt)], [x * y for x, y in zip(cnt[b], wt)]
        na, nb = sum(qa), sum(qb)
        if na == 0 or nb == 0:
            return 0.0
        return 1.0 - 0.5 * float(sum(abs(x * nb - y * na) for x, y in zip(qa, qb))) / (float(na) * float(nb))
    floor = max(min_weight, 1)
    conn = [q for q in range(n) if q != p and Wm[p][q] >= floor]
    sc = [score(p, k) for k in range(n)]
    min_score = 1.0
    for q in conn:
        min_score = min(min_score, sc[q])
    common = [0] * n
    for k in range(n):
        if k != p and k not in conn:
            common[k] = sum(1 for x in range(len(wt)) if wt[x] > 0 and cnt[p][x] > 0 and cnt[k][x] > 0)
    S = [k for k in range(n) if common[k] > 4 * max(common) // 5]
    M = [k for k in S if sc[k] >= min_score]
    acc, best = {}, {}
    for k in M:
        left = [q for q in range(n) if q != k and Wm[k][q] >= floor]
        a, bs, b = sc[k], sc[k], k
        for _ in range(n_best):
            if not left:
                break
            q = left[0]
            for x in left:   # the largest weight, ties to the later position
                if Wm[k][x] > Wm[k][q] or (Wm[k][x] == Wm[k][q] and x > q):
                    q = x
            left.remove(q)
            if q in S:
                a = a + sc[q]
                if sc[q] > bs:
                    bs, b = sc[q], q
        acc[k], best[k] = a, b
    top = max(acc.values()) if acc else 0.0
    cands = {}
    for k in M:
        if acc[k] > 0.75 * top and acc[k] > cands.get(best[k], -1.0):
            cands[best[k]] = acc[k]
    order = sorted(cands, key=lambda k: (-cands[k], k))
    point_of = [[-1] * r for r in rows]
    for i in range(len(valid) - 1, -1, -1):
        for k, r in valid[i]:
            point_of[k][r] = i
    res = {"cand": order[:max_cand], "acc": [cands[k] for k in order[:max_cand]], "score": [sc[k] for k in order[:max_cand]],
           "n_found": len(order), "connected": sorted(conn + [p]), "min_score": min_score, "max_common": max(common), "n_scored": len(S),
           "n_passed": len(M), "group": [sorted([k] + [q for q in range(n) if q != k and Wm[k][q] >= floor]) for k in order[:max_cand]],
           "cur_point": point_of[p], "match_point": [], "match_row": [], "n_match": []}
    for c in res["cand"]:
        holder = {}   # train row -> (distance, query row, point)
        for i, qd in enumerate(w.kf_desc[p]):
            dist = [_popcount(qd, td) for td in w.kf_desc[c]]
            if not dist:
                continue
            order_t = sorted(range(len(dist)), key=lambda j: (dist[j], j))
            j = order_t[0]
            if len(dist) >= 2 and not float(dist[j]) < ratio * float(dist[order_t[1]]):
                continue
            a, b = point_of[p][i], point_of[c][j]
            if a < 0 or b < 0 or a == b:
                continue
            if j not in holder or (dist[j], i) < holder[j][:2]:
                holder[j] = (dist[j], i, b)
        mpt, mrow = [-1] * rows[p], [-1] * rows[p]
        for j, (_, i, b) in holder.items():
            mpt[i], mrow[i] = b, j
        res["match_point"].append(mpt); res["match_row"].append(mrow); res["n_match"].append(len(holder))
    return res


def _equal(r, b):
    for f in ("cand", "acc", "score", "n_found", "connected", "min_score", "max_common", "n_scored", "n_passed", "group", "n_match"):
        assert r[f] == b[f], f
    assert r["cur_point"].tolist() == b["cur_point"]
    assert [m.tolist() for m in r["match_point"]] == b["match_point"] and [m.tolist() for m in r["match_row"]] == b["match_row"]


def _restate(w, p, **kw):
    return LR.loop_candidates(w.kf_desc, w.obs_off, w.obs_kf, w.obs_kp, w.words, w.weights, p, **kw)


@pytest.mark.parametrize("n_kf", [70, 129])
def test_restatement_equals_brute_force_on_the_tiny_maps(n_kf):
    w = LW.tiny_world(n_kf)
    seen = {"tie": 0, "cut": 0, "dropped": 0, "cand": 0, "match": 0}
    for p in w.asking():
        for n_best, max_cand in ((10, 4), (2, 4), (0, 1)):
            r = _restate(w, p, min_weight=LW.TINY_MIN_WEIGHT, n_best=n_best, max_cand=max_cand)
            _equal(r, _brute(w, p, LW.TINY_MIN_WEIGHT, n_best, max_cand))
            seen["tie"] += len(r["acc_of"]) - len(set(r["acc_of"].values()))
            seen["cut"] += r["n_found"] > max_cand
            seen["dropped"] += len(r["retained"]) < len(r["M"])
            seen["cand"] += len(r["cand"])
            seen["match"] += sum(r["n_match"])
    assert all(seen.values()), seen   # accumulated scores tie, lists are cut, the 0.75 rule drops keyframes, rows match


def test_hand_cases():
    cases = LW.hand_cases()
    res = {}
    for name, (w, kw) in cases.items():
        res[name] = r = _restate(w, -1, **kw)
        _equal(r, _brute(w, w.n_kf - 1, kw.get("min_weight", 15), kw.get("n_best", 10), kw.get("max_cand", 4)))
    r = res["no_connected"]
    assert r["connected"] == [3] and r["min_score"] == 1.0 and r["cand"] == [0] and r["score"] == [1.0]   # only p's exact counts pass
    r = res["all_connected"]
    assert r["connected"] == [0, 1, 2] and r["max_common"] == 0 and r["cand"] == [] and r["n_scored"] == 0
    r = res["zero_weights"]
    assert r["max_common"] == 0 and r["cand"] == [] and all(s == 0.0 for s in r["scores"])
    r = res["groups"]
    assert r["min_score"] == 0.0 and r["M"] == [0, 1, 3] and r["best_of"] == {0: 0, 1: 0, 3: 0} and r["cand"] == [0] and r["group"] == [[0, 1, 3]]
    assert r["acc"] == [(1.0 + r["scores"][1]) + r["scores"][3]]                                            # N_0 = [1, 3] in rank order
    r = res["n_best_0"]
    assert r["cand"] == [0, 1] and r["acc"] == r["score"] and r["retained"] == [0, 1]
    r = res["max_cand_0"]
    assert r["cand"] == [] and r["n_found"] == 1 and r["n_passed"] == 3 and r["match_point"] == []
    r = res["max_cand_1"]
    assert r["cand"] == [0] and r["n_found"] == 2
    r = res["matching"]
    assert r["cand"] == [0] and r["n_match"] == [2]
    assert r["match_row"][0].tolist() == [0, -1, -1, -1, 1, -1, -1, -1, -1, -1]    # rows 0 and 4 keep their train rows
    assert r["match_point"][0].tolist() == [6, -1, -1, -1, 7, -1, -1, -1, -1, -1]
    assert r["cur_point"].tolist() == [0, 1, 2, 3, 5, 4, -1, 8, 10, 11]
    r = res["one_row"]
    assert r["cand"] == [0] and r["match_row"][0].tolist() == [0, -1]               # a train frame of one row passes its only neighbour
    assert res["empty_keyframe"]["cand"] == [0]


def test_matching_against_frames_of_no_rows_and_of_one_row():
    qd = LW.hand_words(7)[:3]
    none = LR.match(qd, np.zeros((0, 32), np.uint8), [0, 1, 2], [], 0.75)
    assert none[0].tolist() == [-1, -1, -1] and none[2] == 0
    one = LR.match(qd, LW.hand_words(7)[2:3], [0, 1, 2], [5], 0.75)
    assert one[1].tolist() == [-1, -1, 0] and one[0].tolist() == [-1, -1, 5] and one[2] == 1   # distance 0 beats 64 and 64
    same = LR.match(qd, LW.hand_words(7)[2:3], [0, 1, 5], [5], 0.75)
    assert same[1].tolist() == [0, -1, -1] and same[2] == 1                                    # row 2's match is a = b: row 0 keeps the row


def _loop_results():
    w = LW.loop_world()
    words, weights = LW.loop_vocabulary()
    kc, W, tab = LR.prepared(w.kf_desc, w.obs_off, w.obs_kf, w.obs_kp, words)
    return w, {p: LR.loop_candidates(w.kf_desc, w.obs_off, w.obs_kf, w.obs_kp, words, weights, p, kf_counts=kc, W=W, tab=tab)
               for p in (19,) + LW.RETURN_POS}


def test_loop_world_facts():
    """the restatement's own numbers on the loop world: what tests/test_gpu_loop.py asks the device to equal is a loop detection"""
    from vslam_amd.loop import LoopConsistency
    w, res = _loop_results()
    assert res[20]["connected"] == [20, 22, 24, 26]
    for p in LW.RETURN_POS:
        assert res[p]["cand"] and all(c in A_KEYFRAMES for c in res[p]["cand"]), (p, res[p]["cand"])
    assert res[19]["cand"] == [] and res[19]["S"] and res[19]["M"] == []            # S non-empty, M empty: a keyframe of B fails min_score
    assert any(set(r["M"]) < set(r["S"]) for r in res.values())
    assert any(len(r["retained"]) < len(r["M"]) for r in res.values())              # the 0.75 rule drops a passed keyframe
    lc = LoopConsistency(3)
    found = {}
    for p in LW.RETURN_POS:
        reported, _ = lc.update(list(zip(res[p]["cand"], res[p]["group"])))        # (no keyframe is removed: position = serial)
        found[p] = reported
    assert [p for p in LW.RETURN_POS if found[p]] == [26], found                    # exactly at the fourth return keyframe
    r = res[26]
    c = r["cand"].index(found[26][0])
    assert r["n_match"][c] >= 20
    rows = np.flatnonzero(r["match_point"][c] >= 0)
    assert len(rows) == r["n_match"][c]
    assert (w.ids[r["cur_point"][rows]] - LW.DUP_ID == w.ids[r["match_point"][c][rows]]).all()   # every correspondence a true duplicate pair


def test_loop_world_keyframe_by_keyframe():
    """the same world while it is built: the first return keyframe has no connected keyframe yet (no fallback: min_score 1.0, no
    candidate), so the chain of consistent groups starts at keyframe 22 and reaches 2 at keyframe 26"""
    from vslam_amd.loop import LoopConsistency
    w = LW.loop_world()
    words, weights = LW.loop_vocabulary()
    pts, n_kf, lc, found, cands = [], 0, LoopConsistency(2), {}, {}
    for add, inject, ask in w.steps():
        for k in add:
            n_kf, pts = k + 1, LW.cull(pts)
        pts = pts + inject
        r = LR.loop_candidates(w.kf_desc[:n_kf], *LW.obs_arrays(pts), words, weights, ask)
        found[ask], cands[ask] = lc.update(list(zip(r["cand"], r["group"])))[0], (r["cand"], r["n_match"])
    assert cands[19][0] == [] and cands[20][0] == []
    assert [p for p in found if found[p]] == [26], found
    assert cands[26][1][cands[26][0].index(found[26][0])] >= 20


def test_loop_consistency_hand_sequences():
    from vslam_amd.loop import LoopConsistency
    lc = LoopConsistency(3)
    assert lc.update([(5, {1, 3, 5})]) == ([], [0]) and lc.groups == [(frozenset({1, 3, 5}), 0)]
    assert lc.update([(3, {1, 3}), (9, {8, 9})]) == ([], [1, 0])
    assert lc.groups == [(frozenset({1, 3}), 1), (frozenset({8, 9}), 0)]
    # a candidate consistent with two previous groups: both counts + 1 join the state, its consistency is the larger
    assert lc.update([(3, {3, 8})]) == ([], [2]) and lc.groups == [(frozenset({3, 8}), 2), (frozenset({3, 8}), 1)]
    # two candidates consistent with the same group: the group joins once, both are reported
    lc.groups = [(frozenset({1, 2}), 2)]
    assert lc.update([(1, {1}), (2, {2, 7})]) == ([1, 2], [3, 3]) and lc.groups == [(frozenset({1}), 3)]
    # a candidate is reported once, however many groups make it consistent
    lc.groups = [(frozenset({1}), 2), (frozenset({1, 4}), 5)]
    assert lc.update([(1, {1})]) == ([1], [6])
    # an empty call clears the state
    assert lc.update([]) == ([], []) and lc.groups == []
    assert lc.update([(1, {1})]) == ([], [0])
    # a threshold of 1: the second sighting reports
    one = LoopConsistency(1)
    assert one.update([(4, {4, 5})]) == ([], [0]) and one.update([(5, {5})]) == ([5], [1])
    # serials of removed keyframes stay in old groups and do no harm: the new group shares serial 3 alone
    lc = LoopConsistency(2)
    lc.update([(3, {2, 3, 4})])
    assert lc.update([(3, {3, 6})]) == ([], [1]) and lc.update([(6, {6})]) == ([6], [2])


def test_loop_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of the two new structs as gcc sees include/vslam_amd.h == the ctypes mirrors"""
    import ctypes as C
    import subprocess
    import vslam_amd as V
    structs = [("mo_map_loop_params", V.MapLoopParams), ("mo_map_loop_out", V.MapLoopOut)]
    body = ""
    for cname, cls in structs:
        body += '  printf("%%zu\\n", sizeof(%s));\n' % cname
        body += "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0]) for f in cls._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vslam_amd.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    k = 0
    for cname, cls in structs:
        assert got[k] == C.sizeof(cls), cname
        offs = [getattr(cls, f[0]).offset for f in cls._fields_]
        assert got[k + 1:k + 1 + len(offs)] == offs, cname
        k += 1 + len(offs)
    assert "mo_map_loop_candidates" in V.SIGNATURES
