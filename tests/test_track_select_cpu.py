"""The constructed cases of tests/track_cases.py, checked on the CPU before any of them is handed to the device:
(a) the descriptors realise the designed (train index, distance) per query - by a numpy brute-force matcher and by the oracle's,
(b) a plain restatement of the reference's two filters (matcher.py:109-169) equals oracle.geom_oracle.track_select,
(c) on every gate input math.hypot is the correctly rounded root of the exact sum of squares (rationals + integer sqrt),
(d) the kept counts written next to the cases hold.
Run with -s to see the number of cases and of gate inputs."""
import math

import numpy as np
import pytest

from tests import track_cases as T

CASES = T.all_cases()
IDS = [c.name for c in CASES]


def restate(c, idx, dist, keep):
    """Tracker's two filters as the reference writes them: filter_matches_by_geometric_distance (math.hypot on Python floats, <=),
    then filter_matches_by_distance (sorted by distance, np.median, strict <).  idx, dist, keep: the matcher's output.
    -> (queryIdx, trainIdx, distance) int arrays of the kept matches, in the reference's order"""
    matches = [(q, int(idx[q, 0]), float(dist[q, 0])) for q in range(len(keep)) if keep[q]]
    max_dist = ((c.w + c.h) / 2.0) * c.disp_frac
    filtered = []
    for m in matches:
        pt1 = (float(c.xy1[m[0], 0]), float(c.xy1[m[0], 1]))
        pt2 = (float(c.xy2[m[1], 0]), float(c.xy2[m[1], 1]))
        if math.hypot(pt2[0] - pt1[0], pt2[1] - pt1[1]) <= max_dist:
            filtered.append(m)
    out = []
    if filtered:
        filtered = sorted(filtered, key=lambda m: m[2])
        thr = np.median([m[2] for m in filtered]) * 2.0
        out = [m for m in filtered if m[2] < thr]
    a = np.array(out, np.float64).reshape(-1, 3)
    return a[:, 0].astype(np.int64), a[:, 1].astype(np.int64), a[:, 2].astype(np.int64)


_ORACLE = {}


def oracle_match(c, ratio):
    """the oracle matcher's (idx, dist, keep) for a case - computed once per (case, ratio)"""
    from oracle import orb_oracle as O
    if c.name not in _ORACLE:
        _ORACLE[c.name] = O.match_knn2(c.desc1, c.desc2)
    idx, dist = _ORACLE[c.name]
    return idx, dist, O.ratio_test(idx, dist, ratio if ratio is not None else 0.0, enabled=ratio is not None)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_design_is_realised(c):
    idx, dist = T.brute_knn2(c.desc1, c.desc2)
    assert np.array_equal(idx[:, 0], c.train) and np.array_equal(dist[:, 0], c.dist)
    oi, od, keep = oracle_match(c, None)
    assert np.array_equal(oi, idx) and np.array_equal(od, dist) and keep.all()
    keep = oracle_match(c, 0.75)[2]
    second = dist[:, 1].astype(np.float64)
    expect = (idx[:, 1] < 0) | (dist[:, 0].astype(np.float64) < 0.75 * second)
    assert np.array_equal(keep, expect)
    if len(c.desc2) == 1:   # matcher.py:79-81: a lone match is appended whatever the ratio
        assert keep.all() and (idx[:, 1] == -1).all()


@pytest.mark.parametrize("ratio", T.RATIOS, ids=["ratio_off", "ratio_0.75"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restatement_equals_oracle_and_stated_counts(c, ratio):
    from oracle import geom_oracle as G
    idx, dist, keep = oracle_match(c, ratio)
    q, t, d = restate(c, idx, dist, keep)
    gq, gt, gd = G.track_select(c.xy1, c.xy2, idx, dist, keep, c.w, c.h, c.disp_frac)
    assert np.array_equal(q, gq) and np.array_equal(t, gt) and np.array_equal(d, gd)
    assert np.all(np.diff(d) >= 0) and np.all(np.diff(q)[np.diff(d) == 0] > 0)   # ascending distance, ties in query order
    if ratio in c.kept:
        assert len(q) == c.kept[ratio]
    for s, k in zip(c.gate, c.gate_keep):   # the gate inputs have distances below the fillers' 9: the gate alone decides on them
        assert (s in q) == k


def _gate_inputs():
    return [(c, s) for c in CASES for s in c.gate]


def test_hypot_is_correctly_rounded_on_every_gate_input():
    n = 0
    for c, s in _gate_inputs():
        dx = float(c.xy2[c.train[s], 0]) - float(c.xy1[s, 0])
        dy = float(c.xy2[c.train[s], 1]) - float(c.xy1[s, 1])
        assert math.hypot(dx, dy) == T.exact_hypot(dx, dy), (c.name, s, dx, dy)
        assert (math.hypot(dx, dy) <= c.limit) == c.gate_keep[c.gate.index(s)]
        n += 1
    assert n >= 16
    print("\n%d constructed cases, %d gate inputs checked against exact arithmetic" % (len(CASES), n))


def test_disagreeing_inputs_disagree():
    """on the designed inputs the root of the rounded sum of squares differs from hypot by one ulp, and at the smaller of the two
    limits the two formulas decide differently - two pairs the reference keeps, two it drops, four mirror images each"""
    kinds = {"ref_keeps": 0, "ref_drops": 0}
    for c in CASES:
        if not c.name.startswith("gate_ref_"):
            continue
        for s, k in zip(c.gate, c.gate_keep):
            dx = float(c.xy2[c.train[s], 0]) - float(c.xy1[s, 0])
            dy = float(c.xy2[c.train[s], 1]) - float(c.xy1[s, 1])
            hyp, naive = math.hypot(dx, dy), float(np.sqrt(np.float64(dx) * dx + np.float64(dy) * dy))
            assert hyp < 20.0 and naive in (math.nextafter(hyp, 0.0), math.nextafter(hyp, math.inf))
            assert c.limit == (min(hyp, naive) if c.name.endswith("small") else max(hyp, naive))
            if c.name.endswith("small"):
                assert (naive <= c.limit) != k
                kinds[c.name[5:14]] += 1
            else:
                assert (naive <= c.limit) == k
    assert kinds == {"ref_keeps": 8, "ref_drops": 8}


def test_exact_hypot_itself():
    assert T.exact_hypot(3.0, 4.0) == 5.0 and T.exact_hypot(0.0, 0.0) == 0.0 and T.exact_hypot(-8.0, 6.0) == 10.0
    assert T.exact_hypot(1.0, 1.0) == math.sqrt(2.0) and T.exact_hypot(2.0 ** -30, 0.0) == 2.0 ** -30
    # the midpoint between 1 and the double above it is 1 + 2^-53, whose square is 1 + 2^-52 + 2^-106
    assert T.exact_hypot(1.0, 2.0 ** -26) == 1.0                                       # 1 + 2^-52: below it
    assert T.exact_hypot(1.0, 2.0 ** -26 * (1.0 + 2.0 ** -49)) == 1.0 + 2.0 ** -52     # 1 + 2^-52 + 2^-100 + ...: above it
