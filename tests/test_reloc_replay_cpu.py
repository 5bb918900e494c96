"""The host replay of relocalization's geometry (tests/native/reloc_replay.cpp) on the constructed cases of tests/reloc_cases.py, without
a device: every case meets its conditions, the hand-derived expectations hold, the replay's P3P roots are rotations that reproject
their own sample, its samples are the oracle's, the noise-free cases end at the constructed pose, and every deliberately wrong reading
of the rules (--variant) moves the results of the families aimed at it."""
import shutil

import numpy as np
import pytest

from tests import reloc_cases as RC

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")

# which families each wrong reading must move (best, counts, flags or winner); the full table is printed
MUST_MOVE = {
    "ties_high": ["all_inliers_tie"],
    "drop_last_block": ["n_hyp", "only_the_last_hypothesis"],
    "drop_tail_lanes": ["corr_counts"],
    "no_depth_test": ["behind_the_camera"],
    "one_round": ["second_round_reselects"],
    "winner_by_score": ["more_inliers_beat_a_higher_score", "equal_inliers_lower_position"],
    "root0": [],   # any family: asserted below
}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("reloc_replay")
    exe = RC.build_replay(d)
    cases = RC.all_cases()
    return exe, d, cases, {c.name: RC.run_replay(exe, c, d) for c in cases}


def _corr(case, c):
    """(X [m][3], xy [m][2], point [m]) of candidate c in C_k order, as f64"""
    f = case.front()
    qi, pi = f["C"][f["candidates"][c]]
    return case.xyz[pi].astype(np.float64), case.q_xy[qi].astype(np.float64), pi


def test_every_case_meets_its_conditions(run):
    _, _, cases, rps = run
    smallest = {}
    for c in cases:
        rp = rps[c.name]
        RC.check(c, rp)
        smallest[c.family] = min(smallest.get(c.family, np.inf), rp["margin_hyp"], rp["margin_sel"])
    print("smallest margin |e2 - thr2| / thr2 per family:")
    for fam, v in smallest.items():
        print("  %-36s %.3g" % (fam, v))
    assert {c.family for c in cases} >= {"corr_counts", "n_hyp", "only_the_last_hypothesis", "all_inliers_tie", "more_inliers_beat_a_higher_score",
                                         "equal_inliers_lower_position", "candidate_without_a_pose", "duplicate_point", "behind_the_camera",
                                         "thresholds", "skewed_camera", "query_rows", "many_keyframes"}


def test_hand_expectations(run):
    _, _, cases, rps = run
    for c in cases:
        rp, e, f = rps[c.name], c.expect, c.front()
        win = rp["winner"]
        n, h, root = RC.key_parts(rp["best"][win])
        if "best_h" in e:
            assert h == e["best_h"], (c.name, h)
        if "best_count" in e:
            assert n == e["best_count"], (c.name, n)
        if "ninl" in e:
            assert rp["ninl"][win] == e["ninl"], (c.name, rp["ninl"])
        if "cand_inliers" in e:
            assert rp["ninl"] == e["cand_inliers"], (c.name, rp["ninl"])
        if "winner" in e:
            assert f["candidates"][win] == e["winner"], (c.name, win)
        if "ok" in e:
            assert (rp["ninl"][win] >= c.prm["min_inliers"] and rp["best"][win] != 0) == e["ok"], c.name
        for ci in e.get("no_pose", []):
            assert rp["best"][ci] == 0 and rp["ninl"][ci] == 0 and np.isnan(rp["pose"][ci]).all() and not rp["flags"][ci].any()
            assert (rp["hyp"][ci]["roots"] == 0).all()   # collinear points: no sample has a pose
        if "never_inlier" in e:
            assert not rp["flags"][win][e["never_inlier"]].any() and rp["flags"][win].sum() == e["ninl"]
        if "inlier_idx" in e:   # only_the_last_hypothesis: one hypothesis draws three inliers, the last
            hits = [hh for hh, idx in enumerate(rp["hyp"][0]["idx"]) if set(idx.tolist()) <= set(e["inlier_idx"])]
            assert hits == [c.prm["n_hyp"] - 1] and c.prm["n_hyp"] % 4 == 1, hits
            assert np.flatnonzero(rp["flags"][0]).tolist() == e["inlier_idx"]
        if c.family == "all_inliers_tie":   # the lowest (h, root) whose pose counts all 20
            cnt = rp["hyp"][0]["count"]
            full = np.argwhere(cnt == 20)
            assert len(full) >= 2 and (h, root) == tuple(full[0]), (h, root, full[:3])
        if c.family == "duplicate_point":
            _, _, pts = _corr(c, 0)
            dup = [len(set(pts[idx].tolist())) < 3 for idx in rp["hyp"][0]["idx"]]
            assert sum(dup) >= 3 and (rp["hyp"][0]["roots"][dup] == 0).all(), sum(dup)
            assert len(set(pts.tolist())) == 20 and len(pts) == 24
        if c.family == "thresholds" and c.prm["thr_px"] == 1e6:   # everything in front of the camera is inside
            assert rp["flags"][0].all()
        if c.family == "many_keyframes":
            assert rp["n_cand"] == 64 and len(c.kfs) == 260 and max(f["candidates"]) > 256
            assert len({RC.key_parts(b)[1:] for b in rp["best"]}) > 8   # one stream per position: the candidates do not share a best sample
        if c.family == "second_round_reselects":
            assert rp["rounds"] == [2]


def test_roots_are_rotations_that_reproject_their_sample(run):
    """independent of the device and of pnp.h's own tests: from the dumped poses, in numpy"""
    _, _, cases, rps = run
    n_roots, worst_r, worst_px = 0, 0.0, 0.0
    for c in cases:
        rp = rps[c.name]
        for ci in range(rp["n_cand"]):
            X, xy, _ = _corr(c, ci)
            hy = rp["hyp"][ci]
            for r in range(4):
                sel = np.flatnonzero(hy["roots"] > r)
                if not len(sel):
                    continue
                R = hy["R"][sel, r].reshape(-1, 3, 3)
                t = hy["t"][sel, r]
                orth = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max()
                assert orth < 1e-12 and (np.linalg.det(R) > 0).all(), (c.name, orth)
                Xs, xs = X[hy["idx"][sel]], xy[hy["idx"][sel]]                      # [n][3][3], [n][3][2]
                cam = np.einsum("nij,nkj->nki", R, Xs) + t[:, None, :]
                p = np.einsum("ij,nkj->nki", c.K, cam)
                err = np.abs(p[:, :, :2] / p[:, :, 2:3] - xs).max()
                assert (cam[:, :, 2] > 0).all() and err < 1e-6, (c.name, err)
                n_roots += len(sel); worst_r = max(worst_r, orth); worst_px = max(worst_px, err)
    print("%d roots: worst |R R^T - I| %.3g, worst reprojection of the own sample %.3g px" % (n_roots, worst_r, worst_px))
    assert n_roots > 1000


def test_samples_are_the_oracles(run):
    from oracle.geom_oracle import sample8
    _, _, cases, rps = run
    n = 0
    for c in cases:
        rp, cands = rps[c.name], c.front()["candidates"]
        for ci, k in enumerate(cands):
            for h in range(0, c.prm["n_hyp"], 1 if c.prm["n_hyp"] <= 128 else 7):
                assert rp["hyp"][ci]["idx"][h].tolist() == sample8(c.prm["seed"], h, rp["m"][ci], k)[:3], (c.name, k, h)
                n += 1
    assert n > 3000


def test_noise_free_cases_end_at_the_constructed_pose(run):
    _, _, cases, rps = run
    n = 0
    for c in cases:
        if c.truth is None:
            continue
        rp = rps[c.name]
        pose = rp["pose"][rp["winner"]].reshape(3, 4)
        assert np.abs(pose - c.truth[:3]).max() < 1e-6, (c.name, pose - c.truth[:3])
        n += 1
    assert n >= 10


def _moved(a, b):
    out = []
    if a["best"] != b["best"]:
        out.append("best")
    if a["ninl"] != b["ninl"]:
        out.append("count")
    if any(not np.array_equal(x, y) for x, y in zip(a["flags"], b["flags"])):
        out.append("flags")
    if a["winner"] != b["winner"]:
        out.append("winner")
    return out


def test_cases_fail_under_a_wrong_reading(run):
    exe, d, cases, rps = run
    table, by_case = {}, {}
    for v in RC.VARIANTS:
        fams = {}
        for c in cases:
            m = _moved(rps[c.name], RC.run_replay(exe, c, d, variant=v))
            if m:
                fams.setdefault(c.family, set()).update(m)
                by_case.setdefault(v, set()).add(c.name)
        table[v] = fams
    print("what each wrong reading moves (family: what moved):")
    for v, fams in table.items():
        print("  %-16s %s" % (v, "; ".join("%s: %s" % (f, ", ".join(sorted(m))) for f, m in fams.items()) or "-"))
    for v, need in MUST_MOVE.items():
        assert table[v], v
        for fam in need:
            assert fam in table[v], (v, fam)
    # the sizes around a multiple of 64: a tail of one lane (65, 129) is seen, a full last trip (64, 128) has no tail to drop
    tails = {n for n in by_case["drop_tail_lanes"] if n.startswith("corr_counts:")}
    assert tails == {"corr_counts:15", "corr_counts:63", "corr_counts:65", "corr_counts:129"}, tails
    # n_hyp = 4 fills its block; 1, 3 and 5 lose their last (only) block, 511 its last three hypotheses - which do not hold its best
    assert {n for n in by_case["drop_last_block"] if n.startswith("n_hyp:")} == {"n_hyp:1", "n_hyp:3", "n_hyp:5"}
