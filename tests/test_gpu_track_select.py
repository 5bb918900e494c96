"""k_track_select driven by the constructed match lists of tests/track_cases.py through Context.pair_frontend(MODE_TRACK, n_hyp=0):
the matcher's output equals the oracle matcher's, and the kept list - query index, train index, distance, count - equals the plain
restatement of the reference's two filters (tests/test_track_select_cpu.py) bit for bit, with the ratio test off and at 0.75."""
import numpy as np
import pytest

from tests import track_cases as T
from tests.test_track_select_cpu import oracle_match, restate

pytestmark = pytest.mark.gpu
CASES = T.all_cases()
SHARED = [c for c in CASES if not c.fresh]
K = np.array([[320.0, 0, 320.0], [0, 320.0, 240.0], [0, 0, 1.0]])


def _kps(V, xy):
    k = np.zeros(len(xy), V.KP_DTYPE)
    k["x"], k["y"], k["size"], k["angle"], k["class_id"] = xy[:, 0], xy[:, 1], 31.0, -1.0, -1
    return k


def _run(V, ctx, c, ratio, n_hyp=0):
    return ctx.pair_frontend(_kps(V, c.xy1), c.desc1, _kps(V, c.xy2), c.desc2, V.MODE_TRACK, K, c.w, c.h, ratio=ratio,
                             disp_frac=c.disp_frac, n_hyp=n_hyp, seed=4096, want_matches=True)


def _check(c, ratio, g):
    idx, dist, keep = oracle_match(c, ratio)
    assert np.array_equal(g["idx"], idx) and np.array_equal(g["dist"], dist) and np.array_equal(g["keep"], keep)
    q, t, d = restate(c, idx, dist, keep)
    sel = g["sel"]
    if c.gate:   # name the designed matches a wrong gate decision moves
        want, got = set(q.tolist()), set(sel[:, 0].tolist())
        assert got == want, "case %s: kept but dropped by the reference: queries %s; dropped but kept by the reference: queries %s; " \
                            "designed gate inputs: %s" % (c.name, sorted(got - want), sorted(want - got), list(c.gate))
    assert len(sel) == len(q)
    assert np.array_equal(sel[:, 0], q) and np.array_equal(sel[:, 1], t) and np.array_equal(g["sel_dist"], d)
    if ratio in c.kept:
        assert len(sel) == c.kept[ratio]


@pytest.fixture(scope="module")
def shared_ctx():
    import vslam_amd as V
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=2)
    yield V, ctx
    ctx.close()


@pytest.mark.parametrize("ratio", T.RATIOS, ids=["ratio_off", "ratio_0.75"])
@pytest.mark.parametrize("c", SHARED, ids=[c.name for c in SHARED])
def test_constructed_case(shared_ctx, c, ratio):
    """(the cases come in ascending size: the context's row capacity grows with them)"""
    V, ctx = shared_ctx
    g = _run(V, ctx, c, ratio)
    _check(c, ratio, g)
    if c.tie_heavy:   # the placement has no run-to-run freedom
        g2 = _run(V, ctx, c, ratio)
        for k in ("idx", "dist", "keep", "sel", "sel_dist"):
            assert np.array_equal(g[k], g2[k]), k


@pytest.mark.parametrize("name", ["capacity_5984", "capacity_6000", "capacity_6016"])
def test_capacity_case_in_a_fresh_context(name):
    """row capacity 5984 / 6000 (key arrays in LDS, 6000 the largest that is) / 6016 (HBM scratch); then a small case on the same, grown
    context - the path follows the largest frame the context has seen, not the frame at hand"""
    import vslam_amd as V
    c = T.case(name)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=2)
    try:
        for ratio in T.RATIOS:
            g = _run(V, ctx, c, ratio)
            _check(c, ratio, g)
            g2 = _run(V, ctx, c, ratio)
            for k in ("idx", "dist", "keep", "sel", "sel_dist"):
                assert np.array_equal(g[k], g2[k]), k
        small = T.case("runs_64_65_128")
        _check(small, 0.75, _run(V, ctx, small, 0.75))
    finally:
        ctx.close()


def test_seven_kept_matches_fail_like_the_reference(shared_ctx):
    V, ctx = shared_ctx
    c = T.case("pose_7_kept")
    g = _run(V, ctx, c, 0.75, n_hyp=64)
    _check(c, 0.75, g)
    assert len(g["sel"]) == 7
    assert np.isnan(g["R"]).all() and np.isnan(g["t"]).all() and np.isnan(g["E"]).all()
    assert len(g["inlier"]) == 7 and not g["inlier"].any() and g["n_inliers"] == 0


def test_eight_kept_matches_reach_the_two_view_stage(shared_ctx):
    V, ctx = shared_ctx
    c = T.case("pose_8_kept")
    g = _run(V, ctx, c, 0.75, n_hyp=64)
    _check(c, 0.75, g)
    assert len(g["sel"]) == 8 and len(g["inlier"]) == 8 and g["n_inliers"] == g["inlier"].sum()
