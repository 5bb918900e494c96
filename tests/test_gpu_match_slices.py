"""The default matcher with its train set cut into 1, 2, 4 and 8 slices (VSLAM_AMD_MATCHER=valu1 .. valu8 force the count that
match_launch_pairs otherwise derives from the launch and the device): (idx, dist, pass) equal the CPU oracle bit for bit whatever the
slicing - slices without a tile, descriptors one past a tile, exact ties across slice boundaries - and the launch rule itself slices a
launch of 40 small pairs."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 128  # train descriptors per LDS tile of k_match_lds (ML_TILE): slices are whole tiles


def _context(mode):
    import vslam_amd as V
    old = os.environ.get("VSLAM_AMD_MATCHER")
    os.environ["VSLAM_AMD_MATCHER"] = mode
    try:
        return V.Context(device=0, max_w=1024, max_h=1024, max_batch=4)
    finally:
        if old is None:
            os.environ.pop("VSLAM_AMD_MATCHER", None)
        else:
            os.environ["VSLAM_AMD_MATCHER"] = old


@pytest.fixture(scope="module", params=["valu1", "valu2", "valu4", "valu8"])
def ctx(request):
    c = _context(request.param)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rule_ctx():
    c = _context("valu")
    yield c
    c.close()


def _check(ctx, q, t, ratio):
    """q, t: (B, n, 32) or (n, 32); every pair against the oracle, exactly"""
    from oracle import orb_oracle as O
    idx, dist, ps = ctx.match_knn2_ratio(q, t, ratio)
    pairs = zip(q, t, idx, dist, ps) if q.ndim == 3 else [(q, t, idx, dist, ps)]
    for b, (qb, tb, ib, db, pb) in enumerate(pairs):
        eidx, edist = O.match_knn2(qb, tb)
        assert np.array_equal(ib, eidx), "idx of pair %d" % b
        assert np.array_equal(db, edist), "dist of pair %d" % b
        eps = O.ratio_test(eidx, edist, ratio if ratio is not None else 1.0, enabled=ratio is not None)
        assert np.array_equal(pb, eps), "pass of pair %d" % b
    return idx, dist


@pytest.mark.parametrize("nt", [1, 129, 257, 1000])  # fewer tiles than slices; one descriptor past a tile (twice); several tiles per slice
@pytest.mark.parametrize("nq", [1, 513])             # 513 crosses the 512-query block
def test_batched_sizes(ctx, nq, nt):
    rng = np.random.default_rng(nq * 7919 + nt)
    _check(ctx, rng.integers(0, 256, (3, nq, 32), dtype=np.uint8), rng.integers(0, 256, (3, nt, 32), dtype=np.uint8), 0.8)


def test_ties_across_slice_boundaries(ctx):
    """Train descriptors drawn from 5 words: every distance occurs in every slice, and the lowest train index must win both slots."""
    rng = np.random.default_rng(4 * TILE + 1)
    words = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    nq, nt = 300, 4 * TILE + 1
    q = words[rng.integers(0, 5, nq)].copy()
    t = words[rng.integers(0, 5, nt)].copy()
    q[::3, 7] ^= 4
    idx, dist = _check(ctx, q, t, 0.75)
    d = np.unpackbits(q[:, None, :] ^ t[None, :, :], axis=2).sum(axis=2)  # (nq, nt) Hamming distances
    order = np.argsort(d, axis=1, kind="stable")[:, :2]                   # stable: ties towards the lower train index
    assert np.array_equal(idx, order)
    assert np.array_equal(dist, np.take_along_axis(d, order, axis=1))
    assert (dist[:, 0] == dist[:, 1]).all()  # (every word occurs more than once: the runner-up ties with the winner)


@pytest.mark.parametrize("ratio", [0.75, None])
def test_ratio_and_ratio_off(ctx, ratio):
    rng = np.random.default_rng(11)
    _check(ctx, rng.integers(0, 256, (3, 200, 32), dtype=np.uint8), rng.integers(0, 256, (3, 300, 32), dtype=np.uint8), ratio)


def test_rule_slices_many_small_pairs(rule_ctx):
    """40 pairs of 64 x 200 descriptors: 40 workgroups, more than the 32 that sliced before, far fewer than the device holds - the
    launch rule itself cuts the two train tiles into two slices."""
    rng = np.random.default_rng(40)
    _check(rule_ctx, rng.integers(0, 256, (40, 64, 32), dtype=np.uint8), rng.integers(0, 256, (40, 200, 32), dtype=np.uint8), 0.75)
