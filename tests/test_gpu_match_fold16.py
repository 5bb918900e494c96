"""k_match_lds folds a train tile on 16-bit keys (distance << 7 | index in the tile) and merges the tile's two best into the running pair:
idx, dist and pass must stay, bit for bit, the two smallest (distance, trainIdx) and the f64 ratio test of a numpy brute force - around the
128-row tile, at distance 0 and 256, with ties inside a tile and across tile boundaries, with one train row, and in sliced launches.

The launcher keeps the 32-bit fold for launches of at most one workgroup per CU (match_launch_pairs), which a single small pair is.  So every
case runs twice: as one pair through match_knn2_ratio, and as 8 equal pairs of frames with room for 2000 rows through mo_dev_match_pairs:
8 pairs x 4 workgroups x 16 slices = 512 workgroups, more than the 256 CUs, so the 16-bit fold, sliced.  test_full_launch_unsliced runs it
unsliced."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I32_MAX = np.iinfo(np.int32).max


@pytest.fixture(scope="module")
def ctx():
    import os
    import vslam_amd as V
    old = os.environ.get("VSLAM_AMD_MATCHER")
    os.environ["VSLAM_AMD_MATCHER"] = "valu"
    try:
        c = V.Context(device=0, max_w=64, max_h=64, max_batch=1)
    finally:
        if old is None:
            os.environ.pop("VSLAM_AMD_MATCHER", None)
        else:
            os.environ["VSLAM_AMD_MATCHER"] = old
    yield c
    c.close()


def _brute(q, t, ratio):
    """The first two of the argsort of (distance, trainIdx) and the ratio test in f64.  Distances through one f32 product of the bit
    vectors (integers <= 256: exact).  distance * nt + trainIdx is unique per row, so its two smallest ARE that argsort's first two.
    One train row: no second neighbour -> idx -1, dist INT32_MAX, kept (the convention of tests/test_gpu_match.py's (5, 1) case)."""
    qb = np.unpackbits(q, axis=1).astype(np.float32)
    tb = np.unpackbits(t, axis=1).astype(np.float32)
    d = (qb.sum(1)[:, None] + tb.sum(1)[None, :] - 2.0 * (qb @ tb.T)).astype(np.int32)
    nq, nt = d.shape
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), I32_MAX, np.int32)
    if nt == 1:
        idx[:, 0] = 0
        dist[:, 0] = d[:, 0]
        return idx, dist, np.ones(nq, bool)
    key = d * np.int32(nt) + np.arange(nt, dtype=np.int32)[None, :]  # at most 256 * 2000 + 1999
    two = np.sort(np.partition(key, 1, axis=1)[:, :2], axis=1)
    idx[:] = two % nt
    dist[:] = two // nt
    return idx, dist, dist[:, 0].astype(np.float64) < np.float64(ratio) * dist[:, 1].astype(np.float64)


def _dev_pairs(ctx, frames, qf, tf, cap, ratio):
    """mo_dev_match_pairs over frames of at most `cap` rows -> per pair (idx, dist, pass), cut to the query frame's rows"""
    import torch
    dev = torch.device("cuda:0")
    desc_h = np.zeros((len(frames), cap, 32), np.uint8)
    for i, f in enumerate(frames):
        desc_h[i, :len(f)] = f
    desc = torch.from_numpy(desc_h).to(dev)
    counts = torch.tensor([len(f) for f in frames], dtype=torch.int32, device=dev)
    d_qf, d_tf = torch.tensor(qf, dtype=torch.int32, device=dev), torch.tensor(tf, dtype=torch.int32, device=dev)
    idx = torch.full((len(qf), cap, 2), -7, dtype=torch.int32, device=dev)
    dist = torch.full_like(idx, -7)
    ok = torch.full((len(qf), cap), 7, dtype=torch.uint8, device=dev)
    ctx._check(ctx.lib.mo_dev_match_pairs(ctx.h, desc.data_ptr(), counts.data_ptr(), cap, d_qf.data_ptr(), d_tf.data_ptr(), len(qf),
                                          float(ratio), idx.data_ptr(), dist.data_ptr(), ok.data_ptr()))
    torch.cuda.synchronize()
    idx, dist, ok = idx.cpu().numpy(), dist.cpu().numpy(), ok.cpu().numpy()
    return [(idx[p, :len(frames[a])], dist[p, :len(frames[a])], ok[p, :len(frames[a])].astype(bool)) for p, a in enumerate(qf)]


def _check(ctx, q, t, ratio=0.75):
    want = _brute(q, t, ratio)
    got = [ctx.match_knn2_ratio(q, t, ratio)] + _dev_pairs(ctx, [q, t], [0] * 8, [1] * 8, 2000, ratio)
    for idx, dist, ps in got:
        assert np.array_equal(idx, want[0])
        assert np.array_equal(dist, want[1])
        assert np.array_equal(ps, want[2])
    return got[-1]


def _descriptors(rng, n, pool):
    """n rows drawn from `pool` distinct random descriptors, a third of them with one bit flipped: exact ties and near ties everywhere"""
    words = rng.integers(0, 256, (pool, 32), dtype=np.uint8)
    d = words[rng.integers(0, pool, n)].copy()
    flip = rng.random(n) < 1 / 3
    d[flip, rng.integers(0, 32)] ^= np.uint8(1 << rng.integers(0, 8))
    return d


@pytest.mark.parametrize("nq", [1, 513])  # 513: the second query of a lane and a second workgroup
@pytest.mark.parametrize("nt", [1, 2, 127, 128, 129, 255, 256, 257, 2000])
def test_train_counts_around_the_tile(ctx, nq, nt):
    rng = np.random.default_rng(1000 * nt + nq)
    _check(ctx, _descriptors(rng, nq, 40), _descriptors(rng, nt, 40))
    _check(ctx, rng.integers(0, 256, (nq, 32), dtype=np.uint8), rng.integers(0, 256, (nt, 32), dtype=np.uint8), 0.85)


def test_distance_256_alone_and_beside_distance_0(ctx):
    rng = np.random.default_rng(5)
    q = np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), 513, axis=0)
    idx, dist, ps = _check(ctx, q, ~q[:1])  # one train row, every bit differs
    assert (dist[:, 0] == 256).all() and (idx[:, 0] == 0).all()
    idx, dist, ps = _check(ctx, q, np.concatenate([~q[:1], q[:1]]))
    assert (idx == [1, 0]).all() and (dist == [0, 256]).all() and ps.all()
    # a full tile and one row more of complements: tile-local keys up to 256 << 7 | 127, the largest there is
    idx, dist, ps = _check(ctx, q, np.repeat(~q[:1], 129, axis=0))
    assert (idx == [0, 1]).all() and (dist == 256).all() and not ps.any()
    t = np.repeat(~q[:1], 257, axis=0)
    t[127] = q[0]  # the only near row is the tile's last; the second best is a complement of the same tile
    idx, dist, ps = _check(ctx, q, t)
    assert (idx == [127, 0]).all() and (dist == [0, 256]).all()


@pytest.mark.parametrize("nt", [2, 128, 300])
def test_all_equal_descriptors(ctx, nt):
    z = np.full((513, 32), 0x5A, np.uint8)
    idx, dist, ps = _check(ctx, z, z[:nt])
    assert (idx == [0, 1]).all() and (dist == 0).all() and not ps.any()


@pytest.mark.parametrize("nt,near,nearer", [
    (128, (30, 40), (10, 20)),      # inside one tile
    (256, (126, 129), (127, 128)),  # across the 127 | 128 boundary
    (256, (127, 128), (126, 129)),
    (257, (100, 255), (200, 256)),  # across the last tile of 1 row
    (257, (200, 256), (100, 255)),
])
def test_duplicated_nearest_rows_lower_index_wins(ctx, nt, near, nearer):
    rng = np.random.default_rng(nt + near[0])
    q0 = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)  # ~128 bits away
    a, b = q0[0].copy(), q0[0].copy()
    a[3] ^= 0x10
    b[3] ^= 0x11
    t[list(nearer)] = a  # distance 1, twice
    t[list(near)] = b    # distance 2, twice
    q = np.repeat(q0, 513, axis=0)
    idx, dist, ps = _check(ctx, q, t)
    assert (idx == sorted(nearer)).all() and (dist == 1).all()
    t[max(nearer)] = b   # one row at distance 1, three at distance 2: the second best is the lowest index of those
    idx, dist, ps = _check(ctx, q, t)
    assert (idx == [min(nearer), min(near + (max(nearer),))]).all() and (dist == [1, 2]).all()


def test_single_train_row_has_no_second_neighbour(ctx):
    rng = np.random.default_rng(9)
    q, t = rng.integers(0, 256, (513, 32), dtype=np.uint8), rng.integers(0, 256, (1, 32), dtype=np.uint8)
    idx, dist, ps = _check(ctx, q, t)
    assert (idx[:, 0] == 0).all() and (idx[:, 1] == -1).all() and (dist[:, 1] == I32_MAX).all() and ps.all()


@pytest.fixture(scope="module")
def frames17():
    """17 frames of 2000 descriptors and the brute force of the 16 pairs (i, i + 1), computed once"""
    rng = np.random.default_rng(17)
    words = rng.integers(0, 256, (3000, 32), dtype=np.uint8)
    desc = words[rng.integers(0, 3000, (17, 2000))].copy()
    desc[:, ::5, 11] ^= 8
    return desc, [_brute(desc[i], desc[i + 1], 0.75) for i in range(16)]


@pytest.mark.parametrize("pairs", [1, 16])  # 4 and 64 workgroups: the launch rule slices both 16 times (32-bit fold at 1 pair, 16-bit at 16)
def test_sliced_pairs_on_the_device(ctx, frames17, pairs):
    desc, want = frames17
    got = _dev_pairs(ctx, list(desc[:pairs + 1]), list(range(pairs)), list(range(1, pairs + 1)), 2000, 0.75)
    for p in range(pairs):
        assert np.array_equal(got[p][0], want[p][0]) and np.array_equal(got[p][1], want[p][1]) and np.array_equal(got[p][2], want[p][2]), p


def test_full_launch_unsliced(ctx):
    """1152 pairs of frames with room for 300 rows (3 tiles) are 1152 workgroups: more than half of the 2048 a 256-CU device holds at once,
    so the launch is not sliced, and more than one per CU, so it folds on 16-bit keys and writes its results itself.  Every ordered pair of
    24 frames whose row counts sit around the tile, twice."""
    rng = np.random.default_rng(24)
    counts = [1, 2, 3, 64, 127, 128, 129, 130, 200, 255, 256, 257, 258, 299, 300, 1, 128, 256, 257, 300, 127, 129, 2, 255]
    frames = [_descriptors(rng, n, 12) for n in counts]
    qf = [a for a in range(24) for b in range(24)] * 2
    tf = [b for a in range(24) for b in range(24)] * 2
    got = _dev_pairs(ctx, frames, qf, tf, 300, 0.75)
    for p in range(24 * 24):
        want = _brute(frames[qf[p]], frames[tf[p]], 0.75)
        for g in (got[p], got[p + 24 * 24]):
            assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]) and np.array_equal(g[2], want[2]), (qf[p], tf[p])
