"""Tile staging of k_describe_tiles and of the blurring k_resize2: batched extraction against the CPU oracle, bit for bit, at the
sizes where the staging takes another path - the 16-byte interior form, the clamped 8-byte form, the byte fallback, windows cut
to the border region, a single tile per level - and with keypoints on the outermost rows and columns a tile stages."""
import numpy as np
import pytest

from tests.helpers import synthetic_frame

pytestmark = pytest.mark.gpu

EDGE = 31  # orb_params' default edge_threshold


@pytest.fixture(scope="module")
def ctx():
    import vslam_amd as V
    c = V.Context(device=0, max_w=320, max_h=240, max_batch=9)
    yield c
    c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import orb_oracle
    orb_oracle.lib().orc_set_variant(0, 0)
    yield orb_oracle
    orb_oracle.lib().orc_set_variant(1, 0)


def _same(got, exp):
    (kps, desc), (ek, ed) = got, exp
    assert len(kps) == len(ek)  # counts
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        assert np.array_equal(kps[f], ek[f]), f
    if len(ek):
        assert np.array_equal(desc, ed)
    else:
        assert desc is None


def _batch_against_oracle(ctx, O, imgs, **kw):
    import vslam_amd as V
    p, o = V.orb_params(select_order=V.ORDER_LIBSTDCXX, **kw), O.params(**kw)
    res = ctx.orb_detect_compute(np.stack(imgs), p)
    assert len(res) == len(imgs)
    total = 0
    for img, got in zip(imgs, res):
        exp = O.detect_and_compute(img, o)
        _same(got, exp)
        total += len(exp[0])
    return total


def test_aligned_levels_batch_of_nine(ctx, O):
    """320x240: every level's base and pitch are 16-byte aligned; nine frames = one XCD round of eight and a remainder."""
    n = _batch_against_oracle(ctx, O, [synthetic_frame(700 + i, 320, 240) for i in range(9)], nfeatures=1000)
    assert n > 9 * 500


@pytest.mark.parametrize("w,h", [(318, 240), (301, 233)])
def test_unaligned_level_zero(ctx, O, w, h):
    """A level-0 pitch that is no multiple of 4 (318 is even, 301 odd): level 0 is staged by bytes and resized / blurred by the
    unfused kernels, the levels above keep their 16-byte aligned pitch."""
    n = _batch_against_oracle(ctx, O, [synthetic_frame(710 + i, w, h) for i in range(2)], nfeatures=1000)
    assert n > 2 * 500


def test_one_tile_per_level(ctx, O):
    """200x136: the border region of level 0 is 138x74 - two tile columns (128 + 10) and rows (64 + 10) - and every level above
    is a single partial tile, so all windows are cut in both directions."""
    n = _batch_against_oracle(ctx, O, [synthetic_frame(720 + i, 200, 136) for i in range(2)], nfeatures=1000)
    assert n > 2 * 100


def test_tile_column_a_few_pixels_wide(ctx, O):
    """264x200: level 0's border region is 202 px wide and its second tile column 74; level 1 (220 wide) has a second column of
    30, level 2 (183) is one tile of 121: windows trimmed to few 16-byte pieces."""
    n = _batch_against_oracle(ctx, O, [synthetic_frame(730 + i, 264, 200) for i in range(2)], nfeatures=1000)
    assert n > 2 * 300


def _blocks(seed, w, h, cell):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.integers(0, 256, size=(h // cell + 1, w // cell + 1)).astype(np.uint8)
    return np.kron(c, np.ones((cell, cell), np.uint8))[:h, :w].copy()


def test_keypoints_on_the_outermost_rows_and_columns(ctx, O):
    """A frame of random 5-px blocks has corners everywhere; with every candidate kept, several levels hold keypoints at exactly
    edge_threshold from each of the four borders - they sample the first and last staged row and column of their tiles and the
    reflected halo of the blur.  The oracle's own result says which levels do."""
    w, h = 320, 240
    img = _blocks(3, w, h, 5)
    kw = dict(nfeatures=20000, fast_threshold=5)
    o = O.params(**kw)
    ek, _ = O.detect_and_compute(img, o)
    lw, lh, _, _ = O.levels(w, h, o)
    hit = []
    for L in range(8):
        m = ek["octave"] == L
        s = np.float32(1.2) ** L
        x, y = np.rint(ek["x"][m] / s).astype(int), np.rint(ek["y"][m] / s).astype(int)
        if (x == EDGE).any() and (x == lw[L] - EDGE - 1).any() and (y == EDGE).any() and (y == lh[L] - EDGE - 1).any():
            hit.append(L)
    assert len(hit) >= 3, hit
    _batch_against_oracle(ctx, O, [img, img[::-1].copy()], **kw)


def test_compute_at_caller_keypoints_unaligned_width(ctx, O):
    """compute() blurs whole levels (no fused resize): 318x240, keypoints on several octaves."""
    import vslam_amd as V
    w, h = 318, 240
    img = synthetic_frame(740, w, h)
    p, o = V.orb_params(select_order=V.ORDER_LIBSTDCXX), O.params()
    rng = np.random.default_rng(2)
    n = 200
    k = np.zeros(n, V.KP_DTYPE)
    k["x"] = rng.uniform(0, w, n).astype(np.float32); k["y"] = rng.uniform(0, h, n).astype(np.float32)
    k["size"] = 31; k["class_id"] = -1
    k["octave"] = rng.integers(0, 4, n); k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    kept, desc = ctx.orb_compute(img, p, k)
    ekept, edesc = O.compute(img, o, k)
    assert 0 < len(ekept) < n
    assert np.array_equal(kept, ekept) and np.array_equal(desc, edesc)
