"""Phase C of k_describe_tiles gives a keypoint one wavefront: a workgroup's four wavefronts take the tile's keypoints four at a time and a
wave-wide compare yields 64 descriptor bits.  Batched and single-frame extraction against the CPU oracle, bit for bit, where that
layout can go wrong: tiles with fewer keypoints than wavefronts, partial last rounds, empty tiles, exact multiples of the wave count,
the rare kernel's chunks and passes, and the keypoints-only form.  Every test recomputes the keypoints per tile from the oracle's
result with the plan's grid (border region from edge_threshold, 128 x 64 tiles) and asserts that its regime occurs."""
import numpy as np
import pytest

from tests.helpers import synthetic_frame

EDGE = 31            # orb_params' default edge_threshold
DT_W, DT_H = 128, 64  # plan_tables.h
DT_LIST, DT_CHUNK = 256, 512  # keypoints of a tile / records of a level's list the one-pass kernel takes
NW = 4               # wavefronts of a workgroup


def test_wave_masks_are_the_descriptor_bytes():
    """Test t is bit t & 7 of descriptor byte t >> 3.  Lane l of a wavefront evaluating test 64 r + l, the wave-wide compare of round r
    is a 64-bit mask with test 64 r + l at bit l: four masks stored little-endian are the 32 bytes."""
    rng = np.random.default_rng(11)
    for _ in range(20):
        t0, t1 = rng.integers(0, 256, 256), rng.integers(0, 256, 256)
        bit = t0 < t1
        expect = np.array([sum(int(bit[8 * i + k]) << k for k in range(8)) for i in range(32)], np.uint8)
        masks = np.array([sum(int(bit[64 * r + l]) << l for l in range(64)) for r in range(4)], dtype="<u8")
        assert np.array_equal(masks.view(np.uint8), expect)
        assert np.array_equal(np.packbits(bit, bitorder="little"), expect)


@pytest.fixture(scope="module")
def ctx():
    import vslam_amd as V
    c = V.Context(device=0, max_w=320, max_h=240, max_batch=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import orb_oracle
    orb_oracle.lib().orc_set_variant(0, 0)
    yield orb_oracle
    orb_oracle.lib().orc_set_variant(1, 0)


def _blocks(seed, w, h, cell):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.integers(0, 256, size=(h // cell + 1, w // cell + 1)).astype(np.uint8)
    return np.kron(c, np.ones((cell, cell), np.uint8))[:h, :w].copy()


def _tile_counts(O, img, o, ek):
    """-> per level: (keypoints of the level, [keypoints per tile of the level's grid, row-major]); levels without a border region: no tiles"""
    h, w = img.shape
    lw, lh, _, _ = O.levels(w, h, o)
    out = []
    for L in range(o.nlevels):
        m = ek["octave"] == L
        s = np.float32(1.2) ** L
        x, y = np.rint(ek["x"][m] / s).astype(int), np.rint(ek["y"][m] / s).astype(int)
        bw, bh = lw[L] - 2 * EDGE, lh[L] - 2 * EDGE
        if bw <= 0 or bh <= 0:
            assert not m.any()
            out.append((0, []))
            continue
        c = np.zeros(((bh + DT_H - 1) // DT_H, (bw + DT_W - 1) // DT_W), int)
        np.add.at(c, ((y - EDGE) // DT_H, (x - EDGE) // DT_W), 1)
        out.append((int(m.sum()), c.ravel().tolist()))
    return out


def _same(got, exp, want_desc=True):
    (kps, desc), (ek, ed) = got, exp
    assert len(kps) == len(ek)
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        assert np.array_equal(kps[f], ek[f]), f
    if want_desc and len(ek):
        assert np.array_equal(desc, ed)
    else:
        assert desc is None


def _check(ctx, O, img, want_desc=True, **kw):
    """img alone (one frame: DT_SPLIT_LATENCY workgroups share a tile) and in a batch of three with its two mirror images (one workgroup
    per tile) against the oracle -> the first frame's tile counts"""
    import vslam_amd as V
    p, o = V.orb_params(select_order=V.ORDER_LIBSTDCXX, **kw), O.params(**kw)
    imgs = [img, img[::-1].copy(), img[:, ::-1].copy()]
    exp = [O.detect_and_compute(i, o, want_desc=want_desc) for i in imgs]
    (one,) = ctx.orb_detect_compute(img, p, want_desc=want_desc)
    _same(one, exp[0], want_desc)
    res = ctx.orb_detect_compute(np.stack(imgs), p, want_desc=want_desc)
    assert len(res) == 3
    for got, e in zip(res, exp):
        _same(got, e, want_desc)
    return _tile_counts(O, img, o, exp[0][0])


@pytest.mark.gpu
@pytest.mark.parametrize("nfeatures", [3, 8, 20, 40, 100])
def test_fewer_keypoints_than_wavefronts_and_partial_rounds(ctx, O, nfeatures):
    """200x136: level 0 is 2 x 2 tiles, the levels above one tile each.  With 3 - 100 features wanted the tiles hold 1 .. 18 keypoints:
    wavefronts without a keypoint, last rounds of 1, 2 and 3, and level-0 tiles with none at all."""
    tc = _check(ctx, O, synthetic_frame(720, 200, 136), nfeatures=nfeatures)
    tiles = [n for _, per in tc for n in per]
    assert 0 in tc[0][1], tc                                   # an empty tile beside filled ones on level 0
    assert any(0 < n < NW for n in tiles), tc                  # fewer keypoints than wavefronts
    if nfeatures == 3:
        assert max(tiles) == 1, tc
    if nfeatures >= 20:
        assert {n % NW for n in tiles if n > 0} >= {1, 2, 3}, tc   # last rounds of one, two and three wavefronts
    if nfeatures == 100:
        assert any(n > 16 for n in tiles), tc                  # more than one round of the 16-lane phase A


@pytest.mark.gpu
def test_rare_kernel_chunks_and_list_limits(ctx, O):
    """Random 4-px blocks, every candidate kept: level lists over DT_CHUNK (several chunks, two passes each), tiles over DT_LIST, a tile of
    exactly DT_LIST (the largest the one-pass kernel takes - but its level's list is long, so the rare kernel has it), a single-tile
    level with a short list and a long tile, and small tiles of the one-pass kernel on the coarse levels."""
    tc = _check(ctx, O, _blocks(5, 320, 240, 4), nfeatures=20000)
    lists = [n for n, _ in tc]
    tiles = [n for _, per in tc for n in per]
    assert sum(n > DT_CHUNK for n in lists) >= 3, tc
    assert DT_LIST in tiles and sum(n > DT_LIST for n in tiles) >= 3 and any(n > DT_CHUNK for n in tiles), tc
    assert any(n <= DT_CHUNK and per == [n] and n > DT_LIST for n, per in tc), tc
    assert sum(0 < n <= DT_LIST and ln <= DT_CHUNK for ln, per in tc for n in per) >= 3, tc


@pytest.mark.gpu
def test_exact_multiples_of_the_wave_count(ctx, O):
    """Random 5-px blocks: level 0's list is under DT_CHUNK, so the one-pass kernel describes its nine tiles - among them tiles of 64
    (sixteen full rounds of four wavefronts, no partial one), 1, 2 and 97 keypoints; levels 1 and 2 go to the rare kernel."""
    tc = _check(ctx, O, _blocks(5, 320, 240, 5), nfeatures=20000)
    n0, t0 = tc[0]
    assert 0 < n0 <= DT_CHUNK and len(t0) == 9 and max(t0) <= DT_LIST, tc
    assert any(n > 0 and n % 64 == 0 for n in t0) and 1 in t0 and 2 in t0 and any(n % NW == 1 and n > 64 for n in t0), tc
    assert tc[1][0] > DT_CHUNK and tc[2][0] > DT_CHUNK, tc


@pytest.mark.gpu
def test_keypoints_without_descriptors(ctx, O):
    """The keypoints-only kernels (no phase B / C, phase A as before) on the small-tile frame and on the rare path's frame."""
    tc = _check(ctx, O, synthetic_frame(720, 200, 136), want_desc=False, nfeatures=100)
    assert any(0 < n < NW for _, per in tc for n in per), tc
    tc = _check(ctx, O, _blocks(5, 320, 240, 4), want_desc=False, nfeatures=20000)
    assert any(n > DT_LIST for _, per in tc for n in per), tc
