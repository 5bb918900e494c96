"""The blurring k_resize2 reads a per-tile record of the plan instead of deriving its tile in a scalar prologue: batched extraction
against the CPU oracle, bit for bit, at the geometries where the records differ in kind - interior windows (blur margin >= 4),
windows that leave the level (margin 0: the interior flag clear, reflected staging), single and few-pixel tile columns, levels
without a border region, no resize launch at all, a level that keeps the gather kernel, an unfused level 0 - and on one context
taken through several plans, whose records must be rebuilt with each.  Every case also states whether its plan takes the blurring
resize (the probe mo_dbg_blur_level reports the plan's verdict), so a case meant for the record-reading kernel cannot pass on the
unfused pair, nor a check that refused everything.  Batches of 3 and 9 frames: the batched path needs more than two, and nine is
one XCD round of eight plus a remainder."""
import numpy as np
import pytest

from tests.helpers import synthetic_frame

pytestmark = pytest.mark.gpu


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


def _blocks(seed, w, h, cell=5):
    """Random 5-px blocks: corners everywhere, for levels whose border region is a few pixels."""
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.integers(0, 256, size=(h // cell + 1, w // cell + 1)).astype(np.uint8)
    return np.kron(c, np.ones((cell, cell), np.uint8))[:h, :w].copy()


_expected = {}  # (frame maker, seed, w, h, parameters) -> the oracle's result, computed once and never modified


def _oracle(O, frame, seed, w, h, kw):
    key = (frame.__name__, seed, w, h, tuple(sorted(kw.items())))
    if key not in _expected:
        _expected[key] = O.detect_and_compute(frame(seed, w, h), O.params(**kw))
    return _expected[key]


def _same(got, exp):
    (kps, desc), (ek, ed) = got, exp
    assert len(kps) == len(ek)  # counts
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        assert np.array_equal(kps[f], ek[f]), f
    if len(ek):
        assert np.array_equal(desc, ed)
    else:
        assert desc is None


def _levels_with_room(O, w, h, kw):
    """Levels whose border region is not empty: the ones that can hold a keypoint."""
    o = O.params(**kw)
    lw, lh, _, _ = O.levels(w, h, o)
    return sum(1 for a, b in zip(lw, lh) if a > 2 * o.edge_threshold and b > 2 * o.edge_threshold)


def _run(c, O, seed0, w, h, batch, fused, frame=synthetic_frame, **kw):
    """`batch` frames through the batched path of context c against the oracle; the oracle alone first says that the case is not
    empty: keypoints on at least three levels (or on every level that has room for one).  fused: whether the plan must let the
    resize launches write the blurred levels (the kernel that reads the records)."""
    import vslam_amd as V
    exp = [_oracle(O, frame, seed0 + i, w, h, kw) for i in range(batch)]
    need = min(3, _levels_with_room(O, w, h, kw))
    for ek, _ in exp:
        assert len(np.unique(ek["octave"])) >= need, (np.unique(ek["octave"]), need)
    res = c.orb_detect_compute(np.stack([frame(seed0 + i, w, h) for i in range(batch)]), V.orb_params(select_order=V.ORDER_LIBSTDCXX, **kw))
    assert len(res) == batch
    assert c.dbg_blur_level(0, 0, w, h)[1] == fused, "the plan's verdict on the blurring resize"
    for got, e in zip(res, exp):
        _same(got, e)
    return res


@pytest.mark.parametrize("batch", [3, 9])
@pytest.mark.parametrize("edge,fused", [(31, True), (23, False), (19, True), (21, True)])
def test_interior_and_border_windows(ctx, O, edge, fused, batch):
    """320x240.  edge_threshold 31: blur margin 12, the windows lie inside the level (the record's 16-byte staging form) and the plan
    fuses.  19 and 21: margin 0, the plan fuses, and every border tile's window leaves the level - 52 of its 61 records have the
    interior flag clear and are staged with REFLECT_101.  23: margin 4 without a pyramid margin; the plan refuses the fused form
    (the last partitions of levels 5 and 7 are empty), its records are built and must not be used."""
    _run(ctx, O, 800, 320, 240, batch, fused, nfeatures=1000, edge_threshold=edge)


@pytest.mark.parametrize("batch", [3, 9])
def test_margin_four_fused(ctx, O, batch):
    """304x228 at edge_threshold 23: blur margin 4, and this plan fuses.  The only margin at which the interior flag's "the last tap
    and the resize's sources are pixels" term decides: of the plan's 49 records 41 take the 16-byte form, 5 of them with a window
    that ends in the row's padding, and 8 the reflecting dword form."""
    _run(ctx, O, 860, 304, 228, batch, True, nfeatures=1000, edge_threshold=23)


@pytest.mark.parametrize("batch", [3, 9])
@pytest.mark.parametrize("w,h", [(200, 136), (264, 200)])
def test_single_and_narrow_tile_columns(ctx, O, w, h, batch):
    """200x136: every level above 0 is one resize tile (a grid one tile wide); 264x200: second tile columns of a few pixels."""
    _run(ctx, O, 810, w, h, batch, True, nfeatures=1000)


@pytest.mark.parametrize("batch", [3, 9])
def test_levels_without_border_region(ctx, O, batch):
    """100x80: from level 2 (69x56) up no level has a border region - no describe tiles there - while the resize launches still
    cover those levels, each with its records.  Level 1's border region is 21 x 5: frames of random blocks put keypoints there."""
    assert _levels_with_room(O, 100, 80, dict(nfeatures=500)) == 2
    _run(ctx, O, 820, 100, 80, batch, True, frame=_blocks, nfeatures=500)


@pytest.mark.parametrize("batch", [3, 9])
def test_one_level(ctx, O, batch):
    """nlevels = 1: no resize launch, no resize records, nothing to fuse."""
    _run(ctx, O, 830, 320, 240, batch, False, nfeatures=500, nlevels=1)


@pytest.mark.parametrize("batch", [3, 9])
def test_gather_level_takes_no_records(O, batch):
    """333x96 at scale 2.0: level 1 is 166 wide, its ratio a little above 2, and keeps the gather kernel: the plan is unfused and
    its records must not be used.  (333 columns need a context of their own: the module's is 320 wide.)"""
    import vslam_amd as V
    c = V.Context(device=0, max_w=336, max_h=240, max_batch=9)
    try:
        _run(c, O, 840, 333, 96, batch, False, nfeatures=500, scale_factor=2.0, nlevels=2)
    finally:
        c.close()


@pytest.mark.parametrize("batch", [3, 9])
def test_unaligned_level_zero(ctx, O, batch):
    """318x240: the plan allows the fused form (its verdict is about geometry), but level 0's pitch is no multiple of 4 and the
    launcher then takes the unfused kernels for the whole pyramid: records built, none read."""
    _run(ctx, O, 850, 318, 240, batch, True, nfeatures=1000)


def test_records_follow_the_plan(ctx, O):
    """One context through 320x240 -> 200x136 -> 320x240 and edge_threshold 31 -> 19 -> 31: every result equals the oracle's and
    that of a fresh context, so the records were rebuilt with each plan."""
    import vslam_amd as V
    steps = [(320, 240, 31), (200, 136, 31), (320, 240, 31), (320, 240, 19), (320, 240, 31)]
    fresh = {}
    for w, h, edge in steps:
        got = _run(ctx, O, 800, w, h, 3, True, nfeatures=1000, edge_threshold=edge)
        if (w, h, edge) not in fresh:
            c = V.Context(device=0, max_w=320, max_h=240, max_batch=9)
            try:
                fresh[(w, h, edge)] = _run(c, O, 800, w, h, 3, True, nfeatures=1000, edge_threshold=edge)
            finally:
                c.close()
        for a, b in zip(got, fresh[(w, h, edge)]):
            _same(a, b)
