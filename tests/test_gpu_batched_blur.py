"""The batched extraction (three or more frames) writes the blurred levels 0 .. n-2 from the resize launches (k_resize2's blurring
form) where the plan allows it, and blurs the last level alone.  The pyramid and blur buffers are poisoned before every extraction:
inside the blur region [margin, size - margin) every blurred byte must be the oracle's, and keypoints and descriptors must be the
oracle's bit for bit."""
import numpy as np
import pytest

from tests.helpers import synthetic_frame

pytestmark = pytest.mark.gpu

BATCH = 3

# (w, h), nlevels, edge_threshold: widths that are a multiple of 4 take the blurring resize, the others (478, 333, 331) the
# unfused k_resize / k_blur path, which must give the same bytes
CASES = [
    ((640, 480), 8, 31),
    ((640, 480), 2, 31),
    ((640, 480), 1, 31),
    ((640, 480), 8, 23),
    ((640, 480), 8, 19),
    ((752, 480), 8, 40),
    ((1024, 768), 8, 31),
    ((400, 300), 6, 27),
    ((478, 850), 8, 31),
    ((333, 257), 8, 31),
    ((331, 241), 8, 25),
]


@pytest.fixture(scope="module")
def O():
    from oracle import orb_oracle
    return orb_oracle


@pytest.mark.parametrize("size,nlevels,edge", CASES)
def test_batched_blur_and_outputs_match_oracle(O, size, nlevels, edge):
    import vslam_amd as V
    w, h = size
    frames = [synthetic_frame(4100 + 17 * i + w, w, h) for i in range(BATCH)]
    kw = dict(nfeatures=1000, nlevels=nlevels, edge_threshold=edge, fast_threshold=7)
    p = V.orb_params(select_order=0, **kw)
    o = O.params(**kw)
    bm = (edge - 19) & ~3
    O.lib().orc_set_variant(0, 0)
    try:
        expb = [[O.pyramid_level(f, o, L, blurred=True) for L in range(nlevels)] for f in frames]
        exp = [O.detect_and_compute(f, o) for f in frames]
        for poison in (0, 255, 90):
            c = V.Context(device=0, max_w=1024, max_h=1024, max_batch=4)
            c._check(c.lib.mo_dbg_set_poison(c.h, poison))
            try:
                got = c.orb_detect_compute(np.stack(frames), p)
                for i in range(BATCH):
                    for L in range(nlevels):
                        b, fused = c.dbg_blur_level(i, L, w, h)
                        e = expb[i][L]
                        assert b.shape == e.shape
                        lh, lw = e.shape
                        assert np.array_equal(b[bm:lh - bm, bm:lw - bm], e[bm:lh - bm, bm:lw - bm]), (poison, i, L)
                    if size == (640, 480) and nlevels >= 2 and edge == 31:
                        assert fused, "the default geometry must take the blurring resize"
                    (k, d), (ek, ed) = got[i], exp[i]
                    for fld in ("x", "y", "angle", "response", "octave"):
                        assert np.array_equal(k[fld], ek[fld]), (poison, i, fld)
                    assert np.array_equal(d, ed), (poison, i)
            finally:
                c.close()
    finally:
        O.lib().orc_set_variant(1, 0)
