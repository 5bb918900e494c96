"""k_fast against the oracle at the level widths where its compass loop changes shape.  The loop walks the scored columns of a strip
(w - 60 of them) in 64-column chunks dealt round-robin to four wavefronts, and only a row's last chunk masks its lanes: widths
64 .. 636 give a level narrower than one chunk, a last chunk of 63, 64 and 1 columns, and 4, 5, 8 and 9 chunks per row (once and twice the
wavefront count, and one past each); heights 71 and 135 leave one row to the last 8-row strip.  Images: the 2-px dense texture of test_gpu_fast_masks (its stacks
pass 64 entries many times per strip), its complement (the other polarity's stack), a constant image (no survivor), and the texture with
everything but the last three scored columns flattened, so that only the end of a row pushes.  Batched (8-row) and single-frame
(2-row) strip plans, compared bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDTHS = [64, 123, 124, 125, 187, 188, 189, 316, 380, 572, 636]  # scored widths 4, 63, 64, 65, 127, 128, 129, 256, 320, 512, 576
HEIGHTS = [71, 135]
KINDS = ["dense", "complement", "constant", "last3"]
_ref = {}  # (kind, w, h, thr) -> (image, oracle corners inside the border); computed once, shared by both contexts


@pytest.fixture(scope="module", params=[8, 1], ids=["batched", "single"])
def ctx(request):
    import vslam_amd as V
    c = V.Context(device=0, max_w=1024, max_h=1024, max_batch=request.param)
    yield c
    c.close()


def _texture(thr):
    """the 640 x 480 texture of test_fast_dense_texture_beyond_old_list"""
    rng = np.random.Generator(np.random.PCG64(7 + thr))
    cells = rng.integers(0, 256, size=(240, 320))
    img = np.repeat(np.repeat(cells, 2, 0), 2, 1).astype(np.uint8)
    img[::3, ::3] = rng.integers(0, 256, size=img[::3, ::3].shape)
    return img


def _image(kind, w, h, thr):
    tex = _texture(thr)[:h, :w]
    if kind == "dense":
        return tex.copy()
    if kind == "complement":
        return (255 - tex).astype(np.uint8)
    if kind == "constant":
        return np.full((h, w), 128, np.uint8)
    img = np.full((h, w), 128, np.uint8)  # last3: the scored columns are 30 .. w - 31
    img[:, w - 33:w - 30] = tex[:, w - 33:w - 30]
    return img


def _reference(kind, w, h, thr):
    key = (kind, w, h, thr)
    if key not in _ref:
        from oracle import orb_oracle
        img = _image(kind, w, h, thr)
        f = orb_oracle.fast_level(img, thr)
        f = f[(f[:, 0] >= 31) & (f[:, 0] < w - 31) & (f[:, 1] >= 31) & (f[:, 1] < h - 31)]
        img.setflags(write=False)
        f.setflags(write=False)
        _ref[key] = (img, f)
    return _ref[key]


@pytest.mark.parametrize("thr", [0, 7])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_fast_chunk_shapes(ctx, w, h, kind, thr):
    import vslam_amd as V
    img, want = _reference(kind, w, h, thr)
    if kind in ("dense", "complement") or (kind == "last3" and h == 135):
        assert len(want) > 0  # no vacuous case
    if kind == "constant":
        assert len(want) == 0
    p = V.orb_params(select_order=V.ORDER_LIBSTDCXX, fast_threshold=thr, nlevels=1)
    got = ctx.dbg_fast_level(img, p, 0)
    assert len(got) == len(want) and np.array_equal(got, want)
