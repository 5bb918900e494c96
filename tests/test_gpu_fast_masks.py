"""k_fast against the oracle on images built for the FAST arc network and the non-max suppression: every one of the 65 536
bright / dark circle masks at contrasts around the threshold, and dense textures with far more corners per strip than the
896-entry list the kernel used to keep, on the batched (8-row) and the single-frame (2-row) strip plans."""
import numpy as np
import pytest

from tests.helpers import synthetic_frame

pytestmark = pytest.mark.gpu

CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
          (-2, 2), (-1, 3)]
W, H = 640, 480


@pytest.fixture(scope="module", params=[8, 1], ids=["batched", "single"])
def ctx(request):
    import vslam_amd as V
    c = V.Context(device=0, max_w=1024, max_h=1024, max_batch=request.param)
    yield c
    c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import orb_oracle
    return orb_oracle


def _check_level0(ctx, O, img, thr):
    import vslam_amd as V
    p = V.orb_params(select_order=V.ORDER_LIBSTDCXX, fast_threshold=thr, nlevels=1)
    f = O.fast_level(img, thr)
    f = f[(f[:, 0] >= 31) & (f[:, 0] < W - 31) & (f[:, 1] >= 31) & (f[:, 1] < H - 31)]
    got = ctx.dbg_fast_level(img, p, 0)
    assert len(got) == len(f) and np.array_equal(got, f)
    return len(f)


def _mask_images(thr, seed, equal_for_zero):
    """centres on an 8-px grid inside the border; centre c, circle pixel k = c + t + dt when bit k of the cell's mask is set and
    c - t - dt (or c, equal_for_zero) otherwise, dt in {-1, 0, 1} per pixel; 18 images hold all 65 536 masks"""
    rng = np.random.Generator(np.random.PCG64(seed))
    xs, ys = np.arange(36, W - 36, 8), np.arange(36, H - 34, 8)
    per = len(xs) * len(ys)
    masks = np.arange(65536)
    for first in range(0, 65536, per):
        m = masks[first:first + per]
        img = np.zeros((H, W), np.int32)
        cy, cx = np.meshgrid(ys, xs, indexing="ij")
        cy, cx = cy.ravel()[:len(m)], cx.ravel()[:len(m)]
        c = rng.choice([0, 1, 60, 128, 200, 254, 255], size=len(m))
        img[:] = 128
        img[cy, cx] = c
        for k, (dx, dy) in enumerate(CIRCLE):
            dt = rng.integers(-1, 2, size=len(m))
            bit = (m >> k) & 1
            lo = c if equal_for_zero else c - thr - dt
            img[cy + dy, cx + dx] = np.where(bit == 1, c + thr + dt, lo)
        yield np.clip(img, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("thr", [1, 7, 20])
def test_fast_all_circle_masks(ctx, O, thr):
    n = 0
    for i, img in enumerate(_mask_images(thr, 100 + thr, equal_for_zero=False)):
        n += _check_level0(ctx, O, img, thr)
        n += _check_level0(ctx, O, 255 - img, thr)
    for img in _mask_images(thr, 200 + thr, equal_for_zero=True):
        n += _check_level0(ctx, O, img, thr)
    assert n > 0


@pytest.mark.parametrize("thr", [0, 7])
def test_fast_dense_texture_beyond_old_list(ctx, O, thr):
    """2-px texture: about half the pixels of the band are corners, several times the old list's 896 entries per 8-row strip"""
    rng = np.random.Generator(np.random.PCG64(7 + thr))
    cells = rng.integers(0, 256, size=(H // 2, W // 2))
    img = np.repeat(np.repeat(cells, 2, 0), 2, 1).astype(np.uint8)
    img[::3, ::3] = rng.integers(0, 256, size=img[::3, ::3].shape)
    kept = O.fast_level(img, thr)
    kept = kept[(kept[:, 1] >= 31) & (kept[:, 1] < H - 31)]
    assert np.bincount((kept[:, 1] - 31) // 8).max() > 150  # corners after the NMS per 8 rows; the scored band of a strip holds ~3000
    _check_level0(ctx, O, img, thr)
    tex = synthetic_frame(3)
    _check_level0(ctx, O, tex, thr)
