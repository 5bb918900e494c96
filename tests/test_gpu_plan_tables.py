"""A plan is complete when mo_build_plan returns: its tables, its work buffers and the describe kernels' list of left-over tiles are made
there, not by whichever launcher first runs under it.  So a call's result cannot depend on which entry point ran first under the plan:
every entry point of the extraction path, in several orders on fresh contexts, gives byte-identical results, and leaves no error and
no device flag behind."""
import numpy as np
import pytest

import vslam_amd as V
from oracle import orb_oracle as O
from tests.helpers import synthetic_frame

pytestmark = pytest.mark.gpu

# name, w, h, ORB parameters
SHAPES = [
    ("level_without_border", 96, 80, dict(nfeatures=100, nlevels=3)),    # level 2 (67 x 56): no strips and no describe tiles on it
    ("four_levels", 160, 120, dict(nfeatures=300, nlevels=4)),
    ("gather_resize", 333, 96, dict(scale_factor=2.0, nlevels=2)),       # level 1 is 166 wide from 333: k_resize, the unpacked coefficients
    # no level has a border region: no describe tile, zero keypoints.  (64 x 64 is the smallest frame; at the default edge_threshold
    # of 31 its level 0 keeps a region of 2 x 2, so the threshold is 32 here)
    ("no_border_anywhere", 64, 64, dict(nfeatures=300, nlevels=2, edge_threshold=32)),
]
CALLS = ["detect", "detect_nodesc", "batch3", "compute", "compute_octave", "grid", "pyramid"]
# every call first on a fresh context once, and the whole list backwards; batch3 (a larger batch) and compute_octave (more levels)
# rebuild the plan, as does the call after compute_octave: the calls behind them run first under a plan in the middle of a context's life
ORDERS = [CALLS[i:] + CALLS[:i] for i in range(len(CALLS))] + [CALLS[::-1]]


def _bytes_of(x):
    if isinstance(x, (list, tuple)):
        return [_bytes_of(v) for v in x]
    return None if x is None else np.asarray(x).tobytes()


def _call(ctx, name, imgs, prm, kps):
    img = imgs[0]
    if name == "detect":
        return ctx.orb_detect_compute(img, prm)
    if name == "detect_nodesc":
        return ctx.orb_detect_compute(img, prm, want_desc=False)
    if name == "batch3":
        return ctx.orb_detect_compute(imgs, prm)
    if name == "compute":
        return ctx.orb_compute(img, prm, kps)
    if name == "compute_octave":
        k = kps.copy()
        if len(k):
            k["octave"][len(k) // 2] = prm.nlevels   # above the plan's last level: the call builds a plan with one level more
        return ctx.orb_compute(img, prm, k)
    if name == "grid":
        return ctx.grid_detect_compute(img, prm, 128)
    assert name == "pyramid"
    return [ctx.dbg_pyramid_level(img, prm, L, blurred=True) for L in range(prm.nlevels)]


def _sequence(order, w, h, imgs, prm, kps):
    ctx = V.Context(max_w=w, max_h=h, max_batch=4)
    try:
        out = {name: _call(ctx, name, imgs, prm, kps) for name in order}
        assert ctx.lib.mo_last_error(ctx.h).decode() == "", order
        assert ctx.dev_status() == 0, order
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("name,w,h,kw", SHAPES, ids=[s[0] for s in SHAPES])
def test_results_do_not_depend_on_the_first_entry_point(name, w, h, kw):
    imgs = np.stack([synthetic_frame(20261018 + i, w, h) for i in range(3)])
    prm = V.orb_params(**kw)
    ctx = V.Context(max_w=w, max_h=h, max_batch=4)
    (kps, desc), = ctx.orb_detect_compute(imgs[0], prm)   # the keypoints the compute calls of every order are given
    ctx.close()
    if name == "no_border_anywhere":
        assert len(kps) == 0 and desc is None
    else:
        # what the compute calls need of their input: one keypoint whose octave compute_octave raises and one that stays.  (No more can
        # be asked of the smallest shape: the border region of 96 x 80 is 34 x 18 positions on level 0 and 18 x 5 on level 1.)
        assert len(kps) >= 2

    first = _sequence(ORDERS[0], w, h, imgs, prm, kps)
    assert _bytes_of(first["detect"]) == _bytes_of([(kps, desc)])
    assert len(first["compute"][0]) == len(first["compute_octave"][0]) == len(kps)
    # the blurred levels against the oracle: the whole-level blur tiles and the resize coefficients, anchored outside the library
    o = O.params(**kw)
    for L in range(prm.nlevels):
        assert np.array_equal(first["pyramid"][L], O.pyramid_level(imgs[0], o, L, blurred=True)), L
    want = {k: _bytes_of(v) for k, v in first.items()}
    for order in ORDERS[1:]:
        got = _sequence(order, w, h, imgs, prm, kps)
        for call in CALLS:
            assert _bytes_of(got[call]) == want[call], (call, "in the order", order)
