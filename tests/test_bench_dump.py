"""CPU: bench.py --dump-outputs writes the last timed step's arrays as finite float32 / float64 .npy files within the size bound, with
the rows past a frame's keypoint count blanked, the library's NaN markers turned into validity masks and a fixed sample of the frames
once the batch is larger than the dump keeps."""
import os

import numpy as np

import bench


def _outputs(n, seed=0):
    rng = np.random.default_rng(seed)
    cap = bench.CAP
    kps = rng.random((n, cap, 7), dtype=np.float32)
    kps.view(np.int32)[..., 5] = rng.integers(0, 8, (n, cap))
    kps.view(np.int32)[..., 6] = -1
    counts = rng.integers(cap - 100, cap + 50, n).astype(np.int32)   # a count above cap: the frame overflowed and was truncated
    pts = rng.random((n - 1, cap, 3), dtype=np.float32)
    pts[rng.random((n - 1, cap)) < 0.5] = np.nan    # the library's "no map point"
    pose = rng.random((n - 1, 12))
    pose[1] = np.nan                                 # the library's "no model" for a pair
    return dict(kps=kps, desc=rng.integers(0, 256, (n, cap, 32), dtype=np.uint8), counts=counts,
                midx=rng.integers(0, cap, (n - 1, cap, 2)).astype(np.int32), mdist=rng.integers(0, 257, (n - 1, cap, 2)).astype(np.int32),
                mpass=rng.integers(0, 2, (n - 1, cap)).astype(np.uint8), pose=pose, pts=pts, npts=rng.integers(0, cap, n - 1).astype(np.int32))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_of_a_default_batch(tmp_path):
    o = _outputs(256)
    bench.dump_outputs(str(tmp_path), **o)
    got = _load(str(tmp_path))
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= bench.DUMP_MAX_BYTES == 64 * 10 ** 6
    assert np.array_equal(got["frames"], np.arange(256)) and got["keypoints"].shape == (256, bench.CAP, 7)
    assert got["match_idx"].shape == (255, bench.CAP, 2) and got["pose"].shape == (255, 12)
    c = int(o["counts"][0])
    k = min(c, bench.CAP)
    assert np.array_equal(got["keypoints"][0, :k, :5], o["kps"][0, :k, :5])
    assert np.array_equal(got["keypoints"][0, :k, 5], o["kps"].view(np.int32)[0, :k, 5]) and (got["keypoints"][0, :k, 6] == -1).all()
    assert (got["keypoints"][0, k:] == 0).all() and (got["map_points"][0, k:] == 0).all() and (got["map_point_valid"][0, k:] == 0).all()
    has = ~np.isnan(o["pts"][0, :k, 0])
    assert np.array_equal(got["map_point_valid"][0, :k], has) and np.array_equal(got["map_points"][0, :k][has], o["pts"][0, :k][has])
    assert (got["map_points"][0, :k][~has] == 0).all()
    assert np.array_equal(got["pose_valid"], np.arange(255) != 1) and (got["pose"][1] == 0).all()
    assert np.array_equal(np.delete(got["pose"], 1, 0), np.delete(o["pose"], 1, 0))
    f = got["descriptor_frames"].astype(int)
    assert len(f) == bench.DUMP_DESC_FRAMES and np.array_equal(f, np.unique(f))
    kf = min(int(o["counts"][f[0]]), bench.CAP)
    assert np.array_equal(got["descriptors"][0, :kf], o["desc"][f[0], :kf])


def test_dump_samples_a_larger_batch_the_same_way_every_time(tmp_path):
    o = _outputs(300, seed=1)
    bench.dump_outputs(str(tmp_path / "a"), **o)
    bench.dump_outputs(str(tmp_path / "b"), **o)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert len(a["frames"]) == bench.DUMP_FRAMES and a.keys() == b.keys()
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    fr = a["frames"].astype(int)
    assert np.array_equal(a["keypoint_counts"], o["counts"][fr]) and len(a["pose"]) == (fr < 299).sum()
