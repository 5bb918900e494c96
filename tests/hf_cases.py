"""TEST INFRASTRUCTURE ONLY: the scenes of the homography / fundamental model-selection tests (tests/test_hf_cpu.py on the restatement,
tests/test_gpu_hf.py on the device).  Every scene comes from the oracle's synthetic_two_view, so nothing is committed as data.
K = 320 / 320 / 320 / 240 unless a case says otherwise; distances are in baselines (|t| = 1)."""
import functools

import numpy as np

from oracle import geom_oracle as G

N_HYP, N_HYP_H, SEED = 1024, 512, 4096   # hypotheses of the essential / homography side, sampling seed of every call
TILTED = (0.3, 0.2, 1.0, 8.0, 0.0)       # exact plane n . X = 8 of camera 1, tilted against the image plane
FRONTO = (0.0, 0.0, 1.0, 8.0, 0.0)
_NOISY = dict(noise_px=0.5, outlier_frac=0.3)
_LONG_K = ((3000.0, 0, 1920.0), (0, 3000.0, 1080.0), (0, 0, 1.0))
_ROT30 = tuple(np.radians(30.0) * np.array([0.3, 0.2, 1.0]) / np.linalg.norm([0.3, 0.2, 1.0]))

# name -> (keyword arguments of synthetic_two_view, expectation): "H" = a plane (model H, accepted, pose near the truth),
# "F" = a general scene (model F), "reject" = not accepted (pure rotation), None = value parity only
CASES = {}
for _s in (1, 2, 3, 4, 5, 4096):
    CASES["plane_s%d" % _s] = (dict(seed=_s, n=360, depth=(0, 0), plane=TILTED, **_NOISY), "H")
CASES["plane_clean"] = (dict(seed=4096, n=360, depth=(0, 0), plane=TILTED, outlier_frac=0.0), "H")
CASES["fronto"] = (dict(seed=4096, n=400, depth=(0, 0), plane=FRONTO, t_dir=(1.0, 0.0, 0.0), **_NOISY), "H")
CASES["fronto_s2"] = (dict(seed=2, n=300, depth=(0, 0), plane=FRONTO, t_dir=(1.0, 0.0, 0.0), **_NOISY), "H")
CASES["general"] = (dict(seed=4096, n=360, depth=(4, 12), **_NOISY), "F")
CASES["sideways"] = (dict(seed=4096, n=400, **_NOISY), "F")
CASES["forward"] = (dict(seed=4096, n=360, depth=(4, 12), t_dir=(0.0, 0.0, -1.0), **_NOISY), "F")
CASES["rot30"] = (dict(seed=4096, n=360, depth=(4, 12), rv=_ROT30, **_NOISY), "F")
# a camera that only rotates, for every purpose: the scene is 4000 - 12000 baselines away
CASES["pure_rotation"] = (dict(seed=4096, n=360, depth=(4000, 12000), rv=(0.03, -0.08, 0.02), **_NOISY), "reject")
CASES["pure_rotation_s3"] = (dict(seed=3, n=300, depth=(4000, 12000), rv=(0.03, -0.08, 0.02), **_NOISY), "reject")
# RH and the parallax are both borderline here: value parity only
CASES["low_parallax"] = (dict(seed=4096, n=360, K=((80.0, 0, 160.0), (0, 80.0, 120.0), (0, 0, 1.0)), w=320, h=240, depth=(25, 45),
                              rv=(0.002, -0.005, 0.001), **_NOISY), None)
# edge shapes
CASES["plane_m8"] = (dict(seed=4096, n=8, depth=(0, 0), plane=TILTED, outlier_frac=0.0), None)
CASES["plane_m9"] = (dict(seed=4096, n=9, depth=(0, 0), plane=TILTED, outlier_frac=0.0), None)
CASES["plane_m40"] = (dict(seed=4096, n=40, depth=(0, 0), plane=TILTED, outlier_frac=0.0), None)
CASES["plane_m4097"] = (dict(seed=4096, n=4097, depth=(0, 0), plane=TILTED, **_NOISY), "H")
CASES["plane_long_f"] = (dict(seed=4096, n=360, K=_LONG_K, w=3840, h=2160, depth=(0, 0), plane=TILTED, **_NOISY), "H")

DECISION = [k for k, (_, e) in CASES.items() if e is not None]


@functools.lru_cache(maxsize=None)
def scene(name):
    kw = dict(CASES[name][0])
    if "K" in kw:
        kw["K"] = np.array(kw["K"], np.float64)
    return G.synthetic_two_view(**kw)


def line_scene(m=200, seed=7):
    """every point on one image row in both images (exactly: the rows are float32 integers), so every 4-sample is collinear"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(20, 620, m)
    p1 = np.stack([x, np.full(m, 100.0)], axis=1).astype(np.float32)
    p2 = np.stack([x + rng.uniform(5, 9, m), np.full(m, 120.0)], axis=1).astype(np.float32)
    return dict(K=np.array([[320.0, 0, 320.0], [0, 320.0, 240.0], [0, 0, 1.0]]), p1=p1, p2=p2)


@functools.lru_cache(maxsize=None)
def essential(name):
    s = scene(name)
    return G.init_two_view(s["p1"], s["p2"], s["K"], 3.0, N_HYP, SEED)


# arguments of the call that differ from the defaults above.  m = 8 and m = 9 have 70 and 126 distinct 4-samples: 512 hypotheses
# would repeat them many times over with costs that differ in the last bits only, so these two cases draw 12
CALL_KW = {"plane_m8": dict(n_hyp_h=12), "plane_m9": dict(n_hyp_h=12)}


def call_kw(name, **kw):
    """keyword arguments of Context.init_two_view_hf / hf_restatement.hf_two_view for a case"""
    args = dict(thr_px=3.0, n_hyp=N_HYP, seed=SEED, n_hyp_h=N_HYP_H)
    args.update(CALL_KW.get(name, {}))
    args.update(kw)
    return args


@functools.lru_cache(maxsize=None)
def restated(name, solver="svd", **kw):
    """the restatement's result on a case (computed once per process and shared; callers do not modify it)"""
    from tests import hf_restatement as HR
    s = scene(name)
    return HR.hf_two_view(s["p1"], s["p2"], s["K"], solver=solver, essential=essential(name), **call_kw(name, **kw))


def rel_err(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / max(np.linalg.norm(b), 1e-300))
