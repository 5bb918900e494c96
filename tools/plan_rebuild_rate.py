#!/usr/bin/env python3
"""Wall time of one plan rebuild: the first orb_detect_compute at another image size on a warm context (work buffers freed and
allocated, the plan's tables built and uploaded, one extraction), alternating between two sizes; median and minimum in ms per size.
For A/B runs of two builds of the library (VSLAM_AMD_LIB): python tools/plan_rebuild_rate.py [repetitions per size, default 20]."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-slam_amd")); sys.path.insert(0, ROOT)
import numpy as np
import vslam_amd as V
from tests.helpers import synthetic_frame

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
sizes = [(640, 480), (480, 360)]
imgs = [synthetic_frame(20250523 + i, w, h) for i, (w, h) in enumerate(sizes)]
ctx = V.Context(max_w=640, max_h=480, max_batch=1)
prm = V.orb_params(nfeatures=2000)
for _ in range(3):
    for img in imgs:
        ctx.orb_detect_compute(img, prm)
ms = np.empty((n, 2))
for i in range(n):
    for j, img in enumerate(imgs):
        t = time.perf_counter(); ctx.orb_detect_compute(img, prm); ms[i, j] = (time.perf_counter() - t) * 1e3
for j, (w, h) in enumerate(sizes):
    print("plan_rebuild %4dx%-4d wall median %7.3f min %7.3f ms (%d rebuilds)" % (w, h, np.median(ms[:, j]), ms[:, j].min(), n), flush=True)
ctx.close()
