#!/usr/bin/env python3
"""Wall time and the C call's own clock (mo_host_times; init_two_view keeps none: its column repeats the call before it) of the
single-frame host calls, many calls each: median and minimum in us.
For A/B runs of two builds of the library (VSLAM_AMD_LIB), where bench.py's single_frame_ms legs (medians of 10 - 20 calls) are too
coarse: python tools/single_call_rate.py [calls per leg, default 2000]."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-slam_amd")); sys.path.insert(0, ROOT)
import numpy as np
import vslam_amd as V
from tests.helpers import synthetic_frame

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
W, H = 640, 480
K = np.array([[320.0, 0, 320.0], [0, 320.0, 240.0], [0, 0, 1.0]])
a = synthetic_frame(20250523)
rng = np.random.Generator(np.random.PCG64(7))
b = np.clip(np.roll(a, 3, axis=1).astype(np.float32) + rng.normal(0, 2.0, a.shape), 0, 255).round().astype(np.uint8)
ctx = V.Context(max_w=4095, max_h=4095, max_batch=1)
prm = V.orb_params(nfeatures=2000)
(k0, d0), = ctx.orb_detect_compute(a, prm)
(k1, d1), = ctx.orb_detect_compute(b, prm)
assert V.resident_token(ctx, d0, k0) and V.resident_token(ctx, d1, k1)
s = np.random.default_rng(3)
p1 = s.uniform(50, 590, (600, 2)).astype(np.float32); p2 = p1 + s.normal(0, 1, p1.shape).astype(np.float32)
legs = [("match_resident", lambda: ctx.match_knn2_ratio(d0, d1, 0.75)),
        ("track_pair_resident", lambda: ctx.track_pair(k0, d0, k1, d1, W, H, K)),
        ("pair_init_resident", lambda: ctx.pair_frontend(k0, d0, k1, d1, V.MODE_INIT, K)),
        ("init_two_view_600", lambda: ctx.init_two_view(p1, p2, K, n_hyp=1024)),
        ("grid_detect_compute", lambda: ctx.grid_detect_compute(a, prm, 2000))]
for name, fn in legs:
    for _ in range(50):
        fn()
    wall, call = np.empty(n), np.empty(n)
    for i in range(n):
        t = time.perf_counter(); fn(); wall[i] = (time.perf_counter() - t) * 1e6
        call[i] = ctx.host_times()["total_us"]
    print("%-22s wall median %8.2f min %8.2f | C call median %8.2f min %8.2f us (%d calls)" % (name, np.median(wall), wall.min(), np.median(call), call.min(), n), flush=True)
# (last: every call makes a new resident result, which ends the residency of k0 / k1)
fn = lambda: ctx.orb_detect_compute(a, prm)
for _ in range(50):
    fn()
wall, call = np.empty(n), np.empty(n)
for i in range(n):
    t = time.perf_counter(); fn(); wall[i] = (time.perf_counter() - t) * 1e6
    call[i] = ctx.host_times()["total_us"]
print("%-22s wall median %8.2f min %8.2f | C call median %8.2f min %8.2f us (%d calls)" % ("orb_detect_compute", np.median(wall), wall.min(), np.median(call), call.min(), n), flush=True)
ctx.close()
