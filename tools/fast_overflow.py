#!/usr/bin/env python3
"""tools/fast_overflow.py [frames] -- CPU count of the pixels with a non-zero FAST score in the scored band ((strip_rows + 2) x (bw + 2))
of every 8-row k_fast strip of the bench scene (survey8d, threshold 7, 8 levels, edge 31), per level, against the 896-entry corner list
the kernel kept before.  The pyramid is the oracle's (bit-identical to the GPU's), the score is the FAST arc network on raw pixels."""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "visual-slam_amd"))
from oracle import orb_oracle as O
from vslam_amd import synth
nfr = int(sys.argv[1]) if len(sys.argv) > 1 else 16
fr = synth.make_frames(torch, "cpu", 0, nfr, scene="survey8d", seed=20250523).numpy()
prm = O.params(nfeatures=2000, scale_factor=1.2, nlevels=8, edge_threshold=31, fast_threshold=7)
t = 7; R = 8; et = 31
CIRC = [(0,3),(1,3),(2,2),(3,1),(3,0),(3,-1),(2,-2),(1,-3),(0,-3),(-1,-3),(-2,-2),(-3,-1),(-3,0),(-3,1),(-2,2),(-1,3)]
def corners(img):
    img = img.astype(np.int16); h, w = img.shape
    v = img[3:h-3, 3:w-3]
    p = np.stack([img[3+dy:h-3+dy, 3+dx:w-3+dx] for dx, dy in CIRC])
    q = np.concatenate([p, p[:8]])
    mx = np.min(np.stack([q[i:i+9].max(0) for i in range(16)]), 0)
    mn = np.max(np.stack([q[i:i+9].min(0) for i in range(16)]), 0)
    L = np.maximum(v - mx, mn - v)
    out = np.zeros((h, w), bool); out[3:h-3, 3:w-3] = L > t
    return out
stats = {}
for f in range(nfr):
    for L in range(8):
        img = O.pyramid_level(fr[f], prm, L)
        h, w = img.shape
        c = corners(img)
        bw, bh = w - 2*et, h - 2*et
        if bw <= 0 or bh <= 0: continue
        ns = (bh + R - 1) // R
        for s in range(ns):
            y0 = et + s*R; rows = min(R, et + bh - y0)
            n = c[y0-1:y0+rows+1, et-1:et+bw+1].sum()
            st = stats.setdefault(L, [0, 0, 0, 0, (w, h)])
            st[0] += 1; st[1] += n > 896; st[2] = max(st[2], n); st[3] += n
for L, (n, o, mx, tot, wh) in sorted(stats.items()):
    print(f"level {L} {wh}: strips {n} overflow(>896) {o} ({100*o/n:.0f} %) max {mx} mean {tot/n:.0f}")
