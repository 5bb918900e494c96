// map_search.h -- what the searches by projection on the device map share: mo_map_track (map_track.hip, a frame against the local map)
// and mo_map_fuse (map_fuse.hip, the local map against its own keyframes).  The local map with its representative descriptors
// (k_trk_rep) and the keypoint grid (k_trk_grid) are defined in map_track.hip and launched through the functions at the end.  Inline
// here, the one projected-window search: trk_project (projection and image test), trk_scale (radius per octave), trk_window (cell range,
// cell walk, box and octave gates, a visitor per keypoint that passes), trk_ham (256-bit distance), trk_take (the (dist, q) tie rule;
// map_grow.hip's epipolar search takes its best row by it too).  Private to the library.
#pragma once
#include <climits>

#include "common.h"
#include "map_store.h"

#define TK_GX 64                        // ORB-SLAM2's FRAME_GRID_COLS x FRAME_GRID_ROWS
#define TK_GY 48
#define TK_CELLS (TK_GX * TK_GY)
#define TK_NOT_LOCAL INT_MIN            // octave slot of a point outside the local map
#define TK_NONE 0xffffffffffffffffull   // keypoint key without a claim

__device__ __forceinline__ int trk_ham(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b) {
    const uint4 a0 = *(const uint4*)a, a1 = *(const uint4*)(a + 16), b0 = *(const uint4*)b, b1 = *(const uint4*)(b + 16);
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) +
           __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// grid column / row of a coordinate: monotone in it, so the cells of [u - r, u + r] hold every keypoint with |x - u| < r
__device__ __forceinline__ int trk_cx(double x, int w) {
    const double v = x * TK_GX / w;
    return v >= 0.0 ? (v < TK_GX ? (int)v : TK_GX - 1) : 0;
}
__device__ __forceinline__ int trk_cy(double y, int h) {
    const double v = y * TK_GY / h;
    return v >= 0.0 ? (v < TK_GY ? (int)v : TK_GY - 1) : 0;
}

// scale_factor^o as repeated products from 1.0 (negative octaves as 0); the information of an octave is ba.h's ba_info
__device__ __forceinline__ double trk_scale(double sf, int o) {
    double s = 1.0;
    for (int i = 0; i < o; i++) s *= sf;
    return s;
}

// The pixel of (X, Y, Z) under the 3 x 4 projection P: true in front of the camera and inside the w x h image.  Each row is summed left
// to right, then the two divisions: the order tests/track_restatement.py and tests/fuse_restatement.py round in (-ffp-contract=off).
__device__ __forceinline__ bool trk_project(const double* P, double X, double Y, double Z, int w, int h, double* u, double* v) {
    const double x = P[0] * X + P[1] * Y + P[2] * Z + P[3];
    const double y = P[4] * X + P[5] * Y + P[6] * Z + P[7];
    const double z = P[8] * X + P[9] * Y + P[10] * Z + P[11];
    if (!(z > 0.0)) return false;
    *u = x / z; *v = y / z;
    return *u >= 0.0 && *u < w && *v >= 0.0 && *v < h;
}

// The keypoints fk of one grid (cell, sorted: k_trk_grid's) in the window of radius r around (u, v): those with |dx| < r and |dy| < r whose
// octave is within 1 of ro, cell by cell in sorted order.  visit(q, keypoint, dx, dy) for each.
template <class V> __device__ __forceinline__ void trk_window(double u, double v, double r, int ro, int w, int h, const int32_t* __restrict__ cell,
                                                              const int32_t* __restrict__ sorted, const mo_keypoint* __restrict__ fk, V visit) {
    const int cx0 = trk_cx(u - r, w), cx1 = trk_cx(u + r, w), cy0 = trk_cy(v - r, h), cy1 = trk_cy(v + r, h);
    for (int cy = cy0; cy <= cy1; cy++)
        for (int cx = cx0; cx <= cx1; cx++) {
            const int c = cy * TK_GX + cx, e1 = cell[c + 1];
            for (int e = cell[c]; e < e1; e++) {
                const int q = sorted[e];
                const mo_keypoint kp = fk[q];
                const double dx = (double)kp.x - u, dy = (double)kp.y - v;
                if (!(fabs(dx) < r && fabs(dy) < r)) continue;
                const long long dl = (long long)kp.octave - ro;
                if (dl < -1 || dl > 1) continue;
                visit(q, kp, dx, dy);
            }
        }
}

// the best match so far (bd, bq) against (dist, q): the lower distance, ties to the lower keypoint; true when (dist, q) took its place
__device__ __forceinline__ bool trk_take(int dist, int q, int& bd, int& bq) {
    if (!(dist < bd || (dist == bd && q < bq))) return false;
    bd = dist; bq = q;
    return true;
}

// k_trk_rep on the live map (the position table uploaded by the caller): rep [point][32], oct [point] (TK_NOT_LOCAL outside the
// local map of the positions >= lo_pos), *n_local += the local points (zeroed by the caller)
int trk_launch_rep(mo_map* m, int lo_pos, uint8_t* rep, int32_t* oct, int32_t* n_local);
// the same with the local map of a keyframe set: lmask [n_kf] on the device, non-zero at a local keyframe (map_covis.hip's selection)
int trk_launch_rep_mask(mo_map* m, const uint8_t* lmask, uint8_t* rep, int32_t* oct, int32_t* n_local);
// k_trk_grid, one block per grid: block b sorts the keypoints of keyframe slot (slots ? slots[b] : slot0) - kcnt[slot] rows at
// kkps + slot * row - into cell [b][TK_CELLS + 1] and sorted [b][row]
int trk_launch_grid(mo_map* m, const int32_t* slots, int slot0, int n_grids, int w, int h, int32_t* cell, int32_t* sorted);
