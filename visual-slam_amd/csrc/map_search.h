// map_search.h -- what the searches by projection on the device map share: mo_map_track (map_track.hip, a frame against the local map)
// and mo_map_fuse (map_fuse.hip, the local map against its own keyframes).  The local map with its representative descriptors
// (k_trk_rep) and the keypoint grid (k_trk_grid) are defined in map_track.hip and launched through the two functions below; the
// device helpers of the cell walk are inline here.  Private to the library.
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

// k_trk_rep on the map in `src` (the position table uploaded by the caller): rep [point][32], oct [point] (TK_NOT_LOCAL outside the
// local map of the positions >= lo_pos), *n_local += the local points (zeroed by the caller)
int trk_launch_rep(mo_map* m, const MapPts& src, int lo_pos, uint8_t* rep, int32_t* oct, int32_t* n_local);
// the same with the local map of a keyframe set: lmask [n_kf] on the device, non-zero at a local keyframe (map_covis.hip's selection)
int trk_launch_rep_mask(mo_map* m, const MapPts& src, const uint8_t* lmask, uint8_t* rep, int32_t* oct, int32_t* n_local);
// k_trk_grid, one block per grid: block b sorts the keypoints of keyframe slot (slots ? slots[b] : slot0) - kcnt[slot] rows at
// kkps + slot * row - into cell [b][TK_CELLS + 1] and sorted [b][row]
int trk_launch_grid(mo_map* m, const int32_t* slots, int slot0, int n_grids, int w, int h, int32_t* cell, int32_t* sorted);
