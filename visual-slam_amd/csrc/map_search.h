// map_search.h -- what the searches by projection on the device map share: the tracker (map_track.h: mo_map_track and its covisible,
// frustum and batch forms), mo_map_fuse (map_fuse.hip, the local map against its own keyframes), and the searches of map_confirm.hip and
// map_correct.hip.  The local map with its representative descriptors (k_trk_rep) and the keypoint grid (k_trk_grid) are defined in
// map_track.hip and launched through the functions at the end.  Inline here, the one projected-window search: trk_project (projection and
// image test), trk_scale (radius per octave), trk_window (cell range, cell walk, box and octave gates, a visitor per keypoint that passes),
// trk_ham (256-bit distance), trk_take (the (dist, q) tie rule; map_grow.hip's epipolar search takes its best row by it too).  The frustum
// mode of the searches (mo_map_track_frustum, mo_map_fuse_frustum) adds trk_window_oct (the window with an octave interval), ViewRec /
// trk_frustum (the view record of a point, the distance and angle tests, the predicted level) and trk_centre; the records come from
// map_view_geom.hip through view_enqueue.  Private to the library.
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

// trk_window with the octave gate lo <= octave <= hi in place of ro +- 1 (the frustum mode: [L - 1, L]).  Two walks still: trk_window as
// trk_window_oct over [ro - 1, ro + 1] keeps every occupancy but moves the searches of fusion and correction (k_merge_search of
// map_merge.h since), k_cf_guided and k_cf_proj by 4 - 10 instructions and k_tb_search from 74 to 76 VGPRs
// (profiles/track_unify_isa.txt); the run times of those searches were not measured.
template <class V> __device__ __forceinline__ void trk_window_oct(double u, double v, double r, int lo, int hi, int w, int h,
                                                                  const int32_t* __restrict__ cell, const int32_t* __restrict__ sorted,
                                                                  const mo_keypoint* __restrict__ fk, V visit) {
    const int cx0 = trk_cx(u - r, w), cx1 = trk_cx(u + r, w), cy0 = trk_cy(v - r, h), cy1 = trk_cy(v + r, h);
    for (int cy = cy0; cy <= cy1; cy++)
        for (int cx = cx0; cx <= cx1; cx++) {
            const int c = cy * TK_GX + cx, e1 = cell[c + 1];
            for (int e = cell[c]; e < e1; e++) {
                const int q = sorted[e];
                const mo_keypoint kp = fk[q];
                const double dx = (double)kp.x - u, dy = (double)kp.y - v;
                if (!(fabs(dx) < r && fabs(dy) < r)) continue;
                if (kp.octave < lo || kp.octave > hi) continue;
                visit(q, kp, dx, dy);
            }
        }
}

// ---- the frustum mode (mo_map_point_views, mo_map_track_frustum, mo_map_fuse_frustum in include/vslam_amd.h) ---------------------------
// the view record of a point: its mean viewing direction (not renormalised) and max_dist, one 16-byte load per search lane
struct __attribute__((aligned(16))) ViewRec { float nx, ny, nz, max_dist; };
// what the frustum test takes besides the point and the camera: mo_map_frustum_params and the scale factor of the search
struct FrustumPrm {
    double sf, range_lo, range_hi, min_cos;
    int n_levels;
};

// the camera centre -R^T t of a pose
__device__ __forceinline__ void trk_centre(const double* R, const double* t, double* C) {
    for (int j = 0; j < 3; j++) C[j] = -(R[j] * t[0] + R[3 + j] * t[1] + R[6 + j] * t[2]);
}

// Frame::isInFrustum's distance and angle tests and PredictScale for the point (X, Y, Z) with record rc seen from the centre C: false
// when the point is not searched, else *L = the smallest level >= 0 with dist * sf^L >= max_dist, capped at n_levels - 1.  Sums left to
// right; a centre that is not a number (a keyframe without one) fails the first test.
__device__ __forceinline__ bool trk_frustum(const FrustumPrm& f, const ViewRec& rc, const double* C, double X, double Y, double Z, int* L) {
    const double px = X - C[0], py = Y - C[1], pz = Z - C[2];
    const double dist = sqrt(px * px + py * py + pz * pz);
    const double mx = (double)rc.max_dist;
    if (!(dist > 0.0) || !(mx > 0.0)) return false;
    const double mn = mx / trk_scale(f.sf, f.n_levels - 1);
    if (dist < f.range_lo * mn || dist > f.range_hi * mx) return false;
    if (px * (double)rc.nx + py * (double)rc.ny + pz * (double)rc.nz < f.min_cos * dist) return false;
    double s = 1.0;
    int l = 0;
    while (l < f.n_levels - 1 && dist * s < mx) { s *= f.sf; l++; }
    *L = l;
    return true;
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
// k_trk_grid, one block per grid: block b sorts the keypoints of row s = (slots ? slots[b] : slot0 + b) of kps [.][row] - cnt[s] of
// them - into cell [b][TK_CELLS + 1] and sorted [b][row].  The second form: kps, row and cnt are the keyframe store's, s a keyframe slot.
int trk_launch_grid(mo_ctx* c, const mo_keypoint* kps, int row, const int32_t* cnt, const int32_t* slots, int slot0, int n_grids, int w, int h,
                    int32_t* cell, int32_t* sorted);
inline int trk_launch_grid(mo_map* m, const int32_t* slots, int slot0, int n_grids, int w, int h, int32_t* cell, int32_t* sorted) {
    return trk_launch_grid(m->c, m->kkps, m->row, m->kcnt, slots, slot0, n_grids, w, h, cell, sorted);
}
// map_view_geom.hip: k_view_centres and k_view_points on the live map (the position table uploaded by the caller), enqueued: *centre
// [n_kf][3] by keyframe position (NaN: no centre) and *rec [point] for the points with oct[point] != TK_NOT_LOCAL (oct NULL: every
// point), in the scratch of the view feature; both valid for the kernels enqueued behind on the context stream
int view_enqueue(mo_map* m, const int32_t* oct, double sf, const ViewRec** rec, const double** centre);
