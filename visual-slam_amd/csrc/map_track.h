// map_track.h -- the one tracker that mo_map_track, mo_map_track_covisible, mo_map_track_frustum (map_track.hip) and mo_map_track_batch
// (map_track_batch.hip) run: its types, the frame view its single-workgroup stages index by, the candidate tail of the three search
// kernels, and the host front.  The stage kernels (k_trk_init, k_trk_grid, k_trk_compact, k_trk_refine) and the host front are defined
// in map_track.hip; a call over one frame is the launch with one workgroup.  Private to the library.
#pragma once
#include "map_search.h"

#define TK_MAX_PASS 4

struct TrackPrm {
    double K[9], radius[TK_MAX_PASS], sf, ratio, chi2;
    int w, h, max_dist, min_matches;
};

struct TrackRes {                         // per frame
    double pose[12];                      // projection pose of the next pass: pose0, then each refined pose
    double pass_pose[TK_MAX_PASS][12];
    double pass_radius[TK_MAX_PASS];
    int32_t pass_cand[TK_MAX_PASS], pass_matches[TK_MAX_PASS], pass_inliers[TK_MAX_PASS];
    int32_t n_local, n_run, n_done;       // points of the local map (a batch counts them once, in its TbHead), passes searched, passes refined
    int32_t ended, retry;                 // the frame has ended (no keypoints; too few matches after the retry); the pass in flight is retried
    int32_t cand, n_match;                // candidates of the attempt in flight (the search), matches of the last compaction
};

struct TrkMatch {                         // one match in keypoint order (32 B): the point's position, the keypoint
    float X, Y, Z, x, y;
    int32_t octave, q, p;
};

struct TrkPose { double v[12]; };         // one predicted pose, by value

// Where frame f's arrays are: rows f * stride .. of every [frame][stride] array, cnt[f] of them in use, grid f of cell, result block f.
// One frame: the spare keyframe slot's rows, stride m->row, cnt = kcnt + spare.  By value to the kernels.
struct TrkFrames {
    const mo_keypoint* fk; const uint8_t* fdesc;   // [frame][stride], [frame][stride][32]
    const int32_t* cnt;                   // [frame]
    const double* pose0;                  // [frame][12] on the device; NULL: one frame, its pose a launch argument
    int stride;
    int32_t *cell, *sorted;               // [frame][TK_CELLS + 1], [frame][stride]
    unsigned long long* key;              // [frame][stride] and so on
    TrkMatch* match; uint8_t* minl;
    int32_t *qpt, *qdist; uint8_t* qinl;
    TrackRes* res;                        // [frame]
    __device__ __forceinline__ size_t at(int f) const { return (size_t)f * stride; }
    __device__ __forceinline__ int n(int f) const { return min(cnt[f], stride); }
    __device__ __forceinline__ const int32_t* cells(int f) const { return cell + (size_t)f * (TK_CELLS + 1); }
};
// the view over a feature's scratch (TrackBufs, TrackBatchBufs: the same member names)
template <class B> TrkFrames trk_frames(B& b, const mo_keypoint* fk, const uint8_t* fdesc, const int32_t* cnt, const double* pose0, int stride) {
    return TrkFrames{fk, fdesc, cnt, pose0, stride, b.cell, b.sorted, b.key, b.match, b.minl, b.qpt, b.qdist, b.qinl, b.res};
}

// a pass's kernels run when the frame has not ended and, for the second attempt, when the first asked for it
__device__ __forceinline__ bool trk_active(const TrackRes* res, int attempt) {
    return !res->ended && (attempt == 0 || res->retry);
}

// The tail of every search: candidate point i (descriptor rep + 32 i) against the keypoints its window walk visits - walk(visit) is
// trk_window or trk_window_oct with the candidate's pixel, radius and octaves bound - the best and second distance, the max_dist and
// ratio gates, and the claim on the best keypoint by a 64-bit atomicMin of (dist << 32) | point.
// trk_claim_as: the same tail for a candidate whose descriptor d is not its point's representative (mo_map_track_reference: a keyframe
// row claims for the point i it observes); returns the keypoint claimed, its distance in *dist, or -1 with *dist = -1.
template <class Walk> __device__ __forceinline__ int trk_claim_as(const TrackPrm& prm, int i, const uint8_t* __restrict__ d, const uint8_t* __restrict__ fdesc,
                                                                  unsigned long long* __restrict__ key, Walk walk, int* dist) {
    int bd = INT_MAX, bq = INT_MAX, sd = INT_MAX;
    *dist = -1;
    walk([&](int q, const mo_keypoint&, double, double) {
        const int dist = trk_ham(d, fdesc + (size_t)q * 32), was = bd;
        if (trk_take(dist, q, bd, bq)) sd = was;
        else if (dist < sd) sd = dist;
    });
    if (bd == INT_MAX || bd > prm.max_dist) return -1;
    if (sd != INT_MAX && !((double)bd <= prm.ratio * (double)sd)) return -1;
    atomicMin(key + bq, ((unsigned long long)(unsigned)bd << 32) | (unsigned)i);
    *dist = bd;
    return bq;
}
template <class Walk> __device__ __forceinline__ void trk_claim(const TrackPrm& prm, int i, const uint8_t* __restrict__ rep, const uint8_t* __restrict__ fdesc,
                                                                unsigned long long* __restrict__ key, Walk walk) {
    int dist;
    trk_claim_as(prm, i, rep + (size_t)i * 32, fdesc, key, walk, &dist);
}

// ---- the single-workgroup stages, one workgroup per frame of fr (map_track.hip), enqueued on the context stream -----------------------
// k_trk_init: result blocks (pose from fr.pose0, or `one`), keys, per-keypoint outputs; a frame without keypoints starts ended;
// *n_local (the counter k_trk_rep adds to) zeroed
int trk_launch_init(mo_ctx* c, const TrkFrames& fr, int n_frames, const double* one, int32_t* n_local);
// k_trk_compact of (pass, attempt); k_trk_refine of pass
int trk_launch_compact(mo_ctx* c, const TrackPrm& p, const TrkFrames& fr, int n_frames, int pass, int attempt, const float* xyz);
int trk_launch_refine(mo_ctx* c, const TrackPrm& p, const TrkFrames& fr, int n_frames, int pass);

// ---- the host front ------------------------------------------------------------------------------------------------------------------
// the parameter rules of every tracking call; pose0 [n_pose][12]
int track_check(mo_ctx* c, const mo_map_track_params* prm, const double* pose0, size_t n_pose);
TrackPrm track_prm(const double K[9], const mo_map_track_params* prm);
// one frame's destinations in the caller's outputs (mo_map_track_out, or row i of mo_map_track_batch_out); point, dist, inlier may be NULL
struct TrackDst {
    int32_t *point, *dist; uint8_t* inlier;
    double *pose, *pass_pose, *pass_radius;          // [12], [TK_MAX_PASS][12], [TK_MAX_PASS]
    int32_t *pass_cand, *pass_matches, *pass_inliers, *n_pass_run, *ok;
};
// what a frame reports when no pass runs: pose0, no pass, not ok; and its n per-keypoint rows: no match
void track_defaults(const TrackDst& d, const double* pose0);
void track_row_defaults(const TrackDst& d, int n);
// a frame's result block into its destinations; returns ok: the last pass finished with >= min_inliers inliers
int track_result(const TrackDst& d, const TrackRes& r, const mo_map_track_params* prm);
