// map_reloc.h -- the one relocalization that mo_map_relocalize, mo_map_relocalize_pre (map_reloc.hip) and mo_map_relocalize_batch
// (map_reloc_batch.hip) run: its result block, the frame view its kernels index by, the launchers of its stages and the host front.
// The kernels are defined in map_reloc.hip; a call over one frame is the launch with one frame.  Private to the library.
#pragma once
#include "common.h"
#include "map_store.h"

#define RL_MAX_CAND 64
#define RL_MIN_SCORE 15   // ORB-SLAM2's Tracking::Relocalization: keyframes with fewer than 15 matches are discarded

struct RelocRes {                         // per frame
    double pose[RL_MAX_CAND][12];         // refined [R | t] per candidate
    unsigned long long best[RL_MAX_CAND]; // (inliers << 32) | ~(h * 4 + root): the largest key is the best hypothesis
    int32_t cand[RL_MAX_CAND], score[RL_MAX_CAND], ncorr[RL_MAX_CAND], ninl[RL_MAX_CAND];
    int32_t n_cand, win;
};

struct RelocGeom {
    double K[9], Kinv[9], thr2;
};

// Where frame f of a launch is: its keypoints fk + f * stride (cnt[f] of them), its result block res[f], its per-keypoint outputs
// qpt / qinl + f * stride, its scores score + f * n_kf and the C_k of its candidate c at ((f * nc + c) * stride) of cq / cinl and, as
// packed records {X, Y, Z, x, y} (the point's position, the keypoint), five times that of rec.  The matcher's pair of (frame, keyframe
// position k): without a preselection every keyframe was matched, keyframe-major (pair k * n_frames + f); with one, frame f's pairs are
// the slice f * pairs .. of the list and mrow[f][k] names the pair inside it (-1: not matched).
// One frame: the spare keyframe slot's rows, stride m->row, cnt = kcnt + spare.  By value to the kernels.
struct RlFrames {
    const mo_keypoint* fk; const int32_t* cnt;
    int stride, n_frames, n_kf, nc, pairs;
    const int32_t* mrow;                  // [frame][n_kf], NULL: no preselection
    int32_t* score;                       // [frame][n_kf]
    int32_t* cq; float* rec; uint8_t* cinl;   // [frame][nc][stride] (rec: [5] each)
    int32_t* qpt; uint8_t* qinl;          // [frame][stride]
    RelocRes* res;                        // [frame]
    __device__ __forceinline__ int n(int f) const { return min(cnt[f], stride); }
    __device__ __forceinline__ int match_row(int f, int k) const {
        if (!mrow) return k * n_frames + f;
        const int r = mrow[(size_t)f * n_kf + k];
        return r < 0 ? -1 : f * pairs + r;
    }
    __device__ __forceinline__ size_t ck(int f, int c) const { return ((size_t)f * nc + c) * stride; }
};

// ---- the stages, enqueued on the context stream (map_reloc.hip) ----------------------------------------------------------------------
// |C_k| of every (frame, keyframe), the ranking (one workgroup per frame: result blocks reset, candidates chosen) and C_k of every
// (frame, candidate) in query order, as query rows and as packed records
int reloc_launch_candidates(mo_ctx* c, const RlFrames& fr, const MatchView& mv, const float* xyz);
// P3P hypotheses scored against the records of their candidate; then, per (frame, candidate), the best hypothesis refined; then, per
// frame, the winner and its per-keypoint outputs.  Stage marks p3p / refine by the names given.
int reloc_launch_poses(mo_ctx* c, const RlFrames& fr, const MatchView& mv, const RelocGeom& g, int n_hyp, uint64_t seed, const char* mark_p3p,
                       const char* mark_refine);

// ---- the host front ------------------------------------------------------------------------------------------------------------------
// the parameter rules of every relocalization call, and the camera as the kernels take it
int reloc_check(mo_ctx* c, const double K[9], const mo_map_reloc_params* prm, RelocGeom* g);
// one frame's destinations in the caller's outputs (mo_map_reloc_out, or row i of mo_map_reloc_batch_out); point, inlier and the
// candidate arrays may be NULL
struct RelocDst {
    int32_t* point; uint8_t* inlier;
    int32_t *cand_pos, *cand_score, *cand_inliers;   // [max_candidates]
    double* pose;                                    // [12]
    int32_t *ok, *kf_pos, *n_cand, *n_corr, *n_inliers;
};
// what a frame reports when nothing ran for it (NaN pose, no candidate), its n per-keypoint rows included
void reloc_defaults(const RelocDst& d, int n, int max_candidates);
// a frame's downloaded result block into its destinations; returns ok
int reloc_result(const RelocDst& d, const RelocRes& r, const mo_map_reloc_params* prm);
