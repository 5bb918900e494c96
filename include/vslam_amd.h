/* vslam_amd.h -- C-ABI of the MI355X-native ORB front-end (libvslam_amd.so).
 *
 * Drop-in boundary for ONE hot path of p2004dr/visual-slam: extract -> match -> two-view
 * initialisation.  The reference has no FFI layer; its boundary is the Python class API that
 * Tracker calls.  Each entry point below replaces the cv2 call(s) behind one reference method
 * (file:line relative to the reference tree) and is bound by the ctypes host classes in
 * visual-slam_amd/orbslam2/ which keep the reference's constructors and method signatures.
 *
 * Conventions: plain C, opaque context, caller-allocated outputs, int status (0 = MO_OK, <0 = error,
 * text via mo_last_error), no exceptions cross the boundary, no torch types.  One context is
 * thread-compatible (one caller at a time), like the single-threaded reference.
 * "host" entry points take host pointers and do the H2D/D2H themselves; "mo_dev_*" entry points take
 * DEVICE pointers (inputs already resident in HBM) and enqueue on the context's stream without
 * synchronising, for the batched / multi-GPU mode and the benchmark.  Exceptions, both one-off: the call that first sees a new
 * (image size, ORB parameters, batch) combination builds its plan and work buffers (hipMalloc, blocking table uploads).
 */
#ifndef VSLAM_AMD_H
#define VSLAM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The structs below (mo_orb_params, mo_batch_io, mo_frame_ref, mo_pair_params, mo_pair_out, mo_stream_params, mo_stream_result) carry no size
 * field: their layout belongs to the header a caller was compiled against.  mo_batch_io gets fields APPENDED per round, so a caller built
 * against an older header hands in a shorter struct than the library reads: every caller must be recompiled with the header of the library
 * it loads, and can check that at load time: mo_abi_version() == MO_ABI_VERSION. */
#define MO_ABI_VERSION 7
int mo_abi_version(void);

#define MO_OK 0
#define MO_ERR_ARG (-1)       /* bad argument */
#define MO_ERR_HIP (-2)       /* HIP runtime error (see mo_last_error) */
#define MO_ERR_CAPACITY (-3)  /* caller buffer or internal capacity too small */
#define MO_ERR_UNSUPPORTED (-4)
#define MO_ERR_INDEX (-5)     /* a map point names a keyframe or keypoint that does not exist (Python's IndexError) */

#define MO_ORDER_LIBSTDCXX 0 /* retainBest order of cv2 wheels linked against libstdc++ (Linux) */
#define MO_ORDER_MSVC 1      /* retainBest order of cv2 wheels linked against the MSVC STL (Windows);
                                the order of the reference's gt.yaml fixtures */

typedef struct mo_ctx mo_ctx;

/* same fields as cv2.KeyPoint: pt, size, angle, response, octave, class_id (28 bytes) */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} mo_keypoint;

/* cv2.ORB_create arguments as the reference passes them (src/orbslam2/extractor.py:38-48).
 * Only the values the reference uses are implemented: edge_threshold any >= 19 (31 in the reference),
 * first_level 0, wta_k 2, score_type 0 (HARRIS), patch_size 31. */
typedef struct {
    int32_t nfeatures;      /* extractor.py:39 */
    float scale_factor;     /* extractor.py:40 */
    int32_t nlevels;        /* extractor.py:41, 1..12 */
    int32_t edge_threshold; /* extractor.py:42 */
    int32_t first_level;    /* extractor.py:43 */
    int32_t wta_k;          /* extractor.py:44 */
    int32_t score_type;     /* extractor.py:45, 0 = HARRIS_SCORE */
    int32_t patch_size;     /* extractor.py:46 */
    int32_t fast_threshold; /* extractor.py:47 (= min_threshold) */
    int32_t select_order;   /* MO_ORDER_*: which STL's nth_element permutation to reproduce */
} mo_orb_params;

/* ---- context ------------------------------------------------------------------------------ */
mo_ctx* mo_create(int device, int max_w, int max_h, int max_batch);
void mo_destroy(mo_ctx*);
const char* mo_last_error(mo_ctx*); /* valid until the next call on ctx; ctx may be NULL (creation errors) */
int mo_set_stream(mo_ctx*, void* hip_stream); /* NULL = the context's own (non-blocking) stream */
int mo_set_stream_null(mo_ctx*);              /* the HIP null stream (handle 0, e.g. torch's default stream): mo_set_stream cannot name it */
int mo_sync(mo_ctx*);                         /* hipStreamSynchronize on the context stream */
int mo_device_count(void);                    /* hipGetDeviceCount, 0 when there is no GPU */

/* ---- ORBExtractor ----------------------------------------------------------------------- */
/* Replaces cv2.cvtColor + orb.detectAndCompute(image, None)   (extractor.py:61-65, detect_and_compute).
 * img: batch images, u8, ch = 1 (gray) or 3 (BGR), row stride in bytes, images packed at stride*h.
 * kps [batch*cap], desc [batch*cap*32] (may be NULL = detect only), counts [batch].
 * Returns MO_ERR_CAPACITY if a frame yields more than cap keypoints (counts then holds the needs). */
int mo_orb_detect_compute(mo_ctx*, const mo_orb_params*, const uint8_t* img, int w, int h, int stride, int ch,
                          int batch, mo_keypoint* kps, uint8_t* desc, int cap, int* counts);

/* Replaces orb.compute(image, keypoints)   (extractor.py:79-83 compute, :140 distribute_keypoints).
 * Keeps cv2's behaviour: keypoints within edge_threshold of the image border are dropped, kp.angle is
 * used as supplied (no re-orientation), kp.octave selects the level.  kept_idx[i] = index into kps_in
 * of descriptor row i; n_out = number of rows. */
int mo_orb_compute(mo_ctx*, const mo_orb_params*, const uint8_t* img, int w, int h, int stride, int ch,
                   const mo_keypoint* kps_in, int n_in, int32_t* kept_idx, uint8_t* desc, int* n_out);

/* Replaces the 64 cv2.goodFeaturesToTrack(image, maxCorners = n_features // 64, qualityLevel 0.01, minDistance 10,
 * mask = grid cell) calls of ORBExtractor.distribute_keypoints (extractor.py:104-136): 8x8 grid, Shi-Tomasi minimum
 * eigenvalue (blockSize 3, Sobel 3), corners in cell-major order, best first inside a cell.
 * xy [64 * (n_features / 64)][2] pixel coordinates; n_out = number of corners.  Descriptors for them come from
 * mo_orb_compute with angle -1 (extractor.py:135,140). */
int mo_orb_grid_good_features(mo_ctx*, const uint8_t* img, int w, int h, int stride, int ch, int n_features, float* xy,
                              int* n_out);
/* ORBExtractor.distribute_keypoints in ONE call (reference extractor.py:85-144, the path Tracker takes by default, tracker.py:87): the
 * grid corners as above, KeyPoint(x, y, 31) for each of them, orb.compute on that list.  xy [64 * (n_features / 64)][2] and n_xy as in
 * mo_orb_grid_good_features; kept_idx [n_kept] = indices into xy of the corners cv2's compute keeps (rounded position at least
 * edge_threshold inside the image), desc [n_kept][32] their descriptors (angle -1, octave 0).  One image upload and one
 * synchronisation instead of two each for the pair mo_orb_grid_good_features + mo_orb_compute; identical results. */
int mo_orb_grid_detect_compute(mo_ctx*, const mo_orb_params*, const uint8_t* img, int w, int h, int stride, int ch, int n_features,
                               float* xy, int* n_xy, int32_t* kept_idx, uint8_t* desc, int* n_kept);

/* Replaces cv2.undistort(image, camera_matrix, distortion)   (utils.py:40-52, applied by run_video.py:145-149 when a distortion
 * coefficient is non-zero): initUndistortRectifyMap (new camera matrix = K, 1/32-pixel fixed-point map) + remap(INTER_LINEAR,
 * constant 0 border).  img / out: h x w x ch u8 (ch 1 or 3), rows at `stride` bytes (out is dense: w * ch); dist = k1, k2, p1, p2, k3.
 * mo_dev_undistort: batch of dense frames already in HBM, enqueued on the context stream (run it ahead of
 * mo_dev_orb_detect_compute / mo_dev_frontend_batch on the same stream). */
int mo_undistort(mo_ctx*, const uint8_t* img, int w, int h, int stride, int ch, const double K[9], const double dist[5], uint8_t* out);
int mo_dev_undistort(mo_ctx*, const uint8_t* d_src, int w, int h, int ch, int batch, const double K[9], const double dist[5],
                     uint8_t* d_dst);

/* ---- DescriptorMatcher ------------------------------------------------------------------- */
/* Replaces BFMatcher(NORM_HAMMING).knnMatch(d1, d2, k=2) + the Lowe ratio loop (matcher.py:70,73-81).
 * q [batch][nq][32], t [batch][nt][32]; ratio NULL = no ratio test (ratio_test=False).
 * train_idx/dist [batch][nq][2] (missing neighbour: idx -1, dist INT32_MAX), pass [batch][nq]. */
int mo_match_knn2_ratio(mo_ctx*, const uint8_t* q, int nq, const uint8_t* t, int nt, const double* ratio,
                        int batch, int32_t* train_idx, int32_t* dist, uint8_t* pass);

/* ---- MapInitializer ---------------------------------------------------------------------- */
/* Replaces calculate_essential_matrix + recover_pose + triangulate_points + the cheirality loop
 * (initializer.py:79-120; utils.py:56-70,120-160).  8-point essential-matrix RANSAC over n_hyp
 * hypotheses scored in parallel, least-squares refit on the consensus set, recoverPose-style
 * cheirality vote (depth in (0, 50)), DLT triangulation.
 * p1,p2 [m][2] pixel coordinates; K row-major 3x3; thr_px Sampson threshold in pixels; prob is
 * accepted for signature compatibility (all n_hyp hypotheses are always scored).
 * Outputs: R [9] row-major, t [3] unit norm, E [9] (may be NULL), inlier [m] = pose mask (RANSAC inlier
 * AND cheirality of the winning pose), X [m][3] triangulated points (valid where inlier), n_good. */
int mo_init_two_view(mo_ctx*, const float* p1, const float* p2, int m, const double K[9], double thr_px,
                     double prob, int n_hyp, uint64_t seed, double R[9], double t[3], double E[9],
                     uint8_t* ransac_inlier /* [m] findEssentialMat mask, may be NULL */, uint8_t* inlier, float* X,
                     int* n_good);

/* Two-view initialisation with ORB-SLAM2's model selection (Initializer.cc: FindHomography / FindFundamental, CheckHomography /
 * CheckFundamental, RH = SH / (SH + SF), ReconstructH with CheckRT); the reference has no counterpart - its initializer knows the
 * essential matrix only and reports a wrong pose as success on a plane or under pure rotation.  The call runs the unchanged
 * essential chain of mo_init_two_view and, on the same stream, the homography chain: n_hyp_h four-point hypotheses in closed
 * form (the first four indices of the essential path's sampling stream), MSAC ranking on the symmetric transfer error truncated at
 * 5.991 sigma^2, at most 5 DLT refits on the inliers, SH, SF = CheckFundamental of K^-T E K^-1 for the essential path's E,
 * Faugeras' eight (R, t, n) candidates, CheckRT of each over the H inliers (reprojection within 4 sigma^2, parallax = the value at
 * index min(50, count - 1) of the ascending cos values).  One synchronisation.
 * model = 1 (H) when RH > rh_threshold, else 0 (F); -1 when m < 8 or the essential path found no model (everything NaN / 0).
 * Selected outputs (R, t, pose_mask, X, n_good) are the chosen model's: for model 0 the bytes mo_init_two_view returns for the same
 * arguments, accepted = n_good > min_triangulated; for model 1 the best candidate's, accepted = second < 0.75 best && parallax >=
 * min_parallax_deg && best > min_triangulated && best > 0.9 H inliers (n_good counts every point that passed CheckRT, pose_mask
 * and X hold those of them with cos(parallax) < 0.99998, as ORB-SLAM2's vbTriangulated). */
typedef struct {
    double thr_px;           /* essential path: Sampson threshold in pixels (3.0) */
    int32_t n_hyp;           /* essential path: hypotheses (4096) */
    int32_t n_hyp_h;         /* homography hypotheses (512) */
    uint64_t seed;           /* both sampling streams (4096) */
    double sigma;            /* pixel noise of CheckHomography / CheckFundamental / CheckRT (1.0) */
    double rh_threshold;     /* 0.40 */
    double min_parallax_deg; /* 1.0 */
    int32_t min_triangulated; /* 50 */
    int32_t reserved;
} mo_hf_params;

typedef struct {
    /* caller-allocated arrays, all required */
    uint8_t* pose_mask;      /* [m] selected model */
    float* X;                /* [m][3] selected model, NaN outside pose_mask */
    uint8_t* ransac_mask;    /* [m] essential path: Sampson inliers */
    uint8_t* h_mask;         /* [m] homography: both transfer directions inside the threshold */
    /* filled by the call */
    int32_t model, accepted, n_good, n_good_e;
    double R[9], t[3];       /* selected model; t unit norm */
    double E[9], R_e[9], t_e[3];  /* essential path (mo_init_two_view's E, R, t; n_good_e) */
    double H[9];             /* pixels, unit Frobenius norm; NaN: no homography model */
    double SH, SF, RH;
    double parallax_h[8];    /* degrees; 0 for a candidate without a passed point */
    int32_t n_good_h[8];
    int32_t best_h, second_h;  /* candidate indices, -1: none */
    int32_t n_inliers_h, accepted_h, winner_h /* winning hypothesis, -1: no model */, refits_h;
    double R_h[9], t_h[3];   /* best candidate (NaN: none) */
} mo_hf_result;

int mo_init_two_view_hf(mo_ctx*, const float* p1, const float* p2, int m, const double K[9], const mo_hf_params* params,
                        mo_hf_result* out);

/* Replaces cv2.recoverPose(E, p1, p2, K, mask)   (utils.py:129-134) for ANY essential matrix the caller holds: decomposition
 * (U W V^T, U W^T V^T, +-u3), cheirality vote over the four candidates on the points selected by mask_in (NULL = all; depth in
 * (0, 50) in both cameras, as cv2), winner's R, t, its mask, and the DLT points of the surviving correspondences.
 * p1, p2 [m][2] pixels, K row-major; mask_out [m]; X [m][3] (may be NULL; NaN where mask_out is 0); n_good. */
int mo_recover_pose(mo_ctx*, const double E[9], const float* p1, const float* p2, int m, const double K[9],
                    const uint8_t* mask_in, double R[9], double t[3], uint8_t* mask_out, float* X, int* n_good);

/* Replaces cv2.findFundamentalMat(points1, points2, cv2.FM_RANSAC, thr_px, prob)   (matcher.py:191 filter_matches_by_fundamental,
 * local_mapper.py:136 keyframe map growth).  Same machinery as mo_init_two_view with the fundamental-matrix model: n_hyp
 * 8-point hypotheses on Hartley-normalised pixel coordinates, rank-2 projection, MSAC ranking on the Sampson distance in pixels,
 * least-squares refit on the consensus set.  (cv2's FM_RANSAC draws 7-point samples; like the 8-point essential RANSAC this
 * is the parallel-hypothesis formulation north_star prescribes - parity is on the inlier set and the epipolar geometry.)
 * p1, p2 [m][2] pixels; F [9] row-major scaled to F[8] = 1 (NaN when m < 8 or no model is found); mask [m]; n_inliers. */
int mo_find_fundamental(mo_ctx*, const float* p1, const float* p2, int m, double thr_px, double prob, int n_hyp, uint64_t seed,
                        double F[9], uint8_t* mask, int* n_inliers);

/* One tracking step of Tracker._track_from_last_frame (tracker.py:214-254) for a single frame pair, host in / host out:
 * matcher.match(prev, cur) -> displacement filter (matcher.py:109-142, frac = 0.02 of (w + h) / 2) -> 2 x median distance
 * filter (matcher.py:144-169) -> cv2.findEssentialMat(RANSAC, 0.999, thr_px = 1.0) -> cv2.recoverPose, all on the device.
 * kps1/desc1 = previous frame (query), kps2/desc2 = current frame (train); a negative ratio disables the ratio test.
 * sel_idx [min(n1, 4096)][2] (queryIdx, trainIdx) and sel_dist receive the kept matches in the reference's order (ascending
 * distance, ties in query order), n_sel their number; inlier [n_sel] the recoverPose mask per kept match.  With fewer than 8
 * kept matches (tracker.py:234) R, t, E are NaN and n_inliers = 0. */
int mo_track_pair(mo_ctx*, const mo_keypoint* kps1, int n1, const uint8_t* desc1, const mo_keypoint* kps2, int n2,
                  const uint8_t* desc2, int w, int h, double ratio, double disp_frac, const double K[9], double thr_px,
                  int n_hyp, uint64_t seed, double R[9], double t[3], double E[9], int32_t* sel_idx, int32_t* sel_dist,
                  int* n_sel, uint8_t* inlier, int* n_inliers);

/* ---- one frame at a time: resident results and the fused pair step -------------------------------------------------------------
 * The reference's Tracker calls the classes once per frame (tracker.py:87 extract_features, then :168-170 initialize or :214-254
 * _track_from_last_frame against the PREVIOUS frame's keypoints and descriptors; tests/tester_map.py:57-75 is that loop).  A
 * single-frame mo_orb_detect_compute (batch == 1, desc != NULL) therefore leaves its keypoints and descriptors RESIDENT on the device
 * (the context keeps the last 4 such results) and mo_last_token names them; mo_pair_frontend runs matcher -> (tracking filters) ->
 * two-view stage on two frames given by token - nothing is uploaded - or by host arrays (uploaded into a slot; out->token1 / token2
 * then name them for the next call).  One call, one synchronisation:
 *   MO_MODE_INIT   MapInitializer.initialize's device work (initializer.py:67-120): matcher.match(d1, d2) with `ratio`, essential matrix at
 *                  thr_px (the reference passes 3.0) on the ratio-test survivors in query order, recoverPose, triangulation
 *   MO_MODE_TRACK  Tracker._track_from_last_frame (tracker.py:214-254): match, displacement filter (disp_frac of (w + h) / 2), 2 x median
 *                  distance filter, essential matrix at thr_px (1.0) + recoverPose on the kept matches in the reference's order
 * n_hyp = 0 stops after the matcher (and the filters).  A token that is no longer resident falls back to the arrays; MO_ERR_ARG when
 * there are none. */
typedef struct {
    uint64_t token;          /* 0 = none */
    const mo_keypoint* kps;  /* [n] host, may be NULL while the token is alive */
    const uint8_t* desc;     /* [n][32] host */
    int32_t n;
} mo_frame_ref;

typedef struct {
    int32_t mode;            /* MO_MODE_INIT or MO_MODE_TRACK */
    int32_t w, h;            /* image size (MO_MODE_TRACK: the displacement gate) */
    double ratio;            /* Lowe ratio; negative = no ratio test */
    double disp_frac;        /* MO_MODE_TRACK: threshold_percent (tracker.py:219: 0.02) */
    double K[9];
    double thr_px;
    int32_t n_hyp;           /* 0 = matcher (+ filters) only */
    uint64_t seed;
    uint64_t pair_index;     /* global index of this pair in a sequence: the sampling stream is a function of (seed, pair_index), so a
                                per-frame loop that counts its pairs gets the poses of the batched mode bit for bit; 0 = stand-alone pair */
} mo_pair_params;

typedef struct {
    /* caller-allocated arrays; n1 = keypoints of frame 1; any of them may be NULL */
    int32_t* match_idx;      /* [n1][2] knn train indices (missing neighbour: -1) */
    int32_t* match_dist;     /* [n1][2] */
    uint8_t* match_pass;     /* [n1] ratio test */
    int32_t* sel_idx;        /* MO_MODE_TRACK: [n1][2] (queryIdx, trainIdx) of the kept matches, ascending distance */
    int32_t* sel_dist;       /* MO_MODE_TRACK: [n1] */
    uint8_t* inlier;         /* MO_MODE_TRACK: [n_sel] recoverPose mask per kept match; MO_MODE_INIT: [n1] pose mask per QUERY keypoint */
    uint8_t* ransac;         /* MO_MODE_INIT: [n1] findEssentialMat mask per query keypoint */
    float* X;                /* MO_MODE_INIT: [n1][3] map point per query keypoint (NaN = none) */
    /* filled by the call */
    double R[9], t[3], E[9]; /* NaN without a model (MO_MODE_TRACK: fewer than 8 kept matches, tracker.py:234) */
    int32_t n_sel;           /* MO_MODE_TRACK: kept matches */
    int32_t n_good;          /* recoverPose inliers */
    int32_t n1, n2;          /* keypoints of the two frames */
    uint64_t token1, token2; /* tokens under which the two frames are resident now */
} mo_pair_out;

int mo_last_token(mo_ctx*, uint64_t* token); /* token of the last single-frame mo_orb_detect_compute with descriptors (0: none) */
int mo_pair_frontend(mo_ctx*, const mo_frame_ref* f1, const mo_frame_ref* f2, const mo_pair_params*, mo_pair_out*);

/* Replaces cv2.triangulatePoints(P1, P2, pts1, pts2)   (utils.py:56-60): per-point 4x4 DLT null vector.
 * P1, P2 row-major 3x4 f64; p1, p2 [n][2] f32; X4 [n][4] f32 homogeneous (unit norm, sign arbitrary -
 * the reference divides by w, utils.py:62-70). */
int mo_triangulate_points(mo_ctx*, const double P1[12], const double P2[12], const float* p1, const float* p2, int n,
                          float* X4);

/* ---- device-resident batched mode (frames independent; shards across GPUs by frame) -------- */
typedef struct {
    /* inputs */
    const uint8_t* d_gray;  /* [batch][h][w] u8, device */
    int32_t w, h, batch;
    int32_t cap;            /* keypoint capacity per frame */
    double ratio;           /* Lowe ratio; a NEGATIVE value disables the test (0.0 is a threshold: nothing with two neighbours passes) */
    double K[9];            /* intrinsics for the two-view stage */
    double thr_px;          /* RANSAC threshold (initializer.py:79 passes 3.0) */
    int32_t n_hyp;          /* hypotheses per pair, 0 = skip the two-view stage */
    uint64_t seed;
    /* outputs, all device pointers */
    mo_keypoint* d_kps;     /* [batch][cap] */
    uint8_t* d_desc;        /* [batch][cap][32] */
    int32_t* d_counts;      /* [batch] */
    int32_t* d_match_idx;   /* [batch-1][cap][2]  pair i = frame i (query) vs frame i+1 (train) */
    int32_t* d_match_dist;  /* [batch-1][cap][2] */
    uint8_t* d_match_pass;  /* [batch-1][cap] */
    double* d_pose;         /* [batch-1][12] R (9) then t (3); may be NULL when n_hyp == 0 */
    float* d_points;        /* [batch-1][cap][3] triangulated points per query keypoint (NaN = none) */
    int32_t* d_n_points;    /* [batch-1] number of valid map points per pair */
    /* ---- appended in round 2 (zero-initialise the struct: all of these are optional) ---- */
    int32_t mode;           /* MO_MODE_INIT (0): two-view stage on the ratio-test survivors in query order (MapInitializer.initialize);
                               MO_MODE_TRACK (1): Tracker._track_from_last_frame (tracker.py:214-254) - displacement filter
                               (matcher.py:109-142) and 2 x median distance filter (matcher.py:144-169) behind the matcher, then the
                               two-view stage on the kept matches in the reference's order (tracker.py:242 passes thr_px = 1.0) */
    double disp_frac;       /* MO_MODE_TRACK: threshold_percent of filter_matches_by_geometric_distance (tracker.py:219: 0.02) */
    int32_t* d_sel_idx;     /* MO_MODE_TRACK: [batch-1][cap][2] (queryIdx, trainIdx) of the kept matches, ascending distance */
    int32_t* d_sel_dist;    /* MO_MODE_TRACK: [batch-1][cap] their Hamming distances; may be NULL */
    int32_t* d_sel_n;       /* MO_MODE_TRACK: [batch-1] number of kept matches */
    uint8_t* d_pose_mask;   /* either mode, may be NULL: [batch-1][cap] recoverPose mask per QUERY keypoint */
    uint64_t pair_index_base; /* global index of this batch's pair 0 when a longer sequence is sharded over calls / ranks: the
                               RANSAC sampling stream of a pair is a function of (seed, global pair index), so the result
                               of a pair does not depend on how the sequence was cut */
    /* ---- appended in round 3 (optional, zero = rounds 1 - 2 behaviour) ---- */
    int32_t detector;       /* MO_DETECT_ORB (0): ORBExtractor.detect_and_compute per frame (FAST / pyramid; extractor.py:50-67);
                               MO_DETECT_GRID (1): ORBExtractor.distribute_keypoints per frame (extractor.py:85-144, what Tracker.process_frame
                               calls through extract_features(frame), tracker.py:87): 8x8 grid of Shi-Tomasi corners, params->nfeatures / 64
                               per cell, KeyPoint(x, y, 31) records, orb.compute at angle -1 on octave 0.  d_kps / d_desc / d_counts then
                               hold the keypoints orb.compute KEEPS (record i = descriptor row i); the reference's own misaligned list
                               (all corners) is available below */
    float* d_grid_xy;       /* MO_DETECT_GRID, may be NULL: [batch][64 * (nfeatures / 64)][2] every grid corner, slot (cell, rank) */
    int32_t* d_grid_n;      /* MO_DETECT_GRID, may be NULL: [batch][66] corners per cell (64), corners in all cells, keypoints kept */
    int32_t* d_grid_kept;   /* MO_DETECT_GRID, may be NULL: [batch][cap] index of keypoint i in the frame's cell-major corner list */
    /* MO_MODE_KEYFRAME (2): LocalMapper._process_new_keyframe (local_mapper.py:116-149) for n_kf_pairs keyframe pairs at once.  The batch's
     * frames are extracted as usual; pair p matches frame d_kf_query[p] (query, the previous keyframe) against frame d_kf_train[p]
     * (train, the new keyframe) with `ratio` (the reference passes 0.8) keeping only queries with two neighbours, runs the
     * fundamental-matrix RANSAC at thr_px (3.0) on the kept matches and triangulates the inliers with the two keyframes' projection
     * matrices K [R|t] (utils.compute_projection_matrix).  Outputs per PAIR (rows = n_kf_pairs instead of batch - 1): d_match_* ,
     * d_points [pair][cap][3] by query keypoint (NaN = no map point), d_n_points [pair] = F-RANSAC inliers, d_pose_mask [pair][cap],
     * d_kf_F [pair][9] (may be NULL; NaN with fewer than 8 matches or no model: the reference returns early in both cases). */
    int32_t n_kf_pairs;
    const int32_t* d_kf_query;  /* [n_kf_pairs] frame index of the query keyframe, 0 <= index < batch (not checked: device data) */
    const int32_t* d_kf_train;  /* [n_kf_pairs] frame index of the train keyframe */
    const double* d_kf_P1;      /* [n_kf_pairs][12] row-major 3x4 projection matrix of the query keyframe */
    const double* d_kf_P2;      /* [n_kf_pairs][12] ... of the train keyframe */
    double* d_kf_F;             /* [n_kf_pairs][9] */
} mo_batch_io;

#define MO_MODE_INIT 0
#define MO_MODE_TRACK 1
#define MO_MODE_KEYFRAME 2
#define MO_DETECT_ORB 0
#define MO_DETECT_GRID 1

/* One pass of the hot path over a batch: extract every frame, match consecutive frames, two-view pose +
 * map points per pair.  Enqueues on the context stream; call mo_sync (or sync the stream) before reading. */
int mo_dev_frontend_batch(mo_ctx*, const mo_orb_params*, const mo_batch_io*);
int mo_dev_orb_detect_compute(mo_ctx*, const mo_orb_params*, const uint8_t* d_gray, int w, int h, int batch,
                              mo_keypoint* d_kps, uint8_t* d_desc, int cap, int32_t* d_counts);
/* pairs: q/t frame indices into d_desc [*][cap][32] with per-frame counts d_counts */
/* ratio < 0 disables the ratio test */
int mo_dev_match_pairs(mo_ctx*, const uint8_t* d_desc, const int32_t* d_counts, int cap, const int32_t* d_qf,
                       const int32_t* d_tf, int n_pairs, double ratio, int32_t* d_idx, int32_t* d_dist,
                       uint8_t* d_pass);

/* ---- a frame SEQUENCE through the batched mode (stream.hip) ---------------------------------------------------------------------
 * The reference's driver hands frames over one at a time (src/tests/tester_map.py:57-75 -> Tracker.process_frame, tracker.py:73-146).
 * A caller that can look a few frames ahead gets the batched mode's rate from host frames: mo_stream cuts the sequence into chunks, runs
 * every chunk as ONE mo_dev_frontend_batch call on chunk + 1 frames (the previous chunk's last frame is staged again in front, so every
 * consecutive pair of the sequence is matched exactly once) and overlaps the upload of chunk i + 1 and the caller's handling of chunk
 * i - 1 with the compute of chunk i (three lanes of pinned / device buffers, an upload and a download stream beside the context's stream).  The sampling
 * stream of a pair is keyed by its global index: poses equal those of a per-frame loop that passes mo_pair_params.pair_index.
 *   mo_stream_submit   n <= chunk host frames (u8, rows of `stride` bytes, frames `frame_stride` bytes apart; 0 = dense): staged by a few
 *                      host threads, uploaded and enqueued; returns without waiting.  At most three chunks may be in flight.
 *   mo_stream_collect  waits for the OLDEST chunk in flight and describes its results: pointers into the lane's pinned host buffer,
 *                      valid until the third submit after the chunk's own.  MO_ERR_CAPACITY when a capacity flag was raised inside the
 *                      chunk (r->flags, bits as in mo_dev_status; the results are still described). */
typedef struct {
    int32_t w, h, ch;          /* frames: u8, ch = 1 (gray) or 3 (BGR, converted on the device) */
    int32_t chunk;             /* frames per batched call; the context needs max_batch >= chunk + 1 */
    int32_t cap;               /* keypoint rows per frame */
    int32_t detector;          /* MO_DETECT_ORB or MO_DETECT_GRID */
    int32_t mode;              /* MO_MODE_TRACK (tracker.py:214-254 on every consecutive pair) or MO_MODE_INIT (initializer.py:67-120) */
    double ratio, disp_frac, K[9], thr_px;
    int32_t n_hyp;
    uint64_t seed;
    uint64_t pair_index_base;  /* global index of the sequence's first pair */
    int32_t want_matches;      /* MO_MODE_TRACK: also return the knn lists (MO_MODE_INIT always does) */
    int32_t want_points;       /* return the map points */
} mo_stream_params;

typedef struct {
    int32_t n_frames, n_pairs;     /* frames of this chunk; pairs = n_frames - 1 for the first chunk, n_frames afterwards */
    uint64_t first_frame;          /* global index of frame row 0 */
    uint64_t first_pair;           /* global index of pair row 0: pair g = (frame g, frame g + 1) */
    int32_t cap, flags;
    int32_t prev_count;            /* keypoints of the frame in front of this chunk (the query frame of pair row 0 when first_pair < first_frame) */
    const int32_t* counts;         /* [n_frames] */
    const mo_keypoint* kps;        /* [n_frames][cap] */
    const uint8_t* desc;           /* [n_frames][cap][32] */
    const int32_t* sel_idx;        /* MO_MODE_TRACK: [n_pairs][cap][2] (queryIdx, trainIdx), the reference's order */
    const int32_t* sel_dist;       /* [n_pairs][cap] */
    const int32_t* sel_n;          /* [n_pairs] */
    const double* pose;            /* [n_pairs][12] R then t (NaN: no model) */
    const uint8_t* pose_mask;      /* [n_pairs][cap] recoverPose mask per QUERY keypoint */
    const int32_t* n_points;       /* [n_pairs] */
    const int32_t* match_idx;      /* [n_pairs][cap][2] or NULL */
    const int32_t* match_dist;     /* [n_pairs][cap][2] or NULL */
    const uint8_t* match_pass;     /* [n_pairs][cap] or NULL */
    const float* points;           /* [n_pairs][cap][3] or NULL */
} mo_stream_result;

typedef struct mo_stream mo_stream;
mo_stream* mo_stream_create(mo_ctx*, const mo_orb_params*, const mo_stream_params*);  /* NULL on failure: mo_last_error(ctx) */
void mo_stream_destroy(mo_stream*);
int mo_stream_submit(mo_stream*, const uint8_t* frames, int n, int stride, size_t frame_stride);
int mo_stream_collect(mo_stream*, mo_stream_result*);
int mo_stream_lanes(void);  /* chunks a stream holds in flight: submit refuses one more before a collect; a collected chunk's result
                               buffer is reused by the mo_stream_lanes()-th submit after it */
const char* mo_stream_last_error(mo_stream*);

/* ---- multi-GPU: the final map-point gather (SURVEY.md 8b mo_gather_map_points, 8e) --------------------------------------
 * One process per GPU, each with its own context; frames are sharded contiguously and nothing is exchanged on the data path.
 * The only collective is this padded gather of the per-pair map points to `root` over RCCL (bound with dlopen at first use).
 *   mo_comm_unique_id : rank 0 creates the 128-byte id; the host program hands it to the other ranks (any channel)
 *   mo_comm_init      : ncclCommInitRank on the context's device; mo_comm_destroy (also done by mo_destroy)
 *   mo_gather_map_points: d_local [rows_max][cap][3] f32 of this rank (rows_local valid rows), d_all on root
 *                       [world][rows_max][cap][3], d_rows_all [world] int32 on every rank; device pointers, enqueued on the
 *                       context stream, no host synchronisation. */
int mo_comm_unique_id(uint8_t id[128]);
int mo_comm_init(mo_ctx*, const uint8_t id[128], int rank, int world);
int mo_comm_destroy(mo_ctx*);
int mo_gather_map_points(mo_ctx*, const float* d_local, int rows_local, int rows_max, int cap, int root, float* d_all,
                         int32_t* d_rows_all);

/* ---- LocalMapper (local_mapper.py): a device-resident keyframe store and map (map_kernels.hip) ------------------------------------
 * Keyframes and map points live on the device; the host keeps the reference's dicts around them (vslam_amd/mapper.py).
 *   mo_map_add_keyframe      LocalMapper.add_keyframe (local_mapper.py:46-77) in one call, one synchronisation: the frame (by token of a
 *                            resident result slot, else the host arrays) and its P = K [R|t] (row-major 3x4, computed by the caller like
 *                            utils.compute_projection_matrix) go into the keyframe store; with two keyframes or more, the previous keyframe
 *                            (query) is matched against this one (train) with `ratio` keeping queries with two neighbours, the fundamental
 *                            matrix RANSAC runs at thr_px with the sampling stream (seed, pair_index) and its inliers, triangulated, are
 *                            appended in query order (position X / w, colour of the previous keyframe's image at (int(x), int(y)) - gray
 *                            [v, v, v], 3 channels as stored, outside [0, 0, 255] - observations {prev: queryIdx, new: trainIdx}, id =
 *                            map size before the point).  From the second keyframe on, every map point is then culled (fewer than 2 observations, or the first
 *                            observation in insertion order whose reprojection error with the P of keyframe POSITION kf_id exceeds 5 px),
 *                            the survivors are compacted in order and the per-keyframe lists rebuilt.  kf_len / kf_redundant [n_kf] receive
 *                            each list's length and the entries _cull_keyframes counts as redundant (local_mapper.py:270-285).
 *                            MO_ERR_INDEX when an observation names a keyframe position or keypoint that does not exist (the map then
 *                            holds the grown points, uncompacted).
 *   mo_map_add_points        LocalMapper.update_map_points: n points appended as given (obs_off [n + 1] into obs_kf / obs_kp; ids >= 0;
 *                            dref_kf / dref_row = the descriptor reference, opaque to the library).
 *   mo_map_remove_keyframes  the removals _cull_keyframes decided: keyframe POSITIONS, renumbering the rest (observations keep stale ids).
 *   mo_map_sizes             out[0] keyframes, [1] map points, [2] observations, [3] rows of the per-keyframe lists, [4] reserved, [5] slots.
 *   mo_map_download          one field (MO_MAP_*), bytes = exactly its size.
 *   mo_map_write_ply         utils.create_point_cloud_ply (utils.py:72-118) of the points with >= min_obs observations, byte for byte:
 *                            floats as Python's repr of the double value, colours as stored.
 *   mo_format_floats         that float formatting alone, one value per line (no GPU).
 *   mo_map_fuse              duplicate map points merged, missing observations gained (the comment at its declaration below).
 *   mo_map_grow              new map points for the last keyframe from its neighbour keyframes (the comment at its declaration below).
 *   mo_map_loop_correct      a confirmed loop corrected: the asking side moved, re-posed and fused into the old side (the comment at its
 *                            declaration below).
 *   mo_map_pose_graph        the essential graph optimised behind such a correction: Sim(3) pose graph over the keyframes, the points
 *                            follow (the comment at its declaration below).
 *   mo_map_global_ba         global bundle adjustment behind that: all keyframes and points, matrix-free Schur conjugate gradient (the
 *                            comment at its declaration below).
 *   mo_map_kf_redundancy, mo_map_erase_keyframes, mo_map_cull_keyframes   ORB-SLAM2's KeyFrameCulling decided on the device, and a removal
 *                            that rewrites the observations (the comment at their declarations below).
 *   mo_map_query_keyframes, mo_map_relocalize_pre   place recognition over a binary vocabulary and relocalization against the keyframes
 *                            it selects (the comment above mo_vocab_train below).
 *   mo_map_relocalize        the absolute pose of a lost frame against the map as it stands (ORB-SLAM2's Tracking::Relocalization with
 *                            brute-force matching in place of the bag-of-words lookup); reads the map, never changes it.  The frame (by
 *                            token of a resident result slot, else the host arrays) is matched against every keyframe (query = the frame,
 *                            train = the keyframe's rows, knn-2 with `ratio` as in mo_map_add_keyframe).  point_of[k][row] = the lowest map
 *                            point whose observations hold (keyframe position k, row), read like the cull reads them (negative values count
 *                            from the end; entries naming a position or row that does not exist are skipped).  C_k = the ratio-test
 *                            survivors q whose best neighbour has a map point, in query order, |C_k| = the score; the candidates are the
 *                            keyframes with a score >= 15, highest first, ties to the lower position, at most max_candidates.  Per
 *                            candidate: n_hyp P3P samples of 3 correspondences (the sampling stream (seed, keyframe position, h) of
 *                            twoview_kernels.hip:sample8), up to 4 poses each; an inlier has depth > 0 and squared reprojection error
 *                            < thr_px^2 under P = K [R|t] (f64); the best pose has the most inliers (ties to the lower (h, root)), then
 *                            Gauss-Newton on SE(3) over its inliers (<= 10 steps), re-selection, once more.  The winner has the most final
 *                            inliers (ties to the lower position); ok = its inliers >= min_inliers.  One synchronisation: the copy-out. */
typedef struct mo_map mo_map;
typedef struct {
    double ratio;            /* 0.8 (local_mapper.py:124) */
    double thr_px;           /* 3.0 (local_mapper.py:136) */
    int32_t n_hyp;
    uint64_t seed;
    uint64_t pair_index;     /* sampling stream of this keyframe pair: the k-th pair of a run = MO_MODE_KEYFRAME's pair_index_base + k */
} mo_map_kf_params;
typedef struct {
    /* caller-allocated, may be NULL; n1 = keypoints of the previous keyframe */
    int32_t* match_idx;      /* [n1][2] knn train indices */
    uint8_t* match_pass;     /* [n1] ratio test */
    uint8_t* inlier;         /* [n1] F-RANSAC inlier per query keypoint */
    float* points;           /* [n1][3] triangulated inlier per query keypoint (NaN = none), before the cull */
    int32_t* kf_len;         /* [n_kf] per-keyframe list lengths after the call */
    int32_t* kf_redundant;   /* [n_kf] */
    /* filled by the call */
    double F[9];             /* NaN: no growth step or no model */
    int32_t n_new;           /* points the growth step appended */
    int32_t from_token;      /* 1: the keyframe was copied from its resident slot */
    int64_t n_points, n_obs; /* map size after the cull */
} mo_map_kf_out;
typedef struct {
    double ratio;            /* Lowe ratio of the keyframe matching (0.75) */
    double thr_px;           /* inlier: squared reprojection error < thr_px^2 (3.0) */
    int32_t min_inliers;     /* ok needs this many final inliers (50) */
    int32_t max_candidates;  /* 1 .. 64 (4) */
    int32_t n_hyp;           /* P3P samples per candidate, 1 .. 2^20 (512) */
    uint64_t seed;
} mo_map_reloc_params;
typedef struct {
    /* caller-allocated, may be NULL; n_q = keypoints of the frame */
    int32_t* point;          /* [n_q] map point of each query keypoint through the winner's point_of (-1: none) */
    uint8_t* inlier;         /* [n_q] final inlier flag of the winner */
    int32_t* cand_pos;       /* [max_candidates] keyframe positions of the candidates in rank order (-1 past n_cand) */
    int32_t* cand_score;     /* [max_candidates] their scores |C_k| */
    int32_t* cand_inliers;   /* [max_candidates] their final inlier counts */
    /* filled by the call */
    double pose[12];         /* [R | t] row-major of the winner (X_cam = R X + t); NaN without a winner */
    int32_t ok;              /* 1: the winner has >= min_inliers inliers */
    int32_t kf_pos;          /* keyframe position of the winner (-1: none) */
    int32_t n_cand;          /* candidates */
    int32_t n_corr;          /* |C_k| of the winner */
    int32_t n_inliers;       /* final inliers of the winner */
    int32_t from_token;      /* 1: the frame was read from its resident slot */
} mo_map_reloc_out;
#define MO_MAP_XYZ 0
#define MO_MAP_COLOR 1
#define MO_MAP_ID 2
#define MO_MAP_OBS_OFF 3
#define MO_MAP_OBS_KF 4
#define MO_MAP_OBS_KP 5
#define MO_MAP_DREF_KF 6
#define MO_MAP_DREF_ROW 7
#define MO_MAP_LIST_OFF 8
#define MO_MAP_LIST_IDS 9
mo_map* mo_map_create(mo_ctx*, int kf_slots, int kf_rows, int64_t pts_cap, int64_t obs_cap); /* initial capacities; NULL: mo_last_error(ctx) */
void mo_map_destroy(mo_map*);
int mo_map_add_keyframe(mo_map*, const mo_frame_ref* f, const double P[12], const uint8_t* img, int w, int h, int ch,
                        const mo_map_kf_params*, mo_map_kf_out*);
int mo_map_add_points(mo_map*, int n, const float* xyz, const uint8_t* col, const int32_t* id, const int32_t* obs_off, const int32_t* obs_kf,
                      const int32_t* obs_kp, const int32_t* dref_kf, const int32_t* dref_row);
int mo_map_remove_keyframes(mo_map*, const int32_t* positions, int n);
int mo_map_sizes(mo_map*, int64_t out[6]);
int mo_map_download(mo_map*, int field, void* dst, size_t bytes);
int mo_map_write_ply(mo_map*, const char* path, int min_obs, int64_t* n_written);
int mo_map_relocalize(mo_map*, const mo_frame_ref* f, const double K[9], const mo_map_reloc_params*, mo_map_reloc_out*);

/* mo_map_track: the pose of a tracked frame against the map as it stands, from a predicted pose (ORB-SLAM2's search by projection and
 * Optimizer::PoseOptimization, monocular, pose only); reads the map, never changes it.  The frame is given like mo_map_relocalize's.
 * pose0 = the predicted [R | t] row-major (X_cam = R X + t, the convention of mo_map_add_keyframe and mo_map_relocalize).
 *   observations  read like the cull reads them (negative keyframe positions and rows count from the end; entries naming a position or
 *                 row that does not exist are skipped).
 *   local map     the points with a valid observation in the last `window` keyframe positions (0: every position).
 *   descriptor    of a point: ComputeDistinctiveDescriptors over all its valid observations: per observation, its distances to all of
 *                 them (itself included) sorted, median = the element at (n - 1) / 2; the smallest median wins, ties to the earlier
 *                 observation in insertion order.  ref_octave = the octave of the winner's keypoint.
 *   candidates    local points whose projection under the pass pose (P = K [R | t], f64, each row summed left to right) has z > 0 and
 *                 u / z in [0, w), v / z in [0, h).
 *   search        r = pass radius * scale_factor^ref_octave (repeated products from 1.0); the frame keypoints with |x - u| < r,
 *                 |y - v| < r and |octave - ref_octave| <= 1; best = the lowest Hamming distance (ties to the lower keypoint), second =
 *                 the next lowest distance; accepted when best <= max_dist and, if a second exists, best <= ratio * second (double).
 *   conflicts     a keypoint goes to the point with the lowest distance, ties to the lower point index; the others stay unmatched.
 *   retry         a pass with fewer than min_matches matches runs once more at twice its radius; still fewer: the call ends (ok = 0).
 *   refinement    4 rounds of at most 10 Gauss-Newton steps on SE(3) over the round's inliers (all matches in round 0); a round stops at a
 *                 step below 1e-12 or a Hessian that is not positive definite.  Residual = projection - keypoint, information
 *                 1 / scale_factor^(2 octave) (octave of the frame keypoint, negative as 0), Huber width sqrt(chi2) in rounds 0 - 2, none
 *                 in round 3.  After each round every match is reclassified: inlier when z > 0 and information * |residual|^2 <= chi2;
 *                 fewer than 10 inliers end the refinement.
 *   passes        pass k + 1 projects from pass k's refined pose and searches from scratch.  ok = the last pass finished with
 *                 >= min_inliers inliers; pose = the refined pose of the last pass that finished, else pose0.
 * An empty frame, a map without keyframes or map points: no pass runs, not an error.  No host round trip inside the call: the retry and
 * the early exits are decided on the device.  One synchronisation: the copy-out. */
typedef struct {
    int32_t w, h;            /* a projection is a candidate only inside [0, w) x [0, h) */
    int32_t window;          /* keyframe positions of the local map, counted from the last (10); 0: all */
    int32_t n_pass;          /* 1 .. 4 (2) */
    double radius[4];        /* search half-width of each pass at octave 0 (15, 4) */
    double scale_factor;     /* scales the window and the information (1.2) */
    double ratio;            /* best-to-second ratio (0.8) */
    double chi2;             /* outlier threshold; the Huber width is its square root (5.991) */
    int32_t max_dist;        /* ORB-SLAM2's TH_HIGH (100) */
    int32_t min_matches;     /* a pass with fewer matches is retried once at twice its radius (20) */
    int32_t min_inliers;     /* ok needs this many inliers after the last pass (30) */
} mo_map_track_params;
typedef struct {
    /* caller-allocated, may be NULL; n_q = keypoints of the frame */
    int32_t* point;          /* [n_q] map point matched to each keypoint by the last pass searched (-1: none) */
    int32_t* dist;           /* [n_q] its Hamming distance (-1: none) */
    uint8_t* inlier;         /* [n_q] final classification of that pass's refinement (0 where it did not refine) */
    /* filled by the call */
    double pose[12];         /* [R | t] row-major of the last pass that finished, else pose0 */
    double pass_pose[4][12]; /* refined pose of each pass (NaN: the pass did not finish) */
    double pass_radius[4];   /* the radius each pass used (twice radius[k] after a retry; 0: did not run) */
    int32_t pass_cand[4];    /* candidates of each pass (of its last attempt) */
    int32_t pass_matches[4]; /* matches of each pass (of its last attempt) */
    int32_t pass_inliers[4]; /* inliers after each pass's refinement */
    int32_t n_pass_run;      /* passes whose search ran (a pass that ended the call included) */
    int32_t n_local;         /* points of the local map */
    int32_t ok;              /* 1: the last pass finished with >= min_inliers inliers */
    int32_t from_token;      /* 1: the frame was read from its resident slot */
} mo_map_track_out;
int mo_map_track(mo_map*, const mo_frame_ref* f, const double K[9], const double pose0[12], const mo_map_track_params*, mo_map_track_out*);

/* mo_map_track_batch: n_frames frames tracked against the map as it stands in one device chain (the cameras of a rig, a recorded sequence
 * localised from odometry priors, a set of relocalised frames, the frames of one stream chunk); reads the map, never changes it.
 *   the rule      for every i, everything the call returns for frame i is what mo_map_track(m, &frames[i], K, pose0 + 12 * i, prm, ...)
 *                 returns for that frame alone on the same map: every integer equal, every double equal bit for bit (pass_pose, pose
 *                 and the pose0 a frame that finished no pass falls back to included).  The order and the company of the frames change
 *                 nothing; a frame that ends early (too few matches after the retry, fewer than 10 inliers in the refinement, a Hessian
 *                 that is not positive definite) has no effect on any other frame.
 *   shared        n_local alone: the local map depends on the map and `window`, and is formed once for the batch (mo_map_track reports 0
 *                 for a frame without keypoints, for which it forms no local map; here n_local is the batch's).  One K, one image
 *                 size and one parameter set serve every frame.
 *   layout        frame i's per-keypoint rows start at i * stride; rows past a frame's n are not written.
 *   no work       n_frames = 0: nothing runs.  A frame without keypoints: no pass runs for it, ok = 0, the others go on.  A map without
 *                 keyframes or map points: no pass runs for any frame, n_local = 0.  None of these is an error.
 *   errors        MO_ERR_ARG for a NULL required pointer, n_frames outside 0 .. MO_TRACK_BATCH_MAX, a frame of more than `stride` rows,
 *                 a pose0 that is not finite, and every parameter mo_map_track refuses.  A token that is no longer resident falls back
 *                 to the frame's arrays.
 * One chain on the context stream, one synchronisation (the copy-out): every retry and early exit is a per-frame flag on the device.
 * Integer atomics and fixed-order f64 reductions only: equal inputs give equal bytes on every run.  Stage marks tb_stage, tb_prep,
 * tb_search, tb_refine (mo_stage_times). */
#define MO_TRACK_BATCH_MAX 1024
typedef struct {
    /* caller-allocated; the per-keypoint arrays may be NULL.  Frame i's rows start at i * stride. */
    int32_t stride;          /* rows per frame in the arrays below, >= every frame's n */
    int32_t* point;          /* [n_frames][stride] as mo_map_track_out.point */
    int32_t* dist;           /* [n_frames][stride] */
    uint8_t* inlier;         /* [n_frames][stride] */
    double* pose;            /* [n_frames][12]     required, like every array below */
    double* pass_pose;       /* [n_frames][4][12] */
    double* pass_radius;     /* [n_frames][4] */
    int32_t* pass_cand;      /* [n_frames][4] */
    int32_t* pass_matches;   /* [n_frames][4] */
    int32_t* pass_inliers;   /* [n_frames][4] */
    int32_t* n_pass_run;     /* [n_frames] */
    int32_t* ok;             /* [n_frames] */
    int32_t* from_token;     /* [n_frames] */
    /* filled by the call */
    int32_t n_local;         /* points of the local map (one local map for the whole batch) */
    int32_t n_ok;            /* frames with ok = 1 */
} mo_map_track_batch_out;
int mo_map_track_batch(mo_map*, const mo_frame_ref* frames, int32_t n_frames, const double K[9], const double* pose0,
                       const mo_map_track_params*, mo_map_track_batch_out*);
int mo_format_floats(const float* v, int64_t n, char* out, size_t cap, size_t* len);

/* mo_map_bundle_adjust: local bundle adjustment on the map as it stands (ORB-SLAM2's Optimizer::LocalBundleAdjustment, monocular): the
 * poses of the last keyframes and the positions of the points they see are refined together.  poses = [n_kf][12], [R | t] row-major per
 * keyframe POSITION (X_cam = R X + t; the store itself only holds P = K [R | t]).
 *   observations  read like the cull and mo_map_track read them (negative positions and rows count from the end; entries naming a position
 *                 or row that does not exist are skipped).  An edge = one valid observation (point, keyframe position, row).
 *   window        the candidate positions are the last `window` (0: all) except position 0, which is never free.  More than 16 candidates
 *                 are refused with MO_ERR_ARG, not truncated.
 *   local points  the points with >= 2 edges of which at least one is at a candidate position (decided before the gauge rule below).
 *   keyframes     a position with an edge to a local point takes part: fixed when it is not a candidate, else free.  Gauge: while fewer
 *                 than two keyframes are fixed, the lowest free position becomes fixed too (two fixed poses pin the 7 degrees of freedom
 *                 of a monocular map: position, orientation and scale).  Fixed keyframes contribute residuals, not unknowns; positions
 *                 without an edge to a local point are outside the problem.
 *   residual      e = keypoint - projection, f64; projection p = K (R X + t), (p0 / p2, p1 / p2) as mo_map_track forms it; information
 *                 1 / scale_factor^(2 octave) (repeated products from 1.0, negative octaves as 0).  An edge whose projection is not finite
 *                 contributes nothing and is an outlier.
 *   rounds        round 0: at most max_steps[0] Levenberg-Marquardt steps over all edges with the Huber cost of width sqrt(chi2) on
 *                 information * |e|^2 (cost s below chi2, 2 sqrt(chi2 s) - chi2 above; weight sqrt(chi2 / s) above); then every edge is
 *                 classified (inlier: depth > 0 and information * |e|^2 <= chi2); round 1: at most max_steps[1] steps over the inliers
 *                 without Huber; then the final classification.
 *   one step      normal equations of the weighted edges with Jacobians of the projection against the left perturbation (rho, w) of the
 *                 pose (R' = exp(w) R, t' = exp(w) t + rho) and against the point.  Damping: every diagonal entry times (1 + lambda);
 *                 lambda is 1e-4 at the start of each round.  Points are eliminated by the Schur complement (per point V 3x3, inverted
 *                 by Cholesky; a V that is not positive definite holds that point fixed for the step), the reduced camera system
 *                 (6 n_free <= 96) is solved by Cholesky, the points are back-substituted.  The step is accepted when it lowers the
 *                 round's cost (lambda / 10), else undone (lambda * 10); both count as a step.  A round ends early at an update below
 *                 1e-10 (largest absolute entry over all unknowns, accepted or not), at lambda > 1e8, or at a reduced system that is not
 *                 positive definite (that attempt is not counted).
 *   writes        xyz of the local points (the f64 result rounded to f32) and, when at least one step was accepted, P = K [R | t] of the free keyframes.  Nothing else: no
 *                 observation is erased, no point removed; points and keyframes outside the problem keep their bytes
 *                 (mo_map_bundle_adjust_local with erase_outliers erases the outlier entries).
 *   returns       ok = the problem ran and n_inliers >= min_inliers.  An empty map, no free keyframe, or no local point: nothing runs,
 *                 nothing is written, every count is 0, ok = 0, not an error.
 * Everything is decided on the device (flags in a result block that later kernels read first): no host round trip inside the call, one
 * synchronisation - the copy-out.  No floating-point atomics: two calls on equal maps give the same bytes. */
typedef struct {
    int32_t window;          /* candidate free positions, counted from the last (10); 0: all */
    int32_t min_inliers;     /* ok needs this many inlier edges at the end (50) */
    int32_t max_steps[2];    /* steps of round 0 and round 1, each 0 .. 100 (5, 10) */
    double scale_factor;     /* of the information (1.2) */
    double chi2;             /* outlier threshold; the Huber width is its square root (5.991) */
} mo_map_ba_params;
typedef struct {
    /* caller-allocated, may be NULL */
    double* poses_out;       /* [n_kf][12] the free ones refined, the rest as given */
    int32_t* kf_state;       /* [n_kf] 0 outside the problem, 1 fixed, 2 free */
    uint8_t* edge_inlier;    /* [n_obs] per entry of the observation arrays: 0 skipped or outside the problem, 1 inlier, 2 outlier */
    double* points_out;      /* [n_pts][3] f64 positions of the local points, NaN elsewhere */
    /* filled by the call */
    double cost[3];          /* robust cost at the start, robust cost after round 0, plain cost of the inliers at the end */
    double lambda;           /* damping after the last step */
    int32_t n_free, n_fixed, n_local, n_edges, n_inliers;
    int32_t steps[2], accepted[2];
    int32_t ok;
} mo_map_ba_out;
int mo_map_bundle_adjust(mo_map*, const double K[9], const double* poses, const mo_map_ba_params*, mo_map_ba_out*);
/* mo_map_add_observations: the observation (kf_pos, row[i]) is appended to map point point[i] (index into the map as it stands), at the
 * end of that point's list.  Skipped: point[i] < 0 or out of range, a point that already has a valid observation at kf_pos (for kf_pos == the number of
 * keyframes: an entry stored with that very position); when two
 * entries name the same point the lower i wins.  kf_pos == the number of keyframes means the keyframe the next mo_map_add_keyframe
 * stores (its cull validates the rows: MO_ERR_INDEX for one that does not exist).  The observation arrays are rebuilt into the other
 * copy of the map store by a scan and a scatter; one synchronisation. */
int mo_map_add_observations(mo_map*, int kf_pos, int n, const int32_t* point, const int32_t* row);

/* mo_map_fuse: map points that are the same 3D feature are merged, and points gain the observations they lack (ORB-SLAM2's
 * LocalMapping::SearchInNeighbors / ORBmatcher::Fuse / MapPoint::Replace), on the map as it stands.  Opt-in: no other call runs it.
 *   observations  read like the cull and mo_map_track read them (negative positions and rows count from the end; entries naming a position
 *                 or row that does not exist are skipped; "valid" below means an entry that names something).
 *   targets       the last `window` keyframe positions (0: every position).
 *   local points  the points with a valid observation at a target: mo_map_track's local map, with its representative descriptor and
 *                 ref_octave (ComputeDistinctiveDescriptors, ties to the earlier observation).
 *   pairs         every (local point i, target k) where i has no valid observation at k.
 *   candidate     a pair whose projection under the store's own P of k (what mo_map_add_keyframe stored or mo_map_bundle_adjust wrote
 *                 back: the call takes no poses; f64, each row summed left to right, z = P[8..11] . (X, 1)) has z > 0 and u / z in [0, w),
 *                 v / z in [0, h).
 *   search        r = radius * scale_factor^ref_octave (repeated products from 1.0); the keypoints of k with |x - u| < r, |y - v| < r,
 *                 |octave - ref_octave| <= 1 and information(octave) * ((x - u)^2 + (y - v)^2) <= chi2 (information = 1 /
 *                 scale_factor^(2 octave), negative octaves as 0); best = the lowest Hamming distance to the representative, ties to the
 *                 lower row; accepted when best <= max_dist.  No ratio test (Fuse has none).  An accepted pair is a proposal
 *                 (i, k, row, dist).
 *   claims        per (k, row) the proposal with the lowest (dist, i) wins; the others are dropped.
 *   owner         of (k, row): the lowest map point with a valid observation (k, row) (mo_map_relocalize's point_of).  A winning
 *                 proposal on an owned row is a merge edge {i, owner}; on a free row it is a gained observation (i, k, row).
 *   components    the connected components of the merge edges over all points; survivor = the member with the most valid observations,
 *                 ties to the lowest index.
 *   merged list   of a survivor, in this order: (1) its own entries as stored (stale ones included, bytes unchanged); (2) the valid
 *                 entries of the other members by (member index, insertion order), written as non-negative (position, row); (3) the gained
 *                 observations of all members by (member index, position).  An entry of (2) or (3) is dropped when the list already holds
 *                 a valid observation at its position (Replace's "already in keyframe").  A point in no merge edge is a component of one:
 *                 it keeps (1) and takes (3).
 *   writes        absorbed members are removed; survivors keep xyz, colour, id and descriptor reference; the map is compacted in index
 *                 order into the other copy of the store, as the cull does.  The per-keyframe lists stay those of the last cull, as after
 *                 mo_map_add_observations.  Points outside the local map and in no merge edge keep their bytes.
 *   no work       an empty map or no keyframes: every count is 0.  No local point or no proposal: nothing is written, n_targets, n_local,
 *                 n_pairs and n_cand are reported, the other counts are 0, into is the identity.  Never an error.
 * Everything is decided on the device (later kernels read n_proposals first): no host round trip inside the call, one synchronisation -
 * the copy-out.  Integer atomics only: two calls on equal maps give the same bytes. */
typedef struct {
    int32_t w, h;            /* a projection is a candidate only inside [0, w) x [0, h) */
    int32_t window;          /* target keyframe positions, counted from the last (10); 0: all */
    double radius;           /* search half-width at octave 0 (3.0) */
    double scale_factor;     /* scales the window and the information (1.2) */
    int32_t max_dist;        /* ORB-SLAM2's TH_LOW (50) */
    double chi2;             /* gate on information * squared pixel distance (5.991) */
} mo_map_fuse_params;
typedef struct {
    /* caller-allocated, may be NULL */
    int32_t* into;           /* [map points before the call] the new index of the point each old point now is */
    /* filled by the call */
    int32_t n_targets, n_local, n_pairs, n_cand, n_proposals, n_gained, n_edges, n_absorbed;
    int64_t n_points, n_obs; /* after the call */
} mo_map_fuse_out;
int mo_map_fuse(mo_map*, const mo_map_fuse_params*, mo_map_fuse_out*);

/* mo_map_grow: new map points for the last keyframe from its neighbour keyframes (ORB-SLAM2's LocalMapping::CreateNewMapPoints /
 * ORBmatcher::SearchForTriangulation), on the map as it stands: every keypoint of the last keyframe that no map point observes is
 * searched along its epipolar line among the unobserved keypoints of the neighbours, triangulated and gated.  Opt-in: no other call
 * runs it.  poses = [n_kf][12], [R | t] row-major per keyframe POSITION, as mo_map_bundle_adjust takes them.  Everything is f64; every
 * sum runs left to right as written; s(o) = scale_factor^o and s2(o) = (scale_factor * scale_factor)^o are repeated products from 1.0
 * (negative octaves as 0; 1 / s2(o) is the information of mo_map_track).
 *   observations  read like every other reader of the map (negative positions and rows count from the end; entries naming a position
 *                 or row that does not exist are skipped).
 *   target        the last keyframe position T = n_kf - 1; its image is the one the last mo_map_add_keyframe stored.
 *   neighbours    the positions max(0, T - window) .. T - 1 (window 0: every earlier position).  Fewer than 2 keyframes: no work, every
 *                 count is 0, not an error.
 *   free row      a row of a keyframe that no map point validly observes (the complement of mo_map_relocalize's point_of).  Only free
 *                 rows take part, on both sides.
 *   camera        fx = K[0], fy = K[4], cx = K[2], cy = K[5]; of a keypoint xn = (x - cx) / fx, yn = (y - cy) / fy.
 *   pair          target (R1, t1), neighbour k (R2, t2):
 *                 R12[i][j] = R1[i][0] R2[j][0] + R1[i][1] R2[j][1] + R1[i][2] R2[j][2];
 *                 t12[i] = t1[i] - (R12[i][0] t2[0] + R12[i][1] t2[1] + R12[i][2] t2[2]);
 *                 E = [t12]x R12: E[0][j] = t12[1] R12[2][j] - t12[2] R12[1][j], E[1][j] = t12[2] R12[0][j] - t12[0] R12[2][j],
 *                 E[2][j] = t12[0] R12[1][j] - t12[1] R12[0][j];
 *                 G = E K^-1: G[i][0] = E[i][0] (1 / fx), G[i][1] = E[i][1] (1 / fy), G[i][2] = (E[i][2] - G[i][0] cx) - G[i][1] cy;
 *                 F = K^-T G: F[0][j] = G[0][j] (1 / fx), F[1][j] = G[1][j] (1 / fy), F[2][j] = (G[2][j] - F[0][j] cx) - F[1][j] cy;
 *                 C1[i] = -(R1[0][i] t1[0] + R1[1][i] t1[1] + R1[2][i] t1[2]) (C2 likewise);
 *                 c2[i] = R2[i][0] C1[0] + R2[i][1] C1[1] + R2[i][2] C1[2] + t2[i]; the epipole ex = (fx c2[0]) / c2[2] + cx,
 *                 ey = (fy c2[1]) / c2[2] + cy in plain IEEE arithmetic: a non-finite epipole excludes nothing.
 *   search        free target row (x1, y1) against free neighbour row (x2, y2, o2): a = x1 F[0][0] + y1 F[1][0] + F[2][0], b and c
 *                 likewise from columns 1 and 2; den = a a + b b; rejected when den == 0; rejected when
 *                 (ex - x2)^2 + (ey - y2)^2 < epipole_r2 s(o2); num = a x2 + b y2 + c; passes when (num num) / den < epi_chi2 s2(o2).
 *                 Among the passing rows best = the lowest Hamming distance, ties to the lower row; accepted when best <= max_dist.
 *                 No ratio test (SearchForTriangulation has none) and no orientation histogram (left out).
 *   claims        per (k, row2) the accepted target row with the lowest (dist, row1) wins; the others lose that neighbour.
 *   base pair     of a target row with at least one won match: rays r1[i] = R1[0][i] xn1 + R1[1][i] yn1 + R1[2][i], r2 likewise;
 *                 cosp = (r1 . r2) / (sqrt(r1 . r1) sqrt(r2 . r2)); a match is usable when 0 < cosp < cos_max; the base pair is the
 *                 usable match with the lowest cosp, ties to the lower position.  No usable match: no point.
 *   triangulation of the base pair: the rows xn T[2] - T[0] and yn T[2] - T[1] of the target, then of the neighbour (T = [R | t], four
 *                 entries each), taken inhomogeneously: A the first three columns, a4 the fourth;
 *                 N[i][j] = A[0][i] A[0][j] + A[1][i] A[1][j] + A[2][i] A[2][j] + A[3][i] A[3][j],
 *                 g[i] = -(A[0][i] a4[0] + A[1][i] a4[1] + A[2][i] a4[2] + A[3][i] a4[3]); Cholesky N = L L^T:
 *                 l00 = sqrt(N00), l10 = N10 / l00, l20 = N20 / l00, l11 = sqrt(N11 - l10 l10), l21 = (N21 - l20 l10) / l11,
 *                 l22 = sqrt((N22 - l20 l20) - l21 l21); y0 = g0 / l00, y1 = (g1 - l10 y0) / l11, y2 = ((g2 - l20 y0) - l21 y1) / l22;
 *                 X2 = y2 / l22, X1 = (y1 - l21 X2) / l11, X0 = ((y0 - l10 X1) - l20 X2) / l00.  A radicand that is not > 0: no point.
 *   gates         on the base pair, in both views: Xc[i] = R[i][0] X0 + R[i][1] X1 + R[i][2] X2 + t[i]; depth Xc[2] > 0; u = (fx Xc[0]) /
 *                 Xc[2] + cx, v likewise; information(octave) ((u - x)^2 + (v - y)^2) <= chi2; d1 = |X - C1| and d2 = |X - C2| (sqrt of
 *                 the squares summed x, y, z) both > 0; with rd = d2 / d1 and ro = s(o1) / s(o2): rejected when rd ratio_factor < ro or
 *                 rd > ro ratio_factor.  A failure means no point: there is no fallback to another pair.
 *   further obs.  the row's other won matches become observations of the new point when depth > 0 and the reprojection gate hold in
 *                 that neighbour; otherwise they are dropped.
 *   writes        the new points are appended to the live copy of the store in order of target row: xyz = the f64 result rounded to
 *                 f32; colour read as mo_map_add_keyframe's growth reads it, from the target's stored image ((0, 0, 255) without an
 *                 image or outside it); id = its index at creation; descriptor reference = (target slot, row); observations written
 *                 non-negative, the neighbours in ascending position, then the target.  The per-keyframe lists stay those of the last
 *                 cull, as after mo_map_fuse.  Existing points keep their bytes.
 * Everything is decided on the device (later kernels read the counts first): no host round trip inside the call, one synchronisation -
 * the copy-out.  Integer atomics only: two calls on equal maps give the same bytes. */
typedef struct {
    int32_t window;          /* neighbour positions before the last (10); 0: all */
    int32_t max_dist;        /* ORB-SLAM2's TH_LOW (50) */
    double scale_factor;     /* of the pyramid (1.2) */
    double epi_chi2;         /* gate on the squared epipolar distance over s2(octave) (3.84) */
    double chi2;             /* gate on information * squared reprojection error (5.991) */
    double cos_max;          /* parallax: the rays' cosine must be below it (0.9998) */
    double ratio_factor;     /* scale consistency (1.5 * scale_factor) */
    double epipole_r2;       /* squared radius of the zone round the epipole at octave 0 (100) */
} mo_map_grow_params;
typedef struct {
    /* caller-allocated, may be NULL; n_rows = keypoints of the last keyframe */
    int32_t* point;          /* [n_rows] index of the map point each row created (-1: none) */
    double* points;          /* [n_rows][3], the first n_new filled: the new points in f64, in order */
    /* filled by the call */
    int32_t n_neighbours;
    int32_t n_free;          /* free target rows */
    int32_t n_accepted;      /* (row1, k) with an accepted best row */
    int32_t n_matches;       /* of them, those that won their claim */
    int32_t n_new;           /* points created */
    int32_t n_obs_new;       /* their observations */
    int64_t n_epi;           /* (row1, k, row2) that passed the epipole and the epipolar gate */
    int64_t n_points, n_obs; /* after the call */
} mo_map_grow_out;
int mo_map_grow(mo_map*, const double K[9], const double* poses, const mo_map_grow_params*, mo_map_grow_out*);

/* Covisibility on the device map, and the local keyframes ORB-SLAM2's Tracking::UpdateLocalKeyFrames picks from it; both read the map,
 * neither changes it.  Opt-in: mo_map_track, mo_map_bundle_adjust, mo_map_fuse and mo_map_grow keep their recency windows
 * (mo_map_track_covisible and mo_map_bundle_adjust_local are the covisible forms of the first two).
 *
 * mo_map_covisibility: the matrix W [n_kf][n_kf] (int32, row-major, by keyframe POSITION) into `weights` (host, may be NULL: compute
 * only) and the number of keyframes into *n_kf.  W stays resident on the device for the calls below.
 *   observations  an observation counts when the one reader of the map (the cull's, mo_map_track's) accepts it: negative positions
 *                 and rows count from the end; entries naming a position or row that does not exist name nothing.
 *   W[p][q]       p != q: the number of map points with at least one valid observation at position p and at least one at q.
 *   W[p][p]       the number of map points with a valid observation at p.
 *   duplicates    a point observed twice in one keyframe counts once for that keyframe.
 *   W is symmetric.  It is recomputed on every call: the map carries no version to cache against.  No map points: all zeros.  No
 *   keyframes: *n_kf = 0, MO_OK, nothing is written to `weights`.
 * Integer atomics only (sums commute): the same exact matrix on every run, whichever of the two accumulation paths (a copy per workgroup
 * in LDS up to 128 keyframes, global atomics beyond) runs.
 *
 * mo_map_local_keyframes: W is computed first; the selection runs on the device from it.
 *   votes         every seed entry (an index into the map points; < 0 or >= the number of points: skipped) votes once for each position
 *                 its point validly observes (twice in one keyframe: one vote).  An index given twice votes twice.
 *   K1            the positions with at least one vote.  ref = the position with the most votes, ties to the later position.  Nothing
 *                 voted (n_seed = 0 included): K1 = {ref_pos} and ref = ref_pos; ref_pos = -1 names the last keyframe.
 *   K2            for each p in K1 the n_best positions q != p with the largest W[p][q] among those with W[p][q] >= max(min_weight, 1),
 *                 ties to the later position.
 *   local         K1 and K2 together: local[k] = 1 for K1, 2 for K2 only, 0 otherwise.
 *   errors        MO_ERR_ARG for NULL arguments, n_best < 0, n_seed < 0, n_seed > 0 with NULL seed_points, and - when the map has at
 *                 least one keyframe - ref_pos outside -1 .. n_kf - 1.  No keyframes: MO_OK, every count 0, ref = -1.
 *
 * mo_map_track_covisible: mo_map_track with one difference: a point is in the local map when it has a valid observation at a local
 * keyframe of mo_map_local_keyframes (K1 or K2).  prm->window is validated as mo_map_track validates it and not used.  The matrix, the
 * selection and the tracking kernels run on the context stream behind each other; one synchronisation, the copy-out.  A selection that
 * makes every keyframe local gives mo_map_track's bytes at window = 0. */
typedef struct {
    const int32_t* seed_points; /* host, map point indices; < 0 or >= n_pts: skipped */
    int32_t n_seed;             /* 0: no seeds, K1 = {ref_pos} */
    int32_t ref_pos;            /* used when no seed votes; -1: the last keyframe */
    int32_t n_best;             /* neighbours taken per K1 keyframe, >= 0 (10) */
    int32_t min_weight;         /* a neighbour needs W >= max(min_weight, 1) (15) */
} mo_map_local_params;
typedef struct {
    /* caller-allocated, may be NULL */
    uint8_t* local;             /* [n_kf] 1 = K1, 2 = K2 only, 0 = not local */
    /* filled by the call */
    int32_t n_k1, n_local_kf, ref; /* ref: the K1 position with the most votes */
} mo_map_local_out;
int mo_map_covisibility(mo_map*, int32_t* weights, int32_t* n_kf);
int mo_map_local_keyframes(mo_map*, const mo_map_local_params*, mo_map_local_out*);
int mo_map_track_covisible(mo_map*, const mo_frame_ref* f, const double K[9], const double pose0[12], const mo_map_track_params*,
                           const mo_map_local_params*, mo_map_local_out*, mo_map_track_out*);

/* ---- Local bundle adjustment over a set of keyframes, and the erase of single observation entries (map_ba.hip) ---------------------------
 * Opt-in: mo_map_bundle_adjust keeps its window and erases nothing; every earlier call launches what it launched.
 *
 * mo_map_bundle_adjust_local: mo_map_bundle_adjust with one difference: the candidate positions are a set C, not the last `window`.
 * prm->window is validated as mo_map_bundle_adjust validates it and not used.
 *   C             free_mask given (host [n_kf], by position): its non-zero positions; more than 16 of them other than position 0 are
 *                 refused with MO_ERR_ARG, not truncated.  free_mask NULL: kf_pos (-1: the last keyframe) and its n_best (0 .. 15)
 *                 heaviest covisible neighbours, a neighbour q needing W[kf_pos][q] >= max(min_weight, 1), heaviest first, ties to the
 *                 later position: mo_map_local_keyframes with n_seed = 0 and ref_pos = kf_pos, run inside this call's chain and read on
 *                 the device.  Position 0 is dropped from C in both forms: it is never free, and takes part as a fixed keyframe when it
 *                 has edges.
 *   rules         every rule of mo_map_bundle_adjust with "candidate position" read as "position in C": a local point has >= 2 edges,
 *                 one of them at a position in C; a position with an edge to a local point is fixed when it is not in C, else free; the
 *                 gauge: while fewer than two keyframes are fixed, the lowest position of C that has edges becomes fixed too; a candidate
 *                 without an edge to a local point is outside the problem.  C = the last w positions gives mo_map_bundle_adjust's bytes at
 *                 window = w.
 *   erase         erase_outliers != 0: when the problem ran and n_inliers >= min_inliers, the entries whose final class is 2 (chi2 above
 *                 the threshold, non-positive depth or a projection that is not finite, after round 1) leave the observation arrays in
 *                 the same device chain, by mo_map_erase_observations' rule.  Otherwise nothing is erased: a failed adjustment does not
 *                 strip the map.  edge_inlier is indexed by the entries as they were before the erase.
 *   deviations    ORB-SLAM2 frees every covisible neighbour and fixes only keyframe 0 and the outside observers; here the dense reduced
 *                 system caps C at 16 and the two-fixed gauge stands (more keyframes: mo_map_global_ba).  ORB-SLAM2's EraseObservation
 *                 also drops a point left with two or fewer observations; this call leaves such points in the map and reports n_under;
 *                 mo_map_cull_points' reason 3 (orphan_obs) removes them.
 *   errors        MO_ERR_ARG as mo_map_bundle_adjust (but for the window's width), for NULL local arguments, n_best outside 0 .. 15,
 *                 and - when the map has a keyframe - kf_pos outside -1 .. n_kf - 1.  An empty map: nothing runs, candidate is all 0.
 * One synchronisation, the copy-out; no floating-point atomics: two calls on equal maps give equal bytes.
 *
 * mo_map_erase_observations: the entries o of the observation arrays with erase[o] != 0 (host [n_obs]) leave.  Every point keeps its
 * index, every field and its life record, and may end with no entries; the surviving entries keep their order and their stored bytes,
 * entries that name nothing included (such an entry may be flagged too: that is how a caller clears stale keys).  The per-keyframe lists
 * stay those of the last cull, as after mo_map_fuse.  Nothing flagged: nothing is written and the store is not rebuilt, as
 * mo_map_erase_points behaves then.  The rebuild is entry-parallel: keep flags, one exclusive scan over the n_obs entries, one thread per
 * entry for the copy and one per point for the offsets (off[i] = S[off[i]]); one synchronisation. */
typedef struct {
    const uint8_t* free_mask; /* host [n_kf] by position, non-zero: candidate; NULL: the covisible set of kf_pos */
    int32_t kf_pos;           /* the keyframe whose neighbours are taken; -1: the last (-1) */
    int32_t n_best;           /* neighbours taken, 0 .. 15 (15) */
    int32_t min_weight;       /* a neighbour needs W >= max(min_weight, 1) (15) */
    int32_t erase_outliers;   /* != 0: the entries of final class 2 are erased behind a successful adjustment (0) */
} mo_map_ba_local_params;
typedef struct {
    /* caller-allocated, may be NULL */
    uint8_t* candidate;       /* [n_kf] 1 at a position of C (before the gauge) */
    /* filled by the call */
    int32_t n_candidates;
    int32_t n_erased;         /* entries erased */
    int32_t n_under;          /* points that lost an entry and now hold fewer than two */
    int64_t n_obs;            /* entries after the call */
} mo_map_ba_local_out;
typedef struct {
    int32_t n_erased;         /* entries that left */
    int32_t n_under;          /* points that lost an entry and now hold fewer than two */
    int64_t n_obs;            /* entries after the call */
} mo_map_obserase_out;
int mo_map_bundle_adjust_local(mo_map*, const double K[9], const double* poses, const mo_map_ba_params*, const mo_map_ba_local_params*,
                               mo_map_ba_out*, mo_map_ba_local_out*);
int mo_map_erase_observations(mo_map*, const uint8_t* erase, mo_map_obserase_out*);

/* ---- Keyframe culling by ORB-SLAM2's rule, and a removal that leaves an exact map (map_kfcull.hip) ---------------------------------------
 * Opt-in: mo_map_add_keyframe's own counts (kf_len / kf_redundant) and mo_map_remove_keyframes are unchanged.
 * tests/kfcull_restatement.py restates all of it in numpy.
 *
 * mo_map_kf_redundancy: ORB-SLAM2's LocalMapping::KeyFrameCulling for a monocular map, decided on the device from the map as it stands;
 * read-only, nothing is stored.
 *   asking        p = kf_pos, -1: the last keyframe.
 *   candidates    the positions q != p with W[p][q] >= max(min_weight, 1), W the matrix of mo_map_covisibility; ordered by W[p][q]
 *                 descending, ties to the later position (the tie rule of mo_map_local_keyframes).  n_local = their number.
 *   observation   valid as above.  Of several valid observations of one point at one keyframe the first in entry order is that keyframe's
 *                 observation of the point: its row, and the octave of that stored keypoint (a negative octave counts as 0).
 *   per candidate c, in that order:
 *                 n_points     the points with a valid observation at c (= W[c][c]).
 *                 n_redundant  those of them that at least min_observers OTHER positions observe validly at an octave <= the octave at
 *                              c + scale_gap.  The observers are all keyframes of the map, candidates or not; positions removed earlier in
 *                              this call do not count.
 *                 removed      (double)n_redundant > ratio * (double)n_points, in f64 (one product, one compare) - except position 0 and
 *                              the positions with protect[q] != 0 (the caller's SetNotErase), which are counted and reported and stay.
 *   sequential    the decision for c sees the removals decided before it in the order (ORB-SLAM2's SetBadFlag inside the loop): of two
 *                 keyframes that are redundant only through each other, the first in the order goes.
 *   outputs       in candidate order, each [n_kf] (entries from n_local on: pos -1, the rest 0); n_local, n_removed.
 *   empty         fewer than two keyframes or no map points: MO_OK, n_local = 0, the arrays are not written.
 *   errors        MO_ERR_ARG for NULL arguments, min_observers < 1, a ratio that is not finite, walk outside 0 .. 2 and - when the map has
 *                 at least one keyframe - kf_pos outside -1 .. n_kf - 1.  MO_ERR_CAPACITY beyond 4096 keyframes.
 *   The matrix, the order, the per-candidate lists and the decisions run behind each other on the context stream; one synchronisation, the
 *   copy-out; the host takes no part in a decision.  Integer atomics only: equal maps give equal results, whichever way the candidates
 *   are walked (walk: one launch per candidate - the default, 0 - or one workgroup through all of them, 1, which is slower).
 *
 * mo_map_erase_keyframes: the keyframes at `positions` (duplicates allowed) removed so that the map is the map that never had them.
 *   observations  rebuilt into the other copy of the store: a point keeps, in entry order, its valid observations at surviving positions,
 *                 the key rewritten to the non-negative position AFTER the removal, the row to the non-negative row.  Observations at
 *                 erased positions and entries that name nothing are dropped.
 *   points        xyz, colour, id and the descriptor reference are unchanged in count, order and bytes: point indices stay valid.  A
 *                 point may be left with one observation or none and stays: ORB-SLAM2's EraseObservation kills a point at two
 *                 observations or fewer, and here that is mo_map_cull_points' part (its orphan_obs rule, below).  Without that call the
 *                 next mo_map_add_keyframe culls the point by its own rule; bundle adjustment ignores it already.
 *   positions     the position table is shortened as mo_map_remove_keyframes shortens it: survivors keep their store slots (freed slots
 *                 are not reused) and so their entries of the keyframe database.
 *   errors        a position outside 0 .. n_kf - 1: MO_ERR_ARG, the map unchanged.  n = 0: MO_OK, nothing happens.
 *   One synchronisation: the new observation count.
 *
 * mo_map_cull_keyframes: with erase = 0 mo_map_kf_redundancy; with erase = 1 the decision and the erase of what it removed in one chain:
 * the rewrite kernels read the decision flags on the device, the host learns them and the new observation count at the one
 * synchronisation and then shortens the position table.  When nothing is removed the map keeps its bytes. */
typedef struct {
    int32_t kf_pos;          /* the asking keyframe; -1: the last */
    int32_t min_weight;      /* a candidate needs W >= max(min_weight, 1) (15) */
    int32_t min_observers;   /* >= 1 (3) */
    int32_t scale_gap;       /* (1) */
    double ratio;            /* finite (0.9) */
    const uint8_t* protect;  /* host [n_kf] by position, non-zero: never removed; may be NULL */
    int32_t erase;           /* mo_map_cull_keyframes: 1 erases what was removed */
    int32_t walk;            /* 0: the library's choice (one launch per candidate), 1: one workgroup walks the candidates, 2: one launch per candidate */
} mo_map_kfcull_params;
typedef struct {
    /* caller-allocated [n_kf] each, may be NULL; in candidate order */
    int32_t* pos;
    int32_t* weight;
    int32_t* n_points;
    int32_t* n_redundant;
    int32_t* removed;
    /* filled by the call */
    int32_t n_local, n_removed;
    int64_t n_obs;           /* observations of the map after the call */
} mo_map_kfcull_out;
int mo_map_kf_redundancy(mo_map*, const mo_map_kfcull_params*, mo_map_kfcull_out*);
int mo_map_erase_keyframes(mo_map*, const int32_t* positions, int n);
int mo_map_cull_keyframes(mo_map*, const mo_map_kfcull_params*, mo_map_kfcull_out*);

/* ---- Point views and the frustum mode of the searches (map_view_geom.hip, map_search.h) -----------------------------------------------
 * Where a map point was seen from, and ORB-SLAM2's use of it (MapPoint::UpdateNormalAndDepth, Frame::isInFrustum, MapPoint::PredictScale,
 * the level gate of ORBmatcher::SearchByProjection and Fuse).  Opt-in: mo_map_track, mo_map_track_covisible and mo_map_fuse decide from
 * ref_octave as before.  Everything below is f64 unless it says f32; every sum runs left to right as written; s(o) = scale_factor^o as
 * repeated products from 1.0 (negative o as 0).  tests/view_restatement.py restates it in numpy, operation for operation.
 *
 * mo_map_point_views: read-only on the map; one chain, one synchronisation - the copy-out.  Nothing is stored: the calls below recompute
 * the same values (for their local points) inside their own chains.
 *   centre        of keyframe position k, from the store's own P = K [R | t] (what mo_map_add_keyframe stored or a bundle adjustment
 *                 wrote back; the call takes no poses): M = P[:, :3], p = P[:, 3];
 *                   a00 = m11 m22 - m12 m21   a01 = m02 m21 - m01 m22   a02 = m01 m12 - m02 m11
 *                   a10 = m12 m20 - m10 m22   a11 = m00 m22 - m02 m20   a12 = m02 m10 - m00 m12
 *                   a20 = m10 m21 - m11 m20   a21 = m01 m20 - m00 m21   a22 = m00 m11 - m01 m10
 *                 det = m00 a00 + m01 a10 + m02 a20;  C_i = -((a_i0 p0 + a_i1 p1 + a_i2 p2) / det).  det == 0 or a C_i that is not
 *                 finite: the keyframe has no centre, reported as three NaN, and its observations are skipped below.
 *   observations  read like the cull and mo_map_track read them, in stored order; usable = valid and at a keyframe with a centre.
 *   per usable observation at keyframe k: d = X - C_k (X: the point's f32 position), dist = sqrt(dx dx + dy dy + dz dz).
 *   reference     the first usable observation: ref_pos = its position, ref_octave = the octave of its keypoint,
 *                 max_dist = dist_ref * s(ref_octave), rounded to f32.  (ORB-SLAM2's mpRefKF, which also passes to the next observation
 *                 when a keyframe goes.)  None: ref_pos = -1, ref_octave = 0, max_dist = 0.
 *   normal        the usable observations with dist > 0 counted in n_valid: sum of (dx / dist, dy / dist, dz / dist) in stored order,
 *                 each component divided by n_valid and rounded to f32 (0 when n_valid = 0).  Not renormalised, as in ORB-SLAM2: its
 *                 length says how much the viewing directions agree, and the angle test below relies on that.
 *   min_dist      f32(max_dist) / s(n_levels - 1), rounded to f32; wherever it is needed it is derived from the stored f32 max_dist.
 *   A point with max_dist = 0 (no usable observation, or standing in its reference centre) is never a candidate of the searches below.
 *   An empty map: nothing is written.  No keyframes: every point reports "none".  Never an error. */
typedef struct {
    double scale_factor;     /* (1.2) */
    int32_t n_levels;        /* pyramid levels of the extractor, >= 1 (8) */
} mo_map_view_params;
typedef struct {
    /* caller-allocated, may be NULL; n = map points, n_kf = keyframes */
    float* normal;           /* [n][3] */
    float* min_dist;         /* [n] */
    float* max_dist;         /* [n] */
    int32_t* ref_pos;        /* [n] keyframe position of the reference observation (-1: none) */
    int32_t* ref_octave;     /* [n] */
    int32_t* n_valid;        /* [n] observations summed in normal */
    double* centre;          /* [n_kf][3] by keyframe position (NaN: no centre) */
    /* filled by the call */
    int64_t n_points;
    int32_t n_kf;
} mo_map_view_out;
int mo_map_point_views(mo_map*, const mo_map_view_params*, mo_map_view_out*);

/* The frustum mode: mo_map_track / mo_map_track_covisible (lprm NULL / given) and mo_map_fuse as documented above, with three changes.
 * Behind k_trk_rep the view record {normal, max_dist} (f32, 16 bytes) of every local point is computed as mo_map_point_views computes
 * it, with the call's scale_factor.
 *   frustum       of point X with its record, seen from the camera centre C: PO = X - C, dist = sqrt(POx POx + POy POy + POz POz),
 *                 max = f32 max_dist, min = max / s(n_levels - 1).  The point is NOT searched when dist is not > 0, max is not > 0,
 *                 dist < range_lo * min, dist > range_hi * max, or POx nx + POy ny + POz nz < min_cos * dist.
 *                 C of a tracking pass = -R^T t of the pass pose: C_j = -(R[0][j] t0 + R[1][j] t1 + R[2][j] t2); C of a fusion target =
 *                 its centre above (a target without a centre searches nothing).
 *   level         L = the smallest L >= 0 with dist * s(L) >= max, at most n_levels - 1: ORB-SLAM2's ceil(log(max / dist) /
 *                 log(scale_factor)) clamped to [0, n_levels - 1], without a logarithm.
 *   (1) candidates  must also pass the frustum test: pass_cand / n_cand count those; pass_in_image counts the plain candidates.
 *   (2) radius      r = radius * s(L) in place of s(ref_octave).
 *   (3) octave gate L - 1 <= octave <= L in place of |octave - ref_octave| <= 1.
 * The ratio rule, max_dist, claims, the retry, the refinement, fusion's chi2 gate, owners, components and merged lists are unchanged.
 * Not restated from ORB-SLAM2: the 2.5 / 4.0 radius factor by viewing cosine, the "same level" condition of the ratio test.  The
 * mnVisible / mnFound counters are mo_map_note_tracking's (below): the searches themselves stay read-only.
 * One synchronisation per call, no host round trip, integer atomics only: equal maps give equal bytes. */
typedef struct {
    int32_t n_levels;        /* pyramid levels of the extractor, >= 1 (8) */
    double range_lo;         /* (0.8) */
    double range_hi;         /* (1.2) */
    double min_cos;          /* (0.5: within 60 degrees of the mean viewing direction) */
} mo_map_frustum_params;
typedef struct {
    /* caller-allocated, may be NULL; n_q = keypoints of the frame */
    int32_t* level;          /* [n_q] predicted level of the point matched to each keypoint by the last pass searched (-1: none) */
    /* filled by the call */
    int32_t pass_in_image[4];/* plain candidates of each pass (of its last attempt): projections inside the image */
} mo_map_frustum_out;
int mo_map_track_frustum(mo_map*, const mo_frame_ref* f, const double K[9], const double pose0[12], const mo_map_track_params*,
                         const mo_map_local_params* local_or_null, const mo_map_frustum_params*, mo_map_track_out*,
                         mo_map_local_out* local_out_or_null, mo_map_frustum_out*);
int mo_map_fuse_frustum(mo_map*, const mo_map_fuse_params*, const mo_map_frustum_params*, mo_map_fuse_out*);

/* ---- The life of a map point: found / visible counters, culling by ORB-SLAM2's rule, an exact erase (map_ptcull.hip) -------------------
 * Opt-in: no call above returns anything different, mo_map_add_keyframe's own cull is unchanged.  tests/ptcull_restatement.py restates all
 * of it in numpy.
 *
 * The life record: int32 {visible, found, born, 0} per map point, part of the store (ORB-SLAM2's mnVisible, mnFound, mnFirstKFid).
 *   ordinal       the k-th keyframe mo_map_add_keyframe stores has ordinal k, from 0 (ORB-SLAM2's mnId).  Removing or erasing keyframes
 *                 never changes ordinals.  now = the ordinal of the last stored keyframe, 0 on a map without keyframes.
 *   created       {1, 1, now, 0}: by the growth step of mo_map_add_keyframe (now = the ordinal of the keyframe being added), by mo_map_grow
 *                 and by mo_map_add_points.
 *   carried       every call that rebuilds the store (mo_map_add_keyframe's cull, mo_map_add_observations, mo_map_erase_keyframes,
 *                 mo_map_fuse, mo_map_loop_correct, mo_map_erase_points, capacity growth) moves the record with its point, byte for byte.
 *   merged        the survivor of a component of mo_map_fuse / mo_map_loop_correct takes visible = the sum of its members' visible and
 *                 found = the sum of their found, formed in int64 and clamped to INT32_MAX, and keeps its own born (MapPoint::Replace).
 *   mo_map_point_life copies the records ([n][4]) and now.  The record is not a field of mo_map_download.
 *
 * mo_map_note_tracking: one tracked frame recorded; mo_map_track* stay read-only, this call takes what they returned.
 *   local         point i has a valid observation at a local position: one of the last `window` positions (0: all), or, with local_mask
 *                 (host [n_kf]), a position whose byte is not zero.
 *   seen[i]       i is local and its projection under P = K [R | t] lies in front of the camera and inside [0, w) x [0, h), as mo_map_track
 *                 decides a candidate; with `frustum`, it also passes the frustum test above from C = -R^T t, its view record computed as
 *                 mo_map_track_frustum computes it (scale_factor, frustum->n_levels).
 *   matched[i]    some q in 0 .. n_q - 1 has point[q] == i (entries outside 0 .. n - 1 are ignored); hit[i]: some such q has inlier[q] != 0.
 *   update        once per point and call, whatever the number of q: visible += (seen || matched), found += hit, each saturating at
 *                 INT32_MAX.  No atomic touches a record: equal inputs give equal bytes.
 *   outputs       n_local, n_seen, n_matched, n_found (the points with hit).  One chain, one synchronisation.
 *   empty         no map points or no keyframes: MO_OK, zeros, nothing happens.
 *   errors        MO_ERR_ARG for NULL arguments, K or pose not finite, w or h <= 0, window < 0, a scale_factor that is not finite and > 0,
 *                 frustum parameters mo_map_track_frustum refuses.
 *
 * mo_map_points_bad: ORB-SLAM2's LocalMapping::MapPointCulling, stateless through born; read-only.
 *   age           now - born.  tested = max_age < 0 || age <= max_age (ORB-SLAM2 drops a point from its recent list once its age reaches 3:
 *                 with one cull per keyframe the same points are tested).
 *   n_obs         the positions at which the point has a valid observation; of several entries at one position the first counts.
 *   reason 1      tested && (double)found < ratio * (double)visible, in f64: one product, one compare.
 *   reason 2      tested && not reason 1 && age >= min_age && n_obs <= max_obs.
 *   reason 3      neither of them && n_obs <= orphan_obs, whatever the age (-1: off).  This is what mo_map_erase_keyframes leaves behind.
 *   removed       reason != 0 && !(protect && protect[i]): a protected point reports its reason and stays.
 *   outputs       reason [n], removed [n] (u8, may be NULL), n_tested, n_removed, n_reason[4] (points per reason, 0: none), now.
 *   empty         no map points: MO_OK, nothing is written.  MO_ERR_ARG for NULL arguments, a ratio that is not finite, min_age < 0.
 *
 * mo_map_erase_points: the points with remove[i] != 0 (host [n]) leave; the map is the map the survivors alone would have built.
 *   survivors     in their order into the other copy of the store: every point field and the life record byte for byte, every observation
 *                 entry as stored, in entry order - entries that name nothing included.  remap[i] (may be NULL) = the new index, -1: removed.
 *   lists         the per-keyframe lists stay those of the last cull, as after mo_map_fuse.
 *   nothing       removed: the map keeps its bytes, remap is the identity.
 *   One synchronisation: the new counts.
 *
 * mo_map_cull_points: with erase = 0 mo_map_points_bad; with erase = 1 the decision and the erase of what it removed in one chain: the
 * scatter reads the flags on the device, the host learns the counts at the one synchronisation; remap is filled. */
typedef struct {
    int32_t w, h;            /* the image a projection must land in */
    int32_t window;          /* local positions, counted from the last (0: all); not used with local_mask (10) */
    double scale_factor;     /* > 0 (1.2): the view records of the frustum test */
    const uint8_t* local_mask;               /* host [n_kf] by position, non-zero: local; may be NULL */
    const mo_map_frustum_params* frustum;    /* may be NULL: the plain candidates count as seen */
} mo_map_note_params;
typedef struct {
    int32_t n_local, n_seen, n_matched, n_found;
} mo_map_note_out;
typedef struct {
    double ratio;            /* finite (0.25) */
    int32_t min_age;         /* >= 0 (2) */
    int32_t max_age;         /* < 0: every point is tested (3) */
    int32_t max_obs;         /* (2) */
    int32_t orphan_obs;      /* -1: off (1) */
    const uint8_t* protect;  /* host [n] by point, non-zero: never removed; may be NULL */
    int32_t erase;           /* mo_map_cull_points: 1 erases what was removed */
} mo_map_ptcull_params;
typedef struct {
    /* caller-allocated [n] each, may be NULL */
    uint8_t* reason;
    uint8_t* removed;
    int32_t* remap;          /* written by an erasing mo_map_cull_points */
    /* filled by the call */
    int32_t n_tested, n_removed;
    int32_t n_reason[4];
    int64_t now;
    int64_t n_points, n_obs; /* of the map after the call */
} mo_map_ptcull_out;
typedef struct {
    int32_t n_removed;
    int64_t n_points, n_obs; /* of the map after the call */
} mo_map_pterase_out;
int mo_map_point_life(mo_map*, int32_t* life /* [n][4] */, int64_t* now);
int mo_map_note_tracking(mo_map*, const double K[9], const double pose[12], const mo_map_note_params*, int32_t n_q, const int32_t* point,
                         const uint8_t* inlier, mo_map_note_out*);
int mo_map_points_bad(mo_map*, const mo_map_ptcull_params*, mo_map_ptcull_out*);
int mo_map_erase_points(mo_map*, const uint8_t* remove, int32_t* remap, mo_map_pterase_out*);
int mo_map_cull_points(mo_map*, const mo_map_ptcull_params*, mo_map_ptcull_out*);

/* ---- Snapshot: the whole state of a device map as host arrays, and a map made from them (map_snapshot.hip) -----------------------------
 * mo_map_export writes the map in a canonical form, mo_map_import makes a map from one; an imported map gives the bytes the exported one
 * gives, for every call above and for every later edit.  Additive: no call above launches anything different.
 *
 * The canonical form: keyframes in position order, their rows packed (no row stride, no dead slots).  It does not depend on capacities,
 * on which copy of the double-buffered store or lists is live, or on how often the store was regrown or restrided.
 *   dims          n_kf keyframes; kf_rows = sum of kf_cnt; n_pts, n_obs; list_rows and list_ids (rows and entries of the per-keyframe lists of
 *                 the last cull; list_off has list_rows + 1 entries, none when list_rows == 0); kf_stored = keyframes ever stored (the
 *                 ordinal counter: mo_map_point_life's now is kf_stored - 1, 0 on a map that never stored one); id_bound; the two keyframe
 *                 images' w, h, ch and bytes (= w * h * ch) and img_cur, the one mo_map_grow reads and the next mo_map_add_keyframe
 *                 colours its points from; st_live = the status words {points, observations, new points} that carry over between calls.
 *   keyframes     kf_cnt [n_kf]; kf_ord [n_kf] the ordinal of each (strictly increasing: positions keep creation order); kf_kps [kf_rows]
 *                 mo_keypoint; kf_desc [kf_rows][32]; kf_P [n_kf][12] f64.
 *   points        xyz [n_pts][3] f32, col [n_pts][3], id, dref_kf, dref_row [n_pts], obs_off [n_pts + 1], obs_kf, obs_kp [n_obs], life
 *                 [n_pts][4].  dref_kf of a point the library made is the ordinal of the keyframe its descriptor came from; the library
 *                 never reads dref_* and takes them as given.
 *   lists, images list_off, list_ids, kf_red [list_rows], img[2] [img_bytes].
 *   stale entries observation entries with negative keys, or positions or rows that do not exist, are state (every reader skips them): they
 *                 round-trip unchanged.
 *   not state     the spare slot, every scratch buffer, every feature's scratch, the keyframe database and the per-row words (after an
 *                 import every slot is stale by the serial rule: the next query recounts it), an attached vocabulary.
 *
 * mo_map_snapshot_dims: the sizes a caller allocates for (one 4-byte read from the device for list_ids).
 * mo_map_export: every array filled.  dims comes in as mo_map_snapshot_dims filled it, and the arrays are caller-allocated for its sizes;
 *   an array whose count is 0 may be NULL.  The keyframe rows are gathered from the slot-strided store by one launch for the keypoints
 *   and one for the descriptors, everything else is one copy per array; one chain on the context stream, one synchronisation.  The map
 *   is read, never changed.  Dims that are not the map's return MO_ERR_CAPACITY, and the arrays then hold nothing to rely on.
 * mo_map_import: a new map in *out with capacities the larger of what is asked (as mo_map_create) and what the snapshot needs; slots ==
 *   keyframes afterwards (mo_map_sizes out[5] == out[0]: dead slots are shed), ordinals and now are the snapshot's.  The snapshot is
 *   checked on the host before anything is uploaded or launched (csrc/snapshot.h lists every rule with the reader that needs it); a
 *   violation returns MO_ERR_ARG with the rule's text in mo_last_error, *out stays NULL, nothing leaks and the context stays usable. */
typedef struct {
    int32_t n_kf, list_rows;
    int64_t kf_rows, n_pts, n_obs, list_ids;
    int64_t kf_stored, id_bound;
    int32_t img_w[2], img_h[2], img_ch[2];
    int32_t img_cur;
    int32_t st_live[3];
    int64_t img_bytes[2];
} mo_map_snapshot_dims_t;   /* (the _t: C keeps typedefs and functions in one namespace, and the call below has the name) */
typedef struct {
    mo_map_snapshot_dims_t dims;
    int32_t* kf_cnt;
    int32_t* kf_ord;
    mo_keypoint* kf_kps;
    uint8_t* kf_desc;
    double* kf_P;
    float* xyz;
    uint8_t* col;
    int32_t* id;
    int32_t* dref_kf;
    int32_t* dref_row;
    int32_t* obs_off;
    int32_t* obs_kf;
    int32_t* obs_kp;
    int32_t* life;
    int32_t* list_off;
    int32_t* list_ids;
    int32_t* kf_red;
    uint8_t* img[2];
} mo_map_snapshot;
int mo_map_snapshot_dims(mo_map*, mo_map_snapshot_dims_t*);
int mo_map_export(mo_map*, mo_map_snapshot*);
int mo_map_import(mo_ctx*, const mo_map_snapshot*, int kf_slots, int kf_rows, int64_t pts_cap, int64_t obs_cap, mo_map** out);

/* ---- Absorb: one device map appended to another (map_absorb.hip, absorb.h) ----------------------------------------------------------------
 * mo_map_absorb appends src to dst on the device and src becomes dst's tail: the absorbed map is the later one, positions keep creation
 * order.  src is only read and stays usable.  Nothing aligns the two frames: that is the loop calls' work (LocalMapper.merge_map).
 * Additive: no call above launches anything different.  The contract: mo_map_export(dst) after the call equals, array for array and in
 * dims, tests/absorb_restatement.py applied to the exports of dst before and of src; the restated snapshot obeys csrc/snapshot.h.
 * With n_kf, n_slots, n_pts, n_obs, id_bound, kf_stored the counters of dst in front of the call:
 *   keyframes     src position k becomes dst position n_kf + k in the new slot n_slots + k.  Dead slots of src are shed, those of dst
 *                 stay.  Its ordinal becomes kf_stored + its ordinal in src.  The slot's serial is bumped: the keyframe database recounts
 *                 it by the lazy rule.  Count and rows are copied, the projection matrix byte for byte.  A src keyframe with more rows
 *                 than dst's row stride restrides dst's store first, as a wide frame does.
 *   points        src point i becomes dst point n_pts + i.  xyz, col and dref_row keep their bytes; id += id_bound; dref_kf >= 0 (an
 *                 ordinal) += kf_stored, dref_kf < 0 (the host's index into its injected dicts, never read here) -= dref_injected_shift;
 *                 life becomes {visible, found, born + kf_stored, 0}, born held at the new now (that binds only for a src that never
 *                 stored a keyframe: its points are then as old as dst's last keyframe, and born <= now stays true).  Consequence: now jumps by src's kf_stored, so the young points of
 *                 dst age past the young-point rules of mo_map_points_bad at once (max_age), as if that many keyframes had been stored.
 *   observations  entries keep their order; obs_off[n_pts + i + 1] = n_obs + src's obs_off[i + 1].  An entry that names a row of a src
 *                 keyframe (as every reader reads it: negative values from the end) is written normalised as (n_kf + position, row), both
 *                 non-negative.  An entry that names nothing in src is written as (INT32_MIN, its row value unchanged): it names nothing
 *                 in dst whatever is added later.  dst's own entries are not touched - their negative keys already change meaning
 *                 with every mo_map_add_keyframe, and do so here: a key -1 of dst names src's last keyframe afterwards.
 *   counters      kf_stored, id_bound, n_pts, n_obs and the live status words {points, observations} take the sums.  The third live
 *                 word (new points) stays dst's: its one reader, mo_map_add_keyframe, reads what its own chain wrote and clears it.
 *   images        when src has a keyframe, dst takes src's two keyframe images, their sizes and img_cur: the tail's image is the one the
 *                 next mo_map_add_keyframe colours from.
 *   lists         dst's per-keyframe lists and kf_red are untouched (list_rows stays): absorbed keyframes have no list row until the next
 *                 cull.
 *   dst's bytes   apart from a restride, no byte of dst's own keyframes, points or entries changes: everything is appended in place in
 *                 the live copy, the store is not flipped.
 *   errors        checked before anything is reserved or written, dst unchanged: MO_ERR_ARG for NULL arguments, src == dst, maps of
 *                 different contexts, dref_injected_shift outside 0 .. INT32_MAX; MO_ERR_CAPACITY for a sum past the snapshot's bounds
 *                 (n_pts, n_obs <= INT32_MAX / 2, id_bound <= 2^31, kf_stored <= INT32_MAX); MO_ERR_UNSUPPORTED for more than 65535
 *                 keyframes after the call.  A src without keyframes and without points is a complete no-op (no counter moves): MO_OK.
 *   chain         reserve, then on the context stream: one launch for the keypoint rows and one for the descriptor rows (slot-strided to
 *                 slot-strided, no staging; 16-byte units when both ends of a keyframe's run are aligned, else 4-byte units), one launch
 *                 over the points, one over the entries, the image copies; one synchronisation.  No atomics: equal inputs give equal
 *                 bytes.  Stage marks absorb_rows, absorb_points, absorb_obs.
 * out: the offsets that were applied (also on the no-op) and dst's counters after the call. */
typedef struct {
    int64_t dref_injected_shift;   /* subtracted from every negative dref_kf of src, >= 0 (the caller's count of injected dicts) */
} mo_map_absorb_params;
typedef struct {
    int32_t kf_offset, slot_offset;                             /* n_kf, n_slots of dst in front of the call */
    int64_t point_offset, obs_offset, id_offset, ordinal_offset; /* n_pts, n_obs, id_bound, kf_stored in front of the call */
    int64_t n_kf, n_slots, n_pts, n_obs, id_bound, kf_stored;   /* after the call */
} mo_map_absorb_out;
int mo_map_absorb(mo_map* dst, mo_map* src, const mo_map_absorb_params*, mo_map_absorb_out*);

/* ---- Place recognition: a binary vocabulary, the keyframe database of a map, relocalization with preselection (bow.hip) ----------------
 * "Which keyframes look like this frame": DBoW2's L1 score of tf-idf vectors over a flat vocabulary of binary words.  Everything is
 * integer work except the logarithm of the weights (host, once per training) and the one division of the score; tests/bow_restatement.py
 * restates every rule below in numpy and the device results equal it bit for bit.
 *   vocabulary    W words of 32 bytes and one int32 weight per word, 2 <= W <= MO_BOW_MAX_WORDS (8192).  The limit: the score kernel
 *                 keeps q_w of every word in LDS as one int32, 32 KB at 8192 words, so five workgroups still share a CU's 160 KB; the
 *                 histogram kernel's counters take the same.  Any W in range, not only multiples of 64.  0 <= weight <= 14 * 1024.
 *   quantisation  the word of a descriptor is the word with the lowest Hamming distance, ties to the lower word index (the matcher's
 *                 best neighbour with the words as train rows).
 *   training      mo_vocab_train: desc = host descriptors [n][32], img_off [n_img + 1] = the image (keyframe) boundaries as in obs_off
 *                 (img_off[0] = 0, img_off[n_img] = n, not decreasing).  MO_ERR_ARG unless n >= W, 1 <= n_img <= 2^20, iters >= 0.
 *                 Initial word j = training row floor(j * n / W) (int64).  An iteration quantises every row, then sets bit b of a word
 *                 to 1 iff 2 * (members with bit b set) > members; a word without members keeps its bits.  Training stops after `iters`
 *                 iterations or after the first one that changes no word (*iters_run = iterations run).  Duplicate words are allowed:
 *                 the higher index then has no members and stays.  n_w = the images with at least one row quantised to word w under
 *                 the final words (integers, on the device); weight_w = rint(log(n_img / max(n_w, 1)) * 1024) in f64 on the host
 *                 (n_img <= 2^20 keeps it <= 14 * 1024).  One synchronisation per iteration: training is offline.
 *   mo_vocab_create     a vocabulary from host arrays (words [W][32], weights [W]): a trained one survives the process as those two arrays.
 *   mo_vocab_download   the two arrays back (either may be NULL); mo_vocab_words: W.  mo_vocab_destroy: detach it from every map first.
 *   database      mo_map_set_vocabulary attaches a vocabulary to a map (NULL detaches; the map does not own it).  The database is dense:
 *                 one row of W term counts per keyframe slot and one for the spare slot a query frame is staged in.  A count is a
 *                 uint16: a count cannot exceed the rows of its frame, so frames and keyframes of up to MO_BOW_MAX_ROWS (65535) rows
 *                 never wrap one; a query on a frame, or with a keyframe not yet counted, of more rows returns MO_ERR_UNSUPPORTED.
 *                 Rows are made lazily: the keyframe store bumps a per-slot serial whenever mo_map_add_keyframe stores rows in a slot,
 *                 the database remembers the serial it counted, and a query first brings every stale slot up to date in one quantise
 *                 launch (one pair per stale keyframe, one for the frame) and one histogram launch.  Keyframes stored before the
 *                 vocabulary was attached, slots stored after mo_map_remove_keyframes and a store restrided between two queries are
 *                 all covered by that rule: rows are kept by slot, not by position, and do not depend on the store's row stride.
 *   query         mo_map_query_keyframes: the frame is given and staged like mo_map_track's; one chain, one synchronisation; reads the
 *                 map, never changes it.  With count_w the frame's term counts: q_w = count_w * weight_w, |q| = sum_w q_w (int64; k_w
 *                 and |k| likewise for keyframe k).  D_k = sum_w |q_w * |k| - k_w * |q||, int64: counts of a frame sum to <= 65535 and
 *                 weights are <= 14336, so |q|, |k| < 2^30, every term < 2^60 and D_k <= 2 |q| |k| < 2^61.
 *                 score_k = 1.0 - 0.5 * (double)D_k / ((double)|q| * (double)|k|), exactly those f64 operations; 0 when either norm is 0.
 *                 (DBoW2's L1 score of the L1-normalised vectors, 1 - 0.5 * sum |q/|q| - k/|k||, the weights fixed in the vocabulary.)
 *                 Result: the keyframe positions with score > 0, highest first, ties to the lower position, at most n_best; pos = -1
 *                 and score = 0 past n.  An empty frame, a map without keyframes and n_best = 0 give n = 0 and are not errors;
 *                 MO_ERR_ARG without a vocabulary.  Stage marks bow_quantise, bow_hist, bow_score, bow_rank (mo_stage_times).
 *   mo_map_relocalize_pre   mo_map_relocalize with one difference: when n_pre < the number of keyframes, the frame is matched only
 *                 against the keyframes the query above ranks in its first n_pre places (those with score > 0: fewer than n_pre when
 *                 fewer score above 0, none when none does); |C_k| = 0 for every other keyframe.  The selection stays on the device: the
 *                 rank kernel writes the matcher's pair list, and there is still one synchronisation.  When n_pre >= the number of
 *                 keyframes every keyframe is matched and the result is mo_map_relocalize's, byte for byte.  Everything after the
 *                 matching is mo_map_relocalize's own body.  MO_ERR_ARG for n_pre < 1 or without a vocabulary. */
#define MO_BOW_MAX_WORDS 8192
#define MO_BOW_MAX_WEIGHT (14 * 1024)
#define MO_BOW_MAX_ROWS 65535
#define MO_BOW_MAX_IMAGES (1 << 20)
typedef struct mo_vocab mo_vocab;
typedef struct {
    int32_t n_best;          /* places asked for, >= 0 (10) */
} mo_map_query_params;
typedef struct {
    /* caller-allocated */
    int32_t* pos;            /* [n_best] keyframe positions in rank order (-1 past n) */
    double* score;           /* [n_best] their scores (0 past n) */
    /* filled by the call */
    int32_t n;               /* places filled */
    int32_t from_token;      /* 1: the frame was read from its resident slot */
} mo_map_query_out;
int mo_vocab_train(mo_ctx*, const uint8_t* desc, int32_t n, const int32_t* img_off, int32_t n_img, int32_t n_words, int32_t iters, mo_vocab** out,
                   int32_t* iters_run);
int mo_vocab_create(mo_ctx*, const uint8_t* words, const int32_t* weights, int32_t n_words, mo_vocab** out);
int mo_vocab_words(const mo_vocab*);
int mo_vocab_download(const mo_vocab*, uint8_t* words, int32_t* weights);
void mo_vocab_destroy(mo_vocab*);
int mo_map_set_vocabulary(mo_map*, mo_vocab*);
int mo_map_query_keyframes(mo_map*, const mo_frame_ref* f, const mo_map_query_params*, mo_map_query_out*);
int mo_map_relocalize_pre(mo_map*, const mo_frame_ref* f, const double K[9], const mo_map_reloc_params*, int32_t n_pre, mo_map_reloc_out*);

/* mo_map_relocalize_batch: n_frames frames relocalized against the map as it stands in one device chain (a directory of query images
 * against a saved map, the cameras of a rig after a tracking loss, the frames of one stream chunk behind a break); reads the map, never
 * changes it - but for what the single call does too: the keyframe store is grown first so that its row stride holds the widest frame.
 *   the rule      for every i, everything the call returns for frame i is what the matching single call returns for that frame alone on
 *                 the same map: mo_map_relocalize(m, &frames[i], K, &p, ...) with n_pre < 0, else mo_map_relocalize_pre(..., n_pre, ...).
 *                 Every integer equal, every double equal bit for bit.  The order, the company and the grouping of the frames change
 *                 nothing (the sampling stream is (seed, keyframe position, h): it does not depend on the frame).  One K and one
 *                 parameter set serve every frame.
 *   layout        frame i's per-keypoint rows start at i * stride, its candidate rows at i * max_candidates; rows past a frame's n are
 *                 not written.
 *   no work       n_frames = 0: nothing runs.  A frame without keypoints: ok = 0, no candidates, a NaN pose, the others go on.  A map
 *                 without keyframes: every frame gets those defaults.  None of these is an error.
 *   errors        MO_ERR_ARG for a NULL required pointer, n_frames outside 0 .. MO_RELOC_BATCH_MAX, a frame of more than `stride` rows,
 *                 n_pre = 0, n_pre >= 1 without a vocabulary, max_pairs < 0 and everything mo_map_relocalize refuses;
 *                 MO_ERR_UNSUPPORTED where mo_map_relocalize_pre returns it (MO_BOW_MAX_ROWS).  On MO_ERR_ARG nothing is written.  A token
 *                 that is no longer resident falls back to the frame's arrays.
 *   groups        the matcher's outputs are 17 bytes per (pair, row): the frames are processed in groups of whole frames, enqueued back
 *                 to back.  A group has at most max_pairs (frame, keyframe) pairs (0: 1 GiB of matcher output / (17 * row stride)), never
 *                 more than 65535, and always at least one frame.  mo_map_reloc_batch_plan is that rule on the host: pairs_per_frame =
 *                 the keyframes matched per frame (all of them, or n_pre when that is fewer), row = the store's row stride.
 * One chain on the context stream, one synchronisation (the copy-out).  Integer atomics only: equal inputs give equal bytes on every
 * run.  Stage marks rlb_stage, rlb_select, then per group rlb_match, rlb_candidates, rlb_p3p, rlb_refine (mo_stage_times; the marks past
 * the 16th of a call are dropped).
 * mo_map_query_keyframes_batch obeys the same rule against mo_map_query_keyframes: frame i's places are pos / score + i * n_best, n[i]
 * of them filled. */
#define MO_RELOC_BATCH_MAX 1024
typedef struct {
    mo_map_reloc_params p;
    int32_t n_pre;           /* < 0: every keyframe is matched (mo_map_relocalize); >= 1: mo_map_relocalize_pre's n_pre; 0: MO_ERR_ARG */
    int64_t max_pairs;       /* 0: the default budget; else the most (frame, keyframe) pairs matched per group */
} mo_map_reloc_batch_params;
typedef struct {
    /* caller-allocated; point and inlier may be NULL.  Frame i's rows start at i * stride. */
    int32_t stride;          /* rows per frame in point / inlier, >= every frame's n */
    int32_t* point;          /* [n_frames][stride] as mo_map_reloc_out.point */
    uint8_t* inlier;         /* [n_frames][stride] */
    int32_t* cand_pos;       /* [n_frames][max_candidates]  required, like every array below */
    int32_t* cand_score;     /* [n_frames][max_candidates] */
    int32_t* cand_inliers;   /* [n_frames][max_candidates] */
    double* pose;            /* [n_frames][12], NaN without a winner */
    int32_t* ok;             /* [n_frames] */
    int32_t* kf_pos;         /* [n_frames] */
    int32_t* n_cand;         /* [n_frames] */
    int32_t* n_corr;         /* [n_frames] */
    int32_t* n_inliers;      /* [n_frames] */
    int32_t* from_token;     /* [n_frames] */
    /* filled by the call */
    int32_t n_ok;            /* frames with ok = 1 */
    int32_t n_groups;        /* groups the frames ran in (0: nothing ran) */
} mo_map_reloc_batch_out;
int mo_map_relocalize_batch(mo_map*, const mo_frame_ref* frames, int32_t n_frames, const double K[9], const mo_map_reloc_batch_params*,
                            mo_map_reloc_batch_out*);
int mo_map_reloc_batch_plan(int32_t n_frames, int64_t pairs_per_frame, int32_t row, int64_t max_pairs, int32_t* frames_per_group, int32_t* n_groups);
int mo_map_query_keyframes_batch(mo_map*, const mo_frame_ref* frames, int32_t n_frames, const mo_map_query_params*, int32_t* pos, double* score,
                                 int32_t* n, int32_t* from_token);

/* ---- Tracking against the reference keyframe (map_trackref.hip) ---------------------------------------------------------------------------
 * mo_map_track_reference: the pose of a frame from its matches by appearance to ONE keyframe of the map (ORB-SLAM2's
 * TrackReferenceKeyFrame: SearchByBoW, the rotation-consistency check, PoseOptimization): what a tracker runs when it has no velocity
 * yet, or when the search by projection found too little.  It needs no good prior - pose0 only starts the refinement - and costs what a
 * tracking call costs.  Reads the map, never changes it; needs a vocabulary (MO_ERR_ARG without one); the frame is given and staged like
 * mo_map_track's.  One chain on the context stream, one synchronisation; integer atomics only: equal inputs give equal bytes.
 * tests/trackref_restatement.py restates every rule below in numpy.
 *   words         word[slot][row], the word of every keyframe row under the database's quantisation (lowest Hamming distance to a word,
 *                 ties to the lower word index), kept by keyframe slot beside the term counts and made by the same lazy rule (a stale
 *                 slot is quantised once, by the next call that needs it); the spare slot's are the staged frame's.  They survive a
 *                 regrow of the database and a restride of the keyframe store.  mo_map_keyframe_words brings the stale rows up to date
 *                 and copies the words of the keyframe at kf_pos (negative: from the end) to out [rows of that keyframe].
 *   buckets       the frame's rows grouped by word, ascending row order within a word (a stable counting sort): woff [W + 1], wrows [n].
 *   candidates    the rows r of the reference keyframe (kf_pos; negative counts from the end, -1 = the last keyframe; MO_ERR_INDEX out of
 *                 range) that have a map point p = point_of[kf_pos][r]: the lowest point with a valid observation of (kf_pos, r), the
 *                 table of mo_map_relocalize.  n_cand counts them.
 *   search        candidate r walks the bucket of word[r] with the keyframe row's own descriptor (not the point's representative): best =
 *                 the lowest Hamming distance (ties to the lower frame row), second = the next lowest distance; accepted when best <=
 *                 max_dist and, if a second exists, (double)best <= ratio * (double)second; the accepted candidate claims frame row bq
 *                 for its point: key[bq] = min(key[bq], best << 32 | p) - mo_map_track's search tail and conflict rule, unchanged.  It
 *                 records cq[r] = bq and cd[r] = best (-1, -1 when it claimed nothing).  n_claims counts the candidates that claimed.
 *   kf_row        of a claimed frame row q: the lowest candidate row r with cq[r] == q and (cd[r] << 32 | point_of[r]) == key[q].
 *   orientation   only when check_orientation != 0 (leave it off for keypoints without angles).  For every claimed q:
 *                 rot = (double)kf.angle[kf_row[q]] - (double)frame.angle[q]; if (rot < 0) rot += 360; bin = (int)rint(rot / 12.0);
 *                 if (bin >= 30) bin -= 30.  hist[30] counts the bins (a bin outside 0 .. 29 - angles outside [0, 360) - is counted
 *                 nowhere and is never kept).  The three highest bins, ties to the lower bin; the second is kept iff 10 * c2 >= c1, the
 *                 third iff the second is kept and 10 * c3 >= c1; a bin of count 0 is never kept.  Claims in any other bin are dropped.
 *                 (ORB-SLAM2's ComputeThreeMaxima over the 12-degree bins its histogram length of 30 intends.)  n_matches_raw counts the
 *                 claims before this stage, n_matches after it.
 *   pose          one pass of mo_map_track's refinement from pose0 over the matches, no retry: fewer than min_matches matches end the
 *                 call without a refinement (ok = 0, pose = pose0).  ok = the pass was refined and has >= min_inliers inliers.
 * An empty frame, a map without keyframes or points, a keyframe none of whose rows has a point: not ok, MO_OK.  A frame or keyframe above
 * MO_BOW_MAX_ROWS: MO_ERR_UNSUPPORTED.  Stage marks trackref_words, trackref_prep, trackref_search, trackref_orient, trackref_refine. */
typedef struct {
    int32_t kf_pos;            /* the reference keyframe's position; negative counts from the end (-1) */
    int32_t check_orientation; /* run the orientation stage (1) */
    double scale_factor;       /* scales the information of an octave (1.2) */
    double ratio;              /* best-to-second ratio (0.7) */
    double chi2;               /* outlier threshold; the Huber width is its square root (5.991) */
    int32_t max_dist;          /* ORB-SLAM2's TH_LOW (50) */
    int32_t min_matches;       /* fewer matches: no refinement (15) */
    int32_t min_inliers;       /* ok needs this many inliers (10) */
} mo_map_trackref_params;
typedef struct {
    /* caller-allocated, may be NULL; n_q = keypoints of the frame */
    int32_t* point;          /* [n_q] map point matched to each keypoint (-1: none) */
    int32_t* dist;           /* [n_q] its Hamming distance (-1: none) */
    uint8_t* inlier;         /* [n_q] final classification of the refinement (0 where it did not refine) */
    int32_t* kf_row;         /* [n_q] the row of the reference keyframe the match came from (-1: none) */
    /* filled by the call */
    double pose[12];         /* [R | t] row-major: the refined pose, else pose0 */
    int32_t n_cand, n_claims, n_matches_raw, n_matches, n_inliers;
    int32_t hist[30];        /* the orientation histogram (zeros when the stage did not run) */
    int32_t kept_bin[3];     /* the bins kept, highest first (-1: none) */
    int32_t ok;              /* 1: refined with >= min_inliers inliers */
    int32_t from_token;      /* 1: the frame was read from its resident slot */
} mo_map_trackref_out;
int mo_map_track_reference(mo_map*, const mo_frame_ref* f, const double K[9], const double pose0[12], const mo_map_trackref_params*,
                           mo_map_trackref_out*);
int mo_map_keyframe_words(mo_map*, int32_t kf_pos, int32_t* out);

/* ---- Loop candidates (map_loop.hip) --------------------------------------------------------------------------------------------------------
 * "Which old keyframe, if any, does this keyframe close a loop with, and which map points of the two correspond": ORB-SLAM2's
 * KeyFrameDatabase::DetectLoopCandidates on the keyframe database above and on mo_map_covisibility's matrix, then the map-point matching
 * that opens ComputeSim3.  Reads the map, never changes it.  Integer work and a fixed sequence of f64 operations:
 * tests/loop_restatement.py restates every rule below in numpy and the device result equals it bit for bit.
 * mo_map_loop_candidates: p = the asking keyframe position (kf_pos; -1: the last).  The database is brought up to date first by the
 * query's lazy rule (no frame is staged), then W = mo_map_covisibility's matrix is computed; count_k[w] and weight_w are the database's
 * term counts and the vocabulary's weights.
 *   connected(k)  the positions q != k with W[k][q] >= max(min_weight, 1).  There is NO fallback to "the single best neighbour" when none
 *                 reaches it (ORB-SLAM2's UpdateConnections keeps the best one then): such a keyframe is connected to nothing.
 *                 connected[q] = 1 for q in connected(p) and for p itself; n_connected = |connected(p)| (p not counted).
 *   score_k       mo_map_query_keyframes' D_k and score with keyframe p's own database row as the query (q_w = count_p[w] * weight_w).
 *   min_score     the lowest score_q over q in connected(p); 1.0 when connected(p) is empty (ORB-SLAM2's initial value).
 *   common_k      for k != p and k not in connected(p): the number of words w with weight_w > 0, count_p[w] > 0 and count_k[w] > 0; 0 for p
 *                 and for connected keyframes, which take no part below.  max_common = max_k common_k; 0: no candidates.  Counted in
 *                 the pass over the database rows that forms D_k.
 *   S             common_k > (4 * max_common) / 5 in integer division (ORB-SLAM2's int(maxCommonWords * 0.8f)).  n_scored = |S|.
 *   M             k in S with score_k >= min_score.  n_passed = |M|.
 *   group         of k in M: N_k = the n_best positions q != k with the largest W[k][q] among connected(k), ties to the later position
 *                 (mo_map_local_keyframes' K2 rule, in that rank order).  acc_k = score_k, then acc_k = acc_k + score_q for each q in
 *                 N_k that is in S, in rank order: plain f64 adds in exactly that order.  best_k = k, replaced by such a q whenever
 *                 score_q is strictly greater than the best score so far, walking the same order.
 *   retained      k in M with acc_k > 0.75 * max_{k in M} acc_k (one f64 multiply, a strict compare).
 *   candidates    the distinct best_k of the retained k, each with the largest acc_k that named it and its own score, ordered by that
 *                 acc, highest first, ties to the lower position.  n_found counts them all; the first max_cand are returned
 *                 (n_cand = min(n_found, max_cand)); cand = -1, acc = score = 0 past n_cand.
 *   group[c]      [n_kf] 1 at the candidate's position and at connected(candidate); all 0 past n_cand.
 *   matching      per returned candidate c, with p's rows as queries and c's rows as train rows: the matcher's knn-2, ties to the lower
 *                 train row, passing when (double)d0 < ratio * (double)d1; a train frame of one row passes its only neighbour, one of
 *                 no rows matches nothing (mo_map_relocalize's behaviour).  cur_point[i] = the lowest map point with a valid
 *                 observation (p, i) (mo_map_relocalize's point_of), -1: none; the candidate's rows are looked up the same way.  A
 *                 passing match i -> j counts when a = cur_point[i] >= 0, b = point_of(c, j) >= 0 and a != b.  When several query rows
 *                 name the same train row j, the one with the lowest distance keeps it, ties to the lower query row; the others get -1.
 *                 match_point[c][i] = b, match_row[c][i] = j of the rows kept, -1 elsewhere; n_match[c] = the rows kept.
 *                 cur_point is written when it is given or max_cand > 0.
 *   chain         database update, k_covis, score and common words, selection (one workgroup, any number of keyframes), point_of,
 *                 matcher, gather, copy-out on the context stream; one synchronisation.  The selection kernel writes the matcher's
 *                 pair list on the device (pairs past n_cand name the empty frame): no host round trip between candidates and matching.
 *                 Stage marks bow_quantise, bow_hist, covis, loop_score, loop_select, loop_match, loop_gather (the last two only when
 *                 something is matched or cur_point is asked for).
 *   errors        MO_ERR_ARG for NULL params or out, kf_pos outside -1 .. n_kf - 1, n_best < 0, max_cand outside 0 .. 16, ratio not in
 *                 (0, 1], and without a vocabulary; MO_ERR_UNSUPPORTED as for the query on a keyframe of more than 65535 rows.  A map
 *                 without keyframes: MO_OK, every count 0, min_score 1.0.  max_cand = 0 is legal: the counts and min_score are
 *                 returned, nothing is matched.
 * Integer atomics only (minima and maxima commute): two calls on equal maps give the same bytes. */
typedef struct {
    int32_t kf_pos;      /* the keyframe that asks, by position; -1: the last */
    int32_t min_weight;  /* q is connected to p when W[p][q] >= max(min_weight, 1) (15) */
    int32_t n_best;      /* covisible neighbours a candidate's group score takes, >= 0 (10) */
    int32_t max_cand;    /* candidates returned and matched, 0 .. 16 (4) */
    double  ratio;       /* Lowe ratio of the matching (0.75) */
} mo_map_loop_params;
typedef struct {
    /* caller-allocated; any may be NULL */
    int32_t* cand;        /* [max_cand] candidate positions, -1 past n_cand */
    double*  acc;         /* [max_cand] accumulated group score */
    double*  score;       /* [max_cand] the candidate's own score against p */
    uint8_t* connected;   /* [n_kf] 1: connected to p (p itself included) */
    uint8_t* group;       /* [max_cand][n_kf] 1: the candidate or connected to it */
    int32_t* cur_point;   /* [rows of p] map point of each keypoint row of p, -1: none */
    int32_t* match_point; /* [max_cand][rows of p] the candidate's map point matched to that row, -1 */
    int32_t* match_row;   /* [max_cand][rows of p] its keypoint row in the candidate, -1 */
    int32_t* n_match;     /* [max_cand] */
    /* filled by the call */
    int32_t n_cand, n_found;   /* n_found: distinct candidates before the cut at max_cand */
    int32_t n_connected, max_common, n_scored, n_passed;
    double  min_score;
} mo_map_loop_out;
int mo_map_loop_candidates(mo_map*, const mo_map_loop_params*, mo_map_loop_out*);
/* mo_map_loop_candidates_among: the candidates among a given keyframe set only (the merge of two maps asks one side about the other: an
 * unrelated keyframe of the asking side would otherwise outscore the true match and push it under the retain test).  among: [n_kf] on the
 * host, or NULL, which behaves as mo_map_loop_candidates.  One added rule: common_k = 0 where among[k] == 0; such a keyframe takes no part
 * in S, M, the group sums or the candidates, exactly like a connected one.  connected, min_score and every other rule are unchanged.  The
 * mask is applied by one [n_kf] launch between the score and the selection (stage mark loop_among); the kernels of the plain call are
 * the same code and the plain call launches what it launched. */
int mo_map_loop_candidates_among(mo_map*, const mo_map_loop_params*, const uint8_t* among /* [n_kf] */, mo_map_loop_out*);

/* ---- Loop alignment (map_sim3.hip, sim3.h) ------------------------------------------------------------------------------------------------
 * "Is the candidate the same place, and at which relative scale": ORB-SLAM2's ComputeSim3 on the correspondences
 * mo_map_loop_candidates returned - a 3-point RANSAC over Horn's closed form, then Gauss-Newton on sim(3).  Reads the map, never changes
 * it.  The consistency bookkeeping of a loop detector sits between the two calls on the host, so the match lists come back in as host
 * arrays; any list of the same shape may be given.  tests/native/sim3_replay.cpp restates the chain from the pairs on over the same
 * sim3.h; integers are equal, models agree to the rounding of exp / sin / cos.
 * mo_map_loop_sim3: p = kf_pos, the asking keyframe; poses [n_kf][12] are the keyframes' [R | t] (mo_map_bundle_adjust's convention).
 *   model         X1 = s R X2 + t takes a point of the candidate's camera frame (2) into p's camera frame (1).
 *   pairs         of candidate c, in row order: the rows i of p with a = cur_point[i], b = match_point[c][i], j = match_row[c][i] all >= 0,
 *                 a and b map points that exist, j a row of the candidate.  Anything else is dropped.  n_corr[c] counts the pairs.
 *                 X1 = R1 xyz[a] + t1, X2 = R2 xyz[b] + t2 (f64, each row summed left to right); keypoints (p, i) and (cand[c], j) with
 *                 information = 1 / scale_factor^(2 octave) (repeated products from 1.0, negative octaves as 0: mo_map_track's).
 *   hypotheses    h = 0 .. n_hyp - 1 per candidate with at least 3 pairs: three distinct pairs drawn by the relocalization's sampler on
 *                 the stream (seed, cand[c]); Horn's closed form (symmetric 4x4 by cyclic Jacobi).  No model: a non-finite value, a
 *                 denominator or scale not > 0, or a largest eigenvalue not separated from the second (collinear or coincident points).
 *   inlier        a pair is an inlier when X2 taken into frame 1 has z > 0 and information1 * squared pixel error < chi2 against p's
 *                 keypoint, and X1 taken into frame 2 has z > 0 and information2 * squared pixel error < chi2 against the candidate's
 *                 (strict).  ORB-SLAM2 compares with the projections of the 3D points; here the keypoints are the measurement.
 *   best          per candidate the hypothesis with the most inliers, ties to the lower h: key (inliers << 32) | ~h, 0: no model.
 *   refinement    the best hypothesis re-solved, its inliers selected; then twice, while at least 3 inliers remain: at most 10
 *                 Gauss-Newton steps on (translation, rotation, log-scale) over both reprojection residuals of the inliers (points
 *                 fixed, information weights, Huber width sqrt(chi2); a step below 1e-12 or a normal matrix that is not positive
 *                 definite ends the round), then the inliers are selected again.
 *   outputs       per candidate scale, R, t (NaN without a model), n_corr, n_inliers, inlier [rows of p] (1 at the rows of final
 *                 inliers).  win = the candidate with a model and the most final inliers, ties to the earlier one in the given order,
 *                 -1: none; win_inliers its count; ok = win_inliers >= min_inliers.
 *   chain         uploads, gather (one workgroup per candidate, block scans), hypotheses (one wave each, all candidates in one launch),
 *                 refinement (one wave per candidate), winner, copy-out; one synchronisation.  Stage marks sim3_gather, sim3_hyp,
 *                 sim3_refine, sim3_finish.
 *   errors        MO_ERR_ARG for NULL params, out, K or poses, non-finite K or poses, kf_pos or a cand entry outside the map, n_cand
 *                 outside 0 .. 16, n_hyp outside 1 .. 2^20, chi2 not finite or < 0, scale_factor not finite or not > 0, and for NULL
 *                 cand / cur_point / match_point / match_row when n_cand > 0.  n_cand = 0 or a map without keyframes: MO_OK, win = -1,
 *                 ok = 0.
 * Integer atomics only (maxima commute): two calls on equal inputs give the same bytes. */
typedef struct {
    int32_t kf_pos;              /* the asking keyframe, by position */
    int32_t n_cand;              /* 0 .. 16 */
    const int32_t* cand;         /* [n_cand] candidate keyframe positions */
    const int32_t* cur_point;    /* [rows of p] mo_map_loop_candidates' cur_point */
    const int32_t* match_point;  /* [n_cand][rows of p] */
    const int32_t* match_row;    /* [n_cand][rows of p] */
    int32_t n_hyp;               /* 1 .. 2^20 (300) */
    int32_t min_inliers;         /* ok needs this many final inliers (20) */
    uint64_t seed;
    double chi2;                 /* 9.210 */
    double scale_factor;         /* of the information (1.2) */
} mo_map_sim3_params;
typedef struct {
    /* caller-allocated; any may be NULL */
    double*  scale;       /* [n_cand] */
    double*  R;           /* [n_cand][9] */
    double*  t;           /* [n_cand][3] */
    int32_t* n_corr;      /* [n_cand] */
    int32_t* n_inliers;   /* [n_cand] */
    uint8_t* inlier;      /* [n_cand][rows of p] */
    /* filled by the call */
    int32_t win, ok;      /* win: index into cand, -1: none */
    int32_t win_inliers;  /* n_inliers of the winner (the array above holds every candidate's) */
} mo_map_sim3_out;
int mo_map_loop_sim3(mo_map*, const double K[9], const double* poses, const mo_map_sim3_params*, mo_map_sim3_out*);

/* ---- Loop confirmation (map_confirm.hip) ----------------------------------------------------------------------------------------------------
 * "Which map points of the loop side does each keypoint of the asking keyframe correspond to": the second half of ORB-SLAM2's
 * ComputeSim3 - SearchBySim3 guided by the similarities mo_map_loop_sim3 found, OptimizeSim3 on the larger set, SearchByProjection of
 * the loop keyframe's neighbourhood - and its acceptance rule (40 matches).  Reads the map, never changes it.  tests/confirm_restatement.py
 * restates every rule but the refit in numpy, tests/native/confirm_replay.cpp the refit over the same sim3.h; integers are equal, models
 * agree to the rounding of exp / sin / cos.
 * mo_map_loop_confirm: p = kf_pos; K, poses, cand, cur_point, match_point, match_row as for mo_map_loop_sim3; scale / R / t its models
 * (X1 = s R X2 + t), inlier its flags (NULL: every listed row counts as flagged), group mo_map_loop_candidates' (NULL: the candidate alone).
 *   take part     a candidate whose model has a non-finite entry or a scale not > 0 takes no part: n_pairs = n_guided = n_inliers = 0, its
 *                 model out is NaN, fwd / bwd -1.  Not an error.
 *   representatives  L = p, every candidate, every keyframe of every group.  Every point with a valid observation in L has
 *                 mo_map_track's representative descriptor rep and ref_octave (over all its valid observations); other points take part
 *                 in nothing below.
 *   seeds         of candidate c: the rows i of p that mo_map_loop_sim3 would pair (a = cur_point[i], b = match_point[c][i] points that
 *                 exist, j = match_row[c][i] a row of the candidate) with inlier[c][i] != 0.  When several such rows name one j, the
 *                 lowest i is the seed; the others are no seeds.  Row i of p and row j of c of a seed are taken.
 *   guided search per candidate, both ways.  1 -> 2: every row i of p that is not taken with a = cur_point[i] a point that exists and
 *                 has a representative: X1 = R1 xyz[a] + t1 (f64, each row summed left to right), Y = S21 X1 (S21 = the inverse as
 *                 mo_map_loop_sim3 forms it, Y[d] = s21 * (row d of R21 . X1) + t21[d]), pixel = K Y (rows summed left to right, two
 *                 divisions); a source when the third row is > 0 and the pixel lies in [0, w) x [0, h).  Among the candidate's rows that are not taken,
 *                 with |dx| < r and |dy| < r, r = radius_guided * scale_factor^ref_octave[a] (repeated products), and octave within 1 of
 *                 ref_octave[a]: the lowest Hamming distance to rep[a], ties to the lower row, accepted when <= max_dist (no ratio
 *                 test).  fwd[c][i] = that row, else -1.  2 -> 1: every row j of c that is not taken with b = point_of(c, j) >= 0 having
 *                 a representative: X2 = R2 xyz[b] + t2, Y = S12 X2, the same search over p's rows that are not taken, with rep[b];
 *                 bwd[c][j] = the row of p, else -1.  A guided match is (i, j) with fwd[c][i] = j, bwd[c][j] = i and a != b.
 *                 Deviation from ORB-SLAM2: the octave is the representative observation's with a +-1 gate (mo_map_track, mo_map_fuse),
 *                 not a level predicted from the distance.
 *   refit         pairs of c = seeds and guided matches in row order of p, packed as mo_map_loop_sim3's pairs (b of a guided match is
 *                 point_of(c, j)); n_pairs, n_guided count them.  From the given model: mo_map_loop_sim3's inlier selection, then its
 *                 refinement rounds unchanged (twice, while at least 3 inliers remain: at most 10 Gauss-Newton steps, re-selection).
 *                 n_inliers = the final count, pair_inlier = 1 at the rows of final inliers.  Fewer than 3 pairs: the model out is the
 *                 model in, n_inliers = 0.
 *   winner        the candidate that takes part with n_inliers >= min_inliers and the most, ties to the earlier in the given order; -1:
 *                 none.  For its final inlier pairs loop_point[i] = b, source[i] = 1 (seed) or 2 (guided).
 *   projection    winner only.  Loop points: the points with a valid observation at a keyframe of group[win] (n_loop_points).  One is
 *                 skipped when it is the b of a final inlier pair or has a valid observation at p.  The others: X2 = R2 xyz[x] + t2 with
 *                 the winner's pose, Y = S12 X2 with the refined model, projected as above (n_proj_cand counts those in the image).
 *                 Over p's rows without a loop_point, |dx|, |dy| < radius_proj * scale_factor^ref_octave[x], octave within 1: the lowest
 *                 distance to rep[x], ties to the lower row, accepted when <= max_dist.  Per row the lowest (distance, x) wins, one
 *                 round, losers are not searched again: loop_point[i] = x, source[i] = 3 (n_proj counts them).  Deviation: ORB-SLAM2
 *                 hands out rows in list order; here the better match wins and the result does not depend on order.
 *   outputs       n_total = rows with a loop_point; ok = win >= 0 and n_total >= min_matches.  bwd is [n_cand][R2], R2 = the largest row
 *                 count among the candidates (at least 1).
 *   chain         uploads, point_of, representatives, keypoint grids (p and the candidates), seeds, guided search (one lane per source
 *                 row, grid.y = candidate x direction), pairs (one workgroup per candidate, block scans), refit (one wave per candidate),
 *                 winner, projection (one lane per map point), claims, copy-out; one synchronisation.  Stage marks confirm_prep,
 *                 confirm_seed, confirm_guided, confirm_pairs, confirm_refit, confirm_win, confirm_proj, confirm_claim.
 *   errors        as mo_map_loop_sim3 for the arguments they share; also MO_ERR_ARG for w or h < 1, radius_guided / radius_proj /
 *                 scale_factor not finite or not > 0, chi2 not finite or < 0, max_dist outside 0 .. 256, min_inliers or min_matches < 0,
 *                 NULL scale / R / t with n_cand > 0.  n_cand = 0 or a map without keyframes: MO_OK, win = -1, ok = 0, every count 0.  An
 *                 asking keyframe without rows or a map without points: MO_OK, nothing is searched, a model comes back as given.
 * Integer atomics only (minima, counts): two calls on equal inputs give the same bytes. */
typedef struct {
    int32_t kf_pos;              /* the asking keyframe, by position */
    int32_t n_cand;              /* 0 .. 16 */
    const int32_t* cand;         /* [n_cand] candidate keyframe positions */
    const int32_t* cur_point;    /* [rows of p] */
    const int32_t* match_point;  /* [n_cand][rows of p] */
    const int32_t* match_row;    /* [n_cand][rows of p] */
    const uint8_t* inlier;       /* [n_cand][rows of p] mo_map_loop_sim3's flags; NULL: all */
    const double*  scale;        /* [n_cand] mo_map_loop_sim3's models */
    const double*  R;            /* [n_cand][9] */
    const double*  t;            /* [n_cand][3] */
    const uint8_t* group;        /* [n_cand][n_kf] mo_map_loop_candidates' group; NULL: the candidate alone */
    int32_t w, h;                /* image size */
    int32_t max_dist;            /* 0 .. 256 (50) */
    int32_t min_inliers;         /* the winner needs this many final inliers (20) */
    int32_t min_matches;         /* ok needs this many loop points (40) */
    double radius_guided;        /* 7.5 */
    double radius_proj;          /* 10.0 */
    double chi2;                 /* 9.210 */
    double scale_factor;         /* 1.2 */
} mo_map_confirm_params;
typedef struct {
    /* caller-allocated; any may be NULL */
    double*  scale;        /* [n_cand] refined */
    double*  R;            /* [n_cand][9] */
    double*  t;            /* [n_cand][3] */
    int32_t* n_pairs;      /* [n_cand] */
    int32_t* n_guided;     /* [n_cand] */
    int32_t* n_inliers;    /* [n_cand] */
    uint8_t* pair_inlier;  /* [n_cand][rows of p] */
    int32_t* fwd;          /* [n_cand][rows of p] */
    int32_t* bwd;          /* [n_cand][R2] */
    int32_t* loop_point;   /* [rows of p] -1: none */
    uint8_t* source;       /* [rows of p] 0 none, 1 seed, 2 guided, 3 projection */
    /* filled by the call */
    int32_t win, ok;       /* win: index into cand, -1: none */
    int32_t win_inliers;
    int32_t n_loop_points, n_proj_cand, n_proj, n_total;
} mo_map_confirm_out;
int mo_map_loop_confirm(mo_map*, const double K[9], const double* poses, const mo_map_confirm_params*, mo_map_confirm_out*);

/* ---- Loop correction (map_correct.hip) ------------------------------------------------------------------------------------------------------
 * mo_map_loop_correct: a confirmed loop corrected on the map as it stands (the first half of ORB-SLAM2's LoopClosing::CorrectLoop): the
 * similarity is carried to the asking keyframe's neighbourhood, the neighbourhood's points and poses move, and the loop side's points
 * replace and absorb the neighbourhood's duplicates (SearchAndFuse).  The essential-graph optimisation is mo_map_pose_graph below, a call
 * of its own, and so is the global bundle adjustment behind it, mo_map_global_ba.  Opt-in: no other call runs it.  tests/correct_restatement.py restates every rule in numpy.  p = kf_pos; K, poses [n_kf][12] as for mo_map_loop_confirm; cand_pos the winning
 * candidate; scale, R, t its confirmed model, X_p = scale R X_cand + t in camera coordinates (mo_map_loop_sim3's convention); corrected
 * [n_kf]: non-zero at the keyframes that move; group [n_kf] (NULL: empty): non-zero at the old side, whose points are the loop points (a
 * point with a valid observation at a group position: mo_map_loop_confirm's rule; "valid" as for mo_map_fuse); loop_point [rows of p]:
 * mo_map_loop_confirm's output (NULL: all -1).  Rules, in this order:
 *   1 transform     S_cw' = S_pc o T_cand; A = S_cw'^-1 o T_p, of scale 1 / scale: the map-frame transform that takes the drifted side
 *                   onto the old side (the inverse of confirm's `world`).  In exact arithmetic ORB-SLAM2's per-keyframe
 *                   CorrectedSwi o NonCorrectedSiw is this same A for every corrected keyframe: one transform, no owner rule.  Formed
 *                   on the host in f64, each row summed left to right: Rq = R R_cand, tq = scale (R t_cand) + t, RA = Rq^T R_p,
 *                   tA = Rq^T (t_p - tq), A = (1 / scale) [RA | tA].  Returned in A [12] (3 x 4, row-major) and A_scale.
 *   2 poses         for every corrected position i: S_iw' = T_i o A^-1; the new pose is [R_i' | t_i' / scale] with R_i' = R_i RA^T and
 *                   t_i' = t_i - R_i' tA.  poses_out holds them, the other positions as given.  kP of those slots becomes
 *                   K [R_i' | t_i' / scale] (the product order of mo_map_bundle_adjust's write-back).
 *   3 moved points  a point with a valid observation at a corrected position and none at a group position moves to A (X, 1), computed in
 *                   f64 from the f32 store, each row summed left to right, rounded once to f32.  ORB-SLAM2 also moves a loop point that
 *                   a corrected keyframe happens to see; this call does not: the old side is the anchor.  moved [point] is per old index.
 *   4 direct        a row r of p with loop_point[r] = L in [0, points) (other values are skipped): when the owner of (p, r) is a point
 *                   o != L, {o, L} is a merge edge; when the row is free and L has no valid observation at p, L gains (p, r); when two
 *                   rows name one L, the lower row wins the gain and the other row stays free.
 *   5 search        pairs are every (loop point i, corrected position k) where i has no valid observation at k.  From there on,
 *                   under the new P of k, the candidate, search, claim and owner rules are mo_map_fuse's, word for word (projection, window
 *                   of radius * scale_factor^ref_octave, octave +-1, information * d^2 <= chi2, Hamming <= max_dist, claims by the lowest
 *                   (dist, i), owner = the lowest point with a valid observation of the row).  A row that rule 4 gave to a loop point
 *                   counts as owned by it.  More than 16384 corrected positions: MO_ERR_UNSUPPORTED.
 *   6 components    the connected components of the edges of rules 4 and 5.  Survivor: a loop point beats any other member; within that
 *                   the most valid observations, then the lowest index.  Merged lists, compaction into the other copy of the store and
 *                   `into` as mo_map_fuse states them; a member's gains are its gain of rule 4, then those of rule 5 by position.  The
 *                   survivor keeps its own xyz: for a loop point the unmoved one.
 *   7 nothing fuses (no edge, no gain, no proposal): moved xyz and kP are still written, in place in the live copy; the store is not
 *                   flipped and `into` is the identity.
 *   8 no work       an empty map or no keyframes: all counts 0, A the identity, poses_out = poses, MO_OK.  MO_ERR_ARG: kf_pos or
 *                   cand_pos out of range; corrected[kf_pos] == 0; a position in both masks; a scale that is not finite or <= 0;
 *                   non-finite R, t, K or poses; w or h <= 0; radius < 0; scale_factor <= 0; chi2 < 0.
 * Everything is decided on the device: one chain, one synchronisation.  Integer atomics only: two calls on equal inputs give equal bytes. */
typedef struct {
    int32_t kf_pos, cand_pos;
    double scale, R[9], t[3];
    const uint8_t* corrected;    /* [n_kf] */
    const uint8_t* group;        /* [n_kf], may be NULL */
    const int32_t* loop_point;   /* [rows of p], may be NULL */
    int32_t w, h;                /* image size */
    double radius;               /* 4.0 */
    double scale_factor;         /* 1.2 */
    int32_t max_dist;            /* 50 */
    double chi2;                 /* 5.991 */
} mo_map_correct_params;
typedef struct {
    /* caller-allocated; any may be NULL */
    double*  poses_out;          /* [n_kf][12] */
    int32_t* into;               /* [map points before the call] the new index of the point each old point now is */
    uint8_t* moved;              /* [map points before the call] */
    /* filled by the call */
    double A[12], A_scale;
    int32_t n_corrected, n_moved, n_loop_points, n_direct_edges, n_direct_gained, n_pairs, n_cand, n_proposals, n_gained, n_edges, n_absorbed;
    int64_t n_points, n_obs;     /* after the call */
} mo_map_correct_out;
int mo_map_loop_correct(mo_map*, const double K[9], const double* poses, const mo_map_correct_params*, mo_map_correct_out*);

/* ---- Essential-graph optimisation (map_posegraph.hip, posegraph.h) ------------------------------------------------------------------------
 * mo_map_pose_graph: the second half of ORB-SLAM2's LoopClosing::CorrectLoop, Optimizer::OptimizeEssentialGraph (monocular: the scale is
 * free): after mo_map_loop_correct moved one end of a loop, the error that is left sits at the edge of the corrected set; this call
 * spreads it along the trajectory.  Opt-in: no other call runs it.  tests/native/posegraph_replay.cpp is the whole call on the host,
 * tests/posegraph_restatement.py restates rule 1 in numpy.  A vertex is a similarity S_i = (s, R, t), X_cam = s R X + t, one per keyframe
 * position; delta = (rho, w, lambda) moves it as mo_map_loop_sim3's refinement does: s' = e^lambda s, R' = exp(w) R,
 * t' = e^lambda exp(w) t + rho.  An edge (a, b), a < b, carries M_ba, which should equal S_b o S_a^-1; its residual is the 7-vector
 * (t_E, log R_E, ln s_E) of E = M_ba o S_a o S_b^-1, its information the identity.
 * poses [n_kf][12]: [R | t] of every position before the correction, at scale 1: the measurement source.  init [n_kf][13]: s, R [9], t [3]
 * per position: for a corrected keyframe T_i o A^-1 with its scale (mo_map_loop_correct's S_iw'), for every other its pose with s = 1.
 * fixed [n_kf]: non-zero at the positions that do not move; extra_a / extra_b [n_extra]: the loop connections and earlier loop edges.
 * Rules, in this order:
 *   1 edges       from the covisibility matrix W of the map as it stands (mo_map_covisibility's, so after the fusion).  parent[b], b >= 1:
 *                 the position a < b of the largest W[a][b], ties to the lowest; b - 1 when that weight is 0.  This is a stand-in for
 *                 ORB-SLAM2's spanning tree, which is maintained at keyframe insertion: it keeps the graph connected to position 0.
 *                 The edges are the unordered pairs {a, b} that are an extra edge (kind 0), else {parent[b], b} (kind 1), else have
 *                 W[a][b] >= min_weight (kind 2; min_weight < 1 counts as 1), less the pairs of two fixed positions; each once, ordered by
 *                 (a, b).  Measurement of an extra edge: S_b,init o S_a,init^-1 (its residual starts at 0, as ORB-SLAM2's loop edges do;
 *                 it is never measured from poses); of any other edge: T_b o T_a^-1 from poses.  More edges than 32 n_kf + n_extra:
 *                 MO_ERR_CAPACITY, nothing written.
 *   2 steps       Levenberg-Marquardt on the free vertices with mo_map_bundle_adjust's conventions: the diagonal of the normal equations
 *                 times (1 + lambda), lambda 1e-4 at the start; a step is accepted when the cost (the sum of the squared residuals)
 *                 falls, then lambda / 10, otherwise it is undone and lambda * 10.  The end: max_steps, a largest update below step_tol,
 *                 lambda > 1e8.
 *   3 solve       every step's linear system by block-sparse conjugate gradient from 0, preconditioned by the inverse of the damped 7x7
 *                 diagonal blocks (a block that is not positive definite holds its vertex for the step); it ends at
 *                 r.z <= cg_tol^2 r0.z0 or after max_cg iterations.  A truncated solve is legitimate: rule 2 accepts on the true cost.
 *   4 writes      when at least one step was accepted: every free position's pose becomes [R | t / s] and its kP K [R | t / s]
 *                 (mo_map_bundle_adjust's product order); a point whose reference - the position of its first valid observation in
 *                 list order - is free becomes S_r,final^-1 (S_r,init X), computed in f64 and rounded once to f32.  A point without a
 *                 valid observation or with a fixed reference keeps its bytes.  No observation or point is added or removed.
 *   5 no work     an empty map, one keyframe, no free position, max_steps = 0, no accepted step: nothing is written, ok = 0 (the first
 *                 three: every count 0 and the output arrays untouched).  MO_ERR_ARG: no fixed position; non-finite poses, init or K;
 *                 a scale of init <= 0; an extra edge out of range or with a == b; max_steps outside 0 .. 100; max_cg < 1; a negative
 *                 tolerance.  The int32 and n_kf^2 guards of mo_map_covisibility apply.
 * Everything is decided on the device: one chain, one synchronisation.  No floating-point atomics, every sum a fixed tree: two calls
 * on equal inputs give equal bytes.
 * poses_out [n_kf][12]: [R | t / s] of every position's final similarity (the initial one where nothing moved); sim3_out [n_kf][13];
 * edge_a / edge_b / edge_kind: the first edge_cap edges (n_edges is the full count); moved [map points]; cost: before the first step and at the end
 * (0 when no step ran); cg_iters: the iterations of all solves. */
typedef struct {
    const uint8_t* fixed;        /* [n_kf] */
    const int32_t* extra_a;      /* [n_extra], may be NULL when n_extra is 0 */
    const int32_t* extra_b;
    int32_t n_extra;
    int32_t min_weight;          /* 100 */
    int32_t max_steps;           /* 20 */
    int32_t max_cg;              /* 200 */
    double cg_tol;               /* 1e-8 */
    double step_tol;             /* 1e-10 */
    double K[9];
} mo_map_pg_params;
typedef struct {
    /* caller-allocated; any may be NULL */
    double*  poses_out;          /* [n_kf][12] */
    double*  sim3_out;           /* [n_kf][13] */
    int32_t* edge_a;             /* [edge_cap] */
    int32_t* edge_b;             /* [edge_cap] */
    uint8_t* edge_kind;          /* [edge_cap] 0 extra, 1 parent, 2 covisibility */
    uint8_t* moved;              /* [map points] */
    int32_t  edge_cap;
    /* filled by the call */
    int32_t steps, accepted, cg_iters;
    int32_t n_free, n_fixed, n_edges, n_extra_used, n_moved, ok;
    double cost[2], lambda;
} mo_map_pg_out;
int mo_map_pose_graph(mo_map*, const double* poses, const double* init, const mo_map_pg_params*, mo_map_pg_out*);

/* ---- Global bundle adjustment (map_gba.hip, gba.h) -------------------------------------------------------------------------------------
 * mo_map_global_ba: the last link of ORB-SLAM2's loop closing, Optimizer::GlobalBundleAdjustemnt (monocular): the poses of all keyframes
 * that are not held fixed and every point with at least two observations are refined together.  mo_map_pose_graph spreads a loop's error
 * with identity information and drags the points behind their reference keyframes; this call puts the map back onto its reprojection
 * minimum.  Opt-in: no other call runs it.  The reduced camera system is never formed: Levenberg-Marquardt with the points eliminated,
 * each step's system solved by a block-Jacobi-preconditioned conjugate gradient whose operator is applied matrix-free over the edges, so
 * there is no limit of 16 free keyframes (mo_map_bundle_adjust keeps its own).  tests/gba_restatement.py restates the rules in numpy with
 * a dense solve.  K, poses [n_kf][12] as for mo_map_bundle_adjust.  Rules:
 *   1 edges       an edge = one valid observation, read as mo_map_bundle_adjust reads it; edges are numbered point by point in index
 *                 order, within a point in list order.  Problem points: the points with >= 2 edges.  A position with an edge to a
 *                 problem point takes part: fixed when fixed[pos] is non-zero, else free; fixed == NULL: position 0 only (ORB-SLAM2's
 *                 gauge: the scale is held only by the damping).  MO_ERR_ARG when the problem has points and no fixed position takes part.
 *                 n_free goes up to the number of keyframes, under the int32 guards of the other calls.
 *   2 cost        residual, information and the Huber cost of width sqrt(chi2) as in round 0 of mo_map_bundle_adjust.  One round of at
 *                 most max_steps steps (0 .. 100), no outlier round.  At the end every edge is classified (inlier: depth > 0 and
 *                 information * |e|^2 <= chi2) into edge_inlier and n_inliers: reported only, nothing is erased.
 *   3 one step    damping (every diagonal entry times (1 + lambda), lambda 1e-4 at the start, / 10 after an accepted step, * 10 after
 *                 a rejected one), acceptance on the true robust cost, the end at an update below step_tol or lambda > 1e8, and a point
 *                 whose V is not positive definite (held for the step) as in mo_map_bundle_adjust.  Per problem point: the damped V,
 *                 V^-1, g_p.  Per free keyframe k, over its edges in ascending edge order: the damped H_kk, b_k = g_k - sum W_e V^-1 g_p
 *                 and the preconditioner block M_k = H_kk - sum_e W_e V^-1 W_e^T (same-edge terms only), factored by 6x6 Cholesky; if M_k
 *                 is not positive definite the damped H_kk is factored instead; if that fails too the vertex is held for the step.
 *   4 solve       S x = b by preconditioned conjugate gradient from x = 0, S p = H p - W V^-1 W^T p in two passes: per point
 *                 q = V^-1 sum_e W_e^T p_kf(e) in edge order, per free keyframe y_k = H_kk p_k - sum_e W_e q_pt(e) in ascending edge order.
 *                 It ends at r.z <= cg_tol^2 r0.z0, after max_cg iterations, or when p.Sp is not positive and finite; the x so far is
 *                 used.  When that happens at iteration 0, or r0.z0 is not a finite number >= 0, the step counts as rejected (lambda * 10,
 *                 no test against step_tol).  A truncated solve is legitimate: rule 3 accepts on the true cost.  The points are
 *                 back-substituted as in mo_map_bundle_adjust.
 *   5 writes      when at least one step was accepted: xyz of every problem point (the f64 result rounded once to f32) and
 *                 P = K [R | t] of every free position (mo_map_bundle_adjust's product order).  Otherwise nothing is written.  Points and
 *                 keyframes outside the problem keep their bytes.  ok = the problem ran and n_inliers >= min_inliers.  An empty map, no
 *                 free position, no problem point or max_steps = 0: every count is 0, ok = 0, not an error.  MO_ERR_ARG: NULL arguments;
 *                 non-finite K or poses; scale_factor not finite and > 0; chi2 or a tolerance not finite and >= 0; max_steps outside
 *                 0 .. 100; max_cg < 1; the gauge of rule 1.
 *   6 determinism no floating-point atomics.  Per-point sums are serial in edge order; per-keyframe sums take the edges strided over the
 *                 lanes, each lane in order, then the wave's shuffle tree, then the waves in order; the dot products over 6 n_free use a
 *                 fixed assignment and tree.  Two calls on equal maps return equal bytes.  Integer atomics count (the keyframe-side
 *                 edge lists, which are then sorted).
 *   7 decisions   every decision is a flag in a result block that later kernels read first.  The host waits on that block after the
 *                 set-up, between steps and between chunks of 32 conjugate-gradient iterations, only to stop enqueuing: the results do
 *                 not depend on where it waits.
 * poses_out [n_kf][12]: the free ones refined, the rest as given; kf_state as mo_map_bundle_adjust's; edge_inlier [n_obs] per entry of
 * the observation arrays (0 skipped or outside the problem, 1 inlier, 2 outlier); points_out [n_pts][3]: f64 positions of the problem
 * points, NaN elsewhere; cost: the robust cost at the start and at the end; cg_iters: the iterations of all solves. */
typedef struct {
    const uint8_t* fixed;    /* [n_kf] non-zero: the position is held; NULL: position 0 only */
    int32_t max_steps;       /* 0 .. 100 (10) */
    int32_t max_cg;          /* 200 */
    double cg_tol;           /* 1e-8 */
    double step_tol;         /* 1e-10 */
    int32_t min_inliers;     /* ok needs this many inlier edges at the end (50) */
    double scale_factor;     /* of the information (1.2) */
    double chi2;             /* outlier threshold; the Huber width is its square root (5.991) */
} mo_map_gba_params;
typedef struct {
    /* caller-allocated, may be NULL */
    double* poses_out;       /* [n_kf][12] */
    int32_t* kf_state;       /* [n_kf] 0 outside the problem, 1 fixed, 2 free */
    uint8_t* edge_inlier;    /* [n_obs] */
    double* points_out;      /* [n_pts][3] */
    /* filled by the call */
    double cost[2];
    double lambda;           /* damping after the last step */
    int32_t n_free, n_fixed, n_points, n_edges, n_inliers;
    int32_t steps, accepted, cg_iters;
    int32_t ok;
} mo_map_gba_out;
int mo_map_global_ba(mo_map*, const double K[9], const double* poses, const mo_map_gba_params*, mo_map_gba_out*);

/* Status of the mo_dev_* calls enqueued since the last mo_dev_status: the kernels never fault on overflow, they clamp and
 * raise a bit.  Host entry points keep their own flag words (checked inside each call): interleaving them with mo_dev_* calls
 * neither clears nor pollutes this status.  Synchronises the context stream, copies the flag word to flags[0] (flags may be NULL; [1..3] reserved, 0)
 * and clears it.  bit 0 (1): a level's internal keypoint slot overflowed (response ties at the quota cut: retainBest keeps every
 * element that ties with the boundary; the slots grow eightfold when this status is read, so repeating the call succeeds after
 * at most a few rounds - host entry points repeat by themselves);
 * bit 1 (2): a frame produced more keypoints than `cap` - its rows are truncated to cap while d_counts[frame] holds the
 * number it needed (so d_counts can EXCEED cap: clamp before indexing, or retry with cap >= max(d_counts));
 * bit 3 (8): a pair had more than 4096 correspondences (rows longer than 4096 are fine, a pair's ratio-test survivors or kept
 * tracking matches beyond that are not): that pair gets no model (NaN pose, 0 points), the others are unaffected;
 * bit 2 (4): not raised any more (rounds 2 - 3: more than 2048 local maxima in one grid cell; such cells are now processed in rounds).
 * Returns MO_OK when no bit is set, MO_ERR_CAPACITY otherwise. */
int mo_dev_status(mo_ctx*, int32_t flags[4]);

/* per-stage device time of the last mo_dev_* call, measured with hipEvents on the context stream.
 * names: NULL-terminated array of stage names owned by the library; ms [n] filled. Returns n stages. */
int mo_stage_times(mo_ctx*, const char*** names, float* ms, int cap);
/* The same for the call `back` calls ago (0 = the last one, at most MO_TIMING_SLOTS - 1 = 63): the library keeps a ring of event
 * sets, one per call, so a caller can enqueue many calls back to back and read their stage times after a single synchronisation
 * instead of waiting for every call's last event (bench.py's timed region). */
int mo_stage_times_back(mo_ctx*, int back, const char*** names, float* ms, int cap);

/* Host-side clock of the last single-call host entry point (mo_orb_detect_compute, mo_match_knn2_ratio, mo_track_pair, mo_init_two_view),
 * microseconds: us[0] entry -> everything enqueued (staging copies, launches), us[1] the wait for the stream, us[2] unpacking into
 * the caller's arrays, us[3] the whole call.  With mo_stage_times (device spans incl. the "h2d" / "d2h" copies) this is the batch-1
 * latency breakdown bench.py reports (single_frame_ms.breakdown). */
int mo_host_times(mo_ctx*, double us[4]);
/* Stage events inside the single-call host entry points (off by default: an event between two kernels idles the GPU for ~ 4.5 us,
 * five of them were 9 % of a single-frame extraction; the mo_dev_* calls always record theirs).  on != 0: mo_stage_times reports the
 * spans of the next host calls ("h2d", the kernel stages, "d2h"). */
int mo_set_host_timing(mo_ctx*, int on);

/* internal-stage probes used by the parity tests (device pipeline, host in/out) */
/* blurred: bit 0 = the blurred level instead of the raw one; bit 1 = through the single-frame kernel (pyramid + blur in one launch,
   the route of calls on one or two frames) instead of the batched path's kernels: MO_ERR_UNSUPPORTED for a geometry it does not cover */
int mo_dbg_pyramid_level(mo_ctx*, const mo_orb_params*, const uint8_t* gray, int w, int h, int level, int blurred,
                         uint8_t* out /* lw*lh */, int* lw, int* lh);
/* the blurred level `level` of frame `frame` as the last extraction on this context left it (no launch); resize_blur (may be NULL):
   1 when the plan lets the batched path's resize launches write the blurred levels (k_resize2's blurring form) */
int mo_dbg_blur_level(mo_ctx*, int frame, int level, uint8_t* out /* lw*lh */, int* lw, int* lh, int* resize_blur);
int mo_dbg_fast_level(mo_ctx*, const mo_orb_params*, const uint8_t* gray, int w, int h, int level,
                      int32_t* xys /* [cap][3] */, int cap, int* n);
int mo_dbg_min_eigen(mo_ctx*, const uint8_t* gray, int w, int h, float* eig /* [h*w] */);
/* byte 0..255: every device block the library allocates from now on is filled with it before its first use, and every scratch buffer -
   the pyramid buffers among them - is filled with it over its whole capacity at the start of every call: the context's and the plan's
   at every host and mo_dev_* entry point, a map's at every mo_map_* call on it, a stream lane's at every submit.  Scratch is what no
   call may read before its own chain wrote it; no result may move.  -1 (the default): off.  Either way the totals below start at 0. */
int mo_dbg_set_poison(mo_ctx*, int byte);
/* buffers and bytes filled since the last mo_dbg_set_poison (either may be NULL) */
int mo_dbg_poison_filled(mo_ctx*, int64_t* n_buffers, int64_t* n_bytes);
/* what the last mo_map_relocalize / mo_map_relocalize_pre on this map downloaded, per candidate in rank order (arrays of 64; entries past
   n_cand: cand -1, the rest 0 and a NaN pose): cand = keyframe position, best = the winning hypothesis' key (inliers << 32) |
   ~(h * 4 + root), 0: no pose had an inlier; ncorr = |C_k|; ninl = final inliers; pose[c][12] = the refined [R | t] (NaN without a key).
   Read from the call's pinned result block: no launch, no copy from the device, no synchronisation.  MO_ERR_ARG when no
   relocalization has finished its chain on the map (a call that found nothing to match - no keyframe, no keypoint - runs none). */
int mo_dbg_map_reloc_last(mo_map*, int32_t* n_cand, int32_t* cand /* [64] */, uint64_t* best /* [64] */, int32_t* ncorr /* [64] */,
                          int32_t* ninl /* [64] */, double* pose /* [64][12] */);
/* what the last mo_map_loop_sim3 on this map downloaded, per candidate in the given order (arrays of 16; entries past n_cand: cand -1, the
   rest 0 and a NaN model): best = the winning hypothesis' key (inliers << 32) | ~h, 0: no model; ncorr = the pairs; ninl = final
   inliers; model[c][13] = s, R [9], t [3] (NaN without a key); *win as the call returned it.  Read from the call's pinned result block:
   no launch, no copy from the device, no synchronisation.  MO_ERR_ARG when no alignment has finished its chain on the map (a call
   with n_cand = 0 or on a map without keyframes runs none). */
int mo_dbg_map_sim3_last(mo_map*, int32_t* n_cand, int32_t* win, int32_t* cand /* [16] */, uint64_t* best /* [16] */, int32_t* ncorr /* [16] */,
                         int32_t* ninl /* [16] */, double* model /* [16][13] */);
int mo_dbg_retain_best(mo_ctx*, const float* resp, int n, int n_points, int select_order, int32_t* order, int* n_out);

#ifdef __cplusplus
}
#endif
#endif
