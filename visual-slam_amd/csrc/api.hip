// api.hip -- extern "C" entry points declared in include/vslam_amd.h.
// Host entry points stage their inputs into HBM, run the same device pipeline the batched mode uses, and
// copy the results back; there is no CPU implementation behind any of them.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"

// Flag words: kernels raise bits in c->flags_cur[0].  mo_dev_* calls point it at words 0..3 (accumulated until mo_dev_status reads
// and clears them); host entry points point it at words 4..7, which they clear before and check after their own kernels - a host
// call between mo_dev_frontend_batch and mo_dev_status neither erases nor inherits the pending device-call bits.
int mo_decode_host_flags(mo_ctx* c, int f0, int f1, const char* cap_msg) {
    if (f0 & 1) { c->tie_overflow = true; c->tie_levels = f1; return mo_fail(c, MO_ERR_CAPACITY, "internal per-level keypoint capacity exceeded (response ties)"); }
    if (f0 & 2) return mo_fail(c, MO_ERR_CAPACITY, cap_msg);
    return MO_OK;
}

extern "C" int mo_set_host_timing(mo_ctx* c, int on) {
    if (!c) return MO_ERR_ARG;
    c->host_timing = on != 0;
    return MO_OK;
}

extern "C" int mo_host_times(mo_ctx* c, double us[4]) {
    if (!c || !us) return MO_ERR_ARG;
    for (int i = 0; i < 4; i++) us[i] = c->host_us[i];
    return MO_OK;
}

static bool grow_fin_slots(mo_ctx* c, int levels);

static int check_flags(mo_ctx* c) {
    int f[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(f, mo_host_flags(c), sizeof(f), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return mo_decode_host_flags(c, f[0], f[1]);
}

extern "C" int mo_dev_status(mo_ctx* c, int32_t flags[4]) {
    if (!c) return MO_ERR_ARG;
    MO_ENTER(c);
    int f[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(f, c->d_flags, sizeof(f), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_flags, 0, 4 * sizeof(int), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (flags) { flags[0] = f[0]; flags[1] = f[1]; flags[2] = flags[3] = 0; }
    if (f[0] & 1) grow_fin_slots(c, f[1]);  // response ties overflowed a level's slot: the next call of the same shape rebuilds its plan with larger ones
    if (f[0] & 15) return mo_fail(c, MO_ERR_CAPACITY, "a capacity flag was raised by a mo_dev_* call (see mo_dev_status in vslam_amd.h)");
    return MO_OK;
}

// device pipeline on frames already resident as dense gray [batch][h][w]
int mo_run_extract(mo_ctx* c, const mo_orb_params* p, const uint8_t* d_gray, int w, int h, int batch,
                   mo_keypoint* d_kps, uint8_t* d_desc, int cap, int32_t* d_counts, int host_call) {
    int rc = mo_build_plan(c, p, w, h, batch);
    if (rc) return rc;
    if (cap < 1) return mo_fail(c, MO_ERR_ARG, "cap must be >= 1");
    // host calls check their own flag words before they return; mo_dev_* calls accumulate theirs until mo_dev_status
    c->flags_cur = host_call ? mo_host_flags(c) : c->d_flags;
    if (host_call == 1) HIPCHK(c, hipMemsetAsync(mo_host_flags(c), 0, 4 * sizeof(int), c->stream));  // (2: the upload kernel cleared them)
    // (mo_dbg_set_poison: the entry point filled d_pyr and d_blur with the rest of the scratch, and a plan built above came filled:
    //  whatever the margins skip must never reach a result)
    if (host_call) mo_stage_mark(c, "h2d");  // (the host call opened its event set before the upload)
    else mo_stage_begin(c);
    // margins of the levels nothing in this pipeline reads (see orb_launch_blur / orb_launch_pyramid)
    const int blur_margin = mo_blur_margin(c->plan.edge_threshold), pyr_margin = mo_pyr_margin(c->plan.edge_threshold);
    // (one frame of a host call: the finest level's FAST + selection on a second stream beside the pyramid and the other levels was
    //  measured in round 4 - no gain, level 1's chain is as long as level 0's: profiles/r04_ab_single_split.txt)
    if (batch <= MO_FS_MAX_BATCH && c->pb.fs_ok) {
        // one or two frames: pyramid and blur in ONE launch whose workgroups chain the levels of their own tile through LDS
        // (front_single.hip; the seven dependent resize launches + the blur were 62 of 202 us of a one-frame call)
        if ((rc = orb_launch_front_single(c, d_gray, batch, d_desc != nullptr))) return rc;
        mo_stage_mark(c, "pyramid");
        if (d_desc) mo_stage_mark(c, "blur");  // (inside the same launch: the stage keeps its name, its time is in "pyramid")
    } else {
        // with descriptors, the resize launch of level L also writes the blurred level L-1 where the plan allows it (k_resize2's
        // blurring form); the blur stage is then the last level alone, and the blurred levels' time shows under "pyramid"
        bool blurred = false;
        if ((rc = orb_launch_pyramid(c, d_gray, batch, c->plan.nlevels, pyr_margin, d_desc ? blur_margin : -1, &blurred))) return rc;
        mo_stage_mark(c, "pyramid");
        // the Gaussian blur only depends on the pyramid: in line, right behind it (an aux-stream fork beside FAST + selection gained <= 1 %
        // in the BATCHED mode in rounds 1 - 2 and was retired there: profiles/r02_ab_serial_blur.txt)
        if (d_desc) {
            const int nl = c->plan.nlevels;
            if ((rc = orb_launch_blur(c, d_gray, batch, nl, blur_margin, blurred ? nl - 1 : 0))) return rc;
            mo_stage_mark(c, "blur");
        }
    }
    if ((rc = orb_launch_fast(c, d_gray, batch))) return rc;
    mo_stage_mark(c, "fast_nms");
    if ((rc = orb_launch_select(c, d_gray, batch))) return rc;
    mo_stage_mark(c, "select_harris");
    if ((rc = orb_launch_describe(c, d_gray, batch, d_kps, d_desc, cap, d_counts))) return rc;
    mo_stage_mark(c, "angle_rbrief");
    return MO_OK;
}

// ORBExtractor.distribute_keypoints (reference extractor.py:85-144, the path Tracker.process_frame takes: tracker.py:87) for a whole
// batch of frames resident in HBM: min-eigenvalue map, the 64 per-cell corner picks, KeyPoint(x, y, 31) records of the corners
// orb.compute keeps, blur of level 0, descriptors at angle -1 - one launch per step for all frames.  d_kps / d_desc / d_counts receive
// the KEPT keypoints (record i belongs to descriptor row i, which is what the match / pose stages need); the reference's own list (all
// corners, misaligned with the rows whenever a corner lies in the border band) is in the optional d_grid_* outputs.
static int run_grid_extract(mo_ctx* c, const mo_orb_params* p, const mo_batch_io* io) {
    const int w = io->w, h = io->h, batch = io->batch, cap = io->cap;
    int rc = mo_build_plan(c, p, w, h, batch);
    if (rc) return rc;
    if (p->nfeatures < 64) return mo_fail(c, MO_ERR_ARG, "n_features must be >= 64 (8x8 grid)");
    if (cap < 1) return mo_fail(c, MO_ERR_ARG, "cap must be >= 1");
    const int per_cell = p->nfeatures / 64, slots = 64 * per_cell;
    const size_t B = (size_t)batch;
    Layout L;
    const size_t o_eig = L.take(B * w * h * sizeof(float)), o_xy = L.take(B * slots * 2 * sizeof(float)), o_n = L.take(B * 66 * sizeof(int)),
                 o_kb = L.take(B * 65 * sizeof(int32_t));
    if ((rc = c->d_tmp.reserve_exact(c, L.total))) return rc;
    float* d_eig = L.at<float>(c->d_tmp, o_eig);
    float* d_xy = io->d_grid_xy ? io->d_grid_xy : L.at<float>(c->d_tmp, o_xy);
    int* d_n = io->d_grid_n ? io->d_grid_n : L.at<int>(c->d_tmp, o_n);
    c->flags_cur = c->d_flags;
    mo_stage_begin(c);
    if ((rc = gftt_launch(c, io->d_gray, w, h, p->nfeatures, d_eig, d_xy, d_n, batch))) return rc;
    int32_t* d_kb = L.at<int32_t>(c->d_tmp, o_kb);
    if ((rc = gftt_records_launch(c, d_xy, d_n, per_cell, w, h, p->edge_threshold, io->d_kps, io->d_grid_kept, cap, io->d_counts, batch, d_kb))) return rc;
    mo_stage_mark(c, "grid_good_features");
    const int blur_margin = mo_blur_margin(c->plan.edge_threshold);
    if ((rc = orb_launch_blur(c, io->d_gray, batch, 1, blur_margin))) return rc;  // the records all sit on octave 0
    mo_stage_mark(c, "blur");
    // descriptors out of one blurred LDS tile per grid cell; cells too large for the tile (frames beyond ~ 720 x 480) take the
    // one-wavefront-per-keypoint kernel that samples global memory
    rc = orb_launch_describe_cells(c, io->d_kps, d_kb, io->d_desc, cap, batch);
    if (rc == MO_ERR_UNSUPPORTED) rc = orb_launch_describe_given(c, io->d_gray, io->d_kps, cap, io->d_desc, io->d_counts, batch, 1);
    if (rc) return rc;
    mo_stage_mark(c, "compute");
    return MO_OK;
}

// copy host images (any stride / 1 or 3 channels) into a dense device gray batch; returns the device pointer
static int stage_images(mo_ctx* c, const uint8_t* img, int w, int h, int stride, int ch, int batch, const uint8_t** d_gray) {
    if (!img) return mo_fail(c, MO_ERR_ARG, "img is NULL");
    if (ch != 1 && ch != 3) return mo_fail(c, MO_ERR_ARG, "ch must be 1 (gray) or 3 (BGR)");
    if (stride < w * ch) return mo_fail(c, MO_ERR_ARG, "stride smaller than a row");
    size_t row = (size_t)w * ch, frame = row * h;
    int rc = c->d_in.reserve_exact(c, frame * batch);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy2DAsync(c->d_in, row, img, (size_t)stride, row, (size_t)h * batch, hipMemcpyHostToDevice, c->stream));
    if (ch == 3) {
        rc = c->d_gray.reserve_exact(c, (size_t)w * h * batch);
        if (rc) return rc;
        if ((rc = orb_launch_gray(c, c->d_in, w, h, batch, c->d_gray))) return rc;
        *d_gray = c->d_gray;
    } else {
        *d_gray = c->d_in;
    }
    return MO_OK;
}

// output staging of a batched host call (rows f * cap + i: a byte bound per array is enough)
static int reserve_out(mo_ctx* c, int batch, int cap) {
    const size_t n = (size_t)batch * cap;
    int rc = c->d_kps.reserve_exact(c, n);
    if (!rc) rc = c->d_desc.reserve_exact(c, n * 32);
    if (!rc) rc = c->d_counts.reserve_exact(c, (size_t)batch);
    return rc;
}

// pinned host staging owned by the context (small host-API transfers: one copy each way and one synchronisation instead of a blocking
// round trip per pageable array).  Mapped + coherent: k_ingest / k_pack_out read and write it from the device.
int mo_host_stage(mo_ctx* c, size_t bytes) {
    return c->h_stage.reserve(c, mo_align(bytes, (size_t)1 << 20), hipHostMallocMapped | hipHostMallocCoherent);
}

// true when an overflowed level's final-keypoint slot can still grow (then the plan is invalidated so that the next call rebuilds it).
// retainBest keeps EVERY element that ties with the quota boundary, so a level of a periodic synthetic pattern can keep all its
// candidates; the slots are sized for 4 quota + 256 and the levels named in `levels` (bit L) grow eightfold, up to the level's
// candidate capacity - the other levels, and other image sizes / parameter sets, keep their sizes.
static bool grow_fin_slots(mo_ctx* c, int levels) {
    if (!c->plan_valid) return false;
    if (!levels) levels = (1 << c->plan.nlevels) - 1;  // (no level named: an older flag word; grow them all)
    bool grown = false;
    for (int L = 0; L < c->plan.nlevels; L++)
        if (((levels >> L) & 1) && c->plan.lv[L].fin_cap < c->plan.lv[L].cand_cap && c->fin_slack[L] < (1 << 24)) { c->fin_slack[L] *= 8; grown = true; }
    c->fin_slack_dirty = c->fin_slack_dirty || grown;
    return grown;
}

static int detect_compute_once(mo_ctx* c, const mo_orb_params* p, const uint8_t* img, int w, int h, int stride, int ch,
                               int batch, mo_keypoint* kps, uint8_t* desc, int cap, int* counts) {
    MO_ENTER(c);
    // one frame (the drop-in classes, a Tracker): pinned staging both ways, a resident result slot, one synchronisation (frame_api.hip)
    if (batch == 1 && (size_t)w * h * ch + (size_t)cap * 60 <= (size_t)64 << 20) return mo_detect_single(c, p, img, w, h, stride, ch, kps, desc, cap, counts);
    HostClock clk(c);
    const uint8_t* d_gray = nullptr;
    int rc = mo_build_plan(c, p, w, h, batch);  // validates sizes before any staging
    if (rc) return rc;
    mo_stage_begin(c);
    if ((rc = stage_images(c, img, w, h, stride, ch, batch, &d_gray))) return rc;
    if ((rc = reserve_out(c, batch, cap))) return rc;
    if ((rc = mo_run_extract(c, p, d_gray, w, h, batch, c->d_kps, desc ? c->d_desc : nullptr, cap, c->d_counts, true))) return rc;
    // Small results (the single-frame calls of the drop-in classes): flags, counts, keypoints and descriptors travel into ONE pinned
    // staging buffer behind one synchronisation; copies into the caller's pageable arrays cost a blocking round trip each (four
    // per call before: counts, flags, keypoints, descriptors).
    const size_t n_rows = (size_t)batch * cap, o_cnt = 4 * sizeof(int), o_kps = (o_cnt + (size_t)batch * sizeof(int) + 15) & ~(size_t)15;
    const size_t o_desc = o_kps + n_rows * sizeof(mo_keypoint), total = o_desc + (desc ? n_rows * 32 : 0);
    if (total <= (size_t)2 << 20) {
        if ((rc = mo_host_stage(c, total))) return rc;
        uint8_t* hs = c->h_stage;
        HIPCHK(c, hipMemcpyAsync(hs, mo_host_flags(c), 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(hs + o_cnt, c->d_counts, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(hs + o_kps, c->d_kps, n_rows * sizeof(mo_keypoint), hipMemcpyDeviceToHost, c->stream));
        if (desc) HIPCHK(c, hipMemcpyAsync(hs + o_desc, c->d_desc, n_rows * 32, hipMemcpyDeviceToHost, c->stream));
        mo_stage_mark(c, "d2h");
        clk.enqueued();
        HIPCHK(c, hipStreamSynchronize(c->stream));
        clk.waited();
        std::memcpy(counts, hs + o_cnt, (size_t)batch * sizeof(int));  // MO_ERR_CAPACITY: counts already holds the sizes a retry needs
        if ((rc = mo_decode_host_flags(c, ((const int*)hs)[0], ((const int*)hs)[1]))) return rc;
        for (int f = 0; f < batch; f++) {
            const int n = std::min(counts[f], cap);
            if (n <= 0) continue;
            std::memcpy(kps + (size_t)f * cap, hs + o_kps + (size_t)f * cap * sizeof(mo_keypoint), (size_t)n * sizeof(mo_keypoint));
            if (desc) std::memcpy(desc + (size_t)f * cap * 32, hs + o_desc + (size_t)f * cap * 32, (size_t)n * 32);
        }
        return MO_OK;
    }
    HIPCHK(c, hipMemcpyAsync(counts, c->d_counts, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    rc = check_flags(c);  // MO_ERR_CAPACITY: counts already holds the sizes a retry needs
    if (rc) return rc;
    for (int f = 0; f < batch; f++) {
        int n = std::min(counts[f], cap);
        if (n <= 0) continue;
        HIPCHK(c, hipMemcpyAsync(kps + (size_t)f * cap, c->d_kps + (size_t)f * cap, (size_t)n * sizeof(mo_keypoint),
                                 hipMemcpyDeviceToHost, c->stream));
        if (desc)
            HIPCHK(c, hipMemcpyAsync(desc + (size_t)f * cap * 32, c->d_desc + (size_t)f * cap * 32, (size_t)n * 32,
                                     hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MO_OK;
}

extern "C" int mo_orb_detect_compute(mo_ctx* c, const mo_orb_params* p, const uint8_t* img, int w, int h, int stride, int ch,
                                     int batch, mo_keypoint* kps, uint8_t* desc, int cap, int* counts) {
    if (!c) return MO_ERR_ARG;
    if (!kps || !counts) return mo_fail(c, MO_ERR_ARG, "kps/counts is NULL");
    for (;;) {  // (at most 8 rounds: the slots reach the candidate capacity, where no overflow is possible)
        c->tie_overflow = false; c->tie_levels = 0;
        const int rc = detect_compute_once(c, p, img, w, h, stride, ch, batch, kps, desc, cap, counts);
        if (rc != MO_ERR_CAPACITY || !c->tie_overflow || !grow_fin_slots(c, c->tie_levels)) return rc;
    }
}

extern "C" int mo_orb_compute(mo_ctx* c, const mo_orb_params* p, const uint8_t* img, int w, int h, int stride, int ch,
                              const mo_keypoint* kps_in, int n_in, int32_t* kept_idx, uint8_t* desc, int* n_out) {
    if (!c) return MO_ERR_ARG;
    if (!p || !n_out || (n_in > 0 && (!kps_in || !kept_idx || !desc))) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    MO_ENTER(c);
    *n_out = 0;
    // host-side list logic of Feature2D::compute / ORB_Impl::detectAndCompute(useProvidedKeypoints):
    // level count from the octaves, border filter on the full image, regroup by octave when unsorted
    int nlevels = 0;
    bool sorted = true;
    for (int i = 0; i < n_in; i++) {
        int L = kps_in[i].octave;
        if (L < 0) return mo_fail(c, MO_ERR_ARG, "keypoint octave < 0");
        if (i > 0 && L < kps_in[i - 1].octave) sorted = false;
        nlevels = std::max(nlevels, L);
    }
    nlevels++;
    if (nlevels > MO_MAX_LEVELS) return mo_fail(c, MO_ERR_UNSUPPORTED, "keypoint octave >= 12");
    std::vector<int> keep;
    int et = p->edge_threshold;
    if (!(et > 0 && (h <= et * 2 || w <= et * 2))) {
        for (int i = 0; i < n_in; i++) {
            int x = (int)lrintf(kps_in[i].x), y = (int)lrintf(kps_in[i].y);
            if (et > 0 && !(x >= et && x < w - et && y >= et && y < h - et)) continue;
            keep.push_back(i);
        }
    }
    if (!sorted) {
        std::vector<int> re;
        for (int L = 0; L < nlevels; L++)
            for (int i : keep)
                if (kps_in[i].octave == L) re.push_back(i);
        keep.swap(re);
    }
    int n = (int)keep.size();
    for (int i = 0; i < n; i++) kept_idx[i] = keep[i];
    *n_out = n;
    if (n == 0) return MO_OK;
    mo_orb_params pp = *p;
    if (nlevels > pp.nlevels) pp.nlevels = nlevels;
    int rc = mo_build_plan(c, &pp, w, h, 1);
    if (rc) return rc;
    const uint8_t* d_gray = nullptr;
    if ((rc = stage_images(c, img, w, h, stride, ch, 1, &d_gray))) return rc;
    std::vector<mo_keypoint> kk(n);
    for (int i = 0; i < n; i++) kk[i] = kps_in[keep[i]];
    const size_t kb = (size_t)n * sizeof(mo_keypoint);
    Layout L;
    const size_t o_k = L.take(kb), o_d = L.take((size_t)n * 32);
    if ((rc = c->d_tmp.reserve_exact(c, L.total))) return rc;
    mo_keypoint* d_k = L.at<mo_keypoint>(c->d_tmp, o_k);
    uint8_t* d_d = L.at<uint8_t>(c->d_tmp, o_d);
    HIPCHK(c, hipMemcpyAsync(d_k, kk.data(), kb, hipMemcpyHostToDevice, c->stream));
    mo_stage_begin(c);
    if ((rc = orb_launch_pyramid(c, d_gray, 1, nlevels, 0))) return rc;
    if ((rc = orb_launch_blur(c, d_gray, 1, nlevels, 0))) return rc;
    if ((rc = orb_launch_describe_given(c, d_gray, d_k, n, d_d))) return rc;
    mo_stage_mark(c, "compute");
    HIPCHK(c, hipMemcpyAsync(desc, d_d, (size_t)n * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MO_OK;
}

extern "C" int mo_dev_undistort(mo_ctx* c, const uint8_t* d_src, int w, int h, int ch, int batch, const double K[9],
                                const double dist[5], uint8_t* d_dst) {
    if (!c) return MO_ERR_ARG;
    if (!d_src || !d_dst || !K || !dist || d_src == d_dst) return mo_fail(c, MO_ERR_ARG, "NULL argument (or in-place)");
    if (w < 1 || h < 1 || batch < 1 || (ch != 1 && ch != 3)) return mo_fail(c, MO_ERR_ARG, "bad size / channel count");
    if (!(K[0] != 0.0) || !(K[4] != 0.0)) return mo_fail(c, MO_ERR_ARG, "focal length is zero");
    MO_ENTER(c);
    return undistort_launch(c, d_src, d_dst, w, h, ch, batch, K, dist);
}

extern "C" int mo_undistort(mo_ctx* c, const uint8_t* img, int w, int h, int stride, int ch, const double K[9], const double dist[5],
                            uint8_t* out) {
    if (!c) return MO_ERR_ARG;
    if (!img || !out || !K || !dist) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (w < 1 || h < 1 || (ch != 1 && ch != 3) || stride < w * ch) return mo_fail(c, MO_ERR_ARG, "bad size / stride / channel count");
    if (!(K[0] != 0.0) || !(K[4] != 0.0)) return mo_fail(c, MO_ERR_ARG, "focal length is zero");
    MO_ENTER(c);
    const size_t row = (size_t)w * ch, frame = row * h;
    Layout L;
    const size_t o_src = L.take(frame), o_dst = L.take(frame);
    int rc = c->d_tmp.reserve_exact(c, L.total);
    if (rc) return rc;
    uint8_t* d_src = L.at<uint8_t>(c->d_tmp, o_src);
    uint8_t* d_dst = L.at<uint8_t>(c->d_tmp, o_dst);
    HIPCHK(c, hipMemcpy2DAsync(d_src, row, img, (size_t)stride, row, (size_t)h, hipMemcpyHostToDevice, c->stream));
    mo_stage_begin(c);
    if ((rc = undistort_launch(c, d_src, d_dst, w, h, ch, 1, K, dist))) return rc;
    mo_stage_mark(c, "undistort");
    HIPCHK(c, hipMemcpyAsync(out, d_dst, frame, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MO_OK;
}

static int gftt_run(mo_ctx* c, const uint8_t* img, int w, int h, int stride, int ch, int n_features, float* xy, int* n_out,
                    float* eig_out) {
    if (w < 64 || h < 64 || w > c->max_w || h > c->max_h) return mo_fail(c, MO_ERR_ARG, "image size outside the context limits");
    if (n_features < 64) return mo_fail(c, MO_ERR_ARG, "n_features must be >= 64 (8x8 grid)");
    const uint8_t* d_gray = nullptr;
    int rc = stage_images(c, img, w, h, stride, ch, 1, &d_gray);
    if (rc) return rc;
    const int per_cell = n_features / 64;
    const size_t eig_b = (size_t)w * h * sizeof(float), xy_b = (size_t)64 * per_cell * 2 * sizeof(float);
    Layout L;
    const size_t o_eig = L.take(eig_b), o_xy = L.take(xy_b), o_n = L.take(64 * sizeof(int));
    if ((rc = c->d_tmp.reserve_exact(c, L.total))) return rc;
    float* d_eig = L.at<float>(c->d_tmp, o_eig);
    float* d_xy = L.at<float>(c->d_tmp, o_xy);
    int* d_n = L.at<int>(c->d_tmp, o_n);
    c->flags_cur = mo_host_flags(c);
    HIPCHK(c, hipMemsetAsync(mo_host_flags(c), 0, 4 * sizeof(int), c->stream));
    mo_stage_begin(c);
    if ((rc = gftt_launch(c, d_gray, w, h, n_features, d_eig, d_xy, d_n))) return rc;
    mo_stage_mark(c, "grid_good_features");
    if (eig_out) HIPCHK(c, hipMemcpyAsync(eig_out, d_eig, eig_b, hipMemcpyDeviceToHost, c->stream));
    std::vector<float> hxy((size_t)64 * per_cell * 2);
    int hn[64];
    HIPCHK(c, hipMemcpyAsync(hxy.data(), d_xy, xy_b, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hn, d_n, sizeof(hn), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int n = 0;
    if (xy)
        for (int cell = 0; cell < 64; cell++)
            for (int i = 0; i < hn[cell]; i++, n++) {
                xy[2 * n] = hxy[((size_t)cell * per_cell + i) * 2];
                xy[2 * n + 1] = hxy[((size_t)cell * per_cell + i) * 2 + 1];
            }
    if (n_out) *n_out = n;
    return MO_OK;
}

extern "C" int mo_orb_grid_good_features(mo_ctx* c, const uint8_t* img, int w, int h, int stride, int ch, int n_features,
                                         float* xy, int* n_out) {
    if (!c) return MO_ERR_ARG;
    if (!img || !xy || !n_out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    MO_ENTER(c);
    return gftt_run(c, img, w, h, stride, ch, n_features, xy, n_out, nullptr);
}

// ORBExtractor.distribute_keypoints in one call (reference extractor.py:85-144: the grid corners, KeyPoint(x, y, 31) each, then
// orb.compute on all of them): ONE upload of the image, the corner lists stay on the device, the records of the corners cv2 keeps are
// built there (k_gftt_records), blur of level 0 + descriptors, ONE synchronisation.  Same outputs as mo_orb_grid_good_features followed
// by mo_orb_compute on KeyPoint(x, y, 31) records.
extern "C" int mo_orb_grid_detect_compute(mo_ctx* c, const mo_orb_params* p, const uint8_t* img, int w, int h, int stride, int ch,
                                          int n_features, float* xy, int* n_xy, int32_t* kept_idx, uint8_t* desc, int* n_kept) {
    if (!c) return MO_ERR_ARG;
    if (!p || !img || !xy || !n_xy || !kept_idx || !desc || !n_kept) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    MO_ENTER(c);
    HostClock clk(c);
    *n_xy = 0; *n_kept = 0;
    c->last_token = 0;
    if (w < 64 || h < 64 || w > c->max_w || h > c->max_h) return mo_fail(c, MO_ERR_ARG, "image size outside the context limits");
    if (n_features < 64) return mo_fail(c, MO_ERR_ARG, "n_features must be >= 64 (8x8 grid)");
    if (ch != 1 && ch != 3) return mo_fail(c, MO_ERR_ARG, "ch must be 1 (gray) or 3 (BGR)");
    if (stride < w * ch) return mo_fail(c, MO_ERR_ARG, "stride smaller than a row");
    int rc = mo_build_plan(c, p, w, h, 1);
    if (rc) return rc;
    const int per_cell = n_features / 64, slots = 64 * per_cell;
    // Like the single-frame ORB call (frame_api.hip): the image through pinned staging and the upload kernel, the KEPT keypoints
    // (KeyPoint(x, y, 31) records, aligned with the descriptor rows) and their descriptors in a resident result slot - mo_last_token
    // names them for mo_pair_frontend -, everything the caller gets in one region that one small kernel pushes back, one synchronisation.
    int slot = 0;
    if ((rc = mo_slot_acquire(c, slots, &slot))) return rc;
    const int scap = c->slot_cap;
    mo_keypoint* d_rec = c->d_slot_kps + (size_t)slot * scap;
    uint8_t* d_desc = c->d_slot_desc + (size_t)slot * scap * 32;
    int32_t* d_cnt = c->d_slot_cnt + slot;
    const size_t rowb = (size_t)w * ch, in_bytes = rowb * h, eig_b = (size_t)w * h * sizeof(float), xy_b = (size_t)slots * 2 * sizeof(float);
    Layout L;
    const size_t o_eig = L.take(eig_b), o_out = L.total, o_fl = L.take(16), o_xy = L.take(xy_b), o_n = L.take(66 * sizeof(int)),
                 o_kept = L.take((size_t)slots * sizeof(int32_t)), o_desc = L.take((size_t)slots * 32), out_end = L.total;
    if ((rc = c->d_tmp.reserve_exact(c, out_end))) return rc;
    if ((rc = c->d_in.reserve_exact(c, mo_align((size_t)w * h, 256)))) return rc;
    const size_t h_out = mo_align(in_bytes, 256);
    if ((rc = mo_host_stage(c, h_out + (out_end - o_out)))) return rc;
    uint8_t* hs = c->h_stage;
    uint8_t* hs_dev = mo_stage_dev(c);
    if (!hs_dev) return mo_fail(c, MO_ERR_HIP, "the pinned staging buffer is not mapped into the device");
    mo_copy_rows(hs, img, rowb, h, (size_t)stride);
    uint8_t* b = c->d_tmp;
    float* d_eig = L.at<float>(b, o_eig); float* d_xy = L.at<float>(b, o_xy); int* d_n = L.at<int>(b, o_n);
    int32_t* d_kept = L.at<int32_t>(b, o_kept);
    c->flags_cur = mo_host_flags(c);
    mo_stage_begin(c);
    if ((rc = orb_launch_ingest(c, hs_dev, w, h, ch, c->d_in, mo_host_flags(c)))) return rc;
    mo_stage_mark(c, "h2d");
    const uint8_t* d_gray = c->d_in;
    if ((rc = gftt_launch(c, d_gray, w, h, n_features, d_eig, d_xy, d_n))) return rc;
    if ((rc = gftt_records_launch(c, d_xy, d_n, per_cell, w, h, p->edge_threshold, d_rec, d_kept, scap, d_cnt, 1))) return rc;  // (totals: d_n[64], d_n[65])
    mo_stage_mark(c, "grid_good_features");
    if ((rc = orb_launch_blur(c, d_gray, 1, 1, 0))) return rc;  // the records all sit on octave 0
    if ((rc = orb_launch_describe_given(c, d_gray, d_rec, slots, d_desc, d_n + 65, 1, 0))) return rc;
    mo_stage_mark(c, "compute");
    // descriptors of the kept corners and the flag words into the result region, then the region into the pinned buffer
    HIPCHK(c, hipMemcpyAsync(b + o_desc, d_desc, (size_t)slots * 32, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_fl, mo_host_flags(c), 16, hipMemcpyDeviceToDevice, c->stream));
    mo_copy_out_launch(c, b + o_out, hs_dev + h_out, out_end - o_out);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "d2h");
    clk.enqueued();
    HIPCHK(c, hipStreamSynchronize(c->stream));
    clk.waited();
    const uint8_t* ho = hs + h_out;
    const int* hn = (const int*)(ho + (o_n - o_out));
    const float* hxy = (const float*)(ho + (o_xy - o_out));
    const int* fl = (const int*)(ho + (o_fl - o_out));
    if ((rc = mo_decode_host_flags(c, fl[0], fl[1], "more grid corners than the result slot holds"))) return rc;
    int n = 0;
    for (int cell = 0; cell < 64; cell++)
        for (int i = 0; i < std::min(hn[cell], per_cell); i++, n++) {
            xy[2 * n] = hxy[((size_t)cell * per_cell + i) * 2];
            xy[2 * n + 1] = hxy[((size_t)cell * per_cell + i) * 2 + 1];
        }
    const int nk = hn[65];
    if (hn[64] != n || nk < 0 || nk > n) return mo_fail(c, MO_ERR_HIP, "grid corner counts disagree between host and device");
    *n_xy = n; *n_kept = nk;
    std::memcpy(kept_idx, ho + (o_kept - o_out), (size_t)nk * sizeof(int32_t));
    std::memcpy(desc, ho + (o_desc - o_out), (size_t)nk * 32);
    mo_slot_commit(c, slot, nk);
    return MO_OK;
}

extern "C" int mo_dbg_set_poison(mo_ctx* c, int byte) {
    if (!c) return MO_ERR_ARG;
    c->poison = byte < 0 ? -1 : (byte & 255);
    c->poison_bufs = 0; c->poison_bytes = 0;
    return MO_OK;
}

extern "C" int mo_dbg_poison_filled(mo_ctx* c, int64_t* n_buffers, int64_t* n_bytes) {
    if (!c) return MO_ERR_ARG;
    if (n_buffers) *n_buffers = c->poison_bufs;
    if (n_bytes) *n_bytes = c->poison_bytes;
    return MO_OK;
}

extern "C" int mo_dbg_min_eigen(mo_ctx* c, const uint8_t* gray, int w, int h, float* eig) {
    if (!c) return MO_ERR_ARG;
    MO_ENTER(c);
    return gftt_run(c, gray, w, h, w, 1, 64, nullptr, nullptr, eig);
}

extern "C" int mo_match_knn2_ratio(mo_ctx* c, const uint8_t* q, int nq, const uint8_t* t, int nt, const double* ratio,
                                   int batch, int32_t* train_idx, int32_t* dist, uint8_t* pass) {
    if (!c) return MO_ERR_ARG;
    if (nq < 0 || nt < 0 || batch < 1) return mo_fail(c, MO_ERR_ARG, "bad sizes");
    if (nq == 0) return MO_OK;
    if (!q || !train_idx || !dist || !pass || (nt > 0 && !t)) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    MO_ENTER(c);
    HostClock clk(c);
    size_t qb = (size_t)batch * nq * 32, tb = (size_t)batch * std::max(nt, 1) * 32, n = (size_t)batch * nq;
    int rc;
    if ((rc = c->d_mq.reserve_exact(c, qb))) return rc;
    if ((rc = c->d_mt.reserve_exact(c, tb))) return rc;
    if ((rc = c->d_midx.reserve_exact(c, n * 2))) return rc;
    if ((rc = c->d_mdist.reserve_exact(c, n * 2))) return rc;
    if ((rc = c->d_mpass.reserve_exact(c, n))) return rc;
    const size_t tbytes = (size_t)batch * nt * 32, o_t = (qb + 15) & ~(size_t)15, o_idx = (o_t + tbytes + 15) & ~(size_t)15;
    const size_t o_dist = o_idx + n * 2 * sizeof(int32_t), o_pass = o_dist + n * 2 * sizeof(int32_t), total = o_pass + n;
    const bool staged = total <= (size_t)2 << 20;  // the single-pair calls of the drop-in classes
    if (staged) {
        if ((rc = mo_host_stage(c, total))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (the staging buffer of a previous call has been consumed)
        std::memcpy(c->h_stage, q, qb);
        if (nt > 0) std::memcpy(c->h_stage + o_t, t, tbytes);
        mo_stage_begin(c);
        HIPCHK(c, hipMemcpyAsync(c->d_mq, c->h_stage, qb, hipMemcpyHostToDevice, c->stream));
        if (nt > 0) HIPCHK(c, hipMemcpyAsync(c->d_mt, c->h_stage + o_t, tbytes, hipMemcpyHostToDevice, c->stream));
    } else {
        mo_stage_begin(c);
        HIPCHK(c, hipMemcpyAsync(c->d_mq, q, qb, hipMemcpyHostToDevice, c->stream));
        if (nt > 0) HIPCHK(c, hipMemcpyAsync(c->d_mt, t, tbytes, hipMemcpyHostToDevice, c->stream));
    }
    mo_stage_mark(c, "h2d");
    rc = match_launch_pairs(c, c->d_mq, c->d_mt, (size_t)nq * 32, (size_t)nt * 32, nullptr, nullptr, nullptr, nq, nt, batch,
                            nq, ratio ? *ratio : -1.0, c->d_midx, c->d_mdist, c->d_mpass);
    if (rc) return rc;
    mo_stage_mark(c, "match_knn2_ratio");
    if (staged) {
        HIPCHK(c, hipMemcpyAsync(c->h_stage + o_idx, c->d_midx, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->h_stage + o_dist, c->d_mdist, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->h_stage + o_pass, c->d_mpass, n, hipMemcpyDeviceToHost, c->stream));
        mo_stage_mark(c, "d2h");
        clk.enqueued();
        HIPCHK(c, hipStreamSynchronize(c->stream));
        clk.waited();
        std::memcpy(train_idx, c->h_stage + o_idx, n * 2 * sizeof(int32_t));
        std::memcpy(dist, c->h_stage + o_dist, n * 2 * sizeof(int32_t));
        std::memcpy(pass, c->h_stage + o_pass, n);
        return MO_OK;
    }
    HIPCHK(c, hipMemcpyAsync(train_idx, c->d_midx, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dist, c->d_mdist, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(pass, c->d_mpass, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MO_OK;
}

extern "C" int mo_init_two_view(mo_ctx* c, const float* p1, const float* p2, int m, const double K[9], double thr_px,
                                double prob, int n_hyp, uint64_t seed, double R[9], double t[3], double E[9],
                                uint8_t* ransac_inlier, uint8_t* inlier, float* X, int* n_good) {
    (void)prob;
    if (!c) return MO_ERR_ARG;
    if (!p1 || !p2 || !K || !R || !t || !inlier || !X || !n_good) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (m < 0) return mo_fail(c, MO_ERR_ARG, "m must be >= 0");
    MO_ENTER(c);
    *n_good = 0;
    if (m < 8) {
        for (int i = 0; i < 9; i++) R[i] = NAN;
        for (int i = 0; i < 3; i++) t[i] = NAN;
        std::memset(inlier, 0, (size_t)m);
        if (ransac_inlier) std::memset(ransac_inlier, 0, (size_t)m);
        if (E) for (int i = 0; i < 9; i++) E[i] = NAN;
        for (int i = 0; i < 3 * m; i++) X[i] = NAN;
        return MO_OK;
    }
    const size_t pb = (size_t)m * 2 * sizeof(float);
    Layout L;
    const size_t o_pose = L.take(12 * sizeof(double)), o_E = L.take(9 * sizeof(double)), o_n = L.take(sizeof(int32_t)), o_p1 = L.take(pb),
                 o_p2 = L.take(pb), o_X = L.take((size_t)m * 3 * sizeof(float)), o_inl = L.take(m), o_ran = L.take(m);
    int rc = c->d_tmp.reserve_exact(c, L.total);
    if (rc) return rc;
    uint8_t* b = c->d_tmp;
    double* d_pose = L.at<double>(b, o_pose);
    double* d_E = L.at<double>(b, o_E);
    int32_t* d_n = L.at<int32_t>(b, o_n);
    float* d_p1 = L.at<float>(b, o_p1);
    float* d_p2 = L.at<float>(b, o_p2);
    float* d_X = L.at<float>(b, o_X);
    uint8_t* d_inl = b + o_inl;
    uint8_t* d_ran = b + o_ran;
    HIPCHK(c, hipMemcpyAsync(d_p1, p1, pb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_p2, p2, pb, hipMemcpyHostToDevice, c->stream));
    TwoViewArgs a;
    a.n_pairs = 1; a.cap = m; a.n_hyp = n_hyp;
    for (int i = 0; i < 9; i++) a.K[i] = K[i];
    a.thr_px = thr_px; a.seed = seed;
    a.d_p1 = d_p1; a.d_p2 = d_p2; a.m_fixed = m;
    a.d_pose = d_pose; a.d_E = d_E; a.d_points = d_X; a.d_inlier = d_inl; a.d_ransac = d_ran; a.d_n_points = d_n;
    mo_stage_begin(c);
    if ((rc = twoview_launch(c, a))) return rc;
    mo_stage_mark(c, "two_view");
    double pose[12];
    int32_t ng = 0;
    HIPCHK(c, hipMemcpyAsync(pose, d_pose, sizeof(pose), hipMemcpyDeviceToHost, c->stream));
    if (E) HIPCHK(c, hipMemcpyAsync(E, d_E, 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&ng, d_n, sizeof(ng), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(X, d_X, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(inlier, d_inl, (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (ransac_inlier) HIPCHK(c, hipMemcpyAsync(ransac_inlier, d_ran, (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 9; i++) R[i] = pose[i];
    for (int i = 0; i < 3; i++) t[i] = pose[9 + i];
    *n_good = ng;
    return MO_OK;
}

extern "C" int mo_init_two_view_hf(mo_ctx* c, const float* p1, const float* p2, int m, const double K[9], const mo_hf_params* pr,
                                   mo_hf_result* o) {
    if (!c) return MO_ERR_ARG;
    if (!p1 || !p2 || !K || !pr || !o || !o->pose_mask || !o->X || !o->ransac_mask || !o->h_mask) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (m < 0) return mo_fail(c, MO_ERR_ARG, "m must be >= 0");
    if (!(pr->sigma > 0.0) || !(pr->min_parallax_deg >= 0.0) || !(pr->min_parallax_deg < 180.0) || !(pr->rh_threshold == pr->rh_threshold) ||
        pr->min_triangulated < 0)
        return mo_fail(c, MO_ERR_ARG, "sigma must be positive, min_parallax_deg in [0, 180), rh_threshold a number, min_triangulated >= 0");
    if (pr->n_hyp < 1 || pr->n_hyp > (1 << 20) || pr->n_hyp_h < 1 || pr->n_hyp_h > (1 << 20)) return mo_fail(c, MO_ERR_ARG, "n_hyp / n_hyp_h out of range");
    MO_ENTER(c);
    // the no-model result
    uint8_t* const pm = o->pose_mask; float* const X = o->X; uint8_t* const rm = o->ransac_mask; uint8_t* const hm = o->h_mask;
    *o = mo_hf_result{};
    o->pose_mask = pm; o->X = X; o->ransac_mask = rm; o->h_mask = hm;
    o->model = -1; o->best_h = o->second_h = o->winner_h = -1;
    for (double* v : {o->R, o->E, o->R_e, o->H, o->R_h}) std::fill(v, v + 9, (double)NAN);
    for (double* v : {o->t, o->t_e, o->t_h}) std::fill(v, v + 3, (double)NAN);
    std::memset(pm, 0, (size_t)m); std::memset(rm, 0, (size_t)m); std::memset(hm, 0, (size_t)m);
    for (int i = 0; i < 3 * m; i++) X[i] = NAN;
    if (m < 8) return MO_OK;
    const size_t pb = (size_t)m * 2 * sizeof(float), xb = (size_t)m * 3 * sizeof(float);
    Layout L;
    const size_t o_pose = L.take(12 * sizeof(double)), o_E = L.take(9 * sizeof(double)), o_n = L.take(sizeof(int32_t)), o_p1 = L.take(pb),
                 o_p2 = L.take(pb), o_X = L.take(xb), o_inl = L.take(m), o_ran = L.take(m), o_H = L.take(9 * sizeof(double)),
                 o_stat = L.take(HF_NSTAT * sizeof(double)), o_info = L.take(HF_NINFO * sizeof(int32_t)), o_hm = L.take(m), o_good = L.take(m),
                 o_Xh = L.take(xb);
    int rc = c->d_tmp.reserve_exact(c, L.total);
    if (rc) return rc;
    uint8_t* b = c->d_tmp;
    float* d_p1 = L.at<float>(b, o_p1);
    float* d_p2 = L.at<float>(b, o_p2);
    HIPCHK(c, hipMemcpyAsync(d_p1, p1, pb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_p2, p2, pb, hipMemcpyHostToDevice, c->stream));
    TwoViewArgs a;  // the essential chain, argument for argument what mo_init_two_view launches
    a.n_pairs = 1; a.cap = m; a.n_hyp = pr->n_hyp;
    for (int i = 0; i < 9; i++) a.K[i] = K[i];
    a.thr_px = pr->thr_px; a.seed = pr->seed;
    a.d_p1 = d_p1; a.d_p2 = d_p2; a.m_fixed = m;
    a.d_pose = L.at<double>(b, o_pose); a.d_E = L.at<double>(b, o_E); a.d_points = L.at<float>(b, o_X); a.d_inlier = b + o_inl;
    a.d_ransac = b + o_ran; a.d_n_points = L.at<int32_t>(b, o_n);
    HfArgs h;
    h.n_pairs = 1; h.cap = m; h.n_hyp = pr->n_hyp_h; h.m_fixed = m;
    for (int i = 0; i < 9; i++) h.K[i] = K[i];
    h.sigma = pr->sigma; h.cos_max = std::cos(pr->min_parallax_deg * (M_PI / 180.0)); h.min_triangulated = pr->min_triangulated;
    h.seed = pr->seed;
    h.d_p1 = d_p1; h.d_p2 = d_p2; h.d_E = a.d_E;
    h.d_H = L.at<double>(b, o_H); h.d_stat = L.at<double>(b, o_stat); h.d_info = L.at<int32_t>(b, o_info);
    h.d_hmask = b + o_hm; h.d_good = b + o_good; h.d_X = L.at<float>(b, o_Xh);
    mo_stage_begin(c);
    if ((rc = twoview_launch(c, a))) return rc;
    mo_stage_mark(c, "two_view");
    if ((rc = twoview_h_launch(c, h))) return rc;
    mo_stage_mark(c, "two_view_h");
    double pose[12], stat[HF_NSTAT];
    int32_t ng = 0, info[HF_NINFO];
    std::vector<uint8_t> inl_e((size_t)m), good_h((size_t)m);
    std::vector<float> X_e((size_t)m * 3), X_h((size_t)m * 3);
    HIPCHK(c, hipMemcpyAsync(pose, a.d_pose, sizeof(pose), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(o->E, a.d_E, 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&ng, a.d_n_points, sizeof(ng), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(X_e.data(), a.d_points, xb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(inl_e.data(), a.d_inlier, (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(rm, a.d_ransac, (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(o->H, h.d_H, 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(stat, h.d_stat, sizeof(stat), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(info, h.d_info, sizeof(info), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hm, h.d_hmask, (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(good_h.data(), h.d_good, (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(X_h.data(), h.d_X, xb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 9; i++) { o->R_e[i] = pose[i]; o->R_h[i] = stat[11 + i]; }
    for (int i = 0; i < 3; i++) { o->t_e[i] = pose[9 + i]; o->t_h[i] = stat[20 + i]; }
    o->n_good_e = ng;
    o->SH = stat[0]; o->SF = stat[1]; o->RH = stat[2];
    for (int k = 0; k < 8; k++) {
        o->n_good_h[k] = info[k];
        const double cs = stat[3 + k];  // 2: no passed point
        o->parallax_h[k] = cs > 1.5 ? 0.0 : std::acos(std::fmin(std::fmax(cs, -1.0), 1.0)) * (180.0 / M_PI);
    }
    o->best_h = info[8]; o->second_h = info[9]; o->n_inliers_h = info[10]; o->accepted_h = info[11]; o->winner_h = info[12]; o->refits_h = info[13];
    if (!(o->E[0] == o->E[0])) {  // the essential path reports no model: so does the call (the raw homography fields stay for inspection)
        std::memset(rm, 0, (size_t)m);
        return MO_OK;
    }
    if (o->RH > pr->rh_threshold) {
        o->model = 1; o->accepted = o->accepted_h; o->n_good = o->best_h >= 0 ? o->n_good_h[o->best_h] : 0;
        std::memcpy(o->R, o->R_h, sizeof(o->R)); std::memcpy(o->t, o->t_h, sizeof(o->t));
        std::memcpy(pm, good_h.data(), (size_t)m); std::memcpy(X, X_h.data(), xb);
    } else {
        o->model = 0; o->accepted = ng > pr->min_triangulated ? 1 : 0; o->n_good = ng;
        std::memcpy(o->R, o->R_e, sizeof(o->R)); std::memcpy(o->t, o->t_e, sizeof(o->t));
        std::memcpy(pm, inl_e.data(), (size_t)m); std::memcpy(X, X_e.data(), xb);
    }
    return MO_OK;
}

extern "C" int mo_recover_pose(mo_ctx* c, const double E[9], const float* p1, const float* p2, int m, const double K[9],
                               const uint8_t* mask_in, double R[9], double t[3], uint8_t* mask_out, float* X, int* n_good) {
    if (!c) return MO_ERR_ARG;
    if (!E || !K || !R || !t || !n_good || m < 0 || (m > 0 && (!p1 || !p2 || !mask_out))) return mo_fail(c, MO_ERR_ARG, "NULL / negative argument");
    MO_ENTER(c);
    *n_good = 0;
    for (int i = 0; i < 9; i++) R[i] = NAN;
    for (int i = 0; i < 3; i++) t[i] = NAN;
    if (m == 0) return MO_OK;
    const size_t pb = (size_t)m * 2 * sizeof(float);
    Layout L;
    const size_t o_p1 = L.take(pb), o_p2 = L.take(pb), o_E = L.take(9 * sizeof(double)), o_min = L.take(m), o_pose = L.take(12 * sizeof(double)),
                 o_X = L.take((size_t)m * 3 * sizeof(float)), o_inl = L.take(m), o_n = L.take(sizeof(int32_t));
    int rc = c->d_tmp.reserve_exact(c, L.total);
    if (rc) return rc;
    uint8_t* b = c->d_tmp;
    HIPCHK(c, hipMemcpyAsync(b + o_p1, p1, pb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_p2, p2, pb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_E, E, 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (mask_in) HIPCHK(c, hipMemcpyAsync(b + o_min, mask_in, (size_t)m, hipMemcpyHostToDevice, c->stream));
    TwoViewArgs a;
    a.n_pairs = 1; a.cap = m;
    for (int i = 0; i < 9; i++) a.K[i] = K[i];
    a.thr_px = 1.0;
    a.d_p1 = L.at<float>(b, o_p1); a.d_p2 = L.at<float>(b, o_p2); a.m_fixed = m;
    a.d_E_in = L.at<double>(b, o_E); a.d_mask_in = mask_in ? b + o_min : nullptr;
    a.d_pose = L.at<double>(b, o_pose); a.d_points = L.at<float>(b, o_X); a.d_inlier = b + o_inl; a.d_n_points = L.at<int32_t>(b, o_n);
    mo_stage_begin(c);
    if ((rc = twoview_launch(c, a))) return rc;
    mo_stage_mark(c, "recover_pose");
    double pose[12];
    int32_t ng = 0;
    HIPCHK(c, hipMemcpyAsync(pose, b + o_pose, sizeof(pose), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(mask_out, b + o_inl, (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (X) HIPCHK(c, hipMemcpyAsync(X, b + o_X, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&ng, b + o_n, sizeof(ng), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 9; i++) R[i] = pose[i];
    for (int i = 0; i < 3; i++) t[i] = pose[9 + i];
    *n_good = ng;
    return MO_OK;
}

extern "C" int mo_find_fundamental(mo_ctx* c, const float* p1, const float* p2, int m, double thr_px, double prob, int n_hyp,
                                   uint64_t seed, double F[9], uint8_t* mask, int* n_inliers) {
    (void)prob;
    if (!c) return MO_ERR_ARG;
    if (!F || !n_inliers || m < 0 || (m > 0 && (!p1 || !p2 || !mask))) return mo_fail(c, MO_ERR_ARG, "NULL / negative argument");
    MO_ENTER(c);
    *n_inliers = 0;
    for (int i = 0; i < 9; i++) F[i] = NAN;
    if (m < 8) { if (m > 0) std::memset(mask, 0, (size_t)m); return MO_OK; }
    const size_t pb = (size_t)m * 2 * sizeof(float);
    Layout L;
    const size_t o_p1 = L.take(pb), o_p2 = L.take(pb), o_F = L.take(9 * sizeof(double)), o_X = L.take((size_t)m * 3 * sizeof(float)),
                 o_ran = L.take(m), o_n = L.take(sizeof(int32_t));
    int rc = c->d_tmp.reserve_exact(c, L.total);
    if (rc) return rc;
    uint8_t* b = c->d_tmp;
    HIPCHK(c, hipMemcpyAsync(b + o_p1, p1, pb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_p2, p2, pb, hipMemcpyHostToDevice, c->stream));
    TwoViewArgs a = tv_fundamental(1, m, n_hyp, thr_px, seed, 0);
    a.d_p1 = L.at<float>(b, o_p1); a.d_p2 = L.at<float>(b, o_p2); a.m_fixed = m;
    a.d_E = L.at<double>(b, o_F); a.d_points = L.at<float>(b, o_X); a.d_ransac = b + o_ran; a.d_n_points = L.at<int32_t>(b, o_n);
    mo_stage_begin(c);
    if ((rc = twoview_launch(c, a))) return rc;
    mo_stage_mark(c, "find_fundamental");
    int32_t ng = 0;
    HIPCHK(c, hipMemcpyAsync(F, b + o_F, 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(mask, b + o_ran, (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&ng, b + o_n, sizeof(ng), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_inliers = ng;
    return MO_OK;
}

extern "C" int mo_track_pair(mo_ctx* c, const mo_keypoint* kps1, int n1, const uint8_t* desc1, const mo_keypoint* kps2, int n2,
                             const uint8_t* desc2, int w, int h, double ratio, double disp_frac, const double K[9], double thr_px,
                             int n_hyp, uint64_t seed, double R[9], double t[3], double E[9], int32_t* sel_idx, int32_t* sel_dist,
                             int* n_sel, uint8_t* inlier, int* n_inliers) {
    if (!c) return MO_ERR_ARG;
    if (!K || !R || !t || !n_sel || !n_inliers || n1 < 0 || n2 < 0) return mo_fail(c, MO_ERR_ARG, "NULL / negative argument");
    *n_sel = 0; *n_inliers = 0;
    for (int i = 0; i < 9; i++) { R[i] = NAN; if (E) E[i] = NAN; }
    for (int i = 0; i < 3; i++) t[i] = NAN;
    if (n1 == 0 || n2 == 0) return MO_OK;
    if (!kps1 || !kps2 || !desc1 || !desc2 || !sel_idx || !inlier) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    // the host-array form of mo_pair_frontend(MO_MODE_TRACK) (frame_api.hip): both frames are uploaded into resident slots
    mo_frame_ref f1 = {0, kps1, desc1, n1}, f2 = {0, kps2, desc2, n2};
    mo_pair_params pp;
    std::memset(&pp, 0, sizeof(pp));
    pp.mode = MO_MODE_TRACK; pp.w = w; pp.h = h; pp.ratio = ratio; pp.disp_frac = disp_frac; pp.thr_px = thr_px; pp.n_hyp = n_hyp; pp.seed = seed;
    for (int i = 0; i < 9; i++) pp.K[i] = K[i];
    mo_pair_out o;
    std::memset(&o, 0, sizeof(o));
    o.sel_idx = sel_idx; o.sel_dist = sel_dist; o.inlier = inlier;
    const int rc = mo_pair_frontend(c, &f1, &f2, &pp, &o);
    if (rc) return rc;
    *n_sel = o.n_sel; *n_inliers = o.n_good;
    for (int i = 0; i < 9; i++) { R[i] = o.R[i]; if (E) E[i] = o.E[i]; }
    for (int i = 0; i < 3; i++) t[i] = o.t[i];
    return MO_OK;
}

extern "C" int mo_triangulate_points(mo_ctx* c, const double P1[12], const double P2[12], const float* p1, const float* p2,
                                     int n, float* X4) {
    if (!c) return MO_ERR_ARG;
    if (n < 0 || !P1 || !P2 || (n > 0 && (!p1 || !p2 || !X4))) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (n == 0) return MO_OK;
    MO_ENTER(c);
    const size_t pb = (size_t)n * 2 * sizeof(float);
    Layout L;
    const size_t o_p1 = L.take(pb), o_p2 = L.take(pb), o_X = L.take((size_t)n * 4 * sizeof(float));
    int rc = c->d_tmp.reserve_exact(c, L.total);
    if (rc) return rc;
    float* d_p1 = L.at<float>(c->d_tmp, o_p1);
    float* d_p2 = L.at<float>(c->d_tmp, o_p2);
    float* d_X = L.at<float>(c->d_tmp, o_X);
    HIPCHK(c, hipMemcpyAsync(d_p1, p1, pb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_p2, p2, pb, hipMemcpyHostToDevice, c->stream));
    if ((rc = triangulate_launch(c, P1, P2, d_p1, d_p2, n, d_X))) return rc;
    HIPCHK(c, hipMemcpyAsync(X4, d_X, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MO_OK;
}

// ---- device-resident batched mode -----------------------------------------------------------------
extern "C" int mo_dev_orb_detect_compute(mo_ctx* c, const mo_orb_params* p, const uint8_t* d_gray, int w, int h, int batch,
                                         mo_keypoint* d_kps, uint8_t* d_desc, int cap, int32_t* d_counts) {
    if (!c) return MO_ERR_ARG;
    if (!d_gray || !d_kps || !d_counts) return mo_fail(c, MO_ERR_ARG, "NULL device pointer");
    MO_ENTER(c);
    return mo_run_extract(c, p, d_gray, w, h, batch, d_kps, d_desc, cap, d_counts, false);
}

extern "C" int mo_dev_match_pairs(mo_ctx* c, const uint8_t* d_desc, const int32_t* d_counts, int cap, const int32_t* d_qf,
                                  const int32_t* d_tf, int n_pairs, double ratio, int32_t* d_idx, int32_t* d_dist,
                                  uint8_t* d_pass) {
    if (!c) return MO_ERR_ARG;
    if (!d_desc || !d_counts || !d_idx || !d_dist || !d_pass) return mo_fail(c, MO_ERR_ARG, "NULL device pointer");
    MO_ENTER(c);
    mo_stage_begin(c);
    int rc = match_launch_pairs(c, d_desc, d_desc, (size_t)cap * 32, (size_t)cap * 32, d_counts, d_qf, d_tf, 0, 0, n_pairs, cap,
                                ratio, d_idx, d_dist, d_pass);
    mo_stage_mark(c, "match_knn2_ratio");
    return rc;
}

__global__ void k_pair_frames(int32_t* qf, int32_t* tf, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { qf[i] = i; tf[i] = i + 1; }
}

extern "C" int mo_dev_frontend_batch(mo_ctx* c, const mo_orb_params* p, const mo_batch_io* io) {
    if (!c) return MO_ERR_ARG;
    if (!io || !io->d_gray || !io->d_kps || !io->d_desc || !io->d_counts) return mo_fail(c, MO_ERR_ARG, "NULL in mo_batch_io");
    MO_ENTER(c);
    if (io->detector != MO_DETECT_ORB && io->detector != MO_DETECT_GRID) return mo_fail(c, MO_ERR_ARG, "mo_batch_io.detector must be MO_DETECT_ORB or MO_DETECT_GRID");
    int rc = io->detector == MO_DETECT_GRID ? run_grid_extract(c, p, io)
                                            : mo_run_extract(c, p, io->d_gray, io->w, io->h, io->batch, io->d_kps, io->d_desc, io->cap, io->d_counts, false);
    if (rc) return rc;
    if (io->mode == MO_MODE_KEYFRAME) {
        // LocalMapper._process_new_keyframe (local_mapper.py:116-149) for n_kf_pairs (query keyframe, train keyframe) pairs of the batch
        const int np = io->n_kf_pairs;
        if (np < 1) return MO_OK;
        if (!io->d_kf_query || !io->d_kf_train || !io->d_kf_P1 || !io->d_kf_P2 || !io->d_match_idx || !io->d_match_dist || !io->d_match_pass ||
            !io->d_points || !io->d_n_points)
            return mo_fail(c, MO_ERR_ARG, "MO_MODE_KEYFRAME needs d_kf_query / d_kf_train / d_kf_P1 / d_kf_P2, the match outputs, d_points and d_n_points");
        if (io->n_hyp < 1) return mo_fail(c, MO_ERR_ARG, "MO_MODE_KEYFRAME needs n_hyp >= 1");
        rc = match_launch_pairs(c, io->d_desc, io->d_desc, (size_t)io->cap * 32, (size_t)io->cap * 32, io->d_counts, io->d_kf_query, io->d_kf_train,
                                0, 0, np, io->cap, io->ratio, io->d_match_idx, io->d_match_dist, io->d_match_pass);
        if (rc) return rc;
        mo_stage_mark(c, "match_knn2_ratio");
        TwoViewArgs a = tv_fundamental(np, io->cap, io->n_hyp, io->thr_px, io->seed, io->pair_index_base);
        a.d_kps = io->d_kps; a.d_counts = io->d_counts; a.d_match_idx = io->d_match_idx; a.d_match_pass = io->d_match_pass;
        a.d_qf = io->d_kf_query; a.d_tf = io->d_kf_train; a.need_two = 1; a.d_P1 = io->d_kf_P1; a.d_P2 = io->d_kf_P2;
        a.d_E = io->d_kf_F; a.d_points = io->d_points; a.d_n_points = io->d_n_points; a.d_inlier = io->d_pose_mask;
        if ((rc = twoview_launch(c, a))) return rc;
        mo_stage_mark(c, "keyframe_f_ransac_triangulate");
        return MO_OK;
    }
    int n_pairs = io->batch - 1;
    if (n_pairs < 1 || !io->d_match_idx) return MO_OK;
    if (!io->d_match_dist || !io->d_match_pass) return mo_fail(c, MO_ERR_ARG, "match outputs missing");
    // (query, train) frame of every pair: written once per batch size into a buffer of its own (it was a 5 us launch per call)
    if (c->pair_frames_n < n_pairs) {
        c->pair_frames_n = 0;
        if (c->d_pair_frames) HIPCHK(c, hipStreamSynchronize(c->stream));
        if ((rc = c->d_pair_frames.reserve_exact(c, (size_t)n_pairs * 2))) return rc;
        hipLaunchKernelGGL(k_pair_frames, dim3((n_pairs + 255) / 256), dim3(256), 0, c->stream, c->d_pair_frames, c->d_pair_frames + n_pairs,
                           n_pairs);
        HIPCHK(c, hipGetLastError());
        c->pair_frames_n = n_pairs;
    }
    int32_t* qf = c->d_pair_frames;
    int32_t* tf = qf + c->pair_frames_n;
    rc = match_launch_pairs(c, io->d_desc, io->d_desc, (size_t)io->cap * 32, (size_t)io->cap * 32, io->d_counts, qf, tf, 0, 0,
                            n_pairs, io->cap, io->ratio, io->d_match_idx, io->d_match_dist, io->d_match_pass);
    if (rc) return rc;
    mo_stage_mark(c, "match_knn2_ratio");
    if (io->n_hyp > 0) {
        if (!io->d_points || !io->d_n_points) return mo_fail(c, MO_ERR_ARG, "two-view outputs missing");
        TwoViewArgs a;
        a.n_pairs = n_pairs; a.cap = io->cap; a.n_hyp = io->n_hyp;
        for (int i = 0; i < 9; i++) a.K[i] = io->K[i];
        a.thr_px = io->thr_px; a.seed = io->seed; a.pair_base = io->pair_index_base;
        a.d_kps = io->d_kps; a.d_counts = io->d_counts; a.d_match_idx = io->d_match_idx; a.d_match_pass = io->d_match_pass;
        a.d_pose = io->d_pose; a.d_points = io->d_points; a.d_n_points = io->d_n_points; a.d_inlier = io->d_pose_mask;
        if (io->mode == MO_MODE_TRACK) {
            if (!io->d_sel_idx || !io->d_sel_n) return mo_fail(c, MO_ERR_ARG, "MO_MODE_TRACK needs d_sel_idx and d_sel_n");
            if ((rc = track_select_launch(c, io->d_kps, io->d_counts, qf, tf, io->d_match_idx, io->d_match_dist, io->d_match_pass,
                                          io->cap, n_pairs, io->w, io->h, io->disp_frac, io->d_sel_idx, io->d_sel_dist, io->d_sel_n)))
                return rc;
            mo_stage_mark(c, "track_filters");
            a.d_sel = io->d_sel_idx; a.d_sel_n = io->d_sel_n;
        } else if (io->mode != MO_MODE_INIT) return mo_fail(c, MO_ERR_ARG, "mo_batch_io.mode must be MO_MODE_INIT or MO_MODE_TRACK");
        if ((rc = twoview_launch(c, a))) return rc;
        mo_stage_mark(c, "two_view");
    }
    return MO_OK;
}

// ---- probes for stage-level parity tests -------------------------------------------------------------
extern "C" int mo_dbg_pyramid_level(mo_ctx* c, const mo_orb_params* p, const uint8_t* gray, int w, int h, int level,
                                    int blurred, uint8_t* out, int* lw, int* lh) {
    if (!c) return MO_ERR_ARG;
    MO_ENTER(c);
    int rc = mo_build_plan(c, p, w, h, 1);
    if (rc) return rc;
    if (level < 0 || level >= c->plan.nlevels) return mo_fail(c, MO_ERR_ARG, "level out of range");
    const uint8_t* d_gray = nullptr;
    if ((rc = stage_images(c, gray, w, h, w, 1, 1, &d_gray))) return rc;
    const bool fused = (blurred & 2) != 0;  // bit 1: through the single-frame kernel (front_single.hip) instead of k_resize2 / k_blur
    blurred &= 1;
    if (fused) {
        if (!c->pb.fs_ok) return mo_fail(c, MO_ERR_UNSUPPORTED, std::string("the single-frame pyramid kernel does not cover this geometry: ") + c->pb.fs_why);
        HIPCHK(c, hipMemsetAsync(c->pb.d_pyr, 0xA5, (size_t)c->plan.pyr_stride, c->stream));   // whatever it does not write shows
        HIPCHK(c, hipMemsetAsync(c->pb.d_blur, 0xA5, (size_t)c->plan.blur_stride, c->stream));
        if ((rc = orb_launch_front_single(c, d_gray, 1, 1))) return rc;
    } else if ((rc = orb_launch_pyramid(c, d_gray, 1, c->plan.nlevels, 0))) return rc;
    const LevelInfo& v = c->plan.lv[level];
    *lw = v.w; *lh = v.h;
    if (blurred) {
        if (!fused && (rc = orb_launch_blur(c, d_gray, 1, c->plan.nlevels, 0))) return rc;
        HIPCHK(c, hipMemcpy2DAsync(out, v.w, c->pb.d_blur + v.boff, v.bpitch, v.w, v.h, hipMemcpyDeviceToHost, c->stream));
    } else {
        const uint8_t* src = level == 0 ? d_gray : c->pb.d_pyr + v.off;
        HIPCHK(c, hipMemcpy2DAsync(out, v.w, src, v.pitch, v.w, v.h, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MO_OK;
}

extern "C" int mo_dbg_blur_level(mo_ctx* c, int frame, int level, uint8_t* out, int* lw, int* lh, int* resize_blur) {
    if (!c) return MO_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));  // (not MO_ENTER: what the last extraction left in d_blur is what this probe reads)
    if (!c->plan_valid) return mo_fail(c, MO_ERR_ARG, "no extraction has run on this context");
    if (level < 0 || level >= c->plan.nlevels) return mo_fail(c, MO_ERR_ARG, "level out of range");
    if (frame < 0 || frame >= c->pb.batch_alloc) return mo_fail(c, MO_ERR_ARG, "frame out of range");
    const LevelInfo& v = c->plan.lv[level];
    *lw = v.w; *lh = v.h;
    if (resize_blur) *resize_blur = c->pb.rb_ok ? 1 : 0;
    HIPCHK(c, hipMemcpy2DAsync(out, v.w, c->pb.d_blur + (size_t)frame * c->plan.blur_stride + v.boff, v.bpitch, v.w, v.h,
                               hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MO_OK;
}

extern "C" int mo_dbg_fast_level(mo_ctx* c, const mo_orb_params* p, const uint8_t* gray, int w, int h, int level,
                                 int32_t* xys, int cap, int* n) {
    if (!c) return MO_ERR_ARG;
    MO_ENTER(c);
    int rc = mo_build_plan(c, p, w, h, 1);
    if (rc) return rc;
    if (level < 0 || level >= c->plan.nlevels) return mo_fail(c, MO_ERR_ARG, "level out of range");
    const uint8_t* d_gray = nullptr;
    if ((rc = stage_images(c, gray, w, h, w, 1, 1, &d_gray))) return rc;
    if ((rc = orb_launch_pyramid(c, d_gray, 1, c->plan.nlevels, 0))) return rc;
    if ((rc = orb_launch_fast(c, d_gray, 1))) return rc;
    const LevelInfo& v = c->plan.lv[level];
    std::vector<int> cnt(std::max(v.nstrips, 1));
    std::vector<uint32_t> ent((size_t)std::max(v.cand_cap, 1));
    if (v.nstrips > 0) {
        HIPCHK(c, hipMemcpyAsync(cnt.data(), c->pb.d_strip_cnt + v.strip_base, v.nstrips * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(ent.data(), c->pb.d_cand + v.cand_off, (size_t)v.cand_cap * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int k = 0;
    for (int s = 0; s < v.nstrips; s++)
        for (int i = 0; i < cnt[s]; i++) {
            uint32_t e = ent[(size_t)s * v.strip_cap + i];
            if (k < cap) { xys[3 * k] = e & 0xFFF; xys[3 * k + 1] = (e >> 12) & 0xFFF; xys[3 * k + 2] = e >> 24; }
            k++;
        }
    *n = k;
    return MO_OK;
}

extern "C" int mo_dbg_retain_best(mo_ctx* c, const float* resp, int n, int n_points, int select_order, int32_t* order,
                                  int* n_out) {
    if (!c) return MO_ERR_ARG;
    MO_ENTER(c);
    if (n <= 0) { *n_out = 0; return MO_OK; }
    DevBuf<float> d_r; DevBuf<int32_t> d_o; DevBuf<int> d_n;  // (freed on every return)
    int rc;
    if ((rc = d_r.reserve_exact(c, (size_t)n)) || (rc = d_o.reserve_exact(c, (size_t)n)) || (rc = d_n.reserve_exact(c, 1))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_r, resp, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((rc = orb_launch_retain_probe(c, d_r, n, n_points, select_order, d_o, d_n))) return rc;
    HIPCHK(c, hipMemcpyAsync(n_out, d_n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(order, d_o, (size_t)(*n_out) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MO_OK;
}
