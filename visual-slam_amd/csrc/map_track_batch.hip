// map_track_batch.hip -- a batch of frames tracked against the device map in one chain (mo_map_track_batch in include/vslam_amd.h).
// The rule: frame i's results are mo_map_track's for that frame alone, integers equal and doubles equal bit for bit.
//
// The tracker is map_track.h's, the one mo_map_track runs: one TrackRes per frame, the stage kernels of map_track.hip launched with one
// workgroup per frame over the [frame][stride] buffers below, the candidate tail (trk_claim) and the host front.  The batch's own: the
// staging, the local points as a list, and k_tb_search, which maps threads to (local point, frame) and keeps a frame's workgroups on one XCD.
//
// Chain (one synchronisation, the copy-out; a frame's retry and early exits are flags in its TrackRes that every later workgroup of that
// frame reads first):
//   staging         (map_frames.h, shared with mo_map_relocalize_batch) host frames packed into pinned memory and uploaded in one copy per array, resident frames copied on the device,
//                   into [frame][stride] batch buffers; the store's spare slot is not used
//   k_trk_init      one workgroup per frame: its result block, keys and per-keypoint outputs; a frame without keypoints starts ended
//   k_trk_rep       (trk_launch_rep, as mo_map_track runs it) local-map membership, representative descriptors, octaves: once per batch
//   k_tb_count / k_tb_scan / k_tb_scatter   the local points as an ascending index list: per-block counts, their scan, the scatter
//   k_trk_grid      one workgroup per frame: stable counting sort of its keypoints into the 64 x 48 cells
//   per pass, per attempt:
//     k_tb_search   workgroups over (list block, frame), one thread per (local point, frame), list blocks strided inside a workgroup
//     k_trk_compact one workgroup per frame
//   k_trk_refine    one workgroup of 256 per frame
// Integer atomics only (sums and minima commute), fixed-order f64 reductions: equal inputs give equal bytes on every run.
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"
#include "map_store.h"
#include "map_frames.h"
#include "map_track.h"
#include "ba.h"           // pnp.h comes with it

#define TB_XCDS 8            // workgroups b and b + 8 of a launch share an XCD and its L2 (observed dispatch order; used for speed only)
#define TB_SEARCH_WGS 2048   // workgroups a search launch aims at over all frames ...
#ifndef TB_MIN_LB
#define TB_MIN_LB 128         // ... with at least this many per frame (fewer frames in flight per XCD: their rows stay in its L2)
#endif

struct TbHead {                           // per batch
    int32_t n_local, n_list;              // points of the local map (k_trk_rep's count), entries of the local list (the scan's total)
};

struct TrackBatchBufs : MapFeature {
    DevBuf<mo_keypoint> fk;               // [frame][stride] staged keypoints
    DevBuf<uint8_t> fdesc;                // [frame][stride][32]
    DevBuf<int32_t> fcnt;                 // [frame] rows of each frame
    DevBuf<double> pose0;                 // [frame][12]
    DevBuf<uint8_t> rep;                  // [point][32] representative descriptors
    DevBuf<int32_t> oct;                  // [point] ref_octave (TK_NOT_LOCAL: not in the local map)
    DevBuf<int32_t> part;                 // [point block] local points of each block of 256, then their exclusive scan
    DevBuf<int32_t> list;                 // [n_list] the local points, ascending
    DevBuf<int32_t> cell;                 // [frame][TK_CELLS + 1]
    DevBuf<int32_t> sorted;               // [frame][stride]
    DevBuf<unsigned long long> key;       // [frame][stride]
    DevBuf<TrkMatch> match;               // [frame][stride]
    DevBuf<uint8_t> minl;                 // [frame][stride]
    DevBuf<int32_t> qpt, qdist; DevBuf<uint8_t> qinl;   // [frame][stride]
    DevBuf<TrackRes> res;                 // [frame]
    ResBlock<TbHead> head;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) {
        f(fk); f(fdesc); f(fcnt); f(pose0); f(rep); f(oct); f(part); f(list); f(cell); f(sorted); f(key); f(match); f(minl); f(qpt); f(qdist);
        f(qinl); f(res); f(head);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
    // pinned host sides (not device scratch): the packed host frames on the way in, the result blocks and per-keypoint rows on the way out
    PinnedBuf<mo_keypoint> h_fk; PinnedBuf<uint8_t> h_fdesc; PinnedBuf<int32_t> h_fcnt; PinnedBuf<double> h_pose0;
    PinnedBuf<TrackRes> h_res; PinnedBuf<int32_t> h_qpt, h_qdist; PinnedBuf<uint8_t> h_qinl;
};

// ---- the local list: count per block of 256 points, one-workgroup scan of the counts, scatter in point order ---------------------------
__global__ __launch_bounds__(256) void k_tb_count(int n_pts, const int32_t* __restrict__ oct, int32_t* __restrict__ part) {
    __shared__ int cnt[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool local = i < n_pts && oct[i] != TK_NOT_LOCAL;
    const unsigned long long b = __ballot(local);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = (int)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

__global__ __launch_bounds__(1024) void k_tb_scan(int n_blocks, int32_t* __restrict__ part, TbHead* __restrict__ head) {
    __shared__ int lw[40];
    int run = 0;
    for (int b = 0; b < n_blocks; b += 1024) {
        const int j = b + threadIdx.x;
        const int v = j < n_blocks ? part[j] : 0;
        int tot;
        const int r = block_excl_scan(v, lw, &tot);
        if (j < n_blocks) part[j] = run + r;
        run += tot;
    }
    if (threadIdx.x == 0) head->n_list = run;
}

__global__ __launch_bounds__(256) void k_tb_scatter(int n_pts, const int32_t* __restrict__ oct, const int32_t* __restrict__ part, int32_t* __restrict__ list) {
    __shared__ int lw[40];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool local = i < n_pts && oct[i] != TK_NOT_LOCAL;
    int tot;
    const int r = block_excl_scan(local ? 1 : 0, lw, &tot);
    if (local) list[part[blockIdx.x] + r] = i;   // (part + r < n_list <= n_pts: the list has n_pts entries)
}

// k_trk_search over (list block, frame).  The launch is 1-D over TB_XCDS * per workgroups; workgroup b takes the pair
// v = (b % 8) * per + b / 8 of the frame-major order v = frame * lb_per_frame + list block, so that the workgroups of one frame - which
// all read that frame's descriptors, keypoints, cells and keys - are dealt to one XCD and meet them in its L2.  A workgroup strides over
// the list blocks lb, lb + lb_per_frame, ...; one thread handles one (local point, frame).
__global__ __launch_bounds__(256) void k_tb_search(TrackPrm prm, TrkFrames fr, int n_frames, int pass, int attempt, int lb_per_frame, int per,
                                                   const float* __restrict__ xyz, const uint8_t* __restrict__ rep, const int32_t* __restrict__ oct,
                                                   const int32_t* __restrict__ list, const TbHead* __restrict__ head) {
#ifdef TB_NO_XCD_REMAP
    const int v = blockIdx.x;
#else
    const int v = (int)(blockIdx.x % TB_XCDS) * per + (int)(blockIdx.x / TB_XCDS);
#endif
    if (v >= lb_per_frame * n_frames) return;
    const int f = v / lb_per_frame, lb = v - f * lb_per_frame;
    TrackRes* __restrict__ res = fr.res + f;
    if (!trk_active(res, attempt)) return;
    const size_t at = fr.at(f);
    const mo_keypoint* __restrict__ fk = fr.fk + at;
    const uint8_t* __restrict__ fdesc = fr.fdesc + at * 32;
    const int32_t* __restrict__ cell = fr.cells(f);
    const int32_t* __restrict__ sorted = fr.sorted + at;
    unsigned long long* __restrict__ key = fr.key + at;
    const int n_list = head->n_list;
    double R[9], t[3], P[12];
    pose_split(res->pose, R, t);
    pnp_projection(prm.K, R, t, P);
    const double rad = attempt ? 2.0 * prm.radius[pass] : prm.radius[pass];
    for (int base = lb * 256; base < n_list; base += lb_per_frame * 256) {
        const int j = base + threadIdx.x;
        int i = 0, ro = 0;
        bool cand = false;
        double uu = 0.0, vv = 0.0;
        if (j < n_list) {
            i = list[j];
            ro = oct[i];
            cand = trk_project(P, xyz[(size_t)i * 3], xyz[(size_t)i * 3 + 1], xyz[(size_t)i * 3 + 2], prm.w, prm.h, &uu, &vv);
        }
        wave_count_add(cand, &res->cand);
        if (!cand) continue;
        const double r = rad * trk_scale(prm.sf, ro);
        trk_claim(prm, i, rep, fdesc, key, [&](auto visit) { trk_window(uu, vv, r, ro, prm.w, prm.h, cell, sorted, fk, visit); });
    }
}

extern "C" int mo_map_track_batch(mo_map* m, const mo_frame_ref* frames, int32_t n_frames, const double K[9], const double* pose0,
                                  const mo_map_track_params* prm, mo_map_track_batch_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!K || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (n_frames < 0 || n_frames > MO_TRACK_BATCH_MAX) return mo_fail(c, MO_ERR_ARG, "n_frames must be in 0 .. MO_TRACK_BATCH_MAX");
    if (n_frames > 0 && (!frames || !pose0 || !out->pose || !out->pass_pose || !out->pass_radius || !out->pass_cand || !out->pass_matches ||
                         !out->pass_inliers || !out->n_pass_run || !out->ok || !out->from_token))
        return mo_fail(c, MO_ERR_ARG, "NULL argument");
    int rc;
    if ((rc = track_check(c, prm, pose0, (size_t)n_frames))) return rc;
    if (out->stride < 0) return mo_fail(c, MO_ERR_ARG, "stride must be >= 0");
    MAP_ENTER(m);
    HostClock clk(c);
    out->n_local = 0; out->n_ok = 0;
    if (n_frames == 0) return MO_OK;
    const int nf = n_frames, stride = out->stride;
    TrackBatchBufs& b = map_feature<TrackBatchBufs>(m);
    auto dst = [&](int i) {   // frame i's rows of the caller's outputs
        const size_t at = (size_t)i * stride, pi = (size_t)i * TK_MAX_PASS;
        return TrackDst{out->point ? out->point + at : nullptr, out->dist ? out->dist + at : nullptr, out->inlier ? out->inlier + at : nullptr,
                        out->pose + (size_t)i * 12, out->pass_pose + pi * 12, out->pass_radius + pi, out->pass_cand + pi, out->pass_matches + pi,
                        out->pass_inliers + pi, out->n_pass_run + i, out->ok + i};
    };
    if ((rc = mo_reserve(c, b.h_fcnt, (size_t)nf, b.h_pose0, (size_t)nf * 12, b.h_res, (size_t)nf))) return rc;
    // the frames looked up: every row count known and checked before anything is written
    BatchFrames bf;
    if ((rc = batch_frames_lookup(c, frames, nf, stride, "a frame has more rows than stride", b.h_fcnt, &bf))) return rc;
    const std::vector<int>& slot = bf.slot;
    const bool any_rows = bf.any_rows;
    for (int i = 0; i < nf; i++) {
        track_defaults(dst(i), pose0 + (size_t)i * 12);
        track_row_defaults(dst(i), b.h_fcnt[i]);
        out->from_token[i] = slot[i] >= 0;
    }
    if (m->pos_slot.empty() || m->n_pts == 0) return MO_OK;   // (nothing to search against: not tracked, not an error)
    if ((rc = map_int32_guard(m)) || (rc = upload_pos_slot(m))) return rc;
    const int n_kf = (int)m->pos_slot.size();
    const size_t np = (size_t)m->n_pts, rows = std::max((size_t)nf * stride, (size_t)1);
    const unsigned pblocks = (unsigned)((m->n_pts + 255) / 256);
    if ((rc = mo_reserve(c, b.fk, rows, b.fdesc, rows * 32, b.fcnt, (size_t)nf, b.pose0, (size_t)nf * 12, b.rep, np * 32, b.oct, np, b.part, (size_t)pblocks,
                         b.list, np, b.cell, (size_t)nf * (TK_CELLS + 1), b.sorted, rows, b.key, rows, b.match, rows, b.minl, rows, b.qpt, rows, b.qdist,
                         rows, b.qinl, rows, b.res, (size_t)nf, b.head)))
        return rc;
    if ((rc = batch_frames_reserve_host(c, bf, rows, b.h_fk, b.h_fdesc))) return rc;
    if ((out->point && (rc = b.h_qpt.reserve(c, rows))) || (out->dist && (rc = b.h_qdist.reserve(c, rows))) || (out->inlier && (rc = b.h_qinl.reserve(c, rows))))
        return rc;
    mo_stage_begin(c);
    // ---- staging (map_frames.h): the host frames in one upload per array, then the resident frames device to device
    if ((rc = batch_frames_stage(c, frames, nf, (size_t)stride, bf, b.h_fcnt, b.h_fk, b.h_fdesc, b.fk, b.fdesc))) return rc;
    std::memcpy(b.h_pose0, pose0, (size_t)nf * 12 * sizeof(double));
    HIPCHK(c, hipMemcpyAsync(b.fcnt, b.h_fcnt, (size_t)nf * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.pose0, b.h_pose0, (size_t)nf * 12 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    mo_stage_mark(c, "tb_stage");
    const TrackPrm p = track_prm(K, prm);
    const TrkFrames fr = trk_frames(b, b.fk, b.fdesc, b.fcnt, b.pose0, stride);
    const float* xyz = m->P[m->cur].view().xyz;
    // ---- shared preparation, once per batch
    if ((rc = trk_launch_init(c, fr, nf, nullptr, &b.head.p->n_local))) return rc;
    if ((rc = trk_launch_rep(m, map_window_lo(prm->window, n_kf), b.rep, b.oct, &b.head.p->n_local))) return rc;
    hipLaunchKernelGGL(k_tb_count, dim3(pblocks), dim3(256), 0, c->stream, (int)m->n_pts, b.oct, b.part);
    hipLaunchKernelGGL(k_tb_scan, dim3(1), dim3(1024), 0, c->stream, (int)pblocks, b.part, b.head);
    hipLaunchKernelGGL(k_tb_scatter, dim3(pblocks), dim3(256), 0, c->stream, (int)m->n_pts, b.oct, b.part, b.list);
    HIPCHK(c, hipGetLastError());
    if ((rc = trk_launch_grid(c, b.fk, stride, b.fcnt, nullptr, 0, nf, prm->w, prm->h, b.cell, b.sorted))) return rc;
    mo_stage_mark(c, "tb_prep");
    // list blocks a frame's workgroups stride over: all of them when the batch is small, fewer per frame as it grows
    const int lb_per_frame = (int)std::min<unsigned>(pblocks, (unsigned)std::max(TB_MIN_LB, (TB_SEARCH_WGS + nf - 1) / nf));
    const int per = (lb_per_frame * nf + TB_XCDS - 1) / TB_XCDS;
    for (int k = 0; k < prm->n_pass; k++) {
        for (int a = 0; a < 2; a++) {
            if (any_rows)
                hipLaunchKernelGGL(k_tb_search, dim3((unsigned)(per * TB_XCDS)), dim3(256), 0, c->stream, p, fr, nf, k, a, lb_per_frame, per, xyz, b.rep, b.oct,
                                   b.list, b.head);
            if ((rc = trk_launch_compact(c, p, fr, nf, k, a, xyz))) return rc;
        }
        mo_stage_mark(c, "tb_search");
        if ((rc = trk_launch_refine(c, p, fr, nf, k))) return rc;
        mo_stage_mark(c, "tb_refine");
    }
    // ---- copy-out: the result blocks, and one download per requested per-keypoint array
    HIPCHK(c, hipMemcpyAsync(b.h_res, b.res, (size_t)nf * sizeof(TrackRes), hipMemcpyDeviceToHost, c->stream));
    if ((rc = b.head.download(c))) return rc;
    if (any_rows) {
        if (out->point) HIPCHK(c, hipMemcpyAsync(b.h_qpt, b.qpt, rows * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->dist) HIPCHK(c, hipMemcpyAsync(b.h_qdist, b.qdist, rows * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->inlier) HIPCHK(c, hipMemcpyAsync(b.h_qinl, b.qinl, rows, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = map_sync(c, clk))) return rc;
    out->n_local = b.head.host().n_local;
    for (int i = 0; i < nf; i++) {
        const size_t at = (size_t)i * stride, n = (size_t)b.h_fcnt[i];
        out->n_ok += track_result(dst(i), b.h_res[i], prm);
        if (out->point) std::memcpy(out->point + at, b.h_qpt + at, n * 4);
        if (out->dist) std::memcpy(out->dist + at, b.h_qdist + at, n * 4);
        if (out->inlier) std::memcpy(out->inlier + at, b.h_qinl + at, n);
    }
    return MO_OK;
}
