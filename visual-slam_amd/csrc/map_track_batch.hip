// map_track_batch.hip -- a batch of frames tracked against the device map in one chain (mo_map_track_batch in include/vslam_amd.h).
// The rule: frame i's results are mo_map_track's for that frame alone, integers equal and doubles equal bit for bit.
//
// Second copies, on purpose: k_tb_grid, k_tb_search, k_tb_compact and k_tb_refine restate k_trk_grid, k_trk_search, k_trk_compact and
// k_trk_refine of map_track.hip with a frame index in front of every per-frame array; nothing of map_track.hip is edited or lifted into
// a header, so its kernels keep the instruction sequences they had (profiles/track_batch_isa.txt; k_trk_search_frustum is a kernel of
// its own for the same reason, profiles/frustum_isa.txt).  The arithmetic they share is the inline code of map_search.h, map_store.h,
// pnp.h and ba.h, called with the same operands in the same order; tests/test_gpu_track_batch.py compares the two copies byte for byte.
//
// Chain (one synchronisation, the copy-out; a frame's retry and early exits are flags in its TbRes that every later workgroup of that
// frame reads first):
//   staging         host frames packed into pinned memory and uploaded in one copy per array, resident frames copied on the device,
//                   into [frame][stride] batch buffers; the store's spare slot is not used
//   k_tb_init       one workgroup per frame: its result block, keys and per-keypoint outputs; a frame without keypoints starts ended
//   k_trk_rep       (trk_launch_rep, as mo_map_track runs it) local-map membership, representative descriptors, octaves: once per batch
//   k_tb_count / k_tb_scan / k_tb_scatter   the local points as an ascending index list: per-block counts, their scan, the scatter
//   k_tb_grid       one workgroup per frame: stable counting sort of its keypoints into the 64 x 48 cells
//   per pass, per attempt:
//     k_tb_search   workgroups over (list block, frame), one thread per (local point, frame), list blocks strided inside a workgroup
//     k_tb_compact  one workgroup per frame
//   k_tb_refine     one workgroup of 256 per frame
// Integer atomics only (sums and minima commute), fixed-order f64 reductions: equal inputs give equal bytes on every run.
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"
#include "map_store.h"
#include "map_search.h"
#include "ba.h"

#define TB_GRID_BLOCK 1024
#define TB_CELLS_PER_THREAD (TK_CELLS / TB_GRID_BLOCK)
#define TB_MAX_PASS 4
#define TB_REFINE_BLOCK 256
#define TB_XCDS 8            // workgroups b and b + 8 of a launch share an XCD and its L2 (observed dispatch order; used for speed only)
#define TB_SEARCH_WGS 2048   // workgroups a search launch aims at over all frames ...
#ifndef TB_MIN_LB
#define TB_MIN_LB 128         // ... with at least this many per frame (fewer frames in flight per XCD: their rows stay in its L2)
#endif
static_assert(TK_CELLS % TB_GRID_BLOCK == 0, "cells per thread");

struct TbPrm {                            // mo_map_track's TrackPrm without the pose, which is per frame
    double K[9], radius[TB_MAX_PASS], sf, ratio, chi2;
    int w, h, max_dist, min_matches;
    int n_frames, stride;
};

struct TbRes {                            // per frame, the fields of mo_map_track's result block
    double pose[12];
    double pass_pose[TB_MAX_PASS][12];
    double pass_radius[TB_MAX_PASS];
    int32_t pass_cand[TB_MAX_PASS], pass_matches[TB_MAX_PASS], pass_inliers[TB_MAX_PASS];
    int32_t n_run, n_done;
    int32_t ended, retry;
    int32_t cand, n_match;
};

struct TbHead {                           // per batch
    int32_t n_local, n_list;              // points of the local map (k_trk_rep's count), entries of the local list (the scan's total)
};

struct TbMatch {
    float X, Y, Z, x, y;
    int32_t octave, q, p;
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
    DevBuf<TbMatch> match;                // [frame][stride]
    DevBuf<uint8_t> minl;                 // [frame][stride]
    DevBuf<int32_t> qpt, qdist; DevBuf<uint8_t> qinl;   // [frame][stride]
    DevBuf<TbRes> res;                    // [frame]
    ResBlock<TbHead> head;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) {
        f(fk); f(fdesc); f(fcnt); f(pose0); f(rep); f(oct); f(part); f(list); f(cell); f(sorted); f(key); f(match); f(minl); f(qpt); f(qdist);
        f(qinl); f(res); f(head);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
    // pinned host sides (not device scratch): the packed host frames on the way in, the result blocks and per-keypoint rows on the way out
    PinnedBuf<mo_keypoint> h_fk; PinnedBuf<uint8_t> h_fdesc; PinnedBuf<int32_t> h_fcnt; PinnedBuf<double> h_pose0;
    PinnedBuf<TbRes> h_res; PinnedBuf<int32_t> h_qpt, h_qdist; PinnedBuf<uint8_t> h_qinl;
};

__device__ __forceinline__ bool tb_active(const TbRes* res, int attempt) {
    return !res->ended && (attempt == 0 || res->retry);
}

// one workgroup per frame
__global__ __launch_bounds__(256) void k_tb_init(int stride, const int32_t* __restrict__ fcnt, const double* __restrict__ pose0, TbRes* __restrict__ res_all,
                                                 TbHead* __restrict__ head, unsigned long long* __restrict__ key, int32_t* __restrict__ qpt,
                                                 int32_t* __restrict__ qdist, uint8_t* __restrict__ qinl) {
    const int f = blockIdx.x, n = fcnt[f];
    const size_t at = (size_t)f * stride;
    for (int q = threadIdx.x; q < n; q += 256) { key[at + q] = TK_NONE; qpt[at + q] = -1; qdist[at + q] = -1; qinl[at + q] = 0; }
    if (threadIdx.x == 0) {
        TbRes* res = res_all + f;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int i = 0; i < 12; i++) res->pose[i] = pose0[(size_t)f * 12 + i];
        for (int k = 0; k < TB_MAX_PASS; k++) {
            for (int i = 0; i < 12; i++) res->pass_pose[k][i] = nan;
            res->pass_radius[k] = 0.0;
            res->pass_cand[k] = 0; res->pass_matches[k] = 0; res->pass_inliers[k] = 0;
        }
        res->n_run = 0; res->n_done = 0; res->ended = n == 0; res->retry = 0; res->cand = 0; res->n_match = 0;
        if (f == 0) { head->n_local = 0; head->n_list = 0; }
    }
}

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

// one workgroup per frame: k_trk_grid's stable counting sort over the batch buffers
__global__ __launch_bounds__(TB_GRID_BLOCK) void k_tb_grid(const mo_keypoint* __restrict__ fk_all, int stride, const int32_t* __restrict__ fcnt, int w, int h,
                                                           int32_t* __restrict__ cell, int32_t* __restrict__ sorted) {
    const mo_keypoint* __restrict__ fk = fk_all + (size_t)blockIdx.x * stride;
    const int n = min(fcnt[blockIdx.x], stride);
    cell += (size_t)blockIdx.x * (TK_CELLS + 1);
    sorted += (size_t)blockIdx.x * stride;
    __shared__ int cur[TK_CELLS];
    __shared__ int lw[40];
    const int tid = threadIdx.x;
    for (int c = tid; c < TK_CELLS; c += TB_GRID_BLOCK) cur[c] = 0;
    __syncthreads();
    for (int q = tid; q < n; q += TB_GRID_BLOCK) atomicAdd(cur + trk_cy(fk[q].y, h) * TK_GX + trk_cx(fk[q].x, w), 1);
    __syncthreads();
    int v[TB_CELLS_PER_THREAD], s = 0;
    for (int j = 0; j < TB_CELLS_PER_THREAD; j++) { v[j] = cur[tid * TB_CELLS_PER_THREAD + j]; s += v[j]; }
    int tot;
    int base = block_excl_scan(s, lw, &tot);
    for (int j = 0; j < TB_CELLS_PER_THREAD; j++) {
        cur[tid * TB_CELLS_PER_THREAD + j] = base;
        cell[tid * TB_CELLS_PER_THREAD + j] = base;
        base += v[j];
    }
    if (tid == 0) cell[TK_CELLS] = tot;
    __syncthreads();
    for (int q = tid; q < n; q += TB_GRID_BLOCK) sorted[atomicAdd(cur + trk_cy(fk[q].y, h) * TK_GX + trk_cx(fk[q].x, w), 1)] = q;
    __syncthreads();
    for (int j = 0; j < TB_CELLS_PER_THREAD; j++) {
        const int c = tid * TB_CELLS_PER_THREAD + j;
        sort_run(sorted + cell[c], cur[c] - cell[c]);
    }
}

// k_trk_search over (list block, frame).  The launch is 1-D over TB_XCDS * per workgroups; workgroup b takes the pair
// v = (b % 8) * per + b / 8 of the frame-major order v = frame * lb_per_frame + list block, so that the workgroups of one frame - which
// all read that frame's descriptors, keypoints, cells and keys - are dealt to one XCD and meet them in its L2.  A workgroup strides over
// the list blocks lb, lb + lb_per_frame, ...; one thread handles one (local point, frame).
__global__ __launch_bounds__(256) void k_tb_search(TbPrm prm, int pass, int attempt, int lb_per_frame, int per, const float* __restrict__ xyz,
                                                   const uint8_t* __restrict__ rep, const int32_t* __restrict__ oct, const int32_t* __restrict__ list,
                                                   const TbHead* __restrict__ head, const mo_keypoint* __restrict__ fk_all,
                                                   const uint8_t* __restrict__ fdesc_all, const int32_t* __restrict__ cell_all,
                                                   const int32_t* __restrict__ sorted_all, unsigned long long* __restrict__ key_all,
                                                   TbRes* __restrict__ res_all) {
#ifdef TB_NO_XCD_REMAP
    const int v = blockIdx.x;
#else
    const int v = (int)(blockIdx.x % TB_XCDS) * per + (int)(blockIdx.x / TB_XCDS);
#endif
    if (v >= lb_per_frame * prm.n_frames) return;
    const int f = v / lb_per_frame, lb = v - f * lb_per_frame;
    TbRes* __restrict__ res = res_all + f;
    if (!tb_active(res, attempt)) return;
    const size_t at = (size_t)f * prm.stride;
    const mo_keypoint* __restrict__ fk = fk_all + at;
    const uint8_t* __restrict__ fdesc = fdesc_all + at * 32;
    const int32_t* __restrict__ cell = cell_all + (size_t)f * (TK_CELLS + 1);
    const int32_t* __restrict__ sorted = sorted_all + at;
    unsigned long long* __restrict__ key = key_all + at;
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
        const uint8_t* d = rep + (size_t)i * 32;
        int bd = INT_MAX, bq = INT_MAX, sd = INT_MAX;
        trk_window(uu, vv, r, ro, prm.w, prm.h, cell, sorted, fk, [&](int q, const mo_keypoint&, double, double) {
            const int dist = trk_ham(d, fdesc + (size_t)q * 32), was = bd;
            if (trk_take(dist, q, bd, bq)) sd = was;
            else if (dist < sd) sd = dist;
        });
        if (bd == INT_MAX || bd > prm.max_dist) continue;
        if (sd != INT_MAX && !((double)bd <= prm.ratio * (double)sd)) continue;
        atomicMin(key + bq, ((unsigned long long)(unsigned)bd << 32) | (unsigned)i);
    }
}

// one workgroup per frame: k_trk_compact
__global__ __launch_bounds__(1024) void k_tb_compact(TbPrm prm, int pass, int attempt, const int32_t* __restrict__ fcnt, const mo_keypoint* __restrict__ fk_all,
                                                     const float* __restrict__ xyz, unsigned long long* __restrict__ key_all, TbMatch* __restrict__ match_all,
                                                     int32_t* __restrict__ qpt_all, int32_t* __restrict__ qdist_all, uint8_t* __restrict__ qinl_all,
                                                     TbRes* __restrict__ res_all) {
    __shared__ int lw[40];
    __shared__ int active;
    const int f = blockIdx.x;
    TbRes* __restrict__ res = res_all + f;
    if (threadIdx.x == 0) active = tb_active(res, attempt);
    __syncthreads();
    if (!active) return;
    const size_t at = (size_t)f * prm.stride;
    const mo_keypoint* __restrict__ fk = fk_all + at;
    unsigned long long* __restrict__ key = key_all + at;
    TbMatch* __restrict__ match = match_all + at;
    int32_t* __restrict__ qpt = qpt_all + at;
    int32_t* __restrict__ qdist = qdist_all + at;
    uint8_t* __restrict__ qinl = qinl_all + at;
    const int n = min(fcnt[f], prm.stride);
    int added = 0;
    for (int b = 0; b < n; b += 1024) {
        const int q = b + threadIdx.x;
        const unsigned long long k = q < n ? key[q] : TK_NONE;
        const bool has = k != TK_NONE;
        int tot;
        const int r = block_excl_scan(has ? 1 : 0, lw, &tot);
        if (q < n) {
            const int p = has ? (int)(k & 0xffffffffu) : -1;
            qpt[q] = p;
            qdist[q] = has ? (int)(k >> 32) : -1;
            qinl[q] = 0;
            key[q] = TK_NONE;
            if (has) {
                const mo_keypoint kp = fk[q];
                TbMatch mt;
                mt.X = xyz[(size_t)p * 3]; mt.Y = xyz[(size_t)p * 3 + 1]; mt.Z = xyz[(size_t)p * 3 + 2];
                mt.x = kp.x; mt.y = kp.y; mt.octave = kp.octave; mt.q = q; mt.p = p;
                match[added + r] = mt;
            }
        }
        added += tot;
    }
    if (threadIdx.x == 0) {
        res->pass_cand[pass] = res->cand;
        res->cand = 0;
        res->pass_matches[pass] = added;
        res->pass_radius[pass] = attempt ? 2.0 * prm.radius[pass] : prm.radius[pass];
        res->n_match = added;
        res->n_run = pass + 1;
        const int few = added < prm.min_matches;
        if (few && attempt) res->ended = 1;
        res->retry = few && !attempt;
    }
}

// inlier test of one match under (R, t): k_trk_refine's
__device__ __forceinline__ bool tb_inlier(const TbPrm& prm, const double* R, const double* t, const TbMatch& mt) {
    const double X = mt.X, Y = mt.Y, Z = mt.Z;
    const double xc = R[0] * X + R[1] * Y + R[2] * Z + t[0];
    const double yc = R[3] * X + R[4] * Y + R[5] * Z + t[1];
    const double zc = R[6] * X + R[7] * Y + R[8] * Z + t[2];
    const double* K = prm.K;
    const double p0 = K[0] * xc + K[1] * yc + K[2] * zc, p1 = K[3] * xc + K[4] * yc + K[5] * zc, p2 = K[6] * xc + K[7] * yc + K[8] * zc;
    const double du = p0 / p2 - (double)mt.x, dv = p1 / p2 - (double)mt.y;
    return zc > 0.0 && ba_info(prm.sf, mt.octave) * (du * du + dv * dv) <= prm.chi2;
}

// one workgroup of 256 per frame: k_trk_refine, operation for operation (per-thread partial sums in match order with stride 256, the
// wave shuffle tree, the four wave sums added left to right by thread 0, one Cholesky solve per step, four rounds)
__global__ __launch_bounds__(TB_REFINE_BLOCK) void k_tb_refine(TbPrm prm, int pass, const TbMatch* __restrict__ match_all, uint8_t* __restrict__ minl_all,
                                                               uint8_t* __restrict__ qinl_all, TbRes* __restrict__ res_all) {
    constexpr int NW = TB_REFINE_BLOCK / 64;
    __shared__ double red[NW][27];
    __shared__ double sRt[12];
    __shared__ int flag, cnt[NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    TbRes* __restrict__ res = res_all + blockIdx.x;
    if (tid == 0) flag = !res->ended && !res->retry;
    __syncthreads();
    if (!flag) return;
    const size_t at = (size_t)blockIdx.x * prm.stride;
    const TbMatch* __restrict__ match = match_all + at;
    uint8_t* __restrict__ minl = minl_all + at;
    uint8_t* __restrict__ qinl = qinl_all + at;
    const int m = res->n_match;
    double R[9], t[3];
    pose_split(res->pose, R, t);
    for (int j = tid; j < m; j += TB_REFINE_BLOCK) minl[j] = 1;
    int n_inl = m;
    for (int round = 0; round < 4; round++) {
        const double huber2 = round < 3 ? prm.chi2 : 0.0;
        for (int it = 0; it < 10; it++) {
            double a[27];
            for (int i = 0; i < 27; i++) a[i] = 0.0;
            for (int j = tid; j < m; j += TB_REFINE_BLOCK) {
                if (!minl[j]) continue;
                const TbMatch mt = match[j];
                pnp_gn_accumulate_w(prm.K, R, t, mt.X, mt.Y, mt.Z, mt.x, mt.y, ba_info(prm.sf, mt.octave), huber2, a, a + 21);
            }
            for (int i = 0; i < 27; i++) a[i] = wave_sum_all(a[i]);
            if (lane == 0)
                for (int i = 0; i < 27; i++) red[wv][i] = a[i];
            __syncthreads();
            if (tid == 0) {
                double s[27];
                for (int i = 0; i < 27; i++) {
                    s[i] = red[0][i];
                    for (int w = 1; w < NW; w++) s[i] += red[w][i];
                }
                double step = 0.0;
                const bool ok = pnp_gn_update(s, s + 21, R, t, &step);
                for (int j = 0; j < 9; j++) sRt[j] = R[j];
                for (int j = 0; j < 3; j++) sRt[9 + j] = t[j];
                flag = !ok || step < 1e-12;
            }
            __syncthreads();
            for (int j = 0; j < 9; j++) R[j] = sRt[j];
            for (int j = 0; j < 3; j++) t[j] = sRt[9 + j];
            const int stop = flag;
            __syncthreads();
            if (stop) break;
        }
        int n = 0;
        for (int j = tid; j < m; j += TB_REFINE_BLOCK) {
            const bool in = tb_inlier(prm, R, t, match[j]);
            minl[j] = in;
            n += in;
        }
        n = wave_sum_int(n);
        if (lane == 0) cnt[wv] = n;
        __syncthreads();
        n_inl = 0;
        for (int w = 0; w < NW; w++) n_inl += cnt[w];
        __syncthreads();
        if (n_inl < 10) break;
    }
    for (int j = tid; j < m; j += TB_REFINE_BLOCK) qinl[match[j].q] = minl[j];
    if (tid == 0) {
        for (int j = 0; j < 3; j++) {
            for (int l = 0; l < 3; l++) res->pose[j * 4 + l] = res->pass_pose[pass][j * 4 + l] = R[j * 3 + l];
            res->pose[j * 4 + 3] = res->pass_pose[pass][j * 4 + 3] = t[j];
        }
        res->pass_inliers[pass] = n_inl;
        res->n_done = pass + 1;
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
    if (prm->n_pass < 1 || prm->n_pass > TB_MAX_PASS) return mo_fail(c, MO_ERR_ARG, "n_pass must be in 1 .. 4");
    if (prm->w <= 0 || prm->h <= 0) return mo_fail(c, MO_ERR_ARG, "w and h must be > 0");
    if (prm->window < 0) return mo_fail(c, MO_ERR_ARG, "window must be >= 0");
    if (!(prm->scale_factor > 0.0) || !std::isfinite(prm->scale_factor)) return mo_fail(c, MO_ERR_ARG, "scale_factor must be finite and > 0");
    if (!(prm->chi2 >= 0.0) || !std::isfinite(prm->ratio)) return mo_fail(c, MO_ERR_ARG, "chi2 must be >= 0 and ratio finite");
    for (int k = 0; k < prm->n_pass; k++)
        if (!(prm->radius[k] >= 0.0) || !std::isfinite(prm->radius[k])) return mo_fail(c, MO_ERR_ARG, "radius must be finite and >= 0");
    if (out->stride < 0) return mo_fail(c, MO_ERR_ARG, "stride must be >= 0");
    for (size_t i = 0; i < (size_t)n_frames * 12; i++)
        if (!std::isfinite(pose0[i])) return mo_fail(c, MO_ERR_ARG, "pose0 must be finite");
    MAP_ENTER(m);
    HostClock clk(c);
    out->n_local = 0; out->n_ok = 0;
    if (n_frames == 0) return MO_OK;
    const int nf = n_frames, stride = out->stride;
    TrackBatchBufs& b = map_feature<TrackBatchBufs>(m);
    int rc;
    if ((rc = mo_reserve(c, b.h_fcnt, (size_t)nf, b.h_pose0, (size_t)nf * 12, b.h_res, (size_t)nf))) return rc;
    // the frames looked up: every row count known and checked before anything is written
    std::vector<int> slot(nf);
    bool any_host = false, any_rows = false;
    for (int i = 0; i < nf; i++) {
        int n;
        if ((rc = mo_frame_lookup(c, &frames[i], "frame", &slot[i], &n))) return rc;
        if (n > stride) return mo_fail(c, MO_ERR_ARG, "a frame has more rows than stride");
        b.h_fcnt[i] = n;
        any_host |= slot[i] < 0 && n > 0;
        any_rows |= n > 0;
    }
    for (int i = 0; i < nf; i++) {   // mo_map_track's defaults
        const int n = b.h_fcnt[i];
        const size_t at = (size_t)i * stride;
        for (int j = 0; j < 12; j++) out->pose[(size_t)i * 12 + j] = pose0[(size_t)i * 12 + j];
        for (int j = 0; j < TB_MAX_PASS * 12; j++) out->pass_pose[(size_t)i * TB_MAX_PASS * 12 + j] = NAN;
        for (int k = 0; k < TB_MAX_PASS; k++) {
            out->pass_radius[i * TB_MAX_PASS + k] = 0.0;
            out->pass_cand[i * TB_MAX_PASS + k] = 0; out->pass_matches[i * TB_MAX_PASS + k] = 0; out->pass_inliers[i * TB_MAX_PASS + k] = 0;
        }
        out->n_pass_run[i] = 0; out->ok[i] = 0; out->from_token[i] = slot[i] >= 0;
        if (out->point) for (int q = 0; q < n; q++) out->point[at + q] = -1;
        if (out->dist) for (int q = 0; q < n; q++) out->dist[at + q] = -1;
        if (out->inlier) std::memset(out->inlier + at, 0, (size_t)n);
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
    if (any_host && (rc = mo_reserve(c, b.h_fk, rows, b.h_fdesc, rows * 32))) return rc;
    if ((out->point && (rc = b.h_qpt.reserve(c, rows))) || (out->dist && (rc = b.h_qdist.reserve(c, rows))) || (out->inlier && (rc = b.h_qinl.reserve(c, rows))))
        return rc;
    mo_stage_begin(c);
    // ---- staging: the host frames in one upload per array, then the resident frames device to device
    if (any_host) {
        for (int i = 0; i < nf; i++) {
            if (slot[i] >= 0 || b.h_fcnt[i] == 0) continue;
            const size_t at = (size_t)i * stride, n = (size_t)b.h_fcnt[i];
            std::memcpy(b.h_fk + at, frames[i].kps, n * sizeof(mo_keypoint));
            std::memcpy(b.h_fdesc + at * 32, frames[i].desc, n * 32);
        }
        HIPCHK(c, hipMemcpyAsync(b.fk, b.h_fk, rows * sizeof(mo_keypoint), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b.fdesc, b.h_fdesc, rows * 32, hipMemcpyHostToDevice, c->stream));
    }
    for (int i = 0; i < nf; i++)
        if (slot[i] >= 0 && (rc = mo_frame_copy_rows(c, &frames[i], slot[i], b.h_fcnt[i], b.fk + (size_t)i * stride, b.fdesc + (size_t)i * stride * 32)))
            return rc;
    std::memcpy(b.h_pose0, pose0, (size_t)nf * 12 * sizeof(double));
    HIPCHK(c, hipMemcpyAsync(b.fcnt, b.h_fcnt, (size_t)nf * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.pose0, b.h_pose0, (size_t)nf * 12 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    mo_stage_mark(c, "tb_stage");
    TbPrm p;
    for (int i = 0; i < 9; i++) p.K[i] = K[i];
    for (int k = 0; k < TB_MAX_PASS; k++) p.radius[k] = k < prm->n_pass ? prm->radius[k] : 0.0;
    p.sf = prm->scale_factor; p.ratio = prm->ratio; p.chi2 = prm->chi2;
    p.w = prm->w; p.h = prm->h; p.max_dist = prm->max_dist; p.min_matches = prm->min_matches;
    p.n_frames = nf; p.stride = stride;
    const float* xyz = m->P[m->cur].view().xyz;
    // ---- shared preparation, once per batch
    hipLaunchKernelGGL(k_tb_init, dim3((unsigned)nf), dim3(256), 0, c->stream, stride, b.fcnt, b.pose0, b.res, b.head, b.key, b.qpt, b.qdist, b.qinl);
    if ((rc = trk_launch_rep(m, map_window_lo(prm->window, n_kf), b.rep, b.oct, &b.head.p->n_local))) return rc;
    hipLaunchKernelGGL(k_tb_count, dim3(pblocks), dim3(256), 0, c->stream, (int)m->n_pts, b.oct, b.part);
    hipLaunchKernelGGL(k_tb_scan, dim3(1), dim3(1024), 0, c->stream, (int)pblocks, b.part, b.head);
    hipLaunchKernelGGL(k_tb_scatter, dim3(pblocks), dim3(256), 0, c->stream, (int)m->n_pts, b.oct, b.part, b.list);
    hipLaunchKernelGGL(k_tb_grid, dim3((unsigned)nf), dim3(TB_GRID_BLOCK), 0, c->stream, b.fk, stride, b.fcnt, prm->w, prm->h, b.cell, b.sorted);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "tb_prep");
    // list blocks a frame's workgroups stride over: all of them when the batch is small, fewer per frame as it grows
    const int lb_per_frame = (int)std::min<unsigned>(pblocks, (unsigned)std::max(TB_MIN_LB, (TB_SEARCH_WGS + nf - 1) / nf));
    const int per = (lb_per_frame * nf + TB_XCDS - 1) / TB_XCDS;
    for (int k = 0; k < prm->n_pass; k++) {
        for (int a = 0; a < 2; a++) {
            if (any_rows)
                hipLaunchKernelGGL(k_tb_search, dim3((unsigned)(per * TB_XCDS)), dim3(256), 0, c->stream, p, k, a, lb_per_frame, per, xyz, b.rep, b.oct, b.list,
                                   b.head, b.fk, b.fdesc, b.cell, b.sorted, b.key, b.res);
            hipLaunchKernelGGL(k_tb_compact, dim3((unsigned)nf), dim3(1024), 0, c->stream, p, k, a, b.fcnt, b.fk, xyz, b.key, b.match, b.qpt, b.qdist, b.qinl,
                               b.res);
        }
        HIPCHK(c, hipGetLastError());
        mo_stage_mark(c, "tb_search");
        hipLaunchKernelGGL(k_tb_refine, dim3((unsigned)nf), dim3(TB_REFINE_BLOCK), 0, c->stream, p, k, b.match, b.minl, b.qinl, b.res);
        HIPCHK(c, hipGetLastError());
        mo_stage_mark(c, "tb_refine");
    }
    // ---- copy-out: the result blocks, and one download per requested per-keypoint array
    HIPCHK(c, hipMemcpyAsync(b.h_res, b.res, (size_t)nf * sizeof(TbRes), hipMemcpyDeviceToHost, c->stream));
    if ((rc = b.head.download(c))) return rc;
    if (any_rows) {
        if (out->point) HIPCHK(c, hipMemcpyAsync(b.h_qpt, b.qpt, rows * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->dist) HIPCHK(c, hipMemcpyAsync(b.h_qdist, b.qdist, rows * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->inlier) HIPCHK(c, hipMemcpyAsync(b.h_qinl, b.qinl, rows, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = map_sync(c, clk))) return rc;
    out->n_local = b.head.host().n_local;
    for (int i = 0; i < nf; i++) {
        const TbRes& r = b.h_res[i];
        const size_t at = (size_t)i * stride, n = (size_t)b.h_fcnt[i];
        for (int j = 0; j < 12; j++) out->pose[(size_t)i * 12 + j] = r.pose[j];
        for (int k = 0; k < TB_MAX_PASS; k++) {
            for (int j = 0; j < 12; j++) out->pass_pose[((size_t)i * TB_MAX_PASS + k) * 12 + j] = r.pass_pose[k][j];
            out->pass_radius[i * TB_MAX_PASS + k] = r.pass_radius[k];
            out->pass_cand[i * TB_MAX_PASS + k] = r.pass_cand[k]; out->pass_matches[i * TB_MAX_PASS + k] = r.pass_matches[k];
            out->pass_inliers[i * TB_MAX_PASS + k] = r.pass_inliers[k];
        }
        out->n_pass_run[i] = r.n_run;
        out->ok[i] = r.n_done == prm->n_pass && r.pass_inliers[prm->n_pass - 1] >= prm->min_inliers;
        out->n_ok += out->ok[i];
        if (out->point) std::memcpy(out->point + at, b.h_qpt + at, n * 4);
        if (out->dist) std::memcpy(out->dist + at, b.h_qdist + at, n * 4);
        if (out->inlier) std::memcpy(out->inlier + at, b.h_qinl + at, n);
    }
    return MO_OK;
}
