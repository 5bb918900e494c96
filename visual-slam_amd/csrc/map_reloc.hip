// map_reloc.hip -- relocalization against the device map (mo_map_relocalize and mo_map_relocalize_pre in include/vslam_amd.h): a lost
// frame against every keyframe - or against the keyframes the place-recognition query of bow.hip selects on the device -, 2D-3D
// correspondences through the observations, P3P RANSAC per candidate keyframe (pnp.h).  Read-only on the map; the frame is staged in
// the spare keyframe slot (map_stage_frame).
// Chain: [preselection: bow_select_enqueue ->] point_of scatter -> knn-2 matching of the frame against every (selected) keyframe
// (match_launch_pairs, one pair per keyframe) -> scores
// |C_k| -> ranking -> C_k of the candidates (block scans, query order) -> P3P hypotheses + scoring (one wave per hypothesis, all
// candidates in one launch) -> best hypothesis + Gauss-Newton refinement (one wave per candidate) -> winner.  One synchronisation.
// -ffp-contract=off (Makefile, every map file): pnp.h rounds on the device as in a host build.  tests/test_gpu_reloc_replay.py holds
// the device to that: the chain from C_k on, restated on the host over the same pnp.h (tests/native/reloc_replay.cpp), gives the same
// keys, counts, flags and winner, and the same poses up to libm's sin / cos.
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"
#include "bow.h"
#include "map_store.h"
#include "pnp.h"

#define RL_MAX_CAND 64
#define RL_MIN_SCORE 15   // ORB-SLAM2's Tracking::Relocalization: keyframes with fewer than 15 matches are discarded
#define RL_HYP_WAVES 4    // hypotheses per block of k_reloc_hyp (one per wave)

struct RelocRes {
    double pose[RL_MAX_CAND][12];         // refined [R | t] per candidate
    unsigned long long best[RL_MAX_CAND]; // (inliers << 32) | ~(h * 4 + root): the largest key is the best hypothesis
    int32_t cand[RL_MAX_CAND], score[RL_MAX_CAND], ncorr[RL_MAX_CAND], ninl[RL_MAX_CAND];
    int32_t n_cand, win;
};

struct RelocGeom {
    double K[9], Kinv[9], thr2;
};

struct RelocBufs : MapFeature {
    DevBuf<int32_t> tab;                      // point_of [position][row] (map_launch_point_of)
    DevBuf<int32_t> qf;                       // [n_kf] query frame of every pair: the spare slot
    MatchBufs match;                          // [pair][row] (a pair per keyframe, or per preselected keyframe)
    DevBuf<int32_t> score;                    // [n_kf] |C_k|
    DevBuf<int32_t> cq, cp; DevBuf<uint8_t> cinl;         // [candidate][row] C_k (query, point), final inliers
    DevBuf<int32_t> qpt; DevBuf<uint8_t> qinl;            // [row] per query keypoint
    ResBlock<RelocRes> res;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) { f(tab); f(qf); match.each_scratch(f); f(score); f(cq); f(cp); f(cinl); f(qpt); f(qinl); f(res); }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// the row of the matcher outputs that holds keyframe position k: k itself when every keyframe was matched (mrow NULL), else the pair the
// preselection gave it, -1: not matched
__device__ __forceinline__ int reloc_mrow(const int32_t* __restrict__ mrow, int k) { return mrow ? mrow[k] : k; }

// |C_k|, one block per keyframe position
__global__ __launch_bounds__(256) void k_reloc_score(const int32_t* __restrict__ kcnt, int spare, MatchView mv, const int32_t* __restrict__ mrow,
                                                     int32_t* __restrict__ score) {
    __shared__ int lw[4];
    const int k = blockIdx.x, mr = reloc_mrow(mrow, k);
    const int nq = min(kcnt[spare], mv.row);
    int n = 0;
    for (int q = threadIdx.x; q < nq; q += 256) n += map_match_point(mv, mr, k, q) >= 0;
    n = wave_sum_int(n);
    if ((threadIdx.x & 63) == 0) lw[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) score[k] = lw[0] + lw[1] + lw[2] + lw[3];
}

// candidates: scores >= RL_MIN_SCORE, highest first, ties to the lower position; one block, one max reduction per rank
__global__ __launch_bounds__(256) void k_reloc_rank(const int32_t* __restrict__ score, int n_kf, int max_cand, RelocRes* __restrict__ res) {
    __shared__ unsigned long long red[256];
    const int tid = threadIdx.x;
    if (tid < RL_MAX_CAND) {
        res->best[tid] = 0; res->ninl[tid] = 0; res->ncorr[tid] = 0; res->cand[tid] = -1; res->score[tid] = 0;
        for (int j = 0; j < 12; j++) res->pose[tid][j] = __longlong_as_double(0x7ff8000000000000ll);
    }
    __syncthreads();
    unsigned long long prev = ~0ull;
    int nc = 0;
    for (int r = 0; r < max_cand; r++) {
        unsigned long long b = 0;
        for (int k = tid; k < n_kf; k += 256) {
            const int s = score[k];
            const unsigned long long key = ((unsigned long long)(unsigned)s << 32) | (unsigned)(0x7fffffff - k);
            if (s >= RL_MIN_SCORE && key < prev && key > b) b = key;
        }
        red[tid] = b;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) red[tid] = max(red[tid], red[tid + w]);
            __syncthreads();
        }
        b = red[0];
        __syncthreads();
        if (!b) break;
        if (tid == 0) { res->cand[r] = 0x7fffffff - (int)(b & 0xffffffffu); res->score[r] = (int)(b >> 32); }
        nc = r + 1;
        prev = b;
    }
    if (tid == 0) { res->n_cand = nc; res->win = -1; }
}

// C_k of candidate blockIdx.x in query order (block scans, no atomics)
__global__ __launch_bounds__(1024) void k_reloc_gather(const int32_t* __restrict__ kcnt, int spare, MatchView mv, const int32_t* __restrict__ mrow,
                                                       RelocRes* __restrict__ res, int32_t* __restrict__ cq, int32_t* __restrict__ cp) {
    __shared__ int lw[40];
    const int c = blockIdx.x, k = res->cand[c];
    if (k < 0) return;
    const int row = mv.row, nq = min(kcnt[spare], row), mr = reloc_mrow(mrow, k);
    int added = 0;
    for (int b = 0; b < nq; b += 1024) {
        const int q = b + threadIdx.x;
        const int p = q < nq ? map_match_point(mv, mr, k, q) : -1;
        int tot;
        const int r = block_excl_scan(p >= 0 ? 1 : 0, lw, &tot);
        if (p >= 0) { cq[(size_t)c * row + added + r] = q; cp[(size_t)c * row + added + r] = p; }
        added += tot;
    }
    if (threadIdx.x == 0) res->ncorr[c] = added;
}

// the P3P poses of hypothesis h of candidate c (every lane of a wave solves the same sample)
__device__ __forceinline__ int reloc_solve(const RelocGeom& g, const float* __restrict__ xyz, const mo_keypoint* __restrict__ qkps,
                                           const int32_t* __restrict__ cq, const int32_t* __restrict__ cp, int m, uint64_t stream, int h,
                                           double (&R)[4][9], double (&t)[4][3]) {
    int idx[3];
    pnp_sample<3>(stream, h, m, idx);
    double X[3][3], b[3][3];
    for (int i = 0; i < 3; i++) {
        const int p = cp[idx[i]];
        X[i][0] = xyz[(size_t)p * 3]; X[i][1] = xyz[(size_t)p * 3 + 1]; X[i][2] = xyz[(size_t)p * 3 + 2];
        const mo_keypoint kp = qkps[cq[idx[i]]];
        const double x = kp.x, y = kp.y;
        for (int r = 0; r < 3; r++) b[i][r] = g.Kinv[r * 3] * x + g.Kinv[r * 3 + 1] * y + g.Kinv[r * 3 + 2];
    }
    return pnp_p3p(X, b, R, t);
}

// one wave per (hypothesis, candidate): up to 4 poses, each scored over C_k by the 64 lanes; the best key per candidate by atomicMax
__global__ __launch_bounds__(64 * RL_HYP_WAVES) void k_reloc_hyp(RelocGeom g, const float* __restrict__ xyz, const mo_keypoint* __restrict__ qkps,
                                                                 int row, int n_hyp, uint64_t seed, const int32_t* __restrict__ cq,
                                                                 const int32_t* __restrict__ cp, RelocRes* __restrict__ res) {
    const int c = blockIdx.y, k = res->cand[c];
    const int h = blockIdx.x * RL_HYP_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k < 0 || h >= n_hyp) return;   // wave-uniform
    const int m = res->ncorr[c];
    const int32_t* q = cq + (size_t)c * row;
    const int32_t* p = cp + (size_t)c * row;
    double R[4][9], t[4][3];
    const int nr = reloc_solve(g, xyz, qkps, q, p, m, pnp_stream_seed(seed, k), h, R, t);
    unsigned long long best = 0;
    for (int r = 0; r < nr; r++) {
        double P[12];
        pnp_projection(g.K, R[r], t[r], P);
        int n = 0;
        for (int j = lane; j < m; j += 64) {
            const int pj = p[j];
            const mo_keypoint kp = qkps[q[j]];
            double e2;
            n += pnp_reproj2(P, xyz[(size_t)pj * 3], xyz[(size_t)pj * 3 + 1], xyz[(size_t)pj * 3 + 2], kp.x, kp.y, &e2) && e2 < g.thr2;
        }
        n = wave_sum_int(n);
        const unsigned long long key = ((unsigned long long)(unsigned)n << 32) | (0xffffffffu - (unsigned)(h * 4 + r));
        if (n > 0 && key > best) best = key;
    }
    if (lane == 0 && best) atomicMax(&res->best[c], best);
}

// inlier flags of C_k under (R, t) into fl, their number
__device__ __forceinline__ int reloc_select(const RelocGeom& g, const double* R, const double* t, const float* __restrict__ xyz,
                                            const mo_keypoint* __restrict__ qkps, const int32_t* __restrict__ q, const int32_t* __restrict__ p,
                                            int m, uint8_t* __restrict__ fl) {
    double P[12];
    pnp_projection(g.K, R, t, P);
    int n = 0;
    for (int j = threadIdx.x; j < m; j += 64) {
        const int pj = p[j];
        const mo_keypoint kp = qkps[q[j]];
        double e2;
        const bool in = pnp_reproj2(P, xyz[(size_t)pj * 3], xyz[(size_t)pj * 3 + 1], xyz[(size_t)pj * 3 + 2], kp.x, kp.y, &e2) && e2 < g.thr2;
        fl[j] = in;
        n += in;
    }
    return wave_sum_int(n);
}

// one wave per candidate: the best hypothesis' pose, (Gauss-Newton over its inliers, re-selection) twice
__global__ __launch_bounds__(64) void k_reloc_refine(RelocGeom g, const float* __restrict__ xyz, const mo_keypoint* __restrict__ qkps, int row,
                                                     uint64_t seed, const int32_t* __restrict__ cq, const int32_t* __restrict__ cp,
                                                     uint8_t* __restrict__ cinl, RelocRes* __restrict__ res) {
    const int c = blockIdx.x, k = res->cand[c];
    if (k < 0) return;
    const unsigned long long best = res->best[c];
    if (!best) return;   // no pose with an inlier: 0 inliers, NaN pose (k_reloc_rank)
    const int m = res->ncorr[c];
    const int32_t* q = cq + (size_t)c * row;
    const int32_t* p = cp + (size_t)c * row;
    uint8_t* fl = cinl + (size_t)c * row;
    const unsigned hr = 0xffffffffu - (unsigned)(best & 0xffffffffu);
    double Rs[4][9], ts[4][3];
    reloc_solve(g, xyz, qkps, q, p, m, pnp_stream_seed(seed, k), (int)(hr >> 2), Rs, ts);
    double R[9], t[3];
    for (int i = 0; i < 9; i++) R[i] = Rs[hr & 3][i];
    for (int i = 0; i < 3; i++) t[i] = ts[hr & 3][i];
    int n = reloc_select(g, R, t, xyz, qkps, q, p, m, fl);
    for (int round = 0; round < 2; round++) {
        for (int it = 0; it < 10; it++) {
            double H[21], gr[6];
            for (int i = 0; i < 21; i++) H[i] = 0.0;
            for (int i = 0; i < 6; i++) gr[i] = 0.0;
            for (int j = threadIdx.x; j < m; j += 64) {
                if (!fl[j]) continue;
                const int pj = p[j];
                const mo_keypoint kp = qkps[q[j]];
                pnp_gn_accumulate(g.K, R, t, xyz[(size_t)pj * 3], xyz[(size_t)pj * 3 + 1], xyz[(size_t)pj * 3 + 2], kp.x, kp.y, H, gr);
            }
            for (int i = 0; i < 21; i++) H[i] = wave_sum_all(H[i]);
            for (int i = 0; i < 6; i++) gr[i] = wave_sum_all(gr[i]);
            double step;
            if (!pnp_gn_update(H, gr, R, t, &step) || step < 1e-12) break;
        }
        n = reloc_select(g, R, t, xyz, qkps, q, p, m, fl);
    }
    if (threadIdx.x == 0) {
        res->ninl[c] = n;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) res->pose[c][i * 4 + j] = R[i * 3 + j];
            res->pose[c][i * 4 + 3] = t[i];
        }
    }
}

// the winner (most final inliers, ties to the lower position) and its per-query-keypoint map point and inlier flag
__global__ __launch_bounds__(256) void k_reloc_finish(const int32_t* __restrict__ kcnt, int spare, MatchView mv, const int32_t* __restrict__ mrow,
                                                      const int32_t* __restrict__ cq, const uint8_t* __restrict__ cinl, RelocRes* __restrict__ res,
                                                      int32_t* __restrict__ qpt, uint8_t* __restrict__ qinl) {
    __shared__ int win;
    if (threadIdx.x == 0) {
        int w = -1;
        for (int c = 0; c < res->n_cand; c++)
            if (w < 0 || res->ninl[c] > res->ninl[w] || (res->ninl[c] == res->ninl[w] && res->cand[c] < res->cand[w])) w = c;
        win = w;
        res->win = w;
    }
    __syncthreads();
    const int w = win, k = w >= 0 ? res->cand[w] : -1, mr = k >= 0 ? reloc_mrow(mrow, k) : -1;
    const int row = mv.row, nq = min(kcnt[spare], row);
    for (int q = threadIdx.x; q < nq; q += 256) {
        qpt[q] = map_match_point(mv, mr, k, q);
        qinl[q] = 0;
    }
    __syncthreads();
    if (w < 0 || !res->best[w]) return;
    const int m = res->ncorr[w];
    for (int j = threadIdx.x; j < m; j += 256) qinl[cq[(size_t)w * row + j]] = cinl[(size_t)w * row + j];
}

// mo_map_relocalize (n_pre < 0) and mo_map_relocalize_pre: one body; they differ in which keyframes are matched
static int reloc_run(mo_map* m, const mo_frame_ref* f, const double K[9], const mo_map_reloc_params* prm, int n_pre, mo_map_reloc_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!f || !K || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (n_pre >= 0) {
        if (n_pre < 1) return mo_fail(c, MO_ERR_ARG, "n_pre must be >= 1");
        if (int rv = bow_require(m)) return rv;
    }
    if (prm->max_candidates < 1 || prm->max_candidates > RL_MAX_CAND) return mo_fail(c, MO_ERR_ARG, "max_candidates must be in 1 .. 64");
    if (prm->n_hyp < 1 || prm->n_hyp > (1 << 20)) return mo_fail(c, MO_ERR_ARG, "n_hyp must be in 1 .. 2^20");
    if (!(prm->thr_px >= 0.0)) return mo_fail(c, MO_ERR_ARG, "thr_px must be >= 0");
    RelocGeom g;
    {
        const double* A = K;
        const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
        const double det = A[0] * c0 + A[1] * c1 + A[2] * c2;
        if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return mo_fail(c, MO_ERR_ARG, "K is singular");
        const double inv[9] = {c0, A[2] * A[7] - A[1] * A[8], A[1] * A[5] - A[2] * A[4],
                               c1, A[0] * A[8] - A[2] * A[6], A[2] * A[3] - A[0] * A[5],
                               c2, A[1] * A[6] - A[0] * A[7], A[0] * A[4] - A[1] * A[3]};
        for (int i = 0; i < 9; i++) { g.K[i] = K[i]; g.Kinv[i] = inv[i] / det; }
        g.thr2 = prm->thr_px * prm->thr_px;
    }
    MAP_ENTER(m);
    HostClock clk(c);
    const int nc = prm->max_candidates;
    for (int i = 0; i < 12; i++) out->pose[i] = NAN;
    out->ok = 0; out->kf_pos = -1; out->n_cand = 0; out->n_corr = 0; out->n_inliers = 0; out->from_token = 0;
    int n, rc;
    mo_keypoint* qk; uint8_t* qdesc;
    auto defaults = [&](int nq) {
        if (out->point) for (int i = 0; i < nq; i++) out->point[i] = -1;
        if (out->inlier) std::memset(out->inlier, 0, (size_t)nq);
        for (int i = 0; i < nc; i++) {
            if (out->cand_pos) out->cand_pos[i] = -1;
            if (out->cand_score) out->cand_score[i] = 0;
            if (out->cand_inliers) out->cand_inliers[i] = 0;
        }
    };
    if ((rc = map_stage_frame(m, f, false, &out->from_token, defaults, &n, &qk, &qdesc)) || !qk) return rc;   // (nothing to match: not relocalized, not an error)
    const int n_kf = (int)m->pos_slot.size(), spare = m->kslots, row = m->row;
    // the keyframes that are matched: all of them, or - with fewer than all asked for - the n_pre the query selects on the device
    const bool pre = n_pre >= 0 && n_pre < n_kf;
    const int n_pairs = pre ? n_pre : n_kf;
    BowSel sel;
    if (pre && (rc = bow_select_enqueue(m, n, n_pre, &sel))) return rc;
    RelocBufs& b = map_feature<RelocBufs>(m);
    const size_t tab_n = (size_t)n_kf * row, pair_n = (size_t)n_pairs * row, cand_n = (size_t)nc * row;
    if ((rc = mo_reserve(c, b.tab, tab_n, b.qf, (size_t)n_kf, b.match, pair_n, b.score, (size_t)n_kf, b.cq, cand_n, b.cp, cand_n, b.cinl, cand_n,
                         b.qpt, (size_t)row, b.qinl, (size_t)row, b.res)))
        return rc;
    b.res.host().n_cand = -1;  // until this call's copy-out lands: mo_dbg_map_reloc_last reports no relocalization
    if (!pre) HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)b.qf, spare, (size_t)n_kf, c->stream));
    const MapPts src = m->P[m->cur].view();
    if ((rc = map_launch_point_of(m, 0, n_kf, b.tab))) return rc;
    mo_stage_mark(c, "reloc_point_of");
    if ((rc = match_launch_pairs(c, m->kdesc, m->kdesc, (size_t)row * 32, (size_t)row * 32, pre ? sel.cnt : (const int32_t*)m->kcnt,
                                 pre ? sel.qf : (const int32_t*)b.qf, pre ? sel.tf : (const int32_t*)m->d_pos_slot, 0, 0, n_pairs, row, prm->ratio,
                                 b.match.idx, b.match.dist, b.match.pass)))
        return rc;
    mo_stage_mark(c, "reloc_match");
    const MatchView mv{b.match.idx, b.match.dist, b.match.pass, b.tab, row};
    hipLaunchKernelGGL(k_reloc_score, dim3(n_kf), dim3(256), 0, c->stream, m->kcnt, spare, mv, sel.mrow, b.score);
    hipLaunchKernelGGL(k_reloc_rank, dim3(1), dim3(256), 0, c->stream, b.score, n_kf, nc, b.res);
    hipLaunchKernelGGL(k_reloc_gather, dim3(nc), dim3(1024), 0, c->stream, m->kcnt, spare, mv, sel.mrow, b.res, b.cq,
                       b.cp);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "reloc_candidates");
    hipLaunchKernelGGL(k_reloc_hyp, dim3((unsigned)((prm->n_hyp + RL_HYP_WAVES - 1) / RL_HYP_WAVES), nc), dim3(64 * RL_HYP_WAVES), 0, c->stream, g, src.xyz, qk,
                       row, prm->n_hyp, prm->seed, b.cq, b.cp, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "reloc_p3p");
    hipLaunchKernelGGL(k_reloc_refine, dim3(nc), dim3(64), 0, c->stream, g, src.xyz, qk, row, prm->seed, b.cq, b.cp, b.cinl, b.res);
    hipLaunchKernelGGL(k_reloc_finish, dim3(1), dim3(256), 0, c->stream, m->kcnt, spare, mv, sel.mrow, b.cq, b.cinl, b.res,
                       b.qpt, b.qinl);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "reloc_refine");
    if ((rc = b.res.download(c))) return rc;
    if (out->point) HIPCHK(c, hipMemcpyAsync(out->point, b.qpt, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (out->inlier) HIPCHK(c, hipMemcpyAsync(out->inlier, b.qinl, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if ((rc = map_sync(c, clk))) return rc;
    const RelocRes& r = b.res.host();
    out->n_cand = r.n_cand;
    for (int i = 0; i < r.n_cand; i++) {
        if (out->cand_pos) out->cand_pos[i] = r.cand[i];
        if (out->cand_score) out->cand_score[i] = r.score[i];
        if (out->cand_inliers) out->cand_inliers[i] = r.ninl[i];
    }
    if (r.win >= 0) {
        out->kf_pos = r.cand[r.win];
        out->n_corr = r.ncorr[r.win];
        out->n_inliers = r.ninl[r.win];
        for (int i = 0; i < 12; i++) out->pose[i] = r.pose[r.win][i];
        out->ok = r.ninl[r.win] >= prm->min_inliers && r.best[r.win] != 0;
    }
    return MO_OK;
}

extern "C" int mo_map_relocalize(mo_map* m, const mo_frame_ref* f, const double K[9], const mo_map_reloc_params* prm, mo_map_reloc_out* out) {
    return reloc_run(m, f, K, prm, -1, out);
}

extern "C" int mo_map_relocalize_pre(mo_map* m, const mo_frame_ref* f, const double K[9], const mo_map_reloc_params* prm, int32_t n_pre,
                                     mo_map_reloc_out* out) {
    return reloc_run(m, f, K, prm, n_pre < 0 ? 0 : n_pre, out);
}

// what the map's last relocalization downloaded (the pinned RelocRes): no launch, no copy, no synchronisation
extern "C" int mo_dbg_map_reloc_last(mo_map* m, int32_t* n_cand, int32_t* cand, uint64_t* best, int32_t* ncorr, int32_t* ninl, double* pose) {
    if (!m) return MO_ERR_ARG;
    if (!n_cand || !cand || !best || !ncorr || !ninl || !pose) return mo_fail(m->c, MO_ERR_ARG, "NULL argument");
    const RelocBufs* b = map_feature_if<RelocBufs>(m);
    if (!b || !b->res.pinned.p || b->res.host().n_cand < 0) return mo_fail(m->c, MO_ERR_ARG, "no relocalization has run on this map");
    const RelocRes& r = b->res.host();
    *n_cand = r.n_cand;
    for (int i = 0; i < RL_MAX_CAND; i++) { cand[i] = r.cand[i]; best[i] = r.best[i]; ncorr[i] = r.ncorr[i]; ninl[i] = r.ninl[i]; }
    std::memcpy(pose, r.pose, sizeof(r.pose));
    return MO_OK;
}
