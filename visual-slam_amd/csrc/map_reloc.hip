// map_reloc.hip -- relocalization against the device map (mo_map_relocalize and mo_map_relocalize_pre in include/vslam_amd.h): a lost
// frame against every keyframe - or against the keyframes the place-recognition query of bow.hip selects on the device -, 2D-3D
// correspondences through the observations, P3P RANSAC per candidate keyframe (pnp.h).  Read-only on the map; the frame is staged in
// the spare keyframe slot (map_stage_frame).  The kernels and their launchers (map_reloc.h) index by (frame, ...): these two calls
// launch them for one frame, mo_map_relocalize_batch (map_reloc_batch.hip) for a group of frames.
// Chain: [preselection: bow_select_enqueue ->] point_of scatter -> knn-2 matching of the frame against every (selected) keyframe
// (match_launch_pairs, one pair per keyframe) -> scores
// |C_k| -> ranking -> C_k of the candidates (block scans, query order; the query rows and the packed records {X, Y, Z, x, y}) -> P3P
// hypotheses + scoring (a workgroup stages its candidate's records in LDS, every wave scores its hypotheses against them) -> best
// hypothesis + Gauss-Newton refinement (one wave per candidate) -> winner.  One synchronisation.
// -ffp-contract=off (Makefile, every map file): pnp.h rounds on the device as in a host build.  tests/test_gpu_reloc_replay.py holds
// the device to that: the chain from C_k on, restated on the host over the same pnp.h (tests/native/reloc_replay.cpp), gives the same
// keys, counts, flags and winner, and the same poses up to libm's sin / cos.
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"
#include "bow.h"
#include "map_store.h"
#include "map_reloc.h"
#include "pnp.h"

#define RL_HYP_WAVES 4    // waves per block of k_reloc_hyp
#define RL_HPW_MAX 16     // hypotheses per wave at most: lane L of a wave counts for (hypothesis L / 4, root L % 4)
#define RL_CHUNK 2048     // records a block of k_reloc_hyp holds in LDS at a time (40 KB: four blocks per CU)
#define RL_HYP_BLOCKS_PER_CU 8   // blocks a launch of k_reloc_hyp aims at per CU before a wave takes more than one hypothesis

struct RelocBufs : MapFeature {
    DevBuf<int32_t> tab;                      // point_of [position][row] (map_launch_point_of)
    DevBuf<int32_t> qf;                       // [n_kf] query frame of every pair: the spare slot
    MatchBufs match;                          // [pair][row] (a pair per keyframe, or per preselected keyframe)
    DevBuf<int32_t> score;                    // [n_kf] |C_k|
    DevBuf<int32_t> cq; DevBuf<float> rec; DevBuf<uint8_t> cinl;   // [candidate][row] C_k (query row; record {X, Y, Z, x, y}), final inliers
    DevBuf<int32_t> qpt; DevBuf<uint8_t> qinl;            // [row] per query keypoint
    ResBlock<RelocRes> res;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) { f(tab); f(qf); match.each_scratch(f); f(score); f(cq); f(rec); f(cinl); f(qpt); f(qinl); f(res); }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// |C_k|, one block per (keyframe position, frame)
__global__ __launch_bounds__(256) void k_reloc_score(RlFrames fr, MatchView mv) {
    __shared__ int lw[4];
    const int k = blockIdx.x, f = blockIdx.y, mr = fr.match_row(f, k);
    const int nq = fr.n(f);
    int n = 0;
    for (int q = threadIdx.x; q < nq; q += 256) n += map_match_point(mv, mr, k, q) >= 0;
    n = wave_sum_int(n);
    if ((threadIdx.x & 63) == 0) lw[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) fr.score[(size_t)f * fr.n_kf + k] = lw[0] + lw[1] + lw[2] + lw[3];
}

// candidates: scores >= RL_MIN_SCORE, highest first, ties to the lower position; one block per frame, one max reduction per rank
__global__ __launch_bounds__(256) void k_reloc_rank(RlFrames fr) {
    __shared__ unsigned long long red[256];
    const int tid = threadIdx.x, f = blockIdx.x, n_kf = fr.n_kf;
    RelocRes* __restrict__ res = fr.res + f;
    const int32_t* __restrict__ score = fr.score + (size_t)f * n_kf;
    if (tid < RL_MAX_CAND) {
        res->best[tid] = 0; res->ninl[tid] = 0; res->ncorr[tid] = 0; res->cand[tid] = -1; res->score[tid] = 0;
        for (int j = 0; j < 12; j++) res->pose[tid][j] = __longlong_as_double(0x7ff8000000000000ll);
    }
    __syncthreads();
    unsigned long long prev = ~0ull;
    int nc = 0;
    for (int r = 0; r < fr.nc; r++) {
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

// C_k of candidate blockIdx.x of frame blockIdx.y in query order (block scans, no atomics): the query row, and the record the pose
// kernels read - the point's position and the keypoint's pixel, the floats as they are stored
__global__ __launch_bounds__(1024) void k_reloc_gather(RlFrames fr, MatchView mv, const float* __restrict__ xyz) {
    __shared__ int lw[40];
    const int c = blockIdx.x, f = blockIdx.y;
    RelocRes* __restrict__ res = fr.res + f;
    const int k = res->cand[c];
    if (k < 0) return;
    const int nq = fr.n(f), mr = fr.match_row(f, k);
    const mo_keypoint* __restrict__ fk = fr.fk + (size_t)f * fr.stride;
    int32_t* __restrict__ cq = fr.cq + fr.ck(f, c);
    float* __restrict__ rec = fr.rec + fr.ck(f, c) * 5;
    int added = 0;
    for (int b = 0; b < nq; b += 1024) {
        const int q = b + threadIdx.x;
        const int p = q < nq ? map_match_point(mv, mr, k, q) : -1;
        int tot;
        const int r = block_excl_scan(p >= 0 ? 1 : 0, lw, &tot);
        if (p >= 0) {
            const size_t at = (size_t)added + r;
            const mo_keypoint kp = fk[q];
            cq[at] = q;
            rec[at * 5] = xyz[(size_t)p * 3]; rec[at * 5 + 1] = xyz[(size_t)p * 3 + 1]; rec[at * 5 + 2] = xyz[(size_t)p * 3 + 2];
            rec[at * 5 + 3] = kp.x; rec[at * 5 + 4] = kp.y;
        }
        added += tot;
    }
    if (threadIdx.x == 0) res->ncorr[c] = added;
}

// the P3P poses of hypothesis h over the m records of a candidate
__device__ __forceinline__ int reloc_solve(const RelocGeom& g, const float* __restrict__ rec, int m, uint64_t stream, int h, double (&R)[4][9],
                                           double (&t)[4][3]) {
    int idx[3];
    pnp_sample<3>(stream, h, m, idx);
    double X[3][3], b[3][3];
    for (int i = 0; i < 3; i++) {
        const float* __restrict__ e = rec + (size_t)idx[i] * 5;
        X[i][0] = e[0]; X[i][1] = e[1]; X[i][2] = e[2];
        const double x = e[3], y = e[4];
        for (int r = 0; r < 3; r++) b[i][r] = g.Kinv[r * 3] * x + g.Kinv[r * 3 + 1] * y + g.Kinv[r * 3 + 2];
    }
    return pnp_p3p(X, b, R, t);
}

// Hypotheses scored against the records of (candidate blockIdx.y, frame blockIdx.z).  A wave owns hpw consecutive hypotheses: lane j
// solves the j-th (with hpw = 1 every lane solves the same sample, no divergence) and keeps its up to 4 projections in registers.  The
// workgroup stages the candidate's records in LDS, RL_CHUNK at a time; per chunk every wave takes its hypotheses in turn: the
// projection broadcast from its lane, the 64 lanes over the records, each test pnp_reproj2 in f64 on the f32 inputs.  The inlier
// count of (hypothesis j, root r) is an integer sum kept by lane 4 j + r over the chunks; the best key per candidate by atomicMax.
__global__ __launch_bounds__(64 * RL_HYP_WAVES) void k_reloc_hyp(RelocGeom g, RlFrames fr, int n_hyp, int hpw, uint64_t seed) {
    __shared__ float s_rec[RL_CHUNK * 5];
    const int c = blockIdx.y, f = blockIdx.z;
    RelocRes* __restrict__ res = fr.res + f;
    const int k = res->cand[c];
    if (k < 0) return;   // uniform over the workgroup
    const int m = res->ncorr[c];
    const float* __restrict__ rec = fr.rec + fr.ck(f, c) * 5;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int h0 = (blockIdx.x * RL_HYP_WAVES + wave) * hpw;
    const int nh = min(hpw, n_hyp - h0);   // wave-uniform; <= 0: the wave only helps to stage
    double P[4][12];
    for (int r = 0; r < 4; r++)
        for (int i = 0; i < 12; i++) P[r][i] = 0.0;
    int nr = 0;
    if (nh > 0) {
        double R[4][9], t[4][3];
        nr = reloc_solve(g, rec, m, pnp_stream_seed(seed, k), h0 + min(lane, nh - 1), R, t);
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (r < nr) pnp_projection(g.K, R[r], t[r], P[r]);
    }
    int acc = 0;
    for (int base = 0; base < m; base += RL_CHUNK) {
        const int nrec = min(RL_CHUNK, m - base);
        __syncthreads();   // (the previous chunk has been read)
        for (int i = threadIdx.x; i < nrec * 5; i += 64 * RL_HYP_WAVES) s_rec[i] = rec[(size_t)base * 5 + i];
        __syncthreads();
        for (int j = 0; j < nh; j++) {
            const int nrj = __shfl(nr, j, 64);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                if (r >= nrj) break;   // wave-uniform
                double Pj[12];
#pragma unroll
                for (int i = 0; i < 12; i++) Pj[i] = __shfl(P[r][i], j, 64);
                int n = 0;
                for (int q = lane; q < nrec; q += 64) {
                    const float* e = s_rec + q * 5;
                    double e2;
                    n += pnp_reproj2(Pj, e[0], e[1], e[2], e[3], e[4], &e2) && e2 < g.thr2;
                }
                n = wave_sum_int(n);
                if (lane == j * 4 + r) acc += n;
            }
        }
    }
    const int hj = lane >> 2, r = lane & 3;
    const int nrh = __shfl(nr, hj, 64);
    unsigned long long key = 0;
    if (hj < nh && r < nrh && acc > 0) key = ((unsigned long long)(unsigned)acc << 32) | (0xffffffffu - (unsigned)((h0 + hj) * 4 + r));
    for (int d = 32; d; d >>= 1) key = max(key, (unsigned long long)__shfl_xor((long long)key, d, 64));
    if (lane == 0 && key) atomicMax(&res->best[c], key);
}

// inlier flags of the m records under (R, t) into fl, their number
__device__ __forceinline__ int reloc_select(const RelocGeom& g, const double* R, const double* t, const float* __restrict__ rec, int m,
                                            uint8_t* __restrict__ fl) {
    double P[12];
    pnp_projection(g.K, R, t, P);
    int n = 0;
    for (int j = threadIdx.x; j < m; j += 64) {
        const float* __restrict__ e = rec + (size_t)j * 5;
        double e2;
        const bool in = pnp_reproj2(P, e[0], e[1], e[2], e[3], e[4], &e2) && e2 < g.thr2;
        fl[j] = in;
        n += in;
    }
    return wave_sum_int(n);
}

// one wave per (candidate, frame): the best hypothesis' pose, (Gauss-Newton over its inliers, re-selection) twice
__global__ __launch_bounds__(64) void k_reloc_refine(RelocGeom g, RlFrames fr, uint64_t seed) {
    const int c = blockIdx.x, f = blockIdx.y;
    RelocRes* __restrict__ res = fr.res + f;
    const int k = res->cand[c];
    if (k < 0) return;
    const unsigned long long best = res->best[c];
    if (!best) return;   // no pose with an inlier: 0 inliers, NaN pose (k_reloc_rank)
    const int m = res->ncorr[c];
    const float* __restrict__ rec = fr.rec + fr.ck(f, c) * 5;
    uint8_t* fl = fr.cinl + fr.ck(f, c);
    const unsigned hr = 0xffffffffu - (unsigned)(best & 0xffffffffu);
    double Rs[4][9], ts[4][3];
    reloc_solve(g, rec, m, pnp_stream_seed(seed, k), (int)(hr >> 2), Rs, ts);
    double R[9], t[3];
    for (int i = 0; i < 9; i++) R[i] = Rs[hr & 3][i];
    for (int i = 0; i < 3; i++) t[i] = ts[hr & 3][i];
    int n = reloc_select(g, R, t, rec, m, fl);
    for (int round = 0; round < 2; round++) {
        for (int it = 0; it < 10; it++) {
            double H[21], gr[6];
            for (int i = 0; i < 21; i++) H[i] = 0.0;
            for (int i = 0; i < 6; i++) gr[i] = 0.0;
            for (int j = threadIdx.x; j < m; j += 64) {
                if (!fl[j]) continue;
                const float* __restrict__ e = rec + (size_t)j * 5;
                pnp_gn_accumulate(g.K, R, t, e[0], e[1], e[2], e[3], e[4], H, gr);
            }
            for (int i = 0; i < 21; i++) H[i] = wave_sum_all(H[i]);
            for (int i = 0; i < 6; i++) gr[i] = wave_sum_all(gr[i]);
            double step;
            if (!pnp_gn_update(H, gr, R, t, &step) || step < 1e-12) break;
        }
        n = reloc_select(g, R, t, rec, m, fl);
    }
    if (threadIdx.x == 0) {
        res->ninl[c] = n;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) res->pose[c][i * 4 + j] = R[i * 3 + j];
            res->pose[c][i * 4 + 3] = t[i];
        }
    }
}

// per frame: the winner (most final inliers, ties to the lower position) and its per-query-keypoint map point and inlier flag
__global__ __launch_bounds__(256) void k_reloc_finish(RlFrames fr, MatchView mv) {
    __shared__ int win;
    const int f = blockIdx.x;
    RelocRes* __restrict__ res = fr.res + f;
    if (threadIdx.x == 0) {
        int w = -1;
        for (int c = 0; c < res->n_cand; c++)
            if (w < 0 || res->ninl[c] > res->ninl[w] || (res->ninl[c] == res->ninl[w] && res->cand[c] < res->cand[w])) w = c;
        win = w;
        res->win = w;
    }
    __syncthreads();
    const int w = win, k = w >= 0 ? res->cand[w] : -1, mr = k >= 0 ? fr.match_row(f, k) : -1;
    const int nq = fr.n(f);
    int32_t* __restrict__ qpt = fr.qpt + (size_t)f * fr.stride;
    uint8_t* __restrict__ qinl = fr.qinl + (size_t)f * fr.stride;
    for (int q = threadIdx.x; q < nq; q += 256) {
        qpt[q] = map_match_point(mv, mr, k, q);
        qinl[q] = 0;
    }
    __syncthreads();
    if (w < 0 || !res->best[w]) return;
    const int m = res->ncorr[w];
    const int32_t* __restrict__ cq = fr.cq + fr.ck(f, w);
    const uint8_t* __restrict__ cinl = fr.cinl + fr.ck(f, w);
    for (int j = threadIdx.x; j < m; j += 256) qinl[cq[j]] = cinl[j];
}

int reloc_launch_candidates(mo_ctx* c, const RlFrames& fr, const MatchView& mv, const float* xyz) {
    hipLaunchKernelGGL(k_reloc_score, dim3((unsigned)fr.n_kf, (unsigned)fr.n_frames), dim3(256), 0, c->stream, fr, mv);
    hipLaunchKernelGGL(k_reloc_rank, dim3((unsigned)fr.n_frames), dim3(256), 0, c->stream, fr);
    hipLaunchKernelGGL(k_reloc_gather, dim3((unsigned)fr.nc, (unsigned)fr.n_frames), dim3(1024), 0, c->stream, fr, mv, xyz);
    HIPCHK(c, hipGetLastError());
    return MO_OK;
}

int reloc_launch_poses(mo_ctx* c, const RlFrames& fr, const MatchView& mv, const RelocGeom& g, int n_hyp, uint64_t seed, const char* mark_p3p,
                       const char* mark_refine) {
    // one hypothesis per wave while the launch stays below RL_HYP_BLOCKS_PER_CU blocks per CU (a single call: the widest launch, the
    // shortest chain); beyond that a wave takes several, so that a block's staged records serve up to 4 * RL_HPW_MAX hypotheses
    const long long blocks1 = (long long)((n_hyp + RL_HYP_WAVES - 1) / RL_HYP_WAVES) * fr.nc * fr.n_frames;
    const long long target = (long long)std::max(c->n_cu, 1) * RL_HYP_BLOCKS_PER_CU;
    const int hpw = (int)std::min<long long>(RL_HPW_MAX, std::max<long long>(1, (blocks1 + target - 1) / target));
    const int per_block = RL_HYP_WAVES * hpw;
    hipLaunchKernelGGL(k_reloc_hyp, dim3((unsigned)((n_hyp + per_block - 1) / per_block), (unsigned)fr.nc, (unsigned)fr.n_frames), dim3(64 * RL_HYP_WAVES), 0,
                       c->stream, g, fr, n_hyp, hpw, seed);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, mark_p3p);
    hipLaunchKernelGGL(k_reloc_refine, dim3((unsigned)fr.nc, (unsigned)fr.n_frames), dim3(64), 0, c->stream, g, fr, seed);
    hipLaunchKernelGGL(k_reloc_finish, dim3((unsigned)fr.n_frames), dim3(256), 0, c->stream, fr, mv);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, mark_refine);
    return MO_OK;
}

int reloc_check(mo_ctx* c, const double K[9], const mo_map_reloc_params* prm, RelocGeom* g) {
    if (prm->max_candidates < 1 || prm->max_candidates > RL_MAX_CAND) return mo_fail(c, MO_ERR_ARG, "max_candidates must be in 1 .. 64");
    if (prm->n_hyp < 1 || prm->n_hyp > (1 << 20)) return mo_fail(c, MO_ERR_ARG, "n_hyp must be in 1 .. 2^20");
    if (!(prm->thr_px >= 0.0)) return mo_fail(c, MO_ERR_ARG, "thr_px must be >= 0");
    const double* A = K;
    const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
    const double det = A[0] * c0 + A[1] * c1 + A[2] * c2;
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return mo_fail(c, MO_ERR_ARG, "K is singular");
    const double inv[9] = {c0, A[2] * A[7] - A[1] * A[8], A[1] * A[5] - A[2] * A[4],
                           c1, A[0] * A[8] - A[2] * A[6], A[2] * A[3] - A[0] * A[5],
                           c2, A[1] * A[6] - A[0] * A[7], A[0] * A[4] - A[1] * A[3]};
    for (int i = 0; i < 9; i++) { g->K[i] = K[i]; g->Kinv[i] = inv[i] / det; }
    g->thr2 = prm->thr_px * prm->thr_px;
    return MO_OK;
}

void reloc_defaults(const RelocDst& d, int n, int max_candidates) {
    for (int i = 0; i < 12; i++) d.pose[i] = NAN;
    *d.ok = 0; *d.kf_pos = -1; *d.n_cand = 0; *d.n_corr = 0; *d.n_inliers = 0;
    if (d.point) for (int i = 0; i < n; i++) d.point[i] = -1;
    if (d.inlier) std::memset(d.inlier, 0, (size_t)n);
    for (int i = 0; i < max_candidates; i++) {
        if (d.cand_pos) d.cand_pos[i] = -1;
        if (d.cand_score) d.cand_score[i] = 0;
        if (d.cand_inliers) d.cand_inliers[i] = 0;
    }
}

int reloc_result(const RelocDst& d, const RelocRes& r, const mo_map_reloc_params* prm) {
    *d.n_cand = r.n_cand;
    for (int i = 0; i < r.n_cand; i++) {
        if (d.cand_pos) d.cand_pos[i] = r.cand[i];
        if (d.cand_score) d.cand_score[i] = r.score[i];
        if (d.cand_inliers) d.cand_inliers[i] = r.ninl[i];
    }
    if (r.win >= 0) {
        *d.kf_pos = r.cand[r.win];
        *d.n_corr = r.ncorr[r.win];
        *d.n_inliers = r.ninl[r.win];
        for (int i = 0; i < 12; i++) d.pose[i] = r.pose[r.win][i];
        *d.ok = r.ninl[r.win] >= prm->min_inliers && r.best[r.win] != 0;
    }
    return *d.ok;
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
    RelocGeom g;
    if (int rv = reloc_check(c, K, prm, &g)) return rv;
    MAP_ENTER(m);
    HostClock clk(c);
    const int nc = prm->max_candidates;
    const RelocDst dst{out->point, out->inlier, out->cand_pos, out->cand_score, out->cand_inliers, out->pose, &out->ok, &out->kf_pos, &out->n_cand,
                       &out->n_corr, &out->n_inliers};
    out->from_token = 0;
    reloc_defaults(dst, 0, 0);
    int n, rc;
    mo_keypoint* qk; uint8_t* qdesc;
    if ((rc = map_stage_frame(m, f, false, &out->from_token, [&](int nq) { reloc_defaults(dst, nq, nc); }, &n, &qk, &qdesc)) || !qk)
        return rc;   // (nothing to match: not relocalized, not an error)
    const int n_kf = (int)m->pos_slot.size(), spare = m->kslots, row = m->row;
    // the keyframes that are matched: all of them, or - with fewer than all asked for - the n_pre the query selects on the device
    const bool pre = n_pre >= 0 && n_pre < n_kf;
    const int n_pairs = pre ? n_pre : n_kf;
    BowSel sel;
    if (pre && (rc = bow_select_enqueue(m, n, n_pre, &sel))) return rc;
    RelocBufs& b = map_feature<RelocBufs>(m);
    const size_t tab_n = (size_t)n_kf * row, pair_n = (size_t)n_pairs * row, cand_n = (size_t)nc * row;
    if ((rc = mo_reserve(c, b.tab, tab_n, b.qf, (size_t)n_kf, b.match, pair_n, b.score, (size_t)n_kf, b.cq, cand_n, b.rec, cand_n * 5, b.cinl, cand_n,
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
    const RlFrames fr{qk, m->kcnt + spare, row, 1, n_kf, nc, n_pairs, sel.mrow, b.score, b.cq, b.rec, b.cinl, b.qpt, b.qinl, b.res};
    if ((rc = reloc_launch_candidates(c, fr, mv, src.xyz))) return rc;
    mo_stage_mark(c, "reloc_candidates");
    if ((rc = reloc_launch_poses(c, fr, mv, g, prm->n_hyp, prm->seed, "reloc_p3p", "reloc_refine"))) return rc;
    if ((rc = b.res.download(c))) return rc;
    if (out->point) HIPCHK(c, hipMemcpyAsync(out->point, b.qpt, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (out->inlier) HIPCHK(c, hipMemcpyAsync(out->inlier, b.qinl, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if ((rc = map_sync(c, clk))) return rc;
    reloc_result(dst, b.res.host(), prm);
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
