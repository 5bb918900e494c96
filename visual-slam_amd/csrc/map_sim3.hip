// map_sim3.hip -- loop alignment on the device map (mo_map_loop_sim3 in include/vslam_amd.h): the asking keyframe against the
// candidates mo_map_loop_candidates returned, by the similarity X1 = s R X2 + t between their camera frames (sim3.h; ORB-SLAM2's
// ComputeSim3).  Read-only on the map.  The match lists arrive as host arrays: a loop detector's consistency bookkeeping sits between
// the two calls on the host, and a test can give constructed lists without a vocabulary.
// Chain: uploads -> pairs per candidate in row order, with both camera-frame points and both keypoints packed once (block scans, no
// atomics) -> 3-point hypotheses + two-sided scoring (one wave per (hypothesis, candidate), all candidates in one launch) -> best
// hypothesis + Gauss-Newton refinement on sim(3) (one wave per candidate) -> winner.  One synchronisation.
// -ffp-contract=off (Makefile, every map file): sim3.h rounds on the device as in a host build.  tests/test_gpu_sim3.py holds the
// device to that: the chain from the pairs on, restated on the host over the same sim3.h (tests/native/sim3_replay.cpp), gives the
// same keys, counts, flags and winner, and the same models up to libm's exp / sin / cos.
#include <cmath>
#include <cstring>

#include "common.h"
#include "map_store.h"
#include "sim3.h"
#include "sim3_device.h"

#define S3_MAX_CAND 16
#define S3_HYP_WAVES 4    // hypotheses per block of k_sim3_hyp (one per wave)

struct Sim3Res {
    double model[S3_MAX_CAND][13];          // s, R [9], t [3] per candidate
    unsigned long long best[S3_MAX_CAND];   // (inliers << 32) | ~h: the largest key is the best hypothesis, 0: no model
    int32_t cand[S3_MAX_CAND], ncorr[S3_MAX_CAND], ninl[S3_MAX_CAND];
    int32_t n_cand, win;
};

struct Sim3Prm {
    double K[9], chi2, sf;
    uint64_t seed;
    int32_t n_hyp, n_cand, p, n_p, stride;  // stride = max(n_p, 1): of every [candidate][row of p] array
    int32_t cand[S3_MAX_CAND];
};

struct Sim3Bufs : MapFeature {
    DevBuf<int32_t> cur, mpt, mrow;         // the caller's lists: [n_p], [candidate][n_p] x 2
    DevBuf<double> poses;                   // [n_kf][12]
    DevBuf<Sim3Pair> pr; DevBuf<int32_t> prow;   // [candidate][stride] the pairs and their rows of p
    DevBuf<uint8_t> inl;                    // [candidate][stride] final inlier flag per row of p
    ResBlock<Sim3Res> res;
    // all of it is scratch: every call's chain writes what it reads
    template <class F> void each_scratch(F f) { f(cur); f(mpt); f(mrow); f(poses); f(pr); f(prow); f(inl); f(res); }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

__device__ __forceinline__ void sim3_res_clear(Sim3Res* __restrict__ res, int c, int k) {
    res->best[c] = 0; res->ncorr[c] = 0; res->ninl[c] = 0; res->cand[c] = k;
    for (int j = 0; j < 13; j++) res->model[c][j] = __longlong_as_double(0x7ff8000000000000ll);
}

// the pairs of candidate blockIdx.x in row order (block scans, no atomics); its entry of the result block, and by block 0 the entries
// past n_cand
__global__ __launch_bounds__(1024) void k_sim3_gather(MapView v, const mo_keypoint* __restrict__ kkps, Sim3Prm prm, const int32_t* __restrict__ cur,
                                                      const int32_t* __restrict__ mpt, const int32_t* __restrict__ mrow,
                                                      const double* __restrict__ poses, Sim3Res* __restrict__ res, Sim3Pair* __restrict__ pr,
                                                      int32_t* __restrict__ prow) {
    __shared__ int lw[40];
    const int c = blockIdx.x, k = prm.cand[c];
    if (threadIdx.x == 0) {
        sim3_res_clear(res, c, k);
        if (c == 0) {
            for (int e = prm.n_cand; e < S3_MAX_CAND; e++) sim3_res_clear(res, e, -1);
            res->n_cand = prm.n_cand; res->win = -1;
        }
    }
    const int s1 = v.pos_slot[prm.p], s2 = v.pos_slot[k], n2 = v.kcnt[s2];
    const size_t base = (size_t)c * prm.stride;
    int added = 0;
    for (int b0 = 0; b0 < prm.n_p; b0 += 1024) {
        const int i = b0 + threadIdx.x;
        int a = -1, b = -1, j = -1;
        if (i < prm.n_p) { a = cur[i]; b = mpt[base + i]; j = mrow[base + i]; }
        const bool keep = a >= 0 && a < v.n_pts && b >= 0 && b < v.n_pts && j >= 0 && j < n2;
        int tot;
        const int r = block_excl_scan(keep ? 1 : 0, lw, &tot);
        if (keep) {
            pr[base + added + r] = sim3_pair_pack(v, kkps, prm.sf, poses + (size_t)prm.p * 12, s1, i, a, poses + (size_t)k * 12, s2, j, b);
            prow[base + added + r] = i;
        }
        added += tot;
    }
    if (threadIdx.x == 0) res->ncorr[c] = added;
}

// the model of hypothesis h over the m pairs pr (every lane of a wave solves the same sample)
__device__ __forceinline__ bool sim3_solve(const Sim3Pair* __restrict__ pr, int m, uint64_t stream, int h, Sim3& S) {
    int idx[3];
    pnp_sample<3>(stream, h, m, idx);
    double P1[3][3], P2[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const Sim3Pair* c = pr + idx[i];
#pragma unroll
        for (int d = 0; d < 3; d++) { P1[i][d] = c->X1[d]; P2[i][d] = c->X2[d]; }
    }
    return sim3_horn<3>(P1, P2, S);
}

// one wave per (hypothesis, candidate): the sample's model scored over the pairs by the 64 lanes; the best key per candidate by atomicMax
__global__ __launch_bounds__(64 * S3_HYP_WAVES) void k_sim3_hyp(Sim3Prm prm, const Sim3Pair* __restrict__ pairs, Sim3Res* __restrict__ res) {
    const int c = blockIdx.y;
    const int h = blockIdx.x * S3_HYP_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int m = res->ncorr[c];
    if (h >= prm.n_hyp || m < 3) return;   // wave-uniform
    const Sim3Pair* pr = pairs + (size_t)c * prm.stride;
    Sim3 S, I;
    if (!sim3_solve(pr, m, pnp_stream_seed(prm.seed, prm.cand[c]), h, S)) return;
    sim3_inverse(S, I);
    int n = 0;
    for (int j = lane; j < m; j += 64) {
        double e1, e2;
        n += sim3_inlier(prm.K, S, I, pr[j], prm.chi2, &e1, &e2);
    }
    n = wave_sum_int(n);
    const unsigned long long key = ((unsigned long long)(unsigned)n << 32) | (0xffffffffu - (unsigned)h);
    if (lane == 0) atomicMax(&res->best[c], key);
}

// one wave per candidate: the best hypothesis' model, refined by sim3_refine_rounds (sim3_device.h)
__global__ __launch_bounds__(64) void k_sim3_refine(Sim3Prm prm, const Sim3Pair* __restrict__ pairs, const int32_t* __restrict__ prow,
                                                    uint8_t* __restrict__ inl, Sim3Res* __restrict__ res) {
    const int c = blockIdx.x;
    const unsigned long long best = res->best[c];
    if (!best) return;   // fewer than 3 pairs or no sample with a model: 0 inliers, NaN model (k_sim3_gather)
    const int m = res->ncorr[c];
    const Sim3Pair* pr = pairs + (size_t)c * prm.stride;
    const int32_t* rows = prow + (size_t)c * prm.stride;
    uint8_t* fl = inl + (size_t)c * prm.stride;
    const int h = (int)(0xffffffffu - (unsigned)(best & 0xffffffffu));
    Sim3 S;
    if (!sim3_solve(pr, m, pnp_stream_seed(prm.seed, prm.cand[c]), h, S)) return;   // (it had a model in k_sim3_hyp)
    const int n = sim3_refine_rounds(prm, pr, rows, m, fl, S);
    if (threadIdx.x == 0) {
        res->ninl[c] = n;
        sim3_model_store(S, res->model[c]);
    }
}

// the winner: a model and the most final inliers, ties to the earlier candidate
__global__ __launch_bounds__(64) void k_sim3_finish(Sim3Res* __restrict__ res) {
    if (threadIdx.x != 0) return;
    int w = -1;
    for (int c = 0; c < res->n_cand; c++)
        if (res->best[c] && (w < 0 || res->ninl[c] > res->ninl[w])) w = c;
    res->win = w;
}

extern "C" int mo_map_loop_sim3(mo_map* m, const double K[9], const double* poses, const mo_map_sim3_params* prm, mo_map_sim3_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!K || !poses || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const int n_kf = (int)m->pos_slot.size(), nc = prm->n_cand;
    if (nc < 0 || nc > S3_MAX_CAND) return mo_fail(c, MO_ERR_ARG, "n_cand must be in 0 .. 16");
    if (prm->n_hyp < 1 || prm->n_hyp > (1 << 20)) return mo_fail(c, MO_ERR_ARG, "n_hyp must be in 1 .. 2^20");
    if (!(prm->chi2 >= 0.0) || !std::isfinite(prm->chi2)) return mo_fail(c, MO_ERR_ARG, "chi2 must be finite and >= 0");
    if (!(prm->scale_factor > 0.0) || !std::isfinite(prm->scale_factor)) return mo_fail(c, MO_ERR_ARG, "scale_factor must be finite and > 0");
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(K[i])) return mo_fail(c, MO_ERR_ARG, "K must be finite");
    for (size_t i = 0; i < (size_t)n_kf * 12; i++)
        if (!std::isfinite(poses[i])) return mo_fail(c, MO_ERR_ARG, "poses must be finite");
    out->win = -1; out->ok = 0; out->win_inliers = 0;
    if (n_kf == 0) return MO_OK;   // a map without keyframes: nothing to align, not an error
    if (prm->kf_pos < 0 || prm->kf_pos >= n_kf) return mo_fail(c, MO_ERR_ARG, "kf_pos must be a keyframe position");
    if (nc == 0) return MO_OK;
    if (!prm->cand || !prm->cur_point || !prm->match_point || !prm->match_row) return mo_fail(c, MO_ERR_ARG, "NULL list with n_cand > 0");
    for (int i = 0; i < nc; i++)
        if (prm->cand[i] < 0 || prm->cand[i] >= n_kf) return mo_fail(c, MO_ERR_ARG, "cand must hold keyframe positions");
    const int p = prm->kf_pos, n_p = m->h_kcnt[m->pos_slot[p]], stride = std::max(n_p, 1);
    for (int i = 0; i < nc; i++) {
        if (out->scale) out->scale[i] = NAN;
        if (out->R) for (int j = 0; j < 9; j++) out->R[i * 9 + j] = NAN;
        if (out->t) for (int j = 0; j < 3; j++) out->t[i * 3 + j] = NAN;
        if (out->n_corr) out->n_corr[i] = 0;
        if (out->n_inliers) out->n_inliers[i] = 0;
    }
    if (out->inlier && n_p) std::memset(out->inlier, 0, (size_t)nc * n_p);
    MAP_ENTER(m);
    HostClock clk(c);
    int rc;
    if ((rc = map_int32_guard(m)) || (rc = upload_pos_slot(m))) return rc;
    mo_stage_begin(c);
    Sim3Bufs& b = map_feature<Sim3Bufs>(m);
    const size_t pair_n = (size_t)nc * stride;
    if ((rc = mo_reserve(c, b.cur, (size_t)stride, b.mpt, pair_n, b.mrow, pair_n, b.poses, (size_t)n_kf * 12, b.pr, pair_n, b.prow, pair_n, b.inl, pair_n,
                         b.res)))
        return rc;
    b.res.host().n_cand = -1;  // until this call's copy-out lands: mo_dbg_map_sim3_last reports no alignment
    Sim3Prm g;
    for (int i = 0; i < 9; i++) g.K[i] = K[i];
    g.chi2 = prm->chi2; g.sf = prm->scale_factor; g.seed = prm->seed;
    g.n_hyp = prm->n_hyp; g.n_cand = nc; g.p = p; g.n_p = n_p; g.stride = stride;
    for (int i = 0; i < S3_MAX_CAND; i++) g.cand[i] = i < nc ? prm->cand[i] : -1;
    if (n_p) {
        HIPCHK(c, hipMemcpyAsync(b.cur, prm->cur_point, (size_t)n_p * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b.mpt, prm->match_point, pair_n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b.mrow, prm->match_row, pair_n * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(b.poses, poses, (size_t)n_kf * 96, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(b.inl, 0, pair_n, c->stream));
    hipLaunchKernelGGL(k_sim3_gather, dim3(nc), dim3(1024), 0, c->stream, map_view(m), (const mo_keypoint*)m->kkps, g, b.cur, b.mpt, b.mrow, b.poses, b.res,
                       b.pr, b.prow);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "sim3_gather");
    hipLaunchKernelGGL(k_sim3_hyp, dim3((unsigned)((prm->n_hyp + S3_HYP_WAVES - 1) / S3_HYP_WAVES), nc), dim3(64 * S3_HYP_WAVES), 0, c->stream, g, b.pr,
                       b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "sim3_hyp");
    hipLaunchKernelGGL(k_sim3_refine, dim3(nc), dim3(64), 0, c->stream, g, b.pr, b.prow, b.inl, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "sim3_refine");
    hipLaunchKernelGGL(k_sim3_finish, dim3(1), dim3(64), 0, c->stream, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "sim3_finish");
    if ((rc = b.res.download(c))) return rc;
    if (out->inlier && n_p) HIPCHK(c, hipMemcpyAsync(out->inlier, b.inl, pair_n, hipMemcpyDeviceToHost, c->stream));
    if ((rc = map_sync(c, clk))) return rc;
    const Sim3Res& r = b.res.host();
    for (int i = 0; i < nc; i++) {
        if (out->scale) out->scale[i] = r.model[i][0];
        if (out->R) for (int j = 0; j < 9; j++) out->R[i * 9 + j] = r.model[i][1 + j];
        if (out->t) for (int j = 0; j < 3; j++) out->t[i * 3 + j] = r.model[i][10 + j];
        if (out->n_corr) out->n_corr[i] = r.ncorr[i];
        if (out->n_inliers) out->n_inliers[i] = r.ninl[i];
    }
    out->win = r.win;
    if (r.win >= 0) {
        out->win_inliers = r.ninl[r.win];
        out->ok = r.ninl[r.win] >= prm->min_inliers;
    }
    return MO_OK;
}

// what the map's last alignment downloaded (the pinned Sim3Res): no launch, no copy, no synchronisation
extern "C" int mo_dbg_map_sim3_last(mo_map* m, int32_t* n_cand, int32_t* win, int32_t* cand, uint64_t* best, int32_t* ncorr, int32_t* ninl, double* model) {
    if (!m) return MO_ERR_ARG;
    if (!n_cand || !win || !cand || !best || !ncorr || !ninl || !model) return mo_fail(m->c, MO_ERR_ARG, "NULL argument");
    const Sim3Bufs* b = map_feature_if<Sim3Bufs>(m);
    if (!b || !b->res.pinned.p || b->res.host().n_cand < 0) return mo_fail(m->c, MO_ERR_ARG, "no loop alignment has run on this map");
    const Sim3Res& r = b->res.host();
    *n_cand = r.n_cand; *win = r.win;
    for (int i = 0; i < S3_MAX_CAND; i++) { cand[i] = r.cand[i]; best[i] = r.best[i]; ncorr[i] = r.ncorr[i]; ninl[i] = r.ninl[i]; }
    std::memcpy(model, r.model, sizeof(r.model));
    return MO_OK;
}
