// map_confirm.hip -- loop confirmation on the device map (mo_map_loop_confirm in include/vslam_amd.h): the second half of ORB-SLAM2's
// ComputeSim3.  With the similarities mo_map_loop_sim3 found, both keyframes are searched again, guided by the similarity
// (SearchBySim3), the similarity is refitted on seeds + guided matches (OptimizeSim3), and the loop keyframe's neighbourhood is projected
// into the asking keyframe (SearchByProjection).  The product: per keypoint row of the asking keyframe the loop-side map point it
// corresponds to.  Read-only on the map.
// Chain (one synchronisation, the copy-out; the kernels behind the winner read `win` first and return when it is -1):
//   uploads, point_of of every keyframe (map_launch_point_of), k_trk_rep over the keyframes of the call (trk_launch_rep_mask),
//   k_trk_grid for p and every candidate (trk_launch_grid)
//   k_cf_seed     one workgroup per candidate: the seed rows, the owner of every candidate row a seed names (atomicMin)
//   k_cf_guided   one lane per source row, grid.y = candidate x direction: the projected-window search of map_search.h
//   k_cf_pairs    one workgroup per candidate: seeds and guided matches packed in row order (block scans, as k_sim3_gather)
//   k_cf_refit    one wave per candidate: selection, (Gauss-Newton, selection) twice from the given model (sim3_refine_rounds of
//                 sim3_device.h, which k_sim3_refine runs from its own start model)
//   k_cf_win      one workgroup: the winner, its inlier pairs written to loop_point / source, the claim keys reset
//   k_cf_proj     one lane per map point: the loop's local map projected into p, the best row claimed by a 64-bit atomicMin
//   k_cf_claim    one lane per row of p: the claims become loop points
// Integer atomics only (minima, counts).  -ffp-contract=off (Makefile): tests/confirm_restatement.py rounds as this file does.
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"
#include "map_store.h"
#include "map_search.h"
#include "sim3.h"
#include "sim3_device.h"

#define CF_MAX_CAND 16
#define CF_BLOCK 256

struct CfRes {
    double model[CF_MAX_CAND][13];          // refined s, R [9], t [3] per candidate
    int32_t npairs[CF_MAX_CAND], nguided[CF_MAX_CAND], ninl[CF_MAX_CAND];
    int32_t n_local, win, n_loop_points, n_proj_cand, n_proj, n_total;
};

struct CfPrm {
    double K[9], P[12];                     // P = [K | 0]: trk_project on a point of the camera frame
    double model[CF_MAX_CAND][13];          // the given models
    double r_guided, r_proj, chi2, sf;
    int32_t n_cand, p, n_p, stride, r2, w, h, max_dist, min_inliers;   // stride = max(n_p, 1), r2 = max(rows of a candidate, 1)
    int32_t cand[CF_MAX_CAND];
    uint8_t part[CF_MAX_CAND];              // the candidate takes part (a finite model with scale > 0)
};

// the caller's lists on the device
struct CfIn {
    const int32_t* cur; const int32_t* mpt; const int32_t* mrow; const uint8_t* inl;
};

struct ConfirmBufs : MapFeature {
    DevBuf<int32_t> cur, mpt, mrow; DevBuf<uint8_t> inl;   // the caller's lists: [n_p], [candidate][n_p] x 3
    DevBuf<double> poses;                   // [n_kf][12]
    DevBuf<uint8_t> lmask, gmask;           // [n_kf] the keyframes of the call, [candidate][n_kf] the groups
    DevBuf<int32_t> slots;                  // [1 + candidate] keyframe slot of every grid: p, then the candidates
    DevBuf<uint8_t> rep; DevBuf<int32_t> oct;              // [point][32], [point] (k_trk_rep)
    DevBuf<int32_t> cell, sorted;           // [1 + candidate][TK_CELLS + 1], [1 + candidate][row]
    DevBuf<int32_t> tab;                    // point_of [position][row]
    DevBuf<int32_t> seedj;                  // [candidate][r2] the seed row of p that names this candidate row (INT_MAX: none)
    DevBuf<int32_t> fwd, bwd;               // [candidate][stride], [candidate][r2]
    DevBuf<Sim3Pair> pr; DevBuf<int32_t> prow, pb; DevBuf<uint8_t> pkind;   // [candidate][stride] pairs, their rows of p, b, 1 seed / 2 guided
    DevBuf<uint8_t> fl;                     // [candidate][stride] final inlier flag per row of p
    DevBuf<uint8_t> skip;                   // [point] 1: the b of a final inlier pair of the winner
    DevBuf<int32_t> lpt; DevBuf<uint8_t> src;              // [stride] loop_point, source
    DevBuf<unsigned long long> key;         // [stride] (dist << 32) | point of the claim on each row of p
    ResBlock<CfRes> res;
    // all of it is scratch: every call's chain writes what it reads
    template <class F> void each_scratch(F f) {
        f(cur); f(mpt); f(mrow); f(inl); f(poses); f(lmask); f(gmask); f(slots); f(rep); f(oct); f(cell); f(sorted); f(tab); f(seedj); f(fwd); f(bwd);
        f(pr); f(prow); f(pb); f(pkind); f(fl); f(skip); f(lpt); f(src); f(key); f(res);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// k_sim3_gather's rule for row i of p under candidate c, and the seed flag: what the row names
__device__ __forceinline__ bool cf_listed(const MapView& v, const CfPrm& prm, const CfIn& in, int c, int i, int n2, int* a, int* b, int* j) {
    const size_t e = (size_t)c * prm.stride + i;
    *a = in.cur[i]; *b = in.mpt[e]; *j = in.mrow[e];
    return prm.part[c] && *a >= 0 && *a < v.n_pts && *b >= 0 && *b < v.n_pts && *j >= 0 && *j < n2 && in.inl[e] != 0;
}
// row i of p is a seed of candidate c: listed, and the lowest row of p that names its candidate row
__device__ __forceinline__ bool cf_seed(const MapView& v, const CfPrm& prm, const CfIn& in, const int32_t* __restrict__ seedj, int c, int i, int n2,
                                        int* a, int* b, int* j) {
    return cf_listed(v, prm, in, c, i, n2, a, b, j) && seedj[(size_t)c * prm.r2 + *j] == i;
}

// one workgroup per candidate: its entry of the result block; every listed row enters itself as owner of the candidate row it names
__global__ __launch_bounds__(1024) void k_cf_seed(MapView v, CfPrm prm, CfIn in, int32_t* __restrict__ seedj, CfRes* __restrict__ res) {
    const int c = blockIdx.x;
    if (threadIdx.x == 0) {
        res->npairs[c] = 0; res->nguided[c] = 0; res->ninl[c] = 0;
        for (int j = 0; j < 13; j++) res->model[c][j] = __longlong_as_double(0x7ff8000000000000ll);
        if (c == 0) res->win = -1;
    }
    const int n2 = v.kcnt[v.pos_slot[prm.cand[c]]];
    for (int i = threadIdx.x; i < prm.n_p; i += 1024) {
        int a, b, j;
        if (cf_listed(v, prm, in, c, i, n2, &a, &b, &j)) atomicMin(seedj + (size_t)c * prm.r2 + j, i);
    }
}

// one lane per source row of (candidate, direction): 0: rows of p searched in the candidate (fwd), 1: rows of the candidate in p (bwd)
__global__ __launch_bounds__(CF_BLOCK) void k_cf_guided(MapView v, CfPrm prm, CfIn in, const mo_keypoint* __restrict__ kkps, const uint8_t* __restrict__ kdesc,
                                                         const double* __restrict__ poses, const uint8_t* __restrict__ rep, const int32_t* __restrict__ oct,
                                                         const int32_t* __restrict__ cell, const int32_t* __restrict__ sorted, const int32_t* __restrict__ tab,
                                                         const int32_t* __restrict__ seedj, int32_t* __restrict__ fwd, int32_t* __restrict__ bwd) {
    const int c = blockIdx.y >> 1, dir = blockIdx.y & 1, idx = blockIdx.x * CF_BLOCK + threadIdx.x;
    const int k = prm.cand[c], s1 = v.pos_slot[prm.p], s2 = v.pos_slot[k], n2 = v.kcnt[s2];
    if (idx >= (dir ? prm.r2 : prm.n_p)) return;
    int32_t* out = dir ? bwd + (size_t)c * prm.r2 + idx : fwd + (size_t)c * prm.stride + idx;
    int pt = -1, a, b, j;
    if (!prm.part[c]) {
    } else if (dir == 0) {
        if (!cf_seed(v, prm, in, seedj, c, idx, n2, &a, &b, &j) && in.cur[idx] >= 0 && in.cur[idx] < v.n_pts) pt = in.cur[idx];
    } else if (idx < n2 && seedj[(size_t)c * prm.r2 + idx] == INT_MAX) {
        const int o = tab[(size_t)k * v.row + idx];
        if (o != INT_MAX) pt = o;
    }
    const int ro = pt >= 0 ? oct[pt] : TK_NOT_LOCAL;
    int bd = INT_MAX, bq = INT_MAX;
    if (ro != TK_NOT_LOCAL) {
        Sim3 S, I;
        sim3_model_load(prm.model[c], S);
        sim3_inverse(S, I);
        double X[3], Y[3], uu, vv;
        sim3_camera(v, poses + (size_t)(dir ? k : prm.p) * 12, pt, X);
        sim3_apply(dir ? S : I, X, Y);
        if (trk_project(prm.P, Y[0], Y[1], Y[2], prm.w, prm.h, &uu, &vv)) {
            const int g = dir ? 0 : 1 + c, ts = dir ? s1 : s2;
            const uint8_t* __restrict__ fdesc = kdesc + (size_t)ts * v.row * 32;
            const uint8_t* d = rep + (size_t)pt * 32;
            trk_window(uu, vv, prm.r_guided * trk_scale(prm.sf, ro), ro, prm.w, prm.h, cell + (size_t)g * (TK_CELLS + 1), sorted + (size_t)g * v.row,
                       kkps + (size_t)ts * v.row, [&](int q, const mo_keypoint&, double, double) {
                           const bool taken = dir ? cf_seed(v, prm, in, seedj, c, q, n2, &a, &b, &j) : seedj[(size_t)c * prm.r2 + q] != INT_MAX;
                           if (!taken) trk_take(trk_ham(d, fdesc + (size_t)q * 32), q, bd, bq);
                       });
        }
    }
    *out = bd != INT_MAX && bd <= prm.max_dist ? bq : -1;
}

// the pairs of candidate blockIdx.x in row order of p: seeds and guided matches, packed as k_sim3_gather packs them
__global__ __launch_bounds__(1024) void k_cf_pairs(MapView v, CfPrm prm, CfIn in, const mo_keypoint* __restrict__ kkps, const double* __restrict__ poses,
                                                   const int32_t* __restrict__ tab, const int32_t* __restrict__ seedj, const int32_t* __restrict__ fwd,
                                                   const int32_t* __restrict__ bwd, Sim3Pair* __restrict__ pr, int32_t* __restrict__ prow,
                                                   int32_t* __restrict__ pb, uint8_t* __restrict__ pkind, CfRes* __restrict__ res) {
    __shared__ int lw[40];
    __shared__ int ng;
    const int c = blockIdx.x, k = prm.cand[c];
    if (!prm.part[c]) return;
    if (threadIdx.x == 0) ng = 0;
    const int s1 = v.pos_slot[prm.p], s2 = v.pos_slot[k], n2 = v.kcnt[s2];
    const size_t base = (size_t)c * prm.stride;
    int added = 0;
    for (int b0 = 0; b0 < prm.n_p; b0 += 1024) {
        const int i = b0 + threadIdx.x;
        int a = -1, b = -1, j = -1, kind = 0;
        if (i < prm.n_p) {
            if (cf_seed(v, prm, in, seedj, c, i, n2, &a, &b, &j)) kind = 1;
            else {
                a = in.cur[i]; j = fwd[base + i];
                if (j >= 0 && bwd[(size_t)c * prm.r2 + j] == i) {
                    b = tab[(size_t)k * v.row + j];   // (a point: the row was a source of the other direction)
                    if (a != b) kind = 2;
                }
            }
        }
        int tot;
        const int r = block_excl_scan(kind ? 1 : 0, lw, &tot);
        if (kind) {
            pr[base + added + r] = sim3_pair_pack(v, kkps, prm.sf, poses + (size_t)prm.p * 12, s1, i, a, poses + (size_t)k * 12, s2, j, b);
            prow[base + added + r] = i; pb[base + added + r] = b; pkind[base + added + r] = (uint8_t)kind;
            if (kind == 2) atomicAdd(&ng, 1);
        }
        added += tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) { res->npairs[c] = added; res->nguided[c] = ng; }
}

// one wave per candidate: the given model, refined by sim3_refine_rounds (sim3_device.h) over seeds and guided matches
__global__ __launch_bounds__(64) void k_cf_refit(CfPrm prm, const Sim3Pair* __restrict__ pairs, const int32_t* __restrict__ prow, uint8_t* __restrict__ inl,
                                                 CfRes* __restrict__ res) {
    const int c = blockIdx.x;
    if (!prm.part[c]) return;   // 0 pairs, 0 inliers, NaN model (k_cf_seed)
    const int m = res->npairs[c];
    const Sim3Pair* pr = pairs + (size_t)c * prm.stride;
    const int32_t* rows = prow + (size_t)c * prm.stride;
    uint8_t* fl = inl + (size_t)c * prm.stride;
    Sim3 S;
    sim3_model_load(prm.model[c], S);
    int n = 0;
    if (m >= 3) n = sim3_refine_rounds(prm, pr, rows, m, fl, S);   // (fewer pairs: no inlier, the model as given)
    if (threadIdx.x == 0) {
        res->ninl[c] = n;
        sim3_model_store(S, res->model[c]);
    }
}

// the winner: at least min_inliers and the most final inliers, ties to the earlier candidate; its inlier pairs become loop points
__global__ __launch_bounds__(1024) void k_cf_win(CfPrm prm, const int32_t* __restrict__ prow, const int32_t* __restrict__ pb, const uint8_t* __restrict__ pkind,
                                                 const uint8_t* __restrict__ fl, int32_t* __restrict__ lpt, uint8_t* __restrict__ src,
                                                 uint8_t* __restrict__ skip, unsigned long long* __restrict__ key, CfRes* __restrict__ res) {
    __shared__ int win;
    if (threadIdx.x == 0) {
        int w = -1;
        for (int c = 0; c < prm.n_cand; c++)
            if (prm.part[c] && res->ninl[c] >= prm.min_inliers && (w < 0 || res->ninl[c] > res->ninl[w])) w = c;
        res->win = w;
        win = w;
    }
    for (int i = threadIdx.x; i < prm.n_p; i += 1024) { lpt[i] = -1; src[i] = 0; key[i] = TK_NONE; }
    __syncthreads();
    if (win < 0) return;
    const size_t base = (size_t)win * prm.stride;
    const int m = res->npairs[win];
    for (int e = threadIdx.x; e < m; e += 1024) {
        const int i = prow[base + e];
        if (!fl[base + i]) continue;
        lpt[i] = pb[base + e]; src[i] = pkind[base + e]; skip[pb[base + e]] = 1;
    }
}

// one lane per map point: the loop points of the winner's group that are not matched yet and not seen by p, projected into p
__global__ __launch_bounds__(CF_BLOCK) void k_cf_proj(MapView v, CfPrm prm, const mo_keypoint* __restrict__ kkps, const uint8_t* __restrict__ kdesc,
                                                       const double* __restrict__ poses, const uint8_t* __restrict__ gmask, const uint8_t* __restrict__ rep,
                                                       const int32_t* __restrict__ oct, const int32_t* __restrict__ cell, const int32_t* __restrict__ sorted,
                                                       const uint8_t* __restrict__ skip, const int32_t* __restrict__ lpt, unsigned long long* __restrict__ key,
                                                       CfRes* __restrict__ res) {
    const int win = res->win;
    if (win < 0) return;
    const int x = blockIdx.x * CF_BLOCK + threadIdx.x;
    bool loop = false, at_p = false, cand = false;
    if (x < v.n_pts) {
        const uint8_t* g = gmask + (size_t)win * v.n_kf;
        map_each_obs(v, x, [&](int, int pos, int, int) { loop |= g[pos] != 0; at_p |= pos == prm.p; return false; });
    }
    const int ro = loop ? oct[x] : TK_NOT_LOCAL;
    double uu = 0.0, vv = 0.0;
    if (ro != TK_NOT_LOCAL && !at_p && !skip[x]) {
        Sim3 S;
        sim3_model_load(res->model[win], S);
        double X[3], Y[3];
        sim3_camera(v, poses + (size_t)prm.cand[win] * 12, x, X);
        sim3_apply(S, X, Y);
        cand = trk_project(prm.P, Y[0], Y[1], Y[2], prm.w, prm.h, &uu, &vv);
    }
    int bd = INT_MAX, bq = INT_MAX;
    if (cand) {
        const int s1 = v.pos_slot[prm.p];
        const uint8_t* __restrict__ fdesc = kdesc + (size_t)s1 * v.row * 32;
        const uint8_t* d = rep + (size_t)x * 32;
        trk_window(uu, vv, prm.r_proj * trk_scale(prm.sf, ro), ro, prm.w, prm.h, cell, sorted, kkps + (size_t)s1 * v.row,
                   [&](int q, const mo_keypoint&, double, double) {
                       if (lpt[q] < 0) trk_take(trk_ham(d, fdesc + (size_t)q * 32), q, bd, bq);
                   });
    }
    if (bd != INT_MAX && bd <= prm.max_dist) atomicMin(key + bq, ((unsigned long long)(unsigned)bd << 32) | (unsigned)x);
    wave_count_add(loop, &res->n_loop_points);
    wave_count_add(cand, &res->n_proj_cand);
}

// one lane per row of p: a claimed row takes the point of the lowest (distance, point)
__global__ __launch_bounds__(CF_BLOCK) void k_cf_claim(int n_p, const unsigned long long* __restrict__ key, int32_t* __restrict__ lpt, uint8_t* __restrict__ src,
                                                        CfRes* __restrict__ res) {
    if (res->win < 0) return;
    const int i = blockIdx.x * CF_BLOCK + threadIdx.x;
    bool got = false, any = false;
    if (i < n_p) {
        const unsigned long long k = key[i];
        got = k != TK_NONE;
        if (got) { lpt[i] = (int)(k & 0xffffffffu); src[i] = 3; }
        any = lpt[i] >= 0;
    }
    wave_count_add(got, &res->n_proj);
    wave_count_add(any, &res->n_total);
}

static bool cf_pos(double x) { return x > 0.0 && std::isfinite(x); }

extern "C" int mo_map_loop_confirm(mo_map* m, const double K[9], const double* poses, const mo_map_confirm_params* prm, mo_map_confirm_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!K || !poses || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const int n_kf = (int)m->pos_slot.size(), nc = prm->n_cand;
    if (nc < 0 || nc > CF_MAX_CAND) return mo_fail(c, MO_ERR_ARG, "n_cand must be in 0 .. 16");
    if (!(prm->chi2 >= 0.0) || !std::isfinite(prm->chi2)) return mo_fail(c, MO_ERR_ARG, "chi2 must be finite and >= 0");
    if (!cf_pos(prm->scale_factor)) return mo_fail(c, MO_ERR_ARG, "scale_factor must be finite and > 0");
    if (prm->w < 1 || prm->h < 1) return mo_fail(c, MO_ERR_ARG, "w and h must be >= 1");
    if (!cf_pos(prm->radius_guided) || !cf_pos(prm->radius_proj)) return mo_fail(c, MO_ERR_ARG, "radii must be finite and > 0");
    if (prm->max_dist < 0 || prm->max_dist > 256) return mo_fail(c, MO_ERR_ARG, "max_dist must be in 0 .. 256");
    if (prm->min_inliers < 0 || prm->min_matches < 0) return mo_fail(c, MO_ERR_ARG, "min_inliers and min_matches must be >= 0");
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(K[i])) return mo_fail(c, MO_ERR_ARG, "K must be finite");
    for (size_t i = 0; i < (size_t)n_kf * 12; i++)
        if (!std::isfinite(poses[i])) return mo_fail(c, MO_ERR_ARG, "poses must be finite");
    out->win = -1; out->ok = 0; out->win_inliers = 0;
    out->n_loop_points = out->n_proj_cand = out->n_proj = out->n_total = 0;
    if (n_kf == 0) return MO_OK;   // a map without keyframes: nothing to confirm, not an error
    if (prm->kf_pos < 0 || prm->kf_pos >= n_kf) return mo_fail(c, MO_ERR_ARG, "kf_pos must be a keyframe position");
    if (nc == 0) return MO_OK;
    if (!prm->cand || !prm->cur_point || !prm->match_point || !prm->match_row) return mo_fail(c, MO_ERR_ARG, "NULL list with n_cand > 0");
    if (!prm->scale || !prm->R || !prm->t) return mo_fail(c, MO_ERR_ARG, "NULL model with n_cand > 0");
    for (int i = 0; i < nc; i++)
        if (prm->cand[i] < 0 || prm->cand[i] >= n_kf) return mo_fail(c, MO_ERR_ARG, "cand must hold keyframe positions");
    const int p = prm->kf_pos, n_p = m->h_kcnt[m->pos_slot[p]], stride = std::max(n_p, 1), row = m->row;
    int r2 = 1;
    for (int i = 0; i < nc; i++) r2 = std::max(r2, (int)m->h_kcnt[m->pos_slot[prm->cand[i]]]);
    CfPrm g;
    std::memset(&g, 0, sizeof(g));
    for (int i = 0; i < 9; i++) g.K[i] = K[i];
    for (int i = 0; i < 3; i++) { g.P[i * 4] = K[i * 3]; g.P[i * 4 + 1] = K[i * 3 + 1]; g.P[i * 4 + 2] = K[i * 3 + 2]; g.P[i * 4 + 3] = 0.0; }
    g.r_guided = prm->radius_guided; g.r_proj = prm->radius_proj; g.chi2 = prm->chi2; g.sf = prm->scale_factor;
    g.n_cand = nc; g.p = p; g.n_p = n_p; g.stride = stride; g.r2 = r2; g.w = prm->w; g.h = prm->h; g.max_dist = prm->max_dist; g.min_inliers = prm->min_inliers;
    const bool empty = n_p == 0 || m->n_pts == 0;   // no row or no point: nothing is searched, a model comes back as it was given
    for (int i = 0; i < CF_MAX_CAND; i++) {
        g.cand[i] = i < nc ? prm->cand[i] : -1;
        if (i >= nc) continue;
        g.model[i][0] = prm->scale[i];
        for (int j = 0; j < 9; j++) g.model[i][1 + j] = prm->R[i * 9 + j];
        for (int j = 0; j < 3; j++) g.model[i][10 + j] = prm->t[i * 3 + j];
        bool fin = prm->scale[i] > 0.0;
        for (int j = 0; j < 13; j++) fin = fin && std::isfinite(g.model[i][j]);
        g.part[i] = fin;
        const bool pass = fin && empty;
        if (out->scale) out->scale[i] = pass ? g.model[i][0] : NAN;
        if (out->R) for (int j = 0; j < 9; j++) out->R[i * 9 + j] = pass ? g.model[i][1 + j] : NAN;
        if (out->t) for (int j = 0; j < 3; j++) out->t[i * 3 + j] = pass ? g.model[i][10 + j] : NAN;
        if (out->n_pairs) out->n_pairs[i] = 0;
        if (out->n_guided) out->n_guided[i] = 0;
        if (out->n_inliers) out->n_inliers[i] = 0;
    }
    if (out->pair_inlier && n_p) std::memset(out->pair_inlier, 0, (size_t)nc * n_p);
    if (out->fwd) std::fill(out->fwd, out->fwd + (size_t)nc * n_p, -1);
    if (out->bwd) std::fill(out->bwd, out->bwd + (size_t)nc * r2, -1);
    if (out->loop_point) std::fill(out->loop_point, out->loop_point + n_p, -1);
    if (out->source && n_p) std::memset(out->source, 0, (size_t)n_p);
    if (empty) return MO_OK;
    MAP_ENTER(m);
    HostClock clk(c);
    int rc;
    if ((rc = map_int32_guard(m)) || (rc = upload_pos_slot(m))) return rc;
    if ((size_t)n_kf * row > (size_t)INT32_MAX) return mo_fail(c, MO_ERR_CAPACITY, "map larger than int32 indexing");
    mo_stage_begin(c);
    ConfirmBufs& b = map_feature<ConfirmBufs>(m);
    const size_t np = (size_t)m->n_pts, pair_n = (size_t)nc * stride, back_n = (size_t)nc * r2, ng = (size_t)nc + 1;
    if ((rc = mo_reserve(c, b.cur, (size_t)stride, b.mpt, pair_n, b.mrow, pair_n, b.inl, pair_n, b.poses, (size_t)n_kf * 12, b.lmask, (size_t)n_kf, b.gmask,
                         (size_t)nc * n_kf, b.slots, ng, b.rep, np * 32, b.oct, np, b.cell, ng * (TK_CELLS + 1), b.sorted, ng * row, b.tab, (size_t)n_kf * row,
                         b.seedj, back_n, b.fwd, pair_n, b.bwd, back_n, b.pr, pair_n, b.prow, pair_n, b.pb, pair_n, b.pkind, pair_n, b.fl, pair_n, b.skip, np,
                         b.lpt, (size_t)stride, b.src, (size_t)stride, b.key, (size_t)stride, b.res)))
        return rc;
    // the keyframes of the call (p, the candidates, their groups), the groups, the grid slots
    std::vector<uint8_t> lmask((size_t)n_kf, 0), gmask((size_t)nc * n_kf, 0);
    std::vector<int32_t> slots(ng);
    lmask[p] = 1; slots[0] = m->pos_slot[p];
    for (int i = 0; i < nc; i++) {
        uint8_t* gm = gmask.data() + (size_t)i * n_kf;
        if (prm->group) for (int k = 0; k < n_kf; k++) gm[k] = prm->group[(size_t)i * n_kf + k] != 0;
        else gm[prm->cand[i]] = 1;
        lmask[prm->cand[i]] = 1;
        for (int k = 0; k < n_kf; k++) lmask[k] |= gm[k];
        slots[1 + i] = m->pos_slot[prm->cand[i]];
    }
    HIPCHK(c, hipMemsetAsync(b.res, 0, sizeof(CfRes), c->stream));
    HIPCHK(c, hipMemcpyAsync(b.cur, prm->cur_point, (size_t)n_p * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.mpt, prm->match_point, pair_n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.mrow, prm->match_row, pair_n * 4, hipMemcpyHostToDevice, c->stream));
    if (prm->inlier) HIPCHK(c, hipMemcpyAsync(b.inl, prm->inlier, pair_n, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(b.inl, 1, pair_n, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.poses, poses, (size_t)n_kf * 96, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.lmask, lmask.data(), lmask.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.gmask, gmask.data(), gmask.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.slots, slots.data(), ng * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)b.seedj.p, INT_MAX, back_n, c->stream));
    HIPCHK(c, hipMemsetAsync(b.fl, 0, pair_n, c->stream));
    HIPCHK(c, hipMemsetAsync(b.skip, 0, np, c->stream));
    if ((rc = map_launch_point_of(m, 0, n_kf, b.tab)) || (rc = trk_launch_rep_mask(m, b.lmask, b.rep, b.oct, &b.res.p->n_local)) ||
        (rc = trk_launch_grid(m, b.slots, 0, (int)ng, prm->w, prm->h, b.cell, b.sorted)))
        return rc;
    mo_stage_mark(c, "confirm_prep");
    const MapView v = map_view(m);
    const CfIn in{b.cur, b.mpt, b.mrow, b.inl};
    hipLaunchKernelGGL(k_cf_seed, dim3(nc), dim3(1024), 0, c->stream, v, g, in, b.seedj, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "confirm_seed");
    hipLaunchKernelGGL(k_cf_guided, dim3((unsigned)((std::max(n_p, r2) + CF_BLOCK - 1) / CF_BLOCK), (unsigned)(2 * nc)), dim3(CF_BLOCK), 0, c->stream, v, g, in,
                       (const mo_keypoint*)m->kkps, m->kdesc, b.poses, b.rep, b.oct, b.cell, b.sorted, b.tab, b.seedj, b.fwd, b.bwd);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "confirm_guided");
    hipLaunchKernelGGL(k_cf_pairs, dim3(nc), dim3(1024), 0, c->stream, v, g, in, (const mo_keypoint*)m->kkps, b.poses, b.tab, b.seedj, b.fwd, b.bwd, b.pr, b.prow,
                       b.pb, b.pkind, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "confirm_pairs");
    hipLaunchKernelGGL(k_cf_refit, dim3(nc), dim3(64), 0, c->stream, g, b.pr, b.prow, b.fl, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "confirm_refit");
    hipLaunchKernelGGL(k_cf_win, dim3(1), dim3(1024), 0, c->stream, g, b.prow, b.pb, b.pkind, b.fl, b.lpt, b.src, b.skip, b.key, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "confirm_win");
    hipLaunchKernelGGL(k_cf_proj, dim3((unsigned)((np + CF_BLOCK - 1) / CF_BLOCK)), dim3(CF_BLOCK), 0, c->stream, v, g, (const mo_keypoint*)m->kkps, m->kdesc,
                       b.poses, b.gmask, b.rep, b.oct, b.cell, b.sorted, b.skip, b.lpt, b.key, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "confirm_proj");
    hipLaunchKernelGGL(k_cf_claim, dim3((unsigned)((n_p + CF_BLOCK - 1) / CF_BLOCK)), dim3(CF_BLOCK), 0, c->stream, n_p, b.key, b.lpt, b.src, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "confirm_claim");
    if ((rc = b.res.download(c))) return rc;
    if (out->pair_inlier) HIPCHK(c, hipMemcpyAsync(out->pair_inlier, b.fl, pair_n, hipMemcpyDeviceToHost, c->stream));
    if (out->fwd) HIPCHK(c, hipMemcpyAsync(out->fwd, b.fwd, pair_n * 4, hipMemcpyDeviceToHost, c->stream));
    if (out->bwd) HIPCHK(c, hipMemcpyAsync(out->bwd, b.bwd, back_n * 4, hipMemcpyDeviceToHost, c->stream));
    if (out->loop_point) HIPCHK(c, hipMemcpyAsync(out->loop_point, b.lpt, (size_t)n_p * 4, hipMemcpyDeviceToHost, c->stream));
    if (out->source) HIPCHK(c, hipMemcpyAsync(out->source, b.src, (size_t)n_p, hipMemcpyDeviceToHost, c->stream));
    if ((rc = map_sync(c, clk))) return rc;
    const CfRes& r = b.res.host();
    for (int i = 0; i < nc; i++) {
        if (out->scale) out->scale[i] = r.model[i][0];
        if (out->R) for (int j = 0; j < 9; j++) out->R[i * 9 + j] = r.model[i][1 + j];
        if (out->t) for (int j = 0; j < 3; j++) out->t[i * 3 + j] = r.model[i][10 + j];
        if (out->n_pairs) out->n_pairs[i] = r.npairs[i];
        if (out->n_guided) out->n_guided[i] = r.nguided[i];
        if (out->n_inliers) out->n_inliers[i] = r.ninl[i];
    }
    out->win = r.win;
    if (r.win >= 0) {
        out->win_inliers = r.ninl[r.win];
        out->n_loop_points = r.n_loop_points; out->n_proj_cand = r.n_proj_cand; out->n_proj = r.n_proj; out->n_total = r.n_total;
        out->ok = r.n_total >= prm->min_matches;
    }
    return MO_OK;
}
