// map_ba.hip -- local bundle adjustment on the device map (mo_map_bundle_adjust and mo_map_bundle_adjust_local in include/vslam_amd.h:
// ORB-SLAM2's Optimizer::LocalBundleAdjustment, monocular).  The problem, the passes over its points and the host code around the
// optional outputs are ba_problem.h's, shared with the global solver (map_gba.hip); here are the choice of the local points and of the
// free keyframes, the dense reduced camera system and its solve, and the accept rule of the two rounds.
//
// Chain of one bundle adjustment (one synchronisation, the copy-out; every decision - the gauge, accept / reject, the end of a round -
// is a flag in BaRes that the later kernels read first; [shared]: a kernel of ba_problem.h):
//   k_ba_mark      one thread per map point: its valid edges (map_obs), local-point flag, keyframes with edges
//   scans          local rank of every local point, first compact edge of every local point (the map's device-wide scan)
//   k_ba_setup     one block: free / fixed keyframes and the gauge rule, free index of every position and its inverse fpos
//   k_ba_edges     [shared] the compact edge arrays and the positions as f64
//   k_ba_cost      [shared] cost of every edge, the classification between the rounds; k_ba_reduce [shared] sums
//   per Levenberg-Marquardt step:
//     k_ba_lin     [shared] V (damped, inverted), g_p, the current cost per point
//     k_ba_pair    one workgroup per free-keyframe pair (i <= j): the 6x6 block S_ij (and b_i on the diagonal) summed over the local
//                  points in a fixed thread assignment and a fixed reduction tree; Jacobians are recomputed, not stored
//     k_ba_solve   one workgroup: the reduced system (<= 96) packed in LDS, left-looking Cholesky across the block, substitution, the
//                  trial poses
//     k_ba_back    [shared] back-substitution, trial position, trial cost
//     k_ba_accept  one workgroup: cost sums, accept / reject, lambda, the end-of-round flags; an accepted step becomes the state
//   k_ba_write     [shared] xyz (f32) of the local points, kP of the free keyframes, the optional outputs
// Round 1 runs without the Huber width over the edges round 0 left as inliers (e_inl): the INL instantiation of the shared kernels.
// -ffp-contract=off (Makefile): ba.h rounds on the device as in the host build of tests/native/ba_check.cpp.
//
// mo_map_bundle_adjust_local is the same chain over a set of candidate positions instead of a window (ba_run enqueues both):
//   candidates     the caller's mask, or k_covis and k_covis_select of map_covis.hip in this chain (the covis_* pieces, as
//                  mo_map_track_covisible runs them) and their mask read on the device; k_bal_cand drops position 0 and counts
//   k_ba_mark_set  k_ba_mark with "position in C" for "position >= lo_pos and != 0"
//   k_ba_setup_set k_ba_setup with the same substitution: positions outside C are fixed, the gauge takes the lowest ones of C
//   ... every kernel from k_ba_edges to k_ba_write as above ...
//   erase_outliers the entry erase of map_obs.hip behind k_ba_write, gated on the device by BaRes (run, n_inliers >= min_inliers): class 2
//                  leaves
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "ba_problem.h"

#define BA_MAX_PAIRS (BA_MAX_FREE * (BA_MAX_FREE + 1) / 2)
#define BA_TRI_N (BA_MAX_DIM * (BA_MAX_DIM + 1) / 2)

struct BaPrm {
    double K[9], sf, chi2;
    int n_kf, lo_pos;
};

struct BaRes {
    double cost[3], lambda, upd_c;
    int32_t n_points, n_edges, n_free, n_fixed, n_inliers;
    int32_t steps[2], accepted[2], done[2];
    int32_t run, step_ok;
};
// what the shared kernels ask (ba_problem.h)
__device__ __forceinline__ bool ba_live(const BaRes* res, int round) { return res->run && !res->done[round]; }
__device__ __forceinline__ bool ba_has_trial(const BaRes* res) { return res->step_ok; }
__device__ __forceinline__ bool ba_step_accepted(const BaRes* res) { return res->accepted[0] + res->accepted[1] > 0; }
__device__ __forceinline__ bool ba_xyz_always(const BaRes*) { return true; }   // (X is xyz as stored until a step is accepted)
__device__ __forceinline__ void ba_store_cost(BaRes* res, int idx, double cost, int n_inliers) {
    res->cost[idx] = cost; res->n_inliers = n_inliers;
    if (idx == 1) res->lambda = 1e-4;   // every round starts from the same damping
}

struct BaBufs : MapFeature {
    DevBuf<double> S;                                            // [96][96] reduced system, [96] right side, [96] solution
    ResBlock<BaRes> res;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) { f(S); f(res); }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

__global__ void k_ba_init(BaRes* __restrict__ res) {
    if (threadIdx.x) return;
    for (int i = 0; i < 3; i++) res->cost[i] = 0.0;
    res->lambda = 1e-4; res->upd_c = 0.0;
    res->n_points = 0; res->n_edges = 0; res->n_free = 0; res->n_fixed = 0; res->n_inliers = 0;
    for (int i = 0; i < 2; i++) { res->steps[i] = 0; res->accepted[i] = 0; res->done[i] = 0; }
    res->run = 0; res->step_ok = 0;
}

// local points: >= 2 edges, one of them at a position the window frees (>= lo_pos, never 0); every position with an edge to a local
// point is flagged (plain stores of 1: the racing writers agree)
__global__ __launch_bounds__(BA_BLOCK) void k_ba_mark(MapView v, int lo_pos, int32_t* __restrict__ loc, int32_t* __restrict__ ecnt, int32_t* __restrict__ kf_edge) {
    const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (i >= v.n_pts) return;
    int nv = 0;
    bool fr = false;
    map_each_obs(v, i, [&](int, int pos, int, int) { nv++; fr |= pos >= lo_pos && pos != 0; return false; });
    const bool local = nv >= 2 && fr;
    loc[i] = local;
    ecnt[i] = local ? nv : 0;
    if (local) map_each_obs(v, i, [&](int, int pos, int, int) { kf_edge[pos] = 1; return false; });
}

// free and fixed keyframes.  Outside the window a position with edges is fixed; inside, in position order, the lowest ones are fixed
// too until two keyframes are (the gauge), the rest are free.
__global__ __launch_bounds__(BA_BLOCK) void k_ba_setup(BaPrm prm, const int32_t* __restrict__ kf_edge, int32_t* __restrict__ kf_fidx, int32_t* __restrict__ fpos,
                                                       BaRes* __restrict__ res) {
    __shared__ int nfix;
    if (threadIdx.x == 0) nfix = 0;
    __syncthreads();
    const int lo = prm.lo_pos > 1 ? prm.lo_pos : 1;
    for (int pos = threadIdx.x; pos < prm.n_kf && pos < lo; pos += BA_BLOCK) {
        const int has = kf_edge[pos];
        kf_fidx[pos] = has ? BA_KF_FIXED : BA_KF_OUT;
        if (has) atomicAdd(&nfix, 1);
    }
    __syncthreads();
    if (threadIdx.x) return;
    int nfixed = nfix, nfree = 0;
    for (int pos = lo; pos < prm.n_kf; pos++) {
        if (!kf_edge[pos]) { kf_fidx[pos] = BA_KF_OUT; continue; }
        if (nfixed < 2) { kf_fidx[pos] = BA_KF_FIXED; nfixed++; }
        else if (nfree < BA_MAX_FREE) { kf_fidx[pos] = nfree; fpos[nfree++] = pos; }
        else kf_fidx[pos] = BA_KF_FIXED;   // (the host refuses windows wider than BA_MAX_FREE: not reached)
    }
    res->n_free = nfree; res->n_fixed = nfixed;
    res->run = nfree > 0 && res->n_points > 0;
}

// one workgroup per pair of free keyframes (i <= j): S_ij = [i == j] (H_ii + lambda diag H_ii) - sum over points W_i V^-1 W_j^T, and
// on the diagonal b_i = g_i - sum W_i V^-1 g_p.  Thread t takes the local points t, t + 256, ... in order; 48 sums per thread.
// (The edge arrays as __restrict__ pointers, not as a BaEdges: by value the struct moved this kernel's schedule, round 0 measured 1 % slower.)
__global__ __launch_bounds__(BA_BLOCK) void k_ba_pair(BaPrm prm, int round, const int32_t* __restrict__ eoff, const double* __restrict__ X,
                                                      const int32_t* __restrict__ e_kf, const float* __restrict__ e_xy, const double* __restrict__ e_info,
                                                      const uint8_t* __restrict__ e_inl, const int32_t* __restrict__ kf_fidx, const double* __restrict__ pose,
                                                      const double* __restrict__ Vi, const double* __restrict__ gp, const uint8_t* __restrict__ pfix,
                                                      double* __restrict__ S, const BaRes* __restrict__ res) {
    constexpr int NW = BA_BLOCK / 64;
    __shared__ double red[NW][48];
    if (!ba_live(res, round)) return;
    const int nf = res->n_free;
    int fi = 0, rem = blockIdx.x;
    while (fi < nf && rem >= nf - fi) { rem -= nf - fi; fi++; }
    if (fi >= nf) return;
    const int fj = fi + rem;
    const bool diag = fi == fj;
    const double huber2 = ba_huber2<true>(prm, round), lambda = res->lambda;
    const int n = res->n_points;
    double a[48];   // [0, 36) the block, [36, 42) b_i, [42, 48) diag H_ii
    for (int k = 0; k < 48; k++) a[k] = 0.0;
    for (int r = threadIdx.x; r < n; r += BA_BLOCK) {
        const int e0 = eoff[r], e1 = eoff[r + 1];
        bool hi = false, hj = false;
        for (int e = e0; e < e1; e++) {
            if (round && !e_inl[e]) continue;
            const int f = kf_fidx[e_kf[e]];
            hi |= f == fi; hj |= f == fj;
        }
        if (!hi || !hj) continue;
        const bool fixedp = pfix[r];
        if (fixedp && !diag) continue;
        const double Xp[3] = {X[(size_t)r * 3], X[(size_t)r * 3 + 1], X[(size_t)r * 3 + 2]};
        double inv[6], g[3];
        for (int k = 0; k < 6; k++) inv[k] = Vi[(size_t)r * 6 + k];
        for (int k = 0; k < 3; k++) g[k] = gp[(size_t)r * 3 + k];
        for (int ea = e0; ea < e1; ea++) {
            if ((round && !e_inl[ea]) || kf_fidx[e_kf[ea]] != fi) continue;
            double era[2], wa, e2a, Jca[12], Jpa[6];
            if (!ba_edge_lin(prm, huber2, pose + (size_t)e_kf[ea] * 12, Xp, e_xy[(size_t)ea * 2], e_xy[(size_t)ea * 2 + 1], e_info[ea], era, &wa, &e2a, Jca,
                             Jpa))
                continue;
            if (diag) {
                ba_camera_terms(Jca, wa, era, a, a + 36);
                for (int k = 0; k < 6; k++) a[42 + k] += wa * (Jca[k] * Jca[k] + Jca[6 + k] * Jca[6 + k]);
                if (!fixedp) ba_schur_rhs(Jca, Jpa, wa, inv, g, a + 36);
            }
            if (fixedp) continue;
            for (int eb = e0; eb < e1; eb++) {
                if ((round && !e_inl[eb]) || kf_fidx[e_kf[eb]] != fj) continue;
                double erb[2], wb, e2b, Jcb[12], Jpb[6];
                if (!ba_edge_lin(prm, huber2, pose + (size_t)e_kf[eb] * 12, Xp, e_xy[(size_t)eb * 2], e_xy[(size_t)eb * 2 + 1], e_info[eb], erb, &wb, &e2b,
                                 Jcb, Jpb))
                    continue;
                ba_schur_pair(Jca, Jpa, wa, Jcb, Jpb, wb, inv, a);
            }
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < 48; k++) {
        const double v = wave_sum(a[k]);
        if (lane == 0) red[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 42) {
        const int k = threadIdx.x;
        double s = red[0][k];
        for (int w = 1; w < NW; w++) s += red[w][k];
        if (k < 36) {
            const int rr = k / 6, cc = k % 6;
            if (diag && rr == cc) {
                double d = red[0][42 + rr];
                for (int w = 1; w < NW; w++) d += red[w][42 + rr];
                s += lambda * d;
            }
            S[(size_t)(6 * fi + rr) * BA_MAX_DIM + 6 * fj + cc] = s;
            if (!diag) S[(size_t)(6 * fj + cc) * BA_MAX_DIM + 6 * fi + rr] = s;
        } else if (diag) {
            S[(size_t)BA_MAX_DIM * BA_MAX_DIM + 6 * fi + (k - 36)] = s;
        }
    }
}

// one workgroup: S (lower triangle, packed in LDS) -> Cholesky factor, each entry one thread's dot product in k order as ba_chol_factor
// forms it; substitution; the trial poses.  A system that is not positive definite ends the round.
__global__ __launch_bounds__(BA_BLOCK) void k_ba_solve(int round, const double* __restrict__ S, double* __restrict__ dc, const int32_t* __restrict__ fpos,
                                                       const double* __restrict__ poseC, double* __restrict__ poseT, BaRes* __restrict__ res) {
    __shared__ double L[BA_TRI_N];
    __shared__ double bl[BA_MAX_DIM], x[BA_MAX_DIM];
    __shared__ int bad;
    if (!ba_live(res, round)) return;
    const int tid = threadIdx.x, nf = res->n_free, n = 6 * nf;
    for (int i = 0; i < n; i++)
        for (int j = tid; j <= i; j += BA_BLOCK) L[BA_TRI(i, j)] = S[(size_t)i * BA_MAX_DIM + j];
    for (int i = tid; i < n; i += BA_BLOCK) bl[i] = S[(size_t)BA_MAX_DIM * BA_MAX_DIM + i];
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int j = 0; j < n; j++) {
        if (tid == 0) {
            double s = L[BA_TRI(j, j)];
            for (int k = 0; k < j; k++) s -= L[BA_TRI(j, k)] * L[BA_TRI(j, k)];
            if (!(s > 0.0) || !isfinite(s)) bad = 1; else L[BA_TRI(j, j)] = sqrt(s);
        }
        __syncthreads();
        if (bad) break;
        const double d = L[BA_TRI(j, j)];
        for (int i = j + 1 + tid; i < n; i += BA_BLOCK) {
            double v = L[BA_TRI(i, j)];
            for (int k = 0; k < j; k++) v -= L[BA_TRI(i, k)] * L[BA_TRI(j, k)];
            L[BA_TRI(i, j)] = v / d;
        }
        __syncthreads();
    }
    if (bad) {
        if (tid == 0) { res->done[round] = 1; res->step_ok = 0; }
        return;
    }
    if (tid == 0) {
        ba_chol_subst(n, L, bl, x);
        double mx = 0.0;
        for (int i = 0; i < n; i++) mx = fmax(mx, fabs(x[i]));
        res->upd_c = mx;
        res->step_ok = 1;
    }
    __syncthreads();
    for (int i = tid; i < n; i += BA_BLOCK) dc[i] = x[i];
    if (tid < nf) {
        const int pos = fpos[tid];
        double d[6], T[12], T2[12];
        for (int k = 0; k < 6; k++) d[k] = x[6 * tid + k];
        for (int k = 0; k < 12; k++) T[k] = poseC[(size_t)pos * 12 + k];
        ba_pose_update(d, T, T2);
        for (int k = 0; k < 12; k++) poseT[(size_t)pos * 12 + k] = T2[k];
    }
}

// one workgroup: current and trial cost, the largest update; accept (the trial becomes the state, lambda / 10) or reject (lambda * 10);
// the round ends at an update below 1e-10 or lambda above 1e8
__global__ __launch_bounds__(BA_THREADS) void k_ba_accept(int round, const int32_t* __restrict__ fpos, const double* __restrict__ pc, const double* __restrict__ pt,
                                                          const double* __restrict__ pu, double* __restrict__ X, const double* __restrict__ Xt,
                                                          double* __restrict__ poseC, double* __restrict__ poseT, BaRes* __restrict__ res) {
    __shared__ double lds[BA_THREADS / 64];
    __shared__ int acc;
    if (!ba_live(res, round) || !ba_has_trial(res)) return;
    const int n = res->n_points, tid = threadIdx.x;
    double c0 = 0.0, c1 = 0.0, mu = 0.0;
    for (int r = tid; r < n; r += BA_THREADS) { c0 += pc[r]; c1 += pt[r]; mu = fmax(mu, pu[r]); }
    c0 = block_sum(c0, lds);
    c1 = block_sum(c1, lds);
    mu = block_max(mu, lds);
    if (tid == 0) {
        const bool ok = c1 < c0;
        acc = ok;
        const double upd = fmax(mu, res->upd_c);
        const double lam = ok ? res->lambda / 10.0 : res->lambda * 10.0;
        res->lambda = lam;
        res->steps[round]++;
        res->accepted[round] += ok;
        res->step_ok = 0;
        if (upd < 1e-10 || lam > 1e8) res->done[round] = 1;
    }
    __syncthreads();
    ba_commit(acc, n, res->n_free, fpos, X, Xt, poseC, poseT);
}

// ---- the set form: scratch, kernels ----------------------------------------------------------------------------------------------------
struct BalRes { int32_t n_candidates; };   // C before the gauge

struct BaLocalBufs : MapFeature {
    DevBuf<uint8_t> cand_in, cand;                    // [n_kf] the caller's mask as given; C (position 0 dropped)
    ResBlock<BalRes> res;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) { f(cand_in); f(cand); f(res); }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// C = the non-zero positions of `in` (the caller's mask, or covis_mask: the reference keyframe and its neighbours) except position 0
__global__ __launch_bounds__(BA_BLOCK) void k_bal_cand(const uint8_t* __restrict__ in, int n_kf, uint8_t* __restrict__ cand, BalRes* __restrict__ res) {
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    int n = 0;
    for (int p = threadIdx.x; p < n_kf; p += BA_BLOCK) {
        const bool in_c = p != 0 && in[p] != 0;
        cand[p] = in_c;
        n += in_c;
    }
    n = wave_sum_int(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&cnt, n);
    __syncthreads();
    if (threadIdx.x == 0) res->n_candidates = cnt;
}

// k_ba_mark over a set: local points have >= 2 edges, one of them at a position in C
__global__ __launch_bounds__(BA_BLOCK) void k_ba_mark_set(MapView v, const uint8_t* __restrict__ cand, int32_t* __restrict__ loc, int32_t* __restrict__ ecnt,
                                                          int32_t* __restrict__ kf_edge) {
    const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (i >= v.n_pts) return;
    int nv = 0;
    bool fr = false;
    map_each_obs(v, i, [&](int, int pos, int, int) { nv++; fr |= cand[pos] != 0; return false; });
    const bool local = nv >= 2 && fr;
    loc[i] = local;
    ecnt[i] = local ? nv : 0;
    if (local) map_each_obs(v, i, [&](int, int pos, int, int) { kf_edge[pos] = 1; return false; });
}

// k_ba_setup over a set: a position with edges outside C is fixed; those of C, in position order, are fixed too until two keyframes are
// (the gauge), the rest are free
__global__ __launch_bounds__(BA_BLOCK) void k_ba_setup_set(BaPrm prm, const uint8_t* __restrict__ cand, const int32_t* __restrict__ kf_edge,
                                                           int32_t* __restrict__ kf_fidx, int32_t* __restrict__ fpos, BaRes* __restrict__ res) {
    __shared__ int nfix;
    if (threadIdx.x == 0) nfix = 0;
    __syncthreads();
    for (int pos = threadIdx.x; pos < prm.n_kf; pos += BA_BLOCK) {
        if (cand[pos]) continue;
        const int has = kf_edge[pos];
        kf_fidx[pos] = has ? BA_KF_FIXED : BA_KF_OUT;
        if (has) atomicAdd(&nfix, 1);
    }
    __syncthreads();
    if (threadIdx.x) return;
    int nfixed = nfix, nfree = 0;
    for (int pos = 0; pos < prm.n_kf; pos++) {
        if (!cand[pos]) continue;
        if (!kf_edge[pos]) { kf_fidx[pos] = BA_KF_OUT; continue; }
        if (nfixed < 2) { kf_fidx[pos] = BA_KF_FIXED; nfixed++; }
        else if (nfree < BA_MAX_FREE) { kf_fidx[pos] = nfree; fpos[nfree++] = pos; }
        else kf_fidx[pos] = BA_KF_FIXED;   // (the host refuses sets of more than BA_MAX_FREE: not reached)
    }
    res->n_free = nfree; res->n_fixed = nfixed;
    res->run = nfree > 0 && res->n_points > 0;
}

// mo_map_bundle_adjust (lprm NULL: the window form and exactly the launches it had) and mo_map_bundle_adjust_local
static int ba_run(mo_map* m, const double K[9], const double* poses, const mo_map_ba_params* prm, mo_map_ba_out* out, const mo_map_ba_local_params* lprm,
                  mo_map_ba_local_out* lout) {
    mo_ctx* c = m->c;
    if (!K || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const int n_kf = (int)m->pos_slot.size();
    if (prm->window < 0) return mo_fail(c, MO_ERR_ARG, "window must be >= 0");
    for (int r = 0; r < 2; r++)
        if (prm->max_steps[r] < 0 || prm->max_steps[r] > 100) return mo_fail(c, MO_ERR_ARG, "max_steps must be in 0 .. 100");
    int rc;
    if ((rc = ba_check_common(c, K, poses, n_kf, prm->scale_factor, prm->chi2))) return rc;
    const int lo_pos = lprm ? 0 : map_window_lo(prm->window, n_kf);   // (the set form validates the window and does not use it)
    if (!lprm && n_kf - std::max(lo_pos, 1) > BA_MAX_FREE) return mo_fail(c, MO_ERR_ARG, "more than 16 free keyframes: give a window of at most 16");
    if (lprm) {
        if (lprm->n_best < 0 || lprm->n_best > BA_MAX_FREE - 1) return mo_fail(c, MO_ERR_ARG, "n_best must be in 0 .. 15");
        if (n_kf > 0 && (lprm->kf_pos < -1 || lprm->kf_pos >= n_kf)) return mo_fail(c, MO_ERR_ARG, "kf_pos must be -1 or a keyframe position");
        int n_set = 0;
        for (int p = 1; lprm->free_mask && p < n_kf; p++) n_set += lprm->free_mask[p] != 0;
        if (n_set > BA_MAX_FREE) return mo_fail(c, MO_ERR_ARG, "more than 16 free keyframes: give a set of at most 16 positions");
        if (lout->candidate) std::memset(lout->candidate, 0, (size_t)n_kf);
        lout->n_candidates = lout->n_erased = lout->n_under = 0;
        lout->n_obs = m->n_obs;
    }
    MAP_ENTER(m);
    HostClock clk(c);
    for (int i = 0; i < 3; i++) out->cost[i] = 0.0;
    out->lambda = 0.0;
    out->n_free = out->n_fixed = out->n_local = out->n_edges = out->n_inliers = out->ok = 0;
    for (int r = 0; r < 2; r++) { out->steps[r] = 0; out->accepted[r] = 0; }
    const size_t np = (size_t)m->n_pts, no = (size_t)m->n_obs, nk = (size_t)n_kf;
    ba_clear_outputs(out, poses, nk, np, no);
    if (n_kf == 0 || np == 0 || no == 0) return MO_OK;   // an empty map: nothing runs, not an error
    if ((rc = map_int32_guard(m))) return rc;
    BaProblem& pb = map_feature<BaProblem>(m);
    BaBufs& b = map_feature<BaBufs>(m);
    if ((rc = pb.reserve(c, np, no, nk))) return rc;
    if (out->points_out && (rc = mo_reserve(c, pb.pout, np * 3))) return rc;
    if ((rc = mo_reserve(c, b.res, b.S, BA_MAX_DIM * BA_MAX_DIM + 2 * BA_MAX_DIM))) return rc;
    BaLocalBufs* lb = lprm ? &map_feature<BaLocalBufs>(m) : nullptr;
    const bool erase = lprm && lprm->erase_outliers != 0;
    if (lb && (rc = mo_reserve(c, lb->cand_in, nk, lb->cand, nk, lb->res))) return rc;
    if ((rc = upload_pos_slot(m))) return rc;
    mo_stage_begin(c);
    if (lb) {   // C on the device: the caller's set, or the covisible neighbours of kf_pos selected in this chain
        HIPCHK(c, hipMemsetAsync(lb->res, 0, sizeof(BalRes), c->stream));
        const uint8_t* in = lb->cand_in;
        if (lprm->free_mask) {
            // (from the caller's pageable array, as mo_map_erase_points copies `remove` and mo_map_cull_points `protect`: the runtime stages
            // a pageable source before hipMemcpyAsync returns, so the array is the caller's again on every return path, the error ones too)
            HIPCHK(c, hipMemcpyAsync(lb->cand_in, lprm->free_mask, nk, hipMemcpyHostToDevice, c->stream));
        } else {
            mo_map_local_params q{};
            q.seed_points = nullptr; q.n_seed = 0; q.ref_pos = lprm->kf_pos; q.n_best = lprm->n_best; q.min_weight = lprm->min_weight;
            if ((rc = covis_enqueue(m)) || (rc = covis_select_enqueue(m, &q))) return rc;
            in = covis_mask(m);
        }
        hipLaunchKernelGGL(k_bal_cand, dim3(1), dim3(BA_BLOCK), 0, c->stream, in, n_kf, lb->cand, lb->res);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(pb.poseC, poses, nk * 96, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(pb.poseT, pb.poseC, nk * 96, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(pb.kf_edge, 0, nk * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(pb.einl, 0, no, c->stream));
    BaPrm p;
    for (int i = 0; i < 9; i++) p.K[i] = K[i];
    p.sf = prm->scale_factor; p.chi2 = prm->chi2; p.n_kf = n_kf; p.lo_pos = lo_pos;
    const MapView v = map_view(m);
    const BaEdges E = pb.edges();
    const unsigned pblocks = (unsigned)((np + BA_BLOCK - 1) / BA_BLOCK);
    const unsigned wblocks = (unsigned)((std::max(np, no) + BA_BLOCK - 1) / BA_BLOCK);
    double* dcv = b.S + BA_MAX_DIM * BA_MAX_DIM + BA_MAX_DIM;
    hipLaunchKernelGGL(k_ba_init, dim3(1), dim3(64), 0, c->stream, b.res);
    if (lb) hipLaunchKernelGGL(k_ba_mark_set, dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, v, lb->cand, pb.loc, pb.ecnt, pb.kf_edge);
    else hipLaunchKernelGGL(k_ba_mark, dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, v, lo_pos, pb.loc, pb.ecnt, pb.kf_edge);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, pb.loc, pb.lrank, (int)np, &b.res.p->n_points))) return rc;
    if ((rc = map_scan_excl(m, pb.ecnt, pb.ebase, (int)np, &b.res.p->n_edges))) return rc;
    if (lb) hipLaunchKernelGGL(k_ba_setup_set, dim3(1), dim3(BA_BLOCK), 0, c->stream, p, lb->cand, pb.kf_edge, pb.kf_fidx, pb.fpos, b.res);
    else hipLaunchKernelGGL(k_ba_setup, dim3(1), dim3(BA_BLOCK), 0, c->stream, p, pb.kf_edge, pb.kf_fidx, pb.fpos, b.res);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_edges<false, BaRes>), dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, v, m->kkps, p.sf, pb.loc, pb.lrank, pb.ebase, pb.eoff,
                       pb.X, pb.e_kf, pb.e_obs, nullptr, pb.e_xy, pb.e_info, pb.e_inl, nullptr, nullptr, nullptr, b.res);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_cost<true, BaPrm, BaRes>), dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, p, 0, E, pb.X, pb.poseC, pb.e_inl, pb.pc, pb.pn,
                       b.res);
    hipLaunchKernelGGL(k_ba_reduce<BaRes>, dim3(1), dim3(BA_THREADS), 0, c->stream, 0, pb.pc, pb.pn, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "ba_prep");
    for (int r = 0; r < 2; r++) {
        for (int s = 0; s < prm->max_steps[r]; s++) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_lin<true, BaPrm, BaRes>), dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, p, r, E, pb.X, pb.poseC, pb.Vi, pb.gp,
                               pb.pfix, pb.pc, b.res);
            hipLaunchKernelGGL(k_ba_pair, dim3(BA_MAX_PAIRS), dim3(BA_BLOCK), 0, c->stream, p, r, pb.eoff, pb.X, pb.e_kf, pb.e_xy, pb.e_info, pb.e_inl, pb.kf_fidx,
                               pb.poseC, pb.Vi, pb.gp, pb.pfix, b.S, b.res);
            hipLaunchKernelGGL(k_ba_solve, dim3(1), dim3(BA_BLOCK), 0, c->stream, r, b.S, dcv, pb.fpos, pb.poseC, pb.poseT, b.res);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_back<true, BaPrm, BaRes>), dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, p, r, E, pb.kf_fidx, pb.X, pb.poseC,
                               pb.poseT, pb.Vi, pb.gp, pb.pfix, dcv, pb.Xt, pb.pt, pb.pu, b.res);
            hipLaunchKernelGGL(k_ba_accept, dim3(1), dim3(BA_THREADS), 0, c->stream, r, pb.fpos, pb.pc, pb.pt, pb.pu, pb.X, pb.Xt, pb.poseC, pb.poseT, b.res);
        }
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_cost<true, BaPrm, BaRes>), dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, p, r + 1, E, pb.X, pb.poseC, pb.e_inl, pb.pc,
                           pb.pn, b.res);
        hipLaunchKernelGGL(k_ba_reduce<BaRes>, dim3(1), dim3(BA_THREADS), 0, c->stream, r + 1, pb.pc, pb.pn, b.res);
        HIPCHK(c, hipGetLastError());
        mo_stage_mark(c, r ? "ba_round1" : "ba_round0");
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_write<BaPrm, BaRes>), dim3(wblocks), dim3(BA_BLOCK), 0, c->stream, p, (int)np, (int)no, pb.loc, pb.lrank, pb.X, v.src.xyz,
                       out->points_out ? pb.pout.p : nullptr, pb.e_obs, pb.e_inl, pb.einl, m->d_pos_slot, pb.fpos, pb.poseC, m->kP, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "ba_write");
    if (erase && (rc = obs_erase_enqueue(m, pb.einl, &b.res.p->run, &b.res.p->n_inliers, prm->min_inliers))) return rc;
    std::vector<int32_t> fidx(out->kf_state ? nk : 0);
    if ((rc = b.res.download(c))) return rc;
    if (lb) {
        if ((rc = lb->res.download(c))) return rc;
        if (lout->candidate) HIPCHK(c, hipMemcpyAsync(lout->candidate, lb->cand, nk, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = ba_copy_outputs(c, pb, out, nk, np, no, fidx)) || (rc = map_sync(c, clk))) return rc;
    const BaRes& r = b.res.host();
    if (lb) {
        lout->n_candidates = lb->res.host().n_candidates;
        if (erase) { obs_erase_finish(m, &lout->n_erased, &lout->n_under); lout->n_obs = m->n_obs; }
    }
    if (!r.run) return MO_OK;   // no free keyframe with an edge, or no local point
    out->n_local = r.n_points;
    for (int i = 0; i < 3; i++) out->cost[i] = r.cost[i];
    out->lambda = r.lambda;
    out->n_free = r.n_free; out->n_fixed = r.n_fixed; out->n_edges = r.n_edges; out->n_inliers = r.n_inliers;
    for (int k = 0; k < 2; k++) { out->steps[k] = r.steps[k]; out->accepted[k] = r.accepted[k]; }
    ba_fill_kf_state(out, fidx, nk);
    out->ok = r.n_inliers >= prm->min_inliers;
    return MO_OK;
}

extern "C" int mo_map_bundle_adjust(mo_map* m, const double K[9], const double* poses, const mo_map_ba_params* prm, mo_map_ba_out* out) {
    if (!m) return MO_ERR_ARG;
    return ba_run(m, K, poses, prm, out, nullptr, nullptr);
}

extern "C" int mo_map_bundle_adjust_local(mo_map* m, const double K[9], const double* poses, const mo_map_ba_params* prm, const mo_map_ba_local_params* lprm,
                                          mo_map_ba_out* out, mo_map_ba_local_out* lout) {
    if (!m) return MO_ERR_ARG;
    if (!lprm || !lout) return mo_fail(m->c, MO_ERR_ARG, "NULL argument");
    return ba_run(m, K, poses, prm, out, lprm, lout);
}
