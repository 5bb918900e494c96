// ba_problem.h -- what the local (map_ba.hip) and the global (map_gba.hip) bundle adjustment share on the device and on the host: the
// problem both build from the map (the marked points' edges as compact CSR arrays, the points as f64), the passes over its points, and
// the host code around the optional outputs.  The build has no relocatable device code: the kernels here are templates, instantiated
// in each of the two files.  ba.h holds the arithmetic; the reduced camera system and its solve are each solver's own.
//
// A solver brings a parameter block Prm (K, chi2 are read here) and a result block Res (run, n_points, n_edges, n_free are read here)
// and defines beside its result block what the shared kernels ask it:
//   ba_live(res, round)        this phase of the optimisation still runs (the local solver has two rounds, the global one phase)
//   ba_has_trial(res)          the step in flight got as far as trial poses
//   ba_step_accepted(res)      a step was accepted: the write forms kP from the poses (and, unless ba_xyz_always(res), only then xyz)
//   ba_store_cost(res, idx, cost, n_inliers)     where the sums of k_ba_reduce go
// INL (compile time) is "the solver masks edges by e_inl": the local one, in its round 1, with Huber width 0.  The global instantiation
// (INL false) has one phase, never masks and never loads e_inl.
//
// The shared kernels (the chains in map_ba.hip and map_gba.hip name them in order):
//   k_ba_edges   one thread per map point: its edges in CSR order into the compact edge arrays, its position as f64; with KF_LISTS also
//                e_pt and every edge appended to its position's list (integer atomic: the order of arrival)
//   k_ba_lin     one thread per problem point: V (damped, inverted), g_p, its current cost
//   k_ba_back    one thread per problem point: back-substitution, trial position, trial cost
//   k_ba_cost    one thread per problem point: every edge classified, its cost (mode 0: robust cost only; 1: robust cost and every edge
//                classified; 2: classified, plain cost of the inliers; the global solver has mode 1 alone)
//   k_ba_reduce  one workgroup: the costs and inlier counts summed in a fixed tree
//   k_ba_write   xyz (f32) of the problem points, kP of the free keyframes, the optional outputs
// No floating-point atomics anywhere: sums are per-thread in index order, then fixed wave / workgroup trees (block_sum of map_store.h).
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "map_store.h"
#include "ba.h"

#define BA_BLOCK 256
#define BA_THREADS 1024   // the one-workgroup kernels (sums over all points)
#define BA_KF_OUT (-2)    // kf_fidx: the position has no edge to a problem point
#define BA_KF_FIXED (-1)  // kf_fidx: fixed keyframe (>= 0: index among the free ones)

// the compact edge arrays as the kernels read them (by value): CSR offsets by point rank; per edge its keyframe position, its point's
// rank (global solver only), keypoint, information, inlier flag
struct BaEdges {
    const int32_t* eoff; const int32_t* e_kf; const int32_t* e_pt; const float* e_xy; const double* e_info; const uint8_t* e_inl;
};

// The scratch of a problem.  One per map, whichever solver runs: every chain writes what it reads, nothing passes from one call to the
// next (tests/test_gpu_ba_shared_scratch.py runs the solvers behind each other under poison).
struct BaProblem : MapFeature {
    // per map point
    DevBuf<int32_t> loc, ecnt, lrank, ebase;
    DevBuf<double> pout;                                         // [point][3] the optional f64 output
    // per problem point (by rank)
    DevBuf<int32_t> eoff, pn; DevBuf<uint8_t> pfix;
    DevBuf<double> X, Xt, Vi, gp, pc, pt, pu;
    // per edge (compact, CSR order of the problem points)
    DevBuf<int32_t> e_kf, e_obs, e_pt; DevBuf<float> e_xy; DevBuf<double> e_info; DevBuf<uint8_t> e_inl;
    DevBuf<uint8_t> einl;                                        // [observation] 0 / 1 / 2
    // per keyframe position
    DevBuf<int32_t> kf_edge, kf_fidx, fpos; DevBuf<double> poseC, poseT;   // fpos [free index] -> position
    // (pout is reserved by the caller that is asked for points_out)
    int reserve(mo_ctx* c, size_t np, size_t no, size_t nk) {
        return mo_reserve(c, loc, np, ecnt, np, lrank, np, ebase, np, eoff, np + 1, pn, np, pfix, np, X, np * 3, Xt, np * 3, Vi, np * 6, gp, np * 3,
                          pc, np, pt, np, pu, np, e_kf, no, e_obs, no, e_pt, no, e_xy, no * 2, e_info, no, e_inl, no, einl, no, kf_edge, nk, kf_fidx, nk,
                          fpos, nk, poseC, nk * 12, poseT, nk * 12);
    }
    BaEdges edges() const { return BaEdges{eoff, e_kf, e_pt, e_xy, e_info, e_inl}; }
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) {
        f(loc); f(ecnt); f(lrank); f(ebase); f(pout); f(eoff); f(pn); f(pfix); f(X); f(Xt); f(Vi); f(gp); f(pc); f(pt); f(pu);
        f(e_kf); f(e_obs); f(e_pt); f(e_xy); f(e_info); f(e_inl); f(einl); f(kf_edge); f(kf_fidx); f(fpos); f(poseC); f(poseT);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// residual, weight and Jacobians of an edge at the current state; false when the edge contributes nothing
template <class Prm> __device__ __forceinline__ bool ba_edge_lin(const Prm& prm, double huber2, const double* T, const double* Xp, float x, float y, double info,
                                                                 double* er, double* w, double* e2, double* Jc, double* Jp) {
    double zc;
    if (!ba_residual(prm.K, T, Xp, x, y, er, &zc)) return false;
    *e2 = info * (er[0] * er[0] + er[1] * er[1]);
    *w = info * ba_weight(*e2, huber2);
    return ba_jacobians(prm.K, T, Xp, Jc, Jp);
}

// the Huber width^2 of a phase: chi2, and none in the round that masks
template <bool INL, class Prm> __device__ __forceinline__ double ba_huber2(const Prm& prm, int round) { return !INL || round == 0 ? prm.chi2 : 0.0; }
// edge e is left out of this phase
template <bool INL> __device__ __forceinline__ bool ba_masked(const BaEdges& E, int round, int e) { return INL && round && !E.e_inl[e]; }

template <bool KF_LISTS, class Res>
__global__ __launch_bounds__(BA_BLOCK) void k_ba_edges(MapView v, const mo_keypoint* __restrict__ kkps, double sf, const int32_t* __restrict__ loc,
                                                       const int32_t* __restrict__ lrank, const int32_t* __restrict__ ebase, int32_t* __restrict__ eoff,
                                                       double* __restrict__ X, int32_t* __restrict__ e_kf, int32_t* __restrict__ e_obs,
                                                       int32_t* __restrict__ e_pt, float* __restrict__ e_xy, double* __restrict__ e_info,
                                                       uint8_t* __restrict__ e_inl, const int32_t* __restrict__ kbase, int32_t* __restrict__ kfill,
                                                       int32_t* __restrict__ karr, const Res* __restrict__ res) {
    if (KF_LISTS && !res->run) return;   // (the lists' bases are set up for a problem that runs)
    const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (i == 0) eoff[res->n_points] = res->n_edges;
    if (i >= v.n_pts || !loc[i]) return;
    const int r = lrank[i];
    int e = ebase[i];
    eoff[r] = e;
    for (int k = 0; k < 3; k++) X[(size_t)r * 3 + k] = v.src.xyz[(size_t)i * 3 + k];
    map_each_obs(v, i, [&](int o, int pos, int s, int kp) {
        const mo_keypoint q = kkps[(size_t)s * v.row + kp];
        e_kf[e] = pos; e_obs[e] = o;
        if (KF_LISTS) e_pt[e] = r;
        e_xy[(size_t)e * 2] = q.x; e_xy[(size_t)e * 2 + 1] = q.y; e_info[e] = ba_info(sf, q.octave);
        if (KF_LISTS) {
            const int at = atomicAdd(kfill + pos, 1);   // (the mark kernel counted this very walk: at < kbase[pos + 1] - kbase[pos])
            karr[kbase[pos] + at] = e;
        } else {
            e_inl[e] = 1;
        }
        e++;
        return false;
    });
}

template <bool INL, class Prm, class Res>
__global__ __launch_bounds__(BA_BLOCK) void k_ba_lin(Prm prm, int round, BaEdges E, const double* __restrict__ X, const double* __restrict__ pose,
                                                     double* __restrict__ Vi, double* __restrict__ gp, uint8_t* __restrict__ pfix, double* __restrict__ pc,
                                                     const Res* __restrict__ res) {
    if (!ba_live(res, round)) return;
    const int r = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (r >= res->n_points) return;
    const double huber2 = ba_huber2<INL>(prm, round), damp = 1.0 + res->lambda;
    const double Xp[3] = {X[(size_t)r * 3], X[(size_t)r * 3 + 1], X[(size_t)r * 3 + 2]};
    double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, cost = 0.0;
    for (int e = E.eoff[r]; e < E.eoff[r + 1]; e++) {
        if (ba_masked<INL>(E, round, e)) continue;
        double er[2], w, e2, Jc[12], Jp[6];
        if (!ba_edge_lin(prm, huber2, pose + (size_t)E.e_kf[e] * 12, Xp, E.e_xy[(size_t)e * 2], E.e_xy[(size_t)e * 2 + 1], E.e_info[e], er, &w, &e2, Jc, Jp)) continue;
        cost += ba_rho(e2, huber2);
        ba_point_terms(Jp, w, er, V, g);
    }
    V[0] *= damp; V[3] *= damp; V[5] *= damp;
    double inv[6] = {0, 0, 0, 0, 0, 0};
    const bool ok = ba_inv3(V, inv);
    for (int k = 0; k < 6; k++) Vi[(size_t)r * 6 + k] = inv[k];
    for (int k = 0; k < 3; k++) gp[(size_t)r * 3 + k] = g[k];
    pfix[r] = !ok;
    pc[r] = cost;
}

// dc [free index][6]: the solved pose updates
template <bool INL, class Prm, class Res>
__global__ __launch_bounds__(BA_BLOCK) void k_ba_back(Prm prm, int round, BaEdges E, const int32_t* __restrict__ kf_fidx, const double* __restrict__ X,
                                                      const double* __restrict__ poseC, const double* __restrict__ poseT, const double* __restrict__ Vi,
                                                      const double* __restrict__ gp, const uint8_t* __restrict__ pfix, const double* __restrict__ dc,
                                                      double* __restrict__ Xt, double* __restrict__ pt, double* __restrict__ pu,
                                                      const Res* __restrict__ res) {
    if (!ba_live(res, round) || !ba_has_trial(res)) return;
    const int r = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (r >= res->n_points) return;
    const double huber2 = ba_huber2<INL>(prm, round);
    const double Xp[3] = {X[(size_t)r * 3], X[(size_t)r * 3 + 1], X[(size_t)r * 3 + 2]};
    const int e0 = E.eoff[r], e1 = E.eoff[r + 1];
    double dp[3] = {0, 0, 0};
    if (!pfix[r]) {
        double g[3], inv[6];
        for (int k = 0; k < 3; k++) g[k] = gp[(size_t)r * 3 + k];
        for (int k = 0; k < 6; k++) inv[k] = Vi[(size_t)r * 6 + k];
        for (int e = e0; e < e1; e++) {
            if (ba_masked<INL>(E, round, e)) continue;
            const int f = kf_fidx[E.e_kf[e]];
            if (f < 0) continue;
            double er[2], w, e2, Jc[12], Jp[6];
            if (!ba_edge_lin(prm, huber2, poseC + (size_t)E.e_kf[e] * 12, Xp, E.e_xy[(size_t)e * 2], E.e_xy[(size_t)e * 2 + 1], E.e_info[e], er, &w, &e2, Jc, Jp)) continue;
            ba_back_edge(Jc, Jp, w, dc + (size_t)f * 6, g);
        }
        ba_sym3_mul(inv, g, dp);
    }
    const double Xn[3] = {Xp[0] + dp[0], Xp[1] + dp[1], Xp[2] + dp[2]};
    double cost = 0.0;
    for (int e = e0; e < e1; e++) {
        if (ba_masked<INL>(E, round, e)) continue;
        double er[2], zc;
        if (!ba_residual(prm.K, poseT + (size_t)E.e_kf[e] * 12, Xn, E.e_xy[(size_t)e * 2], E.e_xy[(size_t)e * 2 + 1], er, &zc)) continue;
        cost += ba_rho(E.e_info[e] * (er[0] * er[0] + er[1] * er[1]), huber2);
    }
    for (int k = 0; k < 3; k++) Xt[(size_t)r * 3 + k] = Xn[k];
    pt[r] = cost;
    pu[r] = fmax(fabs(dp[0]), fmax(fabs(dp[1]), fabs(dp[2])));
}

// e_inl is written here (E.e_inl is not read: a phase's mask is the classification in front of it)
template <bool INL, class Prm, class Res>
__global__ __launch_bounds__(BA_BLOCK) void k_ba_cost(Prm prm, int mode_arg, BaEdges E, const double* __restrict__ X, const double* __restrict__ pose,
                                                      uint8_t* __restrict__ e_inl, double* __restrict__ pc, int32_t* __restrict__ pn,
                                                      const Res* __restrict__ res) {
    if (!res->run) return;
    const int r = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (r >= res->n_points) return;
    const int mode = INL ? mode_arg : 1;
    const double Xp[3] = {X[(size_t)r * 3], X[(size_t)r * 3 + 1], X[(size_t)r * 3 + 2]};
    double cost = 0.0;
    int n = 0;
    for (int e = E.eoff[r]; e < E.eoff[r + 1]; e++) {
        double er[2], zc;
        const bool fin = ba_residual(prm.K, pose + (size_t)E.e_kf[e] * 12, Xp, E.e_xy[(size_t)e * 2], E.e_xy[(size_t)e * 2 + 1], er, &zc);
        const double e2 = fin ? E.e_info[e] * (er[0] * er[0] + er[1] * er[1]) : 0.0;
        const bool in = fin && zc > 0.0 && e2 <= prm.chi2;
        if (mode) e_inl[e] = in;
        n += in;
        if (fin && mode < 2) cost += ba_rho(e2, prm.chi2);
        if (in && mode == 2) cost += e2;
    }
    pc[r] = cost;
    pn[r] = n;
}

template <class Res>
__global__ __launch_bounds__(BA_THREADS) void k_ba_reduce(int idx, const double* __restrict__ pc, const int32_t* __restrict__ pn, Res* __restrict__ res) {
    __shared__ double lds[BA_THREADS / 64];
    __shared__ int cnt;
    if (!res->run) return;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const int n = res->n_points;
    double s = 0.0;
    int c = 0;
    for (int r = threadIdx.x; r < n; r += BA_THREADS) { s += pc[r]; c += pn[r]; }
    s = block_sum(s, lds);
    c = wave_sum_int(c);
    if ((threadIdx.x & 63) == 0) atomicAdd(&cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) ba_store_cost(res, idx, s, cnt);
}

// the end of an accept kernel (one workgroup of BA_THREADS): an accepted trial becomes the state, a rejected one is rolled back
__device__ __forceinline__ void ba_commit(bool accepted, int n, int nf, const int32_t* __restrict__ fpos, double* __restrict__ X, const double* __restrict__ Xt,
                                          double* __restrict__ poseC, double* __restrict__ poseT) {
    const int tid = threadIdx.x;
    if (accepted) {
        for (int k = tid; k < n * 3; k += BA_THREADS) X[k] = Xt[k];
        for (int k = tid; k < nf * 12; k += BA_THREADS) { const size_t o = (size_t)fpos[k / 12] * 12 + k % 12; poseC[o] = poseT[o]; }
    } else {
        for (int k = tid; k < nf * 12; k += BA_THREADS) { const size_t o = (size_t)fpos[k / 12] * 12 + k % 12; poseT[o] = poseC[o]; }
    }
}

// the results into the map: xyz of the problem points, kP = K [R | t] of the free keyframes; the optional outputs
template <class Prm, class Res>
__global__ __launch_bounds__(BA_BLOCK) void k_ba_write(Prm prm, int n_pts, int n_obs_edges, const int32_t* __restrict__ loc, const int32_t* __restrict__ lrank,
                                                       const double* __restrict__ X, float* __restrict__ xyz, double* __restrict__ pout,
                                                       const int32_t* __restrict__ e_obs, const uint8_t* __restrict__ e_inl, uint8_t* __restrict__ einl,
                                                       const int32_t* __restrict__ pos_slot, const int32_t* __restrict__ fpos, const double* __restrict__ poseC,
                                                       double* __restrict__ kP, const Res* __restrict__ res) {
    const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
    const bool run = res->run, wr = run && ba_step_accepted(res);
    if (i < n_pts) {
        const bool prob = run && loc[i];
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int k = 0; k < 3; k++) {
            const double v = prob ? X[(size_t)lrank[i] * 3 + k] : nan;
            if (pout) pout[(size_t)i * 3 + k] = v;
            if (prob && (wr || ba_xyz_always(res))) xyz[(size_t)i * 3 + k] = (float)v;
        }
    }
    if (!run) return;
    if (i < res->n_edges && i < n_obs_edges) einl[e_obs[i]] = e_inl[i] ? 1 : 2;
    if (i < res->n_free && wr) {   // (no accepted step: the poses are the given ones, kP stays)
        const int pos = fpos[i];
        double R[9], t[3], P[12];
        pose_split(poseC + (size_t)pos * 12, R, t);
        pnp_projection(prm.K, R, t, P);
        for (int k = 0; k < 12; k++) kP[(size_t)pos_slot[pos] * 12 + k] = P[k];
    }
}

// ---- host side: what mo_map_bundle_adjust(_local) and mo_map_global_ba check and do alike ----------------------------------------------
inline int ba_check_common(mo_ctx* c, const double K[9], const double* poses, int n_kf, double scale_factor, double chi2) {
    if (n_kf > 0 && !poses) return mo_fail(c, MO_ERR_ARG, "poses is NULL");
    if (!(scale_factor > 0.0) || !std::isfinite(scale_factor)) return mo_fail(c, MO_ERR_ARG, "scale_factor must be finite and > 0");
    if (!(chi2 >= 0.0) || !std::isfinite(chi2)) return mo_fail(c, MO_ERR_ARG, "chi2 must be finite and >= 0");
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(K[i])) return mo_fail(c, MO_ERR_ARG, "K must be finite");
    for (size_t i = 0; i < (size_t)n_kf * 12; i++)
        if (!std::isfinite(poses[i])) return mo_fail(c, MO_ERR_ARG, "poses must be finite");
    return MO_OK;
}

// the optional outputs (named alike in mo_map_ba_out and mo_map_gba_out) as a call that runs nothing leaves them
template <class Out> void ba_clear_outputs(Out* out, const double* poses, size_t nk, size_t np, size_t no) {
    if (out->poses_out && nk) std::memcpy(out->poses_out, poses, nk * 96);
    if (out->kf_state) for (size_t i = 0; i < nk; i++) out->kf_state[i] = 0;
    if (out->edge_inlier && no) std::memset(out->edge_inlier, 0, no);
    if (out->points_out) for (size_t i = 0; i < np * 3; i++) out->points_out[i] = NAN;
}

// ... their copies enqueued behind the write (fidx: room for kf_fidx on the host when kf_state is asked for), and behind the
// synchronisation kf_state from it: 2 free, 1 fixed, 0 outside
template <class Out> int ba_copy_outputs(mo_ctx* c, BaProblem& pb, Out* out, size_t nk, size_t np, size_t no, std::vector<int32_t>& fidx) {
    if (out->poses_out) HIPCHK(c, hipMemcpyAsync(out->poses_out, pb.poseC, nk * 96, hipMemcpyDeviceToHost, c->stream));
    if (out->edge_inlier) HIPCHK(c, hipMemcpyAsync(out->edge_inlier, pb.einl, no, hipMemcpyDeviceToHost, c->stream));
    if (out->points_out) HIPCHK(c, hipMemcpyAsync(out->points_out, pb.pout, np * 24, hipMemcpyDeviceToHost, c->stream));
    if (out->kf_state) HIPCHK(c, hipMemcpyAsync(fidx.data(), pb.kf_fidx, nk * 4, hipMemcpyDeviceToHost, c->stream));
    return MO_OK;
}
template <class Out> void ba_fill_kf_state(Out* out, const std::vector<int32_t>& fidx, size_t nk) {
    if (out->kf_state) for (size_t i = 0; i < nk; i++) out->kf_state[i] = fidx[i] >= 0 ? 2 : fidx[i] == BA_KF_FIXED ? 1 : 0;
}
