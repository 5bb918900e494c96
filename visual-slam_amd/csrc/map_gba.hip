// map_gba.hip -- global bundle adjustment on the device map (mo_map_global_ba in include/vslam_amd.h: ORB-SLAM2's
// Optimizer::GlobalBundleAdjustemnt, monocular): every keyframe that is not held fixed and every point with two observations,
// Levenberg-Marquardt with the points eliminated, the reduced camera system never formed.  The problem, the passes over its points and
// the host code around the optional outputs are ba_problem.h's, shared with the local solver (map_ba.hip); ba.h holds the arithmetic of
// an edge and of a point block, gba.h the matrix-free operator, the preconditioner block and the scalar decisions of the conjugate
// gradient; tests/native/gba_check.cpp checks gba.h on the host against ba.h's dense Schur terms.  Here are the per-keyframe edge lists,
// the conjugate-gradient solve and the accept rule.
//
// Chain (every decision - the gauge, the end of a solve, accept / reject, the end - is a flag in GbaRes that the later kernels read first;
// the host waits on that block after the set-up, between steps and between chunks of GBA_CG_CHUNK iterations, only to stop enqueuing;
// [shared]: a kernel of ba_problem.h, instantiated without the e_inl mask and with the Huber width chi2 throughout):
//   k_gba_mark     one thread per map point: its valid edges, problem-point flag, keyframes with edges and their edge counts (integer
//                  atomics count)
//   scans          rank of every problem point, first edge of every problem point, first list entry of every position
//   k_gba_setup    one block: free / fixed / outside per position, the free index and its inverse fpos, the gauge flag
//   k_ba_edges     [shared, with the lists] the compact edge arrays; every edge appended to its position's list
//   k_gba_sort     one workgroup per position: its list ranked into ascending edge order
//   per Levenberg-Marquardt step:
//     k_ba_lin       [shared] V (damped, inverted), g_p, the current cost per point
//     k_gba_diag     one wavefront per free keyframe: H_kk, b_k and the preconditioner block over its edges (strided over the lanes, each
//                    lane in order, wave_sum); lane 0 damps and factors, and starts the solve: x = 0, r = b, z = M^-1 r, p = z
//     k_gba_cg_init  one workgroup: r0.z0
//     per conjugate-gradient iteration:
//       k_gba_mv_pt      one thread per problem point: q = V^-1 sum_e W_e^T p_kf(e)
//       k_gba_mv_kf      one workgroup per free keyframe: y_k = H_kk p_k - sum_e W_e q_pt(e), and p_k . y_k
//       k_gba_cg_update  one workgroup: p.Sp, alpha, x, r, z, r.z, beta, p; the end of the solve
//     k_gba_trial    one workgroup: the trial poses, the largest pose update
//     k_ba_back      [shared] back-substitution, trial position, trial cost
//     k_gba_accept   one workgroup: cost sums, accept / reject, lambda, the end flag; an accepted step becomes the state
//   k_ba_cost      [shared] every edge classified, the final robust cost; k_ba_reduce [shared] sums
//   k_ba_write     [shared] xyz of the problem points and kP of the free keyframes when a step was accepted; the optional outputs
// The Jacobians of an edge (J_c 2x6, J_p 2x3, the weight) are recomputed in every pass from pose, point and keypoint, not stored:
// profiles/gba_rate.txt has the measurement of the stored variant, which NOTES.md records as removed.  No floating-point atomics: sums
// are per-thread in edge order, then wave_sum, then the waves in order.  -ffp-contract=off (Makefile): gba.h and ba.h round on the device
// as in the host build of the test.
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "ba_problem.h"
#include "gba.h"

#define GBA_BLOCK BA_BLOCK
#define GBA_THREADS BA_THREADS
#define GBA_CG_CHUNK 32       // conjugate-gradient iterations enqueued between two looks at the result block

struct GbaPrm {
    double K[9], sf, chi2, step_tol, cg_tol2;
    int32_t n_kf;
};

struct GbaRes {
    double cost[2], lambda, upd_c, rz, rz0;
    int32_t n_points, n_edges, n_free, n_fixed, n_inliers;
    int32_t steps, accepted, cg_iters;
    int32_t run, err, done;            // the problem runs; no fixed position takes part; the optimisation has ended
    int32_t cg_done, cg_it, reject;    // of the step in flight
};
__device__ __forceinline__ bool gba_active(const GbaRes* res) { return res->run && !res->done; }
__device__ __forceinline__ bool gba_cg_active(const GbaRes* res) { return res->run && !res->done && !res->cg_done; }
// what the shared kernels ask (ba_problem.h)
__device__ __forceinline__ bool ba_live(const GbaRes* res, int) { return gba_active(res); }
__device__ __forceinline__ bool ba_has_trial(const GbaRes* res) { return !res->reject; }
__device__ __forceinline__ bool ba_step_accepted(const GbaRes* res) { return res->accepted > 0; }
__device__ __forceinline__ bool ba_xyz_always(const GbaRes*) { return false; }
__device__ __forceinline__ void ba_store_cost(GbaRes* res, int, double cost, int n_inliers) {
    if (res->steps == 0) res->cost[0] = cost;
    res->cost[1] = cost; res->n_inliers = n_inliers;
}

struct GbaBufs : MapFeature {
    DevBuf<double> q;                                            // [problem point][3] V^-1 W^T p
    DevBuf<int32_t> karr, klist;                                 // [edge] the positions' lists in order of arrival, in ascending edge order
    // per keyframe position
    DevBuf<uint8_t> fixed;
    DevBuf<int32_t> kcnt, kbase, kfill;
    // per free keyframe
    DevBuf<double> Hd, L, x, r, z, p, Sp, pdot; DevBuf<uint8_t> kfix;
    ResBlock<GbaRes> res;
    // all of it is scratch: every call's chain writes what it reads
    template <class F> void each_scratch(F f) {
        f(q); f(karr); f(klist); f(fixed); f(kcnt); f(kbase); f(kfill); f(Hd); f(L); f(x); f(r); f(z); f(p); f(Sp); f(pdot); f(kfix); f(res);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

__global__ void k_gba_init(GbaRes* __restrict__ res) {
    if (threadIdx.x) return;
    res->cost[0] = res->cost[1] = 0.0; res->lambda = 1e-4; res->upd_c = 0.0; res->rz = 0.0; res->rz0 = 0.0;
    res->n_points = 0; res->n_edges = 0; res->n_free = 0; res->n_fixed = 0; res->n_inliers = 0;
    res->steps = 0; res->accepted = 0; res->cg_iters = 0;
    res->run = 0; res->err = 0; res->done = 0; res->cg_done = 1; res->cg_it = 0; res->reject = 0;
}

// problem points: >= 2 edges; every position with an edge to one is flagged (plain stores of 1: the racing writers agree) and counts it
__global__ __launch_bounds__(GBA_BLOCK) void k_gba_mark(MapView v, int32_t* __restrict__ loc, int32_t* __restrict__ ecnt, int32_t* __restrict__ kf_edge,
                                                         int32_t* __restrict__ kcnt) {
    const int i = blockIdx.x * GBA_BLOCK + threadIdx.x;
    if (i >= v.n_pts) return;
    int nv = 0;
    map_each_obs(v, i, [&](int, int, int, int) { nv++; return false; });
    const bool prob = nv >= 2;
    loc[i] = prob;
    ecnt[i] = prob ? nv : 0;
    if (prob) map_each_obs(v, i, [&](int, int pos, int, int) { kf_edge[pos] = 1; atomicAdd(kcnt + pos, 1); return false; });
}

// free, fixed and outside positions, the free index in position order, the gauge
__global__ __launch_bounds__(GBA_BLOCK) void k_gba_setup(GbaPrm prm, const uint8_t* __restrict__ fixed, const int32_t* __restrict__ kf_edge,
                                                          int32_t* __restrict__ kf_fidx, int32_t* __restrict__ fpos, int32_t* __restrict__ kbase,
                                                          GbaRes* __restrict__ res) {
    if (threadIdx.x) return;
    int nfixed = 0, nfree = 0;
    for (int pos = 0; pos < prm.n_kf; pos++) {
        if (!kf_edge[pos]) { kf_fidx[pos] = BA_KF_OUT; continue; }
        if (fixed[pos]) { kf_fidx[pos] = BA_KF_FIXED; nfixed++; }
        else { kf_fidx[pos] = nfree; fpos[nfree++] = pos; }
    }
    kbase[prm.n_kf] = res->n_edges;
    res->n_free = nfree; res->n_fixed = nfixed;
    res->err = res->n_points > 0 && nfixed == 0;
    res->run = nfree > 0 && nfixed > 0 && res->n_points > 0;
}

// one workgroup per position: its list into ascending edge order (the edges are distinct: the rank of an edge is the number of smaller
// ones).  Thread t ranks the entries t, t + 256, ... one at a time against the whole list, which passes through LDS in tiles.
#define GBA_SORT_TILE 2048
__global__ __launch_bounds__(GBA_BLOCK) void k_gba_sort(const int32_t* __restrict__ kbase, const int32_t* __restrict__ karr, int32_t* __restrict__ klist,
                                                         const GbaRes* __restrict__ res) {
    __shared__ int32_t tile[GBA_SORT_TILE];
    if (!res->run) return;
    const int b = kbase[blockIdx.x], n = kbase[blockIdx.x + 1] - b;
    for (int i0 = 0; i0 < n; i0 += GBA_BLOCK) {
        const int i = i0 + (int)threadIdx.x;
        const int e = i < n ? karr[b + i] : INT_MAX;
        int rank = 0;
        for (int t0 = 0; t0 < n; t0 += GBA_SORT_TILE) {
            const int m = min(n - t0, GBA_SORT_TILE);
            __syncthreads();
            for (int j = threadIdx.x; j < m; j += GBA_BLOCK) tile[j] = karr[b + t0 + j];
            __syncthreads();
            for (int j = 0; j < m; j++) rank += tile[j] < e;
        }
        if (i < n) klist[b + rank] = e;
    }
}

// residual, weight and Jacobians of edge e of the compact arrays at the current state; false when it contributes nothing
__device__ __forceinline__ bool gba_edge_at(const GbaPrm& prm, const BaEdges& E, int e, const double* __restrict__ pose, const double* __restrict__ X,
                                            double* er, double* w, double* e2, double* Jc, double* Jp) {
    const size_t r = (size_t)E.e_pt[e];
    const double Xp[3] = {X[r * 3], X[r * 3 + 1], X[r * 3 + 2]};
    return ba_edge_lin(prm, prm.chi2, pose + (size_t)E.e_kf[e] * 12, Xp, E.e_xy[(size_t)e * 2], E.e_xy[(size_t)e * 2 + 1], E.e_info[e], er, w, e2, Jc, Jp);
}

// one wavefront per free keyframe: a [0, 36) H_kk, [36, 42) b_k, [42, 78) - sum_e W_e V^-1 W_e^T; lane l takes the list entries l, l + 64, ...
__global__ __launch_bounds__(64) void k_gba_diag(GbaPrm prm, BaEdges E, const int32_t* __restrict__ kbase, const int32_t* __restrict__ klist,
                                                  const int32_t* __restrict__ fpos, const double* __restrict__ X, const double* __restrict__ pose,
                                                  const double* __restrict__ Vi, const double* __restrict__ gp, const uint8_t* __restrict__ pfix,
                                                  double* __restrict__ Hd, double* __restrict__ L, uint8_t* __restrict__ kfix,
                                                  double* __restrict__ x, double* __restrict__ r, double* __restrict__ z, double* __restrict__ p,
                                                  const GbaRes* __restrict__ res) {
    __shared__ double sm[78], H6[36], M[36], Lf[GBA_TRI_N];
    if (!gba_active(res)) return;
    const int f = blockIdx.x;
    if (f >= res->n_free) return;
    const int pos = fpos[f], c0 = kbase[pos], c1 = kbase[pos + 1];
    double a[78];
#pragma unroll
    for (int k = 0; k < 78; k++) a[k] = 0.0;
    for (int c = c0 + (int)threadIdx.x; c < c1; c += 64) {
        const int e = klist[c];
        double er[2], w, e2, Jc[12], Jp[6];
        if (!gba_edge_at(prm, E, e, pose, X, er, &w, &e2, Jc, Jp)) continue;
        ba_camera_terms(Jc, w, er, a, a + 36);
        const size_t pr = (size_t)E.e_pt[e];
        if (pfix[pr]) continue;
        double inv[6], g[3];
        for (int k = 0; k < 6; k++) inv[k] = Vi[pr * 6 + k];
        for (int k = 0; k < 3; k++) g[k] = gp[pr * 3 + k];
        ba_schur_rhs(Jc, Jp, w, inv, g, a + 36);
        gba_precond_edge(Jc, Jp, w, inv, a + 42);
    }
#pragma unroll
    for (int k = 0; k < 78; k++) {
        const double s = wave_sum(a[k]);
        if (threadIdx.x == 0) sm[k] = s;
    }
    if (threadIdx.x) return;
    // lane 0: the blocks in LDS (indexed by loop counters: kept out of the registers the sums above live in)
    double b6[6], z6[6] = {0, 0, 0, 0, 0, 0};
    gba_damp6(sm, res->lambda, H6);
    for (int k = 0; k < 36; k++) M[k] = H6[k] + sm[42 + k];
    const int how = gba_precond_factor(M, H6, Lf);
    for (int k = 0; k < 6; k++) b6[k] = sm[36 + k];
    if (how < 2) gba_solve6(Lf, b6, z6);
    for (int k = 0; k < 36; k++) Hd[(size_t)f * 36 + k] = H6[k];
    for (int k = 0; k < GBA_TRI_N; k++) L[(size_t)f * GBA_TRI_N + k] = Lf[k];
    kfix[f] = how == 2;
    for (int k = 0; k < 6; k++) {
        const size_t j = (size_t)f * 6 + k;
        x[j] = 0.0; r[j] = b6[k]; z[j] = z6[k]; p[j] = z6[k];
    }
}

// thread t takes the free keyframes t, t + 1024, ... in order, each its six entries in order
__device__ __forceinline__ double gba_dot6(int nf, const double* __restrict__ a, const double* __restrict__ b, double* lds) {
    double s = 0.0;
    for (int f = threadIdx.x; f < nf; f += GBA_THREADS)
        for (int k = 0; k < 6; k++) s += a[(size_t)f * 6 + k] * b[(size_t)f * 6 + k];
    return block_sum(s, lds);
}

__global__ __launch_bounds__(GBA_THREADS) void k_gba_cg_init(const double* __restrict__ r, const double* __restrict__ z, GbaRes* __restrict__ res) {
    __shared__ double red[GBA_THREADS / 64];
    if (!gba_active(res)) return;
    const double rz0 = gba_dot6(res->n_free, r, z, red);
    if (threadIdx.x) return;
    const int st = gba_cg_start(rz0);
    res->rz = rz0; res->rz0 = rz0;
    res->cg_done = st != 1; res->cg_it = 0; res->reject = st < 0;
}

// pass (a): q = V^-1 sum_e W_e^T p_kf(e) over the point's edges at free keyframes, in edge order; 0 at a point held for the step
__global__ __launch_bounds__(GBA_BLOCK) void k_gba_mv_pt(GbaPrm prm, BaEdges E, const int32_t* __restrict__ kf_fidx, const double* __restrict__ X,
                                                          const double* __restrict__ pose, const double* __restrict__ Vi, const uint8_t* __restrict__ pfix,
                                                          const double* __restrict__ p, double* __restrict__ q, const GbaRes* __restrict__ res) {
    if (!gba_cg_active(res)) return;
    const int rk = blockIdx.x * GBA_BLOCK + threadIdx.x;
    if (rk >= res->n_points) return;
    double t[3] = {0, 0, 0}, qq[3] = {0, 0, 0};
    if (!pfix[rk]) {
        const double Xp[3] = {X[(size_t)rk * 3], X[(size_t)rk * 3 + 1], X[(size_t)rk * 3 + 2]};
        for (int e = E.eoff[rk]; e < E.eoff[rk + 1]; e++) {
            const int f = kf_fidx[E.e_kf[e]];
            if (f < 0) continue;
            double w, Jc[12], Jp[6], pk[6];
            double er[2], e2;
            if (!ba_edge_lin(prm, prm.chi2, pose + (size_t)E.e_kf[e] * 12, Xp, E.e_xy[(size_t)e * 2], E.e_xy[(size_t)e * 2 + 1], E.e_info[e], er, &w, &e2, Jc, Jp)) continue;
            for (int k = 0; k < 6; k++) pk[k] = p[(size_t)f * 6 + k];
            gba_wt_p(Jc, Jp, w, pk, t);
        }
        double inv[6];
        for (int k = 0; k < 6; k++) inv[k] = Vi[(size_t)rk * 6 + k];
        ba_sym3_mul(inv, t, qq);
    }
    for (int k = 0; k < 3; k++) q[(size_t)rk * 3 + k] = qq[k];
}

// pass (b): one workgroup per free keyframe: y_k = H_kk p_k - sum_e W_e q_pt(e); thread t takes the list entries t, t + blockDim.x, ...
// (256 threads, or 1024 where the free keyframes are few and their lists long: gba_mv_threads)
__global__ __launch_bounds__(GBA_THREADS) void k_gba_mv_kf(GbaPrm prm, BaEdges E, const int32_t* __restrict__ kbase, const int32_t* __restrict__ klist,
                                                          const int32_t* __restrict__ fpos, const double* __restrict__ X, const double* __restrict__ pose,
                                                          const uint8_t* __restrict__ pfix, const double* __restrict__ Hd, const uint8_t* __restrict__ kfix,
                                                          const double* __restrict__ p, const double* __restrict__ q, double* __restrict__ Sp,
                                                          double* __restrict__ pdot, const GbaRes* __restrict__ res) {
    __shared__ double red[GBA_THREADS / 64][6];
    if (!gba_cg_active(res)) return;
    const int NW = blockDim.x >> 6;
    const int f = blockIdx.x;
    if (f >= res->n_free) return;
    if (kfix[f]) {   // (a held vertex: p_k is 0 throughout the solve)
        if (threadIdx.x < 6) Sp[(size_t)f * 6 + threadIdx.x] = 0.0;
        if (threadIdx.x == 0) pdot[f] = 0.0;
        return;
    }
    const int pos = fpos[f], c0 = kbase[pos], c1 = kbase[pos + 1];
    double a[6] = {0, 0, 0, 0, 0, 0};
    for (int c = c0 + (int)threadIdx.x; c < c1; c += (int)blockDim.x) {
        const int e = klist[c];
        const size_t pr = (size_t)E.e_pt[e];
        if (pfix[pr]) continue;
        double er[2], w, e2, Jc[12], Jp[6];
        if (!gba_edge_at(prm, E, e, pose, X, er, &w, &e2, Jc, Jp)) continue;
        const double qq[3] = {q[pr * 3], q[pr * 3 + 1], q[pr * 3 + 2]};
        gba_w_q(Jc, Jp, w, qq, a);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < 6; k++) {
        const double s = wave_sum(a[k]);
        if (lane == 0) red[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x) return;
    double pk[6], y[6], d = 0.0;
    for (int k = 0; k < 6; k++) pk[k] = p[(size_t)f * 6 + k];
    gba_block_mul(Hd + (size_t)f * 36, pk, y);
    for (int k = 0; k < 6; k++) {
        double s = red[0][k];
        for (int w = 1; w < NW; w++) s += red[w][k];
        y[k] -= s;
        Sp[(size_t)f * 6 + k] = y[k];
        d += pk[k] * y[k];
    }
    pdot[f] = d;
}

// one workgroup: p.Sp from the keyframes' partial sums, then the iteration's updates; thread t owns the free keyframes t, t + 1024, ...
__global__ __launch_bounds__(GBA_THREADS) void k_gba_cg_update(GbaPrm prm, const double* __restrict__ L, const uint8_t* __restrict__ kfix,
                                                                const double* __restrict__ Sp, const double* __restrict__ pdot, double* __restrict__ x,
                                                                double* __restrict__ r, double* __restrict__ z, double* __restrict__ p,
                                                                GbaRes* __restrict__ res) {
    __shared__ double red[GBA_THREADS / 64];
    if (!gba_cg_active(res)) return;
    const int nf = res->n_free, tid = threadIdx.x;
    const double rz = res->rz, rz0 = res->rz0;
    const int it = res->cg_it;
    double s = 0.0;
    for (int f = tid; f < nf; f += GBA_THREADS) s += pdot[f];
    const double pSp = block_sum(s, red);
    double alpha;
    if (!gba_cg_alpha(rz, pSp, &alpha)) {
        if (tid == 0) { res->cg_done = 1; res->reject = it == 0; }
        return;
    }
    s = 0.0;
    for (int f = tid; f < nf; f += GBA_THREADS) {
        double r6[6], z6[6] = {0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 6; k++) {
            const size_t j = (size_t)f * 6 + k;
            x[j] += alpha * p[j];
            r6[k] = r[j] - alpha * Sp[j];
            r[j] = r6[k];
        }
        if (!kfix[f]) gba_solve6(L + (size_t)f * GBA_TRI_N, r6, z6);
        for (int k = 0; k < 6; k++) { z[(size_t)f * 6 + k] = z6[k]; s += r6[k] * z6[k]; }
    }
    const double rzn = block_sum(s, red);
    double beta = 0.0;
    const bool go = gba_cg_continue(rzn, prm.cg_tol2, rz0, rz, &beta);
    if (go)
        for (int f = tid; f < nf; f += GBA_THREADS)
            for (int k = 0; k < 6; k++) { const size_t j = (size_t)f * 6 + k; p[j] = z[j] + beta * p[j]; }
    if (tid == 0) {
        res->cg_it = it + 1; res->cg_iters++;
        res->rz = rzn;
        if (!go) res->cg_done = 1;
    }
}

// one workgroup: the trial poses exp(x_k) T_k, the largest pose update
__global__ __launch_bounds__(GBA_THREADS) void k_gba_trial(const int32_t* __restrict__ fpos, const double* __restrict__ x, const double* __restrict__ poseC,
                                                            double* __restrict__ poseT, GbaRes* __restrict__ res) {
    __shared__ double red[GBA_THREADS / 64];
    if (!gba_active(res)) return;
    const int nf = res->n_free;
    double mu = 0.0;
    for (int f = threadIdx.x; f < nf; f += GBA_THREADS) {
        const int pos = fpos[f];
        double d[6], T[12], T2[12];
        for (int k = 0; k < 6; k++) { d[k] = x[(size_t)f * 6 + k]; mu = fmax(mu, fabs(d[k])); }
        for (int k = 0; k < 12; k++) T[k] = poseC[(size_t)pos * 12 + k];
        ba_pose_update(d, T, T2);
        for (int k = 0; k < 12; k++) poseT[(size_t)pos * 12 + k] = T2[k];
    }
    mu = block_max(mu, red);
    if (threadIdx.x == 0) res->upd_c = mu;
}

// one workgroup: current and trial cost, the largest update; accept (the trial becomes the state, lambda / 10) or reject (lambda * 10);
// the end at an update below step_tol or lambda above 1e8.  A step the solve rejected has no trial: lambda * 10, no test of the update.
__global__ __launch_bounds__(GBA_THREADS) void k_gba_accept(GbaPrm prm, const int32_t* __restrict__ fpos, const double* __restrict__ pc,
                                                             const double* __restrict__ pt, const double* __restrict__ pu, double* __restrict__ X,
                                                             const double* __restrict__ Xt, double* __restrict__ poseC, double* __restrict__ poseT,
                                                             GbaRes* __restrict__ res) {
    __shared__ double lds[GBA_THREADS / 64];
    __shared__ int acc;
    if (!gba_active(res)) return;
    const int n = res->n_points, tid = threadIdx.x;
    const bool rej = res->reject;
    double c0 = 0.0, c1 = 0.0, mu = 0.0;
    for (int r = tid; r < n; r += GBA_THREADS) {
        c0 += pc[r];
        if (!rej) { c1 += pt[r]; mu = fmax(mu, pu[r]); }
    }
    c0 = block_sum(c0, lds);
    c1 = block_sum(c1, lds);
    mu = block_max(mu, lds);
    if (tid == 0) {
        const bool ok = !rej && c1 < c0;
        acc = ok;
        const double upd = fmax(mu, res->upd_c);
        const double lam = ok ? res->lambda / 10.0 : res->lambda * 10.0;
        if (res->steps == 0) res->cost[0] = c0;
        res->cost[1] = ok ? c1 : c0;
        res->lambda = lam;
        res->steps++;
        res->accepted += ok;
        res->reject = 0;
        if ((!rej && upd < prm.step_tol) || lam > 1e8) res->done = 1;
    }
    __syncthreads();
    ba_commit(acc, n, res->n_free, fpos, X, Xt, poseC, poseT);
}

// the workgroup of k_gba_mv_kf: 1024 threads where a free keyframe's list averages 4096 edges or more (a function of the map alone)
static unsigned gba_mv_threads(int n_edges, int n_free) { return n_free > 0 && n_edges / n_free >= 4096 ? GBA_THREADS : GBA_BLOCK; }

// the result block read on the host: the chain so far has run
static int gba_look(mo_ctx* c, GbaBufs& b) {
    if (int rc = b.res.download(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MO_OK;
}

extern "C" int mo_map_global_ba(mo_map* m, const double K[9], const double* poses, const mo_map_gba_params* prm, mo_map_gba_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!K || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const int n_kf = (int)m->pos_slot.size();
    if (prm->max_steps < 0 || prm->max_steps > 100) return mo_fail(c, MO_ERR_ARG, "max_steps must be in 0 .. 100");
    if (prm->max_cg < 1) return mo_fail(c, MO_ERR_ARG, "max_cg must be >= 1");
    if (!(prm->cg_tol >= 0.0) || !std::isfinite(prm->cg_tol) || !(prm->step_tol >= 0.0) || !std::isfinite(prm->step_tol))
        return mo_fail(c, MO_ERR_ARG, "cg_tol and step_tol must be finite and >= 0");
    int rc;
    if ((rc = ba_check_common(c, K, poses, n_kf, prm->scale_factor, prm->chi2))) return rc;
    MAP_ENTER(m);
    HostClock clk(c);
    out->cost[0] = out->cost[1] = 0.0; out->lambda = 0.0;
    out->n_free = out->n_fixed = out->n_points = out->n_edges = out->n_inliers = out->steps = out->accepted = out->cg_iters = out->ok = 0;
    const size_t np = (size_t)m->n_pts, no = (size_t)m->n_obs, nk = (size_t)n_kf;
    ba_clear_outputs(out, poses, nk, np, no);
    if (n_kf == 0 || np == 0 || no == 0 || prm->max_steps == 0) return MO_OK;   // nothing runs, not an error
    if ((rc = map_int32_guard(m))) return rc;
    std::vector<uint8_t> fixed(nk, 0);
    if (prm->fixed) { for (size_t i = 0; i < nk; i++) fixed[i] = prm->fixed[i] != 0; }
    else fixed[0] = 1;
    BaProblem& pb = map_feature<BaProblem>(m);
    GbaBufs& b = map_feature<GbaBufs>(m);
    if ((rc = pb.reserve(c, np, no, nk))) return rc;
    if ((rc = mo_reserve(c, b.q, np * 3, b.karr, no, b.klist, no, b.fixed, nk, b.kcnt, nk, b.kbase, nk + 1, b.kfill, nk, b.Hd, nk * 36, b.L, nk * GBA_TRI_N,
                         b.x, nk * 6, b.r, nk * 6, b.z, nk * 6, b.p, nk * 6, b.Sp, nk * 6, b.pdot, nk, b.kfix, nk, b.res)))
        return rc;
    if (out->points_out && (rc = mo_reserve(c, pb.pout, np * 3))) return rc;
    if ((rc = upload_pos_slot(m))) return rc;
    mo_stage_begin(c);
    HIPCHK(c, hipMemcpyAsync(pb.poseC, poses, nk * 96, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(pb.poseT, pb.poseC, nk * 96, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.fixed, fixed.data(), nk, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(pb.kf_edge, 0, nk * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(b.kcnt, 0, nk * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(b.kfill, 0, nk * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(pb.einl, 0, no, c->stream));
    GbaPrm p;
    std::memset(&p, 0, sizeof(p));
    for (int i = 0; i < 9; i++) p.K[i] = K[i];
    p.sf = prm->scale_factor; p.chi2 = prm->chi2; p.step_tol = prm->step_tol; p.cg_tol2 = prm->cg_tol * prm->cg_tol; p.n_kf = n_kf;
    const MapView v = map_view(m);
    const BaEdges E = pb.edges();
    const unsigned mblocks = (unsigned)((np + GBA_BLOCK - 1) / GBA_BLOCK);
    hipLaunchKernelGGL(k_gba_init, dim3(1), dim3(64), 0, c->stream, b.res);
    hipLaunchKernelGGL(k_gba_mark, dim3(mblocks), dim3(GBA_BLOCK), 0, c->stream, v, pb.loc, pb.ecnt, pb.kf_edge, b.kcnt);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, pb.loc, pb.lrank, (int)np, &b.res.p->n_points))) return rc;
    if ((rc = map_scan_excl(m, pb.ecnt, pb.ebase, (int)np, &b.res.p->n_edges))) return rc;
    if ((rc = map_scan_excl(m, b.kcnt, b.kbase, n_kf, b.kbase + n_kf))) return rc;
    hipLaunchKernelGGL(k_gba_setup, dim3(1), dim3(GBA_BLOCK), 0, c->stream, p, b.fixed, pb.kf_edge, pb.kf_fidx, pb.fpos, b.kbase, b.res);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_edges<true, GbaRes>), dim3(mblocks), dim3(GBA_BLOCK), 0, c->stream, v, m->kkps, p.sf, pb.loc, pb.lrank, pb.ebase, pb.eoff,
                       pb.X, pb.e_kf, pb.e_obs, pb.e_pt, pb.e_xy, pb.e_info, nullptr, b.kbase, b.kfill, b.karr, b.res);
    hipLaunchKernelGGL(k_gba_sort, dim3((unsigned)n_kf), dim3(GBA_BLOCK), 0, c->stream, b.kbase, b.karr, b.klist, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "gba_prep");
    if ((rc = gba_look(c, b))) return rc;
    const GbaRes& r = b.res.host();
    if (r.err) return mo_fail(c, MO_ERR_ARG, "no fixed position takes part in the problem");
    const bool run = r.run != 0;
    const int nf = r.n_free;
    const unsigned pblocks = (unsigned)((std::max(r.n_points, 1) + GBA_BLOCK - 1) / GBA_BLOCK), mvt = gba_mv_threads(r.n_edges, nf);
    for (int s = 0; run && s < prm->max_steps && !b.res.host().done; s++) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_lin<false, GbaPrm, GbaRes>), dim3(pblocks), dim3(GBA_BLOCK), 0, c->stream, p, 0, E, pb.X, pb.poseC, pb.Vi, pb.gp,
                           pb.pfix, pb.pc, b.res);
        hipLaunchKernelGGL(k_gba_diag, dim3((unsigned)nf), dim3(64), 0, c->stream, p, E, b.kbase, b.klist, pb.fpos, pb.X, pb.poseC, pb.Vi, pb.gp, pb.pfix, b.Hd,
                           b.L, b.kfix, b.x, b.r, b.z, b.p, b.res);
        hipLaunchKernelGGL(k_gba_cg_init, dim3(1), dim3(GBA_THREADS), 0, c->stream, b.r, b.z, b.res);
        HIPCHK(c, hipGetLastError());
        for (int it = 0; it < prm->max_cg; it++) {
            hipLaunchKernelGGL(k_gba_mv_pt, dim3(pblocks), dim3(GBA_BLOCK), 0, c->stream, p, E, pb.kf_fidx, pb.X, pb.poseC, pb.Vi, pb.pfix, b.p, b.q, b.res);
            hipLaunchKernelGGL(k_gba_mv_kf, dim3((unsigned)nf), dim3(mvt), 0, c->stream, p, E, b.kbase, b.klist, pb.fpos, pb.X, pb.poseC, pb.pfix, b.Hd, b.kfix,
                               b.p, b.q, b.Sp, b.pdot, b.res);
            hipLaunchKernelGGL(k_gba_cg_update, dim3(1), dim3(GBA_THREADS), 0, c->stream, p, b.L, b.kfix, b.Sp, b.pdot, b.x, b.r, b.z, b.p, b.res);
            if ((it + 1) % GBA_CG_CHUNK == 0 && it + 1 < prm->max_cg) {
                HIPCHK(c, hipGetLastError());
                if ((rc = gba_look(c, b))) return rc;
                if (b.res.host().cg_done) break;
            }
        }
        // (the iterations end at max_cg: a solve still open is closed by the trial, which reads x as it stands)
        hipLaunchKernelGGL(k_gba_trial, dim3(1), dim3(GBA_THREADS), 0, c->stream, pb.fpos, b.x, pb.poseC, pb.poseT, b.res);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_back<false, GbaPrm, GbaRes>), dim3(pblocks), dim3(GBA_BLOCK), 0, c->stream, p, 0, E, pb.kf_fidx, pb.X, pb.poseC,
                           pb.poseT, pb.Vi, pb.gp, pb.pfix, b.x, pb.Xt, pb.pt, pb.pu, b.res);
        hipLaunchKernelGGL(k_gba_accept, dim3(1), dim3(GBA_THREADS), 0, c->stream, p, pb.fpos, pb.pc, pb.pt, pb.pu, pb.X, pb.Xt, pb.poseC, pb.poseT, b.res);
        HIPCHK(c, hipGetLastError());
        if ((rc = gba_look(c, b))) return rc;
    }
    mo_stage_mark(c, "gba_steps");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_cost<false, GbaPrm, GbaRes>), dim3(pblocks), dim3(GBA_BLOCK), 0, c->stream, p, 1, E, pb.X, pb.poseC, pb.e_inl, pb.pc, pb.pn,
                       b.res);
    hipLaunchKernelGGL(k_ba_reduce<GbaRes>, dim3(1), dim3(GBA_THREADS), 0, c->stream, 1, pb.pc, pb.pn, b.res);
    const unsigned wblocks = (unsigned)((std::max(np, no) + GBA_BLOCK - 1) / GBA_BLOCK);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_write<GbaPrm, GbaRes>), dim3(wblocks), dim3(GBA_BLOCK), 0, c->stream, p, (int)np, (int)no, pb.loc, pb.lrank, pb.X,
                       v.src.xyz, out->points_out ? pb.pout.p : nullptr, pb.e_obs, pb.e_inl, pb.einl, m->d_pos_slot, pb.fpos, pb.poseC, m->kP, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "gba_write");
    std::vector<int32_t> fidx(out->kf_state ? nk : 0);
    if ((rc = b.res.download(c))) return rc;
    if (run && (rc = ba_copy_outputs(c, pb, out, nk, np, no, fidx))) return rc;
    if ((rc = map_sync(c, clk))) return rc;
    if (!run) return MO_OK;   // no free position with an edge, or no problem point
    out->cost[0] = r.cost[0]; out->cost[1] = r.cost[1]; out->lambda = r.lambda;
    out->n_free = r.n_free; out->n_fixed = r.n_fixed; out->n_points = r.n_points; out->n_edges = r.n_edges; out->n_inliers = r.n_inliers;
    out->steps = r.steps; out->accepted = r.accepted; out->cg_iters = r.cg_iters;
    ba_fill_kf_state(out, fidx, nk);
    out->ok = r.n_inliers >= prm->min_inliers;
    return MO_OK;
}
