// map_ba.hip -- local bundle adjustment on the device map (mo_map_bundle_adjust in include/vslam_amd.h: ORB-SLAM2's
// Optimizer::LocalBundleAdjustment, monocular) and the call that gives it multi-view tracks (mo_map_add_observations).
//
// Chain of one bundle adjustment (one synchronisation, the copy-out; every decision - the gauge, accept / reject, the end of a round -
// is a flag in BaRes that the later kernels read first):
//   k_ba_mark      one thread per map point: its valid edges (map_obs), local-point flag, keyframes with edges
//   scans          local rank of every local point, first compact edge of every local point (the map's device-wide scan)
//   k_ba_setup     one block: free / fixed keyframes and the gauge rule, free index of every position
//   k_ba_edges     one thread per map point: its edges in CSR order into the compact edge arrays, its position as f64
//   k_ba_cost      one thread per local point: cost of its edges, classification between the rounds; k_ba_reduce sums in a fixed tree
//   per Levenberg-Marquardt step:
//     k_ba_lin     one thread per local point: V (damped, inverted), g_p, its current cost
//     k_ba_pair    one workgroup per free-keyframe pair (i <= j): the 6x6 block S_ij (and b_i on the diagonal) summed over the local
//                  points in a fixed thread assignment and a fixed reduction tree; Jacobians are recomputed, not stored
//     k_ba_solve   one workgroup: the reduced system (<= 96) packed in LDS, left-looking Cholesky across the block, substitution, the
//                  trial poses
//     k_ba_back    one thread per local point: back-substitution, trial position, trial cost
//     k_ba_accept  one workgroup: cost sums, accept / reject, lambda, the end-of-round flags; an accepted step becomes the state
//   k_ba_write     xyz (f32) of the local points, kP of the free keyframes, the optional outputs
// No floating-point atomics anywhere: sums are per-thread in index order, then fixed wave / workgroup trees.
// -ffp-contract=off (Makefile): ba.h rounds on the device as in the host build of tests/native/ba_check.cpp.
//
// mo_map_bundle_adjust_local is the same chain over a set of candidate positions instead of a window (ba_run enqueues both):
//   candidates     the caller's mask, or k_covis and k_covis_select of map_covis.hip in this chain (the covis_* pieces, as
//                  mo_map_track_covisible runs them) and their mask read on the device; k_bal_cand drops position 0 and counts
//   k_ba_mark_set  k_ba_mark with "position in C" for "position >= lo_pos and != 0"
//   k_ba_setup_set k_ba_setup with the same substitution: positions outside C are fixed, the gauge takes the lowest ones of C
//   ... every kernel from k_ba_edges to k_ba_write as above ...
//   erase_outliers the entry erase below behind k_ba_write, gated on the device by BaRes (run, n_inliers >= min_inliers), class 2 leaves
// The entry erase (mo_map_erase_observations; entry-parallel, no point walks its own list):
//   k_oe_keep      one thread per entry: keep[o] (int32)
//   map_scan_excl  over the n_obs entries: S[o] = the new place of a kept entry, the total = the new n_obs
//   k_oe_points    one thread per point: its fields (map_point_copy) and off[i] = S[off[i]] into the other copy; the points that lost an
//                  entry and hold fewer than two are counted in registers, one integer atomic per workgroup
//   k_oe_entries   one thread per entry: okf / okp of a kept entry to S[o], coalesced reads, ascending writes
// With nothing flagged both kernels return at once and the host does not flip the copies (mo_map_erase_points' behaviour).
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "map_store.h"
#include "ba.h"

#define BA_BLOCK 256
#define BA_MAX_PAIRS (BA_MAX_FREE * (BA_MAX_FREE + 1) / 2)
#define BA_TRI_N (BA_MAX_DIM * (BA_MAX_DIM + 1) / 2)
#define BA_KF_OUT (-2)    // kf_fidx: the position has no edge to a local point
#define BA_KF_FIXED (-1)  // kf_fidx: fixed keyframe (>= 0: index among the free ones)

struct BaPrm {
    double K[9], sf, chi2;
    int n_kf, lo_pos;
};

struct BaRes {
    double cost[3], lambda, upd_c;
    int32_t n_local, n_edges, n_free, n_fixed, n_inliers;
    int32_t steps[2], accepted[2], done[2];
    int32_t run, step_ok;
    int32_t free_pos[BA_MAX_FREE];
};

struct BaBufs : MapFeature {
    // per map point
    DevBuf<int32_t> loc, ecnt, lrank, ebase;
    DevBuf<double> pout;                                         // [point][3] the optional f64 output
    // per local point (by local rank)
    DevBuf<int32_t> lpt, eoff, pn; DevBuf<uint8_t> pfix;
    DevBuf<double> X, Xt, Vi, gp, pc, pt, pu;
    // per edge (compact, CSR order of the local points)
    DevBuf<int32_t> e_kf, e_obs; DevBuf<float> e_xy; DevBuf<double> e_info; DevBuf<uint8_t> e_inl;
    DevBuf<uint8_t> einl;                                        // [observation] 0 / 1 / 2
    // per keyframe position
    DevBuf<int32_t> kf_edge, kf_fidx; DevBuf<double> poseC, poseT;
    DevBuf<double> S;                                            // [96][96] reduced system, [96] right side, [96] solution
    ResBlock<BaRes> res;
    // mo_map_add_observations
    DevBuf<int32_t> ao_pt, ao_row, ao_claim, ao_cnt, ao_base, ao_total;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) {
        f(loc); f(ecnt); f(lrank); f(ebase); f(pout); f(lpt); f(eoff); f(pn); f(pfix); f(X); f(Xt); f(Vi); f(gp); f(pc); f(pt); f(pu);
        f(e_kf); f(e_obs); f(e_xy); f(e_info); f(e_inl); f(einl); f(kf_edge); f(kf_fidx); f(poseC); f(poseT); f(S); f(res);
        f(ao_pt); f(ao_row); f(ao_claim); f(ao_cnt); f(ao_base); f(ao_total);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// fixed-order sums: lane 0's shuffle tree per wave (wave_sum), then the waves in order; every thread receives the result
__device__ __forceinline__ double ba_block_sum(double v, double* lds) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    v = wave_sum(v);
    if (lane == 0) lds[wv] = v;
    __syncthreads();
    double s = lds[0];
    for (int w = 1; w < nw; w++) s += lds[w];
    __syncthreads();
    return s;
}
__device__ __forceinline__ double ba_block_max(double v, double* lds) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int d = 32; d; d >>= 1) v = fmax(v, __shfl_down(v, d, 64));
    if (lane == 0) lds[wv] = v;
    __syncthreads();
    double s = lds[0];
    for (int w = 1; w < nw; w++) s = fmax(s, lds[w]);
    __syncthreads();
    return s;
}

__global__ void k_ba_init(BaRes* __restrict__ res) {
    if (threadIdx.x) return;
    for (int i = 0; i < 3; i++) res->cost[i] = 0.0;
    res->lambda = 1e-4; res->upd_c = 0.0;
    res->n_local = 0; res->n_edges = 0; res->n_free = 0; res->n_fixed = 0; res->n_inliers = 0;
    for (int i = 0; i < 2; i++) { res->steps[i] = 0; res->accepted[i] = 0; res->done[i] = 0; }
    res->run = 0; res->step_ok = 0;
    for (int i = 0; i < BA_MAX_FREE; i++) res->free_pos[i] = -1;
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
__global__ __launch_bounds__(BA_BLOCK) void k_ba_setup(BaPrm prm, const int32_t* __restrict__ kf_edge, int32_t* __restrict__ kf_fidx, BaRes* __restrict__ res) {
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
        else if (nfree < BA_MAX_FREE) { kf_fidx[pos] = nfree; res->free_pos[nfree++] = pos; }
        else kf_fidx[pos] = BA_KF_FIXED;   // (the host refuses windows wider than BA_MAX_FREE: not reached)
    }
    res->n_free = nfree; res->n_fixed = nfixed;
    res->run = nfree > 0 && res->n_local > 0;
}

__global__ __launch_bounds__(BA_BLOCK) void k_ba_edges(MapView v, const mo_keypoint* __restrict__ kkps, double sf, const int32_t* __restrict__ loc,
                                                       const int32_t* __restrict__ lrank, const int32_t* __restrict__ ebase, int32_t* __restrict__ lpt,
                                                       int32_t* __restrict__ eoff, double* __restrict__ X, int32_t* __restrict__ e_kf,
                                                       int32_t* __restrict__ e_obs, float* __restrict__ e_xy, double* __restrict__ e_info,
                                                       uint8_t* __restrict__ e_inl, const BaRes* __restrict__ res) {
    const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (i == 0) eoff[res->n_local] = res->n_edges;
    if (i >= v.n_pts || !loc[i]) return;
    const int r = lrank[i];
    lpt[r] = i;
    int e = ebase[i];
    eoff[r] = e;
    for (int k = 0; k < 3; k++) X[(size_t)r * 3 + k] = v.src.xyz[(size_t)i * 3 + k];
    map_each_obs(v, i, [&](int o, int pos, int s, int kp) {
        const mo_keypoint q = kkps[(size_t)s * v.row + kp];
        e_kf[e] = pos; e_obs[e] = o; e_xy[(size_t)e * 2] = q.x; e_xy[(size_t)e * 2 + 1] = q.y; e_info[e] = ba_info(sf, q.octave); e_inl[e] = 1;
        e++;
        return false;
    });
}

// mode 0: robust cost of every edge; 1: the same and every edge classified; 2: every edge classified, plain cost of the inliers
__global__ __launch_bounds__(BA_BLOCK) void k_ba_cost(BaPrm prm, int mode, const int32_t* __restrict__ eoff, const double* __restrict__ X,
                                                      const int32_t* __restrict__ e_kf, const float* __restrict__ e_xy, const double* __restrict__ e_info,
                                                      uint8_t* __restrict__ e_inl, const double* __restrict__ pose, double* __restrict__ pc,
                                                      int32_t* __restrict__ pn, const BaRes* __restrict__ res) {
    if (!res->run) return;
    const int r = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (r >= res->n_local) return;
    const double Xp[3] = {X[(size_t)r * 3], X[(size_t)r * 3 + 1], X[(size_t)r * 3 + 2]};
    double cost = 0.0;
    int n = 0;
    for (int e = eoff[r]; e < eoff[r + 1]; e++) {
        double er[2], zc;
        const bool fin = ba_residual(prm.K, pose + (size_t)e_kf[e] * 12, Xp, e_xy[(size_t)e * 2], e_xy[(size_t)e * 2 + 1], er, &zc);
        const double e2 = fin ? e_info[e] * (er[0] * er[0] + er[1] * er[1]) : 0.0;
        const bool in = fin && zc > 0.0 && e2 <= prm.chi2;
        if (mode) e_inl[e] = in;
        n += in;
        if (fin && mode < 2) cost += ba_rho(e2, prm.chi2);
        if (in && mode == 2) cost += e2;
    }
    pc[r] = cost;
    pn[r] = n;
}

__global__ __launch_bounds__(1024) void k_ba_reduce(int idx, const double* __restrict__ pc, const int32_t* __restrict__ pn, BaRes* __restrict__ res) {
    __shared__ double lds[16];
    __shared__ int cnt;
    if (!res->run) return;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const int n = res->n_local;
    double s = 0.0;
    int c = 0;
    for (int r = threadIdx.x; r < n; r += 1024) { s += pc[r]; c += pn[r]; }
    s = ba_block_sum(s, lds);
    c = wave_sum_int(c);
    if ((threadIdx.x & 63) == 0) atomicAdd(&cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) {
        res->cost[idx] = s; res->n_inliers = cnt;
        if (idx == 1) res->lambda = 1e-4;   // every round starts from the same damping
    }
}

__device__ __forceinline__ bool ba_active(const BaRes* res, int round) { return res->run && !res->done[round]; }

// residual, weight and Jacobians of edge e at the current state; false when the edge contributes nothing
__device__ __forceinline__ bool ba_edge_lin(const BaPrm& prm, double huber2, const double* T, const double* Xp, float x, float y, double info, double* er,
                                            double* w, double* e2, double* Jc, double* Jp) {
    double zc;
    if (!ba_residual(prm.K, T, Xp, x, y, er, &zc)) return false;
    *e2 = info * (er[0] * er[0] + er[1] * er[1]);
    *w = info * ba_weight(*e2, huber2);
    return ba_jacobians(prm.K, T, Xp, Jc, Jp);
}

__global__ __launch_bounds__(BA_BLOCK) void k_ba_lin(BaPrm prm, int round, const int32_t* __restrict__ eoff, const double* __restrict__ X,
                                                     const int32_t* __restrict__ e_kf, const float* __restrict__ e_xy, const double* __restrict__ e_info,
                                                     const uint8_t* __restrict__ e_inl, const double* __restrict__ pose, double* __restrict__ Vi,
                                                     double* __restrict__ gp, uint8_t* __restrict__ pfix, double* __restrict__ pc,
                                                     const BaRes* __restrict__ res) {
    if (!ba_active(res, round)) return;
    const int r = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (r >= res->n_local) return;
    const double huber2 = round == 0 ? prm.chi2 : 0.0, damp = 1.0 + res->lambda;
    const double Xp[3] = {X[(size_t)r * 3], X[(size_t)r * 3 + 1], X[(size_t)r * 3 + 2]};
    double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, cost = 0.0;
    for (int e = eoff[r]; e < eoff[r + 1]; e++) {
        if (round && !e_inl[e]) continue;
        double er[2], w, e2, Jc[12], Jp[6];
        if (!ba_edge_lin(prm, huber2, pose + (size_t)e_kf[e] * 12, Xp, e_xy[(size_t)e * 2], e_xy[(size_t)e * 2 + 1], e_info[e], er, &w, &e2, Jc, Jp)) continue;
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

// one workgroup per pair of free keyframes (i <= j): S_ij = [i == j] (H_ii + lambda diag H_ii) - sum over points W_i V^-1 W_j^T, and
// on the diagonal b_i = g_i - sum W_i V^-1 g_p.  Thread t takes the local points t, t + 256, ... in order; 48 sums per thread.
__global__ __launch_bounds__(BA_BLOCK) void k_ba_pair(BaPrm prm, int round, const int32_t* __restrict__ eoff, const double* __restrict__ X,
                                                      const int32_t* __restrict__ e_kf, const float* __restrict__ e_xy, const double* __restrict__ e_info,
                                                      const uint8_t* __restrict__ e_inl, const int32_t* __restrict__ kf_fidx, const double* __restrict__ pose,
                                                      const double* __restrict__ Vi, const double* __restrict__ gp, const uint8_t* __restrict__ pfix,
                                                      double* __restrict__ S, const BaRes* __restrict__ res) {
    constexpr int NW = BA_BLOCK / 64;
    __shared__ double red[NW][48];
    if (!ba_active(res, round)) return;
    const int nf = res->n_free;
    int fi = 0, rem = blockIdx.x;
    while (fi < nf && rem >= nf - fi) { rem -= nf - fi; fi++; }
    if (fi >= nf) return;
    const int fj = fi + rem;
    const bool diag = fi == fj;
    const double huber2 = round == 0 ? prm.chi2 : 0.0, lambda = res->lambda;
    const int n = res->n_local;
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
            if (!ba_edge_lin(prm, huber2, pose + (size_t)e_kf[ea] * 12, Xp, e_xy[(size_t)ea * 2], e_xy[(size_t)ea * 2 + 1], e_info[ea], era, &wa, &e2a, Jca, Jpa))
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
                if (!ba_edge_lin(prm, huber2, pose + (size_t)e_kf[eb] * 12, Xp, e_xy[(size_t)eb * 2], e_xy[(size_t)eb * 2 + 1], e_info[eb], erb, &wb, &e2b, Jcb,
                                 Jpb))
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
__global__ __launch_bounds__(BA_BLOCK) void k_ba_solve(int round, const double* __restrict__ S, double* __restrict__ dc, const double* __restrict__ poseC,
                                                       double* __restrict__ poseT, BaRes* __restrict__ res) {
    __shared__ double L[BA_TRI_N];
    __shared__ double bl[BA_MAX_DIM], x[BA_MAX_DIM];
    __shared__ int bad;
    if (!ba_active(res, round)) return;
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
        const int pos = res->free_pos[tid];
        double d[6], T[12], T2[12];
        for (int k = 0; k < 6; k++) d[k] = x[6 * tid + k];
        for (int k = 0; k < 12; k++) T[k] = poseC[(size_t)pos * 12 + k];
        ba_pose_update(d, T, T2);
        for (int k = 0; k < 12; k++) poseT[(size_t)pos * 12 + k] = T2[k];
    }
}

__global__ __launch_bounds__(BA_BLOCK) void k_ba_back(BaPrm prm, int round, const int32_t* __restrict__ eoff, const double* __restrict__ X,
                                                      const int32_t* __restrict__ e_kf, const float* __restrict__ e_xy, const double* __restrict__ e_info,
                                                      const uint8_t* __restrict__ e_inl, const int32_t* __restrict__ kf_fidx, const double* __restrict__ poseC,
                                                      const double* __restrict__ poseT, const double* __restrict__ Vi, const double* __restrict__ gp,
                                                      const uint8_t* __restrict__ pfix, const double* __restrict__ dc, double* __restrict__ Xt,
                                                      double* __restrict__ pt, double* __restrict__ pu, const BaRes* __restrict__ res) {
    if (!ba_active(res, round) || !res->step_ok) return;
    const int r = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (r >= res->n_local) return;
    const double huber2 = round == 0 ? prm.chi2 : 0.0;
    const double Xp[3] = {X[(size_t)r * 3], X[(size_t)r * 3 + 1], X[(size_t)r * 3 + 2]};
    const int e0 = eoff[r], e1 = eoff[r + 1];
    double dp[3] = {0, 0, 0};
    if (!pfix[r]) {
        double g[3], inv[6];
        for (int k = 0; k < 3; k++) g[k] = gp[(size_t)r * 3 + k];
        for (int k = 0; k < 6; k++) inv[k] = Vi[(size_t)r * 6 + k];
        for (int e = e0; e < e1; e++) {
            if (round && !e_inl[e]) continue;
            const int f = kf_fidx[e_kf[e]];
            if (f < 0) continue;
            double er[2], w, e2, Jc[12], Jp[6];
            if (!ba_edge_lin(prm, huber2, poseC + (size_t)e_kf[e] * 12, Xp, e_xy[(size_t)e * 2], e_xy[(size_t)e * 2 + 1], e_info[e], er, &w, &e2, Jc, Jp)) continue;
            ba_back_edge(Jc, Jp, w, dc + 6 * f, g);
        }
        ba_sym3_mul(inv, g, dp);
    }
    const double Xn[3] = {Xp[0] + dp[0], Xp[1] + dp[1], Xp[2] + dp[2]};
    double cost = 0.0;
    for (int e = e0; e < e1; e++) {
        if (round && !e_inl[e]) continue;
        double er[2], zc;
        if (!ba_residual(prm.K, poseT + (size_t)e_kf[e] * 12, Xn, e_xy[(size_t)e * 2], e_xy[(size_t)e * 2 + 1], er, &zc)) continue;
        cost += ba_rho(e_info[e] * (er[0] * er[0] + er[1] * er[1]), huber2);
    }
    for (int k = 0; k < 3; k++) Xt[(size_t)r * 3 + k] = Xn[k];
    pt[r] = cost;
    pu[r] = fmax(fabs(dp[0]), fmax(fabs(dp[1]), fabs(dp[2])));
}

// one workgroup: current and trial cost, the largest update; accept (the trial becomes the state, lambda / 10) or reject (lambda * 10);
// the round ends at an update below 1e-10 or lambda above 1e8
__global__ __launch_bounds__(1024) void k_ba_accept(int round, const double* __restrict__ pc, const double* __restrict__ pt, const double* __restrict__ pu,
                                                    double* __restrict__ X, const double* __restrict__ Xt, double* __restrict__ poseC,
                                                    double* __restrict__ poseT, BaRes* __restrict__ res) {
    __shared__ double lds[16];
    __shared__ int acc;
    if (!ba_active(res, round) || !res->step_ok) return;
    const int n = res->n_local, tid = threadIdx.x;
    double c0 = 0.0, c1 = 0.0, mu = 0.0;
    for (int r = tid; r < n; r += 1024) { c0 += pc[r]; c1 += pt[r]; mu = fmax(mu, pu[r]); }
    c0 = ba_block_sum(c0, lds);
    c1 = ba_block_sum(c1, lds);
    mu = ba_block_max(mu, lds);
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
    const int nf = res->n_free;
    if (acc) {
        for (int k = tid; k < n * 3; k += 1024) X[k] = Xt[k];
        for (int k = tid; k < nf * 12; k += 1024) { const size_t o = (size_t)res->free_pos[k / 12] * 12 + k % 12; poseC[o] = poseT[o]; }
    } else {
        for (int k = tid; k < nf * 12; k += 1024) { const size_t o = (size_t)res->free_pos[k / 12] * 12 + k % 12; poseT[o] = poseC[o]; }
    }
}

// the results into the map: xyz of the local points, kP = K [R | t] of the free keyframes; the optional outputs
__global__ __launch_bounds__(BA_BLOCK) void k_ba_write(BaPrm prm, int n_pts, int n_obs_edges, const int32_t* __restrict__ loc, const int32_t* __restrict__ lrank,
                                                       const double* __restrict__ X, float* __restrict__ xyz, double* __restrict__ pout,
                                                       const int32_t* __restrict__ e_obs, const uint8_t* __restrict__ e_inl, uint8_t* __restrict__ einl,
                                                       const int32_t* __restrict__ pos_slot, const double* __restrict__ poseC, double* __restrict__ kP,
                                                       const BaRes* __restrict__ res) {
    const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
    const bool run = res->run;
    if (i < n_pts) {
        const bool local = run && loc[i];
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int k = 0; k < 3; k++) {
            const double v = local ? X[(size_t)lrank[i] * 3 + k] : nan;
            if (pout) pout[(size_t)i * 3 + k] = v;
            if (local) xyz[(size_t)i * 3 + k] = (float)v;
        }
    }
    if (!run) return;
    if (i < res->n_edges && i < n_obs_edges) einl[e_obs[i]] = e_inl[i] ? 1 : 2;
    if (i < res->n_free && res->accepted[0] + res->accepted[1] > 0) {   // (no accepted step: the poses are the given ones, kP stays)
        const int pos = res->free_pos[i];
        double R[9], t[3], P[12];
        pose_split(poseC + (size_t)pos * 12, R, t);
        pnp_projection(prm.K, R, t, P);
        for (int k = 0; k < 12; k++) kP[(size_t)pos_slot[pos] * 12 + k] = P[k];
    }
}

// ---- the set form and the entry erase: scratch, kernels ------------------------------------------------------------------------------
struct BalRes { int32_t n_candidates, n_obs, n_under; };   // C before the gauge; the entries behind the erase; the points left under two

struct BaLocalBufs : MapFeature {
    DevBuf<uint8_t> cand_in, cand;                    // [n_kf] the caller's mask as given; C (position 0 dropped)
    DevBuf<uint8_t> flag;                             // [n_obs] the caller's erase flags (mo_map_erase_observations)
    DevBuf<int32_t> keep, S;                          // [n_obs] 1 at an entry that stays; its exclusive scan
    ResBlock<BalRes> res;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) { f(cand_in); f(cand); f(flag); f(keep); f(S); f(res); }
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
                                                           int32_t* __restrict__ kf_fidx, BaRes* __restrict__ res) {
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
        else if (nfree < BA_MAX_FREE) { kf_fidx[pos] = nfree; res->free_pos[nfree++] = pos; }
        else kf_fidx[pos] = BA_KF_FIXED;   // (the host refuses sets of more than BA_MAX_FREE: not reached)
    }
    res->n_free = nfree; res->n_fixed = nfixed;
    res->run = nfree > 0 && res->n_local > 0;
}

// entry o leaves where the caller's flag is set (gate NULL) or, behind a bundle adjustment, where its final class is 2 and the problem ran
// and ended with >= min_inliers inliers (a failed adjustment erases nothing)
__global__ __launch_bounds__(BA_BLOCK) void k_oe_keep(const uint8_t* __restrict__ flag, const BaRes* __restrict__ gate, int min_inliers, int n_obs,
                                                      int32_t* __restrict__ keep) {
    const int o = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (o >= n_obs) return;
    const bool gone = gate ? gate->run && gate->n_inliers >= min_inliers && flag[o] == 2 : flag[o] != 0;
    keep[o] = !gone;
}

// the place of entry o behind the erase; o == n_obs (the end of the last list): the total
__device__ __forceinline__ int oe_place(const int32_t* __restrict__ S, int o, int n_obs, int total) { return o < n_obs ? S[o] : total; }

// every point's fields and its new offset into the other copy (the points keep their indices); workgroups stride over the points and add
// their count of points that lost an entry and hold fewer than two once
__global__ __launch_bounds__(BA_BLOCK) void k_oe_points(MapPts src, MapPts dst, int n_pts, int n_obs, const int32_t* __restrict__ S, BalRes* res,
                                                        int32_t* __restrict__ st) {
    __shared__ int sw[BA_BLOCK / 64];
    const int total = res->n_obs;
    if (total == n_obs) return;   // (nothing leaves: nothing is written, the host does not flip the copies)
    int under = 0;
    for (int i = blockIdx.x * BA_BLOCK + threadIdx.x; i < n_pts; i += gridDim.x * BA_BLOCK) {
        const int a = src.off[i], b = src.off[i + 1];
        const int na = oe_place(S, a, n_obs, total), nb = oe_place(S, b, n_obs, total);
        map_point_copy(src, i, dst, i);
        dst.off[i] = na;
        under += nb - na < b - a && nb - na < 2;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { dst.off[n_pts] = total; st[ST_NPTS] = n_pts; st[ST_NOBS] = total; }   // (the next call's live counts)
    under = wave_sum_int(under);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = under;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < BA_BLOCK / 64; w++) t += sw[w];
        if (t) atomicAdd(&res->n_under, t);
    }
}

// a kept entry's stored bytes at its new place
__global__ __launch_bounds__(BA_BLOCK) void k_oe_entries(MapPts src, MapPts dst, int n_obs, const int32_t* __restrict__ keep, const int32_t* __restrict__ S,
                                                         const BalRes* __restrict__ res) {
    const int o = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (o >= n_obs || res->n_obs == n_obs || !keep[o]) return;
    const int d = S[o];
    dst.okf[d] = src.okf[o]; dst.okp[d] = src.okp[o];
}

#define OE_MAX_BLOCKS 2048   // workgroups of k_oe_points (one atomic each)

// keep -> S and the two copies enqueued (keep, S and the other copy of the store reserved by the caller, res zeroed in front)
static int oe_enqueue(mo_map* m, BaLocalBufs& lb, const uint8_t* flag, const BaRes* gate, int min_inliers) {
    mo_ctx* c = m->c;
    const size_t np = (size_t)m->n_pts, no = (size_t)m->n_obs;
    const unsigned oblocks = (unsigned)((no + BA_BLOCK - 1) / BA_BLOCK);
    const unsigned pblocks = (unsigned)std::min<size_t>((np + BA_BLOCK - 1) / BA_BLOCK, OE_MAX_BLOCKS);
    const MapPts src = m->P[m->cur].view(), dst = m->P[m->cur ^ 1].view();
    int rc;
    hipLaunchKernelGGL(k_oe_keep, dim3(oblocks), dim3(BA_BLOCK), 0, c->stream, flag, gate, min_inliers, (int)no, lb.keep);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, lb.keep, lb.S, (int)no, &lb.res.p->n_obs))) return rc;
    hipLaunchKernelGGL(k_oe_points, dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, src, dst, (int)np, (int)no, lb.S, lb.res, m->st);
    hipLaunchKernelGGL(k_oe_entries, dim3(oblocks), dim3(BA_BLOCK), 0, c->stream, src, dst, (int)no, lb.keep, lb.S, lb.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "obs_erase");
    return MO_OK;
}

// behind the synchronisation: the copies flipped, the count taken; returns the number of entries that left
static int32_t oe_finish(mo_map* m, const BalRes& r) {
    const int64_t gone = m->n_obs - r.n_obs;
    if (gone) { m->cur ^= 1; m->n_obs = r.n_obs; }
    return (int32_t)gone;
}

// mo_map_bundle_adjust (lprm NULL: the window form and exactly the launches it had) and mo_map_bundle_adjust_local
static int ba_run(mo_map* m, const double K[9], const double* poses, const mo_map_ba_params* prm, mo_map_ba_out* out, const mo_map_ba_local_params* lprm,
                  mo_map_ba_local_out* lout) {
    mo_ctx* c = m->c;
    if (!K || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const int n_kf = (int)m->pos_slot.size();
    if (n_kf > 0 && !poses) return mo_fail(c, MO_ERR_ARG, "poses is NULL");
    if (prm->window < 0) return mo_fail(c, MO_ERR_ARG, "window must be >= 0");
    if (!(prm->scale_factor > 0.0) || !std::isfinite(prm->scale_factor)) return mo_fail(c, MO_ERR_ARG, "scale_factor must be finite and > 0");
    if (!(prm->chi2 >= 0.0) || !std::isfinite(prm->chi2)) return mo_fail(c, MO_ERR_ARG, "chi2 must be finite and >= 0");
    for (int r = 0; r < 2; r++)
        if (prm->max_steps[r] < 0 || prm->max_steps[r] > 100) return mo_fail(c, MO_ERR_ARG, "max_steps must be in 0 .. 100");
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(K[i])) return mo_fail(c, MO_ERR_ARG, "K must be finite");
    for (size_t i = 0; i < (size_t)n_kf * 12; i++)
        if (!std::isfinite(poses[i])) return mo_fail(c, MO_ERR_ARG, "poses must be finite");
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
    const size_t np = (size_t)m->n_pts, no = (size_t)m->n_obs;
    if (out->poses_out && n_kf) std::memcpy(out->poses_out, poses, (size_t)n_kf * 96);
    if (out->kf_state) for (int i = 0; i < n_kf; i++) out->kf_state[i] = 0;
    if (out->edge_inlier && no) std::memset(out->edge_inlier, 0, no);
    if (out->points_out) for (size_t i = 0; i < np * 3; i++) out->points_out[i] = NAN;
    if (n_kf == 0 || np == 0 || no == 0) return MO_OK;   // an empty map: nothing runs, not an error
    int rc;
    if ((rc = map_int32_guard(m))) return rc;
    BaBufs& b = map_feature<BaBufs>(m);
    if ((rc = mo_reserve(c, b.loc, np, b.ecnt, np, b.lrank, np, b.ebase, np, b.lpt, np, b.eoff, np + 1, b.pn, np, b.pfix, np, b.X, np * 3, b.Xt, np * 3,
                         b.Vi, np * 6, b.gp, np * 3, b.pc, np, b.pt, np, b.pu, np, b.e_kf, no, b.e_obs, no, b.e_xy, no * 2, b.e_info, no, b.e_inl, no,
                         b.einl, no, b.kf_edge, (size_t)n_kf, b.kf_fidx, (size_t)n_kf, b.poseC, (size_t)n_kf * 12, b.poseT, (size_t)n_kf * 12)))
        return rc;
    if (out->points_out && (rc = mo_reserve(c, b.pout, np * 3))) return rc;
    if ((rc = mo_reserve(c, b.res, b.S, BA_MAX_DIM * BA_MAX_DIM + 2 * BA_MAX_DIM))) return rc;
    BaLocalBufs* lb = lprm ? &map_feature<BaLocalBufs>(m) : nullptr;
    const bool erase = lprm && lprm->erase_outliers != 0;
    if (lb && (rc = mo_reserve(c, lb->cand_in, (size_t)n_kf, lb->cand, (size_t)n_kf, lb->res))) return rc;
    if (erase && ((rc = mo_reserve(c, lb->keep, no, lb->S, no)) || (rc = map_pts_reserve(m, m->cur ^ 1, np, no, false)))) return rc;
    if ((rc = upload_pos_slot(m))) return rc;
    mo_stage_begin(c);
    if (lb) {   // C on the device: the caller's set, or the covisible neighbours of kf_pos selected in this chain
        HIPCHK(c, hipMemsetAsync(lb->res, 0, sizeof(BalRes), c->stream));
        const uint8_t* in = lb->cand_in;
        if (lprm->free_mask) {
            // (from the caller's pageable array, as mo_map_erase_points copies `remove` and mo_map_cull_points `protect`: the runtime stages
            // a pageable source before hipMemcpyAsync returns, so the array is the caller's again on every return path, the error ones too)
            HIPCHK(c, hipMemcpyAsync(lb->cand_in, lprm->free_mask, (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
        } else {
            mo_map_local_params q{};
            q.seed_points = nullptr; q.n_seed = 0; q.ref_pos = lprm->kf_pos; q.n_best = lprm->n_best; q.min_weight = lprm->min_weight;
            if ((rc = covis_enqueue(m)) || (rc = covis_select_enqueue(m, &q))) return rc;
            in = covis_mask(m);
        }
        hipLaunchKernelGGL(k_bal_cand, dim3(1), dim3(BA_BLOCK), 0, c->stream, in, n_kf, lb->cand, lb->res);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(b.poseC, poses, (size_t)n_kf * 96, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.poseT, b.poseC, (size_t)n_kf * 96, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(b.kf_edge, 0, (size_t)n_kf * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(b.einl, 0, no, c->stream));
    BaPrm p;
    for (int i = 0; i < 9; i++) p.K[i] = K[i];
    p.sf = prm->scale_factor; p.chi2 = prm->chi2; p.n_kf = n_kf; p.lo_pos = lo_pos;
    const MapView v = map_view(m);
    const unsigned pblocks = (unsigned)((np + BA_BLOCK - 1) / BA_BLOCK);
    const unsigned wblocks = (unsigned)((std::max(np, no) + BA_BLOCK - 1) / BA_BLOCK);
    double* dcv = b.S + BA_MAX_DIM * BA_MAX_DIM + BA_MAX_DIM;
    hipLaunchKernelGGL(k_ba_init, dim3(1), dim3(64), 0, c->stream, b.res);
    if (lb) hipLaunchKernelGGL(k_ba_mark_set, dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, v, lb->cand, b.loc, b.ecnt, b.kf_edge);
    else hipLaunchKernelGGL(k_ba_mark, dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, v, lo_pos, b.loc, b.ecnt, b.kf_edge);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, b.loc, b.lrank, (int)np, &b.res.p->n_local))) return rc;
    if ((rc = map_scan_excl(m, b.ecnt, b.ebase, (int)np, &b.res.p->n_edges))) return rc;
    if (lb) hipLaunchKernelGGL(k_ba_setup_set, dim3(1), dim3(BA_BLOCK), 0, c->stream, p, lb->cand, b.kf_edge, b.kf_fidx, b.res);
    else hipLaunchKernelGGL(k_ba_setup, dim3(1), dim3(BA_BLOCK), 0, c->stream, p, b.kf_edge, b.kf_fidx, b.res);
    hipLaunchKernelGGL(k_ba_edges, dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, v, m->kkps, p.sf, b.loc, b.lrank, b.ebase, b.lpt, b.eoff, b.X, b.e_kf, b.e_obs,
                       b.e_xy, b.e_info, b.e_inl, b.res);
    hipLaunchKernelGGL(k_ba_cost, dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, p, 0, b.eoff, b.X, b.e_kf, b.e_xy, b.e_info, b.e_inl, b.poseC, b.pc, b.pn, b.res);
    hipLaunchKernelGGL(k_ba_reduce, dim3(1), dim3(1024), 0, c->stream, 0, b.pc, b.pn, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "ba_prep");
    for (int r = 0; r < 2; r++) {
        for (int s = 0; s < prm->max_steps[r]; s++) {
            hipLaunchKernelGGL(k_ba_lin, dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, p, r, b.eoff, b.X, b.e_kf, b.e_xy, b.e_info, b.e_inl, b.poseC, b.Vi, b.gp,
                               b.pfix, b.pc, b.res);
            hipLaunchKernelGGL(k_ba_pair, dim3(BA_MAX_PAIRS), dim3(BA_BLOCK), 0, c->stream, p, r, b.eoff, b.X, b.e_kf, b.e_xy, b.e_info, b.e_inl, b.kf_fidx, b.poseC,
                               b.Vi, b.gp, b.pfix, b.S, b.res);
            hipLaunchKernelGGL(k_ba_solve, dim3(1), dim3(BA_BLOCK), 0, c->stream, r, b.S, dcv, b.poseC, b.poseT, b.res);
            hipLaunchKernelGGL(k_ba_back, dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, p, r, b.eoff, b.X, b.e_kf, b.e_xy, b.e_info, b.e_inl, b.kf_fidx, b.poseC,
                               b.poseT, b.Vi, b.gp, b.pfix, dcv, b.Xt, b.pt, b.pu, b.res);
            hipLaunchKernelGGL(k_ba_accept, dim3(1), dim3(1024), 0, c->stream, r, b.pc, b.pt, b.pu, b.X, b.Xt, b.poseC, b.poseT, b.res);
        }
        hipLaunchKernelGGL(k_ba_cost, dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, p, r + 1, b.eoff, b.X, b.e_kf, b.e_xy, b.e_info, b.e_inl, b.poseC, b.pc, b.pn,
                           b.res);
        hipLaunchKernelGGL(k_ba_reduce, dim3(1), dim3(1024), 0, c->stream, r + 1, b.pc, b.pn, b.res);
        HIPCHK(c, hipGetLastError());
        mo_stage_mark(c, r ? "ba_round1" : "ba_round0");
    }
    hipLaunchKernelGGL(k_ba_write, dim3(wblocks), dim3(BA_BLOCK), 0, c->stream, p, (int)np, (int)no, b.loc, b.lrank, b.X, v.src.xyz,
                       out->points_out ? b.pout.p : nullptr, b.e_obs, b.e_inl, b.einl, m->d_pos_slot, b.poseC, m->kP, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "ba_write");
    if (erase && (rc = oe_enqueue(m, *lb, b.einl, b.res, prm->min_inliers))) return rc;
    std::vector<int32_t> fidx(out->kf_state ? (size_t)n_kf : 0);
    if ((rc = b.res.download(c))) return rc;
    if (lb) {
        if ((rc = lb->res.download(c))) return rc;
        if (lout->candidate) HIPCHK(c, hipMemcpyAsync(lout->candidate, lb->cand, (size_t)n_kf, hipMemcpyDeviceToHost, c->stream));
    }
    if (out->poses_out) HIPCHK(c, hipMemcpyAsync(out->poses_out, b.poseC, (size_t)n_kf * 96, hipMemcpyDeviceToHost, c->stream));
    if (out->edge_inlier) HIPCHK(c, hipMemcpyAsync(out->edge_inlier, b.einl, no, hipMemcpyDeviceToHost, c->stream));
    if (out->points_out) HIPCHK(c, hipMemcpyAsync(out->points_out, b.pout, np * 24, hipMemcpyDeviceToHost, c->stream));
    if (out->kf_state) HIPCHK(c, hipMemcpyAsync(fidx.data(), b.kf_fidx, (size_t)n_kf * 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = map_sync(c, clk))) return rc;
    const BaRes& r = b.res.host();
    if (lb) {
        const BalRes& lr = lb->res.host();
        lout->n_candidates = lr.n_candidates;
        if (erase) { lout->n_erased = oe_finish(m, lr); lout->n_under = lr.n_under; lout->n_obs = m->n_obs; }
    }
    if (!r.run) return MO_OK;   // no free keyframe with an edge, or no local point
    out->n_local = r.n_local;
    for (int i = 0; i < 3; i++) out->cost[i] = r.cost[i];
    out->lambda = r.lambda;
    out->n_free = r.n_free; out->n_fixed = r.n_fixed; out->n_edges = r.n_edges; out->n_inliers = r.n_inliers;
    for (int k = 0; k < 2; k++) { out->steps[k] = r.steps[k]; out->accepted[k] = r.accepted[k]; }
    if (out->kf_state) for (int i = 0; i < n_kf; i++) out->kf_state[i] = fidx[i] >= 0 ? 2 : fidx[i] == BA_KF_FIXED ? 1 : 0;
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

extern "C" int mo_map_erase_observations(mo_map* m, const uint8_t* erase, mo_map_obserase_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!out || (m->n_obs > 0 && !erase)) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    out->n_erased = out->n_under = 0; out->n_obs = m->n_obs;
    if (m->n_pts == 0 || m->n_obs == 0) return MO_OK;
    int rc;
    if ((rc = map_int32_guard(m))) return rc;
    MAP_ENTER(m);
    HostClock clk(c);
    BaLocalBufs& lb = map_feature<BaLocalBufs>(m);
    const size_t np = (size_t)m->n_pts, no = (size_t)m->n_obs;
    if ((rc = mo_reserve(c, lb.flag, no, lb.keep, no, lb.S, no, lb.res)) || (rc = map_pts_reserve(m, m->cur ^ 1, np, no, false))) return rc;
    mo_stage_begin(c);
    HIPCHK(c, hipMemsetAsync(lb.res, 0, sizeof(BalRes), c->stream));
    HIPCHK(c, hipMemcpyAsync(lb.flag, erase, no, hipMemcpyHostToDevice, c->stream));   // (pageable, staged by the runtime: see ba_run)
    mo_stage_mark(c, "obs_flags");   // (the upload apart from the rebuild's stage)
    if ((rc = oe_enqueue(m, lb, lb.flag, nullptr, 0)) || (rc = lb.res.download(c)) || (rc = map_sync(c, clk))) return rc;
    const BalRes& r = lb.res.host();
    out->n_erased = oe_finish(m, r); out->n_under = r.n_under; out->n_obs = m->n_obs;
    return MO_OK;
}

// ---- mo_map_add_observations ------------------------------------------------------------------------------------------------------
// entry i claims its point: the lowest i wins (integer minimum)
__global__ __launch_bounds__(BA_BLOCK) void k_obs_claim(const int32_t* __restrict__ pt, int n, int n_pts, int32_t* __restrict__ claim) {
    const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int p = pt[i];
    if (p >= 0 && p < n_pts) atomicMin(claim + p, i);
}

// one thread per point: a claimed point that has no valid observation in kf_pos yet gains one; cnt = its new observation count
__global__ __launch_bounds__(BA_BLOCK) void k_obs_count(MapView v, int kf_pos, int32_t* __restrict__ claim, int32_t* __restrict__ cnt) {
    const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (i >= v.n_pts) return;
    const int o0 = v.src.off[i], o1 = v.src.off[i + 1];
    bool add = claim[i] != INT_MAX;
    if (add) {
        if (kf_pos == v.n_kf) {   // (the next keyframe's position names nothing yet: its entries are compared as stored)
            for (int o = o0; o < o1 && add; o++) add = v.src.okf[o] != kf_pos;
        } else {
            add = !map_observes(v, i, kf_pos);
        }
        if (!add) claim[i] = INT_MAX;
    }
    cnt[i] = o1 - o0 + add;
}

// every field of every point into the other copy, the observations at their new offsets, the new one behind them
__global__ __launch_bounds__(BA_BLOCK) void k_obs_scatter(MapPts src, MapPts dst, int n_pts, const int32_t* __restrict__ claim, const int32_t* __restrict__ base,
                                                          const int32_t* __restrict__ total, int kf_pos, const int32_t* __restrict__ row,
                                                          int32_t* __restrict__ st) {
    const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (i == 0) { dst.off[n_pts] = *total; st[ST_NPTS] = n_pts; st[ST_NOBS] = *total; }   // (the next call's live counts)
    if (i >= n_pts) return;
    map_point_copy(src, i, dst, i);
    const int o0 = src.off[i], o1 = src.off[i + 1], ob = base[i];
    dst.off[i] = ob;
    for (int o = o0; o < o1; o++) { dst.okf[ob + o - o0] = src.okf[o]; dst.okp[ob + o - o0] = src.okp[o]; }
    const int cl = claim[i];
    if (cl != INT_MAX) { dst.okf[ob + o1 - o0] = kf_pos; dst.okp[ob + o1 - o0] = row[cl]; }
}

extern "C" int mo_map_add_observations(mo_map* m, int kf_pos, int n, const int32_t* point, const int32_t* row) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (n < 0 || (n > 0 && (!point || !row))) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const int n_kf = (int)m->pos_slot.size();
    if (kf_pos < 0 || kf_pos > n_kf) return mo_fail(c, MO_ERR_ARG, "kf_pos must be a keyframe position, or the number of keyframes for the next one");
    if (n == 0 || m->n_pts == 0) return MO_OK;
    if (m->n_pts > INT32_MAX / 2 || m->n_obs + n > INT32_MAX / 2) return mo_fail(c, MO_ERR_CAPACITY, "map larger than int32 indexing");
    MAP_ENTER(m);
    BaBufs& b = map_feature<BaBufs>(m);
    const size_t np = (size_t)m->n_pts;
    int rc;
    if ((rc = mo_reserve(c, b.ao_pt, (size_t)n, b.ao_row, (size_t)n, b.ao_claim, np, b.ao_cnt, np, b.ao_base, np, b.ao_total, 4))) return rc;
    const size_t new_obs = (size_t)m->n_obs + std::min<size_t>((size_t)n, np);
    if ((rc = map_pts_reserve(m, m->cur ^ 1, np, new_obs, false))) return rc;
    if ((rc = upload_pos_slot(m))) return rc;
    HIPCHK(c, hipMemcpyAsync(b.ao_pt, point, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.ao_row, row, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)b.ao_claim, INT_MAX, np, c->stream));
    const MapPts src = m->P[m->cur].view(), dst = m->P[m->cur ^ 1].view();
    const unsigned pblocks = (unsigned)((np + BA_BLOCK - 1) / BA_BLOCK);
    hipLaunchKernelGGL(k_obs_claim, dim3((unsigned)((n + BA_BLOCK - 1) / BA_BLOCK)), dim3(BA_BLOCK), 0, c->stream, b.ao_pt, n, (int)np, b.ao_claim);
    hipLaunchKernelGGL(k_obs_count, dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, map_view(m), kf_pos, b.ao_claim, b.ao_cnt);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, b.ao_cnt, b.ao_base, (int)np, b.ao_total))) return rc;
    hipLaunchKernelGGL(k_obs_scatter, dim3(pblocks), dim3(BA_BLOCK), 0, c->stream, src, dst, (int)np, b.ao_claim, b.ao_base, b.ao_total, kf_pos, b.ao_row, m->st);
    HIPCHK(c, hipGetLastError());
    int32_t total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, b.ao_total, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    m->cur ^= 1;
    m->n_obs = total;
    return MO_OK;
}
