// map_posegraph.hip -- the essential-graph optimisation behind a loop correction on the device map (mo_map_pose_graph in
// include/vslam_amd.h): ORB-SLAM2's Optimizer::OptimizeEssentialGraph, monocular.  The vertices are the keyframe positions as
// similarities, the edges come from the covisibility matrix of the map as it stands, Levenberg-Marquardt on Sim(3) spreads the loop's
// error along the trajectory, and the points follow their reference keyframes.  posegraph.h holds the geometry and the block operations;
// tests/native/posegraph_replay.cpp is this chain on the host over the same header, with the same orders of summation.
//
// Chain (one synchronisation, the copy-out; every decision - too many edges, accept / reject, the end - is a flag in PgRes that the later
// kernels read first):
//   uploads, covis_enqueue (k_covis: W), k_pg_init
//   k_pg_extra     one thread per extra edge: its pair flagged in X [n_kf][n_kf] (plain stores of 1: the racing writers agree)
//   k_pg_parent    one thread per position b: parent[b]
//   k_pg_count     one thread per position: its edges as the lower end (row) and as the upper end (column); two device-wide scans
//   k_pg_gate      one thread: the edge count against the capacity
//   k_pg_scatter   one thread per position a: its edges (a, b) in b order: ends, kind, measurement, and the edge index of the pair
//   k_pg_cols      one thread per position b: the edges (a, b) in a order (ascending edge order): the as-b half of the vertex CSR; the
//                  as-a half is the run rbase[a] .. rbase[a + 1] of the edge arrays themselves
//   per Levenberg-Marquardt step:
//     k_pg_edge    one thread per edge: residual, J_a, J_b, J_a^T J_b, its cost
//     k_pg_vertex  one wavefront per free vertex: H_ii and g_i summed over its CSR entries in order (as-a, then as-b), one lane per
//                  entry of the block; the damped block and its Cholesky factor
//     k_pg_solve   one workgroup of 1024: the preconditioned conjugate gradient, the trial vertices
//     k_pg_trial   one thread per edge: the cost under the trial vertices
//     k_pg_accept  one workgroup of 1024: the two cost sums, accept / reject, lambda, the end flag; an accepted step becomes the state
//   k_pg_write     poses and kP of the free positions, the points, the outputs
// The solver's shape: one workgroup runs a whole solve, its five vectors in LDS while they fit (PG_LDS_VEC_BYTES), in global scratch
// beyond: a solve is one launch, a step five.  profiles/posegraph_rate.txt has the numbers and what was not built.
// No floating-point atomics anywhere: sums are per-thread in index order, then wave_sum, then the waves in order (block_sum of map_store.h;
// pg_tree_sum of posegraph.h is the same order on the host).  Integer atomics only count.  -ffp-contract=off (Makefile).
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "map_store.h"
#include "posegraph.h"

#define PG_BLOCK 256
#define PG_EDGES_PER_KF 32                       // capacity of the edge arrays: this many per keyframe and the extra edges
#define PG_LDS_VEC_BYTES (158 * 1024)            // the five vectors of a solve in LDS (the workgroup's static LDS is below 1 KiB)
static_assert(PG_LDS_VEC_BYTES + 1024 <= 160 * 1024, "one workgroup's LDS");

enum { PG_EXTRA = 0, PG_TREE = 1, PG_COVIS = 2 };

struct PgPrm {
    double K[9], step_tol, cg_tol2;
    int32_t n_kf, n_free, n_extra, min_weight, max_cg, edge_cap, lds_vec;
};

struct PgRes {
    double cost[2], lambda, upd;
    int32_t n_edges, n_extra_used, n_moved, steps, accepted, cg_iters, done, run, overflow;
};

struct PgBufs : MapFeature {
    DevBuf<uint8_t> fixed;                 // [n_kf]
    DevBuf<int32_t> fidx, fpos;            // [n_kf] index among the free positions (-1: fixed), [n_free] its inverse
    DevBuf<int32_t> xa, xb;                // [n_extra]
    DevBuf<uint8_t> X;                     // [n_kf][n_kf] extra pairs, (a, b) with a < b
    DevBuf<int32_t> parent;                // [n_kf]
    DevBuf<int32_t> rcnt, rbase, ccnt, cbase;   // [n_kf + 1] edges per row / column and their first entries
    DevBuf<int32_t> eid;                   // [n_kf][n_kf] edge index of a pair (written at the edges only)
    DevBuf<int32_t> clist;                 // [edge] the as-b lists
    DevBuf<int32_t> ea, eb; DevBuf<uint8_t> ek;   // [edge]
    DevBuf<double> M, r, Ja, Jb, Wab;      // [edge][13], [7], [49] x 3
    DevBuf<double> ec, et;                 // [edge] cost, trial cost
    DevBuf<double> poses, S0, S, St;       // [n_kf][12], [n_kf][13] x 3: initial, current, trial
    DevBuf<double> H, L, g; DevBuf<uint8_t> pfix;   // [n_free][49] x 2, [7], held for the step
    DevBuf<double> vec;                    // [5][7 n_free] the solve's vectors when they do not fit in LDS
    DevBuf<double> pout; DevBuf<uint8_t> moved;    // [n_kf][12], [point]
    ResBlock<PgRes> res;
    // all of it is scratch: every call's chain writes what it reads
    template <class F> void each_scratch(F f) {
        f(fixed); f(fidx); f(fpos); f(xa); f(xb); f(X); f(parent); f(rcnt); f(rbase); f(ccnt); f(cbase); f(eid); f(clist); f(ea); f(eb); f(ek);
        f(M); f(r); f(Ja); f(Jb); f(Wab); f(ec); f(et); f(poses); f(S0); f(S); f(St); f(H); f(L); f(g); f(pfix); f(vec); f(pout); f(moved); f(res);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// the graph as the kernels read it (by value)
struct PgView {
    const uint8_t* fixed; const int32_t* fidx; const int32_t* fpos;
    const uint8_t* X; const int32_t* parent; const int32_t* W;
    const int32_t* rbase; const int32_t* cbase; const int32_t* clist;
    const int32_t* ea; const int32_t* eb;
};

__global__ void k_pg_init(PgRes* __restrict__ res) {
    if (threadIdx.x) return;
    res->cost[0] = res->cost[1] = 0.0; res->lambda = 1e-4; res->upd = 0.0;
    res->n_edges = 0; res->n_extra_used = 0; res->n_moved = 0; res->steps = 0; res->accepted = 0; res->cg_iters = 0;
    res->done = 0; res->run = 0; res->overflow = 0;
}

__global__ __launch_bounds__(PG_BLOCK) void k_pg_extra(int n_extra, int n_kf, const int32_t* __restrict__ xa, const int32_t* __restrict__ xb,
                                                        uint8_t* __restrict__ X) {
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (i >= n_extra) return;
    const int a = min(xa[i], xb[i]), b = max(xa[i], xb[i]);
    X[(size_t)a * n_kf + b] = 1;
}

// parent[b]: the position a < b of the largest weight, ties to the lowest; b - 1 when that weight is 0
__global__ __launch_bounds__(PG_BLOCK) void k_pg_parent(int n_kf, const int32_t* __restrict__ W, int32_t* __restrict__ parent) {
    const int b = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (b >= n_kf) return;
    int best = 0, at = b - 1;
    for (int a = 0; a < b; a++) {
        const int w = W[(size_t)a * n_kf + b];
        if (w > best) { best = w; at = a; }
    }
    parent[b] = at;   // (-1 at position 0)
}

// the kind of the pair (a, b), a < b; -1: no edge
__device__ __forceinline__ int pg_kind(const PgView& v, int n_kf, int min_weight, int a, int b) {
    if (v.fixed[a] && v.fixed[b]) return -1;
    if (v.X[(size_t)a * n_kf + b]) return PG_EXTRA;
    if (v.parent[b] == a) return PG_TREE;
    return v.W[(size_t)a * n_kf + b] >= min_weight ? PG_COVIS : -1;
}

__global__ __launch_bounds__(PG_BLOCK) void k_pg_count(PgPrm prm, PgView v, int32_t* __restrict__ rcnt, int32_t* __restrict__ ccnt) {
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (i >= prm.n_kf) return;
    int nr = 0, nc = 0;
    for (int a = 0; a < i; a++) nc += pg_kind(v, prm.n_kf, prm.min_weight, a, i) >= 0;
    for (int b = i + 1; b < prm.n_kf; b++) nr += pg_kind(v, prm.n_kf, prm.min_weight, i, b) >= 0;
    rcnt[i] = nr; ccnt[i] = nc;
}

__global__ void k_pg_gate(PgPrm prm, int32_t* __restrict__ rbase, int32_t* __restrict__ cbase, PgRes* __restrict__ res) {
    if (threadIdx.x) return;
    const int ne = res->n_edges;
    rbase[prm.n_kf] = ne; cbase[prm.n_kf] = ne;
    res->overflow = ne > prm.edge_cap;
    res->run = ne > 0 && ne <= prm.edge_cap;
}

__global__ __launch_bounds__(PG_BLOCK) void k_pg_scatter(PgPrm prm, PgView v, const double* __restrict__ poses, const double* __restrict__ S0,
                                                          int32_t* __restrict__ ea, int32_t* __restrict__ eb, uint8_t* __restrict__ ek,
                                                          int32_t* __restrict__ eid, double* __restrict__ M, PgRes* __restrict__ res) {
    if (!res->run) return;
    const int a = blockIdx.x * PG_BLOCK + threadIdx.x;
    int nx = 0;
    if (a < prm.n_kf) {
        int e = v.rbase[a];
        for (int b = a + 1; b < prm.n_kf; b++) {
            const int kind = pg_kind(v, prm.n_kf, prm.min_weight, a, b);
            if (kind < 0) continue;
            Sim3 Sa, Sb, Me;
            if (kind == PG_EXTRA) {
                pg_load(S0 + (size_t)a * 13, Sa); pg_load(S0 + (size_t)b * 13, Sb);
                nx++;
            } else {
                Sa.s = 1.0; Sb.s = 1.0;
                pose_split(poses + (size_t)a * 12, Sa.R, Sa.t); pose_split(poses + (size_t)b * 12, Sb.R, Sb.t);
            }
            pg_measure(Sa, Sb, Me);
            pg_store(Me, M + (size_t)e * 13);
            ea[e] = a; eb[e] = b; ek[e] = (uint8_t)kind; eid[(size_t)a * prm.n_kf + b] = e;
            e++;
        }
    }
    nx = wave_sum_int(nx);
    if ((threadIdx.x & 63) == 0 && nx) atomicAdd(&res->n_extra_used, nx);
}

__global__ __launch_bounds__(PG_BLOCK) void k_pg_cols(PgPrm prm, PgView v, const int32_t* __restrict__ eid, int32_t* __restrict__ clist,
                                                       const PgRes* __restrict__ res) {
    if (!res->run) return;
    const int b = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (b >= prm.n_kf) return;
    int c = v.cbase[b];
    for (int a = 0; a < b; a++)
        if (pg_kind(v, prm.n_kf, prm.min_weight, a, b) >= 0) clist[c++] = eid[(size_t)a * prm.n_kf + b];
}

__device__ __forceinline__ bool pg_active(const PgRes* res) { return res->run && !res->done; }

__global__ __launch_bounds__(PG_BLOCK) void k_pg_edge(PgView v, const double* __restrict__ M, const double* __restrict__ S, double* __restrict__ r,
                                                       double* __restrict__ Ja, double* __restrict__ Jb, double* __restrict__ Wab,
                                                       double* __restrict__ ec, const PgRes* __restrict__ res) {
    if (!pg_active(res)) return;
    const int e = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (e >= res->n_edges) return;
    Sim3 Me, Sa, Sb;
    pg_load(M + (size_t)e * 13, Me); pg_load(S + (size_t)v.ea[e] * 13, Sa); pg_load(S + (size_t)v.eb[e] * 13, Sb);
    double re[7], A[49], B[49];
    pg_linearize(Me, Sa, Sb, re, A, B);
    for (int k = 0; k < 7; k++) r[(size_t)e * 7 + k] = re[k];
    for (int k = 0; k < 49; k++) { Ja[(size_t)e * 49 + k] = A[k]; Jb[(size_t)e * 49 + k] = B[k]; }
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) Wab[(size_t)e * 49 + i * 7 + j] = pg_atb_entry(A, B, i, j);
    ec[e] = pg_cost(re);
}

// one wavefront per free vertex: lanes 0 .. 48 an entry of H_ii, lanes 49 .. 55 an entry of g_i
__global__ __launch_bounds__(64) void k_pg_vertex(PgView v, const double* __restrict__ r, const double* __restrict__ Ja, const double* __restrict__ Jb,
                                                   double* __restrict__ H, double* __restrict__ L, double* __restrict__ g, uint8_t* __restrict__ pfix,
                                                   const PgRes* __restrict__ res) {
    __shared__ double Hs[49];
    if (!pg_active(res)) return;
    const int f = blockIdx.x, pos = v.fpos[f], k = threadIdx.x;
    const int a0 = v.rbase[pos], a1 = v.rbase[pos + 1], c0 = v.cbase[pos], c1 = v.cbase[pos + 1];
    double s = 0.0;
    if (k < 49) {
        const int i = k / 7, j = k - i * 7;
        for (int e = a0; e < a1; e++) s += pg_atb_entry(Ja + (size_t)e * 49, Ja + (size_t)e * 49, i, j);
        for (int c = c0; c < c1; c++) { const size_t e = (size_t)v.clist[c]; s += pg_atb_entry(Jb + e * 49, Jb + e * 49, i, j); }
        Hs[k] = s;
    } else if (k < 56) {
        const int i = k - 49;
        for (int e = a0; e < a1; e++) s += pg_atr_entry(Ja + (size_t)e * 49, r + (size_t)e * 7, i);
        for (int c = c0; c < c1; c++) { const size_t e = (size_t)v.clist[c]; s += pg_atr_entry(Jb + e * 49, r + e * 7, i); }
        g[(size_t)f * 7 + i] = s;
    }
    __syncthreads();
    const double damp = 1.0 + res->lambda;
    if (k < 49) H[(size_t)f * 49 + k] = (k % 8 == 0) ? Hs[k] * damp : Hs[k];
    if (k == 0) {
        double Lf[49];
        const bool ok = pg_chol7(Hs, damp, Lf);
        for (int i = 0; i < 49; i++) L[(size_t)f * 49 + i] = Lf[i];
        pfix[f] = !ok;
    }
}

// z = the preconditioner on r: per free vertex the Cholesky solve of its damped block; 0 at a vertex held for the step
__device__ __forceinline__ void pg_precond(int nf, const double* __restrict__ L, const uint8_t* __restrict__ pfix, const double* r, double* z) {
    for (int f = threadIdx.x; f < nf; f += blockDim.x) {
        double b[7], x[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 7; k++) b[k] = r[f * 7 + k];
        if (!pfix[f]) pg_chol7_solve(L + (size_t)f * 49, b, x);
        for (int k = 0; k < 7; k++) z[f * 7 + k] = x[k];
    }
}

// q = A p, one thread per scalar row: the vertex's damped block, its as-a edges (W p_b), its as-b edges (W^T p_a), in CSR order
__device__ __forceinline__ void pg_matvec(const PgView& v, int nf, const double* __restrict__ H, const double* __restrict__ Wab, const double* p, double* q) {
    for (int j = threadIdx.x; j < 7 * nf; j += blockDim.x) {
        const int f = j / 7, k = j - f * 7, pos = v.fpos[f];
        double s = pg_mulv_entry(H + (size_t)f * 49, p + f * 7, k, false);
        for (int e = v.rbase[pos]; e < v.rbase[pos + 1]; e++) {
            const int fb = v.fidx[v.eb[e]];
            if (fb >= 0) s += pg_mulv_entry(Wab + (size_t)e * 49, p + fb * 7, k, false);
        }
        for (int c = v.cbase[pos]; c < v.cbase[pos + 1]; c++) {
            const int e = v.clist[c], fa = v.fidx[v.ea[e]];
            if (fa >= 0) s += pg_mulv_entry(Wab + (size_t)e * 49, p + fa * 7, k, true);
        }
        q[j] = s;
    }
}

__device__ __forceinline__ double pg_dot(int n, const double* a, const double* b, double* lds) {
    double s = 0.0;
    for (int j = threadIdx.x; j < n; j += blockDim.x) s += a[j] * b[j];
    return block_sum(s, lds);
}

// one workgroup: (H + lambda diag H) x = -g by preconditioned conjugate gradient from x = 0, then the trial vertices D(x_i) o S_i
__global__ __launch_bounds__(PG_THREADS) void k_pg_solve(PgPrm prm, PgView v, const double* __restrict__ H, const double* __restrict__ L,
                                                          const double* __restrict__ g, const uint8_t* __restrict__ pfix, const double* __restrict__ Wab,
                                                          double* __restrict__ gvec, const double* __restrict__ S, double* __restrict__ St,
                                                          PgRes* __restrict__ res) {
    extern __shared__ __attribute__((aligned(16))) double pg_lds[];
    __shared__ double red[PG_THREADS / 64];
    if (!pg_active(res)) return;
    const int nf = prm.n_free, n = 7 * nf, tid = threadIdx.x;
    double* x = prm.lds_vec ? pg_lds : gvec;
    double *r = x + n, *z = r + n, *p = z + n, *q = p + n;
    for (int j = tid; j < n; j += PG_THREADS) { x[j] = 0.0; r[j] = -g[j]; }
    __syncthreads();
    pg_precond(nf, L, pfix, r, z);
    __syncthreads();
    for (int j = tid; j < n; j += PG_THREADS) p[j] = z[j];
    double rz = pg_dot(n, r, z, red);
    const double rz0 = rz;
    int it = 0;
    if (rz0 > 0.0 && isfinite(rz0)) {
        while (it < prm.max_cg) {
            pg_matvec(v, nf, H, Wab, p, q);
            __syncthreads();
            const double pq = pg_dot(n, p, q, red);
            if (!(pq > 0.0) || !isfinite(pq)) break;
            const double alpha = rz / pq;
            for (int j = tid; j < n; j += PG_THREADS) { x[j] += alpha * p[j]; r[j] -= alpha * q[j]; }
            __syncthreads();
            pg_precond(nf, L, pfix, r, z);
            __syncthreads();
            const double rzn = pg_dot(n, r, z, red);
            it++;
            if (!(rzn > prm.cg_tol2 * rz0)) break;
            const double beta = rzn / rz;
            for (int j = tid; j < n; j += PG_THREADS) p[j] = z[j] + beta * p[j];
            rz = rzn;
            __syncthreads();
        }
    }
    __syncthreads();
    double mu = 0.0;
    for (int f = tid; f < nf; f += PG_THREADS) {
        const int pos = v.fpos[f];
        double d[7];
        for (int k = 0; k < 7; k++) d[k] = x[f * 7 + k];
        Sim3 Sc, T;
        pg_load(S + (size_t)pos * 13, Sc);
        pg_retract(d, Sc, T);
        if (sim3_finite(T) && T.s > 0.0) {   // (a vertex whose step is not a similarity stays)
            pg_store(T, St + (size_t)pos * 13);
            for (int k = 0; k < 7; k++) mu = fmax(mu, fabs(d[k]));
        }
    }
    mu = block_max(mu, red);
    if (tid == 0) { res->upd = mu; res->cg_iters += it; }
}

__global__ __launch_bounds__(PG_BLOCK) void k_pg_trial(PgView v, const double* __restrict__ M, const double* __restrict__ St, double* __restrict__ et,
                                                        const PgRes* __restrict__ res) {
    if (!pg_active(res)) return;
    const int e = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (e >= res->n_edges) return;
    Sim3 Me, Sa, Sb;
    pg_load(M + (size_t)e * 13, Me); pg_load(St + (size_t)v.ea[e] * 13, Sa); pg_load(St + (size_t)v.eb[e] * 13, Sb);
    double re[7];
    pg_residual(Me, Sa, Sb, re);
    et[e] = pg_cost(re);
}

// one workgroup: current and trial cost; accept (the trial becomes the state, lambda / 10) or reject (lambda * 10); the end at an update
// below step_tol or lambda above 1e8
__global__ __launch_bounds__(PG_THREADS) void k_pg_accept(PgPrm prm, const double* __restrict__ ec, const double* __restrict__ et, double* __restrict__ S,
                                                           double* __restrict__ St, PgRes* __restrict__ res) {
    __shared__ double red[PG_THREADS / 64];
    __shared__ int acc;
    if (!pg_active(res)) return;
    const int ne = res->n_edges, tid = threadIdx.x;
    double c0 = 0.0, c1 = 0.0;
    for (int e = tid; e < ne; e += PG_THREADS) { c0 += ec[e]; c1 += et[e]; }
    c0 = block_sum(c0, red);
    c1 = block_sum(c1, red);
    if (tid == 0) {
        const bool ok = c1 < c0;
        acc = ok;
        const double lam = ok ? res->lambda / 10.0 : res->lambda * 10.0;
        if (res->steps == 0) res->cost[0] = c0;
        res->cost[1] = ok ? c1 : c0;
        res->lambda = lam;
        res->steps++;
        res->accepted += ok;
        if (res->upd < prm.step_tol || lam > 1e8) res->done = 1;
    }
    __syncthreads();
    const int n = prm.n_kf * 13;
    if (acc) { for (int k = tid; k < n; k += PG_THREADS) S[k] = St[k]; }
    else { for (int k = tid; k < n; k += PG_THREADS) St[k] = S[k]; }
}

// poses_out of every position; with an accepted step the map follows: kP of the free positions, the points of a free reference
__global__ __launch_bounds__(PG_BLOCK) void k_pg_write(PgPrm prm, MapView v, PgView g, const double* __restrict__ S0, const double* __restrict__ S,
                                                        double* __restrict__ pout, double* __restrict__ kP, uint8_t* __restrict__ moved,
                                                        PgRes* __restrict__ res) {
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    const bool write = res->accepted > 0;
    if (i < prm.n_kf) {
        Sim3 Sc;
        pg_load(S + (size_t)i * 13, Sc);
        const double t[3] = {Sc.t[0] / Sc.s, Sc.t[1] / Sc.s, Sc.t[2] / Sc.s};
        for (int j = 0; j < 3; j++) {
            for (int l = 0; l < 3; l++) pout[(size_t)i * 12 + j * 4 + l] = Sc.R[j * 3 + l];
            pout[(size_t)i * 12 + j * 4 + 3] = t[j];
        }
        if (write && !g.fixed[i]) {
            double P[12];
            pnp_projection(prm.K, Sc.R, t, P);
            for (int k = 0; k < 12; k++) kP[(size_t)v.pos_slot[i] * 12 + k] = P[k];
        }
    }
    bool mv = false;
    if (i < v.n_pts) {
        int ref = -1;
        map_each_obs(v, i, [&](int, int pos, int, int) { ref = pos; return true; });
        mv = write && ref >= 0 && !g.fixed[ref];
        if (mv) {
            Sim3 A, B, Bi;
            pg_load(S0 + (size_t)ref * 13, A); pg_load(S + (size_t)ref * 13, B);
            sim3_inverse(B, Bi);
            float* x = v.src.xyz + (size_t)i * 3;
            const double X[3] = {(double)x[0], (double)x[1], (double)x[2]};
            double Y[3], Z[3];
            sim3_apply(A, X, Y);
            sim3_apply(Bi, Y, Z);
            for (int d = 0; d < 3; d++) x[d] = (float)Z[d];
        }
        moved[i] = mv;
    }
    wave_count_add(mv, &res->n_moved);
}

extern "C" int mo_map_pose_graph(mo_map* m, const double* poses, const double* init, const mo_map_pg_params* prm, mo_map_pg_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const int n_kf = (int)m->pos_slot.size();
    if (n_kf > 0 && (!poses || !init || !prm->fixed)) return mo_fail(c, MO_ERR_ARG, "poses, init or fixed is NULL");
    if (prm->n_extra < 0 || (prm->n_extra > 0 && (!prm->extra_a || !prm->extra_b))) return mo_fail(c, MO_ERR_ARG, "n_extra extra edges need extra_a and extra_b");
    if (prm->max_steps < 0 || prm->max_steps > 100) return mo_fail(c, MO_ERR_ARG, "max_steps must be in 0 .. 100");
    if (prm->max_cg < 1) return mo_fail(c, MO_ERR_ARG, "max_cg must be >= 1");
    if (!(prm->cg_tol >= 0.0) || !std::isfinite(prm->cg_tol) || !(prm->step_tol >= 0.0) || !std::isfinite(prm->step_tol))
        return mo_fail(c, MO_ERR_ARG, "cg_tol and step_tol must be finite and >= 0");
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(prm->K[i])) return mo_fail(c, MO_ERR_ARG, "K must be finite");
    for (size_t i = 0; i < (size_t)n_kf * 12; i++)
        if (!std::isfinite(poses[i])) return mo_fail(c, MO_ERR_ARG, "poses must be finite");
    for (size_t i = 0; i < (size_t)n_kf * 13; i++)
        if (!std::isfinite(init[i])) return mo_fail(c, MO_ERR_ARG, "init must be finite");
    for (int i = 0; i < n_kf; i++)
        if (!(init[(size_t)i * 13] > 0.0)) return mo_fail(c, MO_ERR_ARG, "a scale of init is not > 0");
    for (int i = 0; i < prm->n_extra; i++) {
        const int a = prm->extra_a[i], b = prm->extra_b[i];
        if (a < 0 || a >= n_kf || b < 0 || b >= n_kf || a == b) return mo_fail(c, MO_ERR_ARG, "an extra edge must join two different keyframe positions");
    }
    std::vector<uint8_t> fixed((size_t)n_kf);
    std::vector<int32_t> fidx((size_t)n_kf), fpos;
    for (int i = 0; i < n_kf; i++) {
        fixed[i] = prm->fixed[i] != 0;
        fidx[i] = fixed[i] ? -1 : (int32_t)fpos.size();
        if (!fixed[i]) fpos.push_back(i);
    }
    const int nf = (int)fpos.size();
    if (n_kf > 0 && nf == n_kf) return mo_fail(c, MO_ERR_ARG, "no position is fixed");
    out->cost[0] = out->cost[1] = 0.0; out->lambda = 0.0;
    out->steps = out->accepted = out->cg_iters = out->n_free = out->n_fixed = out->n_edges = out->n_extra_used = out->n_moved = out->ok = 0;
    if (n_kf < 2 || nf == 0) return MO_OK;   // (an empty map, one keyframe, no free vertex: nothing runs, nothing is written)
    const size_t nk = (size_t)n_kf, np = (size_t)m->n_pts, nx = (size_t)prm->n_extra;
    if (nk * nk > (size_t)INT32_MAX) return mo_fail(c, MO_ERR_CAPACITY, "map larger than int32 indexing");
    int rc;
    if ((rc = map_int32_guard(m))) return rc;
    const size_t cap = std::min(nk * (nk - 1) / 2, nk * PG_EDGES_PER_KF + nx);
    MAP_ENTER(m);
    HostClock clk(c);
    PgBufs& b = map_feature<PgBufs>(m);
    const size_t nv = 7 * (size_t)nf;
    const bool lds_vec = 5 * nv * 8 <= PG_LDS_VEC_BYTES;
    if ((rc = mo_reserve(c, b.fixed, nk, b.fidx, nk, b.fpos, (size_t)nf, b.xa, std::max(nx, (size_t)1), b.xb, std::max(nx, (size_t)1), b.X, nk * nk, b.parent, nk,
                         b.rcnt, nk + 1, b.rbase, nk + 1, b.ccnt, nk + 1, b.cbase, nk + 1, b.eid, nk * nk, b.clist, cap, b.ea, cap, b.eb, cap, b.ek, cap,
                         b.M, cap * 13, b.r, cap * 7, b.Ja, cap * 49, b.Jb, cap * 49, b.Wab, cap * 49, b.ec, cap, b.et, cap, b.poses, nk * 12, b.S0, nk * 13,
                         b.S, nk * 13, b.St, nk * 13, b.H, (size_t)nf * 49, b.L, (size_t)nf * 49, b.g, nv, b.pfix, (size_t)nf, b.vec, 5 * nv, b.pout, nk * 12,
                         b.moved, std::max(np, (size_t)1), b.res)))
        return rc;
    if ((rc = upload_pos_slot(m))) return rc;
    if (lds_vec && (rc = mo_raise_dyn_lds(c, (const void*)k_pg_solve, PG_LDS_VEC_BYTES))) return rc;
    mo_stage_begin(c);
    HIPCHK(c, hipMemcpyAsync(b.fixed, fixed.data(), nk, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.fidx, fidx.data(), nk * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.fpos, fpos.data(), (size_t)nf * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.poses, poses, nk * 96, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.S0, init, nk * 104, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.S, b.S0, nk * 104, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.St, b.S0, nk * 104, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(b.X, 0, nk * nk, c->stream));
    if (nx) {
        HIPCHK(c, hipMemcpyAsync(b.xa, prm->extra_a, nx * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b.xb, prm->extra_b, nx * 4, hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = covis_enqueue(m))) return rc;
    PgPrm g;
    std::memset(&g, 0, sizeof(g));
    for (int i = 0; i < 9; i++) g.K[i] = prm->K[i];
    g.step_tol = prm->step_tol; g.cg_tol2 = prm->cg_tol * prm->cg_tol;
    g.n_kf = n_kf; g.n_free = nf; g.n_extra = prm->n_extra; g.min_weight = std::max(prm->min_weight, 1); g.max_cg = prm->max_cg;
    g.edge_cap = (int32_t)cap; g.lds_vec = lds_vec;
    const PgView v{b.fixed, b.fidx, b.fpos, b.X, b.parent, covis_weights(m), b.rbase, b.cbase, b.clist, b.ea, b.eb};
    const MapView mv = map_view(m);
    const unsigned kblocks = (unsigned)((nk + PG_BLOCK - 1) / PG_BLOCK), eblocks = (unsigned)((cap + PG_BLOCK - 1) / PG_BLOCK);
    hipLaunchKernelGGL(k_pg_init, dim3(1), dim3(64), 0, c->stream, b.res);
    if (nx) hipLaunchKernelGGL(k_pg_extra, dim3((unsigned)((nx + PG_BLOCK - 1) / PG_BLOCK)), dim3(PG_BLOCK), 0, c->stream, (int)nx, n_kf, b.xa, b.xb, b.X);
    hipLaunchKernelGGL(k_pg_parent, dim3(kblocks), dim3(PG_BLOCK), 0, c->stream, n_kf, v.W, b.parent);
    hipLaunchKernelGGL(k_pg_count, dim3(kblocks), dim3(PG_BLOCK), 0, c->stream, g, v, b.rcnt, b.ccnt);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, b.rcnt, b.rbase, n_kf, &b.res.p->n_edges)) || (rc = map_scan_excl(m, b.ccnt, b.cbase, n_kf, b.ccnt + n_kf))) return rc;
    hipLaunchKernelGGL(k_pg_gate, dim3(1), dim3(64), 0, c->stream, g, b.rbase, b.cbase, b.res);
    hipLaunchKernelGGL(k_pg_scatter, dim3(kblocks), dim3(PG_BLOCK), 0, c->stream, g, v, b.poses, b.S0, b.ea, b.eb, b.ek, b.eid, b.M, b.res);
    hipLaunchKernelGGL(k_pg_cols, dim3(kblocks), dim3(PG_BLOCK), 0, c->stream, g, v, b.eid, b.clist, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "pg_edges");
    for (int s = 0; s < prm->max_steps; s++) {
        hipLaunchKernelGGL(k_pg_edge, dim3(eblocks), dim3(PG_BLOCK), 0, c->stream, v, b.M, b.S, b.r, b.Ja, b.Jb, b.Wab, b.ec, b.res);
        hipLaunchKernelGGL(k_pg_vertex, dim3((unsigned)nf), dim3(64), 0, c->stream, v, b.r, b.Ja, b.Jb, b.H, b.L, b.g, b.pfix, b.res);
        hipLaunchKernelGGL(k_pg_solve, dim3(1), dim3(PG_THREADS), lds_vec ? 5 * nv * 8 : 0, c->stream, g, v, b.H, b.L, b.g, b.pfix, b.Wab, b.vec, b.S, b.St,
                           b.res);
        hipLaunchKernelGGL(k_pg_trial, dim3(eblocks), dim3(PG_BLOCK), 0, c->stream, v, b.M, b.St, b.et, b.res);
        hipLaunchKernelGGL(k_pg_accept, dim3(1), dim3(PG_THREADS), 0, c->stream, g, b.ec, b.et, b.S, b.St, b.res);
        HIPCHK(c, hipGetLastError());
    }
    mo_stage_mark(c, "pg_solve");
    hipLaunchKernelGGL(k_pg_write, dim3((unsigned)((std::max(nk, np) + PG_BLOCK - 1) / PG_BLOCK)), dim3(PG_BLOCK), 0, c->stream, g, mv, v, b.S0, b.S, b.pout, m->kP,
                       b.moved, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "pg_write");
    if ((rc = b.res.download(c))) return rc;
    const size_t ecopy = out->edge_cap > 0 ? std::min((size_t)out->edge_cap, cap) : 0;
    std::vector<int32_t> h_ea(out->edge_a ? ecopy : 0), h_eb(out->edge_b ? ecopy : 0);
    std::vector<uint8_t> h_ek(out->edge_kind ? ecopy : 0), h_moved(out->moved ? np : 0);
    std::vector<double> h_pout(out->poses_out ? nk * 12 : 0), h_S(out->sim3_out ? nk * 13 : 0);
    if (!h_ea.empty()) HIPCHK(c, hipMemcpyAsync(h_ea.data(), b.ea, ecopy * 4, hipMemcpyDeviceToHost, c->stream));
    if (!h_eb.empty()) HIPCHK(c, hipMemcpyAsync(h_eb.data(), b.eb, ecopy * 4, hipMemcpyDeviceToHost, c->stream));
    if (!h_ek.empty()) HIPCHK(c, hipMemcpyAsync(h_ek.data(), b.ek, ecopy, hipMemcpyDeviceToHost, c->stream));
    if (!h_moved.empty()) HIPCHK(c, hipMemcpyAsync(h_moved.data(), b.moved, np, hipMemcpyDeviceToHost, c->stream));
    if (!h_pout.empty()) HIPCHK(c, hipMemcpyAsync(h_pout.data(), b.pout, nk * 96, hipMemcpyDeviceToHost, c->stream));
    if (!h_S.empty()) HIPCHK(c, hipMemcpyAsync(h_S.data(), b.S, nk * 104, hipMemcpyDeviceToHost, c->stream));
    if ((rc = map_sync(c, clk))) return rc;
    const PgRes& r = b.res.host();
    if (r.overflow) return mo_fail(c, MO_ERR_CAPACITY, "more edges than 32 per keyframe and the extra ones: raise min_weight");
    out->n_free = nf; out->n_fixed = n_kf - nf; out->n_edges = r.n_edges; out->n_extra_used = r.n_extra_used;
    const size_t ne = std::min((size_t)r.n_edges, ecopy);   // (the entries behind n_edges were never written)
    if (!h_ea.empty()) std::memcpy(out->edge_a, h_ea.data(), ne * 4);
    if (!h_eb.empty()) std::memcpy(out->edge_b, h_eb.data(), ne * 4);
    if (!h_ek.empty()) std::memcpy(out->edge_kind, h_ek.data(), ne);
    if (!h_moved.empty()) std::memcpy(out->moved, h_moved.data(), np);
    if (!h_pout.empty()) std::memcpy(out->poses_out, h_pout.data(), nk * 96);
    if (!h_S.empty()) std::memcpy(out->sim3_out, h_S.data(), nk * 104);
    out->cost[0] = r.cost[0]; out->cost[1] = r.cost[1]; out->lambda = r.lambda;
    out->steps = r.steps; out->accepted = r.accepted; out->cg_iters = r.cg_iters; out->n_moved = r.n_moved;
    out->ok = r.accepted > 0;
    return MO_OK;
}
