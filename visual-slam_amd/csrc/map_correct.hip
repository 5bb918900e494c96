// map_correct.hip -- the correction of a confirmed loop on the device map (mo_map_loop_correct in include/vslam_amd.h): the first half of
// ORB-SLAM2's LoopClosing::CorrectLoop.  The similarity mo_map_loop_confirm refined is carried to the asking keyframe's neighbourhood
// (one transform A of the map frame, formed on the host in f64), the neighbourhood's points and poses move, and the loop side's points
// replace and absorb the duplicates the neighbourhood holds (SearchAndFuse): confirm's loop_point rows directly, every other loop point
// by mo_map_fuse's search under the corrected projections.  Writes the fused map into the other copy of the store.
//
// Chain (one synchronisation, the copy-out; every kernel behind the resolve reads CrView::any(res) first and returns when nothing fuses):
//   uploads, fills, k_trk_rep over the group's keyframes (trk_launch_rep_mask: the loop points and their representatives)
//   k_cr_move      one thread per point: point_of of every keyframe (map_point_of), valid observations, the moved flag, A (X, 1) written
//                  over xyz of the moved points in the live copy, union-find and survivor tables reset; threads below the corrected count
//                  write kP = K [R' | t' / s] of their keyframe
//   k_trk_grid     one block per corrected keyframe (trk_launch_grid)
//   k_cr_direct    one thread per row of p: the row's loop point against the row's owner: a merge edge, or the point's claim on the free
//                  row (atomicMin of the row per point: the lower row wins)
//   k_merge_search one thread per (point, corrected keyframe): the pair's proposal (map_merge.h)
//   merge_enqueue  resolve, flatten, members, count, scatter: the merge stages of map_merge.h, which mo_map_fuse runs too
// This file is the loop's view of those stages (CrView): target t is the keyframe at position cpos[t]; a row of p that k_cr_direct gave
// to a loop point is owned by it; a component's survivor is a loop point first (then the most valid observations, then the lowest
// index); a member's direct gain stands ahead of its searched gains; and a direct edge or gain makes the call fuse as a proposal does.
// Integer atomics only: equal inputs give equal bytes.  -ffp-contract=off (Makefile): tests/correct_restatement.py rounds as this file does.
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"
#include "map_store.h"
#include "map_search.h"
#include "map_merge.h"
#include "pnp.h"   // pnp_projection

#define CR_BLOCK MG_BLOCK

struct CrPrm {
    double K[9], A[12];
    double radius, sf, chi2;
    int32_t w, h, max_dist, p, n_p, nt;
};

struct CrRes {
    int32_t n_loop_points, n_moved, n_direct_edges, n_direct_gained, n_pairs, n_cand, n_proposals, n_gained, n_edges, n_absorbed;
    int32_t n_points, n_obs, n_members;
};

struct CorrectBufs : MapFeature {
    DevBuf<uint8_t> cmask, gmask;         // [n_kf] the corrected keyframes, the group
    DevBuf<int32_t> cpos, slots;          // [target] position (ascending) and slot of every corrected keyframe
    DevBuf<double> pose;                  // [target][12] the corrected [R' | t' / s]
    DevBuf<int32_t> lp;                   // [rows of p] loop_point
    MergeBufs mg;                         // (oct: TK_NOT_LOCAL is "no loop point")
    DevBuf<int32_t> tab;                  // [position][row] point_of (INT_MAX: a free row)
    DevBuf<int32_t> drow;                 // [point] the row of p rule 4 gives the point (INT_MAX: none)
    DevBuf<uint8_t> moved;                // [point]
    ResBlock<CrRes> res;
    // all of it is scratch: every call's chain writes what it reads
    template <class F> void each_scratch(F f) {
        f(cmask); f(gmask); f(cpos); f(slots); f(pose); f(lp); mg.each_scratch(f); f(tab); f(drow); f(moved); f(res);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// what the kernels read (by value): the map, the call's own tables, and the loop's answers to what the merge stages ask
struct CrView {
    MapView map;
    const int32_t* cpos; const int32_t* lp; const int32_t* drow;
    const int32_t* prop; const unsigned long long* key; const int32_t* tab;
    int p, n_targets;
    __device__ __forceinline__ int pos_of(int t) const { return cpos[t]; }
    // point_of, else the loop point rule 4 gave the row to, else INT_MAX
    __device__ __forceinline__ int owner(int t, int r) const {
        const int pos = cpos[t], o = tab[(size_t)pos * map.row + r];
        if (o != INT_MAX || pos != p) return o;
        const int L = lp[r];
        return L >= 0 && L < map.n_pts && drow[L] == r ? L : INT_MAX;
    }
    // a loop point first, then the most observations, then the lowest index
    __device__ static __forceinline__ unsigned long long surv_key(int i, int nval, int oct) {
        const unsigned long long other = oct == TK_NOT_LOCAL ? 1ull : 0ull;
        return (other << 63) | ((unsigned long long)(0x7fffffffu - (unsigned)nval) << 32) | (unsigned)i;
    }
    __device__ __forceinline__ bool direct(int j, int* pos, int* r) const {
        *pos = p; *r = drow[j];
        return *r != INT_MAX;
    }
    __host__ __device__ static bool any(const CrRes* r) { return r->n_proposals || r->n_direct_edges || r->n_direct_gained; }
};

// one thread per point: point_of, valid observations, the move, the tables of the later kernels reset; kP of the corrected keyframes
__global__ __launch_bounds__(CR_BLOCK) void k_cr_move(MapView v, CrPrm prm, const uint8_t* __restrict__ cmask, const uint8_t* __restrict__ gmask,
                                                       const int32_t* __restrict__ slots, const double* __restrict__ pose, double* __restrict__ kP,
                                                       int32_t* __restrict__ tab, int32_t* __restrict__ nval, int32_t* __restrict__ parent,
                                                       int32_t* __restrict__ mcnt, int32_t* __restrict__ mcur, unsigned long long* __restrict__ surv,
                                                       int32_t* __restrict__ drow, uint8_t* __restrict__ moved, CrRes* __restrict__ res) {
    const int i = blockIdx.x * CR_BLOCK + threadIdx.x;
    if (i < prm.nt) {
        double R[9], t[3], P[12];
        pose_split(pose + (size_t)i * 12, R, t);
        pnp_projection(prm.K, R, t, P);
        for (int k = 0; k < 12; k++) kP[(size_t)slots[i] * 12 + k] = P[k];
    }
    bool mv = false;
    if (i < v.n_pts) {
        nval[i] = map_point_of(v, i, 0, tab); drow[i] = INT_MAX;
        merge_reset(i, parent, mcnt, mcur, surv);
        bool at_c = false, at_g = false;
        map_each_obs(v, i, [&](int, int pos, int, int) { at_c |= cmask[pos] != 0; at_g |= gmask[pos] != 0; return false; });
        mv = at_c && !at_g;
        moved[i] = mv;
        if (mv) {
            float* x = v.src.xyz + (size_t)i * 3;
            const double x0 = (double)x[0], x1 = (double)x[1], x2 = (double)x[2];
            for (int d = 0; d < 3; d++) x[d] = (float)(prm.A[d * 4] * x0 + prm.A[d * 4 + 1] * x1 + prm.A[d * 4 + 2] * x2 + prm.A[d * 4 + 3]);
        }
    }
    wave_count_add(mv, &res->n_moved);
}

// one thread per row of p: its loop point against the row's owner
__global__ __launch_bounds__(CR_BLOCK) void k_cr_direct(MapView v, int p, int n_p, const int32_t* __restrict__ lp, const int32_t* __restrict__ tab,
                                                         int32_t* __restrict__ parent, int32_t* __restrict__ drow, CrRes* __restrict__ res) {
    const int r = blockIdx.x * CR_BLOCK + threadIdx.x;
    bool edge = false, first = false;
    if (r < n_p) {
        const int L = lp[r];
        if (L >= 0 && L < v.n_pts) {
            const int o = tab[(size_t)p * v.row + r];
            if (o != INT_MAX) {
                edge = o != L;
                if (edge) merge_unite(parent, o, L);
            } else if (!map_observes(v, L, p)) {
                first = atomicMin(drow + L, r) == INT_MAX;   // (one first claim per point, whichever row makes it)
            }
        }
    }
    wave_count_add(edge, &res->n_direct_edges);
    wave_count_add(first, &res->n_direct_gained);
}

extern "C" int mo_map_loop_correct(mo_map* m, const double K[9], const double* poses, const mo_map_correct_params* prm, mo_map_correct_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!K || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const int n_kf = (int)m->pos_slot.size();
    if (n_kf > 0 && !poses) return mo_fail(c, MO_ERR_ARG, "poses is NULL");
    if (prm->w <= 0 || prm->h <= 0) return mo_fail(c, MO_ERR_ARG, "w and h must be > 0");
    if (!(prm->scale > 0.0) || !std::isfinite(prm->scale)) return mo_fail(c, MO_ERR_ARG, "scale must be finite and > 0");
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(prm->R[i]) || !std::isfinite(K[i])) return mo_fail(c, MO_ERR_ARG, "R and K must be finite");
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(prm->t[i])) return mo_fail(c, MO_ERR_ARG, "t must be finite");
    if (!(prm->radius >= 0.0) || !std::isfinite(prm->radius)) return mo_fail(c, MO_ERR_ARG, "radius must be finite and >= 0");
    if (!(prm->scale_factor > 0.0) || !std::isfinite(prm->scale_factor)) return mo_fail(c, MO_ERR_ARG, "scale_factor must be finite and > 0");
    if (!(prm->chi2 >= 0.0)) return mo_fail(c, MO_ERR_ARG, "chi2 must be >= 0");
    for (size_t i = 0; i < (size_t)n_kf * 12; i++)
        if (!std::isfinite(poses[i])) return mo_fail(c, MO_ERR_ARG, "poses must be finite");
    out->n_corrected = out->n_moved = out->n_loop_points = out->n_direct_edges = out->n_direct_gained = out->n_pairs = out->n_cand = 0;
    out->n_proposals = out->n_gained = out->n_edges = out->n_absorbed = 0;
    out->n_points = m->n_pts; out->n_obs = m->n_obs;
    for (int i = 0; i < 12; i++) out->A[i] = i % 5 == 0 ? 1.0 : 0.0;
    out->A_scale = 1.0;
    if (out->into) for (int64_t i = 0; i < m->n_pts; i++) out->into[i] = (int32_t)i;
    if (out->moved && m->n_pts) std::memset(out->moved, 0, (size_t)m->n_pts);
    if (out->poses_out && n_kf) std::memcpy(out->poses_out, poses, (size_t)n_kf * 96);
    if (n_kf == 0 || m->n_pts == 0) return MO_OK;   // (nothing to correct: not an error)
    const int p = prm->kf_pos, q = prm->cand_pos;
    if (p < 0 || p >= n_kf || q < 0 || q >= n_kf) return mo_fail(c, MO_ERR_ARG, "kf_pos and cand_pos must be keyframe positions");
    if (!prm->corrected || !prm->corrected[p]) return mo_fail(c, MO_ERR_ARG, "corrected must hold kf_pos");
    std::vector<uint8_t> cmask((size_t)n_kf), gmask((size_t)n_kf, 0);
    std::vector<int32_t> cpos, slots;
    size_t rows_sum = 0;
    for (int k = 0; k < n_kf; k++) {
        cmask[k] = prm->corrected[k] != 0;
        if (prm->group) gmask[k] = prm->group[k] != 0;
        if (cmask[k] && gmask[k]) return mo_fail(c, MO_ERR_ARG, "a position is both corrected and of the group");
        if (cmask[k]) { cpos.push_back(k); slots.push_back(m->pos_slot[k]); rows_sum += (size_t)m->h_kcnt[m->pos_slot[k]]; }
    }
    const int nt = (int)cpos.size(), row = m->row, n_p = m->h_kcnt[m->pos_slot[p]];
    if (nt > FU_MAX_TARGETS) return mo_fail(c, MO_ERR_UNSUPPORTED, "more corrected keyframes than one call searches (16384)");
    // rule 1: A = S_cw'^-1 T_p with S_cw' = S_pc T_cand, f64, each row summed left to right
    const double s = prm->scale, *R = prm->R, *t = prm->t;
    double Rp[9], tp[3], Rc[9], tc[3], Rq[9], tq[3], d[3], RA[9], tA[3];
    pose_split(poses + (size_t)p * 12, Rp, tp);
    pose_split(poses + (size_t)q * 12, Rc, tc);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Rq[i * 3 + j] = R[i * 3] * Rc[j] + R[i * 3 + 1] * Rc[3 + j] + R[i * 3 + 2] * Rc[6 + j];
        const double u = R[i * 3] * tc[0] + R[i * 3 + 1] * tc[1] + R[i * 3 + 2] * tc[2];
        tq[i] = s * u + t[i];
        d[i] = tp[i] - tq[i];
    }
    const double inv = 1.0 / s;
    CrPrm g;
    std::memset(&g, 0, sizeof(g));
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            RA[i * 3 + j] = Rq[i] * Rp[j] + Rq[3 + i] * Rp[3 + j] + Rq[6 + i] * Rp[6 + j];
            g.A[i * 4 + j] = inv * RA[i * 3 + j];
        }
        tA[i] = Rq[i] * d[0] + Rq[3 + i] * d[1] + Rq[6 + i] * d[2];
        g.A[i * 4 + 3] = inv * tA[i];
    }
    // rule 2: S_iw' = T_i A^-1 = [s R_i RA^T | t_i - R_i RA^T tA]; the pose is [R_i RA^T | (t_i - R_i RA^T tA) / s]
    std::vector<double> pose((size_t)nt * 12);
    for (int e = 0; e < nt; e++) {
        double Ri[9], ti[3];
        pose_split(poses + (size_t)cpos[e] * 12, Ri, ti);
        double* o = pose.data() + (size_t)e * 12;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) o[i * 4 + j] = Ri[i * 3] * RA[j * 3] + Ri[i * 3 + 1] * RA[j * 3 + 1] + Ri[i * 3 + 2] * RA[j * 3 + 2];
            const double v = o[i * 4] * tA[0] + o[i * 4 + 1] * tA[1] + o[i * 4 + 2] * tA[2];
            o[i * 4 + 3] = (ti[i] - v) / s;
        }
    }
    MAP_ENTER(m);
    HostClock clk(c);
    const size_t np = (size_t)m->n_pts, trow = (size_t)nt * row, krow = (size_t)n_kf * row;
    const size_t gain_bound = rows_sum + (size_t)n_p;
    int rc;
    if ((rc = merge_int32_guard(m, (size_t)nt, krow, gain_bound))) return rc;
    CorrectBufs& b = map_feature<CorrectBufs>(m);
    MergeBufs& mg = b.mg;
    const size_t np1 = std::max(n_p, 1);
    if ((rc = merge_reserve(m, mg, (size_t)nt, gain_bound)) ||
        (rc = mo_reserve(c, b.cmask, (size_t)n_kf, b.gmask, (size_t)n_kf, b.cpos, (size_t)nt, b.slots, (size_t)nt, b.pose, (size_t)nt * 12, b.lp, np1, b.tab, krow,
                         b.drow, np, b.moved, np, b.res)))
        return rc;
    mo_stage_begin(c);
    HIPCHK(c, hipMemsetAsync(b.res, 0, sizeof(CrRes), c->stream));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)b.tab.p, INT_MAX, krow, c->stream));
    HIPCHK(c, hipMemsetAsync(mg.key, 0xff, trow * 8, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.cmask, cmask.data(), (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.gmask, gmask.data(), (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.cpos, cpos.data(), (size_t)nt * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.slots, slots.data(), (size_t)nt * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.pose, pose.data(), (size_t)nt * 96, hipMemcpyHostToDevice, c->stream));
    if (prm->loop_point && n_p) HIPCHK(c, hipMemcpyAsync(b.lp, prm->loop_point, (size_t)n_p * 4, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(b.lp, 0xff, np1 * 4, c->stream));
    for (int i = 0; i < 9; i++) g.K[i] = K[i];
    g.radius = prm->radius; g.sf = prm->scale_factor; g.chi2 = prm->chi2;
    g.w = prm->w; g.h = prm->h; g.max_dist = prm->max_dist; g.p = p; g.n_p = n_p; g.nt = nt;
    const MapView mv = map_view(m);
    const CrView v{mv, b.cpos, b.lp, b.drow, mg.prop, mg.key, b.tab, p, nt};
    const unsigned pblocks = (unsigned)((std::max(np, (size_t)nt) + CR_BLOCK - 1) / CR_BLOCK);
    if ((rc = trk_launch_rep_mask(m, b.gmask, mg.rep, mg.oct, &b.res.p->n_loop_points))) return rc;
    hipLaunchKernelGGL(k_cr_move, dim3(pblocks), dim3(CR_BLOCK), 0, c->stream, mv, g, b.cmask, b.gmask, b.slots, b.pose, m->kP, b.tab, mg.nval, mg.parent, mg.mcnt,
                       mg.mcur, mg.surv, b.drow, b.moved, b.res);
    HIPCHK(c, hipGetLastError());
    if ((rc = trk_launch_grid(m, b.slots, 0, nt, prm->w, prm->h, mg.cell, mg.sorted))) return rc;
    mo_stage_mark(c, "correct_move");
    hipLaunchKernelGGL(k_cr_direct, dim3((unsigned)((np1 + CR_BLOCK - 1) / CR_BLOCK)), dim3(CR_BLOCK), 0, c->stream, mv, p, n_p, b.lp, b.tab, mg.parent, b.drow,
                       b.res);
    hipLaunchKernelGGL((k_merge_search<CrView, CrPrm, CrRes>), dim3(pblocks, (unsigned)nt), dim3(MG_BLOCK), 0, c->stream, g, v, m->kkps, m->kdesc, m->kP, mg.rep,
                       mg.oct, mg.cell, mg.sorted, mg.key, mg.prop, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "correct_search");
    if ((rc = merge_enqueue(m, v, mg, b.slots, b.res, "correct_merge"))) return rc;
    if (out->moved) HIPCHK(c, hipMemcpyAsync(out->moved, b.moved, np, hipMemcpyDeviceToHost, c->stream));
    bool fused;
    if ((rc = merge_finish<CrView>(m, mg, b.res, clk, out->into, &fused))) return rc;
    const CrRes& r = b.res.host();
    for (int i = 0; i < 12; i++) out->A[i] = g.A[i];
    out->A_scale = inv;
    if (out->poses_out)
        for (int e = 0; e < nt; e++) std::memcpy(out->poses_out + (size_t)cpos[e] * 12, pose.data() + (size_t)e * 12, 96);
    out->n_corrected = nt; out->n_moved = r.n_moved; out->n_loop_points = r.n_loop_points;
    out->n_direct_edges = r.n_direct_edges; out->n_direct_gained = r.n_direct_gained;
    out->n_pairs = r.n_pairs; out->n_cand = r.n_cand; out->n_proposals = r.n_proposals; out->n_gained = r.n_gained; out->n_edges = r.n_edges;
    if (!fused) return MO_OK;   // (the move and kP are written in place)
    out->n_absorbed = r.n_absorbed;
    out->n_points = m->n_pts; out->n_obs = m->n_obs;
    return MO_OK;
}
