// map_fuse.hip -- fusion of duplicate map points on the device map (mo_map_fuse in include/vslam_amd.h): ORB-SLAM2's
// LocalMapping::SearchInNeighbors / ORBmatcher::Fuse / MapPoint::Replace on the map as it stands.  Every local point is projected into
// every target keyframe that does not observe it yet; a keypoint it matches either belongs to another point (the two are one feature:
// a merge edge) or to none (the point gains the observation).  Writes the fused map into the other copy of the store.
//
// Chain (one synchronisation, the copy-out; every kernel behind the search reads n_proposals first and returns when it is 0):
//   k_fuse_prep     one thread per point: point_of of the targets (atomicMin), valid observations, union-find and survivor tables reset
//   k_trk_rep       the local map with its representative descriptors (map_track.hip's kernel, through trk_launch_rep)
//   k_trk_grid      one block per target: its keypoints sorted into 64 x 48 cells (trk_launch_grid)
//   k_merge_search  one thread per (point, target): the pair's proposal (map_merge.h)
//   merge_enqueue   resolve, flatten, members, count, scatter: the merge stages of map_merge.h, which the loop correction runs too
// This file is the plain view of those stages (FuseView): target t is the keyframe at position lo_pos + t, a row is free when point_of
// says so, the survivor of a component has the most valid observations (then the lowest index), and every gain comes from the search.
// mo_map_fuse_frustum: the same chain with k_view_centres and k_view_points (map_view_geom.hip, through view_enqueue) behind k_trk_rep and
// k_fuse_search_frustum in place of k_merge_search.
// Integer atomics only: equal maps give equal bytes.  -ffp-contract=off (Makefile): the projection and the gates round like
// tests/fuse_restatement.py.
#include <climits>
#include <cmath>

#include "common.h"
#include "map_store.h"
#include "map_search.h"
#include "map_merge.h"

struct FusePrm {
    double radius, sf, chi2;
    int w, h, max_dist;
};

struct FuseRes {
    int32_t n_local, n_pairs, n_cand, n_proposals, n_gained, n_edges, n_absorbed;
    int32_t n_points, n_obs, n_members;
};

struct FuseBufs : MapFeature {
    MergeBufs mg;
    DevBuf<int32_t> tab;                  // [target][row] point_of (INT_MAX: a free row)
    ResBlock<FuseRes> res;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) { mg.each_scratch(f); f(tab); f(res); }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// what the kernels read (by value): the map, fuse's own tables and window, and the plain answers to what the merge stages ask
struct FuseView {
    MapView map;
    const int32_t* prop; const unsigned long long* key; const int32_t* tab;
    int lo_pos, n_targets;
    __device__ __forceinline__ int pos_of(int t) const { return lo_pos + t; }
    __device__ __forceinline__ int owner(int t, int r) const { return tab[(size_t)t * map.row + r]; }
    // most observations, then lowest index
    __device__ static __forceinline__ unsigned long long surv_key(int i, int nval, int) {
        return ((unsigned long long)(0xffffffffu - (unsigned)nval) << 32) | (unsigned)i;
    }
    __device__ __forceinline__ bool direct(int, int*, int*) const { return false; }
    __host__ __device__ static bool any(const FuseRes* r) { return r->n_proposals != 0; }
};

// one thread per point: valid observations counted, those at a target entered into point_of; tables of the later kernels reset
__global__ __launch_bounds__(MG_BLOCK) void k_fuse_prep(FuseView v, int32_t* __restrict__ tab, int32_t* __restrict__ nval, int32_t* __restrict__ parent,
                                                         int32_t* __restrict__ mcnt, int32_t* __restrict__ mcur, unsigned long long* __restrict__ surv) {
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= v.map.n_pts) return;
    nval[i] = map_point_of(v.map, i, v.lo_pos, tab);
    merge_reset(i, parent, mcnt, mcur, surv);
}

__global__ __launch_bounds__(MG_BLOCK) void k_fuse_search_frustum(FusePrm prm, FuseFrustum fr, FuseView v, const mo_keypoint* __restrict__ kkps,
                                                                   const uint8_t* __restrict__ kdesc, const double* __restrict__ kP,
                                                                   const uint8_t* __restrict__ rep, const int32_t* __restrict__ oct,
                                                                   const int32_t* __restrict__ cell, const int32_t* __restrict__ sorted,
                                                                   unsigned long long* __restrict__ key, int32_t* __restrict__ prop,
                                                                   FuseRes* __restrict__ res) {
    merge_search<true>(prm, v, kkps, kdesc, kP, rep, oct, cell, sorted, key, prop, res, &fr);
}

// mo_map_fuse (fprm NULL: the plain search and exactly the launches it had) and mo_map_fuse_frustum
static int fuse_run(mo_map* m, const mo_map_fuse_params* prm, const mo_map_frustum_params* fprm, mo_map_fuse_out* out) {
    mo_ctx* c = m->c;
    if (!prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (fprm && (fprm->n_levels < 1 || !std::isfinite(fprm->range_lo) || !std::isfinite(fprm->range_hi) || !std::isfinite(fprm->min_cos)))
        return mo_fail(c, MO_ERR_ARG, "n_levels must be >= 1, range_lo, range_hi and min_cos finite");
    if (prm->w <= 0 || prm->h <= 0) return mo_fail(c, MO_ERR_ARG, "w and h must be > 0");
    if (prm->window < 0) return mo_fail(c, MO_ERR_ARG, "window must be >= 0");
    if (!(prm->radius >= 0.0) || !std::isfinite(prm->radius)) return mo_fail(c, MO_ERR_ARG, "radius must be finite and >= 0");
    if (!(prm->scale_factor > 0.0) || !std::isfinite(prm->scale_factor)) return mo_fail(c, MO_ERR_ARG, "scale_factor must be finite and > 0");
    if (!(prm->chi2 >= 0.0)) return mo_fail(c, MO_ERR_ARG, "chi2 must be >= 0");
    MAP_ENTER(m);
    HostClock clk(c);
    out->n_targets = out->n_local = out->n_pairs = out->n_cand = out->n_proposals = out->n_gained = out->n_edges = out->n_absorbed = 0;
    out->n_points = m->n_pts; out->n_obs = m->n_obs;
    if (out->into) for (int64_t i = 0; i < m->n_pts; i++) out->into[i] = (int32_t)i;
    const int n_kf = (int)m->pos_slot.size();
    if (n_kf == 0 || m->n_pts == 0) return MO_OK;   // (nothing to fuse: not an error)
    const int lo_pos = map_window_lo(prm->window, n_kf);
    const int nt = n_kf - lo_pos, row = m->row;
    if (nt > FU_MAX_TARGETS) return mo_fail(c, MO_ERR_UNSUPPORTED, "more target keyframes than one call searches (16384)");
    const size_t np = (size_t)m->n_pts;
    size_t rows_sum = 0;
    for (int k = lo_pos; k < n_kf; k++) rows_sum += (size_t)m->h_kcnt[m->pos_slot[k]];
    const size_t gain_bound = std::min(np * (size_t)nt, rows_sum);
    const size_t trow = (size_t)nt * row;
    int rc;
    if ((rc = merge_int32_guard(m, (size_t)nt, trow, gain_bound))) return rc;
    FuseBufs& b = map_feature<FuseBufs>(m);
    MergeBufs& g = b.mg;
    if ((rc = merge_reserve(m, g, (size_t)nt, gain_bound)) || (rc = mo_reserve(c, b.tab, trow, b.res))) return rc;
    mo_stage_begin(c);
    HIPCHK(c, hipMemsetAsync(b.res, 0, sizeof(FuseRes), c->stream));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)b.tab.p, INT_MAX, trow, c->stream));
    HIPCHK(c, hipMemsetAsync(g.key, 0xff, trow * 8, c->stream));
    const FuseView v{map_view(m), g.prop, g.key, b.tab, lo_pos, nt};
    const FusePrm p{prm->radius, prm->scale_factor, prm->chi2, prm->w, prm->h, prm->max_dist};
    const unsigned pblocks = (unsigned)((np + MG_BLOCK - 1) / MG_BLOCK);
    const int32_t* slots = m->d_pos_slot + lo_pos;
    hipLaunchKernelGGL(k_fuse_prep, dim3(pblocks), dim3(MG_BLOCK), 0, c->stream, v, b.tab, g.nval, g.parent, g.mcnt, g.mcur, g.surv);
    HIPCHK(c, hipGetLastError());
    if ((rc = trk_launch_rep(m, lo_pos, g.rep, g.oct, &b.res.p->n_local)) || (rc = trk_launch_grid(m, slots, 0, nt, prm->w, prm->h, g.cell, g.sorted)))
        return rc;
    mo_stage_mark(c, "fuse_prep");
    if (fprm) {   // the view records of the local points behind k_trk_rep, the centres of the targets with them
        FuseFrustum fr{FrustumPrm{prm->scale_factor, fprm->range_lo, fprm->range_hi, fprm->min_cos, fprm->n_levels}, nullptr, nullptr};
        if ((rc = view_enqueue(m, g.oct, prm->scale_factor, &fr.rec, &fr.centre))) return rc;
        mo_stage_mark(c, "fuse_view");
        hipLaunchKernelGGL(k_fuse_search_frustum, dim3(pblocks, (unsigned)nt), dim3(MG_BLOCK), 0, c->stream, p, fr, v, m->kkps, m->kdesc, m->kP, g.rep, g.oct,
                           g.cell, g.sorted, g.key, g.prop, b.res);
    } else
        hipLaunchKernelGGL((k_merge_search<FuseView, FusePrm, FuseRes>), dim3(pblocks, (unsigned)nt), dim3(MG_BLOCK), 0, c->stream, p, v, m->kkps, m->kdesc,
                           m->kP, g.rep, g.oct, g.cell, g.sorted, g.key, g.prop, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "fuse_search");
    if ((rc = merge_enqueue(m, v, g, slots, b.res, "fuse_merge"))) return rc;
    bool fused;
    if ((rc = merge_finish<FuseView>(m, g, b.res, clk, out->into, &fused))) return rc;
    const FuseRes& r = b.res.host();
    out->n_targets = nt; out->n_local = r.n_local; out->n_pairs = r.n_pairs; out->n_cand = r.n_cand;
    if (!fused) return MO_OK;
    out->n_proposals = r.n_proposals; out->n_gained = r.n_gained; out->n_edges = r.n_edges; out->n_absorbed = r.n_absorbed;
    out->n_points = m->n_pts; out->n_obs = m->n_obs;
    return MO_OK;
}

extern "C" int mo_map_fuse(mo_map* m, const mo_map_fuse_params* prm, mo_map_fuse_out* out) {
    if (!m) return MO_ERR_ARG;
    return fuse_run(m, prm, nullptr, out);
}

extern "C" int mo_map_fuse_frustum(mo_map* m, const mo_map_fuse_params* prm, const mo_map_frustum_params* fprm, mo_map_fuse_out* out) {
    if (!m) return MO_ERR_ARG;
    if (!fprm) return mo_fail(m->c, MO_ERR_ARG, "NULL argument");
    return fuse_run(m, prm, fprm, out);
}
