// map_fuse.hip -- fusion of duplicate map points on the device map (mo_map_fuse in include/vslam_amd.h): ORB-SLAM2's
// LocalMapping::SearchInNeighbors / ORBmatcher::Fuse / MapPoint::Replace on the map as it stands.  Every local point is projected into
// every target keyframe that does not observe it yet; a keypoint it matches either belongs to another point (the two are one feature:
// a merge edge) or to none (the point gains the observation).  Writes the fused map into the other copy of the store.
//
// Chain (one synchronisation, the copy-out; every kernel behind the search reads n_proposals first and returns when it is 0):
//   k_fuse_prep     one thread per point: point_of of the targets (atomicMin), valid observations, union-find and survivor tables reset
//   k_trk_rep       the local map with its representative descriptors (map_track.hip's kernel, through trk_launch_rep)
//   k_trk_grid      one block per target: its keypoints sorted into 64 x 48 cells (trk_launch_grid)
//   k_fuse_search   one thread per (point, target): pair test, projection under the stored P, window over the cells, 256-bit Hamming
//                   distances, the chi2 gate; the accepted keypoint is claimed by a 64-bit atomicMin of (dist << 32) | point
//   k_fuse_resolve  one thread per (target, row): the winner of a claimed row against the row's owner: a gained observation, or a merge
//                   edge hooked into the lock-free union-find (the larger root under the smaller by atomicCAS)
//   k_fuse_flatten  one thread per point: its root (= the lowest index of its component), the component's size and survivor (atomicMin
//                   of (~valid observations << 32) | point)
//   map_scan_excl + k_fuse_members   the members of every component next to each other
//   k_fuse_count    one thread per point: survivors sort their members by index and count their merged list
//   map_scan_excl x 2 + k_fuse_scatter   new indices and offsets; every field of every survivor into the other copy
// mo_map_fuse_frustum: the same chain with k_view_centres and k_view_points (map_view_geom.hip, through view_enqueue) behind k_trk_rep and
// k_fuse_search_frustum in place of k_fuse_search.
// Integer atomics only (minima, sums, a compare-and-swap whose outcome - the component's lowest index - is the same in any order):
// equal maps give equal bytes.  -ffp-contract=off (Makefile): the projection and the gates round like tests/fuse_restatement.py.
#include <climits>
#include <cmath>

#include "common.h"
#include "map_store.h"
#include "map_search.h"
#include "ba.h"   // ba_info

#define FU_BLOCK 256
#define FU_MAX_TARGETS 16384   // grid.y of the search; also what the per-keyframe list sort holds (map_kernels.hip)

struct FusePrm {
    double radius, sf, chi2;
    int w, h, max_dist;
};

struct FuseRes {
    int32_t n_local, n_pairs, n_cand, n_proposals, n_gained, n_edges, n_absorbed;
    int32_t n_points, n_obs, n_members;
};

struct FuseBufs : MapFeature {
    DevBuf<uint8_t> rep;                  // [point][32] representative descriptors
    DevBuf<int32_t> oct;                  // [point] ref_octave (TK_NOT_LOCAL: not in the local map)
    DevBuf<int32_t> cell, sorted;         // [target][TK_CELLS + 1], [target][row]: the keypoint grids
    DevBuf<int32_t> tab;                  // [target][row] point_of (INT_MAX: a free row)
    DevBuf<unsigned long long> key;       // [target][row] (dist << 32) | point of the claim on each keypoint
    DevBuf<int32_t> prop;                 // [target][point] the row each pair proposed (-1: none)
    DevBuf<int32_t> parent, root, nval;   // [point] union-find, flattened root, valid observations
    DevBuf<unsigned long long> surv;      // [point] at a root: (~valid observations << 32) | point of the survivor
    DevBuf<int32_t> mcnt, mbase, mcur, mem;   // [point] members per root, their first entry, scatter cursors, the member lists
    DevBuf<int32_t> into;                 // [point] new index of the point each old point now is
    ResBlock<FuseRes> res;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) {
        f(rep); f(oct); f(cell); f(sorted); f(tab); f(key); f(prop); f(parent); f(root); f(nval); f(surv); f(mcnt); f(mbase); f(mcur); f(mem); f(into); f(res);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// what the fuse kernels read (by value): the map, and fuse's own tables and window
struct FuseView {
    MapView map;
    const int32_t* prop; const unsigned long long* key; const int32_t* tab;
    int lo_pos, n_targets;
};

// one thread per point: valid observations counted, those at a target entered into point_of; tables of the later kernels reset
__global__ __launch_bounds__(FU_BLOCK) void k_fuse_prep(FuseView v, int32_t* __restrict__ tab, int32_t* __restrict__ nval, int32_t* __restrict__ parent,
                                                         int32_t* __restrict__ mcnt, int32_t* __restrict__ mcur, unsigned long long* __restrict__ surv) {
    const int i = blockIdx.x * FU_BLOCK + threadIdx.x;
    if (i >= v.map.n_pts) return;
    nval[i] = map_point_of(v.map, i, v.lo_pos, tab); parent[i] = i; mcnt[i] = 0; mcur[i] = 0; surv[i] = TK_NONE;
}

// what the frustum mode (mo_map_fuse_frustum) adds to the search's arguments (by value): the view records of the local points and the
// camera centres of the keyframe positions (map_view_geom.hip)
struct FuseFrustum {
    FrustumPrm f;
    const ViewRec* rec;
    const double* centre;
};

// one thread per (point, target): the pair's proposal.  FR = false is mo_map_fuse's search (fr unused); FR = true: a candidate also lies
// in the point's frustum seen from the target's centre, and is searched at its predicted level L with the octave gate [L - 1, L].
template <bool FR> __device__ __forceinline__ void fuse_search(const FusePrm& prm, const FuseView& v, const mo_keypoint* __restrict__ kkps,
                                                               const uint8_t* __restrict__ kdesc, const double* __restrict__ kP,
                                                               const uint8_t* __restrict__ rep, const int32_t* __restrict__ oct,
                                                               const int32_t* __restrict__ cell, const int32_t* __restrict__ sorted,
                                                               unsigned long long* __restrict__ key, int32_t* __restrict__ prop, FuseRes* __restrict__ res,
                                                               const FuseFrustum* fr) {
    const int t = blockIdx.y, i = blockIdx.x * FU_BLOCK + threadIdx.x;
    const MapView& mv = v.map;
    const int pos = v.lo_pos + t, slot = mv.pos_slot[pos];
    const int ro = i < mv.n_pts ? oct[i] : TK_NOT_LOCAL;
    const bool pair = ro != TK_NOT_LOCAL && !map_observes(mv, i, pos);
    double uu = 0.0, vv = 0.0;
    bool cand = pair && trk_project(kP + (size_t)slot * 12, mv.src.xyz[(size_t)i * 3], mv.src.xyz[(size_t)i * 3 + 1], mv.src.xyz[(size_t)i * 3 + 2],
                                    prm.w, prm.h, &uu, &vv);
    int lv = ro;   // the octave the window is scaled by
    if constexpr (FR) {
        if (cand)
            cand = trk_frustum(fr->f, fr->rec[i], fr->centre + (size_t)pos * 3, mv.src.xyz[(size_t)i * 3], mv.src.xyz[(size_t)i * 3 + 1],
                               mv.src.xyz[(size_t)i * 3 + 2], &lv);
    }
    int bd = INT_MAX, bq = INT_MAX;
    if (cand) {
        const uint8_t* __restrict__ fdesc = kdesc + (size_t)slot * mv.row * 32;
        const uint8_t* d = rep + (size_t)i * 32;
        auto visit = [&](int q, const mo_keypoint& kp, double dx, double dy) {
            if (!(ba_info(prm.sf, kp.octave) * (dx * dx + dy * dy) <= prm.chi2)) return;
            trk_take(trk_ham(d, fdesc + (size_t)q * 32), q, bd, bq);
        };
        if constexpr (FR)
            trk_window_oct(uu, vv, prm.radius * trk_scale(prm.sf, lv), lv - 1, lv, prm.w, prm.h, cell + (size_t)t * (TK_CELLS + 1), sorted + (size_t)t * mv.row,
                           kkps + (size_t)slot * mv.row, visit);
        else
            trk_window(uu, vv, prm.radius * trk_scale(prm.sf, ro), ro, prm.w, prm.h, cell + (size_t)t * (TK_CELLS + 1), sorted + (size_t)t * mv.row,
                       kkps + (size_t)slot * mv.row, visit);
    }
    const bool acc = bd != INT_MAX && bd <= prm.max_dist;
    if (acc) atomicMin(key + (size_t)t * mv.row + bq, ((unsigned long long)(unsigned)bd << 32) | (unsigned)i);
    if (i < mv.n_pts) prop[(size_t)t * mv.n_pts + i] = acc ? bq : -1;
    wave_count_add(pair, &res->n_pairs);
    wave_count_add(cand, &res->n_cand);
    wave_count_add(acc, &res->n_proposals);
}

__global__ __launch_bounds__(FU_BLOCK) void k_fuse_search(FusePrm prm, FuseView v, const mo_keypoint* __restrict__ kkps, const uint8_t* __restrict__ kdesc,
                                                           const double* __restrict__ kP, const uint8_t* __restrict__ rep, const int32_t* __restrict__ oct,
                                                           const int32_t* __restrict__ cell, const int32_t* __restrict__ sorted,
                                                           unsigned long long* __restrict__ key, int32_t* __restrict__ prop, FuseRes* __restrict__ res) {
    fuse_search<false>(prm, v, kkps, kdesc, kP, rep, oct, cell, sorted, key, prop, res, nullptr);
}

__global__ __launch_bounds__(FU_BLOCK) void k_fuse_search_frustum(FusePrm prm, FuseFrustum fr, FuseView v, const mo_keypoint* __restrict__ kkps,
                                                                   const uint8_t* __restrict__ kdesc, const double* __restrict__ kP,
                                                                   const uint8_t* __restrict__ rep, const int32_t* __restrict__ oct,
                                                                   const int32_t* __restrict__ cell, const int32_t* __restrict__ sorted,
                                                                   unsigned long long* __restrict__ key, int32_t* __restrict__ prop,
                                                                   FuseRes* __restrict__ res) {
    fuse_search<true>(prm, v, kkps, kdesc, kP, rep, oct, cell, sorted, key, prop, res, &fr);
}

__device__ __forceinline__ int fuse_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// lock-free union: the larger of the two roots is hooked under the smaller; a lost race is retried from the new roots.  parent[x] <= x
// always, so every walk ends, and the root of a finished component is its lowest index whatever the order of the hooks.
__device__ __forceinline__ void fuse_unite(int32_t* parent, int a, int b) {
    for (;;) {
        for (int p; (p = fuse_load(parent + a)) != a;) a = p;
        for (int p; (p = fuse_load(parent + b)) != b;) b = p;
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(parent + hi, hi, lo) == hi) return;
    }
}

// one thread per (target, row): the row's winner against its owner
__global__ __launch_bounds__(FU_BLOCK) void k_fuse_resolve(int row, const int32_t* __restrict__ kcnt, const int32_t* __restrict__ slots,
                                                            const unsigned long long* __restrict__ key, const int32_t* __restrict__ tab,
                                                            int32_t* __restrict__ parent, FuseRes* __restrict__ res) {
    if (!res->n_proposals) return;
    const int t = blockIdx.y, r = blockIdx.x * FU_BLOCK + threadIdx.x;
    bool gain = false, edge = false;
    if (r < row && r < kcnt[slots[t]]) {
        const size_t e = (size_t)t * row + r;
        const unsigned long long k = key[e];
        if (k != TK_NONE) {
            const int owner = tab[e];
            gain = owner == INT_MAX;
            edge = !gain;
            if (edge) fuse_unite(parent, (int)(k & 0xffffffffu), owner);
        }
    }
    wave_count_add(gain, &res->n_gained);
    wave_count_add(edge, &res->n_edges);
}

__global__ __launch_bounds__(FU_BLOCK) void k_fuse_flatten(int n_pts, const int32_t* __restrict__ parent, const int32_t* __restrict__ nval,
                                                            int32_t* __restrict__ root, int32_t* __restrict__ mcnt, unsigned long long* __restrict__ surv,
                                                            const FuseRes* __restrict__ res) {
    if (!res->n_proposals) return;
    const int i = blockIdx.x * FU_BLOCK + threadIdx.x;
    if (i >= n_pts) return;
    int r = i;
    for (int p; (p = parent[r]) != r;) r = p;
    root[i] = r;
    atomicAdd(mcnt + r, 1);
    atomicMin(surv + r, ((unsigned long long)(0xffffffffu - (unsigned)nval[i]) << 32) | (unsigned)i);   // most observations, then lowest index
}

__global__ __launch_bounds__(FU_BLOCK) void k_fuse_members(int n_pts, const int32_t* __restrict__ root, const int32_t* __restrict__ mbase,
                                                            int32_t* __restrict__ mcur, int32_t* __restrict__ mem, const FuseRes* __restrict__ res) {
    if (!res->n_proposals) return;
    const int i = blockIdx.x * FU_BLOCK + threadIdx.x;
    if (i >= n_pts) return;
    const int r = root[i];
    mem[mbase[r] + atomicAdd(mcur + r, 1)] = i;   // (arrival order: the survivor sorts its run)
}

// the gained observation of point j at target t: the row it proposed, won, and that no point owns
__device__ __forceinline__ bool fuse_gained(const FuseView& v, int j, int t, int* r) {
    const int pr = v.prop[(size_t)t * v.map.n_pts + j];
    if (pr < 0) return false;
    const size_t e = (size_t)t * v.map.row + pr;
    if ((int)(v.key[e] & 0xffffffffu) != j || v.tab[e] != INT_MAX) return false;
    *r = pr;
    return true;
}

// The candidate entries of survivor s with members mem[0 .. nm) (ascending) in the order of the merged list: (0) its own valid
// entries, (1) the valid entries of the other members, (2) the gained observations of all members by (member, position).
// f(index, kind, position, row) -> true stops the walk.
template <class F> __device__ __forceinline__ void fuse_walk(const FuseView& v, int s, const int32_t* __restrict__ mem, int nm, F f) {
    int idx = 0, kp;
    bool stop = false;
    map_each_obs(v.map, s, [&](int, int pos, int, int r) { return stop = f(idx++, 0, pos, r); });
    for (int a = 0; a < nm && !stop; a++)
        if (mem[a] != s) map_each_obs(v.map, mem[a], [&](int, int pos, int, int r) { return stop = f(idx++, 1, pos, r); });
    for (int a = 0; a < nm && !stop; a++)
        for (int t = 0; t < v.n_targets; t++)
            if (fuse_gained(v, mem[a], t, &kp) && f(idx++, 2, v.lo_pos + t, kp)) return;
}

// The merged list of survivor s behind its own entries: an entry of kinds 1 and 2 is kept when no earlier candidate stands at its
// position (a dropped one was dropped for a holder of that position before it, so "an earlier candidate" and "the list already holds a
// valid observation there" are the same).  emit(position, row) per kept entry; returns their number.
template <class E> __device__ __forceinline__ int fuse_merge(const FuseView& v, int s, const int32_t* __restrict__ mem, int nm, E emit) {
    int n = 0;
    fuse_walk(v, s, mem, nm, [&](int idx, int kind, int pos, int kp) {
        if (kind == 0) return false;
        bool held = false;
        fuse_walk(v, s, mem, nm, [&](int idx2, int, int pos2, int) {
            if (idx2 >= idx) return true;
            held = pos2 == pos;
            return held;
        });
        if (!held) { emit(pos, kp); n++; }
        return false;
    });
    return n;
}

// one thread per point: keep = it is its component's survivor; a survivor sorts its members and counts its merged list
__global__ __launch_bounds__(FU_BLOCK) void k_fuse_count(FuseView v, const int32_t* __restrict__ root, const unsigned long long* __restrict__ surv,
                                                          const int32_t* __restrict__ mcnt, const int32_t* __restrict__ mbase, int32_t* __restrict__ mem,
                                                          int32_t* __restrict__ keep, int32_t* __restrict__ cnt, FuseRes* __restrict__ res) {
    if (!res->n_proposals) return;
    const int i = blockIdx.x * FU_BLOCK + threadIdx.x;
    bool gone = false;
    if (i < v.map.n_pts) {
        const int r = root[i];
        const bool k = (int)(surv[r] & 0xffffffffu) == i;
        gone = !k;
        int n = 0;
        if (k) {
            int32_t* run = mem + mbase[r];
            const int nm = mcnt[r];
            sort_run(run, nm);
            n = v.map.src.off[i + 1] - v.map.src.off[i] + fuse_merge(v, i, run, nm, [](int, int) {});
        }
        keep[i] = k; cnt[i] = n;
    }
    wave_count_add(gone, &res->n_absorbed);
}

// every field of every survivor to its new index, its own entries as stored, the merged entries behind them
__global__ __launch_bounds__(FU_BLOCK) void k_fuse_scatter(FuseView v, MapPts dst, const int32_t* __restrict__ root, const unsigned long long* __restrict__ surv,
                                                            const int32_t* __restrict__ mcnt, const int32_t* __restrict__ mbase, const int32_t* __restrict__ mem,
                                                            const int32_t* __restrict__ keep, const int32_t* __restrict__ rank, const int32_t* __restrict__ obase,
                                                            int32_t* __restrict__ into, int32_t* __restrict__ st, const FuseRes* __restrict__ res) {
    if (!res->n_proposals) return;
    const int i = blockIdx.x * FU_BLOCK + threadIdx.x;
    if (i == 0) { dst.off[res->n_points] = res->n_obs; st[ST_NPTS] = res->n_points; st[ST_NOBS] = res->n_obs; }   // (the next call's live counts)
    if (i >= v.map.n_pts) return;
    const int rt = root[i];
    into[i] = rank[(int)(surv[rt] & 0xffffffffu)];
    if (!keep[i]) return;
    const MapPts& src = v.map.src;
    const int r = rank[i], ob = obase[i];
    map_point_copy(src, i, dst, r);
    if (mcnt[rt] > 1) map_life_merge(src, i, mem + mbase[rt], mcnt[rt], dst, r);
    dst.off[r] = ob;
    const int o0 = src.off[i], o1 = src.off[i + 1];
    for (int o = o0; o < o1; o++) { dst.okf[ob + o - o0] = src.okf[o]; dst.okp[ob + o - o0] = src.okp[o]; }
    int at = ob + o1 - o0;
    fuse_merge(v, i, mem + mbase[rt], mcnt[rt], [&](int pos, int kp) { dst.okf[at] = pos; dst.okp[at] = kp; at++; });
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
    if (m->n_pts > INT32_MAX / 2 || (size_t)m->n_obs + gain_bound > (size_t)(INT32_MAX / 2) || np * (size_t)nt > (size_t)INT32_MAX ||
        (size_t)nt * row > (size_t)INT32_MAX)
        return mo_fail(c, MO_ERR_CAPACITY, "map larger than int32 indexing");
    FuseBufs& b = map_feature<FuseBufs>(m);
    int rc;
    const size_t trow = (size_t)nt * row;
    if ((rc = mo_reserve(c, b.rep, np * 32, b.oct, np, b.cell, (size_t)nt * (TK_CELLS + 1), b.sorted, trow, b.tab, trow, b.key, trow, b.prop, np * nt,
                         b.parent, np, b.root, np, b.nval, np, b.surv, np, b.mcnt, np, b.mbase, np, b.mcur, np, b.mem, np, b.into, np, b.res,
                         m->keep, np, m->kobs, np, m->rank, np, m->obase, np)))
        return rc;
    if ((rc = map_pts_reserve(m, m->cur ^ 1, np, (size_t)m->n_obs + gain_bound, false)) || (rc = upload_pos_slot(m))) return rc;
    mo_stage_begin(c);
    HIPCHK(c, hipMemsetAsync(b.res, 0, sizeof(FuseRes), c->stream));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)b.tab.p, INT_MAX, trow, c->stream));
    HIPCHK(c, hipMemsetAsync(b.key, 0xff, trow * 8, c->stream));
    const MapPts dst = m->P[m->cur ^ 1].view();
    const FuseView v{map_view(m), b.prop, b.key, b.tab, lo_pos, nt};
    const FusePrm p{prm->radius, prm->scale_factor, prm->chi2, prm->w, prm->h, prm->max_dist};
    const unsigned pblocks = (unsigned)((np + FU_BLOCK - 1) / FU_BLOCK);
    const int32_t* slots = m->d_pos_slot + lo_pos;
    hipLaunchKernelGGL(k_fuse_prep, dim3(pblocks), dim3(FU_BLOCK), 0, c->stream, v, b.tab, b.nval, b.parent, b.mcnt, b.mcur, b.surv);
    HIPCHK(c, hipGetLastError());
    if ((rc = trk_launch_rep(m, lo_pos, b.rep, b.oct, &b.res.p->n_local)) || (rc = trk_launch_grid(m, slots, 0, nt, prm->w, prm->h, b.cell, b.sorted)))
        return rc;
    mo_stage_mark(c, "fuse_prep");
    if (fprm) {   // the view records of the local points behind k_trk_rep, the centres of the targets with them
        FuseFrustum fr{FrustumPrm{prm->scale_factor, fprm->range_lo, fprm->range_hi, fprm->min_cos, fprm->n_levels}, nullptr, nullptr};
        if ((rc = view_enqueue(m, b.oct, prm->scale_factor, &fr.rec, &fr.centre))) return rc;
        mo_stage_mark(c, "fuse_view");
        hipLaunchKernelGGL(k_fuse_search_frustum, dim3(pblocks, (unsigned)nt), dim3(FU_BLOCK), 0, c->stream, p, fr, v, m->kkps, m->kdesc, m->kP, b.rep, b.oct,
                           b.cell, b.sorted, b.key, b.prop, b.res);
    } else
        hipLaunchKernelGGL(k_fuse_search, dim3(pblocks, (unsigned)nt), dim3(FU_BLOCK), 0, c->stream, p, v, m->kkps, m->kdesc, m->kP, b.rep, b.oct, b.cell,
                           b.sorted, b.key, b.prop, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "fuse_search");
    hipLaunchKernelGGL(k_fuse_resolve, dim3((unsigned)((row + FU_BLOCK - 1) / FU_BLOCK), (unsigned)nt), dim3(FU_BLOCK), 0, c->stream, row, m->kcnt, slots, b.key,
                       b.tab, b.parent, b.res);
    hipLaunchKernelGGL(k_fuse_flatten, dim3(pblocks), dim3(FU_BLOCK), 0, c->stream, (int)np, b.parent, b.nval, b.root, b.mcnt, b.surv, b.res);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, b.mcnt, b.mbase, (int)np, &b.res.p->n_members))) return rc;
    hipLaunchKernelGGL(k_fuse_members, dim3(pblocks), dim3(FU_BLOCK), 0, c->stream, (int)np, b.root, b.mbase, b.mcur, b.mem, b.res);
    hipLaunchKernelGGL(k_fuse_count, dim3(pblocks), dim3(FU_BLOCK), 0, c->stream, v, b.root, b.surv, b.mcnt, b.mbase, b.mem, m->keep, m->kobs, b.res);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, m->keep, m->rank, (int)np, &b.res.p->n_points)) || (rc = map_scan_excl(m, m->kobs, m->obase, (int)np, &b.res.p->n_obs))) return rc;
    hipLaunchKernelGGL(k_fuse_scatter, dim3(pblocks), dim3(FU_BLOCK), 0, c->stream, v, dst, b.root, b.surv, b.mcnt, b.mbase, b.mem, m->keep, m->rank, m->obase,
                       b.into, m->st, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "fuse_merge");
    if ((rc = b.res.download(c))) return rc;
    // (into is read only after a call that fused: the kernel behind the flag leaves it unwritten otherwise, and the identity above stays)
    std::vector<int32_t> into;
    if (out->into) {
        into.resize(np);
        HIPCHK(c, hipMemcpyAsync(into.data(), b.into, np * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = map_sync(c, clk))) return rc;
    const FuseRes& r = b.res.host();
    out->n_targets = nt; out->n_local = r.n_local; out->n_pairs = r.n_pairs; out->n_cand = r.n_cand;
    if (!r.n_proposals) return MO_OK;   // (nothing was written)
    out->n_proposals = r.n_proposals; out->n_gained = r.n_gained; out->n_edges = r.n_edges; out->n_absorbed = r.n_absorbed;
    if (out->into) std::copy(into.begin(), into.end(), out->into);
    m->cur ^= 1;
    m->n_pts = r.n_points; m->n_obs = r.n_obs;
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
