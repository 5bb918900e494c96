// map_merge.h -- what the fusion of duplicate points (map_fuse.hip) and the correction of a loop (map_correct.hip) share: the search of
// the local points in the target keyframes and the merge stages behind it, on the device and on the host.  The build has no
// relocatable device code: the kernels here are templates, instantiated in each of the two files.
//
// A feature brings a parameter block Prm (radius, sf, chi2, w, h, max_dist are read here), a result block Res (n_pairs, n_cand,
// n_proposals, n_gained, n_edges, n_absorbed, n_points, n_obs, n_members are read or written here) and a view (by value) with the
// fields map, prop, key, n_targets and, as inline members, the four places where the two features differ:
//   pos_of(t)               the keyframe position of target t
//   owner(t, r)             the point that owns row r of target t before the search's gains (INT_MAX: a free row)
//   surv_key(i, nval, oct)  point i's key for its component's survivor: the lowest key survives (static)
//   direct(j, &pos, &row)   the gain member j holds ahead of its searched gains, if any
//   any(res)                the call fuses something: the gate of every kernel behind the resolve, and of the host's flip (static)
// FuseView (map_fuse.hip) and CrView (map_correct.hip) are the two views.
//
// The stages (merge_enqueue launches them in this order; every kernel reads its gate first and returns when nothing fuses):
//   k_merge_search   one thread per (point, target): pair test, projection under the stored P, window over the cells, 256-bit Hamming
//                    distances, the chi2 gate; the accepted keypoint is claimed by a 64-bit atomicMin of (dist << 32) | point
//   k_merge_resolve  one thread per (target, row): the winner of a claimed row against the row's owner: a gained observation, or a merge
//                    edge hooked into the lock-free union-find (the larger root under the smaller by atomicCAS)
//   k_merge_flatten  one thread per point: its root (= the lowest index of its component), the component's size and survivor (atomicMin
//                    of surv_key)
//   map_scan_excl + k_merge_members   the members of every component next to each other
//   k_merge_count    one thread per point: survivors sort their members by index and count their merged list
//   map_scan_excl x 2 + k_merge_scatter   new indices and offsets; every field of every survivor into the other copy
// Integer atomics only (minima, sums, a compare-and-swap whose outcome - the component's lowest index - is the same in any order):
// equal maps give equal bytes.  Private to the library.
#pragma once
#include <climits>
#include <vector>

#include "common.h"
#include "map_store.h"
#include "map_rebuild.h"
#include "map_search.h"
#include "ba.h"   // ba_info

#define MG_BLOCK 256
#define FU_MAX_TARGETS 16384   // grid.y of the search; also what the per-keyframe list sort holds (map_kernels.hip)

// The buffers both features name alike.  Each feature embeds one (its own instance: nothing passes from one call to the next); tab
// stays with the feature, because its extent differs.
struct MergeBufs {
    DevBuf<uint8_t> rep;                  // [point][32] representative descriptors
    DevBuf<int32_t> oct;                  // [point] ref_octave (TK_NOT_LOCAL: not among the points that are searched)
    DevBuf<int32_t> cell, sorted;         // [target][TK_CELLS + 1], [target][row]: the keypoint grids
    DevBuf<unsigned long long> key;       // [target][row] (dist << 32) | point of the claim on each keypoint
    DevBuf<int32_t> prop;                 // [target][point] the row each pair proposed (-1: none)
    DevBuf<int32_t> parent, root, nval;   // [point] union-find, flattened root, valid observations
    DevBuf<unsigned long long> surv;      // [point] at a root: the survivor's key
    DevBuf<int32_t> mcnt, mbase, mcur, mem;   // [point] members per root, their first entry, scatter cursors, the member lists
    DevBuf<int32_t> into;                 // [point] new index of the point each old point now is
    int reserve(mo_ctx* c, size_t np, size_t nt, size_t row) {
        return mo_reserve(c, rep, np * 32, oct, np, cell, nt * (TK_CELLS + 1), sorted, nt * row, key, nt * row, prop, np * nt, parent, np, root, np,
                          nval, np, surv, np, mcnt, np, mbase, np, mcur, np, mem, np, into, np);
    }
    template <class F> void each_scratch(F f) {
        f(rep); f(oct); f(cell); f(sorted); f(key); f(prop); f(parent); f(root); f(nval); f(surv); f(mcnt); f(mbase); f(mcur); f(mem); f(into);
    }
};

// what the frustum mode (mo_map_fuse_frustum) adds to the search's arguments (by value): the view records of the local points and the
// camera centres of the keyframe positions (map_view_geom.hip)
struct FuseFrustum {
    FrustumPrm f;
    const ViewRec* rec;
    const double* centre;
};

// point i's entries of the union-find and survivor tables as every call starts them
__device__ __forceinline__ void merge_reset(int i, int32_t* __restrict__ parent, int32_t* __restrict__ mcnt, int32_t* __restrict__ mcur,
                                            unsigned long long* __restrict__ surv) {
    parent[i] = i; mcnt[i] = 0; mcur[i] = 0; surv[i] = TK_NONE;
}

// one thread per (point, target): the pair's proposal.  FR = false is the plain search (fr unused); FR = true: a candidate also lies
// in the point's frustum seen from the target's centre, and is searched at its predicted level L with the octave gate [L - 1, L].
template <bool FR, class View, class Prm, class Res>
__device__ __forceinline__ void merge_search(const Prm& prm, const View& v, const mo_keypoint* __restrict__ kkps, const uint8_t* __restrict__ kdesc,
                                             const double* __restrict__ kP, const uint8_t* __restrict__ rep, const int32_t* __restrict__ oct,
                                             const int32_t* __restrict__ cell, const int32_t* __restrict__ sorted, unsigned long long* __restrict__ key,
                                             int32_t* __restrict__ prop, Res* __restrict__ res, const FuseFrustum* fr) {
    const int t = blockIdx.y, i = blockIdx.x * MG_BLOCK + threadIdx.x;
    const MapView& mv = v.map;
    const int pos = v.pos_of(t), slot = mv.pos_slot[pos];
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

template <class View, class Prm, class Res>
__global__ __launch_bounds__(MG_BLOCK) void k_merge_search(Prm prm, View v, const mo_keypoint* __restrict__ kkps, const uint8_t* __restrict__ kdesc,
                                                           const double* __restrict__ kP, const uint8_t* __restrict__ rep, const int32_t* __restrict__ oct,
                                                           const int32_t* __restrict__ cell, const int32_t* __restrict__ sorted,
                                                           unsigned long long* __restrict__ key, int32_t* __restrict__ prop, Res* __restrict__ res) {
    merge_search<false>(prm, v, kkps, kdesc, kP, rep, oct, cell, sorted, key, prop, res, nullptr);
}

__device__ __forceinline__ int merge_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// lock-free union: the larger of the two roots is hooked under the smaller; a lost race is retried from the new roots.  parent[x] <= x
// always, so every walk ends, and the root of a finished component is its lowest index whatever the order of the hooks.
__device__ __forceinline__ void merge_unite(int32_t* parent, int a, int b) {
    for (;;) {
        for (int p; (p = merge_load(parent + a)) != a;) a = p;
        for (int p; (p = merge_load(parent + b)) != b;) b = p;
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(parent + hi, hi, lo) == hi) return;
    }
}

// one thread per (target, row): the row's winner against its owner (its gate is the search's alone: only a proposal claims a row)
template <class View, class Res>
__global__ __launch_bounds__(MG_BLOCK) void k_merge_resolve(View v, const int32_t* __restrict__ slots, int32_t* __restrict__ parent, Res* __restrict__ res) {
    if (!res->n_proposals) return;
    const int t = blockIdx.y, r = blockIdx.x * MG_BLOCK + threadIdx.x;
    bool gain = false, edge = false;
    if (r < v.map.row && r < v.map.kcnt[slots[t]]) {
        const unsigned long long k = v.key[(size_t)t * v.map.row + r];
        if (k != TK_NONE) {
            const int owner = v.owner(t, r);
            gain = owner == INT_MAX;
            edge = !gain;
            if (edge) merge_unite(parent, (int)(k & 0xffffffffu), owner);
        }
    }
    wave_count_add(gain, &res->n_gained);
    wave_count_add(edge, &res->n_edges);
}

template <class View, class Res>
__global__ __launch_bounds__(MG_BLOCK) void k_merge_flatten(int n_pts, const int32_t* __restrict__ parent, const int32_t* __restrict__ nval,
                                                            const int32_t* __restrict__ oct, int32_t* __restrict__ root, int32_t* __restrict__ mcnt,
                                                            unsigned long long* __restrict__ surv, const Res* __restrict__ res) {
    if (!View::any(res)) return;
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= n_pts) return;
    int r = i;
    for (int p; (p = parent[r]) != r;) r = p;
    root[i] = r;
    atomicAdd(mcnt + r, 1);
    atomicMin(surv + r, View::surv_key(i, nval[i], oct[i]));
}

template <class View, class Res>
__global__ __launch_bounds__(MG_BLOCK) void k_merge_members(int n_pts, const int32_t* __restrict__ root, const int32_t* __restrict__ mbase,
                                                            int32_t* __restrict__ mcur, int32_t* __restrict__ mem, const Res* __restrict__ res) {
    if (!View::any(res)) return;
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= n_pts) return;
    const int r = root[i];
    mem[mbase[r] + atomicAdd(mcur + r, 1)] = i;   // (arrival order: the survivor sorts its run)
}

// the gained observation of point j at target t by the search: the row it proposed, won, and that nothing owns
template <class View> __device__ __forceinline__ bool merge_gained(const View& v, int j, int t, int* r) {
    const int pr = v.prop[(size_t)t * v.map.n_pts + j];
    if (pr < 0) return false;
    if ((int)(v.key[(size_t)t * v.map.row + pr] & 0xffffffffu) != j || v.owner(t, pr) != INT_MAX) return false;
    *r = pr;
    return true;
}

// The candidate entries of survivor s with members mem[0 .. nm) (ascending) in the order of the merged list: (0) its own valid
// entries, (1) the valid entries of the other members, (2) the gained observations of all members by member: its direct gain, then
// the search's by target.  f(index, kind, position, row) -> true stops the walk.
template <class View, class F> __device__ __forceinline__ void merge_walk(const View& v, int s, const int32_t* __restrict__ mem, int nm, F f) {
    int idx = 0, dpos, kp;
    bool stop = false;
    map_each_obs(v.map, s, [&](int, int pos, int, int r) { return stop = f(idx++, 0, pos, r); });
    for (int a = 0; a < nm && !stop; a++)
        if (mem[a] != s) map_each_obs(v.map, mem[a], [&](int, int pos, int, int r) { return stop = f(idx++, 1, pos, r); });
    for (int a = 0; a < nm && !stop; a++) {
        if (v.direct(mem[a], &dpos, &kp) && f(idx++, 2, dpos, kp)) return;
        for (int t = 0; t < v.n_targets; t++)
            if (merge_gained(v, mem[a], t, &kp) && f(idx++, 2, v.pos_of(t), kp)) return;
    }
}

// The merged list of survivor s behind its own entries: an entry of kinds 1 and 2 is kept when no earlier candidate stands at its
// position (a dropped one was dropped for a holder of that position before it, so "an earlier candidate" and "the list already holds a
// valid observation there" are the same).  emit(position, row) per kept entry; returns their number.
template <class View, class E> __device__ __forceinline__ int merge_list(const View& v, int s, const int32_t* __restrict__ mem, int nm, E emit) {
    int n = 0;
    merge_walk(v, s, mem, nm, [&](int idx, int kind, int pos, int kp) {
        if (kind == 0) return false;
        bool held = false;
        merge_walk(v, s, mem, nm, [&](int idx2, int, int pos2, int) {
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
template <class View, class Res>
__global__ __launch_bounds__(MG_BLOCK) void k_merge_count(View v, const int32_t* __restrict__ root, const unsigned long long* __restrict__ surv,
                                                          const int32_t* __restrict__ mcnt, const int32_t* __restrict__ mbase, int32_t* __restrict__ mem,
                                                          int32_t* __restrict__ keep, int32_t* __restrict__ cnt, Res* __restrict__ res) {
    if (!View::any(res)) return;
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
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
            n = v.map.src.off[i + 1] - v.map.src.off[i] + merge_list(v, i, run, nm, [](int, int) {});
        }
        keep[i] = k; cnt[i] = n;
    }
    wave_count_add(gone, &res->n_absorbed);
}

// every field of every survivor to its new index, its own entries as stored, the merged entries behind them.  Not k_map_rebuild of
// map_rebuild.h: under that form the correction's merge stage measured 0.115 / 0.130 ms against 0.103 / 0.106 (10^5 points) and 0.215 /
// 0.203 against 0.181 / 0.167 (10^6), so the kernel keeps its own text (NOTES.md); it shares map_store_end, rebuild_reserve and map_commit.
template <class View, class Res>
__global__ __launch_bounds__(MG_BLOCK) void k_merge_scatter(View v, MapPts dst, const int32_t* __restrict__ root, const unsigned long long* __restrict__ surv,
                                                            const int32_t* __restrict__ mcnt, const int32_t* __restrict__ mbase, const int32_t* __restrict__ mem,
                                                            const int32_t* __restrict__ keep, const int32_t* __restrict__ rank, const int32_t* __restrict__ obase,
                                                            int32_t* __restrict__ into, int32_t* __restrict__ st, const Res* __restrict__ res) {
    if (!View::any(res)) return;
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i == 0) map_store_end(dst, st, res->n_points, res->n_obs);
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
    merge_list(v, i, mem + mbase[rt], mcnt[rt], [&](int pos, int kp) { dst.okf[at] = pos; dst.okp[at] = kp; at++; });
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// the int32 bounds of the kernels' indices for a call over nt targets whose point_of table has tab_n entries (no fewer than nt rows of
// the keyframe store) and that gains at most gain_bound observations
inline int merge_int32_guard(mo_map* m, size_t nt, size_t tab_n, size_t gain_bound) {
    return m->n_pts > INT32_MAX / 2 || (size_t)m->n_obs + gain_bound > (size_t)(INT32_MAX / 2) || (size_t)m->n_pts * nt > (size_t)INT32_MAX ||
                   tab_n > (size_t)INT32_MAX
               ? mo_fail(m->c, MO_ERR_CAPACITY, "map larger than int32 indexing")
               : MO_OK;
}

// room for such a call: the shared buffers, the map's compaction scratch, the other copy of the store; the position table uploaded
inline int merge_reserve(mo_map* m, MergeBufs& g, size_t nt, size_t gain_bound) {
    mo_ctx* c = m->c;
    const size_t np = (size_t)m->n_pts;
    int rc;
    if ((rc = g.reserve(c, np, nt, (size_t)m->row)) || (rc = rebuild_reserve(m, np, (size_t)m->n_obs + gain_bound))) return rc;
    return upload_pos_slot(m);
}

// the stages from the resolve to the scatter, enqueued behind the feature's search; slots [target] on the device
template <class View, class Res> int merge_enqueue(mo_map* m, const View& v, MergeBufs& g, const int32_t* slots, ResBlock<Res>& res, const char* mark) {
    mo_ctx* c = m->c;
    const int np = v.map.n_pts, row = v.map.row;
    const dim3 pgrid((unsigned)((np + MG_BLOCK - 1) / MG_BLOCK)), block(MG_BLOCK);
    int rc;
    hipLaunchKernelGGL((k_merge_resolve<View, Res>), dim3((unsigned)((row + MG_BLOCK - 1) / MG_BLOCK), (unsigned)v.n_targets), block, 0, c->stream, v, slots,
                       g.parent, res);
    hipLaunchKernelGGL((k_merge_flatten<View, Res>), pgrid, block, 0, c->stream, np, g.parent, g.nval, g.oct, g.root, g.mcnt, g.surv, res);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, g.mcnt, g.mbase, np, &res.p->n_members))) return rc;
    hipLaunchKernelGGL((k_merge_members<View, Res>), pgrid, block, 0, c->stream, np, g.root, g.mbase, g.mcur, g.mem, res);
    hipLaunchKernelGGL((k_merge_count<View, Res>), pgrid, block, 0, c->stream, v, g.root, g.surv, g.mcnt, g.mbase, g.mem, m->keep, m->kobs, res);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, m->keep, m->rank, np, &res.p->n_points)) || (rc = map_scan_excl(m, m->kobs, m->obase, np, &res.p->n_obs))) return rc;
    hipLaunchKernelGGL((k_merge_scatter<View, Res>), pgrid, block, 0, c->stream, v, m->P[m->cur ^ 1].view(), g.root, g.surv, g.mcnt, g.mbase, g.mem, m->keep, m->rank,
                       m->obase, g.into, m->st, res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, mark);
    return MO_OK;
}

// The end of the chain: the result block and, if asked for, `into` copied out, the one synchronisation; when the call fused, into
// handed over, the store flipped and the map's sizes set.  into is read only after a call that fused: the kernel behind the gate leaves
// it unwritten otherwise, and the identity the caller preset stays.
template <class View, class Res> int merge_finish(mo_map* m, MergeBufs& g, ResBlock<Res>& res, HostClock& clk, int32_t* out_into, bool* fused) {
    mo_ctx* c = m->c;
    const size_t np = (size_t)m->n_pts;
    int rc;
    if ((rc = res.download(c))) return rc;
    std::vector<int32_t> into;
    if (out_into) {
        into.resize(np);
        HIPCHK(c, hipMemcpyAsync(into.data(), g.into, np * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = map_sync(c, clk))) return rc;
    const Res& r = res.host();
    *fused = View::any(&r);
    if (!*fused) return MO_OK;   // (nothing was written to the other copy: the store is not flipped)
    if (out_into) std::copy(into.begin(), into.end(), out_into);
    map_commit(m, r.n_points, r.n_obs);
    return MO_OK;
}
