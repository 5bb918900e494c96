// map_rebuild.h -- the rebuild of the map store that every edit of the points or of their observation lists ends in.  The one kernel
// serves the point erase (map_ptcull.hip) and the added observations (map_obs.hip), its per-point move the cull chain of
// mo_map_add_keyframe (map_kernels.hip); the keyframe erase (map_kfcull.hip) and the merge of fusion and loop correction (map_merge.h)
// keep scatter kernels of their own, which measured faster than the shared form (their comments have the figures), and share the rest:
// map_store_end, rebuild_reserve, the map's scratch, map_commit.  The build has no relocatable device code: the kernel here is a
// template, instantiated in each file that has an edit.
//
// A feature decides per point, into the map's scratch: keep[i] (unless every point stays) and kobs[i], the entries point i will hold.
// The rest is here: rebuild_reserve (that scratch and the other copy of the store), rebuild_enqueue (map_scan_excl over keep and kobs,
// k_map_rebuild, the stage mark) and, behind the synchronisation, map_commit (the flip of the copies and the sizes; a call that changed
// nothing does not commit, and its kernel wrote nothing to the other copy).
//
// The feature's edit (by value, derived from RebuildEdit) answers what differs, as inline members; there is no run-time flag:
//   map                      the live map (MapView)
//   res                      the feature's result block on the device: n_points and n_obs take the scans' totals and are read back by
//                            the kernel as the new sizes (all_kept: n_points is not asked for, the points keep their number)
//   changed()                the gate: false leaves the other copy and st untouched.  RebuildEdit's: always
//   all_kept                 (static) every point stays at its index: keep and rank are not read and no rank scan runs (the add)
//   side_first_out(i, kept, r)   only with side_first (static) set: a per-point output, also of the points that do not survive, written
//                            in front of the gate, so that a call that changes nothing still writes it (remap); point i stays (kept)
//                            at index r.  RebuildEdit has no default: the flag without the hook fails where the kernel is instantiated
//   entries(src, i, o0, o1, dst, ob)   the stored entries of point i (o0 .. o1 - 1) from place ob on; returns the place behind them.
//                            RebuildEdit's: as stored
//   tail(i, dst, r, at)      what follows them from place `at` on (the add's claimed entry).  RebuildEdit's: none
// The entry erase of map_obs.hip is entry-parallel (a third faster at 10^6 points) and takes map_store_end and map_commit alone;
// k_grow_append and k_map_append add points in place and take map_store_end.  Private to the library.
#pragma once
#include "map_store.h"

#define RB_BLOCK 256

// the end of a rebuilt or grown store: the last offset, and the live counts the next call's chain starts from
__device__ __forceinline__ void map_store_end(const MapPts& dst, int32_t* __restrict__ st, int n_pts, int n_obs) { dst.off[n_pts] = n_obs; st[ST_NPTS] = n_pts; st[ST_NOBS] = n_obs; }

// the stored entries o0 .. o1 - 1 as they are, from place ob on; also(place) per entry; returns the place behind them
template <class A> __device__ __forceinline__ int map_entries_copy(const MapPts& src, int o0, int o1, const MapPts& dst, int ob, A also) {
    for (int o = o0; o < o1; o++) { dst.okf[ob + o - o0] = src.okf[o]; dst.okp[ob + o - o0] = src.okp[o]; also(ob + o - o0); }
    return ob + o1 - o0;
}

// what an edit answers when it has nothing to say
struct RebuildEdit {
    static constexpr bool all_kept = false, side_first = false;
    __device__ __forceinline__ int entries(const MapPts& src, int, int o0, int o1, const MapPts& dst, int ob) const {
        return map_entries_copy(src, o0, o1, dst, ob, [](int) {});
    }
    __device__ __forceinline__ void tail(int, const MapPts&, int, int) const {}
    __device__ __forceinline__ bool changed() const { return true; }
};

// point i of src at index r of dst, its list from place ob on: what every rebuild does once it knows the three
template <class Edit> __device__ __forceinline__ void map_point_move(const Edit& e, const MapPts& src, int i, const MapPts& dst, int r, int ob) {
    map_point_copy(src, i, dst, r);
    const int o0 = src.off[i], o1 = src.off[i + 1];   // (read in front of the store: for all the compiler knows the two copies alias)
    dst.off[r] = ob;
    e.tail(i, dst, r, e.entries(src, i, o0, o1, dst, ob));
}

// one thread per point of the live map
template <class Edit>
__global__ __launch_bounds__(RB_BLOCK) void k_map_rebuild(Edit e, MapPts dst, const int32_t* __restrict__ keep, const int32_t* __restrict__ rank,
                                                          const int32_t* __restrict__ obase, int32_t* __restrict__ st) {
    const MapView& v = e.map;
    const int i = blockIdx.x * RB_BLOCK + threadIdx.x;
    // the gate and the new sizes are read in front of every store (scalar loads); the gate is tested behind side_first_out
    const bool changed = e.changed();
    const int n_obs = e.res->n_obs;
    int n_pts = v.n_pts, r = i;
    bool kept = true;
    if constexpr (!Edit::all_kept) n_pts = e.res->n_points;
    auto place = [&] { if constexpr (!Edit::all_kept) { kept = keep[i] != 0; r = rank[i]; } };   // point i's part of the kept set
    if constexpr (Edit::side_first) { if (i >= v.n_pts) return; place(); e.side_first_out(i, kept, r); }   // (a map with points: thread 0 passes)
    if (!changed) return;
    if (i == 0) map_store_end(dst, st, n_pts, n_obs);
    if constexpr (!Edit::side_first) { if (i >= v.n_pts) return; place(); }
    if (kept) map_point_move(e, v.src, i, dst, r, obase[i]);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// room for a rebuild of the live map into new_pts_bound points and new_obs_bound entries at most: the map's four scratch arrays (per
// point of either side) and the other copy of the store
inline int rebuild_reserve(mo_map* m, size_t new_pts_bound, size_t new_obs_bound) {
    const size_t np = std::max((size_t)m->n_pts, new_pts_bound);
    if (int rc = mo_reserve(m->c, m->keep, np, m->kobs, np, m->rank, np, m->obase, np)) return rc;
    return map_pts_reserve(m, m->cur ^ 1, new_pts_bound, new_obs_bound, false);
}

// keep / kobs -> rank / obase and the scatter into the other copy enqueued, the stage marked under the caller's name (NULL: no mark)
template <class Edit> int rebuild_enqueue(mo_map* m, const Edit& e, const char* mark) {
    mo_ctx* c = m->c;
    const int np = e.map.n_pts;
    if constexpr (!Edit::all_kept)
        if (int rc = map_scan_excl(m, m->keep, m->rank, np, &e.res->n_points)) return rc;
    if (int rc = map_scan_excl(m, m->kobs, m->obase, np, &e.res->n_obs)) return rc;
    hipLaunchKernelGGL(k_map_rebuild<Edit>, dim3((unsigned)((np + RB_BLOCK - 1) / RB_BLOCK)), dim3(RB_BLOCK), 0, c->stream, e, m->P[m->cur ^ 1].view(), m->keep,
                       m->rank, m->obase, m->st);
    HIPCHK(c, hipGetLastError());
    if (mark) mo_stage_mark(c, mark);
    return MO_OK;
}

// behind the synchronisation of a chain that changed the store: the other copy is the map
inline void map_commit(mo_map* m, int64_t n_pts, int64_t n_obs) { m->cur ^= 1; m->n_pts = n_pts; m->n_obs = n_obs; }
