// map_obs.hip -- the two edits of the observation lists of the device map (include/vslam_amd.h): mo_map_add_observations, which gives
// the points the multi-view tracks a bundle adjustment needs, and mo_map_erase_observations, the entry erase, which
// mo_map_bundle_adjust_local also runs behind its write (obs_erase_enqueue / obs_erase_finish, declared in map_store.h).
//
// The entry erase (entry-parallel, no point walks its own list):
//   k_oe_keep      one thread per entry: keep[o] (int32)
//   map_scan_excl  over the n_obs entries: S[o] = the new place of a kept entry, the total = the new n_obs
//   k_oe_points    one thread per point: its fields (map_point_copy) and off[i] = S[off[i]] into the other copy; the points that lost an
//                  entry and hold fewer than two are counted in registers, one integer atomic per workgroup
//   k_oe_entries   one thread per entry: okf / okp of a kept entry to S[o], coalesced reads, ascending writes
// With nothing flagged both kernels return at once and the host does not commit (mo_map_erase_points' behaviour).  The erase shares
// map_store_end and map_commit with the point-parallel rebuilds (map_rebuild.h) and nothing else.
// Added observations:
//   k_obs_claim    one thread per given entry: it claims its point, the lowest entry wins
//   k_obs_count    one thread per point: a claimed point without an observation in kf_pos gains one; its new count (the map's kobs)
//   rebuild_enqueue (map_rebuild.h) with the edit ObsAdd: every point into the other copy, the new observation behind its old ones
#include <climits>

#include "common.h"
#include "map_rebuild.h"   // (map_store.h with it)

#define OBS_BLOCK 256
#define OE_MAX_BLOCKS 2048   // workgroups of k_oe_points (one atomic each)

struct OeRes { int32_t n_obs, n_under; };   // the entries behind the erase or the add; the points an erase left under two

struct ObsEditBufs : MapFeature {
    DevBuf<uint8_t> flag;                             // [n_obs] the caller's erase flags (mo_map_erase_observations)
    DevBuf<int32_t> keep, S;                          // [n_obs] 1 at an entry that stays; its exclusive scan (per entry: the map's keep / rank are per point)
    ResBlock<OeRes> res;
    // mo_map_add_observations
    DevBuf<int32_t> ao_pt, ao_row, ao_claim;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) {
        f(flag); f(keep); f(S); f(res); f(ao_pt); f(ao_row); f(ao_claim);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// entry o leaves where the caller's flag is set (run NULL) or, behind a bundle adjustment, where its final class is 2 and the problem ran
// (*run) and ended with *n_inliers >= min_inliers (a failed adjustment erases nothing)
__global__ __launch_bounds__(OBS_BLOCK) void k_oe_keep(const uint8_t* __restrict__ flag, const int32_t* __restrict__ run, const int32_t* __restrict__ n_inliers,
                                                       int min_inliers, int n_obs, int32_t* __restrict__ keep) {
    const int o = blockIdx.x * OBS_BLOCK + threadIdx.x;
    if (o >= n_obs) return;
    const bool gone = run ? *run && *n_inliers >= min_inliers && flag[o] == 2 : flag[o] != 0;
    keep[o] = !gone;
}

// the place of entry o behind the erase; o == n_obs (the end of the last list): the total
__device__ __forceinline__ int oe_place(const int32_t* __restrict__ S, int o, int n_obs, int total) { return o < n_obs ? S[o] : total; }

// every point's fields and its new offset into the other copy (the points keep their indices); workgroups stride over the points and add
// their count of points that lost an entry and hold fewer than two once
__global__ __launch_bounds__(OBS_BLOCK) void k_oe_points(MapPts src, MapPts dst, int n_pts, int n_obs, const int32_t* __restrict__ S, OeRes* res,
                                                         int32_t* __restrict__ st) {
    __shared__ int sw[OBS_BLOCK / 64];
    const int total = res->n_obs;
    if (total == n_obs) return;   // (nothing leaves: nothing is written, the host does not flip the copies)
    int under = 0;
    for (int i = blockIdx.x * OBS_BLOCK + threadIdx.x; i < n_pts; i += gridDim.x * OBS_BLOCK) {
        const int a = src.off[i], b = src.off[i + 1];
        const int na = oe_place(S, a, n_obs, total), nb = oe_place(S, b, n_obs, total);
        map_point_copy(src, i, dst, i);
        dst.off[i] = na;
        under += nb - na < b - a && nb - na < 2;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) map_store_end(dst, st, n_pts, total);
    under = wave_sum_int(under);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = under;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < OBS_BLOCK / 64; w++) t += sw[w];
        if (t) atomicAdd(&res->n_under, t);
    }
}

// a kept entry's stored bytes at its new place
__global__ __launch_bounds__(OBS_BLOCK) void k_oe_entries(MapPts src, MapPts dst, int n_obs, const int32_t* __restrict__ keep, const int32_t* __restrict__ S,
                                                          const OeRes* __restrict__ res) {
    const int o = blockIdx.x * OBS_BLOCK + threadIdx.x;
    if (o >= n_obs || res->n_obs == n_obs || !keep[o]) return;
    const int d = S[o];
    dst.okf[d] = src.okf[o]; dst.okp[d] = src.okp[o];
}

// keep, S, the result block and the other copy of the store
static int oe_reserve(mo_map* m, ObsEditBufs& b) {
    const size_t np = (size_t)m->n_pts, no = (size_t)m->n_obs;
    if (int rc = mo_reserve(m->c, b.keep, no, b.S, no, b.res)) return rc;
    return map_pts_reserve(m, m->cur ^ 1, np, no, false);   // (not rebuild_reserve: the scans here run over the entries, in keep and S)
}

// keep -> S and the two copies enqueued, the result block's download behind them (behind oe_reserve, the block zeroed in front)
static int oe_enqueue(mo_map* m, ObsEditBufs& b, const uint8_t* flag, const int32_t* run, const int32_t* n_inliers, int min_inliers) {
    mo_ctx* c = m->c;
    const size_t np = (size_t)m->n_pts, no = (size_t)m->n_obs;
    int rc;
    const unsigned oblocks = (unsigned)((no + OBS_BLOCK - 1) / OBS_BLOCK);
    const unsigned pblocks = (unsigned)std::min<size_t>((np + OBS_BLOCK - 1) / OBS_BLOCK, OE_MAX_BLOCKS);
    const MapPts src = m->P[m->cur].view(), dst = m->P[m->cur ^ 1].view();
    hipLaunchKernelGGL(k_oe_keep, dim3(oblocks), dim3(OBS_BLOCK), 0, c->stream, flag, run, n_inliers, min_inliers, (int)no, b.keep);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, b.keep, b.S, (int)no, &b.res.p->n_obs))) return rc;
    hipLaunchKernelGGL(k_oe_points, dim3(pblocks), dim3(OBS_BLOCK), 0, c->stream, src, dst, (int)np, (int)no, b.S, b.res, m->st);
    hipLaunchKernelGGL(k_oe_entries, dim3(oblocks), dim3(OBS_BLOCK), 0, c->stream, src, dst, (int)no, b.keep, b.S, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "obs_erase");
    return b.res.download(c);
}

// behind the synchronisation: the copies flipped, the count taken
static void oe_finish(mo_map* m, const OeRes& r, int32_t* n_erased, int32_t* n_under) {
    const int64_t gone = m->n_obs - r.n_obs;
    if (gone) map_commit(m, m->n_pts, r.n_obs);
    *n_erased = (int32_t)gone; *n_under = r.n_under;
}

int obs_erase_enqueue(mo_map* m, const uint8_t* cls, const int32_t* run, const int32_t* n_inliers, int min_inliers) {
    ObsEditBufs& b = map_feature<ObsEditBufs>(m);
    if (int rc = oe_reserve(m, b)) return rc;
    HIPCHK(m->c, hipMemsetAsync(b.res, 0, sizeof(OeRes), m->c->stream));
    return oe_enqueue(m, b, cls, run, n_inliers, min_inliers);
}
void obs_erase_finish(mo_map* m, int32_t* n_erased, int32_t* n_under) { oe_finish(m, map_feature<ObsEditBufs>(m).res.host(), n_erased, n_under); }

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
    ObsEditBufs& b = map_feature<ObsEditBufs>(m);
    const size_t no = (size_t)m->n_obs;
    if ((rc = mo_reserve(c, b.flag, no)) || (rc = oe_reserve(m, b))) return rc;
    mo_stage_begin(c);
    HIPCHK(c, hipMemsetAsync(b.res, 0, sizeof(OeRes), c->stream));
    HIPCHK(c, hipMemcpyAsync(b.flag, erase, no, hipMemcpyHostToDevice, c->stream));   // (pageable: the runtime stages it before the call returns)
    mo_stage_mark(c, "obs_flags");   // (the upload apart from the rebuild's stage)
    if ((rc = oe_enqueue(m, b, b.flag, nullptr, nullptr, 0)) || (rc = map_sync(c, clk))) return rc;
    oe_finish(m, b.res.host(), &out->n_erased, &out->n_under);
    out->n_obs = m->n_obs;
    return MO_OK;
}

// ---- mo_map_add_observations ------------------------------------------------------------------------------------------------------
// entry i claims its point: the lowest i wins (integer minimum)
__global__ __launch_bounds__(OBS_BLOCK) void k_obs_claim(const int32_t* __restrict__ pt, int n, int n_pts, int32_t* __restrict__ claim) {
    const int i = blockIdx.x * OBS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int p = pt[i];
    if (p >= 0 && p < n_pts) atomicMin(claim + p, i);
}

// one thread per point: a claimed point that has no valid observation in kf_pos yet gains one; cnt = its new observation count
__global__ __launch_bounds__(OBS_BLOCK) void k_obs_count(MapView v, int kf_pos, int32_t* __restrict__ claim, int32_t* __restrict__ cnt) {
    const int i = blockIdx.x * OBS_BLOCK + threadIdx.x;
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

// the add as a rebuild: every point stays at its index with its entries as stored, a claimed point's new observation behind them
struct ObsAdd : RebuildEdit {
    static constexpr bool all_kept = true;
    MapView map; const int32_t* claim; const int32_t* row; int kf_pos; OeRes* res;
    __device__ void tail(int i, const MapPts& dst, int, int at) const {
        const int cl = claim[i];
        if (cl != INT_MAX) { dst.okf[at] = kf_pos; dst.okp[at] = row[cl]; }
    }
};

extern "C" int mo_map_add_observations(mo_map* m, int kf_pos, int n, const int32_t* point, const int32_t* row) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (n < 0 || (n > 0 && (!point || !row))) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const int n_kf = (int)m->pos_slot.size();
    if (kf_pos < 0 || kf_pos > n_kf) return mo_fail(c, MO_ERR_ARG, "kf_pos must be a keyframe position, or the number of keyframes for the next one");
    if (n == 0 || m->n_pts == 0) return MO_OK;
    if (m->n_pts > INT32_MAX / 2 || m->n_obs + n > INT32_MAX / 2) return mo_fail(c, MO_ERR_CAPACITY, "map larger than int32 indexing");
    MAP_ENTER(m);
    ObsEditBufs& b = map_feature<ObsEditBufs>(m);
    const size_t np = (size_t)m->n_pts;
    int rc;
    if ((rc = mo_reserve(c, b.ao_pt, (size_t)n, b.ao_row, (size_t)n, b.ao_claim, np, b.res))) return rc;
    if ((rc = rebuild_reserve(m, np, (size_t)m->n_obs + std::min<size_t>((size_t)n, np)))) return rc;
    if ((rc = upload_pos_slot(m))) return rc;
    HIPCHK(c, hipMemcpyAsync(b.ao_pt, point, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.ao_row, row, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)b.ao_claim, INT_MAX, np, c->stream));
    const MapView v = map_view(m);
    const unsigned pblocks = (unsigned)((np + OBS_BLOCK - 1) / OBS_BLOCK);
    hipLaunchKernelGGL(k_obs_claim, dim3((unsigned)((n + OBS_BLOCK - 1) / OBS_BLOCK)), dim3(OBS_BLOCK), 0, c->stream, b.ao_pt, n, (int)np, b.ao_claim);
    hipLaunchKernelGGL(k_obs_count, dim3(pblocks), dim3(OBS_BLOCK), 0, c->stream, v, kf_pos, b.ao_claim, m->kobs);
    HIPCHK(c, hipGetLastError());
    if ((rc = rebuild_enqueue(m, ObsAdd{{}, v, b.ao_claim, b.ao_row, kf_pos, b.res}, nullptr)) || (rc = b.res.download(c))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    map_commit(m, m->n_pts, b.res.host().n_obs);
    return MO_OK;
}
