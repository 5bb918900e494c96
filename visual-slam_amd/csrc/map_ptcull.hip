// map_ptcull.hip -- the life of a map point on the device map: ORB-SLAM2's mnVisible / mnFound counters fed from a tracked frame
// (mo_map_note_tracking), LocalMapping::MapPointCulling decided from them (mo_map_points_bad), and the removal of points that leaves the map
// the survivors alone would have built (mo_map_erase_points, mo_map_cull_points); mo_map_point_life reads the records.
// include/vslam_amd.h states the rules, tests/ptcull_restatement.py restates them.  The record itself lives in the store (map_store.h:
// map_life_new, map_point_copy, map_life_merge) and travels through every rebuild.
//
//   note      k_pc_local    one thread per point: local-map membership, as the view kernels read it (0 / TK_NOT_LOCAL)
//             view_enqueue  (frustum only) the view records of the local points, as mo_map_track_frustum computes them
//             k_pc_match    one thread per frame keypoint: atomicOr of matched / hit into its point's flag word
//             k_pc_note     one thread per point: seen (trk_project, trk_frustum), the flags, the record updated once
//   decide    k_pc_decide   one thread per point: age, the positions that observe it, the reason, keep and the kept entry count
//   erase     k_pc_flags    (mo_map_erase_points) keep and the kept entry count from the caller's mask
//             rebuild_enqueue (map_rebuild.h) with the edit PcErase: survivors in order into the other copy, entries as stored; remap.
//             With nothing removed the rebuild writes remap alone and the host does not commit.
// Integer atomics on flags and counts only, never on a record; the one floating-point decision is the f64 compare found < ratio * visible.
#include <climits>
#include <cmath>

#include "common.h"
#include "map_rebuild.h"   // (map_store.h with it)
#include "map_search.h"
#include "pnp.h"

#define PC_BLOCK 256
// workgroups of the per-point kernels: they stride over the points and add their counts to the result block once per workgroup.  One
// atomic per wavefront on a handful of addresses was what these kernels cost at 10^6 points (profiles/ptcull_rate.txt).
#define PC_MAX_BLOCKS 2048
enum { PC_MATCHED = 1, PC_HIT = 2 };

struct PcRes {
    int32_t n_local, n_seen, n_matched, n_found;      // note
    int32_t n_tested, n_removed, n_reason[4];         // decide (n_removed: erase too)
    int32_t n_points, n_obs;                          // erase: the survivors and their entries
};

struct PtCullBufs : MapFeature {
    DevBuf<int32_t> oct;                              // [point] 0 at a local point, TK_NOT_LOCAL elsewhere
    DevBuf<uint8_t> lmask;                            // [n_kf] the caller's local positions
    DevBuf<int32_t> qpt; DevBuf<uint8_t> qinl;        // [n_q] the tracked frame's matches
    DevBuf<int32_t> flags;                            // [point] PC_MATCHED | PC_HIT
    DevBuf<uint8_t> mask;                             // [point] protect (decide) or remove (erase), the caller's
    DevBuf<uint8_t> reason, removed;                  // [point]
    DevBuf<int32_t> remap;                            // [point]
    ResBlock<PcRes> res;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) { f(oct); f(lmask); f(qpt); f(qinl); f(flags); f(mask); f(reason); f(removed); f(remap); f(res); }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// the workgroup's sums of c[0 .. N) added to first[0 .. N), consecutive counters of the result block: one atomic per counter and workgroup
// (every thread calls it, once)
template <int N> __device__ __forceinline__ void pc_block_add(const int (&c)[N], int32_t* __restrict__ first) {
    __shared__ int s[PC_BLOCK / 64][N];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < N; k++) {
        const int t = wave_sum_int(c[k]);
        if (lane == 0) s[wv][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        int t = 0;
        for (int w = 0; w < PC_BLOCK / 64; w++) t += s[w][threadIdx.x];
        if (t) atomicAdd(first + threadIdx.x, t);
    }
}

// ---- note ------------------------------------------------------------------------------------------------------------------------------
struct NotePrm {
    double K[9], pose[12];
    int w, h;
};

// local: a valid observation at a position >= lo_pos, or with MASK at a position whose byte of lmask is not zero (k_trk_rep's membership)
template <bool MASK> __global__ __launch_bounds__(PC_BLOCK) void k_pc_local(MapView v, int lo_pos, const uint8_t* __restrict__ lmask, int32_t* __restrict__ oct,
                                                                            int32_t* __restrict__ flags, PcRes* __restrict__ res) {
    int c[1] = {0};
    for (int i = blockIdx.x * PC_BLOCK + threadIdx.x; i < v.n_pts; i += gridDim.x * PC_BLOCK) {
        bool local = false;
        map_each_obs(v, i, [&](int, int pos, int, int) { return local = MASK ? lmask[pos] != 0 : pos >= lo_pos; });
        oct[i] = local ? 0 : TK_NOT_LOCAL;
        flags[i] = 0;
        c[0] += local;
    }
    pc_block_add(c, &res->n_local);
}

__global__ __launch_bounds__(PC_BLOCK) void k_pc_match(int n_q, const int32_t* __restrict__ qpt, const uint8_t* __restrict__ qinl, int n_pts,
                                                       int32_t* __restrict__ flags) {
    const int q = blockIdx.x * PC_BLOCK + threadIdx.x;
    if (q >= n_q) return;
    const int p = qpt[q];
    if (p >= 0 && p < n_pts) atomicOr(flags + p, qinl[q] ? PC_MATCHED | PC_HIT : PC_MATCHED);
}

// FRUSTUM: a seen point also passes trk_frustum from the pose's centre (rec: view_enqueue's records)
template <bool FRUSTUM> __global__ __launch_bounds__(PC_BLOCK) void k_pc_note(NotePrm prm, FrustumPrm fp, const ViewRec* __restrict__ rec, MapPts src, int n_pts,
                                                                              const int32_t* __restrict__ oct, const int32_t* __restrict__ flags,
                                                                              PcRes* __restrict__ res) {
    int c[3] = {0, 0, 0};   // n_seen, n_matched, n_found
    double R[9], t[3], P[12];
    pose_split(prm.pose, R, t);
    pnp_projection(prm.K, R, t, P);
    for (int i = blockIdx.x * PC_BLOCK + threadIdx.x; i < n_pts; i += gridDim.x * PC_BLOCK) {
        bool seen = false;
        if (oct[i] != TK_NOT_LOCAL) {
            double u, v;
            const double X = src.xyz[(size_t)i * 3], Y = src.xyz[(size_t)i * 3 + 1], Z = src.xyz[(size_t)i * 3 + 2];
            seen = trk_project(P, X, Y, Z, prm.w, prm.h, &u, &v);
            if (FRUSTUM && seen) {
                double C[3];
                int lv;
                trk_centre(R, t, C);
                seen = trk_frustum(fp, rec[i], C, X, Y, Z, &lv);
            }
        }
        const int f = flags[i];
        const bool matched = (f & PC_MATCHED) != 0, hit = (f & PC_HIT) != 0;
        c[0] += seen; c[1] += matched; c[2] += hit;
        if (seen || matched) {   // once per point and call (the record saturates at INT32_MAX)
            int4 l = src.life[i];
            if (l.x < INT32_MAX) l.x++;
            if (hit && l.y < INT32_MAX) l.y++;
            src.life[i] = l;
        }
    }
    pc_block_add(c, &res->n_seen);
}

// ---- decide ----------------------------------------------------------------------------------------------------------------------------
struct DecidePrm {
    double ratio;
    int min_age, max_age, max_obs, orphan_obs, now;
};

__global__ __launch_bounds__(PC_BLOCK) void k_pc_decide(MapView v, DecidePrm prm, const uint8_t* __restrict__ protect, uint8_t* __restrict__ reason,
                                                        uint8_t* __restrict__ removed, int32_t* __restrict__ keep, int32_t* __restrict__ cnt,
                                                        PcRes* __restrict__ res) {
    int c[6] = {0, 0, 0, 0, 0, 0};   // n_tested, n_removed, n_reason[4]
    for (int i = blockIdx.x * PC_BLOCK + threadIdx.x; i < v.n_pts; i += gridDim.x * PC_BLOCK) {
        const int4 l = v.src.life[i];
        const long long age = (long long)prm.now - l.z;
        const bool tested = prm.max_age < 0 || age <= prm.max_age;
        int n_obs = 0;   // the positions that observe it: the first valid entry per position counts
        map_each_obs(v, i, [&](int o, int pos, int, int) { n_obs += !map_observes(v, i, pos, o); return false; });
        int why = 0;
        if (tested && (double)l.y < prm.ratio * (double)l.x) why = 1;
        else if (tested && age >= prm.min_age && n_obs <= prm.max_obs) why = 2;
        else if (n_obs <= prm.orphan_obs) why = 3;
        const bool gone = why && !protect[i];
        reason[i] = (uint8_t)why; removed[i] = gone;
        keep[i] = !gone; cnt[i] = gone ? 0 : v.src.off[i + 1] - v.src.off[i];
        c[0] += tested; c[1] += gone;
        for (int k = 0; k < 4; k++) c[2 + k] += why == k;
    }
    pc_block_add(c, &res->n_tested);
}

// ---- erase -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_BLOCK) void k_pc_flags(MapPts src, int n_pts, const uint8_t* __restrict__ remove, int32_t* __restrict__ keep,
                                                       int32_t* __restrict__ cnt, PcRes* __restrict__ res) {
    int c[1] = {0};
    for (int i = blockIdx.x * PC_BLOCK + threadIdx.x; i < n_pts; i += gridDim.x * PC_BLOCK) {
        const bool gone = remove[i] != 0;
        keep[i] = !gone; cnt[i] = gone ? 0 : src.off[i + 1] - src.off[i];
        c[0] += gone;
    }
    pc_block_add(c, &res->n_removed);
}

// the erase as a rebuild: remap of every point in front of the gate (a call that removes nothing still returns the identity); with a
// removal, every survivor's fields and its entries as stored at its new index
struct PcErase : RebuildEdit {
    static constexpr bool side_first = true;
    MapView map; PcRes* res; int32_t* remap;
    __device__ bool changed() const { return res->n_removed != 0; }
    __device__ void side_first_out(int i, bool kept, int r) const { remap[i] = kept ? r : -1; }
};

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static unsigned pc_blocks(size_t n) { return (unsigned)((n + PC_BLOCK - 1) / PC_BLOCK); }
static unsigned pc_stride_blocks(size_t n) { return std::min<unsigned>(pc_blocks(n), PC_MAX_BLOCKS); }

extern "C" int mo_map_point_life(mo_map* m, int32_t* life, int64_t* now) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!now || (m->n_pts > 0 && !life)) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    MAP_ENTER(m);
    *now = map_now(m);
    if (m->n_pts > 0) HIPCHK(c, hipMemcpyAsync(life, m->P[m->cur].life, (size_t)m->n_pts * sizeof(int4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MO_OK;
}

extern "C" int mo_map_note_tracking(mo_map* m, const double K[9], const double pose[12], const mo_map_note_params* prm, int32_t n_q, const int32_t* point,
                                    const uint8_t* inlier, mo_map_note_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!K || !pose || !prm || !out || n_q < 0 || (n_q > 0 && (!point || !inlier))) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(K[i])) return mo_fail(c, MO_ERR_ARG, "K must be finite");
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(pose[i])) return mo_fail(c, MO_ERR_ARG, "pose must be finite");
    if (prm->w <= 0 || prm->h <= 0) return mo_fail(c, MO_ERR_ARG, "w and h must be > 0");
    if (prm->window < 0) return mo_fail(c, MO_ERR_ARG, "window must be >= 0");
    if (!(prm->scale_factor > 0.0) || !std::isfinite(prm->scale_factor)) return mo_fail(c, MO_ERR_ARG, "scale_factor must be finite and > 0");
    const mo_map_frustum_params* fprm = prm->frustum;
    if (fprm && (fprm->n_levels < 1 || !std::isfinite(fprm->range_lo) || !std::isfinite(fprm->range_hi) || !std::isfinite(fprm->min_cos)))
        return mo_fail(c, MO_ERR_ARG, "n_levels must be >= 1, range_lo, range_hi and min_cos finite");
    out->n_local = out->n_seen = out->n_matched = out->n_found = 0;
    const int n_kf = (int)m->pos_slot.size();
    if (n_kf == 0 || m->n_pts == 0) return MO_OK;   // (nothing to note: not an error)
    int rc;
    if ((rc = map_int32_guard(m))) return rc;
    MAP_ENTER(m);
    HostClock clk(c);
    PtCullBufs& b = map_feature<PtCullBufs>(m);
    const size_t np = (size_t)m->n_pts;
    if ((rc = mo_reserve(c, b.oct, np, b.flags, np, b.lmask, (size_t)n_kf, b.qpt, (size_t)std::max(n_q, 1), b.qinl, (size_t)std::max(n_q, 1), b.res)) ||
        (rc = upload_pos_slot(m)))
        return rc;
    mo_stage_begin(c);
    HIPCHK(c, hipMemsetAsync(b.res, 0, sizeof(PcRes), c->stream));
    if (prm->local_mask) HIPCHK(c, hipMemcpyAsync(b.lmask, prm->local_mask, (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
    if (n_q) {
        HIPCHK(c, hipMemcpyAsync(b.qpt, point, (size_t)n_q * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b.qinl, inlier, (size_t)n_q, hipMemcpyHostToDevice, c->stream));
    }
    const MapView v = map_view(m);
    if (prm->local_mask)
        hipLaunchKernelGGL(k_pc_local<true>, dim3(pc_stride_blocks(np)), dim3(PC_BLOCK), 0, c->stream, v, 0, b.lmask, b.oct, b.flags, b.res);
    else
        hipLaunchKernelGGL(k_pc_local<false>, dim3(pc_stride_blocks(np)), dim3(PC_BLOCK), 0, c->stream, v, map_window_lo(prm->window, n_kf), nullptr, b.oct, b.flags,
                           b.res);
    if (n_q) hipLaunchKernelGGL(k_pc_match, dim3(pc_blocks((size_t)n_q)), dim3(PC_BLOCK), 0, c->stream, n_q, b.qpt, b.qinl, (int)np, b.flags);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "note_flags");
    NotePrm p;
    for (int i = 0; i < 9; i++) p.K[i] = K[i];
    for (int i = 0; i < 12; i++) p.pose[i] = pose[i];
    p.w = prm->w; p.h = prm->h;
    if (fprm) {
        const ViewRec* rec;
        const double* centre;
        if ((rc = view_enqueue(m, b.oct, prm->scale_factor, &rec, &centre))) return rc;
        mo_stage_mark(c, "note_view");
        const FrustumPrm fp{prm->scale_factor, fprm->range_lo, fprm->range_hi, fprm->min_cos, fprm->n_levels};
        hipLaunchKernelGGL(k_pc_note<true>, dim3(pc_stride_blocks(np)), dim3(PC_BLOCK), 0, c->stream, p, fp, rec, v.src, (int)np, b.oct, b.flags, b.res);
    } else
        hipLaunchKernelGGL(k_pc_note<false>, dim3(pc_stride_blocks(np)), dim3(PC_BLOCK), 0, c->stream, p, FrustumPrm{}, nullptr, v.src, (int)np, b.oct, b.flags, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "note_apply");
    if ((rc = b.res.download(c)) || (rc = map_sync(c, clk))) return rc;
    const PcRes& r = b.res.host();
    out->n_local = r.n_local; out->n_seen = r.n_seen; out->n_matched = r.n_matched; out->n_found = r.n_found;
    return MO_OK;
}

static int pc_check(mo_map* m, const mo_map_ptcull_params* prm, const mo_map_ptcull_out* out) {
    mo_ctx* c = m->c;
    if (!prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (!std::isfinite(prm->ratio)) return mo_fail(c, MO_ERR_ARG, "ratio must be finite");
    if (prm->min_age < 0) return mo_fail(c, MO_ERR_ARG, "min_age must be >= 0");
    return MO_OK;
}

static int pc_cull(mo_map* m, const mo_map_ptcull_params* prm, mo_map_ptcull_out* out, bool erase) {
    mo_ctx* c = m->c;
    int rc;
    if ((rc = pc_check(m, prm, out))) return rc;
    out->n_tested = out->n_removed = 0;
    for (int k = 0; k < 4; k++) out->n_reason[k] = 0;
    out->now = map_now(m); out->n_points = m->n_pts; out->n_obs = m->n_obs;
    if (m->n_pts == 0) return MO_OK;   // (nothing is written)
    if ((rc = map_int32_guard(m))) return rc;
    MAP_ENTER(m);
    HostClock clk(c);
    PtCullBufs& b = map_feature<PtCullBufs>(m);
    const size_t np = (size_t)m->n_pts;
    if ((rc = mo_reserve(c, b.mask, np, b.reason, np, b.removed, np, b.remap, np, b.res)) ||
        (rc = erase ? rebuild_reserve(m, np, (size_t)m->n_obs) : mo_reserve(c, m->keep, np, m->kobs, np)) || (rc = upload_pos_slot(m)))
        return rc;
    mo_stage_begin(c);
    HIPCHK(c, hipMemsetAsync(b.res, 0, sizeof(PcRes), c->stream));
    if (prm->protect) HIPCHK(c, hipMemcpyAsync(b.mask, prm->protect, np, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(b.mask, 0, np, c->stream));
    const DecidePrm p{prm->ratio, prm->min_age, prm->max_age, prm->max_obs, prm->orphan_obs, map_now(m)};
    hipLaunchKernelGGL(k_pc_decide, dim3(pc_stride_blocks(np)), dim3(PC_BLOCK), 0, c->stream, map_view(m), p, b.mask, b.reason, b.removed, m->keep, m->kobs, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "ptcull_decide");
    if (erase && (rc = rebuild_enqueue(m, PcErase{{}, map_view(m), b.res, b.remap}, "ptcull_erase"))) return rc;
    if ((rc = b.res.download(c))) return rc;
    if (out->reason) HIPCHK(c, hipMemcpyAsync(out->reason, b.reason, np, hipMemcpyDeviceToHost, c->stream));
    if (out->removed) HIPCHK(c, hipMemcpyAsync(out->removed, b.removed, np, hipMemcpyDeviceToHost, c->stream));
    if (erase && out->remap) HIPCHK(c, hipMemcpyAsync(out->remap, b.remap, np * 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = map_sync(c, clk))) return rc;
    const PcRes& r = b.res.host();
    out->n_tested = r.n_tested; out->n_removed = r.n_removed;
    for (int k = 0; k < 4; k++) out->n_reason[k] = r.n_reason[k];
    if (erase && r.n_removed) map_commit(m, r.n_points, r.n_obs);
    out->n_points = m->n_pts; out->n_obs = m->n_obs;
    return MO_OK;
}

extern "C" int mo_map_points_bad(mo_map* m, const mo_map_ptcull_params* prm, mo_map_ptcull_out* out) {
    if (!m) return MO_ERR_ARG;
    return pc_cull(m, prm, out, false);
}

extern "C" int mo_map_cull_points(mo_map* m, const mo_map_ptcull_params* prm, mo_map_ptcull_out* out) {
    if (!m) return MO_ERR_ARG;
    return pc_cull(m, prm, out, prm && prm->erase != 0);
}

extern "C" int mo_map_erase_points(mo_map* m, const uint8_t* remove, int32_t* remap, mo_map_pterase_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!out || (m->n_pts > 0 && !remove)) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    out->n_removed = 0; out->n_points = m->n_pts; out->n_obs = m->n_obs;
    if (m->n_pts == 0) return MO_OK;
    int rc;
    if ((rc = map_int32_guard(m))) return rc;
    MAP_ENTER(m);
    HostClock clk(c);
    PtCullBufs& b = map_feature<PtCullBufs>(m);
    const size_t np = (size_t)m->n_pts;
    if ((rc = mo_reserve(c, b.mask, np, b.remap, np, b.res)) || (rc = rebuild_reserve(m, np, (size_t)m->n_obs))) return rc;
    mo_stage_begin(c);
    HIPCHK(c, hipMemsetAsync(b.res, 0, sizeof(PcRes), c->stream));
    HIPCHK(c, hipMemcpyAsync(b.mask, remove, np, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_pc_flags, dim3(pc_stride_blocks(np)), dim3(PC_BLOCK), 0, c->stream, m->P[m->cur].view(), (int)np, b.mask, m->keep, m->kobs, b.res);
    HIPCHK(c, hipGetLastError());
    if ((rc = rebuild_enqueue(m, PcErase{{}, map_view(m), b.res, b.remap}, "ptcull_erase")) || (rc = b.res.download(c))) return rc;
    if (remap) HIPCHK(c, hipMemcpyAsync(remap, b.remap, np * 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = map_sync(c, clk))) return rc;
    const PcRes& r = b.res.host();
    out->n_removed = r.n_removed;
    if (r.n_removed) map_commit(m, r.n_points, r.n_obs);
    out->n_points = m->n_pts; out->n_obs = m->n_obs;
    return MO_OK;
}
