// map_kfcull.hip -- ORB-SLAM2's LocalMapping::KeyFrameCulling on the device map and the removal that goes with it (mo_map_kf_redundancy,
// mo_map_erase_keyframes, mo_map_cull_keyframes in include/vslam_amd.h, which states the rules).  The decision reads the map; the erase
// rebuilds the observation arrays into the other copy of the store the way mo_map_add_observations does (count, the map's scan, scatter).
//
//   covis_enqueue   the matrix W (map_covis.hip), in front of everything else in the same chain
//   k_kc_order      one workgroup: row p of W in LDS, the rank of every candidate by counting the larger keys (W << 32) | position (unique,
//                   so the ranks are a permutation), n_points = W[q][q], the list offsets by a block scan over the ranks
//   k_kc_list       the keyframe-side lists: per candidate the (point, own octave) of every point it observes, the octave its first valid
//                   observation's.  Each workgroup counts its points' entries per candidate in LDS, claims one range per candidate with
//                   one global atomic and scatters into it: the order inside a list depends on the run, only sums are taken from it.
//   the walk        candidate after candidate in rank order, each seeing the removals decided before it.  Two carriers, the same integers:
//     k_kc_step       one launch per candidate over many workgroups: launch r settles candidate r - 1 from its finished sum (every
//                     workgroup for itself, workgroup 0 records it) and counts candidate r into a global sum.  The default.
//     k_kc_walk       one workgroup walks the candidates, the removed flags by position in LDS, a barrier per candidate (walk = 1: the
//                     slower one at every size measured, kept as the launches' cross-check in the tests)
//   k_kc_newpos, k_kc_ecount, map_scan_excl, k_kc_escatter   the erase: position -> position after the removal, the surviving valid
//                   observations per point (the map's kobs), their offsets (obase), every field of every point into the other copy.
//                   With no removal decided the last two do nothing and the host does not commit (map_commit of map_rebuild.h).
// Integer atomics only; the one floating-point operation is the f64 compare n_redundant > ratio * n_points.
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "common.h"
#include "map_rebuild.h"   // (map_store.h with it)

#define KC_BLOCK 256
#define KC_WALK_BLOCK 1024
// keyframes the LDS tables of k_kc_order (row of W, n_points), k_kc_list (two counters per candidate) and k_kc_walk (a flag) hold
#define KC_MAX_KF 4096
#define KC_MAX_BLOCKS 1024

struct KcRes { int32_t n_local, n_removed, n_obs; };
struct KcEnt { int32_t pt, oct; };

struct KfCullBufs : MapFeature {
    DevBuf<int32_t> cidx;                        // [n_kf] by position: rank among the candidates (-1: none)
    DevBuf<int32_t> cpos, cw, cnp, cred, crem;   // [n_kf] by rank: position, weight, n_points, n_redundant, removed
    DevBuf<int32_t> lbase, lcur;                 // [n_kf + 1] list offsets by rank; [n_kf] the ranges claimed so far
    DevBuf<KcEnt> list;                          // [observations] the candidates' lists behind each other
    DevBuf<int32_t> rem, newpos;                 // [n_kf] by position: removed; position after the removal (-1: erased)
    DevBuf<uint8_t> protect; PinnedBuf<uint8_t> h_protect;
    PinnedBuf<int32_t> h_rem;                    // [n_kf] rem as the host reads it behind the synchronisation
    ResBlock<KcRes> res;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) {
        f(cidx); f(cpos); f(cw); f(cnp); f(cred); f(crem); f(lbase); f(lcur); f(list); f(rem); f(newpos); f(protect); f(res);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// ---- the decision ----------------------------------------------------------------------------------------------------------------------
// one workgroup of KC_WALK_BLOCK threads, n_kf <= KC_MAX_KF
__global__ __launch_bounds__(KC_WALK_BLOCK) void k_kc_order(const int32_t* __restrict__ W, int n_kf, int p, int min_w, int32_t* __restrict__ cidx,
                                                            int32_t* __restrict__ cpos, int32_t* __restrict__ cw, int32_t* __restrict__ cnp,
                                                            int32_t* __restrict__ cred, int32_t* __restrict__ crem, int32_t* __restrict__ lbase,
                                                            int32_t* __restrict__ lcur, int32_t* __restrict__ rem, KcRes* __restrict__ res) {
    __shared__ int s_w[KC_MAX_KF], s_np[KC_MAX_KF];   // by position: the weight of a candidate (0: none); by rank: n_points
    __shared__ int lw[40];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    if (tid == 0) s_n = 0;
    for (int q = tid; q < n_kf; q += KC_WALK_BLOCK) {
        const int w = W[(size_t)p * n_kf + q];
        s_w[q] = q != p && w >= min_w ? w : 0;
        s_np[q] = 0;
        cred[q] = 0; crem[q] = 0; lcur[q] = 0; rem[q] = 0;
        cpos[q] = -1; cw[q] = 0; cnp[q] = 0;
    }
    __syncthreads();
    int mine = 0;
    for (int q = tid; q < n_kf; q += KC_WALK_BLOCK) {
        const int w = s_w[q];
        int rank = -1;
        if (w) {
            const unsigned long long key = ((unsigned long long)(unsigned)w << 32) | (unsigned)q;   // largest weight, then the later position
            rank = 0;
            for (int o = 0; o < n_kf; o++) rank += (((unsigned long long)(unsigned)s_w[o] << 32) | (unsigned)o) > key && s_w[o];
            const int np = W[(size_t)q * n_kf + q];
            cpos[rank] = q; cw[rank] = w; cnp[rank] = np;
            s_np[rank] = np;
            mine++;
        }
        cidx[q] = rank;
    }
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    const int n_local = s_n;
    int carry = 0;
    for (int b = 0; b < n_local; b += KC_WALK_BLOCK) {
        const int r = b + tid;
        int t;
        const int e = block_excl_scan(r < n_local ? s_np[r] : 0, lw, &t);
        if (r < n_local) lbase[r] = carry + e;
        carry += t;
    }
    if (tid == 0) { lbase[n_local] = carry; res->n_local = n_local; res->n_removed = 0; res->n_obs = 0; }
}

__device__ __forceinline__ int kc_octave(const MapView& v, const mo_keypoint* __restrict__ kkps, int slot, int kp) {
    const int o = kkps[(size_t)slot * v.row + kp].octave;
    return o < 0 ? 0 : o;
}

// f(rank, slot, kp) for the first valid observation of point i at every candidate position
template <class F> __device__ __forceinline__ void kc_each_entry(const MapView& v, int i, const int32_t* __restrict__ cidx, F f) {
    map_each_obs(v, i, [&](int o, int pos, int slot, int kp) {
        const int r = cidx[pos];
        if (r >= 0 && !map_observes(v, i, pos, o)) f(r, slot, kp);
        return false;
    });
}

__global__ __launch_bounds__(KC_BLOCK) void k_kc_list(MapView v, const mo_keypoint* __restrict__ kkps, const int32_t* __restrict__ cidx,
                                                      const int32_t* __restrict__ lbase, int32_t* __restrict__ lcur, KcEnt* __restrict__ list,
                                                      const KcRes* __restrict__ res) {
    __shared__ int s_cnt[KC_MAX_KF], s_base[KC_MAX_KF];
    const int tid = threadIdx.x, n_local = res->n_local;
    if (n_local == 0) return;
    for (int r = tid; r < n_local; r += KC_BLOCK) s_cnt[r] = 0;
    __syncthreads();
    for (int i = blockIdx.x * KC_BLOCK + tid; i < v.n_pts; i += gridDim.x * KC_BLOCK)
        kc_each_entry(v, i, cidx, [&](int r, int, int) { atomicAdd(s_cnt + r, 1); });
    __syncthreads();
    for (int r = tid; r < n_local; r += KC_BLOCK) {
        const int n = s_cnt[r];
        s_base[r] = lbase[r] + (n ? atomicAdd(lcur + r, n) : 0);
        s_cnt[r] = 0;
    }
    __syncthreads();
    for (int i = blockIdx.x * KC_BLOCK + tid; i < v.n_pts; i += gridDim.x * KC_BLOCK)
        kc_each_entry(v, i, cidx, [&](int r, int slot, int kp) {
            list[s_base[r] + atomicAdd(s_cnt + r, 1)] = KcEnt{i, kc_octave(v, kkps, slot, kp)};
        });
}

// the point of entry e of candidate position c is redundant: at least min_obs other positions, none removed(position), observe it validly at
// an octave (of the first valid observation there) <= its own + gap
template <class Rem> __device__ __forceinline__ bool kc_redundant(const MapView& v, const mo_keypoint* __restrict__ kkps, KcEnt e, int c, int gap, int min_obs,
                                                                  Rem removed) {
    const long long lim = (long long)e.oct + gap;
    int n = 0;
    map_each_obs(v, e.pt, [&](int o, int pos, int slot, int kp) {
        if (pos == c || kc_octave(v, kkps, slot, kp) > lim || removed(pos) || map_observes(v, e.pt, pos, o)) return false;
        return ++n >= min_obs;
    });
    return n >= min_obs;
}

// the rule: position 0 and protected positions stay; the compare is f64
__device__ __forceinline__ int kc_rule(int c, const uint8_t* __restrict__ protect, int n_red, int n_pts, double ratio) {
    return c != 0 && !protect[c] && (double)n_red > ratio * (double)n_pts;
}

// one workgroup walks the candidates
__global__ __launch_bounds__(KC_WALK_BLOCK) void k_kc_walk(MapView v, const mo_keypoint* __restrict__ kkps, const int32_t* __restrict__ cpos,
                                                           const int32_t* __restrict__ lbase, const KcEnt* __restrict__ list, const uint8_t* __restrict__ protect,
                                                           int gap, int min_obs, double ratio, int32_t* __restrict__ cred, int32_t* __restrict__ crem,
                                                           int32_t* __restrict__ rem, KcRes* __restrict__ res) {
    __shared__ uint8_t s_rem[KC_MAX_KF];
    __shared__ int s_sum, s_nrem;
    const int tid = threadIdx.x, n_local = res->n_local;
    for (int q = tid; q < v.n_kf; q += KC_WALK_BLOCK) s_rem[q] = 0;
    if (tid == 0) { s_sum = 0; s_nrem = 0; }
    __syncthreads();
    for (int r = 0; r < n_local; r++) {
        const int c = cpos[r], b0 = lbase[r], b1 = lbase[r + 1];
        int cnt = 0;
        for (int e = b0 + tid; e < b1; e += KC_WALK_BLOCK) cnt += kc_redundant(v, kkps, list[e], c, gap, min_obs, [&](int q) { return s_rem[q] != 0; });
        cnt = wave_sum_int(cnt);
        if ((tid & 63) == 0 && cnt) atomicAdd(&s_sum, cnt);
        __syncthreads();
        if (tid == 0) {
            const int sum = s_sum, rm = kc_rule(c, protect, sum, b1 - b0, ratio);
            cred[r] = sum; crem[r] = rm;
            if (rm) { s_rem[c] = 1; s_nrem++; }
            s_sum = 0;
        }
        __syncthreads();
    }
    for (int q = tid; q < v.n_kf; q += KC_WALK_BLOCK) rem[q] = s_rem[q];
    if (tid == 0) res->n_removed = s_nrem;
}

// launch r of the walk by launches (r = 0 .. n_kf - 1, so that r = n_local is among them): candidate r - 1 settled, candidate r counted.
// cred and rem are written by earlier launches, except rem at candidate r - 1's position, which nobody reads here (prev stands for it).
__global__ __launch_bounds__(KC_BLOCK) void k_kc_step(int r, MapView v, const mo_keypoint* __restrict__ kkps, const int32_t* __restrict__ cpos,
                                                      const int32_t* __restrict__ lbase, const KcEnt* __restrict__ list, const uint8_t* __restrict__ protect,
                                                      int gap, int min_obs, double ratio, int32_t* cred, int32_t* __restrict__ crem, int32_t* rem,
                                                      KcRes* res) {
    __shared__ int s_prev_pos, s_prev;
    const int tid = threadIdx.x, n_local = res->n_local;
    if (r > n_local) return;
    if (tid == 0) {
        s_prev_pos = -1; s_prev = 0;
        if (r > 0) {
            const int c = cpos[r - 1];
            const int rm = kc_rule(c, protect, cred[r - 1], lbase[r] - lbase[r - 1], ratio);
            s_prev_pos = c; s_prev = rm;
            if (blockIdx.x == 0) {
                crem[r - 1] = rm;
                if (rm) { rem[c] = 1; atomicAdd(&res->n_removed, 1); }
            }
        }
    }
    __syncthreads();
    if (r == n_local) return;
    const int c = cpos[r], b1 = lbase[r + 1], prev_pos = s_prev_pos, prev = s_prev;
    int cnt = 0;
    for (int e = lbase[r] + blockIdx.x * KC_BLOCK + tid; e < b1; e += gridDim.x * KC_BLOCK)
        cnt += kc_redundant(v, kkps, list[e], c, gap, min_obs, [&](int q) { return q == prev_pos ? prev != 0 : rem[q] != 0; });
    cnt = wave_sum_int(cnt);
    if ((tid & 63) == 0 && cnt) atomicAdd(cred + r, cnt);
}

// ---- the erase -------------------------------------------------------------------------------------------------------------------------
// one workgroup: newpos[q] = q - the removed positions in front of it (-1 at a removed one); their number into res
__global__ __launch_bounds__(KC_WALK_BLOCK) void k_kc_newpos(const int32_t* __restrict__ rem, int n_kf, int32_t* __restrict__ newpos, KcRes* __restrict__ res) {
    __shared__ int lw[40];
    int carry = 0;
    for (int b = 0; b < n_kf; b += KC_WALK_BLOCK) {
        const int q = b + threadIdx.x;
        const int f = q < n_kf && rem[q] != 0;
        int t;
        const int e = block_excl_scan(f, lw, &t);
        if (q < n_kf) newpos[q] = f ? -1 : q - carry - e;
        carry += t;
    }
    if (threadIdx.x == 0) res->n_removed = carry;
}

__global__ __launch_bounds__(KC_BLOCK) void k_kc_ecount(MapView v, const int32_t* __restrict__ newpos, const KcRes* __restrict__ res, int32_t* __restrict__ cnt) {
    const int i = blockIdx.x * KC_BLOCK + threadIdx.x;
    if (i >= v.n_pts) return;
    int n = 0;
    if (res->n_removed) map_each_obs(v, i, [&](int, int pos, int, int) { n += newpos[pos] >= 0; return false; });
    cnt[i] = n;
}

// every field of every point into the other copy; its valid observations at surviving positions, in entry order, as (position after the
// removal, row), both non-negative.  Not k_map_rebuild of map_rebuild.h: under that form kfcull_erase measured 3 - 5 us above the
// parent's runs (0.093 / 0.094 ms against 0.089 / 0.089 at 10^6 points), so the kernel keeps its own text (NOTES.md); it shares
// map_store_end, rebuild_reserve, the map's kobs / obase and map_commit.
__global__ __launch_bounds__(KC_BLOCK) void k_kc_escatter(MapView v, MapPts dst, const int32_t* __restrict__ newpos, const int32_t* __restrict__ base,
                                                          const KcRes* __restrict__ res, int32_t* __restrict__ st) {
    const int i = blockIdx.x * KC_BLOCK + threadIdx.x;
    if (!res->n_removed) return;
    if (i == 0) map_store_end(dst, st, v.n_pts, res->n_obs);
    if (i >= v.n_pts) return;
    const MapPts& src = v.src;
    map_point_copy(src, i, dst, i);
    int at = base[i];
    dst.off[i] = at;
    map_each_obs(v, i, [&](int, int pos, int, int kp) {
        const int np = newpos[pos];
        if (np >= 0) { dst.okf[at] = np; dst.okp[at] = kp; at++; }
        return false;
    });
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static int kc_check(mo_map* m, const mo_map_kfcull_params* prm, const mo_map_kfcull_out* out) {
    mo_ctx* c = m->c;
    if (!prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (prm->min_observers < 1) return mo_fail(c, MO_ERR_ARG, "min_observers must be >= 1");
    if (!std::isfinite(prm->ratio)) return mo_fail(c, MO_ERR_ARG, "ratio must be finite");
    if (prm->walk < 0 || prm->walk > 2) return mo_fail(c, MO_ERR_ARG, "walk must be 0, 1 or 2");
    const int n_kf = (int)m->pos_slot.size();
    if (n_kf > 0 && (prm->kf_pos < -1 || prm->kf_pos >= n_kf)) return mo_fail(c, MO_ERR_ARG, "kf_pos must be -1 or a keyframe position");
    return MO_OK;
}

// W, the order, the lists and the walk enqueued (the position table uploaded and the stage set opened by the caller; at least two
// keyframes and one point)
static int kc_decide_enqueue(mo_map* m, KfCullBufs& b, const mo_map_kfcull_params* prm) {
    mo_ctx* c = m->c;
    const size_t n_kf = m->pos_slot.size();
    int rc;
    if (n_kf > KC_MAX_KF) return mo_fail(c, MO_ERR_CAPACITY, "more keyframes than the keyframe cull's tables hold (" + std::to_string(KC_MAX_KF) + ")");
    if ((rc = mo_reserve(c, b.cidx, n_kf, b.cpos, n_kf, b.cw, n_kf, b.cnp, n_kf, b.cred, n_kf, b.crem, n_kf, b.lbase, n_kf + 1, b.lcur, n_kf, b.rem, n_kf,
                         b.protect, n_kf, b.h_protect, n_kf, b.list, std::max<size_t>((size_t)m->n_obs, 1), b.res)))
        return rc;
    if (prm->protect) std::memcpy(b.h_protect.p, prm->protect, n_kf); else std::memset(b.h_protect.p, 0, n_kf);
    HIPCHK(c, hipMemcpyAsync(b.protect, b.h_protect, n_kf, hipMemcpyHostToDevice, c->stream));
    if ((rc = covis_enqueue(m))) return rc;
    const MapView v = map_view(m);
    const int p = prm->kf_pos < 0 ? (int)n_kf - 1 : prm->kf_pos;
    hipLaunchKernelGGL(k_kc_order, dim3(1), dim3(KC_WALK_BLOCK), 0, c->stream, covis_weights(m), (int)n_kf, p, std::max(prm->min_weight, 1), b.cidx, b.cpos, b.cw,
                       b.cnp, b.cred, b.crem, b.lbase, b.lcur, b.rem, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "kfcull_order");
    const unsigned blocks = (unsigned)std::min<int64_t>((m->n_pts + KC_BLOCK - 1) / KC_BLOCK, KC_MAX_BLOCKS);
    hipLaunchKernelGGL(k_kc_list, dim3(blocks), dim3(KC_BLOCK), 0, c->stream, v, m->kkps, b.cidx, b.lbase, b.lcur, b.list, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "kfcull_list");
    // walk = 0 takes the launches: 4.5 to 80 times faster than the one workgroup at every size of profiles/kfcull_rate.txt (its 16 wavefronts
    // cannot hide the dependent loads of the observation walks)
    const size_t per_list = (size_t)m->n_obs / n_kf;   // (an estimate: the launches stride over whatever the lists hold)
    const bool steps = prm->walk != 1;
    if (steps) {
        const unsigned sblocks = (unsigned)std::min<size_t>((2 * per_list + KC_BLOCK - 1) / KC_BLOCK + 1, KC_MAX_BLOCKS);
        for (int r = 0; r < (int)n_kf; r++)
            hipLaunchKernelGGL(k_kc_step, dim3(sblocks), dim3(KC_BLOCK), 0, c->stream, r, v, m->kkps, b.cpos, b.lbase, b.list, b.protect, prm->scale_gap,
                               prm->min_observers, prm->ratio, b.cred, b.crem, b.rem, b.res);
    } else {
        hipLaunchKernelGGL(k_kc_walk, dim3(1), dim3(KC_WALK_BLOCK), 0, c->stream, v, m->kkps, b.cpos, b.lbase, b.list, b.protect, prm->scale_gap, prm->min_observers,
                           prm->ratio, b.cred, b.crem, b.rem, b.res);
    }
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, steps ? "kfcull_steps" : "kfcull_walk");
    return MO_OK;
}

// the rebuild for the flags in b.rem enqueued, with the copies the host needs behind it: the result block and the flags
static int kc_erase_enqueue(mo_map* m, KfCullBufs& b) {
    mo_ctx* c = m->c;
    const size_t n_kf = m->pos_slot.size(), np = (size_t)m->n_pts;
    int rc;
    if ((rc = b.newpos.reserve(c, n_kf))) return rc;
    const MapView v = map_view(m);
    const unsigned pblocks = (unsigned)((np + KC_BLOCK - 1) / KC_BLOCK);
    hipLaunchKernelGGL(k_kc_newpos, dim3(1), dim3(KC_WALK_BLOCK), 0, c->stream, b.rem, (int)n_kf, b.newpos, b.res);
    hipLaunchKernelGGL(k_kc_ecount, dim3(pblocks), dim3(KC_BLOCK), 0, c->stream, v, b.newpos, b.res, m->kobs);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, m->kobs, m->obase, (int)np, &b.res.p->n_obs))) return rc;
    hipLaunchKernelGGL(k_kc_escatter, dim3(pblocks), dim3(KC_BLOCK), 0, c->stream, v, m->P[m->cur ^ 1].view(), b.newpos, m->obase, b.res, m->st);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "kfcull_erase");
    HIPCHK(c, hipMemcpyAsync(b.h_rem, b.rem, n_kf * 4, hipMemcpyDeviceToHost, c->stream));
    return MO_OK;
}

// behind the synchronisation: the copies flipped, the position table shortened
static void kc_erase_finish(mo_map* m, KfCullBufs& b) {
    const KcRes& r = b.res.host();
    if (!r.n_removed) return;
    map_commit(m, m->n_pts, r.n_obs);
    for (int q = (int)m->pos_slot.size() - 1; q >= 0; q--)
        if (b.h_rem.p[q]) m->pos_slot.erase(m->pos_slot.begin() + q);
}

static int kc_cull(mo_map* m, const mo_map_kfcull_params* prm, mo_map_kfcull_out* out, bool erase) {
    mo_ctx* c = m->c;
    int rc;
    if ((rc = kc_check(m, prm, out))) return rc;
    out->n_local = 0; out->n_removed = 0; out->n_obs = m->n_obs;
    const size_t n_kf = m->pos_slot.size();
    if (n_kf < 2 || m->n_pts == 0) return MO_OK;
    if ((rc = map_int32_guard(m))) return rc;
    MAP_ENTER(m);
    HostClock clk(c);
    KfCullBufs& b = map_feature<KfCullBufs>(m);
    if (erase && ((rc = rebuild_reserve(m, (size_t)m->n_pts, (size_t)m->n_obs)) || (rc = b.h_rem.reserve(c, n_kf)))) return rc;
    if ((rc = upload_pos_slot(m))) return rc;
    mo_stage_begin(c);
    if ((rc = kc_decide_enqueue(m, b, prm))) return rc;
    if (erase && (rc = kc_erase_enqueue(m, b))) return rc;
    if ((rc = b.res.download(c))) return rc;
    int32_t* const dst[5] = {out->pos, out->weight, out->n_points, out->n_redundant, out->removed};
    const int32_t* const src[5] = {b.cpos, b.cw, b.cnp, b.cred, b.crem};
    for (int k = 0; k < 5; k++)
        if (dst[k]) HIPCHK(c, hipMemcpyAsync(dst[k], src[k], n_kf * 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = map_sync(c, clk))) return rc;
    const KcRes& r = b.res.host();
    out->n_local = r.n_local; out->n_removed = r.n_removed;
    if (erase) kc_erase_finish(m, b);
    out->n_obs = m->n_obs;
    return MO_OK;
}

extern "C" int mo_map_kf_redundancy(mo_map* m, const mo_map_kfcull_params* prm, mo_map_kfcull_out* out) {
    if (!m) return MO_ERR_ARG;
    return kc_cull(m, prm, out, false);
}

extern "C" int mo_map_cull_keyframes(mo_map* m, const mo_map_kfcull_params* prm, mo_map_kfcull_out* out) {
    if (!m) return MO_ERR_ARG;
    return kc_cull(m, prm, out, prm && prm->erase != 0);
}

extern "C" int mo_map_erase_keyframes(mo_map* m, const int32_t* positions, int n) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (n < 0 || (n > 0 && !positions)) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const size_t n_kf = m->pos_slot.size();
    for (int i = 0; i < n; i++)
        if (positions[i] < 0 || (size_t)positions[i] >= n_kf) return mo_fail(c, MO_ERR_ARG, "keyframe position out of range");
    if (n == 0) return MO_OK;
    int rc;
    if (m->n_pts == 0) {   // nothing to rebuild: the position table alone
        std::vector<uint8_t> gone(n_kf, 0);
        for (int i = 0; i < n; i++) gone[positions[i]] = 1;
        for (int q = (int)n_kf - 1; q >= 0; q--)
            if (gone[q]) m->pos_slot.erase(m->pos_slot.begin() + q);
        return MO_OK;
    }
    if ((rc = map_int32_guard(m))) return rc;
    MAP_ENTER(m);
    HostClock clk(c);
    KfCullBufs& b = map_feature<KfCullBufs>(m);
    if ((rc = rebuild_reserve(m, (size_t)m->n_pts, (size_t)m->n_obs)) || (rc = mo_reserve(c, b.rem, n_kf, b.h_rem, n_kf, b.res)) ||
        (rc = upload_pos_slot(m)))
        return rc;
    std::memset(b.h_rem.p, 0, n_kf * 4);
    for (int i = 0; i < n; i++) b.h_rem.p[positions[i]] = 1;
    mo_stage_begin(c);
    HIPCHK(c, hipMemcpyAsync(b.rem, b.h_rem, n_kf * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = kc_erase_enqueue(m, b)) || (rc = b.res.download(c))) return rc;
    if ((rc = map_sync(c, clk))) return rc;
    kc_erase_finish(m, b);
    return MO_OK;
}
