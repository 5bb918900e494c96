// map_loop.hip -- loop candidates on the device map (mo_map_loop_candidates in include/vslam_amd.h): ORB-SLAM2's
// KeyFrameDatabase::DetectLoopCandidates on the keyframe database of bow.hip and the covisibility matrix of map_covis.hip, then the
// map-point matching that opens ComputeSim3.  Read-only on the map; tests/loop_restatement.py restates every rule in numpy.
// Chain: database update (bow_update_enqueue) -> k_covis (covis_enqueue) -> scores and common words in one pass over the database rows
// (bow_loop_score_enqueue) -> k_loop_select -> point_of table -> knn-2 matching of the asking keyframe against the candidates
// (match_launch_pairs; k_loop_select wrote the pair list, pairs past the candidates name the empty frame) -> k_loop_claim / k_loop_gather
// -> copy-out.  One synchronisation.
//
//   k_loop_select   one workgroup of 1024, any number of keyframes in tiles of its size: connected(p), min_score and max_common (two
//                   block reductions, LDS atomics on the bit patterns: scores are >= 0, so their order is the order of the patterns);
//                   the sets S and M; a wavefront per keyframe of M: n_best rounds of the largest (W << 32) | position below the last one
//                   taken (k_covis_select's walk), the f64 adds in that order; the retain test; per best_k the largest acc that names it
//                   (atomicMax on the bit pattern); the rank of a candidate = the candidates before it, counted against tiles of 1024
//                   keys in LDS (k_bow_rank's way); the groups.
//   k_loop_claim    a thread per (candidate, query row): a passing match with two different map points claims its train row with
//                   atomicMin of (distance << 32) | query row.
//   k_loop_gather   the same threads again: the row that holds the claim keeps the match.
// Integer atomics only (minima and maxima commute): two calls on equal maps give the same bytes.  -ffp-contract=off (Makefile): the
// adds and the one multiply round as the restatement's.
#include <climits>
#include <cstring>

#include "common.h"
#include "bow.h"
#include "map_store.h"

#define LP_BLOCK 1024
#define LP_MAX_CAND 16
#define LP_NONE 0xffffffffffffffffull

struct LoopRes {
    double min_score, acc[LP_MAX_CAND], score[LP_MAX_CAND];
    int32_t cand[LP_MAX_CAND], n_match[LP_MAX_CAND];
    int32_t n_cand, n_found, n_connected, max_common, n_scored, n_passed;
};

struct LoopBufs : MapFeature {
    DevBuf<uint8_t> flag;                     // [n_kf] bit 0: in S, bit 1: in M
    DevBuf<double> acc;                       // [n_kf] accumulated group score of a keyframe of M
    DevBuf<int32_t> best;                     // [n_kf] best_k
    DevBuf<unsigned long long> cacc;          // [n_kf] bit pattern of the largest retained acc that names the position, 0: not a candidate
    DevBuf<uint8_t> connected, group;         // [n_kf], [max_cand][n_kf]
    DevBuf<int32_t> qf, tf;                   // [LP_MAX_CAND] the matcher's pair list
    DevBuf<int32_t> tab;                      // point_of [position][row] (map_launch_point_of)
    MatchBufs match;                          // [pair][row]
    DevBuf<unsigned long long> claim;         // [pair][row] per train row: (distance << 32) | query row of the match that keeps it
    DevBuf<int32_t> cur, mpt, mrow;           // [row], [pair][row], [pair][row]
    DevBuf<uint8_t> among;                    // [n_kf] mo_map_loop_candidates_among's mask as uploaded
    ResBlock<LoopRes> res;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) {
        f(flag); f(acc); f(best); f(cacc); f(connected); f(group); f(qf); f(tf); f(tab); match.each_scratch(f); f(claim); f(cur); f(mpt); f(mrow); f(among); f(res);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

__device__ __forceinline__ unsigned long long lp_load(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one workgroup.  flag, acc and best are written with plain stores and read behind a barrier by the same workgroup; cacc is cleared
// with plain stores in the first phase and, three barriers later, written by atomicMax and read by lp_load only
__global__ __launch_bounds__(LP_BLOCK) void k_loop_select(const double* __restrict__ score, const int32_t* __restrict__ common, const int32_t* __restrict__ W,
                                                          int n_kf, int p, int min_w, int n_best, int max_cand, const int32_t* __restrict__ pos_slot,
                                                          int empty, uint8_t* flag, double* acc, int32_t* best, unsigned long long* cacc,
                                                          uint8_t* __restrict__ connected, uint8_t* __restrict__ group, int32_t* __restrict__ sel_qf,
                                                          int32_t* __restrict__ sel_tf, LoopRes* __restrict__ res) {
    __shared__ unsigned long long s_key[LP_BLOCK];
    __shared__ unsigned long long s_min, s_top;
    __shared__ int s_n[5];   // connected, max_common, scored, passed, found
    __shared__ int s_cand[LP_MAX_CAND];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) {
        s_min = (unsigned long long)__double_as_longlong(1.0); s_top = 0;
        for (int i = 0; i < 5; i++) s_n[i] = 0;
    }
    if (tid < LP_MAX_CAND) {
        s_cand[tid] = -1;
        res->cand[tid] = -1; res->acc[tid] = 0.0; res->score[tid] = 0.0; res->n_match[tid] = 0;
        sel_qf[tid] = empty; sel_tf[tid] = empty;
    }
    __syncthreads();
    // connected(p), min_score, max_common
    {
        unsigned long long mn = LP_NONE;
        int nc = 0, mc = 0;
        for (int k = tid; k < n_kf; k += LP_BLOCK) {
            const bool conn = k != p && W[(size_t)p * n_kf + k] >= min_w;
            connected[k] = conn || k == p;
            cacc[k] = 0;
            if (conn) {
                const unsigned long long b = (unsigned long long)__double_as_longlong(score[k]);
                if (b < mn) mn = b;
                nc++;
            }
            mc = max(mc, common[k]);
        }
        if (nc) { atomicMin(&s_min, mn); atomicAdd(&s_n[0], nc); }
        if (mc) atomicMax(&s_n[1], mc);
    }
    __syncthreads();
    const double min_score = __longlong_as_double((long long)s_min);
    const int max_common = s_n[1], floor_c = (4 * max_common) / 5;
    // S and M
    {
        int ns = 0, nm = 0;
        for (int k = tid; k < n_kf; k += LP_BLOCK) {
            const bool in_s = common[k] > floor_c, in_m = in_s && score[k] >= min_score;
            flag[k] = (uint8_t)((in_s ? 1 : 0) | (in_m ? 2 : 0));
            ns += in_s; nm += in_m;
        }
        if (ns) atomicAdd(&s_n[2], ns);
        if (nm) atomicAdd(&s_n[3], nm);
    }
    __syncthreads();
    // the group of every keyframe of M: a wavefront each
    for (int k = wv; k < n_kf; k += LP_BLOCK / 64) {
        if (!(flag[k] & 2)) continue;   // (wave-uniform)
        double a = score[k], bs = a;
        int b = k;
        unsigned long long last = LP_NONE;
        for (int t = 0; t < n_best; t++) {
            unsigned long long bk = 0;
            for (int q = lane; q < n_kf; q += 64) {
                const int w = W[(size_t)k * n_kf + q];
                if (q == k || w < min_w) continue;
                const unsigned long long key = ((unsigned long long)(unsigned)w << 32) | (unsigned)q;   // largest weight, then the later position
                if (key < last && key > bk) bk = key;
            }
            for (int d = 32; d; d >>= 1) {
                const unsigned long long o = __shfl_xor(bk, d, 64);
                if (o > bk) bk = o;
            }
            if (!bk) break;
            const int q = (int)(bk & 0xffffffffu);
            if (flag[q] & 1) {
                const double sq = score[q];
                a = a + sq;
                if (sq > bs) { bs = sq; b = q; }
            }
            last = bk;
        }
        if (lane == 0) {
            acc[k] = a; best[k] = b;
            atomicMax(&s_top, (unsigned long long)__double_as_longlong(a));
        }
    }
    __syncthreads();
    // retained, and per best_k the largest acc that names it
    const double keep = 0.75 * __longlong_as_double((long long)s_top);
    for (int k = tid; k < n_kf; k += LP_BLOCK)
        if ((flag[k] & 2) && acc[k] > keep) atomicMax(cacc + best[k], (unsigned long long)__double_as_longlong(acc[k]));
    __syncthreads();
    // the candidates ranked: the larger acc first, ties to the lower position
    for (int base = 0; base < n_kf; base += LP_BLOCK) {
        const int k = base + tid;
        const unsigned long long my = k < n_kf ? lp_load(cacc + k) : 0;
        int r = 0;
        for (int t0 = 0; t0 < n_kf; t0 += LP_BLOCK) {
            __syncthreads();
            s_key[tid] = t0 + tid < n_kf ? lp_load(cacc + t0 + tid) : 0;
            __syncthreads();
            const int lim = min(LP_BLOCK, n_kf - t0);
            if (my)
#pragma unroll 8
                for (int j = 0; j < lim; j++) {   // (wave-uniform j: broadcast reads)
                    const unsigned long long kj = s_key[j];
                    r += (kj > my) || (kj == my && t0 + j < k);
                }
        }
        if (my) {
            atomicAdd(&s_n[4], 1);
            if (r < max_cand) {
                s_cand[r] = k;
                res->cand[r] = k; res->acc[r] = __longlong_as_double((long long)my); res->score[r] = score[k];
                sel_qf[r] = pos_slot[p]; sel_tf[r] = pos_slot[k];
            }
        }
    }
    __syncthreads();
    const int n_cand = min(s_n[4], max_cand);
    for (int c = 0; c < n_cand; c++) {
        const int ck = s_cand[c];
        for (int q = tid; q < n_kf; q += LP_BLOCK) group[(size_t)c * n_kf + q] = q == ck || W[(size_t)ck * n_kf + q] >= min_w;
    }
    if (tid == 0) {
        res->min_score = min_score;
        res->n_cand = n_cand; res->n_found = s_n[4]; res->n_connected = s_n[0]; res->max_common = max_common;
        res->n_scored = s_n[2]; res->n_passed = s_n[3];
    }
}

// lp_match restates map_match_point's rule (map_store.h) instead of calling it, and k_loop_claim / k_loop_gather keep their pointer tails
// instead of a MatchView: behind the shared function the compiler merges the four refusals into one sentinel test where this form
// leaves the lane at each of them (k_loop_claim 103 -> 119 instructions, k_loop_gather 148 -> 155; profiles/map_features_isa.txt).
// A change to the rule is made in both places.
// the match of query row i of pair c that counts: *j its train row, *b the candidate's map point there, *key its claim; a = cur_point[i]
__device__ __forceinline__ bool lp_match(int c, int i, int row, int a, int ck, const int32_t* __restrict__ midx, const int32_t* __restrict__ mdist,
                                         const uint8_t* __restrict__ mpass, const int32_t* __restrict__ tab, int* j, int* b, unsigned long long* key) {
    const size_t o = (size_t)c * row + i;
    if (a < 0 || !mpass[o]) return false;
    const int t = midx[2 * o];
    if (t < 0) return false;
    const int pb = tab[(size_t)ck * row + t];
    if (pb == INT_MAX || pb == a) return false;
    *j = t; *b = pb;
    *key = ((unsigned long long)(unsigned)mdist[2 * o] << 32) | (unsigned)i;
    return true;
}

// grid (query rows / 256, max(max_cand, 1)); cur_point by the blocks of pair 0
__global__ __launch_bounds__(256) void k_loop_claim(const int32_t* __restrict__ cnt, int q_slot, int p, int row, const int32_t* __restrict__ midx,
                                                    const int32_t* __restrict__ mdist, const uint8_t* __restrict__ mpass, const int32_t* __restrict__ tab,
                                                    const LoopRes* __restrict__ res, int32_t* __restrict__ cur, unsigned long long* __restrict__ claim) {
    const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(cnt[q_slot], row)) return;
    const int t = tab[(size_t)p * row + i], a = t == INT_MAX ? -1 : t;
    if (c == 0) cur[i] = a;
    if (c >= res->n_cand) return;
    int j, b;
    unsigned long long key;
    if (lp_match(c, i, row, a, res->cand[c], midx, mdist, mpass, tab, &j, &b, &key)) atomicMin(claim + (size_t)c * row + j, key);
}

// grid (query rows / 256, max_cand); mpt and mrow arrive as -1, res->n_match as 0
__global__ __launch_bounds__(256) void k_loop_gather(const int32_t* __restrict__ cnt, int q_slot, int p, int row, const int32_t* __restrict__ midx,
                                                     const int32_t* __restrict__ mdist, const uint8_t* __restrict__ mpass, const int32_t* __restrict__ tab,
                                                     const unsigned long long* __restrict__ claim, LoopRes* __restrict__ res, int32_t* __restrict__ mpt,
                                                     int32_t* __restrict__ mrow) {
    const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (c >= res->n_cand) return;   // (uniform over the workgroup)
    bool kept = false;
    if (i < min(cnt[q_slot], row)) {
        const int t = tab[(size_t)p * row + i], a = t == INT_MAX ? -1 : t;
        int j, b;
        unsigned long long key;
        if (lp_match(c, i, row, a, res->cand[c], midx, mdist, mpass, tab, &j, &b, &key) && claim[(size_t)c * row + j] == key) {
            mpt[(size_t)c * row + i] = b; mrow[(size_t)c * row + i] = j;
            kept = true;
        }
    }
    wave_count_add(kept, &res->n_match[c]);
}

// among: NULL, or [n_kf] on the host; the keyframes where it is 0 lose their common-word count between the loop_score and loop_select
// stages (bow_loop_among_enqueue), which is all it takes: k_loop_select admits a keyframe to S, M and a group's sum through common_k > 0
static int loop_candidates(mo_map* m, const mo_map_loop_params* prm, const uint8_t* among, mo_map_loop_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const int n_kf = (int)m->pos_slot.size(), mc = prm->max_cand;
    if (prm->kf_pos < -1 || (prm->kf_pos >= 0 && prm->kf_pos >= n_kf)) return mo_fail(c, MO_ERR_ARG, "kf_pos must be -1 or a keyframe position");
    if (prm->n_best < 0) return mo_fail(c, MO_ERR_ARG, "n_best must be >= 0");
    if (mc < 0 || mc > LP_MAX_CAND) return mo_fail(c, MO_ERR_ARG, "max_cand must be in 0 .. 16");
    if (!(prm->ratio > 0.0 && prm->ratio <= 1.0)) return mo_fail(c, MO_ERR_ARG, "ratio must be in (0, 1]");
    int rc;
    if ((rc = bow_require(m))) return rc;
    out->n_cand = 0; out->n_found = 0; out->n_connected = 0; out->max_common = 0; out->n_scored = 0; out->n_passed = 0;
    out->min_score = 1.0;
    for (int i = 0; i < mc; i++) {
        if (out->cand) out->cand[i] = -1;
        if (out->acc) out->acc[i] = 0.0;
        if (out->score) out->score[i] = 0.0;
        if (out->n_match) out->n_match[i] = 0;
    }
    if (n_kf == 0) return MO_OK;
    const int p = prm->kf_pos < 0 ? n_kf - 1 : prm->kf_pos, q_slot = m->pos_slot[p], n_p = m->h_kcnt[q_slot], row = m->row;
    const int min_w = std::max(prm->min_weight, 1);
    const bool match = mc > 0, need_tab = match || out->cur_point;
    MAP_ENTER(m);
    HostClock clk(c);
    if ((rc = upload_pos_slot(m))) return rc;
    mo_stage_begin(c);
    if ((rc = bow_update_enqueue(m)) || (rc = covis_enqueue(m))) return rc;
    const int32_t* W = covis_weights(m);
    BowLoop sc;
    if ((rc = bow_loop_score_enqueue(m, p, W + (size_t)p * n_kf, min_w, &sc))) return rc;
    LoopBufs& b = map_feature<LoopBufs>(m);
    const size_t nk = (size_t)n_kf, pair_n = (size_t)std::max(mc, 1) * row;
    if (among) {
        if ((rc = b.among.reserve(c, nk))) return rc;
        HIPCHK(c, hipMemcpyAsync(b.among, among, nk, hipMemcpyHostToDevice, c->stream));
        if ((rc = bow_loop_among_enqueue(m, b.among))) return rc;
    }
    if ((rc = mo_reserve(c, b.flag, nk, b.acc, nk, b.best, nk, b.cacc, nk, b.connected, nk, b.group, nk * std::max(mc, 1), b.qf, LP_MAX_CAND,
                         b.tf, LP_MAX_CAND, b.res)))
        return rc;
    if (mc) HIPCHK(c, hipMemsetAsync(b.group, 0, nk * mc, c->stream));
    hipLaunchKernelGGL(k_loop_select, dim3(1), dim3(LP_BLOCK), 0, c->stream, sc.score, sc.common, W, n_kf, p, min_w, prm->n_best, mc, m->d_pos_slot, sc.empty,
                       b.flag, b.acc, b.best, b.cacc, b.connected, b.group, b.qf, b.tf, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "loop_select");
    if (need_tab) {
        if ((rc = mo_reserve(c, b.tab, nk * row, b.match, pair_n, b.claim, pair_n, b.cur, (size_t)row, b.mpt, pair_n, b.mrow, pair_n))) return rc;
        if ((rc = map_launch_point_of(m, 0, n_kf, b.tab))) return rc;
        if (match) {
            HIPCHK(c, hipMemsetAsync(b.claim, 0xff, pair_n * 8, c->stream));
            HIPCHK(c, hipMemsetAsync(b.mpt, 0xff, pair_n * 4, c->stream));
            HIPCHK(c, hipMemsetAsync(b.mrow, 0xff, pair_n * 4, c->stream));
            if ((rc = match_launch_pairs(c, m->kdesc, m->kdesc, (size_t)row * 32, (size_t)row * 32, sc.cnt, b.qf, b.tf, 0, 0, mc, row, prm->ratio,
                                         b.match.idx, b.match.dist, b.match.pass)))
                return rc;
        }
        mo_stage_mark(c, "loop_match");
        if (n_p > 0) {
            const dim3 grid((unsigned)((n_p + 255) / 256), (unsigned)std::max(mc, 1));
            const MatchBufs& mb = b.match;
            hipLaunchKernelGGL(k_loop_claim, grid, dim3(256), 0, c->stream, sc.cnt, q_slot, p, row, mb.idx, mb.dist, mb.pass, b.tab, b.res, b.cur, b.claim);
            if (match)
                hipLaunchKernelGGL(k_loop_gather, grid, dim3(256), 0, c->stream, sc.cnt, q_slot, p, row, mb.idx, mb.dist, mb.pass, b.tab, b.claim, b.res, b.mpt, b.mrow);
            HIPCHK(c, hipGetLastError());
        }
        mo_stage_mark(c, "loop_gather");
    }
    if ((rc = b.res.download(c))) return rc;
    if (out->connected) HIPCHK(c, hipMemcpyAsync(out->connected, b.connected, nk, hipMemcpyDeviceToHost, c->stream));
    if (out->group && mc) HIPCHK(c, hipMemcpyAsync(out->group, b.group, nk * mc, hipMemcpyDeviceToHost, c->stream));
    if (n_p > 0) {
        const size_t w = (size_t)n_p * 4;
        if (out->cur_point) HIPCHK(c, hipMemcpyAsync(out->cur_point, b.cur, w, hipMemcpyDeviceToHost, c->stream));
        if (out->match_point && match) HIPCHK(c, hipMemcpy2DAsync(out->match_point, w, b.mpt, (size_t)row * 4, w, (size_t)mc, hipMemcpyDeviceToHost, c->stream));
        if (out->match_row && match) HIPCHK(c, hipMemcpy2DAsync(out->match_row, w, b.mrow, (size_t)row * 4, w, (size_t)mc, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = map_sync(c, clk))) return rc;
    const LoopRes& r = b.res.host();
    out->n_cand = r.n_cand; out->n_found = r.n_found; out->n_connected = r.n_connected; out->max_common = r.max_common;
    out->n_scored = r.n_scored; out->n_passed = r.n_passed; out->min_score = r.min_score;
    for (int i = 0; i < mc; i++) {
        if (out->cand) out->cand[i] = r.cand[i];
        if (out->acc) out->acc[i] = r.acc[i];
        if (out->score) out->score[i] = r.score[i];
        if (out->n_match) out->n_match[i] = r.n_match[i];
    }
    return MO_OK;
}

extern "C" int mo_map_loop_candidates(mo_map* m, const mo_map_loop_params* prm, mo_map_loop_out* out) { return loop_candidates(m, prm, nullptr, out); }

extern "C" int mo_map_loop_candidates_among(mo_map* m, const mo_map_loop_params* prm, const uint8_t* among, mo_map_loop_out* out) {
    return loop_candidates(m, prm, among, out);
}
