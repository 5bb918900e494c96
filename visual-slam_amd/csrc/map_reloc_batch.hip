// map_reloc_batch.hip -- a batch of frames relocalized against the device map in one chain (mo_map_relocalize_batch and
// mo_map_query_keyframes_batch in include/vslam_amd.h).  The rule: frame i's results are mo_map_relocalize's (or mo_map_relocalize_pre's,
// mo_map_query_keyframes') for that frame alone, integers equal and doubles equal bit for bit.
//
// The relocalization is map_reloc.h's, the one the single calls run: one RelocRes per frame, the kernels of map_reloc.hip launched
// over (frame, ...) on the [frame][row] buffers below.  The batch's own: the staging (map_frames.h), the matcher's numbering of the
// query frames, the pair list, the groups.
//
// Chain (one synchronisation, the copy-out):
//   staging         host frames packed into pinned memory and uploaded in one copy per array, resident frames copied on the device,
//                   into [frame][row] buffers (row = the store's row stride, grown first to the widest frame); the spare slot is not used
//   once per batch  map_launch_point_of; with a preselection bow_batch_enqueue (bow.hip): the database update of the stale slots, one
//                   quantisation launch, a histogram per frame, scores over (frame, keyframe), a ranking workgroup per frame that
//                   writes the frame's slice of the pair list
//   per group       match_launch_pairs over the group's (frame, keyframe) pairs -> reloc_launch_candidates -> reloc_launch_poses
// The matcher indexes one count array with both sides of a pair: the store's slots keep their numbers, frame f is number S + f behind
// them (S = kslots + 1) and the query base is moved back by S frames (bow_batch_qbase), in the manner of bow_update's list.
// Pair order without a preselection: keyframe-major inside a group (pair k * frames + f).  A workgroup reads its query rows once, into
// registers, and streams the whole train side tile by tile; neighbouring pairs in the launch order then stream the same keyframe, whose
// 64 KB stay in the L2 while every frame of the group passes over them.  With a preselection the ranking writes frame-major slices.
// Groups: the matcher's outputs are 17 bytes per (pair, row), so the frames run in groups of whole frames under a pair budget
// (mo_map_reloc_batch_plan), enqueued back to back; what scales with pairs or candidates is sized per group, the frames' rows and
// result blocks (41 bytes per row, 8 KB per frame) per batch.
// Integer atomics only (maxima and minima commute): equal inputs give equal bytes on every run.
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"
#include "bow.h"
#include "map_store.h"
#include "map_frames.h"
#include "map_reloc.h"

#define RLB_BUDGET_BYTES (1ll << 30)   // matcher output of one group by default
#define RLB_MATCH_BYTES 17             // idx [2], dist [2], pass per (pair, row)
#define RLB_MAX_PAIRS 65535            // pairs of one matcher launch (its grid's y extent)

struct RelocBatchBufs : MapFeature {
    DevBuf<mo_keypoint> fk;               // [frame][row] staged keypoints
    DevBuf<uint8_t> fdesc;                // [frame][row][32]
    DevBuf<int32_t> cnt;                  // [S + frames + 2] the matcher's counts: the store's slots, the frames, the words, the empty frame
    DevBuf<int32_t> tab;                  // point_of [position][row]
    DevBuf<int32_t> qf, tf;               // [group pairs] the pair list without a preselection
    MatchBufs match;                      // [group pairs][row]
    DevBuf<int32_t> score;                // [group frames][n_kf]
    DevBuf<int32_t> cq; DevBuf<float> rec; DevBuf<uint8_t> cinl;   // [group frames][candidate][row] (rec: [5] each)
    DevBuf<int32_t> qpt; DevBuf<uint8_t> qinl;                     // [frame][row]
    DevBuf<RelocRes> res;                 // [frame]
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) {
        f(fk); f(fdesc); f(cnt); f(tab); f(qf); f(tf); match.each_scratch(f); f(score); f(cq); f(rec); f(cinl); f(qpt); f(qinl); f(res);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
    // pinned host sides (not device scratch)
    PinnedBuf<mo_keypoint> h_fk; PinnedBuf<uint8_t> h_fdesc; PinnedBuf<int32_t> h_cnt;
    PinnedBuf<RelocRes> h_res; PinnedBuf<int32_t> h_qpt; PinnedBuf<uint8_t> h_qinl;
};

// the group plan: whole frames under the pair budget, at least one frame per group
extern "C" int mo_map_reloc_batch_plan(int32_t n_frames, int64_t pairs_per_frame, int32_t row, int64_t max_pairs, int32_t* frames_per_group,
                                       int32_t* n_groups) {
    if (!frames_per_group || !n_groups || n_frames < 0 || pairs_per_frame < 0 || row < 0 || max_pairs < 0) return MO_ERR_ARG;
    long long budget = max_pairs > 0 ? max_pairs : RLB_BUDGET_BYTES / ((long long)RLB_MATCH_BYTES * std::max(row, 1));
    budget = std::max(1ll, std::min(budget, (long long)RLB_MAX_PAIRS));
    const long long fit = pairs_per_frame > 0 ? budget / pairs_per_frame : (long long)n_frames;
    const long long fpg = std::max(1ll, std::min(fit, (long long)std::max(n_frames, 1)));
    *frames_per_group = (int32_t)fpg;
    *n_groups = (int32_t)((n_frames + fpg - 1) / fpg);
    return MO_OK;
}

// the pair list of a group without a preselection, keyframe-major: pair k * nfg + f = frame q0 + f against the slot of position k
__global__ __launch_bounds__(256) void k_rlb_pairs(int nfg, int n_kf, int q0, const int32_t* __restrict__ pos_slot, int32_t* __restrict__ qf,
                                                   int32_t* __restrict__ tf) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= nfg * n_kf) return;
    const int k = p / nfg, f = p - k * nfg;
    qf[p] = q0 + f;
    tf[p] = pos_slot[k];
}

// the matcher's counts on the host: the store's slots, the frames behind them, the words, the empty frame
static void rlb_counts(const mo_map* m, const int32_t* fcnt, int nf, int32_t* h_cnt) {
    const int S = m->kslots + 1;
    std::fill(h_cnt, h_cnt + S + nf + 2, 0);
    std::copy(m->h_kcnt.begin(), m->h_kcnt.begin() + m->n_slots, h_cnt);
    std::copy(fcnt, fcnt + nf, h_cnt + S);
    h_cnt[S + nf] = bow_words(m);
}

// what both calls do between the lookup and their chains: the store grown to the widest frame, the position table, the frames staged
// in [frame][row] buffers and the counts uploaded, the stage set opened
static int rlb_stage(mo_map* m, RelocBatchBufs& b, const mo_frame_ref* frames, int nf, const BatchFrames& bf, const std::vector<int32_t>& fcnt) {
    mo_ctx* c = m->c;
    int rc;
    if ((rc = map_int32_guard(m)) || (rc = kf_reserve(m, bf.max_n, m->n_slots)) || (rc = upload_pos_slot(m))) return rc;
    const int S = m->kslots + 1;
    const size_t rows = (size_t)nf * m->row;
    if ((rc = mo_reserve(c, b.fk, rows, b.fdesc, rows * 32, b.cnt, (size_t)S + nf + 2, b.h_cnt, (size_t)S + nf + 2)) ||
        (rc = batch_frames_reserve_host(c, bf, rows, b.h_fk, b.h_fdesc)))
        return rc;
    rlb_counts(m, fcnt.data(), nf, b.h_cnt);
    mo_stage_begin(c);
    if ((rc = batch_frames_stage(c, frames, nf, (size_t)m->row, bf, fcnt.data(), b.h_fk, b.h_fdesc, b.fk, b.fdesc))) return rc;
    HIPCHK(c, hipMemcpyAsync(b.cnt, b.h_cnt, ((size_t)S + nf + 2) * 4, hipMemcpyHostToDevice, c->stream));
    mo_stage_mark(c, "rlb_stage");
    return MO_OK;
}

extern "C" int mo_map_relocalize_batch(mo_map* m, const mo_frame_ref* frames, int32_t n_frames, const double K[9],
                                       const mo_map_reloc_batch_params* prm, mo_map_reloc_batch_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!K || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (n_frames < 0 || n_frames > MO_RELOC_BATCH_MAX) return mo_fail(c, MO_ERR_ARG, "n_frames must be in 0 .. MO_RELOC_BATCH_MAX");
    if (n_frames > 0 && (!frames || !out->cand_pos || !out->cand_score || !out->cand_inliers || !out->pose || !out->ok || !out->kf_pos || !out->n_cand ||
                         !out->n_corr || !out->n_inliers || !out->from_token))
        return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const int n_pre = prm->n_pre;
    if (n_pre == 0) return mo_fail(c, MO_ERR_ARG, "n_pre must be >= 1 (or < 0: every keyframe)");
    int rc;
    if (n_pre >= 1 && (rc = bow_require(m))) return rc;
    RelocGeom g;
    if ((rc = reloc_check(c, K, &prm->p, &g))) return rc;
    if (out->stride < 0) return mo_fail(c, MO_ERR_ARG, "stride must be >= 0");
    if (prm->max_pairs < 0) return mo_fail(c, MO_ERR_ARG, "max_pairs must be >= 0");
    MAP_ENTER(m);
    HostClock clk(c);
    if (n_frames == 0) { out->n_ok = 0; out->n_groups = 0; return MO_OK; }
    const int nf = n_frames, stride = out->stride, nc = prm->p.max_candidates;
    auto dst = [&](int i) {   // frame i's rows of the caller's outputs
        const size_t at = (size_t)i * stride, ci = (size_t)i * nc;
        return RelocDst{out->point ? out->point + at : nullptr, out->inlier ? out->inlier + at : nullptr, out->cand_pos + ci, out->cand_score + ci,
                        out->cand_inliers + ci, out->pose + (size_t)i * 12, out->ok + i, out->kf_pos + i, out->n_cand + i, out->n_corr + i, out->n_inliers + i};
    };
    // the frames looked up: every row count known and checked before anything is written
    std::vector<int32_t> fcnt((size_t)nf);
    BatchFrames bf;
    if ((rc = batch_frames_lookup(c, frames, nf, stride, "a frame has more rows than stride", fcnt.data(), &bf))) return rc;
    const int n_kf = (int)m->pos_slot.size();
    // the keyframes that are matched: all of them, or - with fewer than all asked for - the n_pre each frame's query selects on the device
    const bool pre = n_pre >= 1 && n_pre < n_kf;
    if (pre && bf.max_n > MO_BOW_MAX_ROWS) return mo_fail(c, MO_ERR_UNSUPPORTED, "a frame of more than 65535 rows would wrap a term count");
    out->n_ok = 0; out->n_groups = 0;
    for (int i = 0; i < nf; i++) {
        reloc_defaults(dst(i), fcnt[i], nc);
        out->from_token[i] = bf.slot[i] >= 0;
    }
    if (n_kf == 0 || !bf.any_rows) return MO_OK;   // (nothing to match: not relocalized, not an error)
    RelocBatchBufs& b = map_feature<RelocBatchBufs>(m);
    if ((rc = rlb_stage(m, b, frames, nf, bf, fcnt))) return rc;
    const int row = m->row, S = m->kslots + 1, ppf = pre ? n_pre : n_kf;
    int32_t fpg, ng;
    mo_map_reloc_batch_plan(nf, ppf, row, prm->max_pairs, &fpg, &ng);
    const size_t rows = (size_t)nf * row, gpairs = (size_t)fpg * ppf, gcand = (size_t)fpg * nc * row;
    if ((rc = mo_reserve(c, b.tab, (size_t)n_kf * row, b.qf, gpairs, b.tf, gpairs, b.match, gpairs * row, b.score, (size_t)fpg * n_kf, b.cq, gcand, b.rec, gcand * 5,
                         b.cinl, gcand, b.qpt, rows, b.qinl, rows, b.res, (size_t)nf, b.h_res, (size_t)nf)) ||
        (out->point && (rc = b.h_qpt.reserve(c, rows))) || (out->inlier && (rc = b.h_qinl.reserve(c, rows))))
        return rc;
    // ---- once per batch: point_of, and the selection of every frame's keyframes
    if ((rc = map_launch_point_of(m, 0, n_kf, b.tab))) return rc;
    BowBatch sel;
    if (pre && (rc = bow_batch_enqueue(m, b.fdesc, b.cnt, fcnt.data(), nf, row, n_pre, true, &sel))) return rc;
    mo_stage_mark(c, "rlb_select");
    const float* xyz = m->P[m->cur].view().xyz;
    const uint8_t* qbase = bow_batch_qbase(b.fdesc, S, (size_t)row);
    const MatchView mv{b.match.idx, b.match.dist, b.match.pass, b.tab, row};
    // ---- the groups, back to back
    for (int gi = 0; gi < ng; gi++) {
        const int f0 = gi * fpg, nfg = std::min((int)fpg, nf - f0), np = nfg * ppf;
        if (!pre) {
            hipLaunchKernelGGL(k_rlb_pairs, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c->stream, nfg, n_kf, S + f0, m->d_pos_slot.p, b.qf.p, b.tf.p);
            HIPCHK(c, hipGetLastError());
        }
        if ((rc = match_launch_pairs(c, qbase, m->kdesc, (size_t)row * 32, (size_t)row * 32, b.cnt, pre ? sel.qf + (size_t)f0 * n_pre : (const int32_t*)b.qf,
                                     pre ? sel.tf + (size_t)f0 * n_pre : (const int32_t*)b.tf, 0, 0, np, row, prm->p.ratio, b.match.idx, b.match.dist,
                                     b.match.pass)))
            return rc;
        mo_stage_mark(c, "rlb_match");
        const RlFrames fr{b.fk + (size_t)f0 * row, b.cnt + S + f0, row, nfg, n_kf, nc, ppf, pre ? sel.mrow + (size_t)f0 * n_kf : nullptr, b.score, b.cq, b.rec,
                          b.cinl, b.qpt + (size_t)f0 * row, b.qinl + (size_t)f0 * row, b.res + f0};
        if ((rc = reloc_launch_candidates(c, fr, mv, xyz))) return rc;
        mo_stage_mark(c, "rlb_candidates");
        if ((rc = reloc_launch_poses(c, fr, mv, g, prm->p.n_hyp, prm->p.seed, "rlb_p3p", "rlb_refine"))) return rc;
    }
    // ---- copy-out: the result blocks, and one download per requested per-keypoint array
    HIPCHK(c, hipMemcpyAsync(b.h_res, b.res, (size_t)nf * sizeof(RelocRes), hipMemcpyDeviceToHost, c->stream));
    if (out->point) HIPCHK(c, hipMemcpyAsync(b.h_qpt, b.qpt, rows * 4, hipMemcpyDeviceToHost, c->stream));
    if (out->inlier) HIPCHK(c, hipMemcpyAsync(b.h_qinl, b.qinl, rows, hipMemcpyDeviceToHost, c->stream));
    if ((rc = map_sync(c, clk))) return rc;
    for (int i = 0; i < nf; i++) {
        const size_t at = (size_t)i * stride, src = (size_t)i * row, n = (size_t)fcnt[i];
        out->n_ok += reloc_result(dst(i), b.h_res[i], &prm->p);
        if (out->point) std::memcpy(out->point + at, b.h_qpt + src, n * 4);
        if (out->inlier) std::memcpy(out->inlier + at, b.h_qinl + src, n);
    }
    out->n_groups = ng;
    return MO_OK;
}

extern "C" int mo_map_query_keyframes_batch(mo_map* m, const mo_frame_ref* frames, int32_t n_frames, const mo_map_query_params* prm, int32_t* pos,
                                            double* score, int32_t* n, int32_t* from_token) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!prm) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (prm->n_best < 0) return mo_fail(c, MO_ERR_ARG, "n_best must be >= 0");
    if (n_frames < 0 || n_frames > MO_RELOC_BATCH_MAX) return mo_fail(c, MO_ERR_ARG, "n_frames must be in 0 .. MO_RELOC_BATCH_MAX");
    if (n_frames > 0 && (!frames || !n || !from_token || (prm->n_best > 0 && (!pos || !score)))) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    int rc;
    if ((rc = bow_require(m))) return rc;
    MAP_ENTER(m);
    HostClock clk(c);
    if (n_frames == 0) return MO_OK;
    const int nf = n_frames, nb = prm->n_best;
    std::vector<int32_t> fcnt((size_t)nf);
    BatchFrames bf;
    if ((rc = batch_frames_lookup(c, frames, nf, INT_MAX, "", fcnt.data(), &bf))) return rc;
    for (int i = 0; i < nf; i++) { n[i] = 0; from_token[i] = bf.slot[i] >= 0; }
    for (size_t i = 0; i < (size_t)nf * nb; i++) { pos[i] = -1; score[i] = 0.0; }
    if (m->pos_slot.empty() || !bf.any_rows || nb == 0) return MO_OK;   // (nothing to rank: not an error)
    RelocBatchBufs& b = map_feature<RelocBatchBufs>(m);
    if ((rc = rlb_stage(m, b, frames, nf, bf, fcnt))) return rc;
    BowBatch q;
    if ((rc = bow_batch_enqueue(m, b.fdesc, b.cnt, fcnt.data(), nf, m->row, nb, false, &q))) return rc;
    mo_stage_mark(c, "rlb_select");
    HIPCHK(c, hipMemcpyAsync(pos, q.pos, (size_t)nf * nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(score, q.score, (size_t)nf * nb * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(n, q.n, (size_t)nf * 4, hipMemcpyDeviceToHost, c->stream));
    return map_sync(c, clk);
}
