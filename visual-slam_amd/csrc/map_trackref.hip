// map_trackref.hip -- tracking a frame against the reference keyframe (mo_map_track_reference in include/vslam_amd.h): ORB-SLAM2's
// TrackReferenceKeyFrame - SearchByBoW restricted to the rows of one vocabulary word, the rotation-consistency check, the pose-only
// refinement.  Read-only on the map; the frame is staged in the spare keyframe slot (map_stage_frame), like mo_map_track's.
//
// What is here: the bucket sort of the frame's rows by word, the search, the row pass and the orientation stage.  The per-row words are
// the keyframe database's (bow_words_enqueue, bow.hip), the point_of table is map_launch_point_of's, the search tail and the claim are
// trk_claim_as (map_track.h), and k_trk_init, k_trk_compact and k_trk_refine (map_track.hip) run unchanged over a TrkFrames view of this
// feature's scratch.
//
// Chain (one synchronisation, the copy-out):
//   bow_update      stale keyframe rows and the staged frame quantised, their words kept by slot                      trackref_words
//   k_trk_init      result block, keys, per-keypoint outputs
//   k_point_of      tab [n_kf - pos][row]: map_launch_point_of fills every position from the reference keyframe's on; row 0 is read
//   k_tr_bucket     one workgroup: stable counting sort of the frame rows by word (cell = woff [W + 1], sorted = wrows)   trackref_prep
//   k_tr_search     one lane per keyframe row: a row with a point walks the bucket of its word, trk_claim_as
//   k_tr_rows       one lane per keyframe row: the winners of the claims -> kf_row by a second atomicMin                trackref_search
//   k_tr_orient     one workgroup: LDS histogram of the rotation bins, the three maxima, the claims outside them dropped  trackref_orient
//   k_trk_compact, k_trk_refine   pass 0, attempt 0                                                                   trackref_refine
// Integer atomics only (minima and sums commute), the refinement's f64 sums in fixed order: the same bytes on every run.
//
// One lane per candidate, not a group of lanes: the tail of the search (best, second, both gates, the claim) is trk_claim_as, which is a
// lane's own; a group would restate it around a shuffle reduction.  NOTES.md has the measured share of the search in the chain.
#include <climits>
#include <cmath>
#include <cstring>

#include "bow.h"
#include "common.h"
#include "map_store.h"
#include "map_track.h"

#define TR_SORT_BLOCK 1024
#define TR_WORDS_PER_THREAD (MO_BOW_MAX_WORDS / TR_SORT_BLOCK)
#define TR_BINS 30
static_assert(MO_BOW_MAX_WORDS % TR_SORT_BLOCK == 0, "words per thread");

struct TrackRefRes {
    int32_t n_claims, n_raw;              // candidates that claimed; claimed frame rows in front of the orientation stage
    int32_t hist[TR_BINS], kept[3];
};

struct TrackRefBufs : MapFeature {
    DevBuf<int32_t> tab;                  // [n_kf - pos][row] point_of from the reference keyframe's position on (INT_MAX: no point); row 0 is its own
    DevBuf<int32_t> cell;                 // [W + 1] woff: first sorted entry of every word's bucket
    DevBuf<int32_t> sorted;               // [row] wrows: frame rows by word, row order inside a word
    DevBuf<int32_t> cq, cd;               // [row] per keyframe row: the frame row it claimed and the distance (-1: none)
    DevBuf<int32_t> kfrow;                // [row] per frame row: the keyframe row of its match
    DevBuf<unsigned long long> key;       // [row] and the rest: the tracker's frame arrays (TrkFrames, map_track.h)
    DevBuf<TrkMatch> match;
    DevBuf<uint8_t> minl;
    DevBuf<int32_t> qpt, qdist; DevBuf<uint8_t> qinl;
    ResBlock<TrackRes> res;
    ResBlock<TrackRefRes> rres;
    // all of it is scratch: every call's chain writes what it reads
    template <class F> void each_scratch(F f) {
        f(tab); f(cell); f(sorted); f(cq); f(cd); f(kfrow); f(key); f(match); f(minl); f(qpt); f(qdist); f(qinl); f(res); f(rres);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// One workgroup: the frame rows (word fword[q], *cnt of them) grouped by word, ascending row order inside a word.  LDS counters, the
// block scan over the words (8 consecutive words per thread), then the scatter in rounds of 1024 rows: a lane's place inside its wave
// is the number of lower lanes with its word, and the 16 waves take their turns at the LDS cursors in wave order - no atomics in the
// scatter, so the order is the stable counting sort's whatever the bucket lengths are.  Also presets kfrow and zeroes the result block.
__global__ __launch_bounds__(TR_SORT_BLOCK) void k_tr_bucket(const uint16_t* __restrict__ fword, const int32_t* __restrict__ cnt, int stride, int W,
                                                             int32_t* __restrict__ cell, int32_t* __restrict__ sorted, int32_t* __restrict__ kfrow,
                                                             TrackRefRes* __restrict__ rr) {
    __shared__ int cur[MO_BOW_MAX_WORDS];
    __shared__ int lw[40];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = min(*cnt, stride);
    for (int w = tid; w < MO_BOW_MAX_WORDS; w += TR_SORT_BLOCK) cur[w] = 0;
    if (tid == 0) { rr->n_claims = 0; rr->n_raw = 0; }
    if (tid < TR_BINS) rr->hist[tid] = 0;
    if (tid < 3) rr->kept[tid] = -1;
    __syncthreads();
    for (int q = tid; q < n; q += TR_SORT_BLOCK) {
        const int w = fword[q];
        if (w < W) atomicAdd(cur + w, 1);
        kfrow[q] = INT_MAX;
    }
    __syncthreads();
    int v[TR_WORDS_PER_THREAD], s = 0;
    for (int j = 0; j < TR_WORDS_PER_THREAD; j++) { v[j] = cur[tid * TR_WORDS_PER_THREAD + j]; s += v[j]; }
    int tot;
    int base = block_excl_scan(s, lw, &tot);
    for (int j = 0; j < TR_WORDS_PER_THREAD; j++) {
        const int w = tid * TR_WORDS_PER_THREAD + j;
        cur[w] = base;
        if (w < W) cell[w] = base;
        base += v[j];
    }
    if (tid == 0) cell[W] = tot;
    __syncthreads();
    for (int b = 0; b < n; b += TR_SORT_BLOCK) {
        const int q = b + tid;
        const int w = q < n ? (int)fword[q] : W;
        const bool valid = w < W;
        const int wk = valid ? w : -1 - lane;   // (a lane without a word equals no other lane)
        int below = 0, same = 0;
        for (int j = 0; j < 64; j++) {
            const bool eq = __shfl(wk, j, 64) == wk;
            same += eq;
            below += eq && j < lane;
        }
        int at = 0;
        for (int t = 0; t < TR_SORT_BLOCK / 64; t++) {
            if (wv == t && valid) {
                at = cur[w];
                if (below == same - 1) cur[w] = at + same;   // (the last lane of the word in this wave moves the cursor)
            }
            __syncthreads();
        }
        if (valid) sorted[at + below] = q;
    }
}

// One lane per row of the reference keyframe (n_kf_rows = *kcnt of them): a row with a point is a candidate; it walks the bucket of its
// word with its own descriptor; best, second, the gates and the claim are trk_claim_as's.
__global__ __launch_bounds__(256) void k_tr_search(TrackPrm prm, const int32_t* __restrict__ kcnt, int stride, int W, const int32_t* __restrict__ tab,
                                                   const uint8_t* __restrict__ kdesc, const uint16_t* __restrict__ kword,
                                                   const int32_t* __restrict__ cell, const int32_t* __restrict__ sorted,
                                                   const uint8_t* __restrict__ fdesc, unsigned long long* __restrict__ key, int32_t* __restrict__ cq,
                                                   int32_t* __restrict__ cd, TrackRes* __restrict__ res, TrackRefRes* __restrict__ rr) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    const int n = min(*kcnt, stride);
    const int p = r < n ? tab[r] : INT_MAX;
    const int w = r < n ? (int)kword[r] : W;
    const bool cand = p != INT_MAX;
    int bq = -1, bd = -1;
    if (cand && w < W) {
        const mo_keypoint none{};
        bq = trk_claim_as(prm, p, kdesc + (size_t)r * 32, fdesc, key,
                          [&](auto visit) {
                              for (int e = cell[w], e1 = cell[w + 1]; e < e1; e++) visit(sorted[e], none, 0.0, 0.0);
                          },
                          &bd);
    }
    if (r < n) { cq[r] = bq; cd[r] = bd; }
    wave_count_add(cand, &res->cand);
    wave_count_add(bq >= 0, &rr->n_claims);
}

// One lane per row of the reference keyframe: the candidate whose claim stands on its frame row gives the row its kf_row; the lowest
// such row when several carry the same (distance, point)
__global__ __launch_bounds__(256) void k_tr_rows(const int32_t* __restrict__ kcnt, int stride, const int32_t* __restrict__ tab, const int32_t* __restrict__ cq,
                                                 const int32_t* __restrict__ cd, const unsigned long long* __restrict__ key, int32_t* __restrict__ kfrow) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= min(*kcnt, stride)) return;
    const int q = cq[r];
    if (q < 0) return;
    if ((((unsigned long long)(unsigned)cd[r] << 32) | (unsigned)tab[r]) == key[q]) atomicMin(kfrow + q, r);
}

// the rotation bin of a match (include/vslam_amd.h states the rule); -1: outside 0 .. 29
__device__ __forceinline__ int tr_bin(float kf_angle, float f_angle) {
    double rot = (double)kf_angle - (double)f_angle;
    if (rot < 0.0) rot += 360.0;
    const double b = rint(rot / 12.0);
    if (!(b >= 0.0 && b < 2.0 * TR_BINS)) return -1;
    int bin = (int)b;
    if (bin >= TR_BINS) bin -= TR_BINS;
    return bin;
}

// One workgroup: the claims counted, and with `check` the histogram of their rotation bins in LDS (integer atomics), the three maxima
// (thread 0) and the claims outside the kept bins reset; kf_row of every frame row without a match becomes -1.
__global__ __launch_bounds__(256) void k_tr_orient(int check, const mo_keypoint* __restrict__ kk, const int32_t* __restrict__ kcnt, const mo_keypoint* __restrict__ fk,
                                                   const int32_t* __restrict__ cnt, int stride, unsigned long long* __restrict__ key,
                                                   int32_t* __restrict__ kfrow, TrackRefRes* __restrict__ rr) {
    __shared__ int hist[TR_BINS], keep[3], raw;
    const int tid = threadIdx.x;
    const int n = min(*cnt, stride), nk = min(*kcnt, stride);
    if (tid < TR_BINS) hist[tid] = 0;
    if (tid < 3) keep[tid] = -1;
    if (tid == 0) raw = 0;
    __syncthreads();
    int mine = 0;
    for (int q = tid; q < n; q += 256) {
        if (key[q] == TK_NONE) continue;
        mine++;
        const int r = kfrow[q];
        const int bin = check && (unsigned)r < (unsigned)nk ? tr_bin(kk[r].angle, fk[q].angle) : -1;
        if (bin >= 0) atomicAdd(hist + bin, 1);
    }
    if (mine) atomicAdd(&raw, mine);
    __syncthreads();
    if (tid == 0 && check) {
        int b1 = -1, b2 = -1, b3 = -1, c1 = 0, c2 = 0, c3 = 0;
        for (int i = 0; i < TR_BINS; i++) {   // (strictly greater: a tie stays with the lower bin; a count of 0 never enters)
            const int c = hist[i];
            if (c > c1) { c3 = c2; b3 = b2; c2 = c1; b2 = b1; c1 = c; b1 = i; }
            else if (c > c2) { c3 = c2; b3 = b2; c2 = c; b2 = i; }
            else if (c > c3) { c3 = c; b3 = i; }
        }
        keep[0] = b1;
        keep[1] = b2 >= 0 && 10 * c2 >= c1 ? b2 : -1;
        keep[2] = keep[1] >= 0 && b3 >= 0 && 10 * c3 >= c1 ? b3 : -1;
    }
    __syncthreads();
    for (int q = tid; q < n; q += 256) {
        bool has = key[q] != TK_NONE;
        if (has && check) {
            const int r = kfrow[q];
            const int bin = (unsigned)r < (unsigned)nk ? tr_bin(kk[r].angle, fk[q].angle) : -1;
            if (bin < 0 || (bin != keep[0] && bin != keep[1] && bin != keep[2])) { key[q] = TK_NONE; has = false; }
        }
        if (!has) kfrow[q] = -1;
    }
    if (tid == 0) rr->n_raw = raw;
    if (tid < TR_BINS) rr->hist[tid] = hist[tid];
    if (tid < 3) rr->kept[tid] = keep[tid];
}

// the parameter rules of the call
static int trackref_check(mo_ctx* c, const mo_map_trackref_params* prm, const double* pose0) {
    if (!(prm->scale_factor > 0.0) || !std::isfinite(prm->scale_factor)) return mo_fail(c, MO_ERR_ARG, "scale_factor must be finite and > 0");
    if (!(prm->chi2 >= 0.0) || !std::isfinite(prm->ratio)) return mo_fail(c, MO_ERR_ARG, "chi2 must be >= 0 and ratio finite");
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(pose0[i])) return mo_fail(c, MO_ERR_ARG, "pose0 must be finite");
    return MO_OK;
}

extern "C" int mo_map_track_reference(mo_map* m, const mo_frame_ref* f, const double K[9], const double pose0[12], const mo_map_trackref_params* prm,
                                      mo_map_trackref_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!f || !K || !pose0 || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    int n, rc;
    if ((rc = trackref_check(c, prm, pose0)) || (rc = bow_require(m))) return rc;
    const int n_kf = (int)m->pos_slot.size();
    const int pos = prm->kf_pos < 0 ? prm->kf_pos + n_kf : prm->kf_pos;
    if (n_kf > 0 && (pos < 0 || pos >= n_kf)) return mo_fail(c, MO_ERR_INDEX, "keyframe position out of range");
    MAP_ENTER(m);
    HostClock clk(c);
    for (int i = 0; i < 12; i++) out->pose[i] = pose0[i];
    out->n_cand = 0; out->n_claims = 0; out->n_matches_raw = 0; out->n_matches = 0; out->n_inliers = 0;
    for (int i = 0; i < TR_BINS; i++) out->hist[i] = 0;
    for (int i = 0; i < 3; i++) out->kept_bin[i] = -1;
    out->ok = 0; out->from_token = 0;
    mo_keypoint* fk; uint8_t* fdesc;
    auto defaults = [&](int nq) {
        for (int i = 0; i < nq; i++) {
            if (out->point) out->point[i] = -1;
            if (out->dist) out->dist[i] = -1;
            if (out->inlier) out->inlier[i] = 0;
            if (out->kf_row) out->kf_row[i] = -1;
        }
    };
    if ((rc = map_stage_frame(m, f, true, &out->from_token, defaults, &n, &fk, &fdesc)) || !fk) return rc;   // (nothing to search: not tracked, not an error)
    BowWords bw;
    if ((rc = bow_words_enqueue(m, n, &bw))) return rc;
    mo_stage_mark(c, "trackref_words");
    const int row = m->row, slot = m->pos_slot[pos], spare = m->kslots;
    TrackRefBufs& b = map_feature<TrackRefBufs>(m);
    const int n_tab = n_kf - pos;   // (k_point_of writes every position >= pos: the table holds them all)
    if ((rc = mo_reserve(c, b.tab, (size_t)n_tab * row, b.cell, (size_t)bw.W + 1, b.sorted, (size_t)row, b.cq, (size_t)row, b.cd, (size_t)row, b.kfrow, (size_t)row,
                         b.key, (size_t)row, b.match, (size_t)row, b.minl, (size_t)row, b.qpt, (size_t)row, b.qdist, (size_t)row, b.qinl, (size_t)row, b.res,
                         b.rres)))
        return rc;
    TrackPrm p{};
    for (int i = 0; i < 9; i++) p.K[i] = K[i];
    p.sf = prm->scale_factor; p.ratio = prm->ratio; p.chi2 = prm->chi2;
    p.max_dist = prm->max_dist; p.min_matches = prm->min_matches;
    const TrkFrames one = trk_frames(b, fk, fdesc, m->kcnt + spare, nullptr, row);   // one frame: the spare slot's rows and count
    const int32_t* kcnt = m->kcnt + slot;
    const mo_keypoint* kk = m->kkps + (size_t)slot * row;
    const uint8_t* kdesc = m->kdesc + (size_t)slot * row * 32;
    const uint16_t* kword = bw.word + (size_t)slot * bw.stride;
    const uint16_t* fword = bw.word + (size_t)spare * bw.stride;
    const unsigned kblocks = (unsigned)std::max((m->h_kcnt[slot] + 255) / 256, 1);
    const float* xyz = m->P[m->cur].view().xyz;
    if ((rc = trk_launch_init(c, one, 1, pose0, &b.res.p->n_local)) || (rc = map_launch_point_of(m, pos, n_tab, b.tab))) return rc;
    hipLaunchKernelGGL(k_tr_bucket, dim3(1), dim3(TR_SORT_BLOCK), 0, c->stream, fword, m->kcnt + spare, row, bw.W, b.cell, b.sorted, b.kfrow, b.rres);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "trackref_prep");
    hipLaunchKernelGGL(k_tr_search, dim3(kblocks), dim3(256), 0, c->stream, p, kcnt, row, bw.W, b.tab, kdesc, kword, b.cell, b.sorted, fdesc, b.key, b.cq, b.cd,
                       b.res, b.rres);
    hipLaunchKernelGGL(k_tr_rows, dim3(kblocks), dim3(256), 0, c->stream, kcnt, row, b.tab, b.cq, b.cd, b.key, b.kfrow);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "trackref_search");
    hipLaunchKernelGGL(k_tr_orient, dim3(1), dim3(256), 0, c->stream, prm->check_orientation != 0, kk, kcnt, fk, m->kcnt + spare, row, b.key, b.kfrow, b.rres);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "trackref_orient");
    if ((rc = trk_launch_compact(c, p, one, 1, 0, 0, xyz)) || (rc = trk_launch_refine(c, p, one, 1, 0))) return rc;
    mo_stage_mark(c, "trackref_refine");
    if ((rc = b.res.download(c)) || (rc = b.rres.download(c))) return rc;
    if (out->point) HIPCHK(c, hipMemcpyAsync(out->point, b.qpt, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (out->dist) HIPCHK(c, hipMemcpyAsync(out->dist, b.qdist, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (out->inlier) HIPCHK(c, hipMemcpyAsync(out->inlier, b.qinl, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (out->kf_row) HIPCHK(c, hipMemcpyAsync(out->kf_row, b.kfrow, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = map_sync(c, clk))) return rc;
    const TrackRes& r = b.res.host();
    const TrackRefRes& rr = b.rres.host();
    for (int i = 0; i < 12; i++) out->pose[i] = r.pose[i];
    out->n_cand = r.pass_cand[0]; out->n_claims = rr.n_claims; out->n_matches_raw = rr.n_raw;
    out->n_matches = r.pass_matches[0]; out->n_inliers = r.pass_inliers[0];
    for (int i = 0; i < TR_BINS; i++) out->hist[i] = rr.hist[i];
    for (int i = 0; i < 3; i++) out->kept_bin[i] = rr.kept[i];
    out->ok = r.n_done == 1 && r.pass_inliers[0] >= prm->min_inliers;
    return MO_OK;
}
