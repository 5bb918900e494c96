// bow.hip -- place recognition on the device map: a flat binary vocabulary trained on the device (mo_vocab_train), a dense keyframe
// database of term counts on mo_map (mo_map_set_vocabulary), the query that ranks the keyframes by DBoW2's L1 score
// (mo_map_query_keyframes) and the preselection mo_map_relocalize_pre runs inside its own chain (bow_select_enqueue).  The rules
// are stated above mo_vocab_train in include/vslam_amd.h; tests/bow_restatement.py restates them in numpy.
// Quantisation launches the matcher (match_launch_pairs, the words as train rows): its best neighbour is the word with the lowest
// Hamming distance, ties to the lower index.  No Hamming kernel of its own: profiles/bow_rate.txt records what the matcher costs here.
// Everything is integer work; the one f64 expression is the score at the end of k_bow_score (-ffp-contract=off, Makefile).
#include <cmath>
#include <cstring>

#include "bow.h"

// every kernel here keeps all of its LDS in the dynamic region, whose base is 16-byte aligned
#define BOW_RED_BYTES 64   // the block-reduction scratch behind the per-word array

struct BowBufs : MapFeature {
    mo_vocab* v = nullptr;
    int Wp = 0, db_rows = 0, word_rows = 0;
    DevBuf<uint16_t> db;                 // [db_rows][Wp] term counts by keyframe slot; the row of the spare slot is the query frame's
    DevBuf<long long> norm;              // [db_rows] sum of count * weight
    DevBuf<uint16_t> word; int wstride = 0;   // [db_rows][wstride] the word of every row, by keyframe slot like db; the spare slot's are the staged frame's
    std::vector<uint32_t> done;          // by slot: the serial of the keyframe store (mo_map::kserial) the row was made from, 0: none
    std::vector<int32_t> h_lst;          // the slots quantised by the call in flight, the spare slot last
    // one block, built on the host and uploaded in one copy per call (the host knows every row count): cnt [kslots + 3] = the store's
    // row counts by slot, then W (the words as a train frame), then 0 (an empty frame); lst / ltf [stale + 1] = query slot / train
    // frame of every quantisation pair
    std::vector<int32_t> h_up; DevBuf<int32_t> up;
    const int32_t* cnt = nullptr; const int32_t* lst = nullptr; const int32_t* ltf = nullptr;
    MatchBufs match;                     // [pair][stride]: idx[2 * r] is the word of query row r (the layout is emit_match's, match_kernels.hip)
    DevBuf<double> score;                // [n_kf]
    DevBuf<int32_t> common;              // [n_kf] common words with the asking keyframe (mo_map_loop_candidates)
    DevBuf<int32_t> out_pos, out_n; DevBuf<double> out_score;
    DevBuf<int32_t> sel_qf, sel_tf, mrow;
    // scratch: what every call's chain writes before it reads.  db, norm and word are state (the rows `done` vouches for are read by
    // later calls); a DevBuf added above is named here or in this sentence
    template <class F> void each_scratch(F f) {
        f(up); match.each_scratch(f); f(score); f(common); f(out_pos); f(out_n); f(out_score); f(sel_qf); f(sel_tf); f(mrow);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// ---- block sum of int64 over 256 threads, scratch = 4 values in LDS; thread 0 holds the sum ---------------------------------------------
__device__ __forceinline__ long long bow_block_sum(long long v, long long* red) {
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// ---- k_bow_hist: the words of one frame -> its row of term counts and its norm; one workgroup per listed slot ---------------------------
// LDS counters (one per word), then the row written with plain 16-byte vector stores (8 counts each).  The word of every row is kept
// too (word [slot][wstride], uint16: W <= 8192): the rows mo_map_track_reference buckets and mo_map_keyframe_words hands out.
// A listed frame `slot` of the matcher's numbering owns row slot - row0 of db, norm and word (the database: row0 = 0; a batch's own
// rows, bow_batch_enqueue: row0 = its first frame, wstride = 0: no words kept).
__global__ __launch_bounds__(256) void k_bow_hist(const int32_t* __restrict__ lst, const int32_t* __restrict__ cnt, int stride,
                                                  const int32_t* __restrict__ qidx, int W, int Wp, const int32_t* __restrict__ weights, int row0,
                                                  uint16_t* __restrict__ db, long long* __restrict__ norm, uint16_t* __restrict__ word, int wstride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t* s_cnt = (int32_t*)smem;
    long long* red = (long long*)(smem + (size_t)Wp * 4);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(cnt[lst[b]], stride), slot = lst[b] - row0;
    for (int w = tid; w < Wp; w += 256) s_cnt[w] = 0;
    __syncthreads();
    for (int q = tid; q < n; q += 256) {
        const int w = qidx[2 * ((size_t)b * stride + q)];
        if ((unsigned)w < (unsigned)W) atomicAdd(&s_cnt[w], 1);
        if (q < wstride) word[(size_t)slot * wstride + q] = (uint16_t)w;
    }
    __syncthreads();
    uint4* row = (uint4*)(db + (size_t)slot * Wp);
    long long part = 0;
    for (int g = tid; g < Wp / 8; g += 256) {
        const int4 c0 = *(const int4*)(s_cnt + 8 * g), c1 = *(const int4*)(s_cnt + 8 * g + 4);
        const int4 w0 = *(const int4*)(weights + 8 * g), w1 = *(const int4*)(weights + 8 * g + 4);
        row[g] = make_uint4((unsigned)c0.x | ((unsigned)c0.y << 16), (unsigned)c0.z | ((unsigned)c0.w << 16),
                            (unsigned)c1.x | ((unsigned)c1.y << 16), (unsigned)c1.z | ((unsigned)c1.w << 16));
        part += (long long)c0.x * w0.x + (long long)c0.y * w0.y + (long long)c0.z * w0.z + (long long)c0.w * w0.w +
                (long long)c1.x * w1.x + (long long)c1.y * w1.y + (long long)c1.z * w1.z + (long long)c1.w * w1.w;
    }
    const long long tot = bow_block_sum(part, red);
    if (tid == 0) norm[slot] = tot;
}

// ---- k_bow_score: D_k and the score of every keyframe position; a workgroup keeps q_w in LDS and walks keyframes blockIdx.x, + gridDim.x, ...
// q_w = count * weight < 2^30 (count <= 65535, weight <= 14 * 1024): one int32 per word.  A keyframe's row is streamed once, 16 bytes
// (8 counts) per load.
// No overflow: the counts of a frame sum to its rows <= 65535, so |q| and |k| are <= 65535 * 14336 < 2^30; a term |q_w |k| - k_w |q||
// is at most max(q_w |k|, k_w |q|) < 2^60, and D_k <= sum_w q_w |k| + sum_w k_w |q| = 2 |q| |k| < 2^61: every partial sum, in any order,
// stays inside int64.
__device__ __forceinline__ long long bow_term(int q, unsigned k, int w, long long nq, long long nk) {
    const long long d = (long long)q * nk - (long long)(k * (unsigned)w) * nq;
    return d < 0 ? -d : d;
}

// COMMON (mo_map_loop_candidates, the query slot then is the asking keyframe's own): the same pass also counts, per keyframe, the words
// with q_w > 0 (weight and query count both non-zero) that the keyframe has too - no second walk over the rows.  The asking keyframe
// (q_pos) and the keyframes connected to it (wrow[k] >= min_w, wrow = its row of the covisibility matrix) get 0.  The plain query's
// instantiation takes an empty argument and compiles to the kernel it was before the template.
template <bool COMMON> struct BowCommonArg {};
template <> struct BowCommonArg<true> {
    const int32_t* wrow; int q_pos, min_w;
    int32_t* common;
};

// The query: row q0 + blockIdx.y of (qdb, qnorm) - the database's own spare or keyframe row for the one-frame calls, a batch's rows for
// bow_batch_enqueue - and its scores in row blockIdx.y of score [frame][n_kf].
template <bool COMMON> __global__ __launch_bounds__(256) void k_bow_score(const int32_t* __restrict__ pos_slot, int n_kf, int q0, const uint16_t* __restrict__ qdb,
                                                                          const long long* __restrict__ qnorm, const uint16_t* __restrict__ db,
                                                                          const long long* __restrict__ norm, const int32_t* __restrict__ weights, int Wp,
                                                                          double* __restrict__ score, BowCommonArg<COMMON> ca) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t* s_q = (int32_t*)smem;
    long long* red = (long long*)(smem + (size_t)Wp * 4);
    const int tid = threadIdx.x;
    const int qi = q0 + (int)blockIdx.y;
    const uint4* qrow = (const uint4*)(qdb + (size_t)qi * Wp);
    score += (size_t)blockIdx.y * n_kf;
    for (int g = tid; g < Wp / 8; g += 256) {
        const uint4 c = qrow[g];
        const int4 w0 = *(const int4*)(weights + 8 * g), w1 = *(const int4*)(weights + 8 * g + 4);
        *(int4*)(s_q + 8 * g) = make_int4((int)(c.x & 0xffffu) * w0.x, (int)(c.x >> 16) * w0.y, (int)(c.y & 0xffffu) * w0.z, (int)(c.y >> 16) * w0.w);
        *(int4*)(s_q + 8 * g + 4) = make_int4((int)(c.z & 0xffffu) * w1.x, (int)(c.z >> 16) * w1.y, (int)(c.w & 0xffffu) * w1.z, (int)(c.w >> 16) * w1.w);
    }
    __syncthreads();
    const long long nq = qnorm[qi];
    for (int k = blockIdx.x; k < n_kf; k += gridDim.x) {
        const int s = pos_slot[k];
        const long long nk = norm[s];
        const uint4* krow = (const uint4*)(db + (size_t)s * Wp);
        long long D = 0;
        int cw = 0;
        for (int g = tid; g < Wp / 8; g += 256) {
            const uint4 c = krow[g];
            const int4 w0 = *(const int4*)(weights + 8 * g), w1 = *(const int4*)(weights + 8 * g + 4);
            const int4 q0 = *(const int4*)(s_q + 8 * g), q1 = *(const int4*)(s_q + 8 * g + 4);
            D += bow_term(q0.x, c.x & 0xffffu, w0.x, nq, nk) + bow_term(q0.y, c.x >> 16, w0.y, nq, nk) +
                 bow_term(q0.z, c.y & 0xffffu, w0.z, nq, nk) + bow_term(q0.w, c.y >> 16, w0.w, nq, nk) +
                 bow_term(q1.x, c.z & 0xffffu, w1.x, nq, nk) + bow_term(q1.y, c.z >> 16, w1.y, nq, nk) +
                 bow_term(q1.z, c.w & 0xffffu, w1.z, nq, nk) + bow_term(q1.w, c.w >> 16, w1.w, nq, nk);
            if constexpr (COMMON)
                cw += (int)(q0.x > 0 && (c.x & 0xffffu)) + (int)(q0.y > 0 && (c.x >> 16)) + (int)(q0.z > 0 && (c.y & 0xffffu)) +
                      (int)(q0.w > 0 && (c.y >> 16)) + (int)(q1.x > 0 && (c.z & 0xffffu)) + (int)(q1.y > 0 && (c.z >> 16)) +
                      (int)(q1.z > 0 && (c.w & 0xffffu)) + (int)(q1.w > 0 && (c.w >> 16));
        }
        D = bow_block_sum(D, red);
        if (tid == 0) score[k] = (nq == 0 || nk == 0) ? 0.0 : 1.0 - 0.5 * (double)D / ((double)nq * (double)nk);
        if constexpr (COMMON) {
            const long long n = bow_block_sum(cw, red + 4);   // (the second half of the reduction scratch)
            if (tid == 0) ca.common[k] = (k == ca.q_pos || ca.wrow[k] >= ca.min_w) ? 0 : (int32_t)n;
        }
        __syncthreads();   // (red is written again by the next keyframe)
    }
}

// ---- k_bow_rank: the keyframe positions with a score > 0, highest first, ties to the lower position, at most n_best; one workgroup ------
// The rank of a keyframe is the number of keyframes before it in that order (a total order: no two share a rank), counted against
// tiles of 1024 scores in LDS; a keyframe with rank < n_best writes itself to that place.  Any number of keyframes: the workgroup walks
// its own positions in steps of 1024 and, for each step, every tile.
// sel_qf != NULL (mo_map_relocalize_pre): the pair list of the matcher - pair r = the frame in the spare slot against the slot of the
// keyframe at rank r, the pairs past the selected keyframes name the empty frame - and mrow[k] = the pair of position k, -1: none.
// One workgroup per frame (bow_batch_enqueue; the one-frame calls launch one): frame f = blockIdx.x reads row f of score [frame][n_kf],
// writes row f of out_pos / out_score / sel_qf / sel_tf [frame][n_best], of mrow [frame][n_kf] and out_n[f]; its query frame in the
// matcher's numbering is q0 + f, and a pair without a keyframe names the train frame tf_none (any frame the counts cover).
__global__ __launch_bounds__(1024) void k_bow_rank(const double* __restrict__ score, int n_kf, int n_best, int32_t* __restrict__ out_pos,
                                                   double* __restrict__ out_score, int32_t* __restrict__ out_n, const int32_t* __restrict__ pos_slot,
                                                   int q0, int tf_none, int empty, int32_t* __restrict__ sel_qf, int32_t* __restrict__ sel_tf,
                                                   int32_t* __restrict__ mrow) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* s_s = (double*)smem;
    int* s_n = (int*)(smem + 1024 * 8);
    const int tid = threadIdx.x, f = blockIdx.x, spare = q0 + f;
    score += (size_t)f * n_kf; out_pos += (size_t)f * n_best; out_score += (size_t)f * n_best; out_n += f;
    if (sel_qf) { sel_qf += (size_t)f * n_best; sel_tf += (size_t)f * n_best; }
    if (mrow) mrow += (size_t)f * n_kf;
    if (tid == 0) *s_n = 0;
    for (int i = tid; i < n_best; i += 1024) {
        out_pos[i] = -1; out_score[i] = 0.0;
        if (sel_qf) { sel_qf[i] = empty; sel_tf[i] = tf_none; }
    }
    __syncthreads();
    for (int base = 0; base < n_kf; base += 1024) {
        const int k = base + tid;
        const double my = k < n_kf ? score[k] : 0.0;
        int r = 0;
        for (int t0 = 0; t0 < n_kf; t0 += 1024) {
            __syncthreads();
            s_s[tid] = t0 + tid < n_kf ? score[t0 + tid] : 0.0;
            __syncthreads();
            const int lim = min(1024, n_kf - t0);
            if (my > 0.0)
#pragma unroll 8
                for (int j = 0; j < lim; j++) {   // (wave-uniform j: broadcast reads, several in flight)
                    const double sj = s_s[j];
                    r += (sj > my) || (sj == my && t0 + j < k);
                }
        }
        const bool in = my > 0.0 && r < n_best;
        if (in) {
            out_pos[r] = k; out_score[r] = my;
            if (sel_qf) { sel_qf[r] = spare; sel_tf[r] = pos_slot[k]; }
        }
        if (mrow && k < n_kf) mrow[k] = in ? r : -1;
        if (my > 0.0) atomicAdd(s_n, 1);
    }
    __syncthreads();
    if (tid == 0) *out_n = min(*s_n, n_best);
}

// ---- training kernels ---------------------------------------------------------------------------------------------------------------------
// k_vocab_update: the bit counts of every word's members and the new words.  LDS-private counters, not a segmented sum over rows ordered
// by word: a training call has no map, so the map's device-wide scan is not at hand, and ordering the rows would move 32 MB per
// iteration at 10^6 rows.  A workgroup owns `wpb` consecutive words, 256 bit counters and a member counter each, all in its LDS; it reads
// every row's word (4 bytes) and, for the rows of its own words, the descriptor, adding each set bit to an LDS counter.  No global
// atomic at all; integer sums, so the order of the adds does not matter.  The words are then rewritten in place: no workgroup reads
// another's words in this kernel.
__global__ __launch_bounds__(256) void k_vocab_update(const int32_t* __restrict__ idx, const uint8_t* __restrict__ desc, int n, int W, int wpb,
                                                      uint8_t* __restrict__ words, int32_t* __restrict__ changed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t* s_c = (int32_t*)smem;   // [wpb][257]
    const int tid = threadIdx.x, w0 = blockIdx.x * wpb, nw = min(wpb, W - w0);
    for (int i = tid; i < nw * 257; i += 256) s_c[i] = 0;
    __syncthreads();
    for (int r = tid; r < n; r += 256) {
        const int w = idx[2 * (size_t)r] - w0;
        if ((unsigned)w >= (unsigned)nw) continue;
        atomicAdd(&s_c[w * 257 + 256], 1);
        const uint4 lo = *(const uint4*)(desc + (size_t)r * 32), hi = *(const uint4*)(desc + (size_t)r * 32 + 16);
        const uint32_t d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            uint32_t x = d[k];
            while (x) {
                const int bit = __ffs((int)x) - 1;
                x &= x - 1;
                atomicAdd(&s_c[w * 257 + k * 32 + bit], 1);
            }
        }
    }
    __syncthreads();
    for (int t = tid; t < nw * 8; t += 256) {
        const int w = t >> 3, k = t & 7, members = s_c[w * 257 + 256];
        if (members == 0) continue;   // a word without members keeps its bits
        uint32_t x = 0;
        for (int bit = 0; bit < 32; bit++)
            if (2 * s_c[w * 257 + k * 32 + bit] > members) x |= 1u << bit;
        uint32_t* p = (uint32_t*)(words + (size_t)(w0 + w) * 32) + k;
        if (*p != x) { *p = x; *changed = 1; }
    }
}

// k_vocab_df: n_w, the images with at least one row in word w; one workgroup per image, a flag per word in LDS, one integer add per
// (image, word present)
__global__ __launch_bounds__(256) void k_vocab_df(const int32_t* __restrict__ idx, const int32_t* __restrict__ img_off, int W, int32_t* __restrict__ n_w) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t* s_f = (int32_t*)smem;
    const int tid = threadIdx.x, r0 = img_off[blockIdx.x], r1 = img_off[blockIdx.x + 1];
    for (int w = tid; w < W; w += 256) s_f[w] = 0;
    __syncthreads();
    for (int r = r0 + tid; r < r1; r += 256) {
        const int w = idx[2 * (size_t)r];
        if ((unsigned)w < (unsigned)W) s_f[w] = 1;
    }
    __syncthreads();
    for (int w = tid; w < W; w += 256)
        if (s_f[w]) atomicAdd(&n_w[w], 1);
}

// ---- vocabulary ---------------------------------------------------------------------------------------------------------------------------
static int vocab_make(mo_ctx* c, const uint8_t* words, const int32_t* weights, int W, mo_vocab** out) {
    mo_vocab* v = new mo_vocab();
    v->c = c; v->W = W; v->Wp = (W + 7) & ~7;
    v->h_words.assign(words, words + (size_t)W * 32);
    v->h_weights.assign((size_t)v->Wp, 0);
    std::memcpy(v->h_weights.data(), weights, (size_t)W * 4);
    int rc;
    if ((rc = v->words.upload(c, v->h_words)) || (rc = v->weights.upload(c, v->h_weights))) { delete v; return rc; }
    v->h_weights.resize((size_t)W);
    *out = v;
    return MO_OK;
}

extern "C" int mo_vocab_create(mo_ctx* c, const uint8_t* words, const int32_t* weights, int32_t n_words, mo_vocab** out) {
    if (!c) return MO_ERR_ARG;
    if (!words || !weights || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (n_words < 2 || n_words > MO_BOW_MAX_WORDS) return mo_fail(c, MO_ERR_ARG, "a vocabulary has 2 .. 8192 words");
    for (int w = 0; w < n_words; w++)
        if (weights[w] < 0 || weights[w] > MO_BOW_MAX_WEIGHT) return mo_fail(c, MO_ERR_ARG, "a word weight must be in 0 .. 14 * 1024");
    MO_ENTER(c);
    return vocab_make(c, words, weights, n_words, out);
}

extern "C" int mo_vocab_words(const mo_vocab* v) { return v ? v->W : MO_ERR_ARG; }

extern "C" int mo_vocab_download(const mo_vocab* v, uint8_t* words, int32_t* weights) {
    if (!v) return MO_ERR_ARG;
    if (words) std::memcpy(words, v->h_words.data(), v->h_words.size());
    if (weights) std::memcpy(weights, v->h_weights.data(), v->h_weights.size() * 4);
    return MO_OK;
}

extern "C" void mo_vocab_destroy(mo_vocab* v) {
    if (!v) return;
    hipSetDevice(v->c->device);
    hipStreamSynchronize(v->c->stream);
    delete v;
}

extern "C" int mo_vocab_train(mo_ctx* c, const uint8_t* desc, int32_t n, const int32_t* img_off, int32_t n_img, int32_t n_words, int32_t iters,
                              mo_vocab** out, int32_t* iters_run) {
    if (!c) return MO_ERR_ARG;
    if (!desc || !img_off || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (iters_run) *iters_run = 0;
    const int W = n_words;
    if (W < 2 || W > MO_BOW_MAX_WORDS) return mo_fail(c, MO_ERR_ARG, "a vocabulary has 2 .. 8192 words");
    if (n < W) return mo_fail(c, MO_ERR_ARG, "fewer training descriptors than words");
    if (n_img < 1 || n_img > MO_BOW_MAX_IMAGES) return mo_fail(c, MO_ERR_ARG, "training needs 1 .. 2^20 images");
    if (iters < 0) return mo_fail(c, MO_ERR_ARG, "iters must be >= 0");
    if (img_off[0] != 0 || img_off[n_img] != n) return mo_fail(c, MO_ERR_ARG, "image offsets must run from 0 to n");
    for (int i = 0; i < n_img; i++)
        if (img_off[i + 1] < img_off[i]) return mo_fail(c, MO_ERR_ARG, "image offsets must not decrease");
    MO_ENTER(c);
    std::vector<uint8_t> h_words((size_t)W * 32);
    for (int j = 0; j < W; j++) std::memcpy(&h_words[(size_t)j * 32], desc + (size_t)(((int64_t)j * n) / W) * 32, 32);
    DevBuf<uint8_t> d_desc, d_words, d_pass;
    DevBuf<int32_t> d_idx, d_dist, d_changed, d_off, d_nw;
    int rc;
    if ((rc = d_desc.reserve_exact(c, (size_t)n * 32)) || (rc = d_words.upload(c, h_words)) || (rc = d_idx.reserve_exact(c, (size_t)n * 2)) ||
        (rc = d_dist.reserve_exact(c, (size_t)n * 2)) || (rc = d_pass.reserve_exact(c, (size_t)n)) || (rc = d_changed.reserve_exact(c, 1)) ||
        (rc = d_off.reserve_exact(c, (size_t)n_img + 1)) || (rc = d_nw.reserve_exact(c, (size_t)W)))
        return rc;
    HIPCHK(c, hipMemcpyAsync(d_desc, desc, (size_t)n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_off, img_off, ((size_t)n_img + 1) * 4, hipMemcpyHostToDevice, c->stream));
    auto quantise = [&]() { return match_launch_pairs(c, d_desc, d_words, 0, 0, nullptr, nullptr, nullptr, n, W, 1, n, -1.0, d_idx, d_dist, d_pass); };
    const int wpb = std::max(1, std::min(32, W / 256));
    bool current = false;   // d_idx holds the words of every row under the words as they stand
    int ran = 0;
    for (int it = 0; it < iters; it++) {
        if ((rc = quantise())) return rc;
        HIPCHK(c, hipMemsetAsync(d_changed, 0, 4, c->stream));
        hipLaunchKernelGGL(k_vocab_update, dim3((unsigned)((W + wpb - 1) / wpb)), dim3(256), (size_t)wpb * 257 * 4, c->stream, d_idx, d_desc, n, W, wpb,
                           d_words, d_changed);
        HIPCHK(c, hipGetLastError());
        int32_t changed = 0;
        HIPCHK(c, hipMemcpyAsync(&changed, d_changed, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ran++;
        current = !changed;
        if (!changed) break;
    }
    if (!current && (rc = quantise())) return rc;
    HIPCHK(c, hipMemsetAsync(d_nw, 0, (size_t)W * 4, c->stream));
    hipLaunchKernelGGL(k_vocab_df, dim3((unsigned)n_img), dim3(256), (size_t)((W + 3) & ~3) * 4, c->stream, d_idx, d_off, W, d_nw);
    HIPCHK(c, hipGetLastError());
    std::vector<int32_t> n_w((size_t)W), weights((size_t)W);
    HIPCHK(c, hipMemcpyAsync(n_w.data(), d_nw, (size_t)W * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_words.data(), d_words, (size_t)W * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int w = 0; w < W; w++) weights[w] = (int32_t)std::rint(std::log((double)n_img / (double)std::max(n_w[w], 1)) * 1024.0);
    if (iters_run) *iters_run = ran;
    return vocab_make(c, h_words.data(), weights.data(), W, out);
}

// ---- the database on mo_map ---------------------------------------------------------------------------------------------------------------
extern "C" int mo_map_set_vocabulary(mo_map* m, mo_vocab* v) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (v && v->c != c) return mo_fail(c, MO_ERR_ARG, "the vocabulary belongs to another context");
    MAP_ENTER(m);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    map_feature_drop<BowBufs>(m);
    if (v) {
        BowBufs& b = map_feature<BowBufs>(m);
        b.v = v;
        b.Wp = v->Wp;
    }
    return MO_OK;
}

int bow_require(mo_map* m) {
    return map_feature_if<BowBufs>(m) ? MO_OK : mo_fail(m->c, MO_ERR_ARG, "no vocabulary attached to the map (mo_map_set_vocabulary)");
}

// every stale row and the frame's row brought up to date: one quantise launch (a pair per stale keyframe and one for the frame), one
// histogram launch.  frame false (mo_map_loop_candidates: no frame is staged): the spare slot is in neither list and its row stays as
// it is; with no stale keyframe nothing is launched, the two stage marks are still set.
// marks false (mo_map_track_reference, which sets one mark of its own): neither mark is set.
static int bow_update(mo_map* m, int n, bool frame = true, bool marks = true) {
    mo_ctx* c = m->c;
    BowBufs& b = *map_feature_if<BowBufs>(m);
    const mo_vocab& v = *b.v;
    const int spare = m->kslots, rows = m->kslots + 1, row = m->row;
    int rc;
    if (n > MO_BOW_MAX_ROWS) return mo_fail(c, MO_ERR_UNSUPPORTED, "a frame of more than 65535 rows would wrap a term count");
    b.done.resize((size_t)m->n_slots, 0);
    b.h_lst.clear();
    for (int s : m->pos_slot)
        if (b.done[s] != m->kserial[s]) {
            if (m->h_kcnt[s] > MO_BOW_MAX_ROWS) return mo_fail(c, MO_ERR_UNSUPPORTED, "a keyframe of more than 65535 rows would wrap a term count");
            b.h_lst.push_back(s);
        }
    if (frame) b.h_lst.push_back(spare);
    const int n_list = (int)b.h_lst.size();
    if (rows > b.db_rows) {   // the store gained slots: the rows made so far move with it (the spare row is made again by every call)
        const size_t keep = (size_t)std::min(b.db_rows, m->n_slots);
        const int nr = std::max(rows, b.db_rows + b.db_rows / 2);
        if ((rc = b.db.regrow(c, (size_t)nr * b.Wp, keep * b.Wp)) || (rc = b.norm.regrow(c, (size_t)nr, keep))) return rc;
        b.db_rows = nr;
    }
    if (b.db_rows > b.word_rows || row > b.wstride) {   // ... and so do the words, which also follow a restride of the store
        DevBuf<uint16_t> w2;
        const int ns = std::max(row, b.wstride);
        if ((rc = w2.regrow(c, (size_t)b.db_rows * ns, 0))) return rc;
        const size_t keep = (size_t)std::min(b.word_rows, m->n_slots);
        if (keep && b.wstride)
            HIPCHK(c, hipMemcpy2DAsync(w2, (size_t)ns * 2, b.word, (size_t)b.wstride * 2, (size_t)b.wstride * 2, keep, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        b.word.swap(w2); b.wstride = ns; b.word_rows = b.db_rows;   // (the old block is freed here, behind the synchronisation)
    }
    const int stride = std::max(row, v.W);   // the matcher clips both sides of a pair to its output stride
    const size_t out_n = (size_t)n_list * stride;
    b.h_up.assign((size_t)rows + 2 + 2 * (size_t)n_list, 0);
    std::copy(m->h_kcnt.begin(), m->h_kcnt.begin() + m->n_slots, b.h_up.begin());
    b.h_up[spare] = frame ? n : 0; b.h_up[rows] = v.W;
    std::copy(b.h_lst.begin(), b.h_lst.end(), b.h_up.begin() + rows + 2);
    std::fill(b.h_up.begin() + rows + 2 + n_list, b.h_up.end(), rows);
    if ((rc = mo_reserve(c, b.up, b.h_up.size(), b.match, out_n))) return rc;
    b.cnt = b.up; b.lst = b.up + rows + 2; b.ltf = b.lst + n_list;
    HIPCHK(c, hipMemcpyAsync(b.up, b.h_up.data(), b.h_up.size() * 4, hipMemcpyHostToDevice, c->stream));
    // train frame `rows` of a stride of 0 bytes: the words themselves
    if ((rc = match_launch_pairs(c, m->kdesc, v.words, (size_t)row * 32, 0, b.cnt, b.lst, b.ltf, 0, 0, n_list, stride, -1.0, b.match.idx, b.match.dist, b.match.pass)))
        return rc;
    if (marks) mo_stage_mark(c, "bow_quantise");
    if (n_list > 0) {
        hipLaunchKernelGGL(k_bow_hist, dim3((unsigned)n_list), dim3(256), (size_t)b.Wp * 4 + BOW_RED_BYTES, c->stream, b.lst, b.cnt, stride, b.match.idx.p, v.W, b.Wp,
                           v.weights.p, 0, b.db.p, b.norm.p, b.word.p, b.wstride);
        HIPCHK(c, hipGetLastError());
    }
    if (marks) mo_stage_mark(c, "bow_hist");
    for (int i = 0; i < n_list - (frame ? 1 : 0); i++) b.done[b.h_lst[i]] = m->kserial[b.h_lst[i]];
    return MO_OK;
}

// update, scores and ranking for the frame staged in the spare slot, enqueued; sel: also the matcher's pair list
static int bow_enqueue(mo_map* m, int n, int n_best, bool sel) {
    mo_ctx* c = m->c;
    BowBufs& b = *map_feature_if<BowBufs>(m);
    const int n_kf = (int)m->pos_slot.size(), spare = m->kslots;
    int rc;
    if ((rc = bow_update(m, n))) return rc;
    const size_t nb = (size_t)std::max(n_best, 1);
    if ((rc = mo_reserve(c, b.score, (size_t)n_kf, b.out_pos, nb, b.out_score, nb, b.out_n, 1)) ||
        (sel && (rc = mo_reserve(c, b.sel_qf, nb, b.sel_tf, nb, b.mrow, (size_t)n_kf))))
        return rc;
    hipLaunchKernelGGL(k_bow_score<false>, dim3((unsigned)std::min(n_kf, 1024)), dim3(256), (size_t)b.Wp * 4 + BOW_RED_BYTES, c->stream, m->d_pos_slot, n_kf, spare,
                       b.db.p, b.norm.p, b.db.p, b.norm.p, b.v->weights.p, b.Wp, b.score.p, BowCommonArg<false>{});
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "bow_score");
    hipLaunchKernelGGL(k_bow_rank, dim3(1), dim3(1024), 1024 * 8 + 16, c->stream, b.score, n_kf, n_best, b.out_pos, b.out_score, b.out_n, m->d_pos_slot, spare,
                       spare, m->kslots + 2, sel ? (int32_t*)b.sel_qf : nullptr, sel ? (int32_t*)b.sel_tf : nullptr, sel ? (int32_t*)b.mrow : nullptr);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "bow_rank");
    return MO_OK;
}

int bow_select_enqueue(mo_map* m, int n, int n_pre, BowSel* sel) {
    if (int rc = bow_enqueue(m, n, n_pre, true)) return rc;
    BowBufs& b = *map_feature_if<BowBufs>(m);
    sel->cnt = b.cnt; sel->qf = b.sel_qf; sel->tf = b.sel_tf; sel->mrow = b.mrow;
    return MO_OK;
}

int bow_update_enqueue(mo_map* m) { return bow_update(m, 0, false); }

int bow_words_enqueue(mo_map* m, int n, BowWords* out) {
    if (int rc = bow_update(m, n, true, false)) return rc;
    BowBufs& b = *map_feature_if<BowBufs>(m);
    out->word = b.word; out->stride = b.wstride; out->W = b.v->W;
    return MO_OK;
}

extern "C" int mo_map_keyframe_words(mo_map* m, int32_t kf_pos, int32_t* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    int rc;
    if ((rc = bow_require(m))) return rc;
    const int n_kf = (int)m->pos_slot.size();
    const int pos = kf_pos < 0 ? kf_pos + n_kf : kf_pos;
    if (pos < 0 || pos >= n_kf) return mo_fail(c, MO_ERR_INDEX, "keyframe position out of range");
    MAP_ENTER(m);
    HostClock clk(c);
    mo_stage_begin(c);
    if ((rc = bow_update(m, 0, false))) return rc;
    BowBufs& b = *map_feature_if<BowBufs>(m);
    const int slot = m->pos_slot[pos], n = m->h_kcnt[slot];
    std::vector<uint16_t> h((size_t)n);
    if (n) HIPCHK(c, hipMemcpyAsync(h.data(), b.word + (size_t)slot * b.wstride, (size_t)n * 2, hipMemcpyDeviceToHost, c->stream));
    if ((rc = map_sync(c, clk))) return rc;
    for (int i = 0; i < n; i++) out[i] = h[i];
    return MO_OK;
}

int bow_loop_score_enqueue(mo_map* m, int q_pos, const int32_t* wrow, int min_w, BowLoop* out) {
    mo_ctx* c = m->c;
    BowBufs& b = *map_feature_if<BowBufs>(m);
    const int n_kf = (int)m->pos_slot.size(), q_slot = m->pos_slot[q_pos];
    int rc;
    if ((rc = mo_reserve(c, b.score, (size_t)n_kf, b.common, (size_t)n_kf))) return rc;
    hipLaunchKernelGGL(k_bow_score<true>, dim3((unsigned)std::min(n_kf, 1024)), dim3(256), (size_t)b.Wp * 4 + BOW_RED_BYTES, c->stream, m->d_pos_slot, n_kf,
                       q_slot, b.db.p, b.norm.p, b.db.p, b.norm.p, b.v->weights.p, b.Wp, b.score.p, BowCommonArg<true>{wrow, q_pos, min_w, b.common});
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "loop_score");
    out->cnt = b.cnt; out->score = b.score; out->common = b.common; out->empty = m->kslots + 2;
    return MO_OK;
}

// a thread per keyframe position; the scoring kernel stays the code it is
__global__ __launch_bounds__(256) void k_bow_among(const uint8_t* __restrict__ among, int n_kf, int32_t* __restrict__ common) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n_kf && !among[k]) common[k] = 0;
}

int bow_loop_among_enqueue(mo_map* m, const uint8_t* among) {
    mo_ctx* c = m->c;
    BowBufs& b = *map_feature_if<BowBufs>(m);
    const int n_kf = (int)m->pos_slot.size();
    hipLaunchKernelGGL(k_bow_among, dim3((unsigned)((n_kf + 255) / 256)), dim3(256), 0, c->stream, among, n_kf, b.common.p);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "loop_among");
    return MO_OK;
}

extern "C" int mo_map_query_keyframes(mo_map* m, const mo_frame_ref* f, const mo_map_query_params* prm, mo_map_query_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!f || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (prm->n_best < 0) return mo_fail(c, MO_ERR_ARG, "n_best must be >= 0");
    if (prm->n_best > 0 && (!out->pos || !out->score)) return mo_fail(c, MO_ERR_ARG, "pos and score must hold n_best entries");
    int rc;
    if ((rc = bow_require(m))) return rc;
    MAP_ENTER(m);
    HostClock clk(c);
    const int nb = prm->n_best;
    out->n = 0; out->from_token = 0;
    for (int i = 0; i < nb; i++) { out->pos[i] = -1; out->score[i] = 0.0; }
    int n;
    mo_keypoint* qk; uint8_t* qdesc;
    if ((rc = map_stage_frame(m, f, false, &out->from_token, [](int) {}, &n, &qk, &qdesc)) || !qk || nb == 0) return rc;   // (nothing to rank: not an error)
    if ((rc = bow_enqueue(m, n, nb, false))) return rc;
    BowBufs& b = *map_feature_if<BowBufs>(m);
    HIPCHK(c, hipMemcpyAsync(out->pos, b.out_pos, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out->score, b.out_score, (size_t)nb * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&out->n, b.out_n, 4, hipMemcpyDeviceToHost, c->stream));
    return map_sync(c, clk);
}

// ---- a batch of query frames (bow.h) ------------------------------------------------------------------------------------------------
struct BowBatchBufs : MapFeature {
    DevBuf<int32_t> lst;                 // [2 nf]: the quantisation's pair list - query frame S + f (also the histogram's list), then the words' frame
    MatchBufs match;                     // [nf][max(stride, W)]: idx[2 * r] is the word of query row r
    DevBuf<uint16_t> db;                 // [nf][Wp] term counts of every frame
    DevBuf<long long> norm;              // [nf]
    DevBuf<double> score;                // [nf][n_kf]
    DevBuf<int32_t> out_pos, out_n; DevBuf<double> out_score;   // [nf][n_best], [nf]
    DevBuf<int32_t> sel_qf, sel_tf, mrow;                       // [nf][n_best], [nf][n_kf]
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) {
        f(lst); match.each_scratch(f); f(db); f(norm); f(score); f(out_pos); f(out_n); f(out_score); f(sel_qf); f(sel_tf); f(mrow);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
    PinnedBuf<int32_t> h_lst;            // (pinned host side, not device scratch)
};

int bow_words(const mo_map* m) {
    const BowBufs* b = map_feature_if<BowBufs>(m);
    return b ? b->v->W : 0;
}

int bow_batch_enqueue(mo_map* m, const uint8_t* fdesc, const int32_t* cnt, const int32_t* h_fcnt, int nf, int stride, int n_best, bool sel, BowBatch* out) {
    mo_ctx* c = m->c;
    BowBufs& b = *map_feature_if<BowBufs>(m);
    const mo_vocab& v = *b.v;
    const int n_kf = (int)m->pos_slot.size(), S = m->kslots + 1;
    int rc;
    for (int f = 0; f < nf; f++)
        if (h_fcnt[f] > MO_BOW_MAX_ROWS) return mo_fail(c, MO_ERR_UNSUPPORTED, "a frame of more than 65535 rows would wrap a term count");
    if ((rc = bow_update(m, 0, false, false))) return rc;   // the stale keyframe slots, once; the spare row stays as it is
    BowBatchBufs& bb = map_feature<BowBatchBufs>(m);
    const int qs = std::max(stride, v.W);   // the matcher clips both sides of a pair to its output stride
    const size_t nb = (size_t)nf * std::max(n_best, 1), nk = (size_t)nf * n_kf;
    if ((rc = mo_reserve(c, bb.h_lst, 2 * (size_t)nf, bb.lst, 2 * (size_t)nf, bb.match, (size_t)nf * qs, bb.db, (size_t)nf * b.Wp, bb.norm, (size_t)nf, bb.score, nk,
                         bb.out_pos, nb, bb.out_score, nb, bb.out_n, (size_t)nf)) ||
        (sel && (rc = mo_reserve(c, bb.sel_qf, nb, bb.sel_tf, nb, bb.mrow, nk))))
        return rc;
    for (int f = 0; f < nf; f++) { bb.h_lst[f] = S + f; bb.h_lst[nf + f] = S + nf; }
    HIPCHK(c, hipMemcpyAsync(bb.lst, bb.h_lst, 2 * (size_t)nf * 4, hipMemcpyHostToDevice, c->stream));
    // one pair per frame; the words are train frame S + nf of a stride of 0 bytes
    if ((rc = match_launch_pairs(c, bow_batch_qbase(fdesc, S, (size_t)stride), v.words, (size_t)stride * 32, 0, cnt, bb.lst, bb.lst + nf, 0, 0, nf, qs, -1.0,
                                 bb.match.idx, bb.match.dist, bb.match.pass)))
        return rc;
    hipLaunchKernelGGL(k_bow_hist, dim3((unsigned)nf), dim3(256), (size_t)b.Wp * 4 + BOW_RED_BYTES, c->stream, bb.lst.p, cnt, qs, bb.match.idx.p, v.W, b.Wp,
                       v.weights.p, S, bb.db.p, bb.norm.p, (uint16_t*)nullptr, 0);
    // a frame's workgroups keep its q_w in LDS and stride over the keyframes: fewer per frame as the batch grows
    const unsigned gx = (unsigned)std::max(1, std::min(std::min(n_kf, 1024), 4096 / nf));
    hipLaunchKernelGGL(k_bow_score<false>, dim3(gx, (unsigned)nf), dim3(256), (size_t)b.Wp * 4 + BOW_RED_BYTES, c->stream, m->d_pos_slot.p, n_kf, 0, bb.db.p,
                       bb.norm.p, b.db.p, b.norm.p, v.weights.p, b.Wp, bb.score.p, BowCommonArg<false>{});
    hipLaunchKernelGGL(k_bow_rank, dim3((unsigned)nf), dim3(1024), 1024 * 8 + 16, c->stream, bb.score.p, n_kf, n_best, bb.out_pos.p, bb.out_score.p, bb.out_n.p,
                       m->d_pos_slot.p, S, S + nf + 1, S + nf + 1, sel ? bb.sel_qf.p : nullptr, sel ? bb.sel_tf.p : nullptr, sel ? bb.mrow.p : nullptr);
    HIPCHK(c, hipGetLastError());
    out->pos = bb.out_pos; out->score = bb.out_score; out->n = bb.out_n; out->qf = bb.sel_qf; out->tf = bb.sel_tf; out->mrow = bb.mrow;
    return MO_OK;
}
