// twoview_h.hip -- the homography branch of the two-view initialisation on gfx950 (fp64 vector ALU), after ORB-SLAM2's Initializer:
// a homography is computed beside the essential matrix of twoview_kernels.hip, both are scored, RH = SH / (SH + SF) names the model,
// and the homography is decomposed after Faugeras with CheckRT over the eight candidates (homography.h holds every per-item rule).
//
//   k_h_prep    per pair: pixel correspondences -> f64, the two Hartley normalisations, normalised coordinates, DLT rows
//   k_h_hyp     one thread per hypothesis: 4-sample (the first four of the sample8 stream), closed-form H, denormalised to pixels
//   k_h_score   one workgroup per 64 hypotheses (one per lane), wavefront k sums part k of the correspondences (scalar operands):
//               the canonical cost (P0 + P1) + (P2 + P3) of the truncated symmetric transfer error -> one atomicMin per tile
//   k_h_refit   one block per pair: DLT refits on the inliers, SH / SF / RH, ReconstructH -> the eight candidates
//   k_h_check_rt  one thread per (correspondence, candidate) over the whole chip: CheckRT, integer counts
//   k_h_finish  one block per pair: parallax of each candidate, selection, acceptance, the best candidate's map points
// Built with the Makefile's default flags (-ffp-contract=off): a host build of homography.h rounds the same way.
#include "common.h"
#include "homography.h"
#include "tv_eig9.h"

#define TH_BLOCK 256
#define THF_BLOCK 512  // k_h_refit / k_h_finish: 8 wavefronts - one per part of the normal matrix, one per candidate in the parallax selection
#define TH_PARTS 4     // the canonical cost is summed in this many contiguous parts (TV_PARTS of the essential path)
#define THF_NPARTS (THF_BLOCK / 64)

struct HfWork {
    double* px;     // [pairs][cap][4] pixel u1, v1, u2, v2
    double* xn;     // [pairs][cap][4] the same, each image Hartley-normalised
    double* rows;   // [pairs][cap][18] DLT rows of correspondence i in normalised coordinates
    double* norm;   // [pairs][8] image 1: s, cx, cy; image 2: s, cx, cy
    double* hyp;    // [pairs][n_hyp][9] H of hypothesis h in pixels, [0] = NaN: no model
    double* wH;     // [pairs][tiles][9] the best H of each scoring tile
    unsigned long long* wkey;  // [pairs][tiles] its key
    unsigned long long* best;  // [pairs] (float32 bits of the cost << 32) | hypothesis, minimum wins
    unsigned long long* ckey;  // [pairs][8][cap] k_h_check_rt: order-preserving bit pattern of each passed point's cos (~0: not passed)
    double* cand;   // [pairs][96] k_h_refit: R (8 x 9) and t (8 x 3) of the candidates
    float* Xc;      // [pairs][8][cap][3] k_h_check_rt: the point of correspondence i under candidate c, where it is a map point
    int* ngood;     // [pairs][8] points that passed CheckRT under candidate c (integer atomics)
    int* state;     // [pairs][4] k_h_refit: [0] a homography was found, [1] it decomposed, [2] its inliers, [3] refits
    uint8_t* mcur;  // [pairs][cap] inlier set of the current H
    uint8_t* mprev; // [pairs][cap] ... of the H before the last refit
    uint8_t* gb;    // [pairs][8][cap] 1: a map point under candidate c
};

static size_t hf_workspace_bytes(int n_pairs, int cap, int n_hyp) {
    const size_t p = (size_t)n_pairs, nt = (size_t)((n_hyp + 63) / 64);
    return p * ((size_t)cap * (4 + 4 + 18 + 8) * 8 + (8 + 96) * 8 + (size_t)n_hyp * 9 * 8 + nt * 10 * 8 + 8 + (size_t)cap * 8 * 3 * 4 + 12 * 4 +
                (size_t)cap * (2 + 8)) + 256;
}

static HfWork hf_carve(void* base, int n_pairs, int cap, int n_hyp) {
    HfWork w;
    uint8_t* b = (uint8_t*)base;
    const size_t p = (size_t)n_pairs, nt = (size_t)((n_hyp + 63) / 64);
    w.px = (double*)b; b += p * cap * 4 * 8;
    w.xn = (double*)b; b += p * cap * 4 * 8;
    w.rows = (double*)b; b += p * cap * 18 * 8;
    w.ckey = (unsigned long long*)b; b += p * cap * 8 * 8;
    w.norm = (double*)b; b += p * 8 * 8;
    w.hyp = (double*)b; b += p * (size_t)n_hyp * 9 * 8;
    w.wH = (double*)b; b += p * nt * 9 * 8;
    w.wkey = (unsigned long long*)b; b += p * nt * 8;
    w.best = (unsigned long long*)b; b += p * 8;
    w.cand = (double*)b; b += p * 96 * 8;
    w.Xc = (float*)b; b += p * cap * 8 * 3 * 4;
    w.ngood = (int*)b; b += p * 8 * 4;
    w.state = (int*)b; b += p * 4 * 4;
    w.mcur = b; b += p * cap;
    w.mprev = b; b += p * cap;
    w.gb = b;
    return w;
}

// sums over the block in a fixed order (lanes by butterfly, wavefronts in sequence): equal inputs give equal bytes
template <int NW> __device__ inline double h_block_sum(double v, double* s_red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0;
    for (int k = 0; k < NW; k++) r += s_red[k];
    return r;
}
template <int NW> __device__ inline int h_block_sum_i(int v, int* s_red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = 0;
    for (int k = 0; k < NW; k++) r += s_red[k];
    return r;
}

// ---------------------------------------------------------------- prep ----------------------------
__global__ __launch_bounds__(TH_BLOCK) void k_h_prep(HfArgs a, HfWork w) {
    __shared__ double s_red[TH_BLOCK / 64];
    __shared__ double s_nm[6];
    const int pair = blockIdx.x, tid = threadIdx.x, m = a.m_fixed;
    double* px = w.px + (size_t)pair * a.cap * 4;
    double* xn = w.xn + (size_t)pair * a.cap * 4;
    double* rows = w.rows + (size_t)pair * a.cap * 18;
    const float* p1 = a.d_p1 + (size_t)pair * m * 2;
    const float* p2 = a.d_p2 + (size_t)pair * m * 2;
    const int nt = (a.n_hyp + 63) / 64;
    if (tid == 0) w.best[pair] = ~0ull;
    for (int j = tid; j < nt; j += TH_BLOCK) w.wkey[(size_t)pair * nt + j] = ~0ull;
    double acc[4] = {0, 0, 0, 0};
    for (int i = tid; i < m; i += TH_BLOCK) {
        const double u1 = (double)p1[2 * i], v1 = (double)p1[2 * i + 1], u2 = (double)p2[2 * i], v2 = (double)p2[2 * i + 1];
        px[4 * i] = u1; px[4 * i + 1] = v1; px[4 * i + 2] = u2; px[4 * i + 3] = v2;
        acc[0] += u1; acc[1] += v1; acc[2] += u2; acc[3] += v2;
    }
    double sum[4];
    for (int k = 0; k < 4; k++) sum[k] = h_block_sum<TH_BLOCK / 64>(acc[k], s_red);
    if (tid == 0) { hg_norm_centroid(sum[0], sum[1], m, s_nm); hg_norm_centroid(sum[2], sum[3], m, s_nm + 3); }
    __syncthreads();
    double n1[3] = {0.0, s_nm[1], s_nm[2]}, n2[3] = {0.0, s_nm[4], s_nm[5]};
    double d1 = 0, d2 = 0;
    for (int i = tid; i < m; i += TH_BLOCK) {  // (each thread reads back what it wrote)
        d1 += hg_norm_dist(px[4 * i], px[4 * i + 1], n1);
        d2 += hg_norm_dist(px[4 * i + 2], px[4 * i + 3], n2);
    }
    const double sd1 = h_block_sum<TH_BLOCK / 64>(d1, s_red), sd2 = h_block_sum<TH_BLOCK / 64>(d2, s_red);
    hg_norm_scale(sd1, m, n1);
    hg_norm_scale(sd2, m, n2);
    if (tid == 0) {
        double* o = w.norm + (size_t)pair * 8;
        for (int k = 0; k < 3; k++) { o[k] = n1[k]; o[3 + k] = n2[k]; }
    }
    for (int i = tid; i < m; i += TH_BLOCK) {
        const double x1 = n1[0] * (px[4 * i] - n1[1]), y1 = n1[0] * (px[4 * i + 1] - n1[2]);
        const double x2 = n2[0] * (px[4 * i + 2] - n2[1]), y2 = n2[0] * (px[4 * i + 3] - n2[2]);
        xn[4 * i] = x1; xn[4 * i + 1] = y1; xn[4 * i + 2] = x2; xn[4 * i + 3] = y2;
        double r[18];
        hg_dlt_rows(x1, y1, x2, y2, r);
        for (int k = 0; k < 18; k++) rows[(size_t)i * 18 + k] = r[k];
    }
}

// ---------------------------------------------------------------- hypotheses ----------------------
__global__ __launch_bounds__(TH_BLOCK) void k_h_hyp(HfArgs a, HfWork w) {
    const int pair = blockIdx.y, h = blockIdx.x * TH_BLOCK + threadIdx.x, m = a.m_fixed;
    if (h >= a.n_hyp) return;
    const double* xn = w.xn + (size_t)pair * a.cap * 4;
    const double* nm = w.norm + (size_t)pair * 8;
    int idx[4];
    hg_sample4(hg_stream_seed(a.seed, (uint64_t)pair + a.pair_base), h, m, idx);  // GLOBAL pair index, as the essential path
    double pts[16], Hn[9], H[9];
    for (int k = 0; k < 4; k++)
        for (int j = 0; j < 4; j++) pts[k * 4 + j] = xn[(size_t)idx[k] * 4 + j];
    bool ok = hg_homography4(pts, Hn);
    if (ok) {
        hg_denormalise(Hn, nm, nm + 3, H);
        double nn = 0.0;
        for (int j = 0; j < 9; j++) nn += H[j] * H[j];
        ok = nn > 0.0 && hg_finite(nn);
    }
    double* o = w.hyp + ((size_t)pair * a.n_hyp + h) * 9;
    for (int j = 0; j < 9; j++) o[j] = ok ? H[j] : __longlong_as_double(0x7FF8000000000000ll);
}

// ---------------------------------------------------------------- scoring -------------------------
__global__ __launch_bounds__(64 * TH_PARTS) void k_h_score(HfArgs a, HfWork w) {
    __shared__ double s_part[TH_PARTS][64];
    typedef const __attribute__((address_space(4))) double* cdp;  // wave-uniform scalar loads (k_h_prep wrote them in an earlier launch)
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6, pair = blockIdx.y, tile = blockIdx.x, m = a.m_fixed;
    const int h = tile * 64 + lane;
    const bool in_range = h < a.n_hyp;
    const double* rec = w.hyp + ((size_t)pair * a.n_hyp + (in_range ? h : 0)) * 9;
    double H[9], Hi[9];
    for (int j = 0; j < 9; j++) H[j] = rec[j];
    const bool valid = in_range && H[0] == H[0];
    hg_adj3(H, Hi);
    const cdp pts = (cdp)(uintptr_t)(w.px + (size_t)pair * a.cap * 4);
    const double inv_s2 = 1.0 / (a.sigma * a.sigma);
    const int q = (m + TH_PARTS - 1) / TH_PARTS, i0 = min(m, part * q), i1 = min(m, (part + 1) * q);
    double s = 0.0;
    for (int i = i0; i < i1; i++) {
        double c1, c2;
        hg_transfer_chi(H, Hi, pts[4 * i], pts[4 * i + 1], pts[4 * i + 2], pts[4 * i + 3], inv_s2, &c1, &c2);
        s += hg_cost_term(c1, c2);
    }
    s_part[part][lane] = s;
    __syncthreads();
    if (part != 0) return;
    const double cost = (s_part[0][lane] + s_part[1][lane]) + (s_part[2][lane] + s_part[3][lane]);
    unsigned long long key = ~0ull;
    if (valid && cost == cost) key = ((unsigned long long)__float_as_uint((float)cost) << 32) | (unsigned long long)(unsigned)h;
    const unsigned long long own = key;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, 64);
        key = other < key ? other : key;
    }
    if (key != ~0ull && own == key) {  // exactly one lane: the keys are unique, the lowest hypothesis wins a tie
        const size_t slot = (size_t)pair * ((a.n_hyp + 63) / 64) + tile;
        for (int j = 0; j < 9; j++) w.wH[slot * 9 + j] = H[j];
        w.wkey[slot] = key;
        atomicMin(&w.best[pair], key);
    }
}

// ---------------------------------------------------------------- refits, scores, decomposition ---
// order-preserving 64-bit pattern of a double (NaN-free input)
__device__ __forceinline__ unsigned long long h_sort_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double h_sort_val(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? k & 0x7FFFFFFFFFFFFFFFull : ~k));
}

__global__ __launch_bounds__(THF_BLOCK) void k_h_refit(HfArgs a, HfWork w) {
    __shared__ double s_red[THF_NPARTS];
    __shared__ int s_redi[THF_NPARTS];
    __shared__ double s_H[9], s_N[45], s_M[48], s_x[9], s_part[THF_NPARTS][48];
    __shared__ int s_stop;
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = a.m_fixed;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const float qnanf = __uint_as_float(0x7FC00000u);
    double* Hout = a.d_H + (size_t)pair * 9;
    double* stat = a.d_stat + (size_t)pair * HF_NSTAT;
    int32_t* info = a.d_info + (size_t)pair * HF_NINFO;
    uint8_t* hmask = a.d_hmask + (size_t)pair * a.cap;
    uint8_t* good = a.d_good + (size_t)pair * a.cap;
    float* Xout = a.d_X + (size_t)pair * a.cap * 3;
    const double* px = w.px + (size_t)pair * a.cap * 4;
    const double* rows = w.rows + (size_t)pair * a.cap * 18;
    const double* nm = w.norm + (size_t)pair * 8;
    uint8_t* mcur = w.mcur + (size_t)pair * a.cap;
    uint8_t* mprev = w.mprev + (size_t)pair * a.cap;
    int* state = w.state + (size_t)pair * 4;
    for (int i = tid; i < m; i += THF_BLOCK) {
        Xout[3 * i] = qnanf; Xout[3 * i + 1] = qnanf; Xout[3 * i + 2] = qnanf;
        hmask[i] = 0; good[i] = 0;
    }
    if (tid < 8) w.ngood[(size_t)pair * 8 + tid] = 0;
    const double inv_s2 = 1.0 / (a.sigma * a.sigma);
    const unsigned long long best = w.best[pair];
    const bool has_h = m >= 4 && best != ~0ull;  // block-uniform
    // SF: CheckFundamental of the essential path's matrix (it ran on the same stream before this launch)
    double SF = 0.0;
    {
        double E[9], F[9];
        for (int j = 0; j < 9; j++) E[j] = a.d_E ? a.d_E[(size_t)pair * 9 + j] : qnan;
        if (E[0] == E[0]) {  // block-uniform
            hg_fundamental_from_essential(E, a.K, F);
            double sc = 0.0;
            for (int i = tid; i < m; i += THF_BLOCK) {
                double c1, c2;
                hg_fund_chi(F, px[4 * i], px[4 * i + 1], px[4 * i + 2], px[4 * i + 3], inv_s2, &c1, &c2);
                sc += hg_score_term(c1, HG_CHI2_F) + hg_score_term(c2, HG_CHI2_F);
            }
            SF = h_block_sum<THF_NPARTS>(sc, s_red);
        }
    }
    if (!has_h) {
        if (tid == 0) {
            for (int j = 0; j < 9; j++) Hout[j] = qnan;
            stat[0] = 0.0; stat[1] = SF; stat[2] = 0.0;
            for (int k = 0; k < 8; k++) { stat[3 + k] = 2.0; info[k] = 0; }
            for (int k = 11; k < HF_NSTAT; k++) stat[k] = qnan;
            info[8] = -1; info[9] = -1; info[10] = 0; info[11] = 0; info[12] = -1; info[13] = 0; info[14] = 0; info[15] = 0;
            state[0] = 0; state[1] = 0; state[2] = 0; state[3] = 0;  // (nothing left for k_h_check_rt and k_h_finish)
        }
        return;
    }
    {   // the matrix of the winning key
        const int nslot = (a.n_hyp + 63) / 64;
        for (int j = tid; j < nslot; j += THF_BLOCK)
            if (w.wkey[(size_t)pair * nslot + j] == best)
                for (int q = 0; q < 9; q++) s_H[q] = w.wH[((size_t)pair * nslot + j) * 9 + q];
    }
    __syncthreads();
    // ---- a. DLT refits on the current inliers at the fixed threshold: at most 5, until the inlier set repeats or falls below 4
    int refits = 0, n_inl = 0;
    double SH = 0.0;
    for (;;) {
        double H[9], Hi[9];
        for (int j = 0; j < 9; j++) H[j] = s_H[j];
        hg_adj3(H, Hi);
        int cnt = 0, diff = 0;
        double sc = 0.0;
        for (int i = tid; i < m; i += THF_BLOCK) {
            double c1, c2;
            hg_transfer_chi(H, Hi, px[4 * i], px[4 * i + 1], px[4 * i + 2], px[4 * i + 3], inv_s2, &c1, &c2);
            const int in = hg_inlier(c1, c2, HG_CHI2_H) ? 1 : 0;
            sc += hg_score_term(c1, HG_CHI2_H) + hg_score_term(c2, HG_CHI2_H);
            mcur[i] = (uint8_t)in;
            cnt += in;
            if (refits > 0) diff += in != (int)mprev[i];
        }
        n_inl = h_block_sum_i<THF_NPARTS>(cnt, s_redi);
        const int n_diff = h_block_sum_i<THF_NPARTS>(diff, s_redi);
        SH = h_block_sum<THF_NPARTS>(sc, s_red);
        if (n_inl < 4 || (refits > 0 && n_diff == 0) || refits == 5) break;  // block-uniform
        // normal matrix of the inliers' rows: entry e of the packed upper triangle per lane, wavefront g sums part g, parts in sequence
        {
            const int per = (m + THF_NPARTS - 1) / THF_NPARTS, i0 = min(m, wv * per), i1 = min(m, (wv + 1) * per);
            int p = 0, q = lane < 45 ? lane : 0;
            while (q >= 9 - p) { q -= 9 - p; p++; }
            q += p;
            double acc = 0.0;
#pragma unroll 4
            for (int i = i0; i < i1; i++) {  // (the rows are loaded whether selected or not: no load waits for a branch on the mask)
                const double* r = rows + (size_t)i * 18;
                const double v = r[p] * r[q] + r[9 + p] * r[9 + q];
                acc += mcur[i] ? v : 0.0;
            }
            if (lane < 48) s_part[wv][lane] = acc;
        }
        __syncthreads();
        if (tid < 45) {
            double v = 0.0;
            for (int k = 0; k < THF_NPARTS; k++) v += s_part[k][tid];
            s_N[tid] = v;
        }
        if (tid < 9) s_x[tid] = tid == 8 ? 1.0 : 0.0;  // (only the orientation of the result follows it)
        __syncthreads();
        if (tid < 64) {
            const bool conv = wave_smallest_eigvec9(s_N, s_M, s_x, tid);
            if (tid == 0) {
                double Hn[9], Hp[9], nn = 0.0;
                for (int j = 0; j < 9; j++) Hn[j] = s_x[j];
                hg_denormalise(Hn, nm, nm + 3, Hp);
                for (int j = 0; j < 9; j++) nn += Hp[j] * Hp[j];
                const bool ok = conv && nn > 0.0 && hg_finite(nn);
                if (ok) { const double r = 1.0 / sqrt(nn); for (int j = 0; j < 9; j++) s_H[j] = Hp[j] * r; }
                s_stop = ok ? 0 : 1;
            }
        }
        for (int i = tid; i < m; i += THF_BLOCK) mprev[i] = mcur[i];  // (each thread its own rows)
        __syncthreads();
        if (s_stop) break;  // the solver broke down: the previous estimate stays, and mcur / n_inl / SH are its own
        refits++;
    }
    // ---- b. scores and mask of the final H
    for (int i = tid; i < m; i += THF_BLOCK) hmask[i] = mcur[i];
    // ---- c. ReconstructH: the eight candidates go to the workspace, CheckRT is the next launch
    if (tid == 0) {
        double H[9], nn = 0.0, R[72], t[24], n[24];
        for (int j = 0; j < 9; j++) { H[j] = s_H[j]; nn += H[j] * H[j]; }
        const double r = 1.0 / sqrt(nn);
        for (int j = 0; j < 9; j++) Hout[j] = H[j] * r;
        const bool dec = hg_reconstruct(H, a.K, R, t, n);
        double* cand = w.cand + (size_t)pair * 96;
        for (int j = 0; j < 72; j++) cand[j] = dec ? R[j] : qnan;
        for (int j = 0; j < 24; j++) cand[72 + j] = dec ? t[j] : qnan;
        stat[0] = SH; stat[1] = SF; stat[2] = SH + SF > 0.0 ? SH / (SH + SF) : 0.0;
        info[10] = n_inl; info[12] = (int)(unsigned)(best & 0xFFFFFFFFull); info[13] = refits; info[14] = dec ? 1 : 0; info[15] = 0;
        state[0] = 1; state[1] = dec ? 1 : 0; state[2] = n_inl; state[3] = refits;
    }
}

// ---------------------------------------------------------------- CheckRT -------------------------
// One thread per (correspondence, candidate): grid (ceil(m / 256), 8, pairs).  The passes are independent, so they spread over the
// chip instead of queueing on the one compute unit that holds a pair's block.  Counts by integer atomics (one per block).
__global__ __launch_bounds__(TH_BLOCK) void k_h_check_rt(HfArgs a, HfWork w) {
    __shared__ int s_cnt[TH_BLOCK / 64];
    const int pair = blockIdx.z, c = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * TH_BLOCK + tid, m = a.m_fixed;
    if (!w.state[(size_t)pair * 4 + 1]) return;  // no homography, or no decomposition (block-uniform)
    const double* cand = w.cand + (size_t)pair * 96;
    const double* px = w.px + (size_t)pair * a.cap * 4;
    double R[9], t[3];
    for (int j = 0; j < 9; j++) R[j] = cand[c * 9 + j];
    for (int j = 0; j < 3; j++) t[j] = cand[72 + c * 3 + j];
    unsigned long long key = ~0ull;
    int passed = 0, is_good = 0;
    if (i < m && w.mcur[(size_t)pair * a.cap + i]) {
        double cs, X[3];
        const int r = hg_check_rt(a.K, R, t, px[4 * i], px[4 * i + 1], px[4 * i + 2], px[4 * i + 3], 4.0 * a.sigma * a.sigma, &cs, X);
        if (r & 1) { passed = 1; key = h_sort_key(cs == cs ? cs : 2.0); }
        if (r == 3) {
            is_good = 1;
            float* o = w.Xc + (((size_t)pair * 8 + c) * a.cap + i) * 3;
            o[0] = (float)X[0]; o[1] = (float)X[1]; o[2] = (float)X[2];
        }
    }
    if (i < m) {
        w.ckey[((size_t)pair * 8 + c) * a.cap + i] = key;
        w.gb[((size_t)pair * 8 + c) * a.cap + i] = (uint8_t)is_good;
    }
    const int wcnt = __popcll(__ballot(passed));
    if ((tid & 63) == 0) s_cnt[tid >> 6] = wcnt;
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int k = 0; k < TH_BLOCK / 64; k++) n += s_cnt[k];
        if (n) atomicAdd(&w.ngood[(size_t)pair * 8 + c], n);
    }
}

// ---------------------------------------------------------------- finish --------------------------
__global__ __launch_bounds__(THF_BLOCK) void k_h_finish(HfArgs a, HfWork w) {
    __shared__ double s_cos[8];
    __shared__ int s_best;
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = a.m_fixed;
    const int* state = w.state + (size_t)pair * 4;
    if (!state[0]) return;  // no homography: k_h_refit wrote the whole result (block-uniform)
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    double* stat = a.d_stat + (size_t)pair * HF_NSTAT;
    int32_t* info = a.d_info + (size_t)pair * HF_NINFO;
    uint8_t* good = a.d_good + (size_t)pair * a.cap;
    float* Xout = a.d_X + (size_t)pair * a.cap * 3;
    const double* cand = w.cand + (size_t)pair * 96;
    const unsigned long long* ckey = w.ckey + (size_t)pair * a.cap * 8;
    const int dec = state[1], n_inl = state[2];
    int n_good[8];
    for (int k = 0; k < 8; k++) n_good[k] = dec ? w.ngood[(size_t)pair * 8 + k] : 0;
    // ---- d. parallax of candidate wv (one wavefront each): the value at index min(50, count - 1) of its ascending cos values, by
    // bisection on the bit pattern (points that did not pass hold the largest key and sort behind every passed one)
    {
        int count = 0;
        for (int k = 0; k < 8; k++) count = k == wv ? n_good[k] : count;
        double cs = 2.0;
        if (count > 0) {  // wave-uniform
            const int k = min(50, count - 1);
            const unsigned long long* key = ckey + (size_t)wv * a.cap;
            unsigned long long res = 0ull;
            for (int bit = 63; bit >= 0; bit--) {
                const unsigned long long t = res | (1ull << bit);
                int below = 0;
                for (int i = lane; i < m; i += 64) below += key[i] < t ? 1 : 0;
                for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o, 64);
                if (below <= k) res = t;
            }
            cs = h_sort_val(res);
        }
        if (lane == 0) s_cos[wv] = cs;
    }
    __syncthreads();
    // ---- e. selection and acceptance
    if (tid == 0) {
        int bi, si;
        hg_select(n_good, &bi, &si);
        int bg = 0, sg = 0;
        double bc = 2.0;
        for (int k = 0; k < 8; k++) { if (k == bi) { bg = n_good[k]; bc = s_cos[k]; } if (k == si) sg = n_good[k]; }
        const bool acc = bi >= 0 && hg_accept(bg, sg, bc, a.cos_max, a.min_triangulated, n_inl);
        for (int k = 0; k < 8; k++) { stat[3 + k] = s_cos[k]; info[k] = n_good[k]; }
        for (int j = 0; j < 9; j++) stat[11 + j] = bi >= 0 ? cand[bi * 9 + j] : qnan;
        for (int j = 0; j < 3; j++) stat[20 + j] = bi >= 0 ? cand[72 + bi * 3 + j] : qnan;
        info[8] = bi; info[9] = si; info[11] = acc ? 1 : 0;
        s_best = bi;
    }
    __syncthreads();
    const int bi = s_best;
    if (bi < 0) return;
    const uint8_t* gb = w.gb + ((size_t)pair * 8 + bi) * a.cap;
    const float* Xc = w.Xc + ((size_t)pair * 8 + bi) * a.cap * 3;
    for (int i = tid; i < m; i += THF_BLOCK) {
        if (!gb[i]) continue;
        Xout[3 * i] = Xc[3 * i]; Xout[3 * i + 1] = Xc[3 * i + 1]; Xout[3 * i + 2] = Xc[3 * i + 2];
        good[i] = 1;
    }
}

int twoview_h_launch(mo_ctx* c, const HfArgs& a) {
    if (a.n_pairs <= 0) return MO_OK;
    if (a.n_hyp < 1 || a.n_hyp > (1 << 20)) return mo_fail(c, MO_ERR_ARG, "n_hyp_h out of range");
    if (a.m_fixed < 4 || a.m_fixed > a.cap) return mo_fail(c, MO_ERR_ARG, "the homography branch needs 4 <= m <= cap correspondences");
    if (!(a.sigma > 0.0)) return mo_fail(c, MO_ERR_ARG, "sigma must be positive");
    int rc = c->d_hf.reserve_exact(c, hf_workspace_bytes(a.n_pairs, a.cap, a.n_hyp));
    if (rc) return rc;
    const HfWork w = hf_carve(c->d_hf, a.n_pairs, a.cap, a.n_hyp);
    hipLaunchKernelGGL(k_h_prep, dim3(a.n_pairs), dim3(TH_BLOCK), 0, c->stream, a, w);
    hipLaunchKernelGGL(k_h_hyp, dim3((a.n_hyp + TH_BLOCK - 1) / TH_BLOCK, a.n_pairs), dim3(TH_BLOCK), 0, c->stream, a, w);
    hipLaunchKernelGGL(k_h_score, dim3((a.n_hyp + 63) / 64, a.n_pairs), dim3(64 * TH_PARTS), 0, c->stream, a, w);
    hipLaunchKernelGGL(k_h_refit, dim3(a.n_pairs), dim3(THF_BLOCK), 0, c->stream, a, w);
    hipLaunchKernelGGL(k_h_check_rt, dim3((a.m_fixed + TH_BLOCK - 1) / TH_BLOCK, 8, a.n_pairs), dim3(TH_BLOCK), 0, c->stream, a, w);
    hipLaunchKernelGGL(k_h_finish, dim3(a.n_pairs), dim3(THF_BLOCK), 0, c->stream, a, w);
    HIPCHK(c, hipGetLastError());
    return MO_OK;
}
