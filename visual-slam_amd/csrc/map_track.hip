// map_track.hip -- tracking a frame against the device map (mo_map_track in include/vslam_amd.h): ORB-SLAM2's search by projection and
// its monocular pose-only PoseOptimization, on the map as it stands.  Read-only on the map; the frame is staged in the spare keyframe
// slot (map_stage_frame), like mo_map_relocalize's.
//
// The tracker's types, the frame view and the candidate tail of the searches are map_track.h's; the single-workgroup stages below
// (k_trk_init, k_trk_grid, k_trk_compact, k_trk_refine) take blockIdx.x as the frame, and this file launches them with one workgroup over
// the spare slot's rows (stride m->row, count kcnt[spare]); mo_map_track_batch (map_track_batch.hip) launches them over its frames.
//
// Chain (one synchronisation, the copy-out; the retry and the early exits are flags in TrackRes that every later kernel reads first):
//   k_trk_init      result block, per-keypoint keys and outputs
//   k_trk_rep       one thread per point: local-map membership, representative descriptor ([point][32]) and its octave
//                   (mo_map_track_covisible: k_covis and k_covis_select of map_covis.hip run in front of it and give it the local keyframes)
//   k_trk_grid      one block per grid: stable counting sort of the frame keypoints into 64 x 48 cells
//   per pass, per attempt (the second attempt runs only after a pass with too few matches):
//     k_trk_search  one thread per local point: projection, then trk_claim: window over the cells, 256-bit Hamming distances, best /
//                   second, the accepted match claims its keypoint by a 64-bit atomicMin of (dist << 32) | point
//     k_trk_compact one block per frame: the winners in keypoint order (block scans), per-keypoint outputs, the retry / end decision
//   k_trk_refine    one block of 256 per frame: 4 rounds of Gauss-Newton (Huber in rounds 0 - 2), f64 partial sums per thread, fixed-order
//                   wave and workgroup reductions, one Cholesky solve per step
// mo_map_track_frustum: the same chain with k_view_centres and k_view_points (map_view_geom.hip, through view_enqueue) behind k_trk_rep,
// k_trk_search_frustum in place of k_trk_search, and k_trk_level (the predicted level per matched keypoint) behind the last pass.
// Every device result is the same on every run: integer atomics only (sums and minima commute), fixed-order f64 reductions.
// -ffp-contract=off (Makefile): the projection rounds like tests/track_restatement.py's elementwise numpy.
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"
#include "map_store.h"
#include "map_track.h"    // the tracker's types, frame view and candidate tail; map_search.h: the grid geometry, the projected-window search
#include "ba.h"         // ba_info (pnp.h comes with it)

#define TK_GRID_BLOCK 1024
#define TK_CELLS_PER_THREAD (TK_CELLS / TK_GRID_BLOCK)
#define TK_REFINE_BLOCK 256
static_assert(TK_CELLS % TK_GRID_BLOCK == 0, "cells per thread");

struct TrackBufs : MapFeature {
    DevBuf<uint8_t> rep;                  // [point][32] representative descriptors
    DevBuf<int32_t> oct;                  // [point] ref_octave (TK_NOT_LOCAL: not in the local map)
    DevBuf<int32_t> cell;                 // [TK_CELLS + 1] first sorted entry of every cell
    DevBuf<int32_t> sorted;               // [row] keypoint indices by cell, index order inside a cell
    DevBuf<unsigned long long> key;       // [row] (dist << 32) | point of the claim on each keypoint
    DevBuf<TrkMatch> match;               // [row]
    DevBuf<uint8_t> minl;                 // [row] inlier flag of every match
    DevBuf<int32_t> qpt, qdist; DevBuf<uint8_t> qinl;   // [row] per frame keypoint
    ResBlock<TrackRes> res;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) { f(rep); f(oct); f(cell); f(sorted); f(key); f(match); f(minl); f(qpt); f(qdist); f(qinl); f(res); }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// one workgroup per frame: its result block, keys and per-keypoint outputs; frame 0 zeroes the local-map counter
__global__ __launch_bounds__(256) void k_trk_init(TrkFrames fr, TrkPose one, int32_t* __restrict__ n_local) {
    const int f = blockIdx.x, n = fr.n(f);
    const size_t at = fr.at(f);
    unsigned long long* __restrict__ key = fr.key + at;
    int32_t* __restrict__ qpt = fr.qpt + at;
    int32_t* __restrict__ qdist = fr.qdist + at;
    uint8_t* __restrict__ qinl = fr.qinl + at;
    for (int q = threadIdx.x; q < n; q += 256) { key[q] = TK_NONE; qpt[q] = -1; qdist[q] = -1; qinl[q] = 0; }
    if (threadIdx.x == 0) {
        TrackRes* res = fr.res + f;   // (one frame: *n_local is its n_local)
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int i = 0; i < 12; i++) res->pose[i] = fr.pose0 ? fr.pose0[(size_t)f * 12 + i] : one.v[i];
        for (int k = 0; k < TK_MAX_PASS; k++) {
            for (int i = 0; i < 12; i++) res->pass_pose[k][i] = nan;
            res->pass_radius[k] = 0.0;
            res->pass_cand[k] = 0; res->pass_matches[k] = 0; res->pass_inliers[k] = 0;
        }
        res->n_local = 0; res->n_run = 0; res->n_done = 0; res->ended = n == 0; res->retry = 0; res->cand = 0; res->n_match = 0;
        if (f == 0) *n_local = 0;
    }
}

// one thread per point: its valid observations (map_obs); local when one of them is at a local keyframe: a position >= lo_pos, or with
// MASK a position whose byte of lmask is not zero.  The
// representative is ComputeDistinctiveDescriptors' choice: the observation with the smallest median distance to all of them, ties to
// the earlier.  Each median is found by bisection on the distance value (count of distances <= v), only below the best so far.
template <bool MASK> __global__ __launch_bounds__(256) void k_trk_rep(MapView v, const mo_keypoint* __restrict__ kkps, const uint8_t* __restrict__ kdesc,
                                                                      int lo_pos, const uint8_t* __restrict__ lmask, uint8_t* __restrict__ rep,
                                                                      int32_t* __restrict__ oct, int32_t* __restrict__ n_local) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool local = false;
    if (i < v.n_pts) {
        const int o0 = v.src.off[i], o1 = v.src.off[i + 1];
        // the (slot * row + keypoint) entry of observation o, -1 when it names nothing
        auto entry = [&](int o, int* pos) -> long long {
            int s, kp;
            return map_obs(v, o, pos, &s, &kp) ? -1 : (long long)s * v.row + kp;
        };
        int nv = 0, pos = 0;
        long long best = -1;
        for (int o = o0; o < o1; o++) {
            const long long e = entry(o, &pos);
            if (e < 0) continue;
            nv++;
            local |= MASK ? lmask[pos] != 0 : pos >= lo_pos;
            if (best < 0) best = e;
        }
        if (local && nv > 2) {   // (n <= 2: every median is the distance to itself, 0: the first observation)
            const int r = (nv - 1) / 2;
            int best_med = 257;
            for (int o = o0; o < o1; o++) {
                const long long ej = entry(o, &pos);
                if (ej < 0) continue;
                const uint8_t* dj = kdesc + ej * 32;
                auto count_le = [&](int d) {
                    int cnt = 0;
                    for (int l = o0; l < o1; l++) {
                        const long long el = entry(l, &pos);
                        if (el >= 0) cnt += trk_ham(dj, kdesc + el * 32) <= d;
                    }
                    return cnt;
                };
                int hi = best_med - 1;
                if (count_le(hi) <= r) continue;   // median >= the best so far: the earlier observation keeps it
                int lo = 0;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (count_le(mid) > r) hi = mid; else lo = mid + 1;
                }
                best_med = lo;
                best = ej;
            }
        }
        if (local) {
            const uint4* d = (const uint4*)(kdesc + best * 32);
            uint4* o = (uint4*)(rep + (size_t)i * 32);
            o[0] = d[0]; o[1] = d[1];
            oct[i] = kkps[best].octave;
        } else {
            oct[i] = TK_NOT_LOCAL;
        }
    }
    wave_count_add(local, n_local);
}

// one block per grid: histogram of the cells (LDS), exclusive scan, scatter by LDS cursors, then every cell's run sorted by keypoint index (the
// cursors' order is arrival order; the sort makes the layout the stable counting sort's).  Block b sorts the row (slots ? slots[b] :
// slot0 + b) of kkps [.][row] - keyframe slots of the store, the staged frame in its spare slot, the frames of a batch
__global__ __launch_bounds__(TK_GRID_BLOCK) void k_trk_grid(const mo_keypoint* __restrict__ kkps, int row, const int32_t* __restrict__ kcnt,
                                                            const int32_t* __restrict__ slots, int slot0, int w, int h, int32_t* __restrict__ cell,
                                                            int32_t* __restrict__ sorted) {
    const int slot = slots ? slots[blockIdx.x] : slot0 + (int)blockIdx.x;
    const mo_keypoint* __restrict__ fk = kkps + (size_t)slot * row;
    const int n = min(kcnt[slot], row);
    cell += (size_t)blockIdx.x * (TK_CELLS + 1);
    sorted += (size_t)blockIdx.x * row;
    __shared__ int cur[TK_CELLS];
    __shared__ int lw[40];
    const int tid = threadIdx.x;
    for (int c = tid; c < TK_CELLS; c += TK_GRID_BLOCK) cur[c] = 0;
    __syncthreads();
    for (int q = tid; q < n; q += TK_GRID_BLOCK) atomicAdd(cur + trk_cy(fk[q].y, h) * TK_GX + trk_cx(fk[q].x, w), 1);
    __syncthreads();
    int v[TK_CELLS_PER_THREAD], s = 0;
    for (int j = 0; j < TK_CELLS_PER_THREAD; j++) { v[j] = cur[tid * TK_CELLS_PER_THREAD + j]; s += v[j]; }
    int tot;
    int base = block_excl_scan(s, lw, &tot);
    for (int j = 0; j < TK_CELLS_PER_THREAD; j++) {
        cur[tid * TK_CELLS_PER_THREAD + j] = base;
        cell[tid * TK_CELLS_PER_THREAD + j] = base;
        base += v[j];
    }
    if (tid == 0) cell[TK_CELLS] = tot;
    __syncthreads();
    for (int q = tid; q < n; q += TK_GRID_BLOCK) sorted[atomicAdd(cur + trk_cy(fk[q].y, h) * TK_GX + trk_cx(fk[q].x, w), 1)] = q;
    __syncthreads();
    for (int j = 0; j < TK_CELLS_PER_THREAD; j++) {
        const int c = tid * TK_CELLS_PER_THREAD + j;
        sort_run(sorted + cell[c], cur[c] - cell[c]);
    }
}

// What the frustum mode adds to a tracking call (mo_map_track_frustum): its scratch, a feature of its own, so that the plain call's
// TrackBufs is what it was.
struct FrustumRes {
    int32_t in_image[TK_MAX_PASS][2];     // projections inside the image, per pass and attempt
    int32_t attempt[TK_MAX_PASS];         // the last attempt of each pass that searched
};
struct TrackFrustumBufs : MapFeature {
    DevBuf<int32_t> lvl;                  // [point] predicted level of the candidates of the last attempt searched
    DevBuf<int32_t> qlvl;                 // [row] per frame keypoint: the level of its point
    ResBlock<FrustumRes> fres;
    // all of it is scratch: every call's chain writes what it reads
    template <class F> void each_scratch(F f) { f(lvl); f(qlvl); f(fres); }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};
// ... and what its search kernel receives on top of the plain one's arguments (by value)
struct TrkFrustum {
    FrustumPrm f;
    const ViewRec* rec;
    int32_t* lvl;
    FrustumRes* fres;
};

// one thread per point: candidates of the pass (projection in the image), the best and second distance over the window, the claim
__global__ __launch_bounds__(256) void k_trk_search(TrackPrm prm, int pass, int attempt, const float* __restrict__ xyz, int n_pts,
                                                    const uint8_t* __restrict__ rep, const int32_t* __restrict__ oct,
                                                    const mo_keypoint* __restrict__ fk, const uint8_t* __restrict__ fdesc,
                                                    const int32_t* __restrict__ cell, const int32_t* __restrict__ sorted,
                                                    unsigned long long* __restrict__ key, TrackRes* __restrict__ res) {
    if (!trk_active(res, attempt)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int ro = i < n_pts ? oct[i] : TK_NOT_LOCAL;
    bool cand = false;
    double uu = 0.0, vv = 0.0;
    if (ro != TK_NOT_LOCAL) {
        double R[9], t[3], P[12];
        pose_split(res->pose, R, t);
        pnp_projection(prm.K, R, t, P);
        cand = trk_project(P, xyz[(size_t)i * 3], xyz[(size_t)i * 3 + 1], xyz[(size_t)i * 3 + 2], prm.w, prm.h, &uu, &vv);
    }
    wave_count_add(cand, &res->cand);
    if (!cand) return;
    const double r = (attempt ? 2.0 * prm.radius[pass] : prm.radius[pass]) * trk_scale(prm.sf, ro);
    trk_claim(prm, i, rep, fdesc, key, [&](auto visit) { trk_window(uu, vv, r, ro, prm.w, prm.h, cell, sorted, fk, visit); });
}

// k_trk_search under the frustum (mo_map_track_frustum): a candidate also lies in its point's frustum seen from the pass camera, and is
// searched at its predicted level L with the octave gate [L - 1, L].  A kernel of its own for its candidate test and counters; the
// tail is the plain search's (trk_claim).
__global__ __launch_bounds__(256) void k_trk_search_frustum(TrackPrm prm, TrkFrustum fr, int pass, int attempt, const float* __restrict__ xyz, int n_pts,
                                                            const uint8_t* __restrict__ rep, const int32_t* __restrict__ oct,
                                                            const mo_keypoint* __restrict__ fk, const uint8_t* __restrict__ fdesc,
                                                            const int32_t* __restrict__ cell, const int32_t* __restrict__ sorted,
                                                            unsigned long long* __restrict__ key, TrackRes* __restrict__ res) {
    if (!trk_active(res, attempt)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int ro = i < n_pts ? oct[i] : TK_NOT_LOCAL;
    bool in_image = false, cand = false;
    double uu = 0.0, vv = 0.0;
    int lv = 0;
    if (ro != TK_NOT_LOCAL) {
        double R[9], t[3], P[12], C[3];
        pose_split(res->pose, R, t);
        pnp_projection(prm.K, R, t, P);
        const double X = xyz[(size_t)i * 3], Y = xyz[(size_t)i * 3 + 1], Z = xyz[(size_t)i * 3 + 2];
        in_image = trk_project(P, X, Y, Z, prm.w, prm.h, &uu, &vv);
        if (in_image) {
            trk_centre(R, t, C);
            cand = trk_frustum(fr.f, fr.rec[i], C, X, Y, Z, &lv);
            if (cand) fr.lvl[i] = lv;
        }
    }
    if (i == 0) fr.fres->attempt[pass] = attempt;
    wave_count_add(in_image, &fr.fres->in_image[pass][attempt]);
    wave_count_add(cand, &res->cand);
    if (!cand) return;
    const double r = (attempt ? 2.0 * prm.radius[pass] : prm.radius[pass]) * trk_scale(prm.sf, lv);
    trk_claim(prm, i, rep, fdesc, key, [&](auto visit) { trk_window_oct(uu, vv, r, lv - 1, lv, prm.w, prm.h, cell, sorted, fk, visit); });
}

// one thread per frame keypoint, behind the last pass: the predicted level of the point it was matched to (the level and the match are
// of the same attempt: every search that ran was followed by its compaction)
__global__ __launch_bounds__(256) void k_trk_level(int n, const int32_t* __restrict__ qpt, const int32_t* __restrict__ lvl, int32_t* __restrict__ qlvl) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const int p = qpt[q];
    qlvl[q] = p >= 0 ? lvl[p] : -1;
}

// one workgroup per frame: the claimed keypoints in keypoint order -> the match list and the per-keypoint outputs; keys reset for the
// next attempt; the pass's counts and the retry / end decision
__global__ __launch_bounds__(1024) void k_trk_compact(TrackPrm prm, TrkFrames fr, int pass, int attempt, const float* __restrict__ xyz) {
    __shared__ int lw[40];
    __shared__ int active;
    const int f = blockIdx.x;
    TrackRes* __restrict__ res = fr.res + f;
    if (threadIdx.x == 0) active = trk_active(res, attempt);
    __syncthreads();
    if (!active) return;
    const size_t at = fr.at(f);
    const mo_keypoint* __restrict__ fk = fr.fk + at;
    unsigned long long* __restrict__ key = fr.key + at;
    TrkMatch* __restrict__ match = fr.match + at;
    int32_t* __restrict__ qpt = fr.qpt + at;
    int32_t* __restrict__ qdist = fr.qdist + at;
    uint8_t* __restrict__ qinl = fr.qinl + at;
    const int n = fr.n(f);
    int added = 0;
    for (int b = 0; b < n; b += 1024) {
        const int q = b + threadIdx.x;
        const unsigned long long k = q < n ? key[q] : TK_NONE;
        const bool has = k != TK_NONE;
        int tot;
        const int r = block_excl_scan(has ? 1 : 0, lw, &tot);
        if (q < n) {
            const int p = has ? (int)(k & 0xffffffffu) : -1;
            qpt[q] = p;
            qdist[q] = has ? (int)(k >> 32) : -1;
            qinl[q] = 0;
            key[q] = TK_NONE;
            if (has) {
                const mo_keypoint kp = fk[q];
                TrkMatch mt;
                mt.X = xyz[(size_t)p * 3]; mt.Y = xyz[(size_t)p * 3 + 1]; mt.Z = xyz[(size_t)p * 3 + 2];
                mt.x = kp.x; mt.y = kp.y; mt.octave = kp.octave; mt.q = q; mt.p = p;
                match[added + r] = mt;
            }
        }
        added += tot;
    }
    if (threadIdx.x == 0) {
        res->pass_cand[pass] = res->cand;
        res->cand = 0;
        res->pass_matches[pass] = added;
        res->pass_radius[pass] = attempt ? 2.0 * prm.radius[pass] : prm.radius[pass];
        res->n_match = added;
        res->n_run = pass + 1;
        const int few = added < prm.min_matches;
        if (few && attempt) res->ended = 1;
        res->retry = few && !attempt;
    }
}

// inlier test of one match under (R, t): depth > 0 and information * squared pixel error <= chi2
__device__ __forceinline__ bool trk_inlier(const TrackPrm& prm, const double* R, const double* t, const TrkMatch& mt) {
    const double X = mt.X, Y = mt.Y, Z = mt.Z;
    const double xc = R[0] * X + R[1] * Y + R[2] * Z + t[0];
    const double yc = R[3] * X + R[4] * Y + R[5] * Z + t[1];
    const double zc = R[6] * X + R[7] * Y + R[8] * Z + t[2];
    const double* K = prm.K;
    const double p0 = K[0] * xc + K[1] * yc + K[2] * zc, p1 = K[3] * xc + K[4] * yc + K[5] * zc, p2 = K[6] * xc + K[7] * yc + K[8] * zc;
    const double du = p0 / p2 - (double)mt.x, dv = p1 / p2 - (double)mt.y;
    return zc > 0.0 && ba_info(prm.sf, mt.octave) * (du * du + dv * dv) <= prm.chi2;
}

// one workgroup of 256 per frame: Optimizer::PoseOptimization (monocular, pose only) with Gauss-Newton steps; the pass's outputs.  Per-thread
// partial sums in match order with stride 256, the wave shuffle tree, the four wave sums added left to right by thread 0
__global__ __launch_bounds__(TK_REFINE_BLOCK) void k_trk_refine(TrackPrm prm, TrkFrames fr, int pass) {
    constexpr int NW = TK_REFINE_BLOCK / 64;
    __shared__ double red[NW][27];
    __shared__ double sRt[12];
    __shared__ int flag, cnt[NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    TrackRes* __restrict__ res = fr.res + blockIdx.x;
    if (tid == 0) flag = !res->ended && !res->retry;
    __syncthreads();
    if (!flag) return;
    const size_t at = fr.at(blockIdx.x);
    const TrkMatch* __restrict__ match = fr.match + at;
    uint8_t* __restrict__ minl = fr.minl + at;
    uint8_t* __restrict__ qinl = fr.qinl + at;
    const int m = res->n_match;
    double R[9], t[3];
    pose_split(res->pose, R, t);
    for (int j = tid; j < m; j += TK_REFINE_BLOCK) minl[j] = 1;
    int n_inl = m;
    for (int round = 0; round < 4; round++) {
        const double huber2 = round < 3 ? prm.chi2 : 0.0;
        for (int it = 0; it < 10; it++) {
            double a[27];
            for (int i = 0; i < 27; i++) a[i] = 0.0;
            for (int j = tid; j < m; j += TK_REFINE_BLOCK) {
                if (!minl[j]) continue;
                const TrkMatch mt = match[j];
                pnp_gn_accumulate_w(prm.K, R, t, mt.X, mt.Y, mt.Z, mt.x, mt.y, ba_info(prm.sf, mt.octave), huber2, a, a + 21);
            }
            for (int i = 0; i < 27; i++) a[i] = wave_sum_all(a[i]);
            if (lane == 0)
                for (int i = 0; i < 27; i++) red[wv][i] = a[i];
            __syncthreads();
            if (tid == 0) {
                double s[27];
                for (int i = 0; i < 27; i++) {
                    s[i] = red[0][i];
                    for (int w = 1; w < NW; w++) s[i] += red[w][i];
                }
                double step = 0.0;
                const bool ok = pnp_gn_update(s, s + 21, R, t, &step);
                for (int j = 0; j < 9; j++) sRt[j] = R[j];
                for (int j = 0; j < 3; j++) sRt[9 + j] = t[j];
                flag = !ok || step < 1e-12;
            }
            __syncthreads();
            for (int j = 0; j < 9; j++) R[j] = sRt[j];
            for (int j = 0; j < 3; j++) t[j] = sRt[9 + j];
            const int stop = flag;
            __syncthreads();
            if (stop) break;
        }
        int n = 0;
        for (int j = tid; j < m; j += TK_REFINE_BLOCK) {
            const bool in = trk_inlier(prm, R, t, match[j]);
            minl[j] = in;
            n += in;
        }
        n = wave_sum_int(n);
        if (lane == 0) cnt[wv] = n;
        __syncthreads();
        n_inl = 0;
        for (int w = 0; w < NW; w++) n_inl += cnt[w];
        __syncthreads();
        if (n_inl < 10) break;
    }
    for (int j = tid; j < m; j += TK_REFINE_BLOCK) qinl[match[j].q] = minl[j];
    if (tid == 0) {
        for (int j = 0; j < 3; j++) {
            for (int l = 0; l < 3; l++) res->pose[j * 4 + l] = res->pass_pose[pass][j * 4 + l] = R[j * 3 + l];
            res->pose[j * 4 + 3] = res->pass_pose[pass][j * 4 + 3] = t[j];
        }
        res->pass_inliers[pass] = n_inl;
        res->n_done = pass + 1;
    }
}

int trk_launch_rep(mo_map* m, int lo_pos, uint8_t* rep, int32_t* oct, int32_t* n_local) {
    mo_ctx* c = m->c;
    hipLaunchKernelGGL(k_trk_rep<false>, dim3((unsigned)((m->n_pts + 255) / 256)), dim3(256), 0, c->stream, map_view(m), m->kkps, m->kdesc, lo_pos, nullptr, rep,
                       oct, n_local);
    HIPCHK(c, hipGetLastError());
    return MO_OK;
}

int trk_launch_rep_mask(mo_map* m, const uint8_t* lmask, uint8_t* rep, int32_t* oct, int32_t* n_local) {
    mo_ctx* c = m->c;
    hipLaunchKernelGGL(k_trk_rep<true>, dim3((unsigned)((m->n_pts + 255) / 256)), dim3(256), 0, c->stream, map_view(m), m->kkps, m->kdesc, 0, lmask, rep, oct,
                       n_local);
    HIPCHK(c, hipGetLastError());
    return MO_OK;
}

int trk_launch_grid(mo_ctx* c, const mo_keypoint* kps, int row, const int32_t* cnt, const int32_t* slots, int slot0, int n_grids, int w, int h,
                    int32_t* cell, int32_t* sorted) {
    hipLaunchKernelGGL(k_trk_grid, dim3((unsigned)n_grids), dim3(TK_GRID_BLOCK), 0, c->stream, kps, row, cnt, slots, slot0, w, h, cell, sorted);
    HIPCHK(c, hipGetLastError());
    return MO_OK;
}

int trk_launch_init(mo_ctx* c, const TrkFrames& fr, int n_frames, const double* one, int32_t* n_local) {
    TrkPose p{};
    if (one) std::memcpy(p.v, one, sizeof p.v);
    hipLaunchKernelGGL(k_trk_init, dim3((unsigned)n_frames), dim3(256), 0, c->stream, fr, p, n_local);
    HIPCHK(c, hipGetLastError());
    return MO_OK;
}

int trk_launch_compact(mo_ctx* c, const TrackPrm& p, const TrkFrames& fr, int n_frames, int pass, int attempt, const float* xyz) {
    hipLaunchKernelGGL(k_trk_compact, dim3((unsigned)n_frames), dim3(1024), 0, c->stream, p, fr, pass, attempt, xyz);
    HIPCHK(c, hipGetLastError());
    return MO_OK;
}

int trk_launch_refine(mo_ctx* c, const TrackPrm& p, const TrkFrames& fr, int n_frames, int pass) {
    hipLaunchKernelGGL(k_trk_refine, dim3((unsigned)n_frames), dim3(TK_REFINE_BLOCK), 0, c->stream, p, fr, pass);
    HIPCHK(c, hipGetLastError());
    return MO_OK;
}

// ---- the host front (map_track.h) ------------------------------------------------------------------------------------------------------
int track_check(mo_ctx* c, const mo_map_track_params* prm, const double* pose0, size_t n_pose) {
    if (prm->n_pass < 1 || prm->n_pass > TK_MAX_PASS) return mo_fail(c, MO_ERR_ARG, "n_pass must be in 1 .. 4");
    if (prm->w <= 0 || prm->h <= 0) return mo_fail(c, MO_ERR_ARG, "w and h must be > 0");
    if (prm->window < 0) return mo_fail(c, MO_ERR_ARG, "window must be >= 0");
    if (!(prm->scale_factor > 0.0) || !std::isfinite(prm->scale_factor)) return mo_fail(c, MO_ERR_ARG, "scale_factor must be finite and > 0");
    if (!(prm->chi2 >= 0.0) || !std::isfinite(prm->ratio)) return mo_fail(c, MO_ERR_ARG, "chi2 must be >= 0 and ratio finite");
    for (int k = 0; k < prm->n_pass; k++)
        if (!(prm->radius[k] >= 0.0) || !std::isfinite(prm->radius[k])) return mo_fail(c, MO_ERR_ARG, "radius must be finite and >= 0");
    for (size_t i = 0; i < n_pose * 12; i++)
        if (!std::isfinite(pose0[i])) return mo_fail(c, MO_ERR_ARG, "pose0 must be finite");
    return MO_OK;
}

TrackPrm track_prm(const double K[9], const mo_map_track_params* prm) {
    TrackPrm p;
    for (int i = 0; i < 9; i++) p.K[i] = K[i];
    for (int k = 0; k < TK_MAX_PASS; k++) p.radius[k] = k < prm->n_pass ? prm->radius[k] : 0.0;
    p.sf = prm->scale_factor; p.ratio = prm->ratio; p.chi2 = prm->chi2;
    p.w = prm->w; p.h = prm->h; p.max_dist = prm->max_dist; p.min_matches = prm->min_matches;
    return p;
}

void track_defaults(const TrackDst& d, const double* pose0) {
    for (int i = 0; i < 12; i++) d.pose[i] = pose0[i];
    for (int k = 0; k < TK_MAX_PASS; k++) {
        for (int i = 0; i < 12; i++) d.pass_pose[k * 12 + i] = NAN;
        d.pass_radius[k] = 0.0;
        d.pass_cand[k] = 0; d.pass_matches[k] = 0; d.pass_inliers[k] = 0;
    }
    *d.n_pass_run = 0; *d.ok = 0;
}

void track_row_defaults(const TrackDst& d, int n) {
    if (d.point) for (int i = 0; i < n; i++) d.point[i] = -1;
    if (d.dist) for (int i = 0; i < n; i++) d.dist[i] = -1;
    if (d.inlier) std::memset(d.inlier, 0, (size_t)n);
}

int track_result(const TrackDst& d, const TrackRes& r, const mo_map_track_params* prm) {
    for (int i = 0; i < 12; i++) d.pose[i] = r.pose[i];
    for (int k = 0; k < TK_MAX_PASS; k++) {
        for (int i = 0; i < 12; i++) d.pass_pose[k * 12 + i] = r.pass_pose[k][i];
        d.pass_radius[k] = r.pass_radius[k];
        d.pass_cand[k] = r.pass_cand[k]; d.pass_matches[k] = r.pass_matches[k]; d.pass_inliers[k] = r.pass_inliers[k];
    }
    *d.n_pass_run = r.n_run;
    return *d.ok = r.n_done == prm->n_pass && r.pass_inliers[prm->n_pass - 1] >= prm->min_inliers;
}

// mo_map_track (lprm NULL: the local map of the window) and mo_map_track_covisible (the local map of the local keyframes); fprm: the
// frustum mode of either (mo_map_track_frustum), NULL: the plain search and exactly the launches it had
static int track_run(mo_map* m, const mo_frame_ref* f, const double K[9], const double pose0[12], const mo_map_track_params* prm,
                     const mo_map_local_params* lprm, mo_map_local_out* lout, mo_map_track_out* out, const mo_map_frustum_params* fprm = nullptr,
                     mo_map_frustum_out* fout = nullptr) {
    mo_ctx* c = m->c;
    if (!f || !K || !pose0 || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (fprm && (fprm->n_levels < 1 || !std::isfinite(fprm->range_lo) || !std::isfinite(fprm->range_hi) || !std::isfinite(fprm->min_cos)))
        return mo_fail(c, MO_ERR_ARG, "n_levels must be >= 1, range_lo, range_hi and min_cos finite");
    int n, rc;
    if ((rc = track_check(c, prm, pose0, 1))) return rc;
    MAP_ENTER(m);
    HostClock clk(c);
    const TrackDst dst{out->point, out->dist, out->inlier, out->pose, &out->pass_pose[0][0], out->pass_radius, out->pass_cand, out->pass_matches,
                       out->pass_inliers, &out->n_pass_run, &out->ok};
    track_defaults(dst, pose0);
    out->n_local = 0; out->from_token = 0;
    if (fout) for (int k = 0; k < TK_MAX_PASS; k++) fout->pass_in_image[k] = 0;
    mo_keypoint* fk; uint8_t* fdesc;
    auto defaults = [&](int nq) {
        if (fout && fout->level) for (int i = 0; i < nq; i++) fout->level[i] = -1;
        track_row_defaults(dst, nq);
    };
    if ((rc = map_stage_frame(m, f, true, &out->from_token, defaults, &n, &fk, &fdesc))) return rc;
    if (!fk) return lprm ? mo_map_local_keyframes(m, lprm, lout) : MO_OK;   // (nothing to search: not tracked, not an error)
    const int n_kf = (int)m->pos_slot.size(), row = m->row;
    TrackBufs& b = map_feature<TrackBufs>(m);
    const size_t np = (size_t)m->n_pts;
    if ((rc = mo_reserve(c, b.rep, np * 32, b.oct, np, b.cell, TK_CELLS + 1, b.sorted, (size_t)row, b.key, (size_t)row, b.match, (size_t)row,
                         b.minl, (size_t)row, b.qpt, (size_t)row, b.qdist, (size_t)row, b.qinl, (size_t)row, b.res)))
        return rc;
    const TrackPrm p = track_prm(K, prm);
    const TrkFrames one = trk_frames(b, fk, fdesc, m->kcnt + m->kslots, nullptr, row);   // one frame: the spare slot's rows and count
    const int lo_pos = map_window_lo(prm->window, n_kf);
    const MapPts src = m->P[m->cur].view();
    const unsigned pblocks = (unsigned)((m->n_pts + 255) / 256);
    if ((rc = trk_launch_init(c, one, 1, pose0, &b.res.p->n_local))) return rc;
    if (lprm && ((rc = covis_enqueue(m)) || (rc = covis_select_enqueue(m, lprm)))) return rc;
    if ((rc = lprm ? trk_launch_rep_mask(m, covis_mask(m), b.rep, b.oct, &b.res.p->n_local)
                   : trk_launch_rep(m, lo_pos, b.rep, b.oct, &b.res.p->n_local)) ||
        (rc = trk_launch_grid(m, nullptr, m->kslots, 1, prm->w, prm->h, b.cell, b.sorted)))   // (the staged frame: the spare slot)
        return rc;
    mo_stage_mark(c, "track_prep");
    TrackFrustumBufs* fb = nullptr;
    TrkFrustum fr{};
    if (fprm) {   // the view records of the local points behind k_trk_rep
        fb = &map_feature<TrackFrustumBufs>(m);
        const double* centre;
        if ((rc = mo_reserve(c, fb->lvl, np, fb->qlvl, (size_t)row, fb->fres)) || (rc = view_enqueue(m, b.oct, prm->scale_factor, &fr.rec, &centre))) return rc;
        HIPCHK(c, hipMemsetAsync(fb->fres, 0, sizeof(FrustumRes), c->stream));
        fr.f = FrustumPrm{prm->scale_factor, fprm->range_lo, fprm->range_hi, fprm->min_cos, fprm->n_levels};
        fr.lvl = fb->lvl; fr.fres = fb->fres;
        mo_stage_mark(c, "track_view");
    }
    for (int k = 0; k < prm->n_pass; k++) {
        for (int a = 0; a < 2; a++) {
            if (fprm)
                hipLaunchKernelGGL(k_trk_search_frustum, dim3(pblocks), dim3(256), 0, c->stream, p, fr, k, a, src.xyz, (int)m->n_pts, b.rep, b.oct, fk, fdesc,
                                   b.cell, b.sorted, b.key, b.res);
            else
                hipLaunchKernelGGL(k_trk_search, dim3(pblocks), dim3(256), 0, c->stream, p, k, a, src.xyz, (int)m->n_pts, b.rep, b.oct, fk, fdesc, b.cell,
                                   b.sorted, b.key, b.res);
            if ((rc = trk_launch_compact(c, p, one, 1, k, a, src.xyz))) return rc;
        }
        mo_stage_mark(c, "track_search");
        if ((rc = trk_launch_refine(c, p, one, 1, k))) return rc;
        mo_stage_mark(c, "track_refine");
    }
    if (fprm) {
        hipLaunchKernelGGL(k_trk_level, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, b.qpt, fb->lvl, fb->qlvl);
        HIPCHK(c, hipGetLastError());
        if ((rc = fb->fres.download(c))) return rc;
        if (fout->level) HIPCHK(c, hipMemcpyAsync(fout->level, fb->qlvl, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = b.res.download(c))) return rc;
    if (out->point) HIPCHK(c, hipMemcpyAsync(out->point, b.qpt, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (out->dist) HIPCHK(c, hipMemcpyAsync(out->dist, b.qdist, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (out->inlier) HIPCHK(c, hipMemcpyAsync(out->inlier, b.qinl, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (lprm && (rc = covis_copy_enqueue(m, lout))) return rc;
    if ((rc = map_sync(c, clk))) return rc;
    if (lprm) covis_finish(m, lout);
    const TrackRes& r = b.res.host();
    track_result(dst, r, prm);
    if (fprm) {
        const FrustumRes& fres = fb->fres.host();
        for (int k = 0; k < r.n_run; k++) fout->pass_in_image[k] = fres.in_image[k][fres.attempt[k] ? 1 : 0];
    }
    out->n_local = r.n_local;
    return MO_OK;
}

extern "C" int mo_map_track(mo_map* m, const mo_frame_ref* f, const double K[9], const double pose0[12], const mo_map_track_params* prm,
                            mo_map_track_out* out) {
    if (!m) return MO_ERR_ARG;
    return track_run(m, f, K, pose0, prm, nullptr, nullptr, out);
}

extern "C" int mo_map_track_covisible(mo_map* m, const mo_frame_ref* f, const double K[9], const double pose0[12], const mo_map_track_params* prm,
                                      const mo_map_local_params* lprm, mo_map_local_out* lout, mo_map_track_out* out) {
    if (!m) return MO_ERR_ARG;
    int rc;
    if ((rc = covis_check(m, lprm, lout))) return rc;
    lout->n_k1 = 0; lout->n_local_kf = 0; lout->ref = -1;
    return track_run(m, f, K, pose0, prm, lprm, lout, out);
}

extern "C" int mo_map_track_frustum(mo_map* m, const mo_frame_ref* f, const double K[9], const double pose0[12], const mo_map_track_params* prm,
                                    const mo_map_local_params* lprm, const mo_map_frustum_params* fprm, mo_map_track_out* out, mo_map_local_out* lout,
                                    mo_map_frustum_out* fout) {
    if (!m) return MO_ERR_ARG;
    if (!fprm || !fout) return mo_fail(m->c, MO_ERR_ARG, "NULL argument");
    if (lprm) {
        int rc;
        if ((rc = covis_check(m, lprm, lout))) return rc;
        lout->n_k1 = 0; lout->n_local_kf = 0; lout->ref = -1;
    }
    return track_run(m, f, K, pose0, prm, lprm, lprm ? lout : nullptr, out, fprm, fout);
}
