// map_covis.hip -- covisibility on the device map (mo_map_covisibility, mo_map_local_keyframes in include/vslam_amd.h): the matrix W of
// the points each pair of keyframe positions shares, and ORB-SLAM2's Tracking::UpdateLocalKeyFrames on it: K1 = the keyframes observing
// the seed points, K2 = their best covisible neighbours.  Read-only on the map.  mo_map_track_covisible (map_track.hip) runs the same two
// kernels in front of its own through the covis_* pieces (map_store.h).
//
//   k_covis         threads stream the points (grid stride): the distinct valid positions of a point (map_obs), every pair of them one
//                   add.  Up to CV_LDS_MAX_KF keyframes each workgroup adds into a copy of its own in LDS (the upper triangle, LDS
//                   atomics) and ends with one global atomicAdd per non-zero cell and its mirror; beyond, the adds go to the matrix in
//                   global memory.  Global atomics execute at the memory side, a cell at a time: 10^6 points' pairs on the few cells
//                   next to the diagonal would queue there, the per-workgroup copies turn them into at most blocks x cells adds.
//   k_covis_select  one workgroup: the seeds' votes (global atomics on [n_kf]), ref by a 64-bit maximum of (votes << 32) | position, then
//                   a wavefront per K1 row: n_best rounds of the largest (W << 32) | position below the last one taken.
// Integer atomics only (sums and maxima commute): the same result on every run and on either path of k_covis.
#include <climits>
#include <cstring>

#include "common.h"
#include "map_store.h"

#define CV_BLOCK 256
// W as [n_kf][n_kf] int32 in LDS: 64 KiB at the bound, so that two workgroups stay resident in a CU's 160 KiB
#define CV_LDS_MAX_KF 128
#define CV_LDS_MAX_BYTES (CV_LDS_MAX_KF * CV_LDS_MAX_KF * 4)
// workgroups of k_covis: two per CU of an MI355X; each ends with at most n_kf (n_kf + 1) / 2 cells to add to the global matrix
#define CV_MAX_BLOCKS 512
static_assert(2 * CV_LDS_MAX_BYTES <= 160 * 1024, "two workgroups per CU");
static_assert(CV_LDS_MAX_KF <= 128, "k_covis holds a point's positions in two 64-bit words");

struct CovisRes { int32_t n_k1, n_local_kf, ref; };

struct CovisBufs : MapFeature {
    DevBuf<int32_t> W;                    // [n_kf][n_kf] of the last mo_map_covisibility / mo_map_local_keyframes / mo_map_track_covisible
    DevBuf<int32_t> votes, loc;           // [n_kf] votes of the seeds; 1 = K1, 2 = K2 only
    DevBuf<uint8_t> mask;                 // [n_kf] loc as bytes (the output, and k_trk_rep's local-keyframe predicate)
    DevBuf<int32_t> seeds; PinnedBuf<int32_t> h_seeds;
    ResBlock<CovisRes> res;
    // all of it is scratch, W included: every reader (the three calls above, mo_map_loop_candidates) runs covis_enqueue in its own chain
    // first (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) { f(W); f(votes); f(loc); f(mask); f(seeds); f(res); }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

__device__ __forceinline__ int cv_pop(unsigned long long& lo, unsigned long long& hi) {   // the lowest position of the set, removed
    if (lo) { const int p = __ffsll(lo) - 1; lo &= lo - 1; return p; }
    const int p = __ffsll(hi) - 1; hi &= hi - 1;
    return 64 + p;
}

template <bool LDS> __global__ __launch_bounds__(CV_BLOCK) void k_covis(MapView v, int32_t* __restrict__ W) {
    extern __shared__ int32_t sW[];   // [n_kf][n_kf], cells p <= q used
    const int n_kf = v.n_kf, cells = n_kf * n_kf;
    if (LDS) {
        for (int c = threadIdx.x; c < cells; c += CV_BLOCK) sW[c] = 0;
        __syncthreads();
    }
    for (int i = blockIdx.x * CV_BLOCK + threadIdx.x; i < v.n_pts; i += gridDim.x * CV_BLOCK) {
        if (LDS) {
            unsigned long long lo = 0, hi = 0;   // the point's positions as a set: duplicates fold
            map_each_obs(v, i, [&](int, int pa, int, int) {
                if (pa < 64) lo |= 1ull << pa; else hi |= 1ull << (pa - 64);
                return false;
            });
            while (lo | hi) {
                const int p = cv_pop(lo, hi);
                atomicAdd(sW + p * n_kf + p, 1);
                unsigned long long l2 = lo, h2 = hi;
                while (l2 | h2) atomicAdd(sW + p * n_kf + cv_pop(l2, h2), 1);
            }
        } else {
            const int o1 = v.src.off[i + 1];
            map_each_obs(v, i, [&](int a, int pa, int, int) {
                if (map_observes(v, i, pa, a)) return false;
                atomicAdd(W + (size_t)pa * n_kf + pa, 1);
                int pb, s, kp;
                for (int b = a + 1; b < o1; b++) {   // (a first occurrence behind a: another position)
                    if (map_obs(v, b, &pb, &s, &kp) || map_observes(v, i, pb, b)) continue;
                    atomicAdd(W + (size_t)pa * n_kf + pb, 1);
                    atomicAdd(W + (size_t)pb * n_kf + pa, 1);
                }
                return false;
            });
        }
    }
    if (LDS) {
        __syncthreads();
        for (int c = threadIdx.x; c < cells; c += CV_BLOCK) {
            const int p = c / n_kf, q = c - p * n_kf, v = sW[c];
            if (q < p || !v) continue;
            atomicAdd(W + c, v);
            if (q != p) atomicAdd(W + q * n_kf + p, v);
        }
    }
}

__device__ __forceinline__ int cv_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one workgroup.  votes and loc arrive zeroed and are written by atomics and read by cv_load only (the atomics execute behind the L1)
__global__ __launch_bounds__(CV_BLOCK) void k_covis_select(MapView v, const int32_t* __restrict__ W, const int32_t* __restrict__ seeds, int n_seed, int ref_pos, int n_best, int min_w,
                                                           int32_t* __restrict__ votes, int32_t* __restrict__ loc, uint8_t* __restrict__ mask,
                                                           CovisRes* __restrict__ res) {
    __shared__ unsigned long long top;
    __shared__ int cnt[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n_kf = v.n_kf;
    if (tid == 0) { top = 0; cnt[0] = 0; cnt[1] = 0; }
    __syncthreads();
    for (int e = tid; e < n_seed; e += CV_BLOCK) {
        const int i = seeds[e];
        if (i < 0 || i >= v.n_pts) continue;
        map_each_obs(v, i, [&](int o, int p, int, int) {   // (a vote per position: its first valid observation)
            if (!map_observes(v, i, p, o)) atomicAdd(votes + p, 1);
            return false;
        });
    }
    __syncthreads();
    unsigned long long mine = 0;
    for (int k = tid; k < n_kf; k += CV_BLOCK) {
        const int v = cv_load(votes + k);
        if (v <= 0) continue;
        atomicExch(loc + k, 1);
        const unsigned long long key = ((unsigned long long)(unsigned)v << 32) | (unsigned)k;   // most votes, then the later position
        if (key > mine) mine = key;
    }
    if (mine) atomicMax(&top, mine);
    __syncthreads();
    const int ref = top ? (int)(top & 0xffffffffu) : ref_pos;
    if (!top && tid == 0) atomicExch(loc + ref, 1);
    __syncthreads();
    for (int p = wv; p < n_kf; p += CV_BLOCK / 64) {
        if (cv_load(loc + p) != 1) continue;   // (1 is final here: the rounds below only turn a 0 into a 2)
        unsigned long long last = ~0ull;
        for (int t = 0; t < n_best; t++) {
            unsigned long long bk = 0;
            for (int q = lane; q < n_kf; q += 64) {
                const int w = W[(size_t)p * n_kf + q];
                if (q == p || w < min_w) continue;
                const unsigned long long key = ((unsigned long long)(unsigned)w << 32) | (unsigned)q;   // largest weight, then the later position
                if (key < last && key > bk) bk = key;
            }
            for (int d = 32; d; d >>= 1) {
                const unsigned long long o = __shfl_xor(bk, d, 64);
                if (o > bk) bk = o;
            }
            if (!bk) break;
            if (lane == 0) atomicCAS(loc + (int)(bk & 0xffffffffu), 0, 2);
            last = bk;
        }
    }
    __syncthreads();
    int n1 = 0, nl = 0;
    for (int k = tid; k < n_kf; k += CV_BLOCK) {
        const int l = cv_load(loc + k);
        mask[k] = (uint8_t)l;
        n1 += l == 1; nl += l != 0;
    }
    if (n1) atomicAdd(cnt, n1);
    if (nl) atomicAdd(cnt + 1, nl);
    __syncthreads();
    if (tid == 0) { res->n_k1 = cnt[0]; res->n_local_kf = cnt[1]; res->ref = ref; }
}

int covis_check(mo_map* m, const mo_map_local_params* prm, const mo_map_local_out* out) {
    mo_ctx* c = m->c;
    if (!prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (prm->n_best < 0) return mo_fail(c, MO_ERR_ARG, "n_best must be >= 0");
    if (prm->n_seed < 0 || (prm->n_seed > 0 && !prm->seed_points)) return mo_fail(c, MO_ERR_ARG, "n_seed seed points need seed_points");
    const int n_kf = (int)m->pos_slot.size();
    if (n_kf > 0 && (prm->ref_pos < -1 || prm->ref_pos >= n_kf)) return mo_fail(c, MO_ERR_ARG, "ref_pos must be -1 or a keyframe position");
    return MO_OK;
}

int covis_enqueue(mo_map* m) {
    mo_ctx* c = m->c;
    const size_t n_kf = m->pos_slot.size();
    int rc;
    if (n_kf * n_kf > (size_t)INT32_MAX) return mo_fail(c, MO_ERR_CAPACITY, "map larger than int32 indexing");
    if ((rc = map_int32_guard(m))) return rc;
    CovisBufs& b = map_feature<CovisBufs>(m);
    if ((rc = b.W.reserve(c, n_kf * n_kf))) return rc;
    HIPCHK(c, hipMemsetAsync(b.W, 0, n_kf * n_kf * 4, c->stream));
    if (m->n_pts > 0) {
        const unsigned blocks = (unsigned)std::min<int64_t>((m->n_pts + CV_BLOCK - 1) / CV_BLOCK, CV_MAX_BLOCKS);
        if (n_kf <= CV_LDS_MAX_KF) {
            if ((rc = mo_raise_dyn_lds(c, (const void*)k_covis<true>, CV_LDS_MAX_BYTES))) return rc;
            hipLaunchKernelGGL(k_covis<true>, dim3(blocks), dim3(CV_BLOCK), n_kf * n_kf * 4, c->stream, map_view(m), b.W);
        } else {
            hipLaunchKernelGGL(k_covis<false>, dim3(blocks), dim3(CV_BLOCK), 0, c->stream, map_view(m), b.W);
        }
        HIPCHK(c, hipGetLastError());
    }
    mo_stage_mark(c, "covis");
    return MO_OK;
}

int covis_select_enqueue(mo_map* m, const mo_map_local_params* prm) {
    mo_ctx* c = m->c;
    CovisBufs& b = map_feature<CovisBufs>(m);
    const size_t n_kf = m->pos_slot.size(), ns = (size_t)prm->n_seed;
    int rc;
    if ((rc = mo_reserve(c, b.votes, n_kf, b.loc, n_kf, b.mask, n_kf, b.res, b.seeds, std::max(ns, (size_t)1), b.h_seeds, std::max(ns, (size_t)1)))) return rc;
    if (ns) {   // (through a pinned block of the map's own: the caller's array is free again when the call returns, whatever the copy does)
        std::memcpy(b.h_seeds.p, prm->seed_points, ns * 4);
        HIPCHK(c, hipMemcpyAsync(b.seeds, b.h_seeds, ns * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemsetAsync(b.votes, 0, n_kf * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(b.loc, 0, n_kf * 4, c->stream));
    const int ref_pos = prm->ref_pos < 0 ? (int)n_kf - 1 : prm->ref_pos;
    hipLaunchKernelGGL(k_covis_select, dim3(1), dim3(CV_BLOCK), 0, c->stream, map_view(m), b.W, b.seeds, (int)ns, ref_pos, prm->n_best, std::max(prm->min_weight, 1), b.votes, b.loc, b.mask, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "covis_select");
    return MO_OK;
}

int covis_copy_enqueue(mo_map* m, mo_map_local_out* out) {
    mo_ctx* c = m->c;
    CovisBufs& b = map_feature<CovisBufs>(m);
    if (int rc = b.res.download(c)) return rc;
    if (out->local) HIPCHK(c, hipMemcpyAsync(out->local, b.mask, m->pos_slot.size(), hipMemcpyDeviceToHost, c->stream));
    return MO_OK;
}

void covis_finish(mo_map* m, mo_map_local_out* out) {
    const CovisRes& r = map_feature<CovisBufs>(m).res.host();
    out->n_k1 = r.n_k1; out->n_local_kf = r.n_local_kf; out->ref = r.ref;
}

const uint8_t* covis_mask(const mo_map* m) { return map_feature_if<CovisBufs>(m)->mask; }
const int32_t* covis_weights(const mo_map* m) { return map_feature_if<CovisBufs>(m)->W; }

extern "C" int mo_map_covisibility(mo_map* m, int32_t* weights, int32_t* n_kf) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!n_kf) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const size_t n = m->pos_slot.size();
    *n_kf = (int32_t)n;
    if (n == 0) return MO_OK;
    MAP_ENTER(m);
    HostClock clk(c);
    int rc;
    if ((rc = upload_pos_slot(m))) return rc;
    mo_stage_begin(c);
    if ((rc = covis_enqueue(m))) return rc;
    if (weights) HIPCHK(c, hipMemcpyAsync(weights, covis_weights(m), n * n * 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = map_sync(c, clk))) return rc;
    return MO_OK;
}

extern "C" int mo_map_local_keyframes(mo_map* m, const mo_map_local_params* prm, mo_map_local_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    int rc;
    if ((rc = covis_check(m, prm, out))) return rc;
    out->n_k1 = 0; out->n_local_kf = 0; out->ref = -1;
    if (m->pos_slot.empty()) return MO_OK;
    MAP_ENTER(m);
    HostClock clk(c);
    if ((rc = upload_pos_slot(m))) return rc;
    mo_stage_begin(c);
    if ((rc = covis_enqueue(m)) || (rc = covis_select_enqueue(m, prm)) || (rc = covis_copy_enqueue(m, out))) return rc;
    if ((rc = map_sync(c, clk))) return rc;
    covis_finish(m, out);
    return MO_OK;
}
