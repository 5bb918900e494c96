// map_store.h -- the device-resident map (mo_map) shared by map_kernels.hip (growth, cull, relocalization), map_track.hip
// (tracking against the map) and map_ba.hip (bundle adjustment): the stores, their scratch and the helpers that grow them.  Private to the library.
#pragma once
#include <algorithm>
#include <vector>

#include "common.h"

// status block (device, int32): live counts of the call in flight
enum { ST_NPTS = 0, ST_NOBS, ST_NNEW, ST_ERR, ST_KEPT, ST_KOBS, ST_NLIST, ST_NWORDS = 8 };

struct MapPts {
    float* xyz = nullptr; uint8_t* col = nullptr; int32_t* id = nullptr; int32_t* dkf = nullptr; int32_t* drow = nullptr;
    int32_t* off = nullptr;                           // [pcap + 1]
    int32_t* okf = nullptr; int32_t* okp = nullptr;   // [ocap]
    size_t pcap = 0, ocap = 0;
};

struct RelocRes;  // per-call results of mo_map_relocalize (map_kernels.hip)
struct TrackBufs; // scratch of mo_map_track (map_track.hip)
struct BaBufs;    // scratch of mo_map_bundle_adjust and mo_map_add_observations (map_ba.hip)

struct mo_map {
    mo_ctx* c = nullptr;
    // keyframe store
    int row = 0, kslots = 0, n_slots = 0;
    mo_keypoint* kkps = nullptr; uint8_t* kdesc = nullptr; int32_t* kcnt = nullptr; double* kP = nullptr;
    std::vector<int32_t> h_kcnt;
    std::vector<int32_t> pos_slot;                    // keyframe position -> slot
    int32_t* d_pos_slot = nullptr; size_t pos_slot_bytes = 0;
    // the previous and the new keyframe image (colours of the grown points)
    uint8_t* img[2] = {nullptr, nullptr}; size_t img_bytes[2] = {0, 0}; int img_w[2] = {0, 0}, img_h[2] = {0, 0}, img_ch[2] = {0, 0};
    int img_cur = 0;
    // map store
    MapPts P[2]; int cur = 0;
    int64_t n_pts = 0, n_obs = 0;
    int64_t id_bound = 0;                             // every id < id_bound (the first-point table of the keyframe counts)
    // per-keyframe lists of the last cull
    // two sets: a chain writes the set lcur ^ 1, a successful call flips lcur (after MO_ERR_INDEX the previous lists stay readable)
    int32_t* loff[2] = {nullptr, nullptr}; size_t loff_bytes[2] = {0, 0}; int32_t* lids[2] = {nullptr, nullptr}; size_t lids_bytes[2] = {0, 0};
    int lcur = 0, list_rows = 0;
    int32_t* kf_red = nullptr; size_t kf_red_bytes = 0;
    // scratch
    int32_t* st = nullptr;                            // [ST_NWORDS] status
    int32_t* keep = nullptr; int32_t* kobs = nullptr; int32_t* rank = nullptr; int32_t* obase = nullptr;
    size_t keep_bytes = 0, kobs_bytes = 0, rank_bytes = 0, obase_bytes = 0;
    int32_t* part = nullptr; size_t part_bytes = 0;
    int32_t* ent_id = nullptr; size_t ent_bytes = 0;  // id of the point of every observation entry (compacted map)
    int32_t* hist = nullptr; int32_t* hbase = nullptr; size_t hist_bytes = 0, hbase_bytes = 0;
    int32_t* first = nullptr; size_t first_bytes = 0;
    // growth step
    int32_t* midx = nullptr; int32_t* mdist = nullptr; uint8_t* mpass = nullptr; uint8_t* inl = nullptr; float* gpts = nullptr;
    double* F = nullptr; int32_t* gnp = nullptr;
    size_t midx_bytes = 0, mdist_bytes = 0, mpass_bytes = 0, inl_bytes = 0, gpts_bytes = 0, F_bytes = 0, gnp_bytes = 0;
    int32_t* h_stat = nullptr;                        // pinned [ST_NWORDS]
    // relocalization (mo_map_relocalize), grown with the map
    int32_t* rl_tab = nullptr; size_t rl_tab_bytes = 0;                        // point_of [slot][row]
    int32_t* rl_qf = nullptr; size_t rl_qf_bytes = 0;                          // [n_kf] query frame of every pair: the spare slot
    int32_t* rl_midx = nullptr; int32_t* rl_mdist = nullptr; uint8_t* rl_mpass = nullptr;  // [n_kf][row] matcher outputs
    size_t rl_midx_bytes = 0, rl_mdist_bytes = 0, rl_mpass_bytes = 0;
    int32_t* rl_score = nullptr; size_t rl_score_bytes = 0;                    // [n_kf] |C_k|
    int32_t* rl_cq = nullptr; int32_t* rl_cp = nullptr; uint8_t* rl_cinl = nullptr;  // [candidate][row] C_k (query, point), final inliers
    size_t rl_cq_bytes = 0, rl_cp_bytes = 0, rl_cinl_bytes = 0;
    int32_t* rl_qpt = nullptr; uint8_t* rl_qinl = nullptr; size_t rl_qpt_bytes = 0, rl_qinl_bytes = 0;  // [row] per query keypoint
    RelocRes* rl_res = nullptr; RelocRes* h_rl = nullptr;                     // device / pinned
    TrackBufs* tk = nullptr;                                                   // tracking (mo_map_track), made on first use
    BaBufs* ba = nullptr;                                                      // bundle adjustment (map_ba.hip), made on first use
};

template <class T> static int reserve(mo_ctx* c, T*& p, size_t& have, size_t need) {
    if (p && need <= have) return MO_OK;
    need = std::max(need, have + have / 2);
    return mo_reserve(c, p, have, need);
}

// grow a buffer keeping its first `keep` bytes (stream-ordered copy)
template <class T> static int regrow(mo_ctx* c, T*& p, size_t old_bytes, size_t new_bytes, size_t keep) {
    T* q = nullptr;
    HIPCHK(c, hipMalloc((void**)&q, std::max(new_bytes, (size_t)16)));
    if (p && keep) HIPCHK(c, hipMemcpyAsync(q, p, keep, hipMemcpyDeviceToDevice, c->stream));
    if (p) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(p)); }
    p = q;
    (void)old_bytes;
    return MO_OK;
}

// ---- block scans (one-block exclusive scan of int32 in thread order, used by the device-wide scan and the compactions)
__device__ __forceinline__ int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// exclusive scan of the block's values (blockDim.x = MAP_SCAN_BLOCK or 1024); returns the block total in *total
__device__ __forceinline__ int block_excl_scan(int v, int* lds_waves, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int inc = wave_incl_scan(v);
    if (lane == 63) lds_waves[wv] = inc;
    __syncthreads();
    if (threadIdx.x < 64) {
        const int s = threadIdx.x < nw ? lds_waves[threadIdx.x] : 0;
        const int si = wave_incl_scan(s);
        if (threadIdx.x < nw) lds_waves[16 + threadIdx.x] = si - s;
        if (threadIdx.x == nw - 1) lds_waves[32] = si;
    }
    __syncthreads();
    const int r = lds_waves[16 + wv] + inc - v;
    *total = lds_waves[32];
    __syncthreads();
    return r;
}

// map_kernels.hip: the keyframe store grown to `rows` per slot and `slots` slots (+ the spare slot a query frame is staged in); the
// position -> slot table on the device
int kf_reserve(mo_map* m, int rows, int slots);
int upload_pos_slot(mo_map* m);
// map_kernels.hip: the device-wide exclusive scan of int32 (total into *d_total) and the growth of one copy of the map store
int map_scan_excl(mo_map* m, const int32_t* in, int32_t* out, int n, int32_t* d_total);
int map_pts_reserve(mo_map* m, int which, size_t pcap, size_t ocap, bool keep);
// map_track.hip: frees the tracking scratch (mo_map_destroy)
void map_track_free(mo_map* m);
// map_ba.hip: frees the bundle-adjustment scratch (mo_map_destroy)
void map_ba_free(mo_map* m);
