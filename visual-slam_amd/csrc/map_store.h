// map_store.h -- the device-resident map (mo_map) shared by the map sources: map_kernels.hip (stores, device-wide scan, growth, cull),
// map_reloc.hip (relocalization), map_track.hip (tracking), map_ba.hip and map_gba.hip (bundle adjustment; ba_problem.h is what those two share), map_obs.hip (added and erased observations), map_fuse.hip (fusion
// of duplicate points) and map_correct.hip (loop correction; map_merge.h is what those two share), map_sim3.hip and map_confirm.hip (loop alignment and confirmation; sim3_device.h is what those two share), map_grow.hip (new points from neighbour keyframes), map_covis.hip (covisibility, local keyframes), bow.hip (place recognition), map_loop.hip (loop candidates), map_posegraph.hip (essential graph), map_view_geom.hip (point views), map_ptcull.hip (the life of a point: counters, cull, erase), map_io.hip (PLY text), map_snapshot.hip (export / import of the whole state) and map_absorb.hip (one map appended to another).
// Here, in this order:
//   the stores (their owning buffer types DevBuf / PinnedBuf are common.h's);
//   what a feature's host side is made of: MapFeature (its scratch struct's base), ResBlock (a result block, device and pinned copy),
//   mo_reserve (every reservation of a call in one statement), MatchBufs (the matcher's outputs);
//   mo_map and its registry of features, map_feature / map_feature_if / map_feature_drop: where feature scratch lives, is poisoned
//   (map_poison walks the registry) and dies; a new feature edits nothing here;
//   MapView / map_view: the live map as every kernel receives it (by value);
//   MatchView / map_match_point: the matcher's outputs read through a point_of table (restated only by lp_match of map_loop.hip, which says why);
//   map_obs: the one reader of an observation; map_each_obs / map_observes: the walks over a point's valid observations;
//   map_point_copy / map_life_new / map_life_merge: a point's own fields, its life record among them, through every rebuild (the
//   rebuild itself - the scans, the one scatter kernel, the flip of the copies - is map_rebuild.h);
//   map_point_of: the one rule of the point_of tables (k_point_of / map_launch_point_of in map_kernels.hip, k_fuse_prep);
//   wave_sum / wave_sum_all / block_sum / block_max (f64, fixed order), wave_sum_int, wave_count_add, the block scans, sort_run, pose_split;
//   host helpers: map_now, map_window_lo, map_int32_guard, map_sync, map_stage_frame.
// A new reader of the map takes a MapView and these; it does not spell out the stores or restate a rule.
// Private to the library.
#pragma once
#include <algorithm>
#include <climits>
#include <memory>
#include <utility>
#include <vector>

#include "common.h"

// status block (device, int32): live counts of the call in flight
enum { ST_NPTS = 0, ST_NOBS, ST_NNEW, ST_ERR, ST_KEPT, ST_KOBS, ST_NLIST, ST_NWORDS = 8 };

// one copy of the map store as the kernels receive it (by value)
struct MapPts {
    float* xyz = nullptr; uint8_t* col = nullptr; int32_t* id = nullptr; int32_t* dkf = nullptr; int32_t* drow = nullptr;
    int32_t* off = nullptr;                           // [pcap + 1]
    int32_t* okf = nullptr; int32_t* okp = nullptr;   // [ocap]
    int4* life = nullptr;                             // [pcap] {visible, found, born, 0}: map_life_new / map_point_copy / map_life_merge
    size_t pcap = 0, ocap = 0;
};

// ... and its storage (map_pts_reserve grows it)
struct MapPtsStore {
    DevBuf<float> xyz; DevBuf<uint8_t> col; DevBuf<int32_t> id, dkf, drow, off, okf, okp; DevBuf<int4> life;
    size_t pcap = 0, ocap = 0;
    MapPts view() const { return MapPts{xyz, col, id, dkf, drow, off, okf, okp, life, pcap, ocap}; }
};

// A feature's scratch (RelocBufs in map_reloc.hip, TrackBufs, BaProblem in ba_problem.h, BaBufs, ObsEditBufs, FuseBufs, GrowBufs, CovisBufs, BowBufs in bow.hip, LoopBufs): a
// struct in the feature's own file that derives from this, lists its scratch buffers in an each_scratch and implements poison as
// mo_poison_scratch(c, *this) (MergeBufs of map_merge.h, like MatchBufs below, is a member of two such structs and forwards its list).  The map owns it (mo_map::features): made by map_feature<T> on the feature's first call, filled by
// map_poison while a poison byte is set, freed with the map.  Nothing outside its file names it (BaProblem, which the two bundle adjustments share, lives in their header).
struct MapFeature {
    virtual ~MapFeature() = default;
    virtual int poison(mo_ctx* c) = 0;
};

// A call's result block: the device copy (the DevBuf it is: a kernel argument, an entry of the owner's each_scratch) and the pinned copy
// the host reads.  How the device copy is initialised is the feature's business.
template <class T> struct ResBlock : DevBuf<T> {
    PinnedBuf<T> pinned;
    int reserve(mo_ctx* c) { if (int rc = DevBuf<T>::reserve(c, 1)) return rc; return pinned.reserve(c, 1); }
    // the one copy of the block, enqueued on the context stream
    int download(mo_ctx* c) { HIPCHK(c, hipMemcpyAsync(pinned.p, this->p, sizeof(T), hipMemcpyDeviceToHost, c->stream)); return MO_OK; }
    // valid behind map_sync
    T& host() const { return *pinned.p; }
};

// mo_reserve(c, buf, n, buf, n, ..., block, ...): room for n elements in every DevBuf / PinnedBuf / MatchBufs and for every ResBlock
// (which takes no count), in the order written; the first failure is returned and nothing after it is reserved
inline int mo_reserve(mo_ctx*) { return MO_OK; }
template <class T, class... Rest> int mo_reserve(mo_ctx* c, ResBlock<T>& b, Rest&&... rest);
template <class B, class... Rest> int mo_reserve(mo_ctx* c, B& b, size_t n, Rest&&... rest) {
    if (int rc = b.reserve(c, n)) return rc;
    return mo_reserve(c, rest...);
}
template <class T, class... Rest> int mo_reserve(mo_ctx* c, ResBlock<T>& b, Rest&&... rest) {
    if (int rc = b.reserve(c)) return rc;
    return mo_reserve(c, rest...);
}

// The matcher's outputs for `rows` = pairs x stride query rows, in the layout emit_match (match_kernels.hip) defines: idx and dist
// [pair][row][2] (best, second), pass [pair][row].  An owner's each_scratch forwards to this one.
struct MatchBufs {
    DevBuf<int32_t> idx, dist; DevBuf<uint8_t> pass;
    int reserve(mo_ctx* c, size_t rows) { return mo_reserve(c, idx, rows * 2, dist, rows * 2, pass, rows); }
    template <class F> void each_scratch(F f) { f(idx); f(dist); f(pass); }
};

struct mo_map {
    mo_ctx* c = nullptr;
    // keyframe store
    int row = 0, kslots = 0, n_slots = 0;
    DevBuf<mo_keypoint> kkps; DevBuf<uint8_t> kdesc; DevBuf<int32_t> kcnt; DevBuf<double> kP;
    std::vector<int32_t> h_kcnt;
    std::vector<uint32_t> kserial;                    // by slot: bumped whenever mo_map_add_keyframe stores rows there (the keyframe database's staleness test)
    std::vector<int32_t> pos_slot;                    // keyframe position -> slot
    // Ordinals: the k-th keyframe ever stored has ordinal k (include/vslam_amd.h, the life record).  On a map that grew in this process
    // ordinal == slot; a map made by mo_map_import has its slots packed (slot == position then) and keeps the ordinals of the map it
    // was exported from.  kf_stored: keyframes ever stored (map_now); slot_ord: by slot, what a new point's dref_kf names.
    int64_t kf_stored = 0;
    std::vector<int32_t> slot_ord;
    DevBuf<int32_t> d_pos_slot;
    // the previous and the new keyframe image (colours of the grown points)
    DevBuf<uint8_t> img[2]; int img_w[2] = {0, 0}, img_h[2] = {0, 0}, img_ch[2] = {0, 0};
    int img_cur = 0;
    // map store
    MapPtsStore P[2]; int cur = 0;
    int64_t n_pts = 0, n_obs = 0;
    int64_t id_bound = 0;                             // every id < id_bound (the first-point table of the keyframe counts)
    // per-keyframe lists of the last cull
    // two sets: a chain writes the set lcur ^ 1, a successful call flips lcur (after MO_ERR_INDEX the previous lists stay readable)
    DevBuf<int32_t> loff[2], lids[2];
    int lcur = 0, list_rows = 0;
    DevBuf<int32_t> kf_red;
    // scratch
    DevBuf<int32_t> st;                               // [ST_NWORDS] status
    DevBuf<int32_t> keep, kobs, rank, obase;          // [point] every rebuild's decision and its scans (map_rebuild.h); a chain holds one rebuild
    DevBuf<int32_t> part;                             // tile sums of the device-wide scan
    DevBuf<int32_t> ent_id;                           // id of the point of every observation entry (compacted map)
    DevBuf<int32_t> hist, hbase, first;
    // growth step
    MatchBufs match; DevBuf<uint8_t> inl; DevBuf<float> gpts;
    DevBuf<double> F; DevBuf<int32_t> gnp;
    PinnedBuf<int32_t> h_stat;                        // [ST_NWORDS]
    std::vector<std::unique_ptr<MapFeature>> features;   // in the order of their first calls (map_feature)
    // The map's own scratch: what no call reads before its own chain wrote it.  State, and so not listed: the keyframe store (kkps, kdesc,
    // kcnt, kP), d_pos_slot, img, both copies of the map store P, loff / lids, kf_red, and st, whose ST_NPTS / ST_NOBS / ST_NNEW words
    // carry the live counts from one call to the next.  A DevBuf added to this struct is named here or in that sentence.
    template <class Fn> void each_scratch(Fn f) {
        f(keep); f(kobs); f(rank); f(obase); f(part); f(ent_id); f(hist); f(hbase); f(first);
        match.each_scratch(f); f(inl); f(gpts); f(F); f(gnp);
    }
};

// The feature T of a map: null before its first call (map_feature_if), made on first use (map_feature), dropped (map_feature_drop).  A
// lookup by type in a handful of entries, once per call.
template <class T> T* map_feature_if(const mo_map* m) {
    for (const auto& f : m->features)
        if (T* t = dynamic_cast<T*>(f.get())) return t;
    return nullptr;
}
template <class T> T& map_feature(mo_map* m) {
    if (T* t = map_feature_if<T>(m)) return *t;
    m->features.emplace_back(new T());
    return static_cast<T&>(*m->features.back());
}
template <class T> void map_feature_drop(mo_map* m) {
    m->features.erase(std::remove_if(m->features.begin(), m->features.end(), [](const auto& f) { return dynamic_cast<T*>(f.get()) != nullptr; }), m->features.end());
}

// ---- the live map as the kernels receive it (by value): the live copy of the store, the uploaded position table, the keyframe counts
struct MapView {
    MapPts src;
    const int32_t* pos_slot; const int32_t* kcnt;
    int n_kf, row, n_pts;
};
inline MapView map_view(const mo_map* m) {
    return MapView{m->P[m->cur].view(), m->d_pos_slot, m->kcnt, (int)m->pos_slot.size(), m->row, (int)m->n_pts};
}

// ---- the one reader of an observation -----------------------------------------------------------------------------------------------
// Observation o of a map names keyframe position okf[o] and row okp[o] of that keyframe; negative values index from the end (Python
// indexing); anything out of range names nothing.  Returns OBS_OK with the position, the keyframe's slot and the row, else which
// index was out of range (the values are the cull's ST_ERR bits; every other caller skips the observation).
enum { OBS_OK = 0, OBS_BAD_KF = 1, OBS_BAD_KP = 2 };
__device__ __forceinline__ int map_obs(const MapView& v, int o, int* pos, int* slot, int* kp) {
    int kf = v.src.okf[o];
    if (kf < 0) kf += v.n_kf;
    if (kf < 0 || kf >= v.n_kf) return OBS_BAD_KF;
    const int s = v.pos_slot[kf];
    int r = v.src.okp[o];
    const int nk = v.kcnt[s];
    if (r < 0) r += nk;
    if (r < 0 || r >= nk) return OBS_BAD_KP;
    *pos = kf; *slot = s; *kp = r;
    return OBS_OK;
}

// f(o, pos, slot, kp) -> bool for every valid observation of point i, in stored order; true stops the walk
template <class F> __device__ __forceinline__ void map_each_obs(const MapView& v, int i, F f) {
    int pos, slot, kp;
    for (int o = v.src.off[i], o1 = v.src.off[i + 1]; o < o1; o++)
        if (!map_obs(v, o, &pos, &slot, &kp) && f(o, pos, slot, kp)) return;
}

// a valid observation of point i in front of entry o_end (-1: any of them) names position pos
__device__ __forceinline__ bool map_observes(const MapView& v, int i, int pos, int o_end = -1) {
    int p, slot, kp;
    for (int o = v.src.off[i], o1 = o_end < 0 ? v.src.off[i + 1] : o_end; o < o1; o++)
        if (!map_obs(v, o, &p, &slot, &kp) && p == pos) return true;
    return false;
}

// ---- a point's own fields (everything but its observations) from one copy of the store into the other -------------------------------
// Every rebuild moves a point through this, so that a field added to MapPts is added here once.  The life record {visible, found, born, 0}
// (ORB-SLAM2's mnVisible, mnFound, mnFirstKFid; include/vslam_amd.h states its rules) moves as one 16-byte load and store.
__device__ __forceinline__ void map_point_copy(const MapPts& src, int i, const MapPts& dst, int r) {
    for (int k = 0; k < 3; k++) { dst.xyz[(size_t)r * 3 + k] = src.xyz[(size_t)i * 3 + k]; dst.col[(size_t)r * 3 + k] = src.col[(size_t)i * 3 + k]; }
    dst.id[r] = src.id[i]; dst.dkf[r] = src.dkf[i]; dst.drow[r] = src.drow[i];
    dst.life[r] = src.life[i];
}
// the record of a point made while the keyframe of ordinal `born` is the last stored one
__device__ __forceinline__ void map_life_new(const MapPts& dst, int i, int born) { dst.life[i] = make_int4(1, 1, born, 0); }
// ... and of the survivor s of a merged component with the members mem[0 .. nm) (s among them), behind map_point_copy(src, s, dst, r):
// visible and found are the members' sums, formed in int64 and clamped to INT32_MAX; born stays the survivor's (MapPoint::Replace)
__device__ __forceinline__ void map_life_merge(const MapPts& src, int s, const int32_t* __restrict__ mem, int nm, const MapPts& dst, int r) {
    long long vis = 0, fnd = 0;
    for (int a = 0; a < nm; a++) { const int4 l = src.life[mem[a]]; vis += l.x; fnd += l.y; }
    dst.life[r] = make_int4((int)(vis > INT32_MAX ? INT32_MAX : vis), (int)(fnd > INT32_MAX ? INT32_MAX : fnd), src.life[s].z, 0);
}

// point_of: tab [position - lo_pos][row] (preset to INT_MAX) = the lowest point with a valid observation of (position, row), for the
// positions >= lo_pos.  Point i's part of it; returns the number of its valid observations.
__device__ __forceinline__ int map_point_of(const MapView& v, int i, int lo_pos, int32_t* __restrict__ tab) {
    int n = 0;
    map_each_obs(v, i, [&](int, int pos, int, int kp) {
        n++;
        if (pos >= lo_pos) atomicMin(tab + (size_t)(pos - lo_pos) * v.row + kp, i);
        return false;
    });
    return n;
}

// The matcher's outputs (MatchBufs) and a point_of table as a kernel reads them together (by value): pair `match_row` is the matching
// of a query frame against the keyframe at position kf_pos, tab [position][row] covers that position.
struct MatchView {
    const int32_t* idx; const int32_t* dist; const uint8_t* pass; const int32_t* tab;
    int row;
};
// The rule of relocalization and loop matching: the map point a ratio-test survivor's best neighbour belongs to, through point_of.  Query row q of
// pair match_row (-1: the keyframe was not matched); -1: none, else the point and, if asked for, *train_row = the neighbour's row.
// pass is read before idx, idx before tab: a row that fails the ratio test may hold anything in idx.
__device__ __forceinline__ int map_match_point(const MatchView& v, int match_row, int kf_pos, int q, int* train_row = nullptr) {
    if (match_row < 0) return -1;
    const size_t o = (size_t)match_row * v.row + q;
    if (!v.pass[o]) return -1;
    const int t = v.idx[2 * o];
    if (t < 0) return -1;
    const int p = v.tab[(size_t)kf_pos * v.row + t];
    if (p == INT_MAX) return -1;
    if (train_row) *train_row = t;
    return p;
}

// ---- fixed-order f64 wave sum: lane 0's shuffle tree, the same on every run; lane 0 holds the sum, wave_sum_all gives it to every lane
__device__ __forceinline__ double wave_sum(double v) {
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_all(double v) { return __shfl(wave_sum(v), 0, 64); }

// ---- fixed-order f64 sum and maximum of a workgroup (blockDim.x a multiple of 64, lds [blockDim.x / 64]): wave_sum, then the waves in
// order; every thread receives the result
__device__ __forceinline__ double block_sum(double v, double* lds) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    v = wave_sum(v);
    if (lane == 0) lds[wv] = v;
    __syncthreads();
    double s = lds[0];
    for (int w = 1; w < nw; w++) s += lds[w];
    __syncthreads();
    return s;
}
__device__ __forceinline__ double block_max(double v, double* lds) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int d = 32; d; d >>= 1) v = fmax(v, __shfl_down(v, d, 64));
    if (lane == 0) lds[wv] = v;
    __syncthreads();
    double s = lds[0];
    for (int w = 1; w < nw; w++) s = fmax(s, lds[w]);
    __syncthreads();
    return s;
}

// ---- integer wave sum (every lane receives it) and the counter idiom: the wave's set flags added to *counter by lane 0, one atomic
__device__ __forceinline__ int wave_sum_int(int v) {
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ void wave_count_add(bool flag, int32_t* counter) {
    const unsigned long long b = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(counter, (int)__popcll(b));
}

// ---- a short run sorted ascending in place (insertion sort: the runs are a grid cell's keypoints, a component's members)
__device__ __forceinline__ void sort_run(int32_t* run, int n) {
    for (int x = 1; x < n; x++) {
        const int q = run[x];
        int y = x - 1;
        while (y >= 0 && run[y] > q) { run[y + 1] = run[y]; y--; }
        run[y + 1] = q;
    }
}

// ---- [R | t] as 3 x 4 row-major -> R [9], t [3]
__host__ __device__ inline void pose_split(const double* pose12, double* R, double* t) {
    for (int j = 0; j < 3; j++) {
        for (int l = 0; l < 3; l++) R[j * 3 + l] = pose12[j * 4 + l];
        t[j] = pose12[j * 4 + 3];
    }
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

// ---- map_kernels.hip ---------------------------------------------------------------------------------------------------------------
// the keyframe store grown to `rows` per slot and `slots` slots (+ the spare slot a query frame is staged in); the position -> slot
// table on the device
int kf_reserve(mo_map* m, int rows, int slots);
int upload_pos_slot(mo_map* m);
// the device-wide exclusive scan of int32 (total into *d_total) and the growth of one copy of the map store
int map_scan_excl(mo_map* m, const int32_t* in, int32_t* out, int n, int32_t* d_total);
int map_pts_reserve(mo_map* m, int which, size_t pcap, size_t ocap, bool keep);
// point_of of the live map for the positions lo_pos .. lo_pos + n_tab_kf - 1 into tab [n_tab_kf][row]: the INT_MAX fill and k_point_of,
// enqueued (the position table uploaded by the caller)
int map_launch_point_of(mo_map* m, int lo_pos, int n_tab_kf, int32_t* tab);

// ---- host helpers of the calls ---------------------------------------------------------------------------------------------------
// the ordinal of the last stored keyframe (0 on a map without one): the number of keyframes stored so far, whatever was removed since
// (ORB-SLAM2's mnId).  Kept apart from the slot count: an imported map has fewer slots than its history has keyframes.
inline int map_now(const mo_map* m) { return m->kf_stored > 0 ? (int)(m->kf_stored - 1) : 0; }
// the first position of a window of the last `window` keyframes (0: all of them)
inline int map_window_lo(int window, int n_kf) { return window > 0 && window < n_kf ? n_kf - window : 0; }
// points and observations stay below half of int32 (sums of two of them are formed in int)
inline int map_int32_guard(mo_map* m) {
    return m->n_pts > INT32_MAX / 2 || m->n_obs > INT32_MAX / 2 ? mo_fail(m->c, MO_ERR_CAPACITY, "map larger than int32 indexing") : MO_OK;
}
// The first line of every mo_map_* call that touches the device: mo_enter (common.h) and, while a poison byte is set, this map's
// scratch and the scratch of every feature that has run on it filled with the byte (map_kernels.hip)
int map_poison(mo_map* m);
inline int map_enter(mo_map* m) {
    if (int rc = mo_enter(m->c)) return rc;
    return m->c->poison < 0 ? MO_OK : map_poison(m);
}
#define MAP_ENTER(m) do { if (int e__ = map_enter(m)) return e__; } while (0)
// the end of a call's chain: everything is enqueued, the one synchronisation
inline int map_sync(mo_ctx* c, HostClock& clk) {
    clk.enqueued();
    HIPCHK(c, hipStreamSynchronize(c->stream));
    clk.waited();
    return MO_OK;
}

// ---- map_covis.hip -----------------------------------------------------------------------------------------------------------------
// The pieces of mo_map_local_keyframes, for a caller that runs them inside a chain of its own (mo_map_track_covisible): the argument
// rules; the matrix W and the selection enqueued on the context stream (the position table uploaded and the stage set opened by the
// caller, at least one keyframe; stage marks "covis" and "covis_select"); the copies of the result enqueued; after the caller's
// synchronisation, the result read into *out.  covis_mask: [n_kf] on the device, non-zero at a local keyframe, valid behind the selection.
int covis_check(mo_map* m, const mo_map_local_params* prm, const mo_map_local_out* out);
int covis_enqueue(mo_map* m);
int covis_select_enqueue(mo_map* m, const mo_map_local_params* prm);
int covis_copy_enqueue(mo_map* m, mo_map_local_out* out);
void covis_finish(mo_map* m, mo_map_local_out* out);
const uint8_t* covis_mask(const mo_map* m);
// W [n_kf][n_kf] on the device, valid behind covis_enqueue on the context stream (mo_map_loop_candidates reads it)
const int32_t* covis_weights(const mo_map* m);

// ---- map_obs.hip -------------------------------------------------------------------------------------------------------------------
// The entry erase of mo_map_erase_observations for a caller that runs it at the end of a chain of its own (mo_map_bundle_adjust_local):
// cls [n_obs] on the device; the entries of class 2 leave if, when the chain gets there, *run != 0 and *n_inliers >= min_inliers (device
// words).  Enqueued with its scratch reserved (stage mark "obs_erase"); after the caller's synchronisation, finish flips the copies of
// the store, sets m->n_obs and returns the entries that left and the points left with fewer than two.
int obs_erase_enqueue(mo_map* m, const uint8_t* cls, const int32_t* run, const int32_t* n_inliers, int min_inliers);
void obs_erase_finish(mo_map* m, int32_t* n_erased, int32_t* n_under);

// A query frame staged in the spare keyframe slot (mo_map_track, mo_map_relocalize; read-only on the map): the frame looked up,
// *from_token set, defaults(n) run (the caller's per-keypoint output defaults), then - unless there is nothing to search, which leaves
// *fk NULL and returns MO_OK - the int32 bound checked, the store grown (a wider row restrides it), the position table uploaded, the
// call's stage set opened and the rows copied to *fk / *fdesc with kcnt[spare] = n.  The spare slot is m->kslots, its stride m->row.
template <class Defaults> int map_stage_frame(mo_map* m, const mo_frame_ref* f, bool need_points, int32_t* from_token, Defaults defaults, int* n,
                                              mo_keypoint** fk, uint8_t** fdesc) {
    mo_ctx* c = m->c;
    int rs, rc;
    *fk = nullptr; *fdesc = nullptr;
    if ((rc = mo_frame_lookup(c, f, "frame", &rs, n))) return rc;
    *from_token = rs >= 0;
    defaults(*n);
    if (*n == 0 || m->pos_slot.empty() || (need_points && m->n_pts == 0)) return MO_OK;
    if ((rc = map_int32_guard(m)) || (rc = kf_reserve(m, *n, m->n_slots)) || (rc = upload_pos_slot(m))) return rc;
    const size_t at = (size_t)m->kslots * m->row;
    mo_stage_begin(c);
    if ((rc = mo_frame_copy_rows(c, f, rs, *n, m->kkps + at, m->kdesc + at * 32))) return rc;
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)(m->kcnt + m->kslots), *n, 1, c->stream));
    *fk = m->kkps + at; *fdesc = m->kdesc + at * 32;
    return MO_OK;
}
