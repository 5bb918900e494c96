// common.h -- context, plan and helpers shared by the HIP translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <stdint.h>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/vslam_amd.h"
#include "plan_tables.h"  // LevelInfo, Plan, PlanTables and the constants they are sized by

struct FinalKp {  // 8 bytes: survivor of both retainBest passes, level coordinates
    uint16_t x, y;
    float response;
};

struct mo_ctx;
int mo_fail(mo_ctx* c, int code, const std::string& msg);

#define HIPCHK(c, expr)                                                                              \
    do {                                                                                             \
        hipError_t e__ = (expr);                                                                     \
        if (e__ != hipSuccess)                                                                       \
            return mo_fail((c), MO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));     \
    } while (0)

// A device buffer that owns its memory: freed by its destructor, moved but never copied.  Kernels and copies receive the raw pointer
// (the conversion).  Sizes are element counts.  Every hipMalloc / hipFree of the library is in here, and so is the one place a new
// block is filled with the poison byte of mo_dbg_set_poison (realloc_bytes, below mo_ctx).
template <class T> struct DevBuf {
    T* p = nullptr; size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { DevBuf t(std::move(o)); swap(t); return *this; }
    ~DevBuf() { if (p) hipFree(p); }
    operator T*() const { return p; }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(bytes, o.bytes); }
    void reset() { DevBuf().swap(*this); }
    // room for n elements, the contents dropped.  reserve_exact allocates what is asked for (the context's buffers: some are sized
    // for whole 4095 x 4095 frames); reserve grows by half at least (the map's stores, which grow a little with every keyframe).
    int reserve_exact(mo_ctx* c, size_t n) { return n * sizeof(T) <= bytes && p ? MO_OK : realloc_bytes(c, n * sizeof(T)); }
    int reserve(mo_ctx* c, size_t n) { return n * sizeof(T) <= bytes && p ? MO_OK : realloc_bytes(c, std::max(n * sizeof(T), bytes + bytes / 2)); }
    // a new block of n elements that keeps the first `keep`: allocated, copied on the context stream, synchronised, the old one freed
    int regrow(mo_ctx* c, size_t n, size_t keep);
    // a table built on the host: a new block of exactly v.size() elements with the vector copied into it (a failure leaves the old block)
    int upload(mo_ctx* c, const std::vector<T>& v) {
        DevBuf q;
        if (int rc = q.realloc_bytes(c, v.size() * sizeof(T))) return rc;
        HIPCHK(c, hipMemcpy(q.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        swap(q);
        return MO_OK;
    }
private:
    int realloc_bytes(mo_ctx* c, size_t need);
};

// a pinned host block; a larger one replaces it once the context stream has drained (the device may still be reading the old one)
template <class T> struct PinnedBuf {
    T* p = nullptr; size_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept { swap(o); }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { PinnedBuf t(std::move(o)); swap(t); return *this; }
    ~PinnedBuf() { if (p) hipHostFree(p); }
    operator T*() const { return p; }
    void swap(PinnedBuf& o) { std::swap(p, o.p); std::swap(bytes, o.bytes); }
    void reset() { PinnedBuf().swap(*this); }
    int reserve(mo_ctx* c, size_t n, unsigned flags = hipHostMallocDefault);
};

// Everything a plan owns on top of the Plan itself: the launch constants and table offsets (PlanTables), the one block all the
// tables are uploaded in, and the work buffers.  fill_plan (ctx.hip) makes all of it, tables included, before any launcher runs; a
// rebuild drops it whole (c->pb = PlanBufs()): a field added here needs no line anywhere else to be freed or reset.
struct PlanBufs : PlanTables {
    int batch_alloc = 0;           // frames the work buffers below are sized for
    // the batched extraction's resize launches can write the blurred levels too (orb_plan_resize_blur held for every level at
    // the pipeline's margins rb_pyr_margin / rb_margin, the ones the tile records are built for)
    bool rb_ok = false;
    DevBuf<uint32_t> d_tables;     // the block of plan_build_tables and, behind it at word tile_rec, the tile records: the offsets of PlanTables index it
    DevBuf<uint8_t> d_pyr;         // [batch][pyr_stride]
    DevBuf<uint8_t> d_blur;        // [batch][blur_stride]
    DevBuf<uint32_t> d_cand;       // [batch][cand_stride]
    DevBuf<int> d_strip_cnt;       // [batch][strips_per_frame]
    DevBuf<uint64_t> d_scratch;    // [batch][scratch_stride] overflow scratch for the selection replay
    DevBuf<FinalKp> d_fin;         // [batch][fin_stride]
    DevBuf<int> d_fin_cnt;         // [batch][MO_MAX_LEVELS]
    DevBuf<int> d_dtodo;           // k_describe_tiles -> k_describe_tiles_rare: [0] count, then frame * tiles + tile; [1 + n_dtiles * batch * DT_SPLIT_LATENCY]
    DevBuf<uint32_t> d_fs_tab; int fs_tiles = 0, fs_stride = 0, fs_lds = 0; bool fs_ok = false; int fs_geom[10] = {}; const char* fs_why = "";  // k_front_single: per-tile headers + coefficient slices (fs_build)
    // the work buffers no call reads before its own chain wrote them (mo_dbg_set_poison fills them at every entry point); d_tables and
    // d_fs_tab are state: built with the plan, read by every call
    template <class F> void each_scratch(F f) { f(d_pyr); f(d_blur); f(d_cand); f(d_strip_cnt); f(d_scratch); f(d_fin); f(d_fin_cnt); f(d_dtodo); }
};

#define MO_RESULT_SLOTS 4
#define MO_NSTAGES 16
#define MO_TIMING_SLOTS 64

struct TimingSet {
    hipEvent_t ev[MO_NSTAGES + 1] = {};
    const char* names[MO_NSTAGES + 1] = {};
    int n_stages = 0;
};

struct mo_ctx {
    int device = 0;
    int max_w = 0, max_h = 0, max_batch = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    int match_mode = 0;        // VSLAM_AMD_MATCHER: 0 default (XOR + popcount, train tiles through LDS), 1 "mfma" opt-in matrix-core matcher
    int match_slices = 0;      // VSLAM_AMD_MATCHER=valu1|valu2|valu4|valu8: that many train slices in every k_match_lds launch; 0: match_launch_pairs' rule
    int n_cu = 0;              // compute units of the device (what the slicing rule fills)
    int poison = -1;           // mo_dbg_set_poison (tests): >= 0: every new block and, at every entry point, every scratch buffer is filled with that byte
    int64_t poison_bufs = 0, poison_bytes = 0;  // mo_dbg_poison_filled: fills since the last mo_dbg_set_poison
    std::string err;

    // plan (rebuilt when w, h or the ORB parameters change)
    bool plan_valid = false;
    // per-level final-keypoint slots = min(candidates, (4 quota + 256) x fin_slack[L]): a level whose response ties overflow its slot
    // (flag bit 0; the kernel names the level in flag word 1) grows eightfold - that level only - and the plan is rebuilt; the factors
    // start again at 1 whenever the image size or the ORB parameters change
    int fin_slack[MO_MAX_LEVELS] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    bool fin_slack_dirty = false;           // a factor changed since the plan was built
    bool tie_overflow = false;              // the last host extraction raised flag bit 0
    int tie_levels = 0;                     // ... on these levels (bit L)
    mo_orb_params plan_params{};
    Plan plan{};
    PlanBufs pb;                   // what the plan allocated

    // work buffers (device)
    DevBuf<uint8_t> d_in;          // staged host images (any ch)
    DevBuf<uint8_t> d_gray;        // gray level 0 when converted / staged
    DevBuf<int> d_flags;           // [8] error flags raised by kernels: words 0..3 belong to the mo_dev_* calls (they accumulate until
                                   // mo_dev_status), words 4..7 to the host entry points (cleared and checked inside each call)
    int* flags_cur = nullptr;      // the word block the kernels of the current call raise their bits in
    std::vector<const void*> dyn_lds_raised;  // kernels whose max-dynamic-LDS attribute has been raised on this device (mo_raise_dyn_lds)
    // output staging for the host API (batches of frames)
    DevBuf<mo_keypoint> d_kps; DevBuf<uint8_t> d_desc; DevBuf<int> d_counts;
    // Resident results of the last MO_RESULT_SLOTS single-frame extractions of the host API: slot s is "frame s" of these arrays, so the
    // pair stages (matcher, tracking filters, two-view) run on two slots exactly as they run on two frames of a batch, and a Tracker-style
    // caller that hands a frame's token back (mo_pair_frontend) uploads nothing.
    DevBuf<mo_keypoint> d_slot_kps; DevBuf<uint8_t> d_slot_desc; DevBuf<int32_t> d_slot_cnt, d_slot_ids;
    int slot_cap = 0, slot_cur = -1;
    uint64_t slot_token[MO_RESULT_SLOTS] = {}; int slot_n[MO_RESULT_SLOTS] = {}; uint64_t token_next = 1, last_token = 0;
    bool host_timing = false;      // stage events inside the single-call host entry points (mo_set_host_timing; an event between two
                                   // kernels idles the GPU for ~ 4.5 us, five of them were 9 % of a single-frame extraction)
    // matcher staging
    DevBuf<uint8_t> d_mq, d_mt, d_mpass; DevBuf<int32_t> d_midx, d_mdist;
    DevBuf<uint2> d_match_part;     // per-slice keys of a split k_match_lds launch
    DevBuf<uint8_t> d_tv;           // two-view work buffers (carved by twoview_launch)
    DevBuf<uint8_t> d_hf;           // homography branch of the two-view stage (carved by twoview_h_launch)
    DevBuf<float> d_stream_pts;     // mo_stream: map-point scratch of chunks whose caller does not want them
    DevBuf<uint32_t> d_track_keys;  // k_track_select: key arrays of frames too large for LDS
    DevBuf<uint8_t> d_tmp;          // generic temp (carved with Layout)

    // RCCL communicator of the sharded batched mode (comm.hip); null until mo_comm_init
    void* comm = nullptr; int comm_rank = 0, comm_world = 1;
    DevBuf<int32_t> d_comm_cnt;     // this rank's row count for mo_gather_map_points' all-gather

    double host_us[4] = {0, 0, 0, 0};  // mo_host_times: enqueue / wait / unpack / total of the last single-call host entry point
    PinnedBuf<uint8_t> h_stage;        // pinned (mapped, coherent) host staging of small host-API results
    DevBuf<int32_t> d_pair_frames; int pair_frames_n = 0;  // mo_dev_frontend_batch: qf[i] = i, tf[i] = i + 1 ([2][pair_frames_n])
    // stage timing: a ring of event sets, one per mo_* call (mo_stage_begin advances it), so that a caller can enqueue many calls
    // back to back and read the per-stage times of the last MO_TIMING_SLOTS of them after ONE synchronisation (mo_stage_times_back)
    TimingSet tsets[MO_TIMING_SLOTS];
    int tcur = 0;
    bool timing = true;
    // The context's scratch: what no call reads before its own chain wrote it.  State, and so not listed: d_flags (words 0..3 accumulate
    // until mo_dev_status), d_slot_* (resident results), d_pair_frames (written once per size), d_comm_cnt.  A DevBuf added to this
    // struct is named here or in that sentence.
    template <class F> void each_scratch(F f) {
        f(d_in); f(d_gray); f(d_kps); f(d_desc); f(d_counts); f(d_mq); f(d_mt); f(d_mpass); f(d_midx); f(d_mdist); f(d_match_part); f(d_tv); f(d_hf);
        f(d_stream_pts); f(d_track_keys); f(d_tmp);
    }
};

// (the pointer and its size are dropped before the free: a failure leaves nothing that passes the size check)
template <class T> int DevBuf<T>::realloc_bytes(mo_ctx* c, size_t need) {
    T* old = p;
    p = nullptr; bytes = 0;
    if (old) HIPCHK(c, hipFree(old));
    need = std::max(need, (size_t)16);
    HIPCHK(c, hipMalloc((void**)&p, need));
    bytes = need;
    if (c->poison >= 0) {  // mo_dbg_set_poison: no owner may rely on what a fresh block holds (drained: its first use may be on any stream)
        HIPCHK(c, hipMemsetAsync(p, c->poison, need, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->poison_bufs++; c->poison_bytes += (int64_t)need;
    }
    return MO_OK;
}

// mo_dbg_set_poison: one buffer filled over its whole capacity on the context stream; every buffer of a struct's each_scratch list
template <class T> int mo_poison_buf(mo_ctx* c, DevBuf<T>& b) {
    if (!b.p) return MO_OK;
    HIPCHK(c, hipMemsetAsync(b.p, c->poison, b.bytes, c->stream));
    c->poison_bufs++; c->poison_bytes += (int64_t)b.bytes;
    return MO_OK;
}
template <class S> int mo_poison_scratch(mo_ctx* c, S& s) {
    int rc = MO_OK;
    s.each_scratch([&](auto& b) { if (!rc) rc = mo_poison_buf(c, b); });
    return rc;
}
// The first line of every host and mo_dev_* entry point: the device selected and, while a poison byte is set, the context's and the
// plan's scratch filled with it (one branch when it is not).  mo_dbg_blur_level alone selects the device itself: it reads what the last
// extraction left in d_blur.
inline int mo_enter(mo_ctx* c) {
    HIPCHK(c, hipSetDevice(c->device));
    if (c->poison < 0) return MO_OK;
    if (int rc = mo_poison_scratch(c, *c)) return rc;
    return mo_poison_scratch(c, c->pb);
}
#define MO_ENTER(c) do { if (int e__ = mo_enter(c)) return e__; } while (0)

template <class T> int DevBuf<T>::regrow(mo_ctx* c, size_t n, size_t keep) {
    DevBuf q;
    if (int rc = q.realloc_bytes(c, n * sizeof(T))) return rc;
    if (p && keep) HIPCHK(c, hipMemcpyAsync(q.p, p, keep * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
    if (p) HIPCHK(c, hipStreamSynchronize(c->stream));
    swap(q);
    return MO_OK;
}

template <class T> int PinnedBuf<T>::reserve(mo_ctx* c, size_t n, unsigned flags) {
    if (p && n * sizeof(T) <= bytes) return MO_OK;
    if (p) { HIPCHK(c, hipStreamSynchronize(c->stream)); reset(); }
    HIPCHK(c, hipHostMalloc((void**)&p, n * sizeof(T), flags));
    bytes = n * sizeof(T);
    return MO_OK;
}

// the kernel's max-dynamic-LDS attribute raised to `bytes`, once per kernel function and context (ctx.hip)
int mo_raise_dyn_lds(mo_ctx* c, const void* kernel, int bytes);

// bump layout of a scratch region (c->d_tmp, a result slab): every piece starts on a 256-byte boundary
struct Layout {
    size_t total = 0;
    size_t take(size_t bytes) { const size_t o = total; total += mo_align(bytes, 256); return o; }
    template <class T> static T* at(void* base, size_t off) { return (T*)((uint8_t*)base + off); }
};

// a strided host image (h rows of `row` bytes, `stride` apart) -> dense rows at dst (pinned staging)
static inline void mo_copy_rows(uint8_t* dst, const uint8_t* src, size_t row, int h, size_t stride) {
    if (stride == row) std::memcpy(dst, src, row * h);
    else for (int y = 0; y < h; y++) std::memcpy(dst + (size_t)y * row, src + (size_t)y * stride, row);
}

// pinned, device-mapped host staging of the single-call host entry points (grow-only)
int mo_host_stage(mo_ctx* c, size_t bytes);
// flag words of the host entry points (see api.hip)
static inline int* mo_host_flags(mo_ctx* c) { return c->d_flags + 4; }
// the two host flag words read back after a call: bit 0 = response ties overflowed the final-keypoint slots of the levels in word 1
// (recorded in c->tie_overflow / c->tie_levels), bit 1 = more results than the caller's cap (cap_msg); MO_OK or MO_ERR_CAPACITY
int mo_decode_host_flags(mo_ctx* c, int f0, int f1, const char* cap_msg = "more keypoints than cap; counts holds the required sizes");

// Host-side clock of the single-call entry points (mo_host_times): [0] entry -> everything enqueued (staging memcpy, copies, launches),
// [1] the wait for the stream, [2] unpacking into the caller's arrays, [3] the whole call; microseconds.
static inline double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct HostClock {
    mo_ctx* c; double t0, t1 = 0, t2 = 0;
    explicit HostClock(mo_ctx* c_) : c(c_), t0(now_us()) { c->timing = c->host_timing; }
    void enqueued() { t1 = now_us(); }
    void waited() { t2 = now_us(); }
    ~HostClock() {
        const double t3 = now_us();
        if (t1 == 0) t1 = t2 = t3; else if (t2 == 0) t2 = t3;
        c->host_us[0] = t1 - t0; c->host_us[1] = t2 - t1; c->host_us[2] = t3 - t2; c->host_us[3] = t3 - t0;
        c->timing = true;  // (the mo_dev_* calls always record their stage events: bench.py reads them)
    }
};

// device pipeline on frames already resident as dense gray [batch][h][w] (api.hip); host_call != 0: the caller opened the stage set and
// the kernels raise their bits in the host flag words (1: cleared here by a fill, 2: already cleared by the upload kernel)
int mo_run_extract(mo_ctx* c, const mo_orb_params* p, const uint8_t* d_gray, int w, int h, int batch, mo_keypoint* d_kps, uint8_t* d_desc,
                   int cap, int32_t* d_counts, int host_call);
// frame_api.hip: single-frame extraction into a resident result slot (pinned staging in and out, one synchronisation)
int mo_detect_single(mo_ctx* c, const mo_orb_params* p, const uint8_t* img, int w, int h, int stride, int ch, mo_keypoint* kps,
                     uint8_t* desc, int cap, int* counts);

int mo_slot_acquire(mo_ctx* c, int rows, int* slot);   // frame_api.hip: resident result slots for the other single-frame entry points
uint64_t mo_slot_commit(mo_ctx* c, int slot, int n);
uint8_t* mo_stage_dev(mo_ctx* c);                       // device address of the pinned staging buffer
// frame_api.hip: a frame named by the token of a resident slot or by host arrays -> *slot (-1: not resident) and its row count *n;
// MO_ERR_ARG ("<what> token is stale and no host arrays were given") when the token is not alive and the arrays are missing
int mo_slot_of(const mo_ctx* c, uint64_t token);
int mo_frame_lookup(mo_ctx* c, const mo_frame_ref* f, const char* what, int* slot, int* n);
// the n rows of a looked-up frame -> d_kps / d_desc on the context stream: device to device from its slot, else from the host arrays
int mo_frame_copy_rows(mo_ctx* c, const mo_frame_ref* f, int slot, int n, mo_keypoint* d_kps, uint8_t* d_desc);
void mo_copy_out_launch(mo_ctx* c, const void* d_src, void* h_dst_dev, size_t bytes);  // device -> pinned staging, one small kernel

// stage timing helpers (hipEvents on the context stream)
void mo_stage_begin(mo_ctx* c);
void mo_stage_mark(mo_ctx* c, const char* name);

// orb_plan.cpp-equivalent host logic (ctx.hip)
int mo_build_plan(mo_ctx* c, const mo_orb_params* p, int w, int h, int batch);

// kernel launchers (orb_kernels.hip)
int orb_launch_gray(mo_ctx* c, const uint8_t* d_bgr, int w, int h, int batch, uint8_t* d_gray);
int orb_launch_ingest(mo_ctx* c, const uint8_t* src_mapped, int w, int h, int ch, uint8_t* d_gray, int* flags_clear);
// blur_margin >= 0: the resize launches may also write the blurred levels 0 .. nlevels-2 (*blurred says whether they did)
int orb_launch_pyramid(mo_ctx* c, const uint8_t* d_gray, int batch, int nlevels, int margin, int blur_margin = -1,
                       bool* blurred = nullptr);
// front_single.hip: pyramid + blur of a few frames in ONE launch (single-frame calls); fs_build runs with the plan and leaves
// c->fs_ok false for geometries it does not cover, which keep orb_launch_pyramid + orb_launch_blur
#define MO_FS_MAX_BATCH 2
int fs_build(mo_ctx* c);
int orb_launch_front_single(mo_ctx* c, const uint8_t* d_gray, int batch, int want_blur);
int orb_launch_blur(mo_ctx* c, const uint8_t* d_gray, int batch, int nlevels, int margin, int first_level = 0);
int orb_launch_fast(mo_ctx* c, const uint8_t* d_gray, int batch, int level_lo = 0, int level_hi = MO_MAX_LEVELS);
int orb_launch_select(mo_ctx* c, const uint8_t* d_gray, int batch, int level_lo = 0, int level_hi = MO_MAX_LEVELS);
int orb_launch_describe(mo_ctx* c, const uint8_t* d_gray, int batch, mo_keypoint* d_kps, uint8_t* d_desc, int cap,
                        int* d_counts);
int orb_launch_describe_given(mo_ctx* c, const uint8_t* d_gray, const mo_keypoint* d_kps, int n, uint8_t* d_desc, const int* d_n = nullptr,
                              int batch = 1, int n_stride = 0);
int gftt_records_launch(mo_ctx* c, const float* d_xy, int* d_cell_n, int per_cell, int w, int h, int edge, mo_keypoint* d_rec,
                        int32_t* d_kept, int rec_stride, int32_t* d_counts_out, int batch, int32_t* d_kbase = nullptr);
// orb_kernels.hip: descriptors of the batched grid detector's records out of one blurred LDS tile per grid cell; returns MO_ERR_UNSUPPORTED
// (without setting the error text) when a cell + halo does not fit the tile, and the caller takes orb_launch_describe_given
int orb_launch_describe_cells(mo_ctx* c, const mo_keypoint* d_kps, const int32_t* d_kbase, uint8_t* d_desc, int cap, int batch);
int orb_launch_retain_probe(mo_ctx* c, const float* d_resp, int n, int n_points, int order, int32_t* d_order,
                            int* d_nout);
// match_kernels.hip
int match_launch_pairs(mo_ctx* c, const uint8_t* d_q, const uint8_t* d_t, size_t q_stride, size_t t_stride,
                       const int32_t* d_counts, const int32_t* d_qf, const int32_t* d_tf, int nq_fixed, int nt_fixed,
                       int n_pairs, int out_stride, double ratio, int32_t* d_idx, int32_t* d_dist, uint8_t* d_pass);
// gftt_kernels.hip
int gftt_launch(mo_ctx* c, const uint8_t* d_gray, int w, int h, int n_features, float* d_eig, float* d_xy, int* d_n, int batch = 1);
// twoview_kernels.hip
struct TwoViewArgs {  // (an aggregate passed by value to the k_tv_* kernels: every field defaults to zero / null)
    int n_pairs = 0, cap = 0, n_hyp = 0;
    int model = 0;  // 0: essential matrix (K-normalised coordinates, thr_px / focal) + pose + triangulation;
                    // 1: fundamental matrix (pixel coordinates, Hartley-normalised with one common scale): F in d_E, mask in d_ransac
    double K[9] = {}, thr_px = 0;
    uint64_t seed = 0;
    uint64_t pair_base = 0;  // global index of pair 0 (sharded batches): the sampling stream of a pair depends on its global index only
    // per pair: matches are read from the matcher outputs + keypoints, or from explicit point arrays
    const mo_keypoint* d_kps = nullptr; const int32_t* d_counts = nullptr; const int32_t* d_match_idx = nullptr; const uint8_t* d_match_pass = nullptr;
    const int32_t* d_sel = nullptr; const int32_t* d_sel_n = nullptr;  // tracking mode: [pairs][cap][2] (queryIdx, trainIdx) in the caller's order +
                                                                       // counts; when set, these replace the ratio-test flags as the list of correspondences
    const float* d_p1 = nullptr; const float* d_p2 = nullptr; int m_fixed = 0;  // explicit points (host API): [m][2]
    const int32_t* d_qf = nullptr; const int32_t* d_tf = nullptr;  // keyframe mode: [pairs] query / train frame of each pair (null: pair p = frames p, p + 1)
    int need_two = 0;                                   // keyframe mode: only queries with a second neighbour take part
    const double* d_P1 = nullptr; const double* d_P2 = nullptr;  // fundamental model + these ([pairs][12], pixel projection matrices): the inliers are
                                                        // triangulated with them into d_points (local_mapper.py:148-149)
    const double* d_E_in = nullptr; const uint8_t* d_mask_in = nullptr;  // recoverPose on a GIVEN essential matrix ([pairs][9]) and consensus mask
                                                        // ([pairs][cap] by query index, may be null = all): no RANSAC, no refit
    double* d_pose = nullptr;    // [pairs][12]
    double* d_E = nullptr;       // [pairs][9] or null
    float* d_points = nullptr;   // [pairs][cap][3]
    uint8_t* d_inlier = nullptr; // [pairs][cap] pose mask
    uint8_t* d_ransac = nullptr; // [pairs][cap] RANSAC (Sampson) mask or null
    int32_t* d_n_points = nullptr; // [pairs]
    int* flags = nullptr;        // capacity flag word (none raised by this stage any more); set by twoview_launch
};
static_assert(std::is_trivially_copyable<TwoViewArgs>::value, "TwoViewArgs is a kernel argument");
// the fundamental-matrix RANSAC of the F sites (mo_find_fundamental, MO_MODE_KEYFRAME, the LocalMapper): pixel coordinates, identity K
static inline TwoViewArgs tv_fundamental(int n_pairs, int cap, int n_hyp, double thr_px, uint64_t seed, uint64_t pair_base) {
    TwoViewArgs a;
    a.n_pairs = n_pairs; a.cap = cap; a.n_hyp = n_hyp; a.model = 1;
    a.K[0] = a.K[4] = a.K[8] = 1.0;
    a.thr_px = thr_px; a.seed = seed; a.pair_base = pair_base;
    return a;
}
int twoview_launch(mo_ctx* c, const TwoViewArgs& a);
// twoview_h.hip: the homography branch (ORB-SLAM2's H model beside the essential path: hypotheses, CheckHomography scores, DLT refits,
// SH / SF / RH, ReconstructH with CheckRT over the eight candidates).  Explicit correspondences only, batched over pairs.
#define HF_NSTAT 23  // doubles per pair: SH, SF, RH, cos of the parallax of the 8 candidates (2 = none), R (9) and t (3) of the best one
#define HF_NINFO 16  // ints per pair: n_good[8], best, second (-1: none), H inliers, accepted, winning hypothesis (-1: no model), refits, decomposed
struct HfArgs {  // (an aggregate passed by value to the k_h_* kernels)
    int n_pairs = 0, cap = 0, n_hyp = 0, m_fixed = 0;
    double K[9] = {}, sigma = 1.0;
    double cos_max = 0;          // cos(min_parallax): a candidate's parallax is large enough when its cos is at most this
    int min_triangulated = 50;
    uint64_t seed = 0, pair_base = 0;
    const float* d_p1 = nullptr; const float* d_p2 = nullptr;  // [pairs][m_fixed][2] pixels
    const double* d_E = nullptr;  // [pairs][9] the essential path's result for the same pairs (NaN: none): SF is its CheckFundamental score
    double* d_H = nullptr;        // [pairs][9] pixels, unit Frobenius norm (NaN: no model)
    double* d_stat = nullptr;     // [pairs][HF_NSTAT]
    int32_t* d_info = nullptr;    // [pairs][HF_NINFO]
    uint8_t* d_hmask = nullptr;   // [pairs][cap] H inliers (both transfer directions inside the threshold)
    uint8_t* d_good = nullptr;    // [pairs][cap] map points of the best candidate (CheckRT passed with parallax)
    float* d_X = nullptr;         // [pairs][cap][3] their coordinates in camera 1 (NaN elsewhere)
};
static_assert(std::is_trivially_copyable<HfArgs>::value, "HfArgs is a kernel argument");
int twoview_h_launch(mo_ctx* c, const HfArgs& a);
// undistort_kernels.hip
int undistort_launch(mo_ctx* c, const uint8_t* d_src, uint8_t* d_dst, int w, int h, int ch, int batch, const double K[9],
                     const double dist[5]);
// track_kernels.hip
int track_select_launch(mo_ctx* c, const mo_keypoint* d_kps, const int32_t* d_counts, const int32_t* d_qf, const int32_t* d_tf,
                        const int32_t* d_midx, const int32_t* d_mdist, const uint8_t* d_mpass, int cap, int n_pairs, int w, int h,
                        double disp_frac, int32_t* d_sel, int32_t* d_sel_dist, int32_t* d_sel_n);
size_t twoview_workspace_bytes(int n_pairs, int cap, int n_hyp);
int triangulate_launch(mo_ctx* c, const double* P1, const double* P2, const float* d_p1, const float* d_p2, int n, float* d_X4);
