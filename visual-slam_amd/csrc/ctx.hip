// ctx.hip -- context lifetime, the per-(w,h,params) plan, work-buffer sizing and stage timing.
//
// What a plan is, and the host arithmetic that derives it once per image size, is in plan_tables.h; fill_plan below turns it
// into device memory: the table block in one upload, then the work buffers.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include <cstdlib>

#include "common.h"

int mo_fail(mo_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

static std::string g_create_err;

extern "C" int mo_abi_version(void) { return MO_ABI_VERSION; }

extern "C" int mo_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" mo_ctx* mo_create(int device, int max_w, int max_h, int max_batch) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_create_err = "mo_create: no HIP device available (this library has no CPU fallback)";
        return nullptr;
    }
    if (device < 0 || device >= n || max_w < 64 || max_h < 64 || max_w > 4095 || max_h > 4095 || max_batch < 1) {
        g_create_err = "mo_create: bad arguments (need 64 <= w,h <= 4095, batch >= 1, valid device)";
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        g_create_err = "mo_create: hipSetDevice failed";
        return nullptr;
    }
    mo_ctx* c = new mo_ctx();
    c->device = device;
    c->max_w = max_w; c->max_h = max_h; c->max_batch = max_batch;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
        g_create_err = "mo_create: hipStreamCreate failed";
        delete c;
        return nullptr;
    }
    c->stream = c->own_stream;
    // the one environment switch of the library: VSLAM_AMD_MATCHER=mfma selects the opt-in matrix-core matcher (identical results;
    // north_star prescribes XOR + popcount as the default, bench.py times the opt-in beside it); valu1 | valu2 | valu4 | valu8 keep the
    // default kernel and force the number of train slices of every launch (A/B and tests; valu = the launch rule)
    if (const char* e = getenv("VSLAM_AMD_MATCHER")) {
        c->match_mode = std::strcmp(e, "mfma") == 0 ? 1 : 0;
        for (int s : {1, 2, 4, 8})
            if (std::strcmp(e, ("valu" + std::to_string(s)).c_str()) == 0) c->match_slices = s;
    }
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->n_cu <= 0) {
        g_create_err = "mo_create: the device does not report its compute units";
        delete c;
        return nullptr;
    }
    // hipEventDisableSystemFence: these events order work of ONE device (kernel boundaries already release / acquire at agent
    // scope); the default system-scope fence of an event record writes the L2 back and cost 6 - 17 us of idle GPU at every stage mark
    // (kernel trace: gaps only where an event sits between two kernels), 0.06 ms of a 2.2 ms step (profiles/r02_ab_event_fence.txt).
    const unsigned evf = (unsigned)hipEventDisableSystemFence;
    for (TimingSet& t : c->tsets)
        for (int i = 0; i <= MO_NSTAGES; i++) hipEventCreateWithFlags(&t.ev[i], evf);
    if (c->d_flags.reserve_exact(c, 8) != MO_OK) {
        g_create_err = "mo_create: hipMalloc failed";
        delete c;
        return nullptr;
    }
    hipMemset(c->d_flags, 0, 8 * sizeof(int));
    c->flags_cur = c->d_flags;
    return c;
}

// raises a kernel's limit of dynamic LDS once per kernel function: the launchers call this on every launch
int mo_raise_dyn_lds(mo_ctx* c, const void* kernel, int bytes) {
    if (std::find(c->dyn_lds_raised.begin(), c->dyn_lds_raised.end(), kernel) != c->dyn_lds_raised.end()) return MO_OK;
    HIPCHK(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    c->dyn_lds_raised.push_back(kernel);
    return MO_OK;
}

static void free_plan_buffers(mo_ctx* c) {
    c->pb = PlanBufs();
    c->plan_valid = false;
}

extern "C" void mo_destroy(mo_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    mo_comm_destroy(c);
    for (TimingSet& t : c->tsets) {
        for (int i = 0; i <= MO_NSTAGES; i++) if (t.ev[i]) hipEventDestroy(t.ev[i]);
    }
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    delete c;  // every buffer frees itself (DevBuf, PinnedBuf)
}

extern "C" const char* mo_last_error(mo_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

extern "C" int mo_set_stream(mo_ctx* c, void* s) {
    if (!c) return MO_ERR_ARG;
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return MO_OK;
}

// The HIP null stream has the handle 0, which mo_set_stream reads as "the context's own stream": a caller whose work sits on the
// null stream (torch's default stream) selects it with this call, so that the library's launches are ordered with that work.
extern "C" int mo_set_stream_null(mo_ctx* c) {
    if (!c) return MO_ERR_ARG;
    c->stream = nullptr;
    return MO_OK;
}

extern "C" int mo_sync(mo_ctx* c) {
    if (!c) return MO_ERR_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MO_OK;
}

void mo_stage_begin(mo_ctx* c) {
    c->tcur = (c->tcur + 1) % MO_TIMING_SLOTS;
    TimingSet& t = c->tsets[c->tcur];
    t.n_stages = 0;
    if (c->timing) hipEventRecord(t.ev[0], c->stream);
}

void mo_stage_mark(mo_ctx* c, const char* name) {
    TimingSet& t = c->tsets[c->tcur];
    if (!c->timing || t.n_stages >= MO_NSTAGES) return;
    t.names[t.n_stages] = name;
    t.n_stages++;
    hipEventRecord(t.ev[t.n_stages], c->stream);
}

extern "C" int mo_stage_times_back(mo_ctx* c, int back, const char*** names, float* ms, int cap) {
    if (!c) return MO_ERR_ARG;
    if (back < 0 || back >= MO_TIMING_SLOTS) return mo_fail(c, MO_ERR_ARG, "mo_stage_times_back: back outside the ring of event sets");
    TimingSet& t = c->tsets[((c->tcur - back) % MO_TIMING_SLOTS + MO_TIMING_SLOTS) % MO_TIMING_SLOTS];
    if (t.n_stages == 0) return 0;
    HIPCHK(c, hipEventSynchronize(t.ev[t.n_stages]));
    int n = std::min(cap, t.n_stages);
    for (int i = 0; i < n; i++) {
        float v = 0;
        hipEventElapsedTime(&v, t.ev[i], t.ev[i + 1]);
        ms[i] = v;
    }
    t.names[t.n_stages] = nullptr;
    if (names) *names = t.names;
    return n;
}

extern "C" int mo_stage_times(mo_ctx* c, const char*** names, float* ms, int cap) { return mo_stage_times_back(c, 0, names, ms, cap); }

static bool params_equal(const mo_orb_params& a, const mo_orb_params& b) {
    return std::memcmp(&a, &b, sizeof(a)) == 0;
}

static int fill_plan(mo_ctx* c, const mo_orb_params* p, int w, int h, int batch);

int mo_build_plan(mo_ctx* c, const mo_orb_params* p, int w, int h, int batch) {
    if (!p) return mo_fail(c, MO_ERR_ARG, "params is NULL");
    if (w < 64 || h < 64 || w > c->max_w || h > c->max_h)
        return mo_fail(c, MO_ERR_ARG, "image size outside the context's max_w/max_h (or < 64)");
    if (batch < 1 || batch > c->max_batch) return mo_fail(c, MO_ERR_ARG, "batch outside 1..max_batch");
    if (p->nlevels < 1 || p->nlevels > MO_MAX_LEVELS) return mo_fail(c, MO_ERR_ARG, "nlevels must be 1..12");
    if (p->first_level != 0 || p->wta_k != 2 || p->score_type != 0 || p->patch_size != 31)
        return mo_fail(c, MO_ERR_UNSUPPORTED,
                       "only firstLevel=0, WTA_K=2, HARRIS_SCORE, patchSize=31 (the reference's values) are built");
    if (p->edge_threshold < 19 || p->edge_threshold > 1024)
        return mo_fail(c, MO_ERR_UNSUPPORTED, "edge_threshold must be >= 19 (descriptor radius)");
    if (p->nfeatures < 1 || !(p->scale_factor > 1.0f) || p->scale_factor > 2.0f)
        return mo_fail(c, MO_ERR_ARG, "nfeatures >= 1, 1 < scale_factor <= 2");
    if (p->select_order != MO_ORDER_LIBSTDCXX && p->select_order != MO_ORDER_MSVC)
        return mo_fail(c, MO_ERR_ARG, "select_order must be MO_ORDER_LIBSTDCXX or MO_ORDER_MSVC");

    const bool same_key = c->plan_valid && params_equal(c->plan_params, *p) && c->plan.w == w && c->plan.h == h;
    const bool same = same_key && !c->fin_slack_dirty;
    if (!same_key)   // another image size / parameter set: the grown slots were that one's
        for (int L = 0; L < MO_MAX_LEVELS; L++) c->fin_slack[L] = 1;
    if (same && batch <= c->pb.batch_alloc) return MO_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_plan_buffers(c);
    const int rc = fill_plan(c, p, w, h, batch);
    if (rc) free_plan_buffers(c);  // no half plan stays behind
    return rc;
}

static int fill_plan(mo_ctx* c, const mo_orb_params* p, int w, int h, int batch) {
    Plan& P = c->plan;
    PlanBufs& pb = c->pb;
    const char* why = "";
    if (int rc = plan_geometry(P, pb, p, w, h, c->max_batch, c->fin_slack, &why)) return mo_fail(c, rc, why);

    // the tables and, behind them, the tile records (at the margins of the batched pipeline): one buffer, one upload
    std::vector<uint32_t> blk, rec;
    plan_build_tables(P, pb, blk);
    plan_build_tile_records(P, pb, blk, mo_pyr_margin(P.edge_threshold), mo_blur_margin(P.edge_threshold), rec);
    const int nl = P.nlevels;
    pb.rb_ok = nl >= 2;
    for (int L = 1; L < nl && pb.rb_ok; L++) pb.rb_ok = pb.rs[L].two_pass_ok && orb_plan_resize_blur(P, pb, L, rec.data());
    pb.tile_rec = (uint32_t)mo_align(blk.size(), 64);
    blk.resize(pb.tile_rec, 0u);
    blk.insert(blk.end(), rec.begin(), rec.end());
    int rc;
    if ((rc = pb.d_tables.upload(c, blk))) return rc;

    // work buffers for `batch` frames
    size_t B = (size_t)batch;
    if ((rc = pb.d_pyr.reserve_exact(c, B * P.pyr_stride)) || (rc = pb.d_blur.reserve_exact(c, B * P.blur_stride)) ||
        (rc = pb.d_cand.reserve_exact(c, B * P.cand_stride)) || (rc = pb.d_strip_cnt.reserve_exact(c, B * P.strips_per_frame)) ||
        (rc = pb.d_scratch.reserve_exact(c, B * pb.scratch_stride)))
        return rc;
    if (pb.d_fin.reserve_exact(c, B * P.fin_stride) != MO_OK)
        return mo_fail(c, MO_ERR_HIP, "hipMalloc of the final-keypoint slots failed: " + std::to_string(B * P.fin_stride * sizeof(FinalKp)) +
                                          " bytes (" + std::to_string(batch) + " frames x " + std::to_string(P.fin_stride) + " slots; slots grow with response ties)");
    if ((rc = pb.d_fin_cnt.reserve_exact(c, B * MO_MAX_LEVELS))) return rc;
    // the describe kernels' list of left-over tiles (each sharing workgroup may leave an entry); every call's k_select clears the
    // count again
    if ((rc = pb.d_dtodo.reserve_exact(c, 1 + (size_t)pb.n_dtiles * B * DT_SPLIT_LATENCY))) return rc;
    HIPCHK(c, hipMemsetAsync(pb.d_dtodo, 0, sizeof(int), c->stream));
    if ((rc = fs_build(c))) return rc;  // single-frame pyramid + blur kernel: tile boxes of this plan
    pb.batch_alloc = batch;
    c->plan_params = *p;
    c->plan_valid = true;
    c->fin_slack_dirty = false;
    return MO_OK;
}
