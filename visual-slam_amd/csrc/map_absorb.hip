// map_absorb.hip -- one device map appended to another: mo_map_absorb (include/vslam_amd.h states the rules A1 - A9; absorb.h holds the
// per-element rules and the argument checks).  src becomes the tail of dst, device to device, every index relocated; src is only read.
//
// Chain: reserve (a src keyframe wider than dst's row stride restrides dst through kf_reserve) -> k_absorb_rows twice (keypoints, 7
// dwords a row; descriptors, 8) -> k_absorb_points -> k_absorb_obs -> the image copies and the two live words -> one synchronisation.
// k_absorb_rows is k_snap_rows' segmented copy (map_snapshot.hip) with a slot-strided run on both sides: blockIdx.y names src's
// keyframe position, the blocks of one y stride over its run, the unit is 16 bytes when both ends of the run are 16-byte aligned (always
// for the descriptors; for the keypoints when both slot starts are, which a row stride that is a multiple of 4 gives), else 4 bytes.
// Every output element has one writer and no atomics are used: equal inputs give equal bytes.  No scratch: the kernels read src's own
// position table and counts.
#include <string>

#include "common.h"
#include "map_store.h"
#include "absorb.h"

#define ABS_BLOCK 256
#define ABS_MAX_BLOCKS_X 64   // blocks striding over one keyframe's run (map_snapshot.hip's figure)

// Bounds: src position k holds cnt = s_kcnt[s_pos_slot[k]] rows, at most s_row (src's stride) and at most d_row (the caller reserved
// dst for src's largest count); it lands in dst slot slot0 + k < dst's slot capacity (reserved).  The run is clamped to both strides.
// HEAD (the keypoint launch): block x == 0 of every y also writes the new slot's count and its projection matrix, byte for byte.
template <bool HEAD>
__global__ __launch_bounds__(ABS_BLOCK) void k_absorb_rows(const uint32_t* __restrict__ s_rows, uint32_t* __restrict__ d_rows, const int32_t* __restrict__ s_pos_slot,
                                                           const int32_t* __restrict__ s_kcnt, int s_row, int d_row, int slot0, int rd,
                                                           const double* __restrict__ s_P, double* __restrict__ d_P, int32_t* __restrict__ d_kcnt) {
    const int k = blockIdx.y;
    const int ss = s_pos_slot[k], ds = slot0 + k;
    const int cnt = s_kcnt[ss];
    if (HEAD && blockIdx.x == 0) {
        if (threadIdx.x < 12) d_P[(size_t)ds * 12 + threadIdx.x] = s_P[(size_t)ss * 12 + threadIdx.x];
        if (threadIdx.x == 12) d_kcnt[ds] = cnt;
    }
    const size_t n = (size_t)max(min(cnt, min(s_row, d_row)), 0) * rd;   // dwords of the run
    const uint32_t* src = s_rows + (size_t)ss * s_row * rd;
    uint32_t* dst = d_rows + (size_t)ds * d_row * rd;
    const size_t step = (size_t)gridDim.x * ABS_BLOCK, first = (size_t)blockIdx.x * ABS_BLOCK + threadIdx.x;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {   // (uniform over the block)
        const size_t n4 = n >> 2;
        const uint4* src4 = (const uint4*)src;
        uint4* dst4 = (uint4*)dst;
        for (size_t i = first; i < n4; i += step) dst4[i] = src4[i];
        for (size_t i = (n4 << 2) + first; i < n; i += step) dst[i] = src[i];   // (a run of 7-dword rows may end inside a unit)
    } else {
        for (size_t i = first; i < n; i += step) dst[i] = src[i];
    }
}

// one thread per point of src (A2): point i becomes dst point o.pt + i
__global__ __launch_bounds__(ABS_BLOCK) void k_absorb_points(MapPts src, int n, MapPts dst, AbsorbOffsets o) {
    const int i = blockIdx.x * ABS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t r = (size_t)o.pt + i;
    for (int k = 0; k < 3; k++) { dst.xyz[r * 3 + k] = src.xyz[(size_t)i * 3 + k]; dst.col[r * 3 + k] = src.col[(size_t)i * 3 + k]; }
    dst.id[r] = absorb_id(src.id[i], o);
    dst.dkf[r] = absorb_dref_kf(src.dkf[i], o);
    dst.drow[r] = src.drow[i];
    const int4 l = src.life[i];
    const int32_t in[4] = {l.x, l.y, l.z, l.w};
    int32_t out[4];
    absorb_life(in, o, out);
    dst.life[r] = make_int4(out[0], out[1], out[2], out[3]);
    dst.off[r + 1] = absorb_off(src.off[i + 1], o);   // (off[o.pt] is dst's own end and stays)
}

// one thread per observation entry of src (A3): entry e becomes dst entry o.obs + e
__global__ __launch_bounds__(ABS_BLOCK) void k_absorb_obs(MapView sv, int n, MapPts dst, AbsorbOffsets o) {
    const int e = blockIdx.x * ABS_BLOCK + threadIdx.x;
    if (e >= n) return;
    int32_t kf, kp;
    absorb_entry(sv.src.okf[e], sv.src.okp[e], sv.n_kf, [&](int pos) { return sv.kcnt[sv.pos_slot[pos]]; }, o, &kf, &kp);
    dst.okf[(size_t)o.obs + e] = kf; dst.okp[(size_t)o.obs + e] = kp;
}

static AbsorbSizes absorb_sizes(const mo_map* m) {
    return AbsorbSizes{(int64_t)m->pos_slot.size(), m->n_pts, m->n_obs, m->id_bound, m->kf_stored};
}

static void absorb_report(const mo_map* d, mo_map_absorb_out* out) {
    out->n_kf = (int64_t)d->pos_slot.size(); out->n_slots = d->n_slots; out->n_pts = d->n_pts; out->n_obs = d->n_obs;
    out->id_bound = d->id_bound; out->kf_stored = d->kf_stored;
}

extern "C" int mo_map_absorb(mo_map* d, mo_map* s, const mo_map_absorb_params* prm, mo_map_absorb_out* out) {
    if (!d) return MO_ERR_ARG;
    mo_ctx* c = d->c;
    if (const char* why = absorb_args_violation(d, s, prm, out)) return mo_fail(c, MO_ERR_ARG, why);
    const AbsorbSizes ds = absorb_sizes(d), ss = absorb_sizes(s);
    if (const char* why = absorb_sizes_violation(d->c, s->c, ds, ss)) {
        const std::string text = why;
        return mo_fail(c, text == ABSORB_CONTEXT ? MO_ERR_ARG : text == ABSORB_KEYFRAMES ? MO_ERR_UNSUPPORTED : MO_ERR_CAPACITY, text);
    }
    const AbsorbOffsets o{(int32_t)ds.n_kf, (int32_t)ds.n_pts, (int32_t)ds.n_obs, (int32_t)ds.id_bound, (int32_t)ds.kf_stored,
                          (int32_t)prm->dref_injected_shift, (int32_t)std::max<int64_t>(ds.kf_stored + ss.kf_stored - 1, 0)};
    const int slot0 = d->n_slots;
    out->kf_offset = o.kf; out->slot_offset = slot0; out->point_offset = ds.n_pts; out->obs_offset = ds.n_obs; out->id_offset = ds.id_bound;
    out->ordinal_offset = ds.kf_stored;
    absorb_report(d, out);
    if (absorb_is_noop(ss)) return MO_OK;
    MAP_ENTER(d);
    HostClock clk(c);
    int rc;
    const int n_kf_s = (int)ss.n_kf;
    int max_cnt = 0;
    for (int slot : s->pos_slot) max_cnt = std::max(max_cnt, s->h_kcnt[slot]);
    // reserve: the keyframe store (a wider keyframe restrides dst), the live copy of the point store, the images
    if ((rc = kf_reserve(d, max_cnt, slot0 + n_kf_s))) return rc;
    if ((rc = map_pts_reserve(d, d->cur, (size_t)(ds.n_pts + ss.n_pts), (size_t)(ds.n_obs + ss.n_obs), true))) return rc;
    size_t img_bytes[2] = {0, 0};
    if (n_kf_s)
        for (int i = 0; i < 2; i++) {
            img_bytes[i] = s->img[i] ? (size_t)std::max(s->img_w[i], 0) * std::max(s->img_h[i], 0) * std::max(s->img_ch[i], 0) : 0;
            if (img_bytes[i] && (rc = d->img[i].reserve(c, img_bytes[i]))) return rc;
        }
    mo_stage_begin(c);
    if (n_kf_s) {
        if ((rc = upload_pos_slot(s))) return rc;   // (src's own table, rewritten with what it holds)
        auto gx = [&](int rd) { return (unsigned)std::min<size_t>(std::max<size_t>(((size_t)max_cnt * rd / 4 + ABS_BLOCK - 1) / ABS_BLOCK, 1), ABS_MAX_BLOCKS_X); };
        hipLaunchKernelGGL(k_absorb_rows<true>, dim3(gx(7), (unsigned)n_kf_s), dim3(ABS_BLOCK), 0, c->stream, (const uint32_t*)s->kkps.p, (uint32_t*)d->kkps.p,
                           s->d_pos_slot.p, s->kcnt.p, s->row, d->row, slot0, 7, s->kP.p, d->kP.p, d->kcnt.p);
        hipLaunchKernelGGL(k_absorb_rows<false>, dim3(gx(8), (unsigned)n_kf_s), dim3(ABS_BLOCK), 0, c->stream, (const uint32_t*)s->kdesc.p, (uint32_t*)d->kdesc.p,
                           s->d_pos_slot.p, s->kcnt.p, s->row, d->row, slot0, 8, s->kP.p, d->kP.p, d->kcnt.p);
        HIPCHK(c, hipGetLastError());
    }
    mo_stage_mark(c, "absorb_rows");
    const MapPts dp = d->P[d->cur].view();
    if (ss.n_pts) {
        hipLaunchKernelGGL(k_absorb_points, dim3((unsigned)((ss.n_pts + ABS_BLOCK - 1) / ABS_BLOCK)), dim3(ABS_BLOCK), 0, c->stream, s->P[s->cur].view(),
                           (int)ss.n_pts, dp, o);
        HIPCHK(c, hipGetLastError());
    }
    mo_stage_mark(c, "absorb_points");
    if (ss.n_obs) {
        hipLaunchKernelGGL(k_absorb_obs, dim3((unsigned)((ss.n_obs + ABS_BLOCK - 1) / ABS_BLOCK)), dim3(ABS_BLOCK), 0, c->stream, map_view(s), (int)ss.n_obs, dp, o);
        HIPCHK(c, hipGetLastError());
    }
    mo_stage_mark(c, "absorb_obs");
    // A5: the tail's images are the ones the next keyframe colours from
    if (n_kf_s) {
        for (int i = 0; i < 2; i++) {
            if (img_bytes[i]) HIPCHK(c, hipMemcpyAsync(d->img[i].p, s->img[i].p, img_bytes[i], hipMemcpyDeviceToDevice, c->stream));
            d->img_w[i] = img_bytes[i] ? s->img_w[i] : 0; d->img_h[i] = img_bytes[i] ? s->img_h[i] : 0; d->img_ch[i] = s->img_ch[i];
        }
        d->img_cur = s->img_cur;
    }
    // A4: the live words of the next call; ST_NNEW stays dst's (its one reader, mo_map_add_keyframe, reads what its own chain wrote)
    int32_t* w = d->h_stat;   // (pinned and the map's own)
    w[0] = (int32_t)(ds.n_pts + ss.n_pts); w[1] = (int32_t)(ds.n_obs + ss.n_obs);
    HIPCHK(c, hipMemcpyAsync(d->st + ST_NPTS, w, 8, hipMemcpyHostToDevice, c->stream));
    // A1: the host's side of the new slots
    for (int k = 0; k < n_kf_s; k++) {
        const int sl = s->pos_slot[k];
        d->h_kcnt.push_back(s->h_kcnt[sl]);
        d->kserial.resize((size_t)slot0 + k + 1, 0); d->kserial[slot0 + k]++;
        d->slot_ord.resize((size_t)slot0 + k + 1); d->slot_ord[slot0 + k] = (int32_t)(ds.kf_stored + s->slot_ord[sl]);
        d->pos_slot.push_back(slot0 + k);
    }
    d->n_slots = slot0 + n_kf_s;
    d->kf_stored = ds.kf_stored + ss.kf_stored; d->id_bound = ds.id_bound + ss.id_bound;
    d->n_pts = ds.n_pts + ss.n_pts; d->n_obs = ds.n_obs + ss.n_obs;
    if ((rc = map_sync(c, clk))) return rc;
    absorb_report(d, out);
    return MO_OK;
}
