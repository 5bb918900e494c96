// map_snapshot.hip -- the whole state of a device map as host arrays and back: mo_map_snapshot_dims, mo_map_export, mo_map_import
// (include/vslam_amd.h states the canonical form; snapshot.h the rules an imported snapshot must obey).
//
// The keyframe store is slot-strided (row (slot, r) at slot * row + r), the snapshot packed in position order.  k_snap_rows moves the
// rows of every keyframe between the two: one launch for the keypoints (7 dwords a row), one for the descriptors (8), either way.  A
// keyframe's rows are one contiguous run on both sides, so the kernel is a segmented copy: blockIdx.y names the keyframe, the blocks of
// one y stride over its run with consecutive lanes on consecutive units.  The unit is 16 bytes when both ends of the run are 16-byte
// aligned - always for the descriptors, for the keypoints when the keyframe's packed offset is a multiple of 4 rows - else 4 bytes,
// which the 28- and 32-byte rows always allow.  The packed side on the device is a staging buffer: one contiguous copy between it and
// the caller's array.  Everything else is one contiguous copy per array.
#include <string>
#include <vector>

#include "common.h"
#include "map_store.h"
#include "snapshot.h"

#define SNAP_BLOCK 256
#define SNAP_MAX_BLOCKS_X 64   // blocks striding over one keyframe's run (a 2000-row keyframe is 14 blocks of 16-byte units)

// the offsets table, the packed staging of the two row arrays and the host copy of the slot-ordered projection matrices: scratch
struct SnapBufs : MapFeature {
    DevBuf<int32_t> off;          // [n_kf + 1] first packed row of every position
    DevBuf<mo_keypoint> kps;      // [kf_rows]
    DevBuf<uint8_t> desc;         // [kf_rows][32]
    std::vector<int32_t> h_off;   // (alive until the chain's synchronisation)
    std::vector<double> h_P;      // [n_slots][12] as stored, gathered by position behind the synchronisation
    template <class F> void each_scratch(F f) { f(off); f(kps); f(desc); }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// PACK: strided -> packed (export); else packed -> strided (import).  rd: dwords per row.  Bounds: position k moves off[k + 1] - off[k]
// rows, at most `row` (the store's stride, sized by the largest count), inside slot pos_slot[k] and inside [off[k], off[k + 1]) of the
// packed array, whose size is off[n_kf] rows.
template <bool PACK>
__global__ __launch_bounds__(SNAP_BLOCK) void k_snap_rows(uint32_t* __restrict__ strided, uint32_t* __restrict__ packed, const int32_t* __restrict__ pos_slot,
                                                          const int32_t* __restrict__ off, int row, int rd) {
    const int k = blockIdx.y;
    const int o0 = off[k];
    const size_t n = (size_t)(off[k + 1] - o0) * rd;   // dwords of the run
    uint32_t* s = strided + (size_t)pos_slot[k] * row * rd;
    uint32_t* p = packed + (size_t)o0 * rd;
    const uint32_t* src = PACK ? s : p;
    uint32_t* dst = PACK ? p : s;
    const size_t step = (size_t)gridDim.x * SNAP_BLOCK, first = (size_t)blockIdx.x * SNAP_BLOCK + threadIdx.x;
    if ((((uintptr_t)s | (uintptr_t)p) & 15) == 0) {   // (uniform over the block)
        const size_t n4 = n >> 2;
        const uint4* src4 = (const uint4*)src;
        uint4* dst4 = (uint4*)dst;
        for (size_t i = first; i < n4; i += step) dst4[i] = src4[i];
        for (size_t i = (n4 << 2) + first; i < n; i += step) dst[i] = src[i];   // (a run of 7-dword rows may end inside a unit)
    } else {
        for (size_t i = first; i < n; i += step) dst[i] = src[i];
    }
}

// the offsets table of the live keyframes in position order, on the host and enqueued to the device; returns the rows in *total
static int snap_offsets(mo_map* m, SnapBufs& b, int64_t* total, int* max_cnt) {
    mo_ctx* c = m->c;
    const int n_kf = (int)m->pos_slot.size();
    b.h_off.assign((size_t)n_kf + 1, 0);
    int64_t sum = 0;
    int mx = 0;
    for (int k = 0; k < n_kf; k++) {
        const int n = m->h_kcnt[m->pos_slot[k]];
        sum += n; mx = std::max(mx, n);
        if (sum > INT32_MAX) return mo_fail(c, MO_ERR_CAPACITY, "keyframe rows beyond int32 indexing");
        b.h_off[k + 1] = (int32_t)sum;
    }
    *total = sum; *max_cnt = mx;
    if (int rc = b.off.reserve(c, (size_t)n_kf + 1)) return rc;
    HIPCHK(c, hipMemcpyAsync(b.off, b.h_off.data(), b.h_off.size() * 4, hipMemcpyHostToDevice, c->stream));
    return MO_OK;
}

// the two launches (position table and offsets enqueued by the caller); nothing to do without rows
template <bool PACK> static int snap_launch(mo_map* m, SnapBufs& b, int64_t rows, int max_cnt) {
    mo_ctx* c = m->c;
    const int n_kf = (int)m->pos_slot.size();
    if (!n_kf || !rows) return MO_OK;
    if (n_kf > 65535) return mo_fail(c, MO_ERR_UNSUPPORTED, "more keyframes than one launch of the snapshot kernels covers (65535)");
    auto gx = [&](int rd) { return (unsigned)std::min<size_t>(std::max<size_t>(((size_t)max_cnt * rd / 4 + SNAP_BLOCK - 1) / SNAP_BLOCK, 1), SNAP_MAX_BLOCKS_X); };
    hipLaunchKernelGGL(k_snap_rows<PACK>, dim3(gx(7), (unsigned)n_kf), dim3(SNAP_BLOCK), 0, c->stream, (uint32_t*)m->kkps.p, (uint32_t*)b.kps.p, m->d_pos_slot.p,
                       b.off.p, m->row, 7);
    hipLaunchKernelGGL(k_snap_rows<PACK>, dim3(gx(8), (unsigned)n_kf), dim3(SNAP_BLOCK), 0, c->stream, (uint32_t*)m->kdesc.p, (uint32_t*)b.desc.p, m->d_pos_slot.p,
                       b.off.p, m->row, 8);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, PACK ? "snapshot_pack" : "snapshot_unpack");
    return MO_OK;
}

static size_t img_bytes_of(const mo_map* m, int i) {
    return m->img[i] ? (size_t)std::max(m->img_w[i], 0) * std::max(m->img_h[i], 0) * std::max(m->img_ch[i], 0) : 0;
}

// what the host knows of the dims: everything but list_ids and st_live, which live on the device
static void snap_dims_host(const mo_map* m, mo_map_snapshot_dims_t* d) {
    *d = mo_map_snapshot_dims_t{};
    d->n_kf = (int32_t)m->pos_slot.size();
    for (int s : m->pos_slot) d->kf_rows += m->h_kcnt[s];
    d->n_pts = m->n_pts; d->n_obs = m->n_obs;
    d->list_rows = m->list_rows;
    d->kf_stored = m->kf_stored; d->id_bound = m->id_bound;
    for (int i = 0; i < 2; i++) {
        d->img_bytes[i] = (int64_t)img_bytes_of(m, i);
        // an image without pixels is stored as none: its dims say so (a buffer kept from an earlier keyframe is not state)
        d->img_w[i] = d->img_bytes[i] ? m->img_w[i] : 0; d->img_h[i] = d->img_bytes[i] ? m->img_h[i] : 0; d->img_ch[i] = m->img_ch[i];
    }
    d->img_cur = m->img_cur;
}

// the device's part enqueued into tail[4] (the map's pinned h_stat): st_live (3 words) and the end of the live list offsets (0 without lists)
static int snap_tail_enqueue(mo_map* m, int32_t* tail) {
    mo_ctx* c = m->c;
    tail[3] = 0;
    HIPCHK(c, hipMemcpyAsync(tail, m->st + ST_NPTS, 12, hipMemcpyDeviceToHost, c->stream));
    if (m->list_rows) HIPCHK(c, hipMemcpyAsync(tail + 3, m->loff[m->lcur] + m->list_rows, 4, hipMemcpyDeviceToHost, c->stream));
    return MO_OK;
}

extern "C" int mo_map_snapshot_dims(mo_map* m, mo_map_snapshot_dims_t* d) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!d) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    MAP_ENTER(m);
    snap_dims_host(m, d);
    int32_t* tail = m->h_stat;   // (pinned and the map's own: a copy that is still pending when a call fails lands in live memory)
    const int rc = snap_tail_enqueue(m, tail);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (rc) return rc;
    for (int i = 0; i < 3; i++) d->st_live[i] = tail[i];
    d->list_ids = tail[3];
    return MO_OK;
}

#define SNAP_D2H(dst, src, bytes) do { if ((bytes) && (dst)) HIPCHK(c, hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, c->stream)); } while (0)
#define SNAP_H2D(dst, src, bytes) do { if (bytes) HIPCHK(c, hipMemcpyAsync((dst), (src), (bytes), hipMemcpyHostToDevice, c->stream)); } while (0)

// the export behind its argument checks; a failure may leave copies into the caller's arrays pending (mo_map_export drains them)
static int snap_export(mo_map* m, mo_map_snapshot* s) {
    mo_ctx* c = m->c;
    int rc;
    MAP_ENTER(m);
    // s->dims comes in as mo_map_snapshot_dims gave it: the sizes the arrays were allocated for.  What the host knows of them is
    // checked here, what the device knows (list_ids, st_live) behind the call's one synchronisation.
    mo_map_snapshot_dims_t d;
    snap_dims_host(m, &d);
    d.list_ids = s->dims.list_ids;
    for (int i = 0; i < 3; i++) d.st_live[i] = s->dims.st_live[i];
    if (std::memcmp(&d, &s->dims, sizeof d) != 0 || d.list_ids < 0 || (!d.list_rows && d.list_ids))
        return mo_fail(c, MO_ERR_CAPACITY, "the snapshot's dims are not this map's: fill them with mo_map_snapshot_dims and allocate for them");
    const size_t n_kf = (size_t)d.n_kf, np = (size_t)d.n_pts, no = (size_t)d.n_obs;
    if ((n_kf && (!s->kf_cnt || !s->kf_ord || !s->kf_P)) || (d.kf_rows && (!s->kf_kps || !s->kf_desc)) ||
        (np && (!s->xyz || !s->col || !s->id || !s->dref_kf || !s->dref_row || !s->life)) || !s->obs_off || (no && (!s->obs_kf || !s->obs_kp)) ||
        (d.list_rows && (!s->list_off || !s->kf_red)) || (d.list_ids && !s->list_ids) || (d.img_bytes[0] && !s->img[0]) || (d.img_bytes[1] && !s->img[1]))
        return mo_fail(c, MO_ERR_ARG, "NULL array with a count above 0 (mo_map_snapshot_dims gives the counts)");
    HostClock clk(c);
    SnapBufs& b = map_feature<SnapBufs>(m);
    int64_t rows = 0;
    int max_cnt = 0;
    mo_stage_begin(c);
    if ((rc = upload_pos_slot(m)) || (rc = snap_offsets(m, b, &rows, &max_cnt))) return rc;
    if ((rc = mo_reserve(c, b.kps, (size_t)std::max<int64_t>(rows, 1), b.desc, (size_t)std::max<int64_t>(rows, 1) * 32))) return rc;
    if ((rc = snap_launch<true>(m, b, rows, max_cnt))) return rc;
    SNAP_D2H(s->kf_kps, b.kps.p, (size_t)rows * sizeof(mo_keypoint));
    SNAP_D2H(s->kf_desc, b.desc.p, (size_t)rows * 32);
    b.h_P.resize((size_t)m->n_slots * 12);
    SNAP_D2H(b.h_P.data(), m->kP.p, (size_t)m->n_slots * 96);
    const MapPts p = m->P[m->cur].view();
    SNAP_D2H(s->xyz, p.xyz, np * 12); SNAP_D2H(s->col, p.col, np * 3); SNAP_D2H(s->id, p.id, np * 4);
    SNAP_D2H(s->dref_kf, p.dkf, np * 4); SNAP_D2H(s->dref_row, p.drow, np * 4); SNAP_D2H(s->obs_off, p.off, (np + 1) * 4);
    SNAP_D2H(s->obs_kf, p.okf, no * 4); SNAP_D2H(s->obs_kp, p.okp, no * 4); SNAP_D2H(s->life, p.life, np * sizeof(int4));
    if (d.list_rows) {
        SNAP_D2H(s->list_off, m->loff[m->lcur].p, ((size_t)d.list_rows + 1) * 4);
        SNAP_D2H(s->list_ids, m->lids[m->lcur].p, (size_t)d.list_ids * 4);
        SNAP_D2H(s->kf_red, m->kf_red.p, (size_t)d.list_rows * 4);
    }
    for (int i = 0; i < 2; i++) SNAP_D2H(s->img[i], m->img[i].p, (size_t)d.img_bytes[i]);
    int32_t* tail = m->h_stat;
    if ((rc = snap_tail_enqueue(m, tail))) return rc;
    mo_stage_mark(c, "snapshot_copy");
    if ((rc = map_sync(c, clk))) return rc;
    if (tail[3] != d.list_ids || tail[0] != d.st_live[0] || tail[1] != d.st_live[1] || tail[2] != d.st_live[2])
        return mo_fail(c, MO_ERR_CAPACITY, "the snapshot's dims are not this map's: fill them with mo_map_snapshot_dims and allocate for them");
    for (size_t k = 0; k < n_kf; k++) {
        const int slot = m->pos_slot[k];
        s->kf_cnt[k] = m->h_kcnt[slot]; s->kf_ord[k] = m->slot_ord[slot];
        std::copy(b.h_P.begin() + (size_t)slot * 12, b.h_P.begin() + (size_t)slot * 12 + 12, s->kf_P + k * 12);
    }
    return MO_OK;
}

extern "C" int mo_map_export(mo_map* m, mo_map_snapshot* s) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!s) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const int rc = snap_export(m, s);
    if (rc) {   // nothing enqueued may still write into the caller's arrays once the call has returned (the error text stays)
        const std::string why = c->err;
        hipStreamSynchronize(c->stream);
        c->err = why;
    }
    return rc;
}

// the state of a fresh map of enough capacity filled from a checked snapshot: every state buffer is written up to its count
static int snap_fill(mo_map* m, const mo_map_snapshot* s) {
    mo_ctx* c = m->c;
    const mo_map_snapshot_dims_t& d = s->dims;
    const size_t n_kf = (size_t)d.n_kf, np = (size_t)d.n_pts, no = (size_t)d.n_obs;
    int rc;
    HostClock clk(c);
    // the keyframe store: slot == position, serial 1 everywhere (the keyframe database of a map starts at 0: every slot is stale)
    m->h_kcnt.assign(s->kf_cnt, s->kf_cnt + n_kf);
    m->kserial.assign(n_kf, 1);
    m->slot_ord.assign(s->kf_ord, s->kf_ord + n_kf);
    m->pos_slot.resize(n_kf);
    for (size_t k = 0; k < n_kf; k++) m->pos_slot[k] = (int32_t)k;
    m->n_slots = (int)n_kf;
    m->kf_stored = d.kf_stored;
    SnapBufs& b = map_feature<SnapBufs>(m);
    int64_t rows = 0;
    int max_cnt = 0;
    mo_stage_begin(c);
    if ((rc = upload_pos_slot(m)) || (rc = snap_offsets(m, b, &rows, &max_cnt))) return rc;
    if ((rc = mo_reserve(c, b.kps, (size_t)std::max<int64_t>(rows, 1), b.desc, (size_t)std::max<int64_t>(rows, 1) * 32))) return rc;
    SNAP_H2D(m->kcnt.p, s->kf_cnt, n_kf * 4);
    SNAP_H2D(m->kP.p, s->kf_P, n_kf * 96);
    SNAP_H2D(b.kps.p, s->kf_kps, (size_t)rows * sizeof(mo_keypoint));
    SNAP_H2D(b.desc.p, s->kf_desc, (size_t)rows * 32);
    // the points, into copy 0
    const MapPts p = m->P[0].view();
    m->cur = 0;
    SNAP_H2D(p.xyz, s->xyz, np * 12); SNAP_H2D(p.col, s->col, np * 3); SNAP_H2D(p.id, s->id, np * 4);
    SNAP_H2D(p.dkf, s->dref_kf, np * 4); SNAP_H2D(p.drow, s->dref_row, np * 4); SNAP_H2D(p.off, s->obs_off, (np + 1) * 4);
    SNAP_H2D(p.okf, s->obs_kf, no * 4); SNAP_H2D(p.okp, s->obs_kp, no * 4); SNAP_H2D(p.life, s->life, np * sizeof(int4));
    m->n_pts = d.n_pts; m->n_obs = d.n_obs; m->id_bound = d.id_bound;
    // the lists, into set 0
    m->lcur = 0; m->list_rows = d.list_rows;
    if (d.list_rows) {
        if ((rc = mo_reserve(c, m->loff[0], (size_t)d.list_rows + 1, m->lids[0], (size_t)std::max<int64_t>(d.list_ids, 1), m->kf_red, (size_t)d.list_rows))) return rc;
        SNAP_H2D(m->loff[0].p, s->list_off, ((size_t)d.list_rows + 1) * 4);
        SNAP_H2D(m->lids[0].p, s->list_ids, (size_t)d.list_ids * 4);
        SNAP_H2D(m->kf_red.p, s->kf_red, (size_t)d.list_rows * 4);
    }
    for (int i = 0; i < 2; i++) {
        if (d.img_bytes[i]) {
            if ((rc = m->img[i].reserve(c, (size_t)d.img_bytes[i]))) return rc;
            SNAP_H2D(m->img[i].p, s->img[i], (size_t)d.img_bytes[i]);
        }
        m->img_w[i] = d.img_w[i]; m->img_h[i] = d.img_h[i]; m->img_ch[i] = d.img_ch[i];
    }
    m->img_cur = d.img_cur;
    SNAP_H2D(m->st + ST_NPTS, d.st_live, 12);
    mo_stage_mark(c, "snapshot_copy");
    if ((rc = snap_launch<false>(m, b, rows, max_cnt))) return rc;   // (behind every copy: the stage mark times the two scatters alone)
    return map_sync(c, clk);   // (the caller's arrays and the offsets table are read until here)
}

extern "C" int mo_map_import(mo_ctx* c, const mo_map_snapshot* s, int kf_slots, int kf_rows, int64_t pts_cap, int64_t obs_cap, mo_map** out) {
    if (!c) return MO_ERR_ARG;
    if (!out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (const char* why = snapshot_violation(s)) return mo_fail(c, MO_ERR_ARG, why);
    const mo_map_snapshot_dims_t& d = s->dims;
    int max_cnt = 0;
    for (int k = 0; k < d.n_kf; k++) max_cnt = std::max(max_cnt, s->kf_cnt[k]);
    mo_map* m = mo_map_create(c, std::max(kf_slots, d.n_kf), std::max(kf_rows, max_cnt), std::max(pts_cap, d.n_pts), std::max(obs_cap, d.n_obs));
    if (!m) return MO_ERR_HIP;   // (mo_map_create left the text)
    if (int rc = snap_fill(m, s)) {
        const std::string why = c->err;
        mo_map_destroy(m);
        return mo_fail(c, rc, why);
    }
    *out = m;
    return MO_OK;
}
