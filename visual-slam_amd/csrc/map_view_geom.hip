// map_view_geom.hip -- where every map point was seen from (mo_map_point_views in include/vslam_amd.h): the camera centre of every
// keyframe position from the store's own P, and per point ORB-SLAM2's MapPoint::UpdateNormalAndDepth - the mean viewing direction and
// the scale-invariance range.  Scratch, recomputed inside every call that needs it (the frustum mode of mo_map_track_frustum and
// mo_map_fuse_frustum, through view_enqueue of map_search.h): the map carries no per-point state for it, so no compaction moves it.
//
//   k_view_centres  one thread per keyframe position: C = -M^-1 p4 by cofactors (NaN: M is singular, the keyframe has no centre)
//   k_view_points   one thread per point (of the local map, when the caller has one): one walk over its valid observations - the unit
//                   vectors from the centres summed in stored order, the first observation with a centre is the reference; the centres
//                   staged in LDS when they fit (VIEW_LDS_KF keyframes), read from global memory beyond; one 16-byte record per point
// No atomics; every sum in stored order: equal maps give equal bytes.  -ffp-contract=off (Makefile): the arithmetic rounds like
// tests/view_restatement.py's.
#include <cmath>
#include <vector>

#include "common.h"
#include "map_store.h"
#include "map_search.h"

#define VIEW_BLOCK 256
#define VIEW_LDS_KF 2048   // 48 KiB of centres

struct ViewBufs : MapFeature {
    DevBuf<double> centre;                      // [n_kf][3] by keyframe position
    DevBuf<ViewRec> rec;                        // [point]
    DevBuf<int32_t> ref_pos, ref_oct, n_valid;  // [point] what mo_map_point_views reports besides the record
    // all of it is scratch: every call's chain writes what it reads
    template <class F> void each_scratch(F f) { f(centre); f(rec); f(ref_pos); f(ref_oct); f(n_valid); }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

__global__ __launch_bounds__(VIEW_BLOCK) void k_view_centres(const double* __restrict__ kP, const int32_t* __restrict__ pos_slot, int n_kf,
                                                              double* __restrict__ centre) {
    const int k = blockIdx.x * VIEW_BLOCK + threadIdx.x;
    if (k >= n_kf) return;
    const double* P = kP + (size_t)pos_slot[k] * 12;
    const double m00 = P[0], m01 = P[1], m02 = P[2], m10 = P[4], m11 = P[5], m12 = P[6], m20 = P[8], m21 = P[9], m22 = P[10];
    const double p0 = P[3], p1 = P[7], p2 = P[11];
    // adj = the transposed cofactors, row by row; det along the first row of M
    const double a00 = m11 * m22 - m12 * m21, a01 = m02 * m21 - m01 * m22, a02 = m01 * m12 - m02 * m11;
    const double a10 = m12 * m20 - m10 * m22, a11 = m00 * m22 - m02 * m20, a12 = m02 * m10 - m00 * m12;
    const double a20 = m10 * m21 - m11 * m20, a21 = m01 * m20 - m00 * m21, a22 = m00 * m11 - m01 * m10;
    const double det = m00 * a00 + m01 * a10 + m02 * a20;
    double c0 = -((a00 * p0 + a01 * p1 + a02 * p2) / det);
    double c1 = -((a10 * p0 + a11 * p1 + a12 * p2) / det);
    double c2 = -((a20 * p0 + a21 * p1 + a22 * p2) / det);
    if (det == 0.0 || !isfinite(c0) || !isfinite(c1) || !isfinite(c2)) c0 = c1 = c2 = __longlong_as_double(0x7ff8000000000000ll);
    centre[(size_t)k * 3] = c0; centre[(size_t)k * 3 + 1] = c1; centre[(size_t)k * 3 + 2] = c2;
}

// one thread per point: oct (when given) names the local map, the three int outputs may be NULL
template <bool LDS> __global__ __launch_bounds__(VIEW_BLOCK) void k_view_points(MapView v, const mo_keypoint* __restrict__ kkps,
                                                                                const double* __restrict__ centre, const int32_t* __restrict__ oct,
                                                                                double sf, ViewRec* __restrict__ rec, int32_t* __restrict__ ref_pos,
                                                                                int32_t* __restrict__ ref_oct, int32_t* __restrict__ n_valid) {
    extern __shared__ double s_centre[];
    if (LDS) {
        for (int j = threadIdx.x; j < v.n_kf * 3; j += VIEW_BLOCK) s_centre[j] = centre[j];
        __syncthreads();
    }
    const double* cc = LDS ? s_centre : centre;
    const int i = blockIdx.x * VIEW_BLOCK + threadIdx.x;
    if (i >= v.n_pts || (oct && oct[i] == TK_NOT_LOCAL)) return;
    const double X = v.src.xyz[(size_t)i * 3], Y = v.src.xyz[(size_t)i * 3 + 1], Z = v.src.xyz[(size_t)i * 3 + 2];
    double sx = 0.0, sy = 0.0, sz = 0.0, d_ref = 0.0;
    int cnt = 0, rp = -1, ro = 0;
    map_each_obs(v, i, [&](int, int pos, int slot, int kp) {
        const double cx = cc[pos * 3], cy = cc[pos * 3 + 1], cz = cc[pos * 3 + 2];
        if (cx != cx) return false;   // (no centre)
        const double dx = X - cx, dy = Y - cy, dz = Z - cz;
        const double d = sqrt(dx * dx + dy * dy + dz * dz);
        if (rp < 0) { rp = pos; ro = kkps[(size_t)slot * v.row + kp].octave; d_ref = d; }
        if (!(d > 0.0)) return false;
        sx += dx / d; sy += dy / d; sz += dz / d;
        cnt++;
        return false;
    });
    ViewRec r;
    r.nx = cnt ? (float)(sx / cnt) : 0.0f; r.ny = cnt ? (float)(sy / cnt) : 0.0f; r.nz = cnt ? (float)(sz / cnt) : 0.0f;
    r.max_dist = (float)(d_ref * trk_scale(sf, ro));
    rec[i] = r;
    if (ref_pos) { ref_pos[i] = rp; ref_oct[i] = ro; n_valid[i] = cnt; }
}

// both kernels enqueued; aux: the per-point int outputs too
static int view_launch(mo_map* m, ViewBufs& b, const int32_t* oct, double sf, bool aux) {
    mo_ctx* c = m->c;
    const int n_kf = (int)m->pos_slot.size();
    const size_t np = (size_t)m->n_pts;
    int rc;
    if ((rc = mo_reserve(c, b.centre, (size_t)n_kf * 3, b.rec, np))) return rc;
    if (aux && (rc = mo_reserve(c, b.ref_pos, np, b.ref_oct, np, b.n_valid, np))) return rc;
    hipLaunchKernelGGL(k_view_centres, dim3((unsigned)((n_kf + VIEW_BLOCK - 1) / VIEW_BLOCK)), dim3(VIEW_BLOCK), 0, c->stream, m->kP, m->d_pos_slot, n_kf,
                       b.centre);
    HIPCHK(c, hipGetLastError());
    if (np == 0) return MO_OK;
    const unsigned blocks = (unsigned)((np + VIEW_BLOCK - 1) / VIEW_BLOCK);
    int32_t* rp = aux ? b.ref_pos.p : nullptr;
    int32_t* ro = aux ? b.ref_oct.p : nullptr;
    int32_t* nv = aux ? b.n_valid.p : nullptr;
    if (n_kf <= VIEW_LDS_KF)
        hipLaunchKernelGGL(k_view_points<true>, dim3(blocks), dim3(VIEW_BLOCK), (size_t)n_kf * 3 * sizeof(double), c->stream, map_view(m), m->kkps, b.centre,
                           oct, sf, b.rec, rp, ro, nv);
    else
        hipLaunchKernelGGL(k_view_points<false>, dim3(blocks), dim3(VIEW_BLOCK), 0, c->stream, map_view(m), m->kkps, b.centre, oct, sf, b.rec, rp, ro, nv);
    HIPCHK(c, hipGetLastError());
    return MO_OK;
}

int view_enqueue(mo_map* m, const int32_t* oct, double sf, const ViewRec** rec, const double** centre) {
    ViewBufs& b = map_feature<ViewBufs>(m);
    if (int rc = view_launch(m, b, oct, sf, false)) return rc;
    *rec = b.rec; *centre = b.centre;
    return MO_OK;
}

extern "C" int mo_map_point_views(mo_map* m, const mo_map_view_params* prm, mo_map_view_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (!(prm->scale_factor > 0.0) || !std::isfinite(prm->scale_factor)) return mo_fail(c, MO_ERR_ARG, "scale_factor must be finite and > 0");
    if (prm->n_levels < 1) return mo_fail(c, MO_ERR_ARG, "n_levels must be >= 1");
    MAP_ENTER(m);
    HostClock clk(c);
    const int n_kf = (int)m->pos_slot.size();
    const size_t np = (size_t)m->n_pts;
    out->n_points = m->n_pts; out->n_kf = n_kf;
    for (size_t i = 0; i < np; i++) {   // (what a map without keyframes reports)
        if (out->normal) out->normal[i * 3] = out->normal[i * 3 + 1] = out->normal[i * 3 + 2] = 0.0f;
        if (out->min_dist) out->min_dist[i] = 0.0f;
        if (out->max_dist) out->max_dist[i] = 0.0f;
        if (out->ref_pos) out->ref_pos[i] = -1;
        if (out->ref_octave) out->ref_octave[i] = 0;
        if (out->n_valid) out->n_valid[i] = 0;
    }
    if (n_kf == 0) return MO_OK;
    int rc;
    if ((rc = map_int32_guard(m)) || (rc = upload_pos_slot(m))) return rc;
    ViewBufs& b = map_feature<ViewBufs>(m);
    mo_stage_begin(c);
    if ((rc = view_launch(m, b, nullptr, prm->scale_factor, true))) return rc;
    mo_stage_mark(c, "view");
    std::vector<ViewRec> rec(np);
    if (out->centre) HIPCHK(c, hipMemcpyAsync(out->centre, b.centre, (size_t)n_kf * 24, hipMemcpyDeviceToHost, c->stream));
    if (np) {
        HIPCHK(c, hipMemcpyAsync(rec.data(), b.rec, np * sizeof(ViewRec), hipMemcpyDeviceToHost, c->stream));
        if (out->ref_pos) HIPCHK(c, hipMemcpyAsync(out->ref_pos, b.ref_pos, np * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->ref_octave) HIPCHK(c, hipMemcpyAsync(out->ref_octave, b.ref_oct, np * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->n_valid) HIPCHK(c, hipMemcpyAsync(out->n_valid, b.n_valid, np * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = map_sync(c, clk))) return rc;
    double top = 1.0;   // scale_factor^(n_levels - 1), trk_scale's products
    for (int l = 0; l < prm->n_levels - 1; l++) top *= prm->scale_factor;
    for (size_t i = 0; i < np; i++) {
        if (out->normal) { out->normal[i * 3] = rec[i].nx; out->normal[i * 3 + 1] = rec[i].ny; out->normal[i * 3 + 2] = rec[i].nz; }
        if (out->max_dist) out->max_dist[i] = rec[i].max_dist;
        if (out->min_dist) out->min_dist[i] = (float)((double)rec[i].max_dist / top);
    }
    return MO_OK;
}
