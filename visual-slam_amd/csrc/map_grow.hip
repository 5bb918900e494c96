// map_grow.hip -- new map points from neighbour keyframes on the device map (mo_map_grow in include/vslam_amd.h): ORB-SLAM2's
// LocalMapping::CreateNewMapPoints / ORBmatcher::SearchForTriangulation on the map as it stands.  Every keypoint of the last keyframe
// that no map point observes is searched along its epipolar line among the unobserved keypoints of the neighbour keyframes; the
// matches a row wins are triangulated from the pair with the most parallax, gated, and appended to the live copy of the store.
//
// Chain (one synchronisation, the copy-out, into pinned buffers like the upload; the pair geometry - F, epipole, poses per neighbour -
// is formed on the host from the poses the caller passes and uploaded before the first kernel; every kernel behind k_grow_free reads n_free first, the append n_new):
//   k_point_of      one thread per point: the owners of the rows of the target and the neighbours (map_launch_point_of, map_kernels.hip)
//   k_grow_free     one block: the free rows of the target next to each other, in row order (block scan)
//   k_grow_search   one wave per (tile of 64 free target rows, neighbour): the neighbour's free keypoints staged in LDS (x, y and the two
//                   octave-scaled thresholds, in tiles of GR_TILE rows), each lane's epipolar line in registers against the tile;
//                   descriptors are read only for the rows behind both gates; the accepted row is claimed by a 64-bit atomicMin of
//                   (dist << 32) | row1
//   k_grow_points   one thread per free target row: the won matches, base pair, Cholesky, gates, further observations
//   map_scan_excl x 2 + k_grow_append   new indices and observation offsets; every field of every new point
// What bounds the search: free target rows x free neighbour rows x neighbours gate tests, each an LDS broadcast read of 36 bytes and
// about 15 f64 operations, one division among them.  A keyframe of 2000 rows and 10 neighbours are 4 * 10^7 tests in 320 waves: they
// do not fill the chip, all run at once, and the kernel takes as long as ONE wave's walk over its neighbour's rows (0.62 ms measured,
// 0.3 us per staged row; with 50 free target rows left it still takes 0.36 ms).  Latency of the dependent LDS reads and the division
// per row, not throughput and not memory: splitting a neighbour's rows over several waves would shorten it and was not tried.
// Integer atomics only (minima and sums): equal maps give equal bytes.  -ffp-contract=off (Makefile): every expression rounds like
// tests/grow_restatement.py.
#include <climits>
#include <cmath>
#include <vector>

#include "common.h"
#include "map_rebuild.h"   // (map_store.h with it)
#include "map_search.h"
#include "ba.h"   // ba_info

#define GR_BLOCK 256
#define GR_WAVE 64             // block of the search: one wave
#define GR_TILE 1024           // neighbour rows staged at a time (36 KB of LDS)
#define GR_MAX_NB 16384        // grid.y of the search

// a keyframe as the kernels need it: [R | t], its centre, slot and position
struct GrowCam {
    double R[9], t[3], C[3];
    int32_t slot, pos;
};
// a neighbour: its camera and what the search reads
struct GrowPair {
    GrowCam cam;
    double F[9], ex, ey;
};

struct GrowPrm {
    double fx, fy, cx, cy;
    double sf, epi_chi2, chi2, cos_max, ratio_factor, epipole_r2;
    int max_dist, n_nb, row;
    GrowCam tgt;
};

struct GrowRes {
    unsigned long long n_epi;
    int32_t n_free, n_accepted, n_matches, n_new, n_obs_new, pad;
};

struct GrowBufs : MapFeature {
    PinnedBuf<GrowPair> h_pairs;          // [neighbour] as formed on the host
    DevBuf<GrowPair> pairs;               // [neighbour]
    DevBuf<int32_t> tab;                  // [neighbour .. target][row] point_of (INT_MAX: a free row)
    DevBuf<int32_t> frow;                 // [n_free] the free rows of the target
    DevBuf<unsigned long long> key;       // [neighbour][row] (dist << 32) | row1 of the claim on each row
    DevBuf<int32_t> prop;                 // [neighbour][free index] the row the pair proposed, then: the row it observes (-1: none)
    DevBuf<double> X;                     // [free index][3]
    DevBuf<double> outX;                  // [n_new][3]
    DevBuf<int32_t> point;                // [row] the new point of each target row
    PinnedBuf<int32_t> h_point; PinnedBuf<double> h_X;   // the copy-out
    ResBlock<GrowRes> res;
    // all of it is scratch: every call's chain writes what it reads (a DevBuf added above is named here, or kept out with a reason)
    template <class F> void each_scratch(F f) { f(pairs); f(tab); f(frow); f(key); f(prop); f(X); f(outX); f(point); f(res); }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// ---- host: the geometry of the pairs, in the header's operation order ---------------------------------------------------------------
static GrowCam grow_cam(const double* T, int slot, int pos) {
    GrowCam c;
    pose_split(T, c.R, c.t);
    for (int i = 0; i < 3; i++) c.C[i] = -(c.R[i] * c.t[0] + c.R[3 + i] * c.t[1] + c.R[6 + i] * c.t[2]);
    c.slot = slot; c.pos = pos;
    return c;
}

static void grow_pair(const GrowPrm& p, GrowPair* q) {
    const double* R1 = p.tgt.R; const double* t1 = p.tgt.t; const double* R2 = q->cam.R; const double* t2 = q->cam.t;
    double R12[9], t12[3], E[9], G[9], c2[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R12[i * 3 + j] = R1[i * 3] * R2[j * 3] + R1[i * 3 + 1] * R2[j * 3 + 1] + R1[i * 3 + 2] * R2[j * 3 + 2];
    for (int i = 0; i < 3; i++) t12[i] = t1[i] - (R12[i * 3] * t2[0] + R12[i * 3 + 1] * t2[1] + R12[i * 3 + 2] * t2[2]);
    for (int j = 0; j < 3; j++) {
        E[j] = t12[1] * R12[6 + j] - t12[2] * R12[3 + j];
        E[3 + j] = t12[2] * R12[j] - t12[0] * R12[6 + j];
        E[6 + j] = t12[0] * R12[3 + j] - t12[1] * R12[j];
    }
    const double ifx = 1.0 / p.fx, ify = 1.0 / p.fy;
    for (int i = 0; i < 3; i++) {
        G[i * 3] = E[i * 3] * ifx;
        G[i * 3 + 1] = E[i * 3 + 1] * ify;
        G[i * 3 + 2] = (E[i * 3 + 2] - G[i * 3] * p.cx) - G[i * 3 + 1] * p.cy;
    }
    for (int j = 0; j < 3; j++) {
        q->F[j] = G[j] * ifx;
        q->F[3 + j] = G[3 + j] * ify;
        q->F[6 + j] = (G[6 + j] - q->F[j] * p.cx) - q->F[3 + j] * p.cy;
    }
    const double* C1 = p.tgt.C;
    for (int i = 0; i < 3; i++) c2[i] = R2[i * 3] * C1[0] + R2[i * 3 + 1] * C1[1] + R2[i * 3 + 2] * C1[2] + t2[i];
    q->ex = (p.fx * c2[0]) / c2[2] + p.cx;
    q->ey = (p.fy * c2[1]) / c2[2] + p.cy;
}

// ---- device ---------------------------------------------------------------------------------------------------------------------------
// one block: the free rows of the target in row order
__global__ __launch_bounds__(1024) void k_grow_free(const int32_t* __restrict__ ttab, int n_rows, int32_t* __restrict__ frow, GrowRes* __restrict__ res) {
    __shared__ int lw[40];
    int n = 0;
    for (int b = 0; b < n_rows; b += 1024) {
        const int r = b + threadIdx.x;
        const int take = r < n_rows && ttab[r] == INT_MAX ? 1 : 0;
        int t;
        const int e = block_excl_scan(take, lw, &t);
        if (take) frow[n + e] = r;
        n += t;
    }
    if (threadIdx.x == 0) res->n_free = n;
}

// one wave per (tile of free target rows, neighbour)
__global__ __launch_bounds__(GR_WAVE) void k_grow_search(GrowPrm prm, const GrowPair* __restrict__ pairs, const mo_keypoint* __restrict__ kkps,
                                                          const uint8_t* __restrict__ kdesc, const int32_t* __restrict__ kcnt, const int32_t* __restrict__ tab,
                                                          const int32_t* __restrict__ frow, unsigned long long* __restrict__ key, int32_t* __restrict__ prop,
                                                          GrowRes* __restrict__ res) {
    __shared__ double lx[GR_TILE], ly[GR_TILE], lzone[GR_TILE], lepi[GR_TILE];
    __shared__ int lrow[GR_TILE];
    __shared__ int ln;
    const int n_free = res->n_free;
    const int f = blockIdx.x * GR_WAVE + threadIdx.x, nb = blockIdx.y;
    if (blockIdx.x * GR_WAVE >= n_free) return;
    const GrowPair& pr = pairs[nb];
    const int slot2 = pr.cam.slot, n2 = kcnt[slot2];
    const mo_keypoint* __restrict__ k2 = kkps + (size_t)slot2 * prm.row;
    const uint8_t* __restrict__ d2 = kdesc + (size_t)slot2 * prm.row * 32;
    const int32_t* __restrict__ tab2 = tab + (size_t)nb * prm.row;
    const bool live = f < n_free;
    const int row1 = live ? frow[f] : 0;
    const size_t e1 = (size_t)prm.tgt.slot * prm.row + row1;
    const mo_keypoint kp1 = kkps[e1];
    const double x1 = (double)kp1.x, y1 = (double)kp1.y;
    const double a = x1 * pr.F[0] + y1 * pr.F[3] + pr.F[6], b = x1 * pr.F[1] + y1 * pr.F[4] + pr.F[7], c = x1 * pr.F[2] + y1 * pr.F[5] + pr.F[8];
    const double den = a * a + b * b;
    const bool line = live && !(den == 0.0);
    const double ex = pr.ex, ey = pr.ey;
    const uint8_t* dsc1 = kdesc + e1 * 32;
    int bd = INT_MAX, bq = INT_MAX;
    unsigned long long n_epi = 0;
    for (int t0 = 0; t0 < n2; t0 += GR_TILE) {
        if (threadIdx.x == 0) ln = 0;
        __syncthreads();
        const int t1 = min(t0 + GR_TILE, n2);
        for (int r = t0 + threadIdx.x; r < t1; r += GR_WAVE) {
            if (tab2[r] != INT_MAX) continue;
            const mo_keypoint kp = k2[r];
            const int at = atomicAdd(&ln, 1);   // (arrival order: the best row is the lowest (dist, row) whatever the order)
            lx[at] = (double)kp.x; ly[at] = (double)kp.y; lrow[at] = r;
            lzone[at] = prm.epipole_r2 * trk_scale(prm.sf, kp.octave);
            lepi[at] = prm.epi_chi2 * trk_scale(prm.sf * prm.sf, kp.octave);
        }
        __syncthreads();
        const int n = ln;
        if (line)
            for (int j = 0; j < n; j++) {
                const double x2 = lx[j], y2 = ly[j];
                const double dx = ex - x2, dy = ey - y2;
                if (dx * dx + dy * dy < lzone[j]) continue;
                const double num = a * x2 + b * y2 + c;
                if (!((num * num) / den < lepi[j])) continue;
                n_epi++;
                const int q = lrow[j];
                const int dist = trk_ham(dsc1, d2 + (size_t)q * 32);
                trk_take(dist, q, bd, bq);
            }
        __syncthreads();
    }
    const bool acc = bd != INT_MAX && bd <= prm.max_dist;
    if (acc) atomicMin(key + (size_t)nb * prm.row + bq, ((unsigned long long)(unsigned)bd << 32) | (unsigned)row1);
    if (live) prop[(size_t)nb * prm.row + f] = acc ? bq : -1;
    for (int o = 32; o; o >>= 1) n_epi += __shfl_down(n_epi, o, 64);
    if (threadIdx.x == 0 && n_epi) atomicAdd(&res->n_epi, n_epi);
    wave_count_add(acc, &res->n_accepted);
}

__device__ __forceinline__ void grow_cam_point(const GrowCam& c, const double* X, double* Xc) {
    for (int i = 0; i < 3; i++) Xc[i] = c.R[i * 3] * X[0] + c.R[i * 3 + 1] * X[1] + c.R[i * 3 + 2] * X[2] + c.t[i];
}

// depth > 0 and the reprojection gate of X in one view
__device__ __forceinline__ bool grow_seen(const GrowPrm& p, const GrowCam& c, const double* X, double x, double y, int octave) {
    double Xc[3];
    grow_cam_point(c, X, Xc);
    if (!(Xc[2] > 0.0)) return false;
    const double u = (p.fx * Xc[0]) / Xc[2] + p.cx, v = (p.fy * Xc[1]) / Xc[2] + p.cy;
    const double du = u - x, dv = v - y;
    return ba_info(p.sf, octave) * (du * du + dv * dv) <= p.chi2;
}

__device__ __forceinline__ void grow_ray(const GrowCam& c, double xn, double yn, double* r) {
    for (int i = 0; i < 3; i++) r[i] = c.R[i] * xn + c.R[3 + i] * yn + c.R[6 + i];
}

__device__ __forceinline__ double grow_dist(const double* X, const double* C) {
    const double dx = X[0] - C[0], dy = X[1] - C[1], dz = X[2] - C[2];
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// the two-view point of the header: false when a radicand is not > 0
__device__ __forceinline__ bool grow_triangulate(const GrowCam& c1, double xn1, double yn1, const GrowCam& c2, double xn2, double yn2, double* X) {
    double A[4][3], a4[4];
    const double xs[4] = {xn1, yn1, xn2, yn2};
    for (int r = 0; r < 4; r++) {
        const GrowCam& c = r < 2 ? c1 : c2;
        const int w = r & 1;
        for (int j = 0; j < 3; j++) A[r][j] = xs[r] * c.R[6 + j] - c.R[w * 3 + j];
        a4[r] = xs[r] * c.t[2] - c.t[w];
    }
    double N[3][3], g[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j <= i; j++) N[i][j] = A[0][i] * A[0][j] + A[1][i] * A[1][j] + A[2][i] * A[2][j] + A[3][i] * A[3][j];
        g[i] = -(A[0][i] * a4[0] + A[1][i] * a4[1] + A[2][i] * a4[2] + A[3][i] * a4[3]);
    }
    if (!(N[0][0] > 0.0)) return false;
    const double l00 = sqrt(N[0][0]), l10 = N[1][0] / l00, l20 = N[2][0] / l00;
    const double p1 = N[1][1] - l10 * l10;
    if (!(p1 > 0.0)) return false;
    const double l11 = sqrt(p1), l21 = (N[2][1] - l20 * l10) / l11;
    const double p2 = (N[2][2] - l20 * l20) - l21 * l21;
    if (!(p2 > 0.0)) return false;
    const double l22 = sqrt(p2);
    const double y0 = g[0] / l00, y1 = (g[1] - l10 * y0) / l11, y2 = ((g[2] - l20 * y0) - l21 * y1) / l22;
    X[2] = y2 / l22;
    X[1] = (y1 - l21 * X[2]) / l11;
    X[0] = ((y0 - l10 * X[1]) - l20 * X[2]) / l00;
    return true;
}

// one thread per free target row: its point, if any.  prop [nb][f] becomes the row of the observation the point keeps at nb (-1: none)
__global__ __launch_bounds__(GR_BLOCK) void k_grow_points(GrowPrm prm, const GrowPair* __restrict__ pairs, const mo_keypoint* __restrict__ kkps,
                                                           const int32_t* __restrict__ frow, const unsigned long long* __restrict__ key,
                                                           int32_t* __restrict__ prop, double* __restrict__ Xo,
                                                           int32_t* __restrict__ isnew, int32_t* __restrict__ nobs, GrowRes* __restrict__ res) {
    const int f = blockIdx.x * GR_BLOCK + threadIdx.x;
    const int n_free = res->n_free;
    int won = 0, kept = 0;
    if (f < prm.row) { isnew[f] = 0; nobs[f] = 0; }   // (the scans run over every row of the stride)
    if (f < n_free) {
        const int row1 = frow[f];
        const mo_keypoint kp1 = kkps[(size_t)prm.tgt.slot * prm.row + row1];
        const double x1 = (double)kp1.x, y1 = (double)kp1.y;
        const double xn1 = (x1 - prm.cx) / prm.fx, yn1 = (y1 - prm.cy) / prm.fy;
        double r1[3];
        grow_ray(prm.tgt, xn1, yn1, r1);
        const double n1 = sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2]);
        int bk = -1;
        double bcos = 0.0;
        for (int k = 0; k < prm.n_nb; k++) {
            const size_t e = (size_t)k * prm.row + f;
            const int q = prop[e];
            if (q < 0) continue;
            if ((int)(key[(size_t)k * prm.row + q] & 0xffffffffu) != row1) { prop[e] = -1; continue; }
            won++;
            const GrowCam& c2 = pairs[k].cam;
            const mo_keypoint kp2 = kkps[(size_t)c2.slot * prm.row + q];
            double r2[3];
            grow_ray(c2, ((double)kp2.x - prm.cx) / prm.fx, ((double)kp2.y - prm.cy) / prm.fy, r2);
            const double n2 = sqrt(r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2]);
            const double cosp = (r1[0] * r2[0] + r1[1] * r2[1] + r1[2] * r2[2]) / (n1 * n2);
            if (cosp > 0.0 && cosp < prm.cos_max && (bk < 0 || cosp < bcos)) { bk = k; bcos = cosp; }
        }
        double X[3] = {0.0, 0.0, 0.0};
        bool ok = bk >= 0;
        if (ok) {
            const GrowCam& c2 = pairs[bk].cam;
            const mo_keypoint kp2 = kkps[(size_t)c2.slot * prm.row + prop[(size_t)bk * prm.row + f]];
            const double x2 = (double)kp2.x, y2 = (double)kp2.y;
            ok = grow_triangulate(prm.tgt, xn1, yn1, c2, (x2 - prm.cx) / prm.fx, (y2 - prm.cy) / prm.fy, X);
            ok = ok && grow_seen(prm, prm.tgt, X, x1, y1, kp1.octave) && grow_seen(prm, c2, X, x2, y2, kp2.octave);
            if (ok) {
                const double d1 = grow_dist(X, prm.tgt.C), d2 = grow_dist(X, c2.C);
                ok = d1 > 0.0 && d2 > 0.0;
                if (ok) {
                    const double rd = d2 / d1, ro = trk_scale(prm.sf, kp1.octave) / trk_scale(prm.sf, kp2.octave);
                    ok = !(rd * prm.ratio_factor < ro || rd > ro * prm.ratio_factor);
                }
            }
        }
        if (ok) {
            kept = 1;   // (the target's own observation)
            for (int k = 0; k < prm.n_nb; k++) {
                const size_t e = (size_t)k * prm.row + f;
                const int q = prop[e];
                if (q < 0) continue;
                if (k != bk) {
                    const GrowCam& c2 = pairs[k].cam;
                    const mo_keypoint kp2 = kkps[(size_t)c2.slot * prm.row + q];
                    if (!grow_seen(prm, c2, X, (double)kp2.x, (double)kp2.y, kp2.octave)) { prop[e] = -1; continue; }
                }
                kept++;
            }
            Xo[(size_t)f * 3] = X[0]; Xo[(size_t)f * 3 + 1] = X[1]; Xo[(size_t)f * 3 + 2] = X[2];
            isnew[f] = 1; nobs[f] = kept;
        }
    }
    won = wave_sum_int(won);
    if ((threadIdx.x & 63) == 0 && won) atomicAdd(&res->n_matches, won);
}

// one thread per free target row: every field of its new point behind the map's points, in row order
__global__ __launch_bounds__(GR_BLOCK) void k_grow_append(GrowPrm prm, const GrowPair* __restrict__ pairs, const mo_keypoint* __restrict__ kkps,
                                                           const int32_t* __restrict__ frow, const int32_t* __restrict__ prop, const double* __restrict__ Xo,
                                                           const int32_t* __restrict__ isnew, const int32_t* __restrict__ rank, const int32_t* __restrict__ obase,
                                                           const uint8_t* __restrict__ img, int w, int h, int ch, int n0, int o0, int born, int tgt_ord, MapPts dst,
                                                           double* __restrict__ outX, int32_t* __restrict__ point, int32_t* __restrict__ st,
                                                           const GrowRes* __restrict__ res) {
    const int n_new = res->n_new;
    if (!n_new) return;
    const int f = blockIdx.x * GR_BLOCK + threadIdx.x;
    if (f == 0) map_store_end(dst, st, n0 + n_new, o0 + res->n_obs_new);
    if (f >= res->n_free || !isnew[f]) return;
    const int row1 = frow[f], r = rank[f], i = n0 + r;
    for (int k = 0; k < 3; k++) { const double v = Xo[(size_t)f * 3 + k]; dst.xyz[(size_t)i * 3 + k] = (float)v; outX[(size_t)r * 3 + k] = v; }
    const mo_keypoint kp = kkps[(size_t)prm.tgt.slot * prm.row + row1];
    const int x = (int)kp.x, y = (int)kp.y;   // Python's int(): truncation toward zero
    uint8_t c0 = 0, c1 = 0, c2 = 255;
    if (x >= 0 && x < w && y >= 0 && y < h) {
        const uint8_t* px = img + ((size_t)y * w + x) * ch;
        c0 = px[0]; c1 = ch == 3 ? px[1] : px[0]; c2 = ch == 3 ? px[2] : px[0];
    }
    dst.col[(size_t)i * 3] = c0; dst.col[(size_t)i * 3 + 1] = c1; dst.col[(size_t)i * 3 + 2] = c2;
    dst.id[i] = i;
    dst.dkf[i] = tgt_ord; dst.drow[i] = row1;   // (the target's ordinal: its slot, except on an imported map)
    map_life_new(dst, i, born);
    int o = o0 + obase[f];
    dst.off[i] = o;
    for (int k = 0; k < prm.n_nb; k++) {
        const int q = prop[(size_t)k * prm.row + f];
        if (q < 0) continue;
        dst.okf[o] = pairs[k].cam.pos; dst.okp[o] = q; o++;
    }
    dst.okf[o] = prm.tgt.pos; dst.okp[o] = row1;
    point[row1] = i;
}

extern "C" int mo_map_grow(mo_map* m, const double* K, const double* poses, const mo_map_grow_params* prm, mo_map_grow_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!K || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (prm->window < 0) return mo_fail(c, MO_ERR_ARG, "window must be >= 0");
    if (!(prm->scale_factor > 0.0) || !std::isfinite(prm->scale_factor)) return mo_fail(c, MO_ERR_ARG, "scale_factor must be finite and > 0");
    if (!(prm->epi_chi2 >= 0.0) || !(prm->chi2 >= 0.0) || !(prm->epipole_r2 >= 0.0) || !(prm->ratio_factor > 0.0))
        return mo_fail(c, MO_ERR_ARG, "epi_chi2, chi2 and epipole_r2 must be >= 0, ratio_factor > 0");
    if (!(K[0] != 0.0) || !(K[4] != 0.0)) return mo_fail(c, MO_ERR_ARG, "K: focal lengths must not be 0");
    MAP_ENTER(m);
    HostClock clk(c);
    out->n_neighbours = out->n_free = out->n_accepted = out->n_matches = out->n_new = out->n_obs_new = 0;
    out->n_epi = 0;
    out->n_points = m->n_pts; out->n_obs = m->n_obs;
    const int n_kf = (int)m->pos_slot.size();
    const int tslot = n_kf ? m->pos_slot[n_kf - 1] : 0, n_rows = n_kf ? m->h_kcnt[tslot] : 0;
    if (out->point) for (int r = 0; r < n_rows; r++) out->point[r] = -1;
    if (n_kf < 2) return MO_OK;   // (no neighbour: not an error)
    if (!poses) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const int T = n_kf - 1;
    const int lo_pos = map_window_lo(prm->window, T);
    const int nb = T - lo_pos, row = m->row;
    out->n_neighbours = nb;
    if (n_rows == 0) return MO_OK;
    if (nb > GR_MAX_NB) return mo_fail(c, MO_ERR_UNSUPPORTED, "more neighbour keyframes than one call searches (16384)");
    const size_t np = (size_t)m->n_pts, bound_obs = (size_t)n_rows * ((size_t)nb + 1);
    if (np + (size_t)n_rows > (size_t)(INT32_MAX / 2) || (size_t)m->n_obs + bound_obs > (size_t)(INT32_MAX / 2) || ((size_t)nb + 1) * row > (size_t)INT32_MAX)
        return mo_fail(c, MO_ERR_CAPACITY, "map larger than int32 indexing");
    GrowBufs& b = map_feature<GrowBufs>(m);
    int rc;
    const size_t nrow = (size_t)nb * row, trow = nrow + row;
    if ((rc = mo_reserve(c, b.pairs, (size_t)nb, b.tab, trow, b.frow, (size_t)row, b.key, nrow, b.prop, nrow, b.X, (size_t)row * 3, b.outX, (size_t)row * 3,
                         b.point, (size_t)row, b.res, b.h_pairs, (size_t)nb, m->keep, (size_t)row, m->kobs, (size_t)row, m->rank, (size_t)row,
                         m->obase, (size_t)row)) ||
        (out->point && (rc = mo_reserve(c, b.h_point, (size_t)row))) || (out->points && (rc = mo_reserve(c, b.h_X, (size_t)row * 3))))
        return rc;
    // capacity for a point per free target row (bounded by the target's rows) with an observation in every keyframe of the call
    if ((rc = map_pts_reserve(m, m->cur, np + (size_t)n_rows, (size_t)m->n_obs + bound_obs, true)) || (rc = upload_pos_slot(m))) return rc;
    GrowPrm p;
    p.fx = K[0]; p.fy = K[4]; p.cx = K[2]; p.cy = K[5];
    p.sf = prm->scale_factor; p.epi_chi2 = prm->epi_chi2; p.chi2 = prm->chi2; p.cos_max = prm->cos_max; p.ratio_factor = prm->ratio_factor;
    p.epipole_r2 = prm->epipole_r2;
    p.max_dist = prm->max_dist; p.n_nb = nb; p.row = row;
    p.tgt = grow_cam(poses + (size_t)T * 12, tslot, T);
    for (int k = 0; k < nb; k++) {
        b.h_pairs.p[k].cam = grow_cam(poses + (size_t)(lo_pos + k) * 12, m->pos_slot[lo_pos + k], lo_pos + k);
        grow_pair(p, b.h_pairs.p + k);
    }
    mo_stage_begin(c);
    HIPCHK(c, hipMemcpyAsync(b.pairs, b.h_pairs.p, (size_t)nb * sizeof(GrowPair), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(b.res, 0, sizeof(GrowRes), c->stream));
    HIPCHK(c, hipMemsetAsync(b.key, 0xff, nrow * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(b.point, 0xff, (size_t)row * 4, c->stream));
    const MapPts dst = m->P[m->cur].view();
    if ((rc = map_launch_point_of(m, lo_pos, nb + 1, b.tab))) return rc;
    hipLaunchKernelGGL(k_grow_free, dim3(1), dim3(1024), 0, c->stream, b.tab + nrow, n_rows, b.frow, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "grow_prep");
    const unsigned rblocks = (unsigned)((row + GR_BLOCK - 1) / GR_BLOCK);
    hipLaunchKernelGGL(k_grow_search, dim3((unsigned)((n_rows + GR_WAVE - 1) / GR_WAVE), (unsigned)nb), dim3(GR_WAVE), 0, c->stream, p, b.pairs, m->kkps, m->kdesc,
                       m->kcnt, b.tab, b.frow, b.key, b.prop, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "grow_search");
    hipLaunchKernelGGL(k_grow_points, dim3(rblocks), dim3(GR_BLOCK), 0, c->stream, p, b.pairs, m->kkps, b.frow, b.key, b.prop, b.X, m->keep, m->kobs, b.res);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, m->keep, m->rank, row, &b.res.p->n_new)) || (rc = map_scan_excl(m, m->kobs, m->obase, row, &b.res.p->n_obs_new))) return rc;
    const int ib = m->img_cur;   // the target's image
    const bool has_img = m->img[ib] && m->img_w[ib] > 0;
    hipLaunchKernelGGL(k_grow_append, dim3(rblocks), dim3(GR_BLOCK), 0, c->stream, p, b.pairs, m->kkps, b.frow, b.prop, b.X, m->keep, m->rank, m->obase,
                       has_img ? m->img[ib].p : m->kdesc.p, has_img ? m->img_w[ib] : 0, has_img ? m->img_h[ib] : 0, has_img ? m->img_ch[ib] : 1, (int)np,
                       (int)m->n_obs, map_now(m), n_kf ? m->slot_ord[tslot] : 0, dst, b.outX, b.point, m->st, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "grow_points");
    if ((rc = b.res.download(c))) return rc;
    if (out->point) {
        HIPCHK(c, hipMemcpyAsync(b.h_point.p, b.point, (size_t)n_rows * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if (out->points) {
        HIPCHK(c, hipMemcpyAsync(b.h_X.p, b.outX, (size_t)n_rows * 24, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = map_sync(c, clk))) return rc;
    const GrowRes& r = b.res.host();
    out->n_free = r.n_free; out->n_epi = (int64_t)r.n_epi; out->n_accepted = r.n_accepted; out->n_matches = r.n_matches;
    if (!r.n_new) return MO_OK;   // (nothing was written)
    out->n_new = r.n_new; out->n_obs_new = r.n_obs_new;
    if (out->point) std::copy(b.h_point.p, b.h_point.p + n_rows, out->point);
    if (out->points) std::copy(b.h_X.p, b.h_X.p + (size_t)r.n_new * 3, out->points);
    m->n_pts += r.n_new; m->n_obs += r.n_obs_new;
    m->id_bound = std::max<int64_t>(m->id_bound, m->n_pts);
    out->n_points = m->n_pts; out->n_obs = m->n_obs;
    return MO_OK;
}
