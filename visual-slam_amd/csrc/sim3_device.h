// sim3_device.h -- what the loop alignment (map_sim3.hip) and the loop confirmation (map_confirm.hip) share on the device, over sim3.h's
// arithmetic: a pair packed from the map, the 13-double model (s, R [9], t [3]) of a result or parameter block, the selection of a
// model's inliers and the refinement rounds of one wave.  Device only; sim3.h itself stays host / device (the host replays
// tests/native/sim3_replay.cpp and confirm_replay.cpp restate these rounds over it and do not include this file).
#pragma once
#include "map_store.h"
#include "sim3.h"

// X = R xyz[i] + t under the pose [R | t] (f64, each row summed left to right)
__device__ __forceinline__ void sim3_camera(const MapView& v, const double* pose12, int i, double* X) {
    double R[9], t[3];
    pose_split(pose12, R, t);
    const float* x = v.src.xyz + (size_t)i * 3;
    for (int d = 0; d < 3; d++) X[d] = R[d * 3] * (double)x[0] + R[d * 3 + 1] * (double)x[1] + R[d * 3 + 2] * (double)x[2] + t[d];
}

// the pair (point a at row i of the keyframe in slot s1 under pose1, point b at row j of the one in slot s2 under pose2): both points
// in their camera frames, both keypoints with their information
__device__ __forceinline__ Sim3Pair sim3_pair_pack(const MapView& v, const mo_keypoint* __restrict__ kkps, double sf, const double* pose1, int s1, int i, int a,
                                                   const double* pose2, int s2, int j, int b) {
    const mo_keypoint k1 = kkps[(size_t)s1 * v.row + i], k2 = kkps[(size_t)s2 * v.row + j];
    Sim3Pair o;
    sim3_camera(v, pose1, a, o.X1);
    sim3_camera(v, pose2, b, o.X2);
    o.x1 = k1.x; o.y1 = k1.y; o.i1 = ba_info(sf, k1.octave);
    o.x2 = k2.x; o.y2 = k2.y; o.i2 = ba_info(sf, k2.octave);
    return o;
}

__device__ __forceinline__ void sim3_model_load(const double* m13, Sim3& S) {
    S.s = m13[0];
    for (int i = 0; i < 9; i++) S.R[i] = m13[1 + i];
    for (int i = 0; i < 3; i++) S.t[i] = m13[10 + i];
}
__device__ __forceinline__ void sim3_model_store(const Sim3& S, double* m13) {
    m13[0] = S.s;
    for (int i = 0; i < 9; i++) m13[1 + i] = S.R[i];
    for (int i = 0; i < 3; i++) m13[10 + i] = S.t[i];
}

// Prm below is the caller's parameter block, of which K and chi2 are read.  (By reference and not as two values: with the values passed
// k_cf_refit came out 7 % slower, profiles/merge_unify_rate.txt.)
// one wave: inlier flags of the m pairs under S into fl (by row of p), their number
template <class Prm>
__device__ __forceinline__ int sim3_select(const Prm& prm, const Sim3& S, const Sim3Pair* __restrict__ pr, const int32_t* __restrict__ rows, int m,
                                           uint8_t* __restrict__ fl) {
    Sim3 I;
    sim3_inverse(S, I);
    int n = 0;
    for (int j = threadIdx.x; j < m; j += 64) {
        double e1, e2;
        const bool in = sim3_inlier(prm.K, S, I, pr[j], prm.chi2, &e1, &e2);
        fl[rows[j]] = in;
        n += in;
    }
    return wave_sum_int(n);
}

// one wave: S's inliers, then (Gauss-Newton over the inliers, re-selection) twice while three of them are left; S refined in place, the
// final flags in fl, their number returned
template <class Prm>
__device__ __forceinline__ int sim3_refine_rounds(const Prm& prm, const Sim3Pair* __restrict__ pr, const int32_t* __restrict__ rows, int m,
                                                  uint8_t* __restrict__ fl, Sim3& S) {
    int n = sim3_select(prm, S, pr, rows, m, fl);
    for (int round = 0; round < 2 && n >= 3; round++) {
        for (int it = 0; it < 10; it++) {
            Sim3 I;
            sim3_inverse(S, I);
            double H[28], g[7];
#pragma unroll
            for (int i = 0; i < 28; i++) H[i] = 0.0;
#pragma unroll
            for (int i = 0; i < 7; i++) g[i] = 0.0;
            for (int j = threadIdx.x; j < m; j += 64) {
                if (!fl[rows[j]]) continue;
                sim3_gn_accumulate(prm.K, S, I, pr[j], prm.chi2, H, g);
            }
#pragma unroll
            for (int i = 0; i < 28; i++) H[i] = wave_sum_all(H[i]);
#pragma unroll
            for (int i = 0; i < 7; i++) g[i] = wave_sum_all(g[i]);
            double step;
            if (!sim3_gn_update(H, g, S, &step) || step < 1e-12) break;
        }
        n = sim3_select(prm, S, pr, rows, m, fl);
    }
    return n;
}
