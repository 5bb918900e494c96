// Homography model of the two-view initialisation, shared by the kernels of twoview_h.hip and the CPU test of the header
// (tests/native/homography_check.cpp): ORB-SLAM2's Initializer computes a homography beside the fundamental matrix, scores both
// (CheckHomography / CheckFundamental), picks one by RH = SH / (SH + SF) and, for the homography, recovers the motion after Faugeras
// (ReconstructH) with a per-candidate triangulation test (CheckRT).  Everything is f64 with sqrt and fabs only; built with
// -ffp-contract=off on both sides, so a host build computes what the device computes.
//
// Conventions: pixels p = (u, v); a homography H maps image 1 to image 2, x2 ~ H x1 (ORB-SLAM2's H21); F satisfies x2' F x1 = 0;
// pose X2 = R X1 + t; K is read as fx, fy, cx, cy (K[0], K[4], K[2], K[5]) like the essential path.  Matrices are row-major.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define HG_HD __host__ __device__ __forceinline__
#else
#define HG_HD inline
#endif

#define HG_CHI2_H 5.991      // chi-square, 2 degrees of freedom, 95 %: both directions of the symmetric transfer error
#define HG_CHI2_F 3.841      // chi-square, 1 degree of freedom: distance to the epipolar line (the score offset stays HG_CHI2_H)
#define HG_COS_GOOD 0.99998  // CheckRT: a point with less parallax than this is kept out of the map and exempt from the depth test
#define HG_COLLINEAR2 1e-12  // a 4-sample with |det(a, b, c)| <= 1e-6 |a| |b| |c| for three of its points gives no model (squared)

// ---- sampling: the first four indices of the two-view stage's sample8 stream (seed, global pair index, h) ------------------------
// sample8 draws c = splitmix64 % m and redraws while c repeats an EARLIER index, so its first four indices do not depend on the
// later four: drawing four is drawing the prefix (pnp_sample<3> follows the same convention).  m >= 4.
HG_HD uint64_t hg_splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
HG_HD uint64_t hg_stream_seed(uint64_t seed, uint64_t pair) { return seed + pair * 0x632BE59BD9B4E019ull; }
HG_HD void hg_sample4(uint64_t seed, int h, int m, int (&idx)[4]) {
    uint64_t s = seed + (uint64_t)(h + 1) * 0xD1B54A32D192ED03ull;
    for (int k = 0; k < 4; k++) {
        int c;
        bool dup;
        do {
            c = (int)(hg_splitmix64(s) % (uint64_t)m);
            dup = false;
            for (int j = 0; j < k; j++) dup |= idx[j] == c;
        } while (dup);
        idx[k] = c;
    }
}

// ---- Hartley normalisation of ONE image: x_n = s (x - c), mean distance from the centroid -> sqrt 2 -------------------------------
// nm = {s, cx, cy}.  (The fundamental model of twoview_kernels.hip shares one scale between the images; ORB-SLAM2 normalises each
// image on its own, and a homography needs no common scale.)  sum_x, sum_y: coordinate sums; then sum_d: sum of distances.
HG_HD void hg_norm_centroid(double sum_x, double sum_y, int m, double* nm) { nm[1] = sum_x / (double)m; nm[2] = sum_y / (double)m; }
HG_HD double hg_norm_dist(double x, double y, const double* nm) { const double a = x - nm[1], b = y - nm[2]; return sqrt(a * a + b * b); }
HG_HD void hg_norm_scale(double sum_d, int m, double* nm) {
    const double mean = sum_d / (double)m;
    nm[0] = mean > 1e-12 ? 1.4142135623730951 / mean : 1.0;
}
// H in pixels from Hn in normalised coordinates: H = T2^-1 Hn T1 with T = [s 0 -s cx; 0 s -s cy; 0 0 1]
HG_HD void hg_denormalise(const double* Hn, const double* n1, const double* n2, double* H) {
    double A[9];
    for (int i = 0; i < 3; i++) {  // A = Hn T1
        A[i * 3] = Hn[i * 3] * n1[0];
        A[i * 3 + 1] = Hn[i * 3 + 1] * n1[0];
        A[i * 3 + 2] = Hn[i * 3 + 2] - n1[0] * (Hn[i * 3] * n1[1] + Hn[i * 3 + 1] * n1[2]);
    }
    const double is = 1.0 / n2[0];
    for (int j = 0; j < 3; j++) {  // T2^-1 = [1/s 0 cx; 0 1/s cy; 0 0 1]
        H[j] = A[j] * is + n2[1] * A[6 + j];
        H[3 + j] = A[3 + j] * is + n2[2] * A[6 + j];
        H[6 + j] = A[6 + j];
    }
}

// ---- small 3x3 helpers ------------------------------------------------------------------------------------------------------------
HG_HD void hg_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
HG_HD double hg_det3(const double* M) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
// adjugate (the inverse times the determinant): a homography's inverse direction needs no division
HG_HD void hg_adj3(const double* M, double* A) {
    A[0] = M[4] * M[8] - M[5] * M[7]; A[1] = M[2] * M[7] - M[1] * M[8]; A[2] = M[1] * M[5] - M[2] * M[4];
    A[3] = M[5] * M[6] - M[3] * M[8]; A[4] = M[0] * M[8] - M[2] * M[6]; A[5] = M[2] * M[3] - M[0] * M[5];
    A[6] = M[3] * M[7] - M[4] * M[6]; A[7] = M[1] * M[6] - M[0] * M[7]; A[8] = M[0] * M[4] - M[1] * M[3];
}
HG_HD void hg_mul3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
HG_HD bool hg_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN and the infinities

// ---- four-point homography in closed form ----------------------------------------------------------------------------------------
// det of the homogeneous points (a, 1), (b, 1), (c, 1), and whether it is away from 0 relative to their lengths
HG_HD double hg_det_pts(const double* a, const double* b, const double* c) {
    return a[0] * (b[1] - c[1]) - a[1] * (b[0] - c[0]) + (b[0] * c[1] - b[1] * c[0]);
}
HG_HD bool hg_spans(double det, const double* a, const double* b, const double* c) {
    const double na = a[0] * a[0] + a[1] * a[1] + 1.0, nb = b[0] * b[0] + b[1] * b[1] + 1.0, nc = c[0] * c[0] + c[1] * c[1] + 1.0;
    return det * det > HG_COLLINEAR2 * (na * nb * nc);  // (false for a NaN)
}
// The projective basis of a quadruple: B = [l0 a, l1 b, l2 c] maps e0, e1, e2 to a, b, c and (1, 1, 1) to d, with l = adj([a b c]) d:
// by Cramer's rule the three minors det(d, b, c), det(a, d, c), det(a, b, d).  False when three of the four points are (nearly)
// collinear or coincide, or a coordinate is not finite.
HG_HD bool hg_basis(const double* a, const double* b, const double* c, const double* d, double* B) {
    const double l0 = hg_det_pts(d, b, c), l1 = hg_det_pts(a, d, c), l2 = hg_det_pts(a, b, d), dd = hg_det_pts(a, b, c);
    if (!(hg_spans(l0, d, b, c) && hg_spans(l1, a, d, c) && hg_spans(l2, a, b, d) && hg_spans(dd, a, b, c))) return false;
    B[0] = l0 * a[0]; B[1] = l1 * b[0]; B[2] = l2 * c[0];
    B[3] = l0 * a[1]; B[4] = l1 * b[1]; B[5] = l2 * c[1];
    B[6] = l0;        B[7] = l1;        B[8] = l2;
    return true;
}
// pts: [4][4] = x1, y1, x2, y2 of the four correspondences.  H = B2 adj(B1), scaled to unit Frobenius norm: no factorisation, no
// iteration.  False = no model.
HG_HD bool hg_homography4(const double* pts, double* H) {
    double B1[9], B2[9], A1[9];
    const double *p0 = pts, *p1 = pts + 4, *p2 = pts + 8, *p3 = pts + 12;
    if (!hg_basis(p0, p1, p2, p3, B1) || !hg_basis(p0 + 2, p1 + 2, p2 + 2, p3 + 2, B2)) return false;
    hg_adj3(B1, A1);
    hg_mul3(B2, A1, H);
    double nn = 0.0;
    for (int j = 0; j < 9; j++) nn += H[j] * H[j];
    if (!(nn > 0.0) || !hg_finite(nn)) return false;
    const double r = 1.0 / sqrt(nn);
    for (int j = 0; j < 9; j++) H[j] *= r;
    return true;
}

// ---- scores -----------------------------------------------------------------------------------------------------------------------
// CheckHomography for one correspondence: squared transfer errors over sigma^2, image 1 (x2 through H12 = adj(H21)) and image 2
HG_HD void hg_transfer_chi(const double* H21, const double* H12, double u1, double v1, double u2, double v2, double inv_s2, double* c1, double* c2) {
    const double w1 = 1.0 / (H12[6] * u2 + H12[7] * v2 + H12[8]);
    const double a1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w1, b1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w1;
    *c1 = ((u1 - a1) * (u1 - a1) + (v1 - b1) * (v1 - b1)) * inv_s2;
    const double w2 = 1.0 / (H21[6] * u1 + H21[7] * v1 + H21[8]);
    const double a2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w2, b2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w2;
    *c2 = ((u2 - a2) * (u2 - a2) + (v2 - b2) * (v2 - b2)) * inv_s2;
}
// the score a direction adds (0 outside the threshold; a NaN error is outside) and the inlier rule: both directions inside
HG_HD double hg_score_term(double chi, double th) { return chi <= th ? HG_CHI2_H - chi : 0.0; }
HG_HD bool hg_inlier(double c1, double c2, double th) { return c1 <= th && c2 <= th; }
// the MSAC cost the hypotheses are ranked by: the truncated symmetric transfer error, 2 m HG_CHI2_H - score (non-negative, so the
// float32 bit pattern of a sum orders like its value)
HG_HD double hg_cost_term(double c1, double c2) {
    return (c1 <= HG_CHI2_H ? c1 : HG_CHI2_H) + (c2 <= HG_CHI2_H ? c2 : HG_CHI2_H);
}
// CheckFundamental for one correspondence: squared distances to the epipolar lines over sigma^2, image 2 (line F x1) then image 1
HG_HD void hg_fund_chi(const double* F, double u1, double v1, double u2, double v2, double inv_s2, double* c1, double* c2) {
    const double a2 = F[0] * u1 + F[1] * v1 + F[2], b2 = F[3] * u1 + F[4] * v1 + F[5], d2 = F[6] * u1 + F[7] * v1 + F[8];
    const double n2 = a2 * u2 + b2 * v2 + d2;
    *c1 = n2 * n2 / (a2 * a2 + b2 * b2) * inv_s2;
    const double a1 = F[0] * u2 + F[3] * v2 + F[6], b1 = F[1] * u2 + F[4] * v2 + F[7], d1 = F[2] * u2 + F[5] * v2 + F[8];
    const double n1 = a1 * u1 + b1 * v1 + d1;
    *c2 = n1 * n1 / (a1 * a1 + b1 * b1) * inv_s2;
}
// F = K^-T E K^-1 for K = [fx 0 cx; 0 fy cy; 0 0 1]
HG_HD void hg_fundamental_from_essential(const double* E, const double* K, double* F) {
    const double ifx = 1.0 / K[0], ify = 1.0 / K[4], cx = K[2], cy = K[5];
    double A[9];
    for (int i = 0; i < 3; i++) {  // A = E K^-1
        A[i * 3] = E[i * 3] * ifx; A[i * 3 + 1] = E[i * 3 + 1] * ify;
        A[i * 3 + 2] = E[i * 3 + 2] - (E[i * 3] * ifx * cx + E[i * 3 + 1] * ify * cy);
    }
    for (int j = 0; j < 3; j++) {  // F = K^-T A
        F[j] = A[j] * ifx; F[3 + j] = A[3 + j] * ify;
        F[6 + j] = A[6 + j] - (A[j] * ifx * cx + A[3 + j] * ify * cy);
    }
}

// ---- least-squares DLT: the two constraint rows of a correspondence (normalised coordinates), r[0 .. 9) and r[9 .. 18) -----------
HG_HD void hg_dlt_rows(double x1, double y1, double x2, double y2, double* r) {
    r[0] = 0.0; r[1] = 0.0; r[2] = 0.0; r[3] = -x1; r[4] = -y1; r[5] = -1.0; r[6] = y2 * x1; r[7] = y2 * y1; r[8] = y2;
    r[9] = x1; r[10] = y1; r[11] = 1.0; r[12] = 0.0; r[13] = 0.0; r[14] = 0.0; r[15] = -x2 * x1; r[16] = -x2 * y1; r[17] = -x2;
}

// ---- cyclic Jacobi eigen-decomposition of a symmetric NxN matrix (row-major a -> diagonal, eigenvectors in the columns of v) ------
template <int N> HG_HD void hg_jacobi(double* a, double* v) {
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) v[i * N + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; sweep++) {
        double off = 0, diag = 0;
        for (int i = 0; i < N; i++)
            for (int j = 0; j < N; j++) {
                if (i != j) off += a[i * N + j] * a[i * N + j];
                else diag += a[i * N + j] * a[i * N + j];
            }
        if (off <= 1e-30 * diag || off == 0.0 || !(off == off)) break;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int p = 0; p < N - 1; p++)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int q = p + 1; q < N; q++) {
                const double apq = a[p * N + q];
                if (apq != 0.0) {
                    const double theta = (a[q * N + q] - a[p * N + p]) / (2.0 * apq);
                    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    for (int k = 0; k < N; k++) {
                        const double akp = a[k * N + p], akq = a[k * N + q];
                        a[k * N + p] = c * akp - s * akq; a[k * N + q] = s * akp + c * akq;
                    }
                    for (int k = 0; k < N; k++) {
                        const double apk = a[p * N + k], aqk = a[q * N + k];
                        a[p * N + k] = c * apk - s * aqk; a[q * N + k] = s * apk + c * aqk;
                    }
                    for (int k = 0; k < N; k++) {
                        const double vkp = v[k * N + p], vkq = v[k * N + q];
                        v[k * N + p] = c * vkp - s * vkq; v[k * N + q] = s * vkp + c * vkq;
                    }
                }
            }
    }
}

HG_HD void hg_sign_fix(double* v) {
    const double a0 = fabs(v[0]), a1 = fabs(v[1]), a2 = fabs(v[2]);
    const double lead = a0 >= a1 && a0 >= a2 ? v[0] : a1 >= a2 ? v[1] : v[2];
    if (lead < 0.0) { v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; }
}

// SVD of a 3x3 matrix A = U diag(d) V' with d[0] >= d[1] >= d[2] and det(U) = det(V) = +1 (the scheme of svd3_rank2 in
// twoview_kernels.hip): V from the Jacobi eigenvectors of A'A, u_i = A v_i / d_i for the two largest, the third vectors by cross
// products.  (For det(A) < 0 the third singular value is then negative in effect; hg_reconstruct flips A's sign first.)
HG_HD bool hg_svd3(const double* A, double* U, double* V, double* d) {
    double a[9], v[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) a[i * 3 + j] = A[i] * A[j] + A[3 + i] * A[3 + j] + A[6 + i] * A[6 + j];
    hg_jacobi<3>(a, v);
    double l0 = a[0], l1 = a[4], l2 = a[8];
    double c0[3] = {v[0], v[3], v[6]}, c1[3] = {v[1], v[4], v[7]}, c2[3] = {v[2], v[5], v[8]};
#define HG_CSWAP(la, lb, ca, cb)                                                              \
    if (la < lb) {                                                                            \
        const double t_ = la; la = lb; lb = t_;                                               \
        for (int i_ = 0; i_ < 3; i_++) { const double u_ = ca[i_]; ca[i_] = cb[i_]; cb[i_] = u_; } \
    }
    HG_CSWAP(l0, l1, c0, c1)
    HG_CSWAP(l1, l2, c1, c2)
    HG_CSWAP(l0, l1, c0, c1)
#undef HG_CSWAP
    const double s1 = sqrt(l0 > 0.0 ? l0 : 0.0), s2 = sqrt(l1 > 0.0 ? l1 : 0.0), s3 = sqrt(l2 > 0.0 ? l2 : 0.0);
    if (!(s2 > 1e-12 * s1) || !(s1 > 0.0) || !hg_finite(s1)) return false;
    // An SVD fixes its vectors up to a common sign of (u_i, v_i), and the ORDER of Faugeras' candidates follows those signs.  Canonical
    // form, so that two solvers list the candidates alike: the first and the third right vector have their largest component
    // (the first of equals) positive, and the second completes the right-handed frame.
    hg_sign_fix(c0);
    hg_sign_fix(c2);
    hg_cross(c2, c0, c1);
    double u1[3], u2[3], u3[3], v3[3];
    for (int i = 0; i < 3; i++) {
        u1[i] = (A[i * 3] * c0[0] + A[i * 3 + 1] * c0[1] + A[i * 3 + 2] * c0[2]) / s1;
        u2[i] = (A[i * 3] * c1[0] + A[i * 3 + 1] * c1[1] + A[i * 3 + 2] * c1[2]) / s2;
    }
    const double dt = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
    for (int i = 0; i < 3; i++) u2[i] -= dt * u1[i];
    const double n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]), n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    if (!(n1 > 0.0) || !(n2 > 0.0)) return false;
    for (int i = 0; i < 3; i++) { u1[i] /= n1; u2[i] /= n2; }
    hg_cross(u1, u2, u3);
    hg_cross(c0, c1, v3);
    for (int i = 0; i < 3; i++) {
        U[i * 3] = u1[i]; U[i * 3 + 1] = u2[i]; U[i * 3 + 2] = u3[i];
        V[i * 3] = c0[i]; V[i * 3 + 1] = c1[i]; V[i * 3 + 2] = v3[i];
    }
    d[0] = s1; d[1] = s2; d[2] = s3;
    return true;
}

// ---- ReconstructH (Faugeras & Lustman 1988, as ORB-SLAM2 restates it) ------------------------------------------------------------
// A = K^-1 H K, its sign chosen so that det(A) > 0 (H is known up to scale; with det(U) = det(V) = +1 ORB-SLAM2's s = det(U) det(V')
// is then 1).  False = no decomposition: A has no SVD, or d1 / d2 < 1.00001 or d2 / d3 < 1.00001 (a pure rotation, H = K R K^-1, has
// three equal singular values).  Candidates in ORB-SLAM2's order: four with d' = d2 > 0, then four with d' = -d2.  R: [8][9],
// t: [8][3] (unit length), n: [8][3] (plane normal, n_z >= 0).
HG_HD bool hg_reconstruct(const double* H, const double* K, double* R, double* t, double* n) {
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const double Ki[9] = {1.0 / fx, 0.0, -cx / fx, 0.0, 1.0 / fy, -cy / fy, 0.0, 0.0, 1.0};
    const double Kf[9] = {fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0};
    double T[9], A[9], U[9], V[9], d[3];
    hg_mul3(Ki, H, T);
    hg_mul3(T, Kf, A);
    const double det = hg_det3(A);
    if (!hg_finite(det)) return false;
    if (det < 0.0) for (int j = 0; j < 9; j++) A[j] = -A[j];
    if (!hg_svd3(A, U, V, d)) return false;
    const double d1 = d[0], d2 = d[1], d3 = d[2];
    if (!(d3 > 0.0) || d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return false;
    const double q12 = d1 * d1 - d2 * d2, q23 = d2 * d2 - d3 * d3, q13 = d1 * d1 - d3 * d3;
    const double aux1 = sqrt(q12 / q13), aux3 = sqrt(q23 / q13);
    const double x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
    const double ss = sqrt(q12 * q23);
    const double st = ss / ((d1 + d3) * d2), ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const double sp = ss / ((d1 - d3) * d2), cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const double sgn[4] = {1.0, -1.0, -1.0, 1.0};
    double Vt[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Vt[i * 3 + j] = V[j * 3 + i];
    for (int c = 0; c < 8; c++) {
        const int i = c & 3;
        const bool pos = c < 4;
        const double sn = (pos ? st : sp) * sgn[i];
        double Rp[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
        if (pos) { Rp[0] = ct; Rp[2] = -sn; Rp[6] = sn; Rp[8] = ct; }
        else { Rp[0] = cp; Rp[2] = sn; Rp[4] = -1.0; Rp[6] = sn; Rp[8] = -cp; }
        double M[9];
        hg_mul3(U, Rp, M);
        hg_mul3(M, Vt, R + c * 9);
        const double tp0 = x1[i] * (pos ? d1 - d3 : d1 + d3), tp2 = (pos ? -x3[i] : x3[i]) * (pos ? d1 - d3 : d1 + d3);
        double tt[3], nn[3];
        for (int r = 0; r < 3; r++) {
            tt[r] = U[r * 3] * tp0 + U[r * 3 + 2] * tp2;
            nn[r] = V[r * 3] * x1[i] + V[r * 3 + 2] * x3[i];
        }
        const double tn = sqrt(tt[0] * tt[0] + tt[1] * tt[1] + tt[2] * tt[2]);
        const double ns = nn[2] < 0.0 ? -1.0 : 1.0;
        for (int r = 0; r < 3; r++) { t[c * 3 + r] = tt[r] / tn; n[c * 3 + r] = ns * nn[r]; }
    }
    return true;
}

// ---- CheckRT for one correspondence and one candidate ------------------------------------------------------------------------------
// DLT triangulation with P1 = K [I | 0], P2 = K [R | t] in pixels (smallest eigenvector of the 4x4 normal matrix by cyclic Jacobi),
// finite test, cos of the parallax angle between the rays from the two centres, positive depth in both cameras unless
// cos >= HG_COS_GOOD, squared reprojection error <= th2 in both images.  Returns 0 = failed, 1 = passed (counted, its cos enters the
// parallax list), 3 = passed and good (cos < HG_COS_GOOD: a map point).  *cosp and X (camera 1) are set whenever the point is finite.
HG_HD int hg_check_rt(const double* K, const double* R, const double* t, double u1, double v1, double u2, double v2, double th2,
                      double* cosp, double* X) {
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    double P2[12];
    for (int j = 0; j < 3; j++) {
        P2[j] = fx * R[j] + cx * R[6 + j]; P2[4 + j] = fy * R[3 + j] + cy * R[6 + j]; P2[8 + j] = R[6 + j];
    }
    P2[3] = fx * t[0] + cx * t[2]; P2[7] = fy * t[1] + cy * t[2]; P2[11] = t[2];
    const double A[16] = {-fx, 0.0, u1 - cx, 0.0,
                          0.0, -fy, v1 - cy, 0.0,
                          u2 * P2[8] - P2[0], u2 * P2[9] - P2[1], u2 * P2[10] - P2[2], u2 * P2[11] - P2[3],
                          v2 * P2[8] - P2[4], v2 * P2[9] - P2[5], v2 * P2[10] - P2[6], v2 * P2[11] - P2[7]};
    double S[16], Vv[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) S[i * 4 + j] = A[i] * A[j] + A[4 + i] * A[4 + j] + A[8 + i] * A[8 + j] + A[12 + i] * A[12 + j];
    hg_jacobi<4>(S, Vv);
    // the column of the smallest eigenvalue (the first one on a tie), selected without dynamic indexing
    double lb = S[0], q0 = Vv[0], q1 = Vv[4], q2 = Vv[8], q3 = Vv[12];
    if (S[5] < lb) { lb = S[5]; q0 = Vv[1]; q1 = Vv[5]; q2 = Vv[9]; q3 = Vv[13]; }
    if (S[10] < lb) { lb = S[10]; q0 = Vv[2]; q1 = Vv[6]; q2 = Vv[10]; q3 = Vv[14]; }
    if (S[15] < lb) { lb = S[15]; q0 = Vv[3]; q1 = Vv[7]; q2 = Vv[11]; q3 = Vv[15]; }
    const double x = q0 / q3, y = q1 / q3, z = q2 / q3;
    X[0] = x; X[1] = y; X[2] = z;
    *cosp = 2.0;
    if (!(hg_finite(x) && hg_finite(y) && hg_finite(z))) return 0;
    // O1 = 0, O2 = -R' t
    const double o0 = -(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]), o1 = -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]),
                 o2 = -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2]);
    const double m0 = x - o0, m1 = y - o1, m2 = z - o2;
    const double cs = (x * m0 + y * m1 + z * m2) / (sqrt(x * x + y * y + z * z) * sqrt(m0 * m0 + m1 * m1 + m2 * m2));
    *cosp = cs;
    const bool low = !(cs < HG_COS_GOOD);  // (a NaN cos counts as no parallax, like ORB-SLAM2's comparisons)
    if (z <= 0.0 && !low) return 0;
    const double x2 = R[0] * x + R[1] * y + R[2] * z + t[0], y2 = R[3] * x + R[4] * y + R[5] * z + t[1], z2 = R[6] * x + R[7] * y + R[8] * z + t[2];
    if (z2 <= 0.0 && !low) return 0;
    const double iz1 = 1.0 / z, a1 = fx * x * iz1 + cx, b1 = fy * y * iz1 + cy;
    const double e1 = (a1 - u1) * (a1 - u1) + (b1 - v1) * (b1 - v1);
    if (!(e1 <= th2)) return 0;
    const double iz2 = 1.0 / z2, a2 = fx * x2 * iz2 + cx, b2 = fy * y2 * iz2 + cy;
    const double e2 = (a2 - u2) * (a2 - u2) + (b2 - v2) * (b2 - v2);
    if (!(e2 <= th2)) return 0;
    return low ? 1 : 3;
}

// ---- selection among the eight candidates (ORB-SLAM2's loop) and the acceptance rule ---------------------------------------------
// best / second: candidate indices (-1: none), by n_good with the first of equals winning
HG_HD void hg_select(const int* n_good, int* best, int* second) {
    int bg = 0, sg = 0, bi = -1, si = -1;
    for (int i = 0; i < 8; i++) {
        if (n_good[i] > bg) { sg = bg; si = bi; bg = n_good[i]; bi = i; }
        else if (n_good[i] > sg) { sg = n_good[i]; si = i; }
    }
    *best = bi; *second = si;
}
// cos_max = cos(min_parallax): parallax >= min_parallax  <=>  cos <= cos_max
HG_HD bool hg_accept(int best_good, int second_good, double best_cos, double cos_max, int min_triangulated, int n_inliers) {
    return (double)second_good < 0.75 * (double)best_good && best_cos <= cos_max && best_good > min_triangulated &&
           (double)best_good > 0.9 * (double)n_inliers;
}
