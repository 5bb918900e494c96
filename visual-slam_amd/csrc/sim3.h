// Similarity between two keyframes from 3D-3D correspondences, shared by the loop-alignment kernels (map_sim3.hip), the CPU test of
// the solver (tests/native/sim3_check.cpp) and the host replay of the chain (tests/native/sim3_replay.cpp): Horn's closed form, the
// two-sided reprojection test and one Gauss-Newton step on sim(3).  ORB-SLAM2's Sim3Solver::ComputeSim3 / CheckInliers and
// Optimizer::OptimizeSim3.  Everything is f64; built with -ffp-contract=off on both sides, so a host build computes what the device
// computes.  Nothing that decides whether a sample has a model uses libm beyond sqrt / fabs; the Gauss-Newton update takes exp of the
// log-scale step and pnp_exp_so3's sin / cos, which is why a refined model is compared under a tolerance and every test case keeps
// its inlier decisions away from the threshold.
//
// Convention: X1 = s R X2 + t takes a point from the candidate's camera frame (2) to the asking keyframe's camera frame (1).  The
// inverse is s21 = 1 / s, R21 = R^T, t21 = -s21 R21 t.
//
// Closed form (Horn 1987): centroids O1, O2, relative coordinates Pr1, Pr2, M = sum Pr2 Pr1^T, the symmetric 4x4 N of M; the
// eigenvector of N's largest eigenvalue is the unit quaternion (w, x, y, z) of R.  It is found by cyclic Jacobi: the pairs (0,1) (0,2)
// (0,3) (1,2) (1,3) (2,3) in that order, SIM3_SWEEPS sweeps, every rotation from a sqrt and divisions, the pairs unrolled so that no
// matrix entry is indexed by a run-time value.  R comes from the quaternion by products (no axis-angle detour),
// s = sum Pr1 . (R Pr2) / sum |R Pr2|^2, t = O1 - s R O2.  No model: an input or a result that is not finite, a denominator that is
// not > 0, s not > 0, and - one rule more than ORB-SLAM2 has - a largest eigenvalue that is not separated from the second (points
// that are collinear or coincident in either frame leave the rotation about their line free: N then has a double largest eigenvalue,
// and which of its eigenvectors a solver returns is an accident of rounding).
//
// Inlier test, two-sided: pair i is an inlier when X2 taken into frame 1 has z > 0 and its projection by K has
// information1 * squared pixel error < chi2 against the keypoint of keyframe 1, and X1 taken into frame 2 has z > 0 and
// information2 * squared pixel error < chi2 against the candidate's keypoint (strict; information = 1 / scale_factor^(2 octave) by
// ba_info: repeated products from 1.0, negative octaves as 0 - the threshold chi2 * scale_factor^(2 octave) in squared pixels).
// Deviation from ORB-SLAM2: its CheckInliers compares against the projections of the 3D points themselves; here the keypoints are
// the measurement.
//
// Gauss-Newton on sim(3): delta = (rho, w, lambda), left-multiplicative: s' = e^lambda s, R' = exp(w) R,
// t' = e^lambda exp(w) t + rho.  Both reprojection residuals of a pair, the 3D points fixed (OptimizeSim3 with bFixScale = false);
// weight = information * Huber weight of pnp_gn_accumulate_w with huber2 = chi2.  H is the upper triangle of J^T J (row-major, 28
// entries), g = J^T r with r = projection - keypoint.
#pragma once
#include "ba.h"

#define SIM3_HD PNP_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define SIM3_UNROLL _Pragma("unroll")
#else
#define SIM3_UNROLL
#endif
#define SIM3_SWEEPS 8
#define SIM3_EIG_GAP 1e-9   // the largest eigenvalue leads the second by more than this times the largest magnitude

struct Sim3 {
    double s, R[9], t[3];
};

// one gathered correspondence: the two points in their camera frames, the two keypoints with their information
struct Sim3Pair {
    double X1[3], X2[3];
    double x1, y1, i1, x2, y2, i2;
};

SIM3_HD bool sim3_finite(const Sim3& S) {
    bool f = isfinite(S.s);
    for (int i = 0; i < 9; i++) f &= isfinite(S.R[i]);
    for (int i = 0; i < 3; i++) f &= isfinite(S.t[i]);
    return f;
}

SIM3_HD void sim3_inverse(const Sim3& S, Sim3& I) {
    I.s = 1.0 / S.s;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) I.R[i * 3 + j] = S.R[j * 3 + i];
    for (int i = 0; i < 3; i++) I.t[i] = -I.s * (I.R[i * 3] * S.t[0] + I.R[i * 3 + 1] * S.t[1] + I.R[i * 3 + 2] * S.t[2]);
}

// Y = s R X + t (each row summed left to right)
SIM3_HD void sim3_apply(const Sim3& S, const double* X, double* Y) {
    for (int i = 0; i < 3; i++) Y[i] = S.s * (S.R[i * 3] * X[0] + S.R[i * 3 + 1] * X[1] + S.R[i * 3 + 2] * X[2]) + S.t[i];
}

// ---- the eigenvector of the largest eigenvalue of a symmetric 4x4 ------------------------------------------------------------------
// one Jacobi rotation of the pair (P, Q): A <- J^T A J, V <- V J
template <int P, int Q> SIM3_HD void sim3_jacobi_rot(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double th = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double tn = (th < 0.0 ? -1.0 : 1.0) / (fabs(th) + sqrt(th * th + 1.0));
    const double c = 1.0 / sqrt(tn * tn + 1.0), s = tn * c;
SIM3_UNROLL
    for (int k = 0; k < 4; k++) {
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
SIM3_UNROLL
    for (int k = 0; k < 4; k++) {
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
SIM3_UNROLL
    for (int k = 0; k < 4; k++) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// q = the unit eigenvector of the largest eigenvalue of the symmetric A (destroyed); false when it is not separated from the second
SIM3_HD bool sim3_top_eigenvector(double (&A)[4][4], double* q) {
    double V[4][4];
SIM3_UNROLL
    for (int i = 0; i < 4; i++)
SIM3_UNROLL
        for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < SIM3_SWEEPS; sweep++) {
        sim3_jacobi_rot<0, 1>(A, V); sim3_jacobi_rot<0, 2>(A, V); sim3_jacobi_rot<0, 3>(A, V);
        sim3_jacobi_rot<1, 2>(A, V); sim3_jacobi_rot<1, 3>(A, V); sim3_jacobi_rot<2, 3>(A, V);
    }
    const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2], e3 = A[3][3];
    // the largest (ties to the lower index) and the second, by comparisons only
    int b = 0;
    double top = e0;
    if (e1 > top) { top = e1; b = 1; }
    if (e2 > top) { top = e2; b = 2; }
    if (e3 > top) { top = e3; b = 3; }
    double second = -1.0e300, mag = 0.0;
    if (b != 0 && e0 > second) second = e0;
    if (b != 1 && e1 > second) second = e1;
    if (b != 2 && e2 > second) second = e2;
    if (b != 3 && e3 > second) second = e3;
    mag = fabs(e0);
    if (fabs(e1) > mag) mag = fabs(e1);
    if (fabs(e2) > mag) mag = fabs(e2);
    if (fabs(e3) > mag) mag = fabs(e3);
    if (!isfinite(top) || !(top - second > SIM3_EIG_GAP * mag)) return false;
SIM3_UNROLL
    for (int k = 0; k < 4; k++) q[k] = b == 0 ? V[k][0] : b == 1 ? V[k][1] : b == 2 ? V[k][2] : V[k][3];
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(n > 0.0) || !isfinite(n)) return false;
SIM3_UNROLL
    for (int k = 0; k < 4; k++) q[k] /= n;
    return true;
}

// ---- Horn's closed form over N pairs: P1, P2 [N][3] ------------------------------------------------------------------------------------
template <int N> SIM3_HD bool sim3_horn(const double (&P1)[N][3], const double (&P2)[N][3], Sim3& S) {
    static_assert(N >= 3, "three pairs at least");
    double O1[3] = {0.0, 0.0, 0.0}, O2[3] = {0.0, 0.0, 0.0};
SIM3_UNROLL
    for (int i = 0; i < N; i++)
SIM3_UNROLL
        for (int k = 0; k < 3; k++) { O1[k] += P1[i][k]; O2[k] += P2[i][k]; }
SIM3_UNROLL
    for (int k = 0; k < 3; k++) { O1[k] /= (double)N; O2[k] /= (double)N; }
    if (!(isfinite(O1[0]) && isfinite(O1[1]) && isfinite(O1[2]) && isfinite(O2[0]) && isfinite(O2[1]) && isfinite(O2[2]))) return false;
    // M[a][b] = sum Pr2[a] Pr1[b]
    double M[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
SIM3_UNROLL
    for (int i = 0; i < N; i++)
SIM3_UNROLL
        for (int a = 0; a < 3; a++)
SIM3_UNROLL
            for (int b = 0; b < 3; b++) M[a][b] += (P2[i][a] - O2[a]) * (P1[i][b] - O1[b]);
    double A[4][4];
    A[0][0] = M[0][0] + M[1][1] + M[2][2];
    A[0][1] = M[1][2] - M[2][1];
    A[0][2] = M[2][0] - M[0][2];
    A[0][3] = M[0][1] - M[1][0];
    A[1][1] = M[0][0] - M[1][1] - M[2][2];
    A[1][2] = M[0][1] + M[1][0];
    A[1][3] = M[2][0] + M[0][2];
    A[2][2] = -M[0][0] + M[1][1] - M[2][2];
    A[2][3] = M[1][2] + M[2][1];
    A[3][3] = -M[0][0] - M[1][1] + M[2][2];
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[3][0] = A[0][3]; A[2][1] = A[1][2]; A[3][1] = A[1][3]; A[3][2] = A[2][3];
    double q[4];
    if (!sim3_top_eigenvector(A, q)) return false;
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    S.R[0] = 1.0 - 2.0 * (y * y + z * z); S.R[1] = 2.0 * (x * y - w * z); S.R[2] = 2.0 * (x * z + w * y);
    S.R[3] = 2.0 * (x * y + w * z); S.R[4] = 1.0 - 2.0 * (x * x + z * z); S.R[5] = 2.0 * (y * z - w * x);
    S.R[6] = 2.0 * (x * z - w * y); S.R[7] = 2.0 * (y * z + w * x); S.R[8] = 1.0 - 2.0 * (x * x + y * y);
    double nom = 0.0, den = 0.0;
SIM3_UNROLL
    for (int i = 0; i < N; i++) {
        const double r[3] = {P2[i][0] - O2[0], P2[i][1] - O2[1], P2[i][2] - O2[2]};
SIM3_UNROLL
        for (int k = 0; k < 3; k++) {
            const double v = S.R[k * 3] * r[0] + S.R[k * 3 + 1] * r[1] + S.R[k * 3 + 2] * r[2];
            nom += (P1[i][k] - O1[k]) * v;
            den += v * v;
        }
    }
    if (!(den > 0.0) || !isfinite(den)) return false;
    S.s = nom / den;
    if (!(S.s > 0.0)) return false;
SIM3_UNROLL
    for (int k = 0; k < 3; k++) S.t[k] = O1[k] - S.s * (S.R[k * 3] * O2[0] + S.R[k * 3 + 1] * O2[1] + S.R[k * 3 + 2] * O2[2]);
    return sim3_finite(S);
}

// ---- projection and the inlier test ------------------------------------------------------------------------------------------------
// p = K Y; the weighted squared pixel error against (x, y); false when the depth Y[2] is not > 0
SIM3_HD bool sim3_reproj2(const double* K, const double* Y, double x, double y, double info, double* e2) {
    const double p0 = K[0] * Y[0] + K[1] * Y[1] + K[2] * Y[2], p1 = K[3] * Y[0] + K[4] * Y[1] + K[5] * Y[2], p2 = K[6] * Y[0] + K[7] * Y[1] + K[8] * Y[2];
    const double du = p0 / p2 - x, dv = p1 / p2 - y;
    *e2 = info * (du * du + dv * dv);
    return Y[2] > 0.0;
}

// the two weighted errors of a pair under S12 and its inverse S21; true when the pair is an inlier
SIM3_HD bool sim3_inlier(const double* K, const Sim3& S12, const Sim3& S21, const Sim3Pair& c, double chi2, double* e1, double* e2) {
    double Y[3], Z[3];
    sim3_apply(S12, c.X2, Y);
    sim3_apply(S21, c.X1, Z);
    const bool f1 = sim3_reproj2(K, Y, c.x1, c.y1, c.i1, e1), f2 = sim3_reproj2(K, Z, c.x2, c.y2, c.i2, e2);
    return f1 && *e1 < chi2 && f2 && *e2 < chi2;
}

// ---- Gauss-Newton on sim(3) ------------------------------------------------------------------------------------------------------------
// one residual: the point Y in its camera, its derivative D [3][7] against delta, the keypoint and its information
SIM3_HD void sim3_gn_term(const double* K, const double* Y, const double (&D)[3][7], double x, double y, double info, double huber2, double* H,
                          double* g) {
    const double p0 = K[0] * Y[0] + K[1] * Y[1] + K[2] * Y[2], p1 = K[3] * Y[0] + K[4] * Y[1] + K[5] * Y[2], p2 = K[6] * Y[0] + K[7] * Y[1] + K[8] * Y[2];
    if (!(p2 != 0.0)) return;
    const double iz = 1.0 / p2, iz2 = iz * iz;
    const double ru = p0 * iz - x, rv = p1 * iz - y;
    double du[3], dv[3];
SIM3_UNROLL
    for (int k = 0; k < 3; k++) { du[k] = (K[k] * p2 - p0 * K[6 + k]) * iz2; dv[k] = (K[3 + k] * p2 - p1 * K[6 + k]) * iz2; }
    double Ju[7], Jv[7];
SIM3_UNROLL
    for (int k = 0; k < 7; k++) {
        Ju[k] = du[0] * D[0][k] + du[1] * D[1][k] + du[2] * D[2][k];
        Jv[k] = dv[0] * D[0][k] + dv[1] * D[1][k] + dv[2] * D[2][k];
    }
    const double e2 = info * (ru * ru + rv * rv);
    const double wt = huber2 > 0.0 && e2 > huber2 ? info * (sqrt(huber2) / sqrt(e2)) : info;
    int o = 0;
SIM3_UNROLL
    for (int i = 0; i < 7; i++) {
SIM3_UNROLL
        for (int j = i; j < 7; j++) H[o++] += wt * (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
        g[i] += wt * (Ju[i] * ru + Jv[i] * rv);
    }
}

// both residuals of a pair added to H [28], g [7]
SIM3_HD void sim3_gn_accumulate(const double* K, const Sim3& S12, const Sim3& S21, const Sim3Pair& c, double huber2, double* H, double* g) {
    // forward: Y = s R X2 + t; dY / d rho = I, dY / d w = -[Y]x, dY / d lambda = Y
    double Y[3];
    sim3_apply(S12, c.X2, Y);
    const double DF[3][7] = {{1.0, 0.0, 0.0, 0.0, Y[2], -Y[1], Y[0]}, {0.0, 1.0, 0.0, -Y[2], 0.0, Y[0], Y[1]}, {0.0, 0.0, 1.0, Y[1], -Y[0], 0.0, Y[2]}};
    sim3_gn_term(K, Y, DF, c.x1, c.y1, c.i1, huber2, H, g);
    // backward: Z = S21 X1 with S21' = S21 exp(-delta): dZ / d rho = -A, dZ / d w_k = A (X1 x e_k), dZ / d lambda = -A X1, A = s21 R21
    double Z[3];
    sim3_apply(S21, c.X1, Z);
    const double* X = c.X1;
    const double C[3][3] = {{0.0, X[2], -X[1]}, {-X[2], 0.0, X[0]}, {X[1], -X[0], 0.0}};   // C[k] = X1 x e_k
    double DB[3][7];
SIM3_UNROLL
    for (int i = 0; i < 3; i++) {
        const double a0 = S21.s * S21.R[i * 3], a1 = S21.s * S21.R[i * 3 + 1], a2 = S21.s * S21.R[i * 3 + 2];
        DB[i][0] = -a0; DB[i][1] = -a1; DB[i][2] = -a2;
SIM3_UNROLL
        for (int k = 0; k < 3; k++) DB[i][3 + k] = a0 * C[k][0] + a1 * C[k][1] + a2 * C[k][2];
        DB[i][6] = -(a0 * X[0] + a1 * X[1] + a2 * X[2]);
    }
    sim3_gn_term(K, Z, DB, c.x2, c.y2, c.i2, huber2, H, g);
}

// solve H delta = -g (Cholesky) and apply it; false (model unchanged) when H is not positive definite or the result is not a
// similarity (not finite, s not > 0).  *step = |delta|.
SIM3_HD bool sim3_gn_update(const double* H, const double* g, Sim3& S, double* step) {
    double L[7][7];
    int o = 0;
    for (int i = 0; i < 7; i++)
        for (int j = i; j < 7; j++) { L[j][i] = H[o]; L[i][j] = H[o]; o++; }
    for (int j = 0; j < 7; j++) {
        double s = L[j][j];
        for (int k = 0; k < j; k++) s -= L[j][k] * L[j][k];
        if (!(s > 0.0) || !isfinite(s)) return false;
        L[j][j] = sqrt(s);
        for (int i = j + 1; i < 7; i++) {
            double v = L[i][j];
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    double z[7], d[7];
    for (int i = 0; i < 7; i++) {
        double v = -g[i];
        for (int k = 0; k < i; k++) v -= L[i][k] * z[k];
        z[i] = v / L[i][i];
    }
    for (int i = 6; i >= 0; i--) {
        double v = z[i];
        for (int k = i + 1; k < 7; k++) v -= L[k][i] * d[k];
        d[i] = v / L[i][i];
    }
    double E[9];
    pnp_exp_so3(d + 3, E);
    const double el = exp(d[6]);
    Sim3 T;
    T.s = el * S.s;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T.R[i * 3 + j] = E[i * 3] * S.R[j] + E[i * 3 + 1] * S.R[3 + j] + E[i * 3 + 2] * S.R[6 + j];
        T.t[i] = el * (E[i * 3] * S.t[0] + E[i * 3 + 1] * S.t[1] + E[i * 3 + 2] * S.t[2]) + d[i];
    }
    double n2 = 0.0;
    for (int i = 0; i < 7; i++) n2 += d[i] * d[i];
    if (!sim3_finite(T) || !(T.s > 0.0) || !isfinite(n2)) return false;
    S = T;
    *step = sqrt(n2);
    return true;
}
