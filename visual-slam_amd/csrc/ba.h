// Bundle adjustment, the arithmetic shared by the kernels (ba_problem.h: the passes both solvers run; map_ba.hip: the local solver;
// map_gba.hip with gba.h: the global one) and the CPU test of it (tests/native/ba_check.cpp): the
// reprojection residual and its Jacobians, the per-edge terms of the normal equations, the 3x3 SPD inverse of a point block, the
// Schur-complement terms of one point, the dense Cholesky solve of the reduced camera system, back-substitution, the pose update.
// Everything is f64; built with -ffp-contract=off on both sides, so a host build computes what the device computes.
//
// Conventions: pose T = [R | t] row-major 3x4, X_cam = R X + t, p = K X_cam, projection (p0 / p2, p1 / p2) as mo_map_track forms it;
// residual e = keypoint - projection; Jacobians are those of the PROJECTION (J_c 2x6 against the left perturbation delta = (rho, w)
// of pnp.h: R' = exp(w) R, t' = exp(w) t + rho; J_p 2x3 against the point), so the normal equations read
//   [ H_cc  W ] [d_c]   [g_c]      H_cc = sum w J_c^T J_c, V = sum w J_p^T J_p, W = w J_c^T J_p, g = sum w J^T e
//   [ W^T   V ] [d_p] = [g_p]      w = information * Huber weight
// and with the points eliminated: S = H_cc - sum W V^-1 W^T, b = g_c - sum W V^-1 g_p, d_p = V^-1 (g_p - W^T d_c).
// The product W_a V^-1 W_b^T is formed as J_ca^T (w_a w_b J_pa V^-1 J_pb^T) J_cb: a 2x2 core between the two camera Jacobians.
#pragma once
#include "pnp.h"

#define BA_HD PNP_HD
#define BA_MAX_FREE 16                    // free keyframes of one problem
#define BA_MAX_DIM (6 * BA_MAX_FREE)      // unknowns of the reduced camera system
#define BA_TRI(i, j) ((i) * ((i) + 1) / 2 + (j))   // packed lower triangle, j <= i

// information of an octave: 1 / scale_factor^(2 o), repeated products from 1.0 (negative octaves as 0); the one definition, for the
// edges of the bundle adjustment and the matches of mo_map_track's refinement (map_track.hip)
BA_HD double ba_info(double sf, int o) {
    const double sf2 = sf * sf;
    double s = 1.0;
    for (int i = 0; i < o; i++) s *= sf2;
    return 1.0 / s;
}

// Huber on e2 = information * |e|^2 with width^2 = huber2 (0: none): the cost and the weight of the reweighted normal equations
BA_HD double ba_rho(double e2, double huber2) { return huber2 > 0.0 && e2 > huber2 ? 2.0 * sqrt(huber2) * sqrt(e2) - huber2 : e2; }
BA_HD double ba_weight(double e2, double huber2) { return huber2 > 0.0 && e2 > huber2 ? sqrt(huber2) / sqrt(e2) : 1.0; }

// e = keypoint - projection, *zc = the depth; false (nothing usable) when the projection is not finite
BA_HD bool ba_residual(const double* K, const double* T, const double* X, double x, double y, double* e, double* zc) {
    const double xc = T[0] * X[0] + T[1] * X[1] + T[2] * X[2] + T[3];
    const double yc = T[4] * X[0] + T[5] * X[1] + T[6] * X[2] + T[7];
    const double z = T[8] * X[0] + T[9] * X[1] + T[10] * X[2] + T[11];
    const double p0 = K[0] * xc + K[1] * yc + K[2] * z, p1 = K[3] * xc + K[4] * yc + K[5] * z, p2 = K[6] * xc + K[7] * yc + K[8] * z;
    *zc = z;
    if (!(p2 != 0.0)) return false;
    e[0] = x - p0 / p2;
    e[1] = y - p1 / p2;
    return isfinite(e[0]) && isfinite(e[1]);
}

// Jc [2][6] = d projection / d (rho, w), Jp [2][3] = d projection / d X; false like ba_residual
BA_HD bool ba_jacobians(const double* K, const double* T, const double* X, double* Jc, double* Jp) {
    const double c[3] = {T[0] * X[0] + T[1] * X[1] + T[2] * X[2] + T[3], T[4] * X[0] + T[5] * X[1] + T[6] * X[2] + T[7],
                         T[8] * X[0] + T[9] * X[1] + T[10] * X[2] + T[11]};
    const double p0 = K[0] * c[0] + K[1] * c[1] + K[2] * c[2], p1 = K[3] * c[0] + K[4] * c[1] + K[5] * c[2], p2 = K[6] * c[0] + K[7] * c[1] + K[8] * c[2];
    if (!(p2 != 0.0)) return false;
    const double iz = 1.0 / p2, iz2 = iz * iz;
    double d[2][3];   // d (u, v) / d X_cam
    for (int k = 0; k < 3; k++) { d[0][k] = (K[k] * p2 - p0 * K[6 + k]) * iz2; d[1][k] = (K[3 + k] * p2 - p1 * K[6 + k]) * iz2; }
    for (int r = 0; r < 2; r++) {
        const double* q = d[r];
        double* J = Jc + r * 6;
        J[0] = q[0]; J[1] = q[1]; J[2] = q[2];
        // d X_cam / d w = -[X_cam]x
        J[3] = -q[1] * c[2] + q[2] * c[1]; J[4] = q[0] * c[2] - q[2] * c[0]; J[5] = -q[0] * c[1] + q[1] * c[0];
        for (int k = 0; k < 3; k++) Jp[r * 3 + k] = q[0] * T[k] + q[1] * T[4 + k] + q[2] * T[8 + k];
    }
    return true;
}

// point block of one edge: V (upper triangle 00 01 02 11 12 22) += w Jp^T Jp, gp += w Jp^T e
BA_HD void ba_point_terms(const double* Jp, double w, const double* e, double* V, double* gp) {
    int o = 0;
    for (int i = 0; i < 3; i++) {
        for (int j = i; j < 3; j++) V[o++] += w * (Jp[i] * Jp[j] + Jp[3 + i] * Jp[3 + j]);
        gp[i] += w * (Jp[i] * e[0] + Jp[3 + i] * e[1]);
    }
}

// camera block of one edge: A [6][6] += w Jc^T Jc, g += w Jc^T e
BA_HD void ba_camera_terms(const double* Jc, double w, const double* e, double* A, double* g) {
    for (int i = 0; i < 6; i++) {
        for (int j = 0; j < 6; j++) A[i * 6 + j] += w * (Jc[i] * Jc[j] + Jc[6 + i] * Jc[6 + j]);
        g[i] += w * (Jc[i] * e[0] + Jc[6 + i] * e[1]);
    }
}

// inverse of the SPD 3x3 V (upper triangle) by Cholesky; false when a pivot is not > 0 or not finite
BA_HD bool ba_inv3(const double* V, double* Vi) {
    if (!(V[0] > 0.0) || !isfinite(V[0])) return false;
    const double l00 = sqrt(V[0]), l10 = V[1] / l00, l20 = V[2] / l00;
    const double s1 = V[3] - l10 * l10;
    if (!(s1 > 0.0) || !isfinite(s1)) return false;
    const double l11 = sqrt(s1), l21 = (V[4] - l20 * l10) / l11;
    const double s2 = V[5] - l20 * l20 - l21 * l21;
    if (!(s2 > 0.0) || !isfinite(s2)) return false;
    const double l22 = sqrt(s2);
    // M = L^-1 (lower), V^-1 = M^T M
    const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
    const double m10 = -l10 * m00 * m11, m21 = -l21 * m11 * m22, m20 = -(l20 * m00 + l21 * m10) * m22;
    Vi[0] = m00 * m00 + m10 * m10 + m20 * m20; Vi[1] = m10 * m11 + m20 * m21; Vi[2] = m20 * m22;
    Vi[3] = m11 * m11 + m21 * m21; Vi[4] = m21 * m22; Vi[5] = m22 * m22;
    return true;
}

// y = Vi x for the symmetric Vi (upper triangle)
BA_HD void ba_sym3_mul(const double* Vi, const double* x, double* y) {
    y[0] = Vi[0] * x[0] + Vi[1] * x[1] + Vi[2] * x[2];
    y[1] = Vi[1] * x[0] + Vi[3] * x[1] + Vi[4] * x[2];
    y[2] = Vi[2] * x[0] + Vi[4] * x[1] + Vi[5] * x[2];
}

// S [6][6] -= W_a V^-1 W_b^T of one point seen by edge a (rows) and edge b (columns)
BA_HD void ba_schur_pair(const double* Jca, const double* Jpa, double wa, const double* Jcb, const double* Jpb, double wb, const double* Vi, double* S) {
    double M[2][2];
    for (int n = 0; n < 2; n++) {
        double y[3];
        ba_sym3_mul(Vi, Jpb + n * 3, y);
        for (int m = 0; m < 2; m++) M[m][n] = wa * wb * (Jpa[m * 3] * y[0] + Jpa[m * 3 + 1] * y[1] + Jpa[m * 3 + 2] * y[2]);
    }
    for (int r = 0; r < 6; r++) {
        const double l0 = Jca[r] * M[0][0] + Jca[6 + r] * M[1][0], l1 = Jca[r] * M[0][1] + Jca[6 + r] * M[1][1];
        for (int c = 0; c < 6; c++) S[r * 6 + c] -= l0 * Jcb[c] + l1 * Jcb[6 + c];
    }
}

// b [6] -= W_a V^-1 g_p
BA_HD void ba_schur_rhs(const double* Jca, const double* Jpa, double wa, const double* Vi, const double* gp, double* b) {
    double y[3];
    ba_sym3_mul(Vi, gp, y);
    const double q0 = wa * (Jpa[0] * y[0] + Jpa[1] * y[1] + Jpa[2] * y[2]), q1 = wa * (Jpa[3] * y[0] + Jpa[4] * y[1] + Jpa[5] * y[2]);
    for (int r = 0; r < 6; r++) b[r] -= Jca[r] * q0 + Jca[6 + r] * q1;
}

// back-substitution, one edge in a free keyframe: gp -= W^T d_c
BA_HD void ba_back_edge(const double* Jc, const double* Jp, double w, const double* dc, double* gp) {
    double q0 = 0.0, q1 = 0.0;
    for (int k = 0; k < 6; k++) { q0 += Jc[k] * dc[k]; q1 += Jc[6 + k] * dc[k]; }
    for (int k = 0; k < 3; k++) gp[k] -= w * (Jp[k] * q0 + Jp[3 + k] * q1);
}

// A x = b for the SPD A of order n <= BA_MAX_DIM, packed lower triangle (BA_TRI), overwritten by its Cholesky factor (left-looking:
// every entry is one dot product in k order); false when a pivot is not > 0 or not finite
BA_HD bool ba_chol_factor(int n, double* A) {
    for (int j = 0; j < n; j++) {
        double s = A[BA_TRI(j, j)];
        for (int k = 0; k < j; k++) s -= A[BA_TRI(j, k)] * A[BA_TRI(j, k)];
        if (!(s > 0.0) || !isfinite(s)) return false;
        const double d = sqrt(s);
        A[BA_TRI(j, j)] = d;
        for (int i = j + 1; i < n; i++) {
            double v = A[BA_TRI(i, j)];
            for (int k = 0; k < j; k++) v -= A[BA_TRI(i, k)] * A[BA_TRI(j, k)];
            A[BA_TRI(i, j)] = v / d;
        }
    }
    return true;
}
BA_HD void ba_chol_subst(int n, const double* L, const double* b, double* x) {
    for (int i = 0; i < n; i++) {
        double v = b[i];
        for (int k = 0; k < i; k++) v -= L[BA_TRI(i, k)] * x[k];
        x[i] = v / L[BA_TRI(i, i)];
    }
    for (int i = n - 1; i >= 0; i--) {
        double v = x[i];
        for (int k = i + 1; k < n; k++) v -= L[BA_TRI(k, i)] * x[k];
        x[i] = v / L[BA_TRI(i, i)];
    }
}
BA_HD bool ba_chol_solve(int n, double* A, const double* b, double* x) {
    if (!ba_chol_factor(n, A)) return false;
    ba_chol_subst(n, A, b, x);
    return true;
}

// T' = exp(d) T on SE(3), d = (rho, w), the way pnp_gn_update applies its step
BA_HD void ba_pose_update(const double* d, const double* T, double* T2) {
    double E[9];
    pnp_exp_so3(d + 3, E);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T2[i * 4 + j] = E[i * 3] * T[j] + E[i * 3 + 1] * T[4 + j] + E[i * 3 + 2] * T[8 + j];
        T2[i * 4 + 3] = E[i * 3] * T[3] + E[i * 3 + 1] * T[7] + E[i * 3 + 2] * T[11] + d[i];
    }
}
