// Global bundle adjustment, the pieces beyond ba.h shared by the solver's own kernels (map_gba.hip) and the CPU test of them
// (tests/native/gba_check.cpp): the two halves of the matrix-free Schur operator S p = H p - W V^-1 W^T p, the block-Jacobi
// preconditioner block of one keyframe and its 6x6 factor, and the scalar decisions of the preconditioned conjugate gradient.
// Residual, Jacobians, weights, the point block, its inverse and the back-substitution are ba.h's; the kernels that linearise a point,
// back-substitute, classify and write are ba_problem.h's, the ones the local solver runs.  Everything is f64; built with
// -ffp-contract=off on both sides.
#pragma once
#include "ba.h"

#define GBA_HD BA_HD
#define GBA_TRI_N 21   // packed lower triangle of a 6x6 block (BA_TRI)

// pass (a), one edge into its point: acc [3] += W_e^T p = w J_p^T (J_c p), p [6] the keyframe's part of the vector
GBA_HD void gba_wt_p(const double* Jc, const double* Jp, double w, const double* p, double* acc) {
    double q0 = 0.0, q1 = 0.0;
    for (int k = 0; k < 6; k++) { q0 += Jc[k] * p[k]; q1 += Jc[6 + k] * p[k]; }
    for (int k = 0; k < 3; k++) acc[k] += w * (Jp[k] * q0 + Jp[3 + k] * q1);
}

// pass (b), one edge into its keyframe: acc [6] += W_e q = w J_c^T (J_p q), q [3] the point's V^-1 W^T p
GBA_HD void gba_w_q(const double* Jc, const double* Jp, double w, const double* q, double* acc) {
    const double u0 = w * (Jp[0] * q[0] + Jp[1] * q[1] + Jp[2] * q[2]), u1 = w * (Jp[3] * q[0] + Jp[4] * q[1] + Jp[5] * q[2]);
    for (int r = 0; r < 6; r++) acc[r] += Jc[r] * u0 + Jc[6 + r] * u1;
}

// preconditioner, one edge: M [6][6] -= W_e V^-1 W_e^T, the same-edge term of the Schur complement (ba_schur_pair with both ends the edge)
GBA_HD void gba_precond_edge(const double* Jc, const double* Jp, double w, const double* Vi, double* M) { ba_schur_pair(Jc, Jp, w, Jc, Jp, w, Vi, M); }

// the damped block: Hd = H with every diagonal entry times (1 + lambda), formed as H_ii + lambda H_ii like the local solver's S_ii
GBA_HD void gba_damp6(const double* H, double lambda, double* Hd) {
    for (int k = 0; k < 36; k++) Hd[k] = H[k];
    for (int k = 0; k < 6; k++) Hd[k * 7] = H[k * 7] + lambda * H[k * 7];
}

// Cholesky factor of the 6x6 A [36] (its lower triangle is read) into L [21] (BA_TRI): ba_chol_factor on the packed block
GBA_HD bool gba_factor6(const double* A, double* L) {
    for (int i = 0; i < 6; i++)
        for (int j = 0; j <= i; j++) L[BA_TRI(i, j)] = A[i * 6 + j];
    return ba_chol_factor(6, L);
}
GBA_HD void gba_solve6(const double* L, const double* b, double* x) { ba_chol_subst(6, L, b, x); }

// the factor a keyframe's preconditioner uses: of M = Hd - sum_e W_e V^-1 W_e^T, of Hd when M is not positive definite; 0: M, 1: Hd,
// 2: neither (the vertex is held for the step, L is not to be read)
GBA_HD int gba_precond_factor(const double* M, const double* Hd, double* L) {
    if (gba_factor6(M, L)) return 0;
    if (gba_factor6(Hd, L)) return 1;
    return 2;
}

// y [6] = Hd p for one keyframe, each row in column order
GBA_HD void gba_block_mul(const double* Hd, const double* p, double* y) {
    for (int r = 0; r < 6; r++) {
        double s = 0.0;
        for (int c = 0; c < 6; c++) s += Hd[r * 6 + c] * p[c];
        y[r] = s;
    }
}

// the scalar decisions of the conjugate gradient.  start: 1 iterate, 0 the right side is zero (x = 0 is the solution), -1 r0.z0 is not
// a finite non-negative number (the step counts as rejected)
GBA_HD int gba_cg_start(double rz0) { return rz0 > 0.0 && isfinite(rz0) ? 1 : rz0 == 0.0 ? 0 : -1; }
// alpha = r.z / p.Sp; false when p.Sp is not positive and finite (the solve ends with the x so far)
GBA_HD bool gba_cg_alpha(double rz, double pSp, double* alpha) {
    if (!(pSp > 0.0) || !isfinite(pSp)) return false;
    *alpha = rz / pSp;
    return true;
}
// after an iteration: true to go on (beta = rzn / rz), false at r.z <= cg_tol^2 r0.z0
GBA_HD bool gba_cg_continue(double rzn, double cg_tol2, double rz0, double rz, double* beta) {
    if (!(rzn > cg_tol2 * rz0)) return false;
    *beta = rzn / rz;
    return true;
}
