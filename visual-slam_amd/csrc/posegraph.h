// Pose graph on Sim(3), the pieces shared by the kernels (map_posegraph.hip), the CPU test of them (tests/native/posegraph_check.cpp)
// and the host replay of the whole optimisation (tests/native/posegraph_replay.cpp): the logarithm of a rotation, the composition of
// similarities, the residual of an edge and its two Jacobians, the 7x7 block operations of the solver, the fixed-order sums.
// ORB-SLAM2's Optimizer::OptimizeEssentialGraph (monocular: the scale is free).  Everything is f64; built with -ffp-contract=off on both
// sides, so a host build differs from the device only in what libm returns.  Every libm call goes through the PG_* macros below and
// nothing else in this file rounds differently on the two sides (sqrt and the arithmetic are correctly rounded): a host build with
// -DPG_LIBM_NUDGE moves every PG_* result by PG_NUDGE_ULP units in the last place, the direction alternating per call, and the
// difference between the two host builds bounds what another libm may do to a result (tests/posegraph_cases.py: LIBM_SPREAD).
//
// Conventions (sim3.h, ba.h): a vertex is a similarity S = (s, R, t), X_cam = s R X + t.  The retraction is sim3_gn_update's:
// delta = (rho, w, lambda), S' = D(delta) o S with s' = e^lambda s, R' = exp(w) R, t' = e^lambda exp(w) t + rho.  An edge (a, b) carries
// M_ba, which should equal S_b o S_a^-1; its residual is the 7-vector (t_E, log_so3(R_E), ln s_E) of E = M_ba o S_a o S_b^-1.  The
// information matrix is the identity.
//
// Jacobians, analytic.  To first order D(delta) o M = M o D(Ad_M^-1 delta), so a step on S_a turns E into D(Ad_M delta) o E and a step
// on S_b turns it into E o D(-delta) = D(-Ad_E delta) o E.  With L(E) = d residual(D(eps) o E) / d eps at 0,
//   J_a = L(E) Ad_M,  J_b = -L(E) Ad_E,
//   Ad_(s,R,t) (rho, w, lambda) = (s R rho + t x (R w) - lambda t,  R w,  lambda),
//   L(E) = [ I  -[t_E]x  t_E ;  0  Jl^-1(phi)  0 ;  0  0  1 ],  phi = log_so3(R_E),
//   Jl^-1(phi) = I - [phi]x / 2 + c [phi]x^2,  c = 1 / theta^2 - cos(theta / 2) / (2 theta sin(theta / 2))  (1 / 12 below PG_SMALL):
// the half-angle form has no pole at pi.
#pragma once
#include "sim3.h"

#define PG_HD SIM3_HD
#define PG_SMALL 1e-6        // below this angle the series of exp / log / Jl^-1 are exact to f64
#define PG_NEAR_PI 1e-3      // within this of pi the axis comes from the symmetric part of R
#define PG_NUDGE_ULP 2       // the ROCm install documents no f64 error table: 2 units for every function

#if defined(PG_LIBM_NUDGE) && !defined(__HIP_DEVICE_COMPILE__)
#include <cmath>
inline double pg_nudge(double v) {
    static int calls = 0;
    const double to = (calls++ & 1) ? INFINITY : -INFINITY;
    for (int i = 0; i < PG_NUDGE_ULP; i++) v = std::nextafter(v, to);
    return v;
}
#define PG_SIN(x) pg_nudge(sin(x))
#define PG_COS(x) pg_nudge(cos(x))
#define PG_EXP(x) pg_nudge(exp(x))
#define PG_LOG(x) pg_nudge(log(x))
#define PG_ATAN2(y, x) pg_nudge(atan2(y, x))
#else
#define PG_SIN(x) sin(x)
#define PG_COS(x) cos(x)
#define PG_EXP(x) exp(x)
#define PG_LOG(x) log(x)
#define PG_ATAN2(y, x) atan2(y, x)
#endif

// ---- rotations -----------------------------------------------------------------------------------------------------------------------
// E = exp([w]x) (pnp_exp_so3's form, its libm calls through the macros)
PG_HD void pg_exp_so3(const double* w, double* E) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
    double a, b;
    if (th < PG_SMALL) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; }
    else { a = PG_SIN(th) / th; b = (1.0 - PG_COS(th)) / th2; }
    const double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double W2 = W[i * 3] * W[j] + W[i * 3 + 1] * W[3 + j] + W[i * 3 + 2] * W[6 + j];
            E[i * 3 + j] = (i == j ? 1.0 : 0.0) + a * W[i * 3 + j] + b * W2;
        }
}

// w = log(R), |w| in [0, pi].  v = vee(R - R^T) / 2 = sin(theta) axis, c = (trace - 1) / 2 = cos(theta), theta = atan2(|v|, c).
//   small angle (|v| < PG_SMALL, c > 0): w = v (1 + |v|^2 / 6): theta / sin(theta) to second order
//   near pi (theta > pi - PG_NEAR_PI): sin(theta) is too small to carry the axis; from R = c I + sin [a]x + (1 - c) a a^T the largest
//     a_k^2 = (R_kk - c) / (1 - c), the other two components from the symmetric part (R_kj + R_jk) / (2 (1 - c) a_k), and the sign of
//     the axis from v (at exactly pi, where v = 0, the positive a_k)
//   otherwise w = v theta / |v|
PG_HD void pg_log_so3(const double* R, double* w) {
    const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    const double sn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (sn < PG_SMALL && c > 0.0) {
        const double k = 1.0 + sn * sn / 6.0;
        w[0] = k * v[0]; w[1] = k * v[1]; w[2] = k * v[2];
        return;
    }
    const double th = PG_ATAN2(sn, c);
    if (th > 3.14159265358979323846 - PG_NEAR_PI) {
        const double d = 1.0 - c;
        int k = 0;
        if (R[4] > R[0]) k = 1;
        if (R[8] > R[k * 4]) k = 2;
        const int j = (k + 1) % 3, l = (k + 2) % 3;
        double a[3];
        a[k] = sqrt(fmax((R[k * 4] - c) / d, 0.0));
        a[j] = (R[k * 3 + j] + R[j * 3 + k]) / (2.0 * d * a[k]);
        a[l] = (R[k * 3 + l] + R[l * 3 + k]) / (2.0 * d * a[k]);
        const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        const double sg = a[0] * v[0] + a[1] * v[1] + a[2] * v[2] < 0.0 ? -1.0 : 1.0;
        for (int i = 0; i < 3; i++) w[i] = sg * th * a[i] / n;
        return;
    }
    const double k = th / sn;
    w[0] = k * v[0]; w[1] = k * v[1]; w[2] = k * v[2];
}

// J = Jl^-1(phi), row-major 3x3
PG_HD void pg_jl_inv(const double* p, double* J) {
    const double th2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2], th = sqrt(th2);
    double c;
    if (th < PG_SMALL) c = 1.0 / 12.0;
    else { const double h = 0.5 * th; c = 1.0 / th2 - PG_COS(h) / (2.0 * th * PG_SIN(h)); }
    const double W[9] = {0, -p[2], p[1], p[2], 0, -p[0], -p[1], p[0], 0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double W2 = W[i * 3] * W[j] + W[i * 3 + 1] * W[3 + j] + W[i * 3 + 2] * W[6 + j];
            J[i * 3 + j] = (i == j ? 1.0 : 0.0) - 0.5 * W[i * 3 + j] + c * W2;
        }
}

// ---- similarities --------------------------------------------------------------------------------------------------------------------
// C = A o B: X -> A (B X); each row summed left to right.  C may not alias A or B.
PG_HD void pg_compose(const Sim3& A, const Sim3& B, Sim3& C) {
    C.s = A.s * B.s;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) C.R[i * 3 + j] = A.R[i * 3] * B.R[j] + A.R[i * 3 + 1] * B.R[3 + j] + A.R[i * 3 + 2] * B.R[6 + j];
        C.t[i] = A.s * (A.R[i * 3] * B.t[0] + A.R[i * 3 + 1] * B.t[1] + A.R[i * 3 + 2] * B.t[2]) + A.t[i];
    }
}

// the measurement of an edge (a, b) from the two ends: M = S_b o S_a^-1
PG_HD void pg_measure(const Sim3& Sa, const Sim3& Sb, Sim3& M) {
    Sim3 I;
    sim3_inverse(Sa, I);
    pg_compose(Sb, I, M);
}

// S' = D(d) o S, sim3_gn_update's retraction
PG_HD void pg_retract(const double* d, const Sim3& S, Sim3& T) {
    double E[9];
    pg_exp_so3(d + 3, E);
    const double el = PG_EXP(d[6]);
    T.s = el * S.s;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T.R[i * 3 + j] = E[i * 3] * S.R[j] + E[i * 3 + 1] * S.R[3 + j] + E[i * 3 + 2] * S.R[6 + j];
        T.t[i] = el * (E[i * 3] * S.t[0] + E[i * 3 + 1] * S.t[1] + E[i * 3 + 2] * S.t[2]) + d[i];
    }
}

PG_HD void pg_load(const double* p, Sim3& S) {
    S.s = p[0];
    for (int i = 0; i < 9; i++) S.R[i] = p[1 + i];
    for (int i = 0; i < 3; i++) S.t[i] = p[10 + i];
}
PG_HD void pg_store(const Sim3& S, double* p) {
    p[0] = S.s;
    for (int i = 0; i < 9; i++) p[1 + i] = S.R[i];
    for (int i = 0; i < 3; i++) p[10 + i] = S.t[i];
}

// ---- the edge ------------------------------------------------------------------------------------------------------------------------
// E = M o S_a o S_b^-1 and r = (t_E, log_so3(R_E), ln s_E)
PG_HD void pg_error(const Sim3& M, const Sim3& Sa, const Sim3& Sb, Sim3& E, double* r) {
    Sim3 I, Q;
    sim3_inverse(Sb, I);
    pg_compose(Sa, I, Q);
    pg_compose(M, Q, E);
    r[0] = E.t[0]; r[1] = E.t[1]; r[2] = E.t[2];
    pg_log_so3(E.R, r + 3);
    r[6] = PG_LOG(E.s);
}
PG_HD void pg_residual(const Sim3& M, const Sim3& Sa, const Sim3& Sb, double* r) {
    Sim3 E;
    pg_error(M, Sa, Sb, E, r);
}
PG_HD double pg_cost(const double* r) {
    double c = 0.0;
    for (int k = 0; k < 7; k++) c += r[k] * r[k];
    return c;
}

// A = Ad_S, row-major 7x7 on (rho, w, lambda)
PG_HD void pg_adjoint(const Sim3& S, double* A) {
    for (int i = 0; i < 49; i++) A[i] = 0.0;
    const double* t = S.t;
    const double T[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            A[i * 7 + j] = S.s * S.R[i * 3 + j];
            A[i * 7 + 3 + j] = T[i * 3] * S.R[j] + T[i * 3 + 1] * S.R[3 + j] + T[i * 3 + 2] * S.R[6 + j];
            A[(3 + i) * 7 + 3 + j] = S.R[i * 3 + j];
        }
        A[i * 7 + 6] = -t[i];
    }
    A[48] = 1.0;
}

// C = A B, 7x7 row-major, every entry summed in k order; sign * the product
PG_HD void pg_mul77(const double* A, const double* B, double sign, double* C) {
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) {
            double v = 0.0;
            for (int k = 0; k < 7; k++) v += A[i * 7 + k] * B[k * 7 + j];
            C[i * 7 + j] = sign * v;
        }
}

// residual and both Jacobians (row-major 7x7: d r / d delta_a, d r / d delta_b) of one edge
PG_HD void pg_linearize(const Sim3& M, const Sim3& Sa, const Sim3& Sb, double* r, double* Ja, double* Jb) {
    Sim3 E;
    pg_error(M, Sa, Sb, E, r);
    double L[49], Jl[9], A[49];
    for (int i = 0; i < 49; i++) L[i] = 0.0;
    pg_jl_inv(r + 3, Jl);
    const double* t = E.t;
    const double T[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
    for (int i = 0; i < 3; i++) {
        L[i * 7 + i] = 1.0;
        for (int j = 0; j < 3; j++) { L[i * 7 + 3 + j] = -T[i * 3 + j]; L[(3 + i) * 7 + 3 + j] = Jl[i * 3 + j]; }
        L[i * 7 + 6] = t[i];
    }
    L[48] = 1.0;
    pg_adjoint(M, A);
    pg_mul77(L, A, 1.0, Ja);
    pg_adjoint(E, A);
    pg_mul77(L, A, -1.0, Jb);
}

// ---- 7x7 blocks of the solver ----------------------------------------------------------------------------------------------------------
// entry (i, j) of A^T B
PG_HD double pg_atb_entry(const double* A, const double* B, int i, int j) {
    double v = 0.0;
    for (int k = 0; k < 7; k++) v += A[k * 7 + i] * B[k * 7 + j];
    return v;
}
// entry i of A^T r
PG_HD double pg_atr_entry(const double* A, const double* r, int i) {
    double v = 0.0;
    for (int k = 0; k < 7; k++) v += A[k * 7 + i] * r[k];
    return v;
}
// entry i of A x (t = false) or A^T x (t = true)
PG_HD double pg_mulv_entry(const double* A, const double* x, int i, bool t) {
    double v = 0.0;
    for (int k = 0; k < 7; k++) v += (t ? A[k * 7 + i] : A[i * 7 + k]) * x[k];
    return v;
}
// the Cholesky factor L (lower, row-major 7x7, the upper part zero) of the SPD block H with its diagonal times damp; false when a pivot
// is not > 0 or not finite (L is then not to be used)
PG_HD bool pg_chol7(const double* H, double damp, double* L) {
    for (int i = 0; i < 49; i++) L[i] = 0.0;
    for (int j = 0; j < 7; j++) {
        double s = H[j * 7 + j] * damp;
        for (int k = 0; k < j; k++) s -= L[j * 7 + k] * L[j * 7 + k];
        if (!(s > 0.0) || !isfinite(s)) return false;
        const double d = sqrt(s);
        L[j * 7 + j] = d;
        for (int i = j + 1; i < 7; i++) {
            double v = H[i * 7 + j];
            for (int k = 0; k < j; k++) v -= L[i * 7 + k] * L[j * 7 + k];
            L[i * 7 + j] = v / d;
        }
    }
    return true;
}
// x = (L L^T)^-1 b
PG_HD void pg_chol7_solve(const double* L, const double* b, double* x) {
    double z[7];
    for (int i = 0; i < 7; i++) {
        double v = b[i];
        for (int k = 0; k < i; k++) v -= L[i * 7 + k] * z[k];
        z[i] = v / L[i * 7 + i];
    }
    for (int i = 6; i >= 0; i--) {
        double v = z[i];
        for (int k = i + 1; k < 7; k++) v -= L[k * 7 + i] * x[k];
        x[i] = v / L[i * 7 + i];
    }
}

// ---- the fixed summation order of a 1024-thread workgroup, as a host loop ---------------------------------------------------------------
// Thread t adds the elements t, t + PG_THREADS, ... in order; a wave's 64 partial sums fold as wave_sum's shuffle tree does in lane 0
// (v[l] += v[l + d], d = 32 .. 1); the 16 waves are added in order.  The device does this with its threads (block_sum of
// map_store.h); the replay calls this.
#define PG_THREADS 1024
#if !defined(__HIP_DEVICE_COMPILE__)
template <class F> inline double pg_tree_sum(int n, F f) {
    static double part[PG_THREADS];
    for (int t = 0; t < PG_THREADS; t++) {
        double s = 0.0;
        for (int i = t; i < n; i += PG_THREADS) s += f(i);
        part[t] = s;
    }
    double total = 0.0;
    for (int w = 0; w < PG_THREADS / 64; w++) {
        double* v = part + w * 64;
        for (int d = 32; d; d >>= 1)
            for (int l = 0; l < d; l++) v[l] += v[l + d];
        total = w == 0 ? v[0] : total + v[0];
    }
    return total;
}
#endif
