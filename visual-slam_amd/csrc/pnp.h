// Absolute pose from 2D-3D correspondences, shared by the relocalization kernels (map_reloc.hip) and the CPU test of the solver
// (tests/native/pnp_check.cpp): the sampling stream, a P3P solver, the reprojection test and one Gauss-Newton step on SE(3).
// Everything is f64; built with -ffp-contract=off on both sides, so a host build computes what the device computes.
//
// Pose convention: X_cam = R X + t, projection P = K [R | t] (orbslam2.utils.compute_projection_matrix).
//
// P3P (Grunert's distances, closed by a resultant): with unit bearings y_i, distances s_i and the cosines c_ij = y_i . y_j, the law of
// cosines gives s_i^2 + s_j^2 - 2 s_i s_j c_ij = a_ij (squared world distances).  With u = s2 / s1, v = s3 / s1 and s1 eliminated, two
// quadratics in u remain whose coefficients are polynomials in v:
//   A: a13 u^2 - 2 a13 c12 u + (a13 - a12 + 2 a12 c13 v - a12 v^2) = 0
//   B: (a23 - a12) u^2 + (2 a12 c23 v - 2 a23 c12) u + (a23 - a12 v^2) = 0
// Their Sylvester resultant is a quartic in v; every real root v > 0 gives u = -g(v) / h(v) (the combination a2 B - b2 A is linear in
// u), s1 from the first equation, and the three camera-frame points.  The distances are polished by Newton on the three equations and
// R, t follow from the two point triangles.  The quartic's real roots are bracketed between the roots of its derivatives (degree 1
// up to 4) and found by safeguarded Newton: no closed-form cubic or quartic formula, no complex arithmetic.  Degenerate samples
// (coincident or collinear world points, coincident bearings, a non-finite input) give 0 roots.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define PNP_HD __host__ __device__ __forceinline__
#else
#define PNP_HD inline
#endif

// ---- sampling: the draw-and-redraw scheme of twoview_kernels.hip:sample8 for N indices -------------------------------------------
// c = splitmix64 % m, redrawn while it repeats an earlier index; the stream of hypothesis h starts at seed + (h + 1) * golden.
// (sample8 takes the same remainder through 32-bit reductions; the value is the same.)  m >= N.
PNP_HD uint64_t pnp_splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the stream of keyframe position k (relocalization) = the stream of pair k of the two-view stage
PNP_HD uint64_t pnp_stream_seed(uint64_t seed, int k) { return seed + (uint64_t)k * 0x632BE59BD9B4E019ull; }

template <int N> PNP_HD void pnp_sample(uint64_t seed, int h, int m, int (&idx)[N]) {
    uint64_t s = seed + (uint64_t)(h + 1) * 0xD1B54A32D192ED03ull;
    for (int k = 0; k < N; k++) {
        int c;
        bool dup;
        do {
            c = (int)(pnp_splitmix64(s) % (uint64_t)m);
            dup = false;
            for (int j = 0; j < k; j++) dup |= idx[j] == c;
        } while (dup);
        idx[k] = c;
    }
}

// ---- small vector helpers --------------------------------------------------------------------------------------------------------
PNP_HD double pnp_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PNP_HD void pnp_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
PNP_HD bool pnp_unit(double* a) {
    const double n = sqrt(pnp_dot(a, a));
    if (!(n > 0.0) || !isfinite(n)) return false;
    a[0] /= n; a[1] /= n; a[2] /= n;
    return true;
}

// A x = b for a 3x3 A (row-major) by Cramer's rule; false when A is singular
PNP_HD bool pnp_solve3(const double* A, const double* b, double* x) {
    const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
    const double det = A[0] * c0 + A[1] * c1 + A[2] * c2;
    if (!(fabs(det) > 1e-300) || !isfinite(det)) return false;
    x[0] = (b[0] * c0 + A[1] * (A[5] * b[2] - b[1] * A[8]) + A[2] * (b[1] * A[7] - A[4] * b[2])) / det;
    x[1] = (A[0] * (b[1] * A[8] - A[5] * b[2]) + b[0] * c1 + A[2] * (A[3] * b[2] - b[1] * A[6])) / det;
    x[2] = (A[0] * (A[4] * b[2] - b[1] * A[7]) + A[1] * (b[1] * A[6] - A[3] * b[2]) + b[0] * c2) / det;
    return true;
}

// residuals of s_i^2 + s_j^2 - 2 s_i s_j c_ij = a_ij for (1, 2), (1, 3), (2, 3); returns their L1 norm
PNP_HD double pnp_cosine_resid(const double* q, double c12, double c13, double c23, double a12, double a13, double a23, double* e) {
    e[0] = q[0] * q[0] + q[1] * q[1] - 2.0 * q[0] * q[1] * c12 - a12;
    e[1] = q[0] * q[0] + q[2] * q[2] - 2.0 * q[0] * q[2] * c13 - a13;
    e[2] = q[1] * q[1] + q[2] * q[2] - 2.0 * q[1] * q[2] * c23 - a23;
    return fabs(e[0]) + fabs(e[1]) + fabs(e[2]);
}

// ---- real roots of a polynomial of degree <= 4 in [lo, hi] --------------------------------------------------------------------
PNP_HD double pnp_poly(const double* c, int n, double x) {
    double v = c[n];
    for (int i = n - 1; i >= 0; i--) v = v * x + c[i];
    return v;
}

// the one root of c in [a, b] where c(a), c(b) differ in sign (or one is 0): Newton inside the bracket, bisection when it leaves it
PNP_HD double pnp_bracket_root(const double* c, const double* d, int n, double a, double b) {
    double fa = pnp_poly(c, n, a), fb = pnp_poly(c, n, b);
    if (fa == 0.0) return a;
    if (fb == 0.0) return b;
    double x = 0.5 * (a + b);
    for (int it = 0; it < 200; it++) {
        const double fx = pnp_poly(c, n, x);
        if (fx == 0.0) return x;
        if ((fx < 0.0) == (fa < 0.0)) { a = x; fa = fx; } else { b = x; fb = fx; }
        const double dx = pnp_poly(d, n - 1, x);
        double xn = dx != 0.0 ? x - fx / dx : 0.5 * (a + b);
        if (!(xn > a && xn < b)) xn = 0.5 * (a + b);
        if (xn == x || b - a <= 4e-16 * fabs(x)) return xn;
        x = xn;
    }
    return x;
}

// roots of c[0] + c[1] x + ... + c[n] x^n (c[n] != 0, n <= 4) in [lo, hi], ascending; returns their number
PNP_HD int pnp_poly_roots(const double* c0, int n, double lo, double hi, double* roots) {
    // derivative chain: dc[k] = coefficients of the (n - k)-th derivative, degree k
    double dc[5][5];
    for (int i = 0; i <= n; i++) dc[n][i] = c0[i];
    for (int k = n - 1; k >= 1; k--)
        for (int i = 0; i <= k; i++) dc[k][i] = dc[k + 1][i + 1] * (double)(i + 1);
    double r[4];
    int nr = 0;
    // degree 1
    {
        const double x = -dc[1][0] / dc[1][1];
        if (x > lo && x < hi) r[nr++] = x;
    }
    for (int k = 2; k <= n; k++) {
        // the roots of the derivative (in r) split [lo, hi] into monotone pieces
        double e[6];
        int ne = 0;
        e[ne++] = lo;
        for (int i = 0; i < nr; i++) e[ne++] = r[i];
        e[ne++] = hi;
        double nrr[4];
        int nn = 0;
        for (int i = 0; i + 1 < ne; i++) {
            const double fa = pnp_poly(dc[k], k, e[i]), fb = pnp_poly(dc[k], k, e[i + 1]);
            if (fa == 0.0 && i > 0) continue;  // counted as the right end of the previous piece
            if ((fa < 0.0) != (fb < 0.0) || fa == 0.0 || fb == 0.0) {
                const double x = pnp_bracket_root(dc[k], dc[k - 1], k, e[i], e[i + 1]);
                if (nn == 0 || x > nrr[nn - 1]) nrr[nn++] = x;
            }
        }
        nr = nn;
        for (int i = 0; i < nn; i++) r[i] = nrr[i];
    }
    for (int i = 0; i < nr; i++) roots[i] = r[i];
    return nr;
}

// ---- P3P -------------------------------------------------------------------------------------------------------------------------
// X: world points [3][3]; b: bearings [3][3] (any positive scale: K^-1 (x, y, 1)).  Up to 4 poses R (row-major [9]), t [3].
PNP_HD int pnp_p3p(const double (&X)[3][3], const double (&b)[3][3], double (&R)[4][9], double (&t)[4][3]) {
    double y[3][3];
    for (int i = 0; i < 3; i++) {
        for (int k = 0; k < 3; k++) y[i][k] = b[i][k];
        if (!pnp_unit(y[i])) return 0;
        for (int k = 0; k < 3; k++) if (!isfinite(X[i][k])) return 0;
    }
    double d12[3], d13[3], d23[3];
    for (int k = 0; k < 3; k++) { d12[k] = X[0][k] - X[1][k]; d13[k] = X[0][k] - X[2][k]; d23[k] = X[1][k] - X[2][k]; }
    const double a12 = pnp_dot(d12, d12), a13 = pnp_dot(d13, d13), a23 = pnp_dot(d23, d23);
    double cr[3];
    pnp_cross(d12, d13, cr);
    if (!(pnp_dot(cr, cr) > 1e-18 * a12 * a13) || !(a12 > 0.0)) return 0;  // coincident or collinear points
    const double c12 = pnp_dot(y[0], y[1]), c13 = pnp_dot(y[0], y[2]), c23 = pnp_dot(y[1], y[2]);
    for (int i = 0; i < 3; i++) {  // coincident bearings (|y_i x y_j| = sin of their angle)
        double yc[3];
        pnp_cross(y[i], y[(i + 1) % 3], yc);
        if (!(pnp_dot(yc, yc) > 1e-18)) return 0;
    }
    // scaled so that a12 = 1
    const double A13 = a13 / a12, A23 = a23 / a12;
    const double p2 = A13, p1 = -2.0 * A13 * c12;
    const double p0[3] = {A13 - 1.0, 2.0 * c13, -1.0};
    const double q2 = A23 - 1.0;
    const double q1[2] = {-2.0 * A23 * c12, 2.0 * c23};
    const double q0[3] = {A23, 0.0, -1.0};
    // g = p2 q0 - q2 p0, h = p2 q1 - q2 p1, k = p1 q0 - p0 q1; resultant = g^2 - h k
    double g[3], h[2], kk[4];
    for (int i = 0; i < 3; i++) g[i] = p2 * q0[i] - q2 * p0[i];
    h[0] = p2 * q1[0] - q2 * p1; h[1] = p2 * q1[1];
    for (int i = 0; i < 4; i++) kk[i] = 0.0;
    for (int i = 0; i < 3; i++) kk[i] += p1 * q0[i];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 2; j++) kk[i + j] -= p0[i] * q1[j];
    double quart[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) quart[i + j] += g[i] * g[j];
    for (int i = 0; i < 2; i++) for (int j = 0; j < 4; j++) quart[i + j] -= h[i] * kk[j];
    int n = 4;
    double mx = 0.0;
    for (int i = 0; i <= 4; i++) mx = fmax(mx, fabs(quart[i]));
    if (!(mx > 0.0) || !isfinite(mx)) return 0;
    while (n > 0 && fabs(quart[n]) <= 1e-14 * mx) n--;
    if (n == 0) return 0;
    double bound = 0.0;  // Cauchy bound of the roots
    for (int i = 0; i < n; i++) bound = fmax(bound, fabs(quart[i] / quart[n]));
    double vr[4];
    const int nv = pnp_poly_roots(quart, n, 0.0, 1.0 + bound, vr);
    int out = 0;
    for (int r = 0; r < nv; r++) {
        const double v = vr[r];
        if (!(v > 0.0)) continue;
        const double hv = h[0] + h[1] * v, gv = g[0] + (g[1] + g[2] * v) * v;
        if (!(fabs(hv) > 1e-12 * (fabs(h[0]) + fabs(h[1] * v) + 1e-300))) continue;
        const double u = -gv / hv;
        if (!(u > 0.0)) continue;
        const double f1 = 1.0 + u * u - 2.0 * u * c12;
        if (!(f1 > 0.0)) continue;
        double s[3];
        s[0] = sqrt(a12 / f1); s[1] = u * s[0]; s[2] = v * s[0];
        // Newton on the three law-of-cosine equations (kept only while the residual falls)
        double e[3];
        double res = pnp_cosine_resid(s, c12, c13, c23, a12, a13, a23, e);
        for (int it = 0; it < 4 && res > 0.0; it++) {
            const double J[9] = {2.0 * (s[0] - s[1] * c12), 2.0 * (s[1] - s[0] * c12), 0.0,
                                 2.0 * (s[0] - s[2] * c13), 0.0, 2.0 * (s[2] - s[0] * c13),
                                 0.0, 2.0 * (s[1] - s[2] * c23), 2.0 * (s[2] - s[1] * c23)};
            double d[3];
            if (!pnp_solve3(J, e, d)) break;
            double s2[3] = {s[0] - d[0], s[1] - d[1], s[2] - d[2]}, e2[3];
            const double r2 = pnp_cosine_resid(s2, c12, c13, c23, a12, a13, a23, e2);
            if (!(r2 < res)) break;
            for (int k = 0; k < 3; k++) { s[k] = s2[k]; e[k] = e2[k]; }
            res = r2;
        }
        if (!(s[0] > 0.0 && s[1] > 0.0 && s[2] > 0.0)) continue;
        double C[3][3];
        for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) C[i][k] = s[i] * y[i][k];
        // orthonormal frames of the two triangles: columns e1 = P2 - P1, e3 = e1 x (P3 - P1), e2 = e3 x e1
        double fw[3][3], fc[3][3];
        {
            double a[3], bb[3];
            for (int k = 0; k < 3; k++) { a[k] = X[1][k] - X[0][k]; bb[k] = X[2][k] - X[0][k]; }
            double c3[3];
            pnp_cross(a, bb, c3);
            if (!pnp_unit(a) || !pnp_unit(c3)) continue;
            double c2[3];
            pnp_cross(c3, a, c2);
            for (int k = 0; k < 3; k++) { fw[k][0] = a[k]; fw[k][1] = c2[k]; fw[k][2] = c3[k]; }
        }
        {
            double a[3], bb[3];
            for (int k = 0; k < 3; k++) { a[k] = C[1][k] - C[0][k]; bb[k] = C[2][k] - C[0][k]; }
            double c3[3];
            pnp_cross(a, bb, c3);
            if (!pnp_unit(a) || !pnp_unit(c3)) continue;
            double c2[3];
            pnp_cross(c3, a, c2);
            for (int k = 0; k < 3; k++) { fc[k][0] = a[k]; fc[k][1] = c2[k]; fc[k][2] = c3[k]; }
        }
        double* Ro = R[out];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) Ro[i * 3 + j] = fc[i][0] * fw[j][0] + fc[i][1] * fw[j][1] + fc[i][2] * fw[j][2];
        bool fin = true;
        for (int i = 0; i < 3; i++) {
            double m = 0.0;
            for (int k = 0; k < 3; k++) m += (C[k][i] - (Ro[i * 3] * X[k][0] + Ro[i * 3 + 1] * X[k][1] + Ro[i * 3 + 2] * X[k][2]));
            t[out][i] = m / 3.0;
            fin &= isfinite(t[out][i]);
        }
        for (int i = 0; i < 9; i++) fin &= isfinite(Ro[i]);
        if (fin) out++;
    }
    return out;
}

// ---- projection and the inlier test ------------------------------------------------------------------------------------------
// P = K [R | t], each entry K[i][0] M[0][j] + K[i][1] M[1][j] + K[i][2] M[2][j]
PNP_HD void pnp_projection(const double* K, const double* R, const double* t, double* P) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) {
            const double m0 = j < 3 ? R[j] : t[0], m1 = j < 3 ? R[3 + j] : t[1], m2 = j < 3 ? R[6 + j] : t[2];
            P[i * 4 + j] = K[i * 3] * m0 + K[i * 3 + 1] * m1 + K[i * 3 + 2] * m2;
        }
}

// P X_h (each row summed left to right), then the squared pixel error; false when the depth is not > 0
PNP_HD bool pnp_reproj2(const double* P, double X, double Y, double Z, double x, double y, double* e2) {
    const double u = P[0] * X + P[1] * Y + P[2] * Z + P[3];
    const double v = P[4] * X + P[5] * Y + P[6] * Z + P[7];
    const double z = P[8] * X + P[9] * Y + P[10] * Z + P[11];
    const double du = u / z - x, dv = v / z - y;
    *e2 = du * du + dv * dv;
    return z > 0.0;
}

// ---- Gauss-Newton on SE(3) ------------------------------------------------------------------------------------------------------
// Left perturbation X_cam' = exp(w) X_cam + rho, delta = (rho, w): R' = exp(w) R, t' = exp(w) t + rho.  H is the upper triangle of
// J^T J (row-major, 21 entries), g = J^T r with r = projection - observation.
// Weighted form (tracking's pose refinement): each term times info * w, w = the Huber weight sqrt(huber2 / e2) when
// e2 = info * |r|^2 exceeds huber2 > 0, else 1.  info = 1, huber2 = 0 is the unweighted sum (a product by 1.0 is exact).
PNP_HD void pnp_gn_accumulate_w(const double* K, const double* R, const double* t, double X, double Y, double Z, double x, double y,
                                double info, double huber2, double* H, double* g) {
    const double xc = R[0] * X + R[1] * Y + R[2] * Z + t[0];
    const double yc = R[3] * X + R[4] * Y + R[5] * Z + t[1];
    const double zc = R[6] * X + R[7] * Y + R[8] * Z + t[2];
    const double p0 = K[0] * xc + K[1] * yc + K[2] * zc, p1 = K[3] * xc + K[4] * yc + K[5] * zc, p2 = K[6] * xc + K[7] * yc + K[8] * zc;
    if (!(p2 != 0.0)) return;
    const double iz = 1.0 / p2, iz2 = iz * iz;
    const double ru = p0 * iz - x, rv = p1 * iz - y;
    // d(u, v) / d X_cam
    double du[3], dv[3];
    for (int k = 0; k < 3; k++) { du[k] = (K[k] * p2 - p0 * K[6 + k]) * iz2; dv[k] = (K[3 + k] * p2 - p1 * K[6 + k]) * iz2; }
    // d X_cam / d rho = I, d X_cam / d w = -[X_cam]x
    const double c[3] = {xc, yc, zc};
    double Ju[6], Jv[6];
    for (int k = 0; k < 3; k++) { Ju[k] = du[k]; Jv[k] = dv[k]; }
    // -[c]x = [[0, c2, -c1], [-c2, 0, c0], [c1, -c0, 0]]; J_w = d . (-[c]x)
    Ju[3] = -du[1] * c[2] + du[2] * c[1]; Ju[4] = du[0] * c[2] - du[2] * c[0]; Ju[5] = -du[0] * c[1] + du[1] * c[0];
    Jv[3] = -dv[1] * c[2] + dv[2] * c[1]; Jv[4] = dv[0] * c[2] - dv[2] * c[0]; Jv[5] = -dv[0] * c[1] + dv[1] * c[0];
    const double e2 = info * (ru * ru + rv * rv);
    const double wt = huber2 > 0.0 && e2 > huber2 ? info * (sqrt(huber2) / sqrt(e2)) : info;
    int o = 0;
    for (int i = 0; i < 6; i++) {
        for (int j = i; j < 6; j++) H[o++] += wt * (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
        g[i] += wt * (Ju[i] * ru + Jv[i] * rv);
    }
}

PNP_HD void pnp_gn_accumulate(const double* K, const double* R, const double* t, double X, double Y, double Z, double x, double y,
                              double* H, double* g) {
    pnp_gn_accumulate_w(K, R, t, X, Y, Z, x, y, 1.0, 0.0, H, g);
}

PNP_HD void pnp_exp_so3(const double* w, double* E) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
    double a, b;
    if (th < 1e-8) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; }
    else { a = sin(th) / th; b = (1.0 - cos(th)) / th2; }
    const double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double W2 = W[i * 3] * W[j] + W[i * 3 + 1] * W[3 + j] + W[i * 3 + 2] * W[6 + j];
            E[i * 3 + j] = (i == j ? 1.0 : 0.0) + a * W[i * 3 + j] + b * W2;
        }
}

// solve H delta = -g (Cholesky) and apply it; false (pose unchanged) when H is not positive definite.  *step = |delta|.
PNP_HD bool pnp_gn_update(const double* H, const double* g, double* R, double* t, double* step) {
    double L[6][6];
    int o = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) { L[j][i] = H[o]; L[i][j] = H[o]; o++; }
    for (int j = 0; j < 6; j++) {
        double s = L[j][j];
        for (int k = 0; k < j; k++) s -= L[j][k] * L[j][k];
        if (!(s > 0.0) || !isfinite(s)) return false;
        L[j][j] = sqrt(s);
        for (int i = j + 1; i < 6; i++) {
            double v = L[i][j];
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    double z[6], d[6];
    for (int i = 0; i < 6; i++) {
        double v = -g[i];
        for (int k = 0; k < i; k++) v -= L[i][k] * z[k];
        z[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; i--) {
        double v = z[i];
        for (int k = i + 1; k < 6; k++) v -= L[k][i] * d[k];
        d[i] = v / L[i][i];
    }
    double E[9];
    pnp_exp_so3(d + 3, E);
    double R2[9], t2[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R2[i * 3 + j] = E[i * 3] * R[j] + E[i * 3 + 1] * R[3 + j] + E[i * 3 + 2] * R[6 + j];
        t2[i] = E[i * 3] * t[0] + E[i * 3 + 1] * t[1] + E[i * 3 + 2] * t[2] + d[i];
    }
    for (int i = 0; i < 9; i++) R[i] = R2[i];
    for (int i = 0; i < 3; i++) t[i] = t2[i];
    *step = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
    return true;
}
