// Host check of the relocalization solver (visual-slam_amd/csrc/pnp.h), built with g++ -ffp-contract=off.
//   p3p <n> <seed>      n random well-conditioned poses and triplets: one root equals the true pose to 1e-9 (max abs over R and t);
//                       no root is NaN.  Prints "p3p cases <n> misses <m> nonfinite <k> worst <e>".
//   degenerate          collinear, coincident and non-finite points, coincident bearings: 0 roots.  Prints "degenerate bad <m>".
//   refine <n> <seed>   n random poses, 200 noise-free points, Gauss-Newton from a start perturbed by ~0.05 rad / 0.1 in at most 10
//                       steps: the true pose to 1e-9.  Prints "refine cases <n> misses <m> worst <e>".
//   sample <seed> <h> <m> <N>   pnp_sample<N> (N = 3 or 8) of the stream (seed, h): the indices, space separated.
#include "../../visual-slam_amd/csrc/pnp.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

static const double KM[9] = {500.0, 0.0, 320.0, 0.0, 480.0, 240.0, 0.0, 0.0, 1.0};

static void rand_rot(std::mt19937_64& g, double ang_max, double* R) {
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    double w[3];
    do { w[0] = u(g); w[1] = u(g); w[2] = u(g); } while (w[0] * w[0] + w[1] * w[1] + w[2] * w[2] > 1.0);
    const double n = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) + 1e-300;
    const double a = ang_max * std::fabs(u(g));
    for (double& x : w) x *= a / n;
    pnp_exp_so3(w, R);
}

// a camera-frame point inside the image at depth 2 - 10, and its world point
static void rand_point(std::mt19937_64& g, const double* R, const double* t, double* Xw, double* px) {
    std::uniform_real_distribution<double> ux(20.0, 620.0), uy(20.0, 460.0), uz(2.0, 10.0);
    const double x = ux(g), y = uy(g), z = uz(g);
    const double c[3] = {(x - KM[2]) / KM[0] * z, (y - KM[5]) / KM[4] * z, z};
    double d[3] = {c[0] - t[0], c[1] - t[1], c[2] - t[2]};
    for (int i = 0; i < 3; i++) Xw[i] = R[i] * d[0] + R[3 + i] * d[1] + R[6 + i] * d[2];  // R^T (c - t)
    px[0] = x; px[1] = y;
}

static double pose_err(const double* R, const double* t, const double* R0, const double* t0) {
    double e = 0.0;
    for (int i = 0; i < 9; i++) e = std::fmax(e, std::fabs(R[i] - R0[i]));
    for (int i = 0; i < 3; i++) e = std::fmax(e, std::fabs(t[i] - t0[i]));
    return e;
}

static void bearing(const double* px, double* b) {
    b[1] = (px[1] - KM[5]) / KM[4];
    b[0] = (px[0] - KM[2] - KM[1] * b[1]) / KM[0];
    b[2] = 1.0;
}

static int run_p3p(long n, uint64_t seed) {
    std::mt19937_64 g(seed);
    std::uniform_real_distribution<double> ut(-2.0, 2.0);
    long miss = 0, nonfinite = 0, done = 0;
    double worst = 0.0;
    while (done < n) {
        double R0[9], t0[3] = {ut(g), ut(g), ut(g)};
        rand_rot(g, 3.14159, R0);
        double X[3][3], b[3][3], px[3][2];
        for (int i = 0; i < 3; i++) { rand_point(g, R0, t0, X[i], px[i]); bearing(px[i], b[i]); }
        // well-conditioned: image triangle angles >= 10 degrees, sides >= 40 px
        bool ok = true;
        for (int i = 0; i < 3 && ok; i++) {
            const double* a = px[i]; const double* p = px[(i + 1) % 3]; const double* q = px[(i + 2) % 3];
            const double u0 = p[0] - a[0], u1 = p[1] - a[1], v0 = q[0] - a[0], v1 = q[1] - a[1];
            const double lu = std::hypot(u0, u1), lv = std::hypot(v0, v1);
            if (lu < 40.0 || lv < 40.0) ok = false;
            else if (std::fabs(u0 * v1 - u1 * v0) / (lu * lv) < std::sin(10.0 * M_PI / 180.0)) ok = false;
        }
        if (!ok) continue;
        // and away from the danger cylinder: the law-of-cosines system at the true distances s_i is not near singular
        // (|det J| / (s1 s2 s3) >= 1e-3 with J the Jacobian of the three equations over 2; ~ 0.3 % of the triangles are excluded)
        double y[3][3], sd[3];
        for (int i = 0; i < 3; i++) {
            double c[3];
            for (int k = 0; k < 3; k++) c[k] = R0[k * 3] * X[i][0] + R0[k * 3 + 1] * X[i][1] + R0[k * 3 + 2] * X[i][2] + t0[k];
            sd[i] = std::sqrt(pnp_dot(c, c));
            for (int k = 0; k < 3; k++) y[i][k] = c[k] / sd[i];
        }
        const double c12 = pnp_dot(y[0], y[1]), c13 = pnp_dot(y[0], y[2]), c23 = pnp_dot(y[1], y[2]);
        const double J[9] = {sd[0] - sd[1] * c12, sd[1] - sd[0] * c12, 0.0, sd[0] - sd[2] * c13, 0.0, sd[2] - sd[0] * c13,
                             0.0, sd[1] - sd[2] * c23, sd[2] - sd[1] * c23};
        const double det = J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6]);
        if (std::fabs(det) / (sd[0] * sd[1] * sd[2]) < 1e-3) continue;
        done++;
        double R[4][9], t[4][3];
        const int nr = pnp_p3p(X, b, R, t);
        double best = 1e300;
        for (int r = 0; r < nr; r++) {
            for (int i = 0; i < 9; i++) if (!std::isfinite(R[r][i])) nonfinite++;
            for (int i = 0; i < 3; i++) if (!std::isfinite(t[r][i])) nonfinite++;
            best = std::fmin(best, pose_err(R[r], t[r], R0, t0));
        }
        if (!(best <= 1e-9)) {
            if (miss++ < 5) std::printf("miss: roots %d best %.3g\n", nr, best);
        } else {
            worst = std::fmax(worst, best);
        }
    }
    std::printf("p3p cases %ld misses %ld nonfinite %ld worst %.3g\n", n, miss, nonfinite, worst);
    return miss || nonfinite;
}

static int run_degenerate() {
    std::mt19937_64 g(5);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    long bad = 0, cases = 0;
    for (int it = 0; it < 2000; it++) {
        double X[3][3], b[3][3];
        for (int i = 0; i < 3; i++) { for (int k = 0; k < 3; k++) X[i][k] = u(g) * 3.0; X[i][2] += 6.0; for (int k = 0; k < 3; k++) b[i][k] = X[i][k]; }
        double R[4][9], t[4][3];
        const int kind = it % 5;
        double Xd[3][3], bd[3][3];
        std::memcpy(Xd, X, sizeof(X)); std::memcpy(bd, b, sizeof(b));
        if (kind == 0) { const double l = u(g) * 2.0; for (int k = 0; k < 3; k++) Xd[2][k] = X[0][k] + l * (X[1][k] - X[0][k]); }  // collinear
        if (kind == 1) { for (int k = 0; k < 3; k++) Xd[1][k] = X[0][k]; }                                                          // coincident points
        if (kind == 2) { const double s = 1.0 + std::fabs(u(g)); for (int k = 0; k < 3; k++) bd[2][k] = b[0][k] * s; }             // coincident bearings
        if (kind == 3) { Xd[it % 3][it % 2] = NAN; }                                                                                 // non-finite point
        if (kind == 4) { bd[it % 3][0] = 0.0; bd[it % 3][1] = 0.0; bd[it % 3][2] = 0.0; }                                         // zero bearing
        const int nr = pnp_p3p(Xd, bd, R, t);
        cases++;
        if (nr != 0) { if (bad++ < 5) std::printf("degenerate kind %d gave %d roots\n", kind, nr); }
    }
    std::printf("degenerate cases %ld bad %ld\n", cases, bad);
    return bad != 0;
}

static int run_refine(long n, uint64_t seed) {
    std::mt19937_64 g(seed);
    std::uniform_real_distribution<double> ut(-2.0, 2.0), up(-1.0, 1.0);
    long miss = 0;
    double worst = 0.0;
    const int np = 200;
    static double Xw[200][3], px[200][2];
    for (long c = 0; c < n; c++) {
        double R0[9], t0[3] = {ut(g), ut(g), ut(g)};
        rand_rot(g, 3.14159, R0);
        for (int i = 0; i < np; i++) rand_point(g, R0, t0, Xw[i], px[i]);
        double dR[9], R[9], t[3];
        rand_rot(g, 0.05, dR);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i * 3 + j] = dR[i * 3] * R0[j] + dR[i * 3 + 1] * R0[3 + j] + dR[i * 3 + 2] * R0[6 + j];
        for (int i = 0; i < 3; i++) t[i] = t0[i] + 0.1 * up(g);
        for (int it = 0; it < 10; it++) {
            double H[21] = {0}, gr[6] = {0}, step = 0.0;
            for (int i = 0; i < np; i++) pnp_gn_accumulate(KM, R, t, Xw[i][0], Xw[i][1], Xw[i][2], px[i][0], px[i][1], H, gr);
            if (!pnp_gn_update(H, gr, R, t, &step) || step < 1e-13) break;
        }
        const double e = pose_err(R, t, R0, t0);
        if (!(e <= 1e-9)) { if (miss++ < 5) std::printf("refine miss %.3g\n", e); }
        else worst = std::fmax(worst, e);
        // the inlier test at the true pose: every point projects onto its pixel
        double P[12], e2;
        pnp_projection(KM, R0, t0, P);
        for (int i = 0; i < np; i++)
            if (!pnp_reproj2(P, Xw[i][0], Xw[i][1], Xw[i][2], px[i][0], px[i][1], &e2) || !(e2 < 1e-12)) { miss++; break; }
    }
    std::printf("refine cases %ld misses %ld worst %.3g\n", n, miss, worst);
    return miss != 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "p3p")) return run_p3p(argc > 2 ? std::atol(argv[2]) : 100000, argc > 3 ? std::strtoull(argv[3], 0, 10) : 1);
    if (argc >= 2 && !std::strcmp(argv[1], "degenerate")) return run_degenerate();
    if (argc >= 2 && !std::strcmp(argv[1], "refine")) return run_refine(argc > 2 ? std::atol(argv[2]) : 1000, argc > 3 ? std::strtoull(argv[3], 0, 10) : 1);
    if (argc >= 6 && !std::strcmp(argv[1], "sample")) {
        const uint64_t seed = std::strtoull(argv[2], 0, 10);
        const int h = std::atoi(argv[3]), m = std::atoi(argv[4]), N = std::atoi(argv[5]);
        if (N == 3) { int idx[3]; pnp_sample<3>(seed, h, m, idx); std::printf("%d %d %d\n", idx[0], idx[1], idx[2]); }
        else { int idx[8]; pnp_sample<8>(seed, h, m, idx); for (int k = 0; k < 8; k++) std::printf("%d%c", idx[k], k == 7 ? '\n' : ' '); }
        return 0;
    }
    std::fprintf(stderr, "usage: pnp_check p3p|degenerate|refine|sample ...\n");
    return 2;
}
