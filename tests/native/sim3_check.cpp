// Host check of the loop-alignment solver (visual-slam_amd/csrc/sim3.h), built with g++ -ffp-contract=off.
//   horn3 <n> <seed>    n random similarities (scale 0.2 .. 5, any rotation) and 3 exact pairs of a well-shaped triangle: the closed
//                       form against the truth, max abs over s, R and t.  Prints "horn3 cases <n> misses <m> worst <e>" (a miss: no
//                       model).
//   horn50 <n> <seed>   the same over 50 exact pairs.  Prints "horn50 cases <n> misses <m> worst <e>".
//   degenerate          collinear points (in both frames, in one of them), coincident points, a non-finite coordinate, a mirrored
//                       set whose best scale is negative or zero: no model.  Prints "degenerate bad <m>".
//   refine <n> <seed>   n random similarities, 100 noise-free pairs with both keypoints, Gauss-Newton from a start perturbed by ~0.05
//                       rad / 0.1 / 5 % in at most 10 steps: the truth again.  Prints "refine cases <n> misses <m> worst <e>".
//   inverse <n> <seed>  S21 (S12 X) == X.  Prints "inverse cases <n> worst <e>".
#include "../../visual-slam_amd/csrc/sim3.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

static Sim3 rand_sim(std::mt19937_64& g, double ang_max, double s_lo, double s_hi, double t_max) {
    std::uniform_real_distribution<double> u(0.0, 1.0), ut(-t_max, t_max);
    Sim3 S;
    S.s = s_lo * std::pow(s_hi / s_lo, u(g));
    rand_rot(g, ang_max, S.R);
    for (double& v : S.t) v = ut(g);
    return S;
}

static double sim_err(const Sim3& A, const Sim3& B) {
    double e = std::fabs(A.s - B.s);
    for (int i = 0; i < 9; i++) e = std::fmax(e, std::fabs(A.R[i] - B.R[i]));
    for (int i = 0; i < 3; i++) e = std::fmax(e, std::fabs(A.t[i] - B.t[i]));
    return e;
}

template <int N> static int run_horn(const char* name, long n, uint64_t seed) {
    std::mt19937_64 g(seed);
    std::uniform_real_distribution<double> ux(-3.0, 3.0), uz(3.0, 12.0);
    long miss = 0, done = 0;
    double worst = 0.0;
    while (done < n) {
        const Sim3 T = rand_sim(g, 3.14159, 0.2, 5.0, 2.0);
        double P1[N][3], P2[N][3];
        for (int i = 0; i < N; i++) {
            P2[i][0] = ux(g); P2[i][1] = ux(g); P2[i][2] = uz(g);
            sim3_apply(T, P2[i], P1[i]);
        }
        if (N == 3) {   // a well-shaped triangle: the sine of the angle at the first point above 0.3
            double a[3], b[3], cr[3];
            for (int k = 0; k < 3; k++) { a[k] = P2[1][k] - P2[0][k]; b[k] = P2[2][k] - P2[0][k]; }
            pnp_cross(a, b, cr);
            if (!(pnp_dot(cr, cr) > 0.09 * pnp_dot(a, a) * pnp_dot(b, b)) || !(pnp_dot(a, a) > 0.25) || !(pnp_dot(b, b) > 0.25)) continue;
        }
        done++;
        Sim3 S;
        if (!sim3_horn<N>(P1, P2, S)) { miss++; continue; }
        worst = std::fmax(worst, sim_err(S, T));
    }
    std::printf("%s cases %ld misses %ld worst %.3e\n", name, n, miss, worst);
    return 0;
}

static int run_degenerate() {
    int bad = 0;
    Sim3 S;
    const Sim3 T = {1.3, {0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0}, {0.5, -0.25, 1.0}};
    // collinear in both frames (coordinates exact in binary)
    {
        double P1[3][3], P2[3][3] = {{0.0, 1.0, 5.0}, {0.25, 1.0, 5.5}, {0.75, 1.0, 6.5}};
        for (int i = 0; i < 3; i++) sim3_apply(T, P2[i], P1[i]);
        bad += sim3_horn<3>(P1, P2, S);
    }
    // collinear in frame 2 only, and in frame 1 only
    {
        const double L[3][3] = {{0.0, 1.0, 5.0}, {0.25, 1.0, 5.5}, {0.75, 1.0, 6.5}}, G[3][3] = {{1.0, 0.0, 4.0}, {-1.0, 2.0, 6.0}, {0.5, -1.5, 7.0}};
        bad += sim3_horn<3>(G, L, S);
        bad += sim3_horn<3>(L, G, S);
    }
    // five collinear pairs
    {
        double P1[5][3], P2[5][3];
        for (int i = 0; i < 5; i++) { P2[i][0] = 0.5 * i; P2[i][1] = -1.0; P2[i][2] = 4.0 + 0.25 * i; sim3_apply(T, P2[i], P1[i]); }
        bad += sim3_horn<5>(P1, P2, S);
    }
    // coincident points: all three, and two of three
    {
        const double C[3][3] = {{1.0, 2.0, 3.0}, {1.0, 2.0, 3.0}, {1.0, 2.0, 3.0}}, G[3][3] = {{1.0, 0.0, 4.0}, {-1.0, 2.0, 6.0}, {0.5, -1.5, 7.0}};
        bad += sim3_horn<3>(C, C, S);
        bad += sim3_horn<3>(G, C, S);
        const double D2[3][3] = {{1.0, 2.0, 3.0}, {1.0, 2.0, 3.0}, {2.0, 2.5, 4.0}};
        double D1[3][3];
        for (int i = 0; i < 3; i++) sim3_apply(T, D2[i], D1[i]);
        bad += sim3_horn<3>(D1, D2, S);
    }
    // a coordinate that is not finite
    {
        double P1[3][3] = {{1.0, 0.0, 4.0}, {-1.0, 2.0, 6.0}, {0.5, -1.5, 7.0}}, P2[3][3] = {{1.0, 0.0, 4.0}, {-1.0, 2.0, 6.0}, {0.5, -1.5, 7.0}};
        P2[1][2] = std::numeric_limits<double>::quiet_NaN();
        bad += sim3_horn<3>(P1, P2, S);
        P2[1][2] = std::numeric_limits<double>::infinity();
        bad += sim3_horn<3>(P1, P2, S);
        P2[1][2] = 6.0; P1[2][0] = std::numeric_limits<double>::quiet_NaN();
        bad += sim3_horn<3>(P1, P2, S);
    }
    // Gauss-Newton: a normal matrix that is not positive definite is refused and leaves the model alone
    {
        double H[28], g[7] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0}, step = -1.0;
        for (double& v : H) v = 0.0;
        Sim3 U = T;
        bad += sim3_gn_update(H, g, U, &step);
        bad += std::memcmp(&U, &T, sizeof(T)) != 0;
    }
    std::printf("degenerate bad %d\n", bad);
    return 0;
}

static void project(const double* Y, double* px) {
    const double p0 = KM[0] * Y[0] + KM[1] * Y[1] + KM[2] * Y[2], p1 = KM[3] * Y[0] + KM[4] * Y[1] + KM[5] * Y[2], p2 = KM[6] * Y[0] + KM[7] * Y[1] + KM[8] * Y[2];
    px[0] = p0 / p2; px[1] = p1 / p2;
}

static int run_refine(long n, uint64_t seed) {
    std::mt19937_64 g(seed);
    std::uniform_real_distribution<double> ux(-2.0, 2.0), uz(4.0, 10.0), up(-1.0, 1.0);
    long miss = 0, done = 0;
    double worst = 0.0;
    while (done < n) {
        const Sim3 T = rand_sim(g, 0.5, 0.5, 2.0, 0.5);
        const int M = 100;
        Sim3Pair c[M];
        bool front = true;
        for (int i = 0; i < M; i++) {
            c[i].X2[0] = ux(g); c[i].X2[1] = ux(g); c[i].X2[2] = uz(g);
            sim3_apply(T, c[i].X2, c[i].X1);
            front &= c[i].X1[2] > 0.5;
            double px[2];
            project(c[i].X1, px); c[i].x1 = px[0]; c[i].y1 = px[1]; c[i].i1 = ba_info(1.2, i % 4);
            project(c[i].X2, px); c[i].x2 = px[0]; c[i].y2 = px[1]; c[i].i2 = ba_info(1.2, (i / 4) % 4);
        }
        if (!front) continue;
        done++;
        // the start: exp(delta) T for a small delta, through the update itself (H = I, g = -delta)
        Sim3 S = T;
        {
            double H[28], gr[7], step;
            int o = 0;
            for (int i = 0; i < 7; i++) for (int j = i; j < 7; j++) H[o++] = i == j ? 1.0 : 0.0;
            for (int i = 0; i < 3; i++) { gr[i] = -0.1 * up(g); gr[3 + i] = -0.05 * up(g); }
            gr[6] = -0.05 * up(g);
            if (!sim3_gn_update(H, gr, S, &step)) { miss++; continue; }
        }
        bool okk = true;
        for (int it = 0; it < 10; it++) {
            Sim3 I;
            sim3_inverse(S, I);
            double H[28], gr[7], step;
            for (double& v : H) v = 0.0;
            for (double& v : gr) v = 0.0;
            for (int i = 0; i < M; i++) sim3_gn_accumulate(KM, S, I, c[i], 9.21, H, gr);
            if (!sim3_gn_update(H, gr, S, &step)) { okk = false; break; }
            if (step < 1e-12) break;
        }
        const double e = sim_err(S, T);
        if (!okk || !(e < 1e-8)) miss++;
        worst = std::fmax(worst, e);
    }
    std::printf("refine cases %ld misses %ld worst %.3e\n", n, miss, worst);
    return 0;
}

static int run_inverse(long n, uint64_t seed) {
    std::mt19937_64 g(seed);
    std::uniform_real_distribution<double> ux(-3.0, 3.0);
    double worst = 0.0;
    for (long k = 0; k < n; k++) {
        const Sim3 T = rand_sim(g, 3.14159, 0.2, 5.0, 2.0);
        Sim3 I;
        sim3_inverse(T, I);
        const double X[3] = {ux(g), ux(g), ux(g)};
        double Y[3], Z[3];
        sim3_apply(T, X, Y);
        sim3_apply(I, Y, Z);
        for (int i = 0; i < 3; i++) worst = std::fmax(worst, std::fabs(Z[i] - X[i]));
    }
    std::printf("inverse cases %ld worst %.3e\n", n, worst);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "horn3")) return run_horn<3>("horn3", std::atol(argv[2]), std::strtoull(argv[3], 0, 10));
    if (argc == 4 && !std::strcmp(argv[1], "horn50")) return run_horn<50>("horn50", std::atol(argv[2]), std::strtoull(argv[3], 0, 10));
    if (argc == 2 && !std::strcmp(argv[1], "degenerate")) return run_degenerate();
    if (argc == 4 && !std::strcmp(argv[1], "refine")) return run_refine(std::atol(argv[2]), std::strtoull(argv[3], 0, 10));
    if (argc == 4 && !std::strcmp(argv[1], "inverse")) return run_inverse(std::atol(argv[2]), std::strtoull(argv[3], 0, 10));
    std::fprintf(stderr, "usage: sim3_check horn3|horn50|refine|inverse <n> <seed> | degenerate\n");
    return 2;
}
