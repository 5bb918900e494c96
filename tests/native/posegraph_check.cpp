// Host build over visual-slam_amd/csrc/posegraph.h (what map_posegraph.hip compiles for the device): the logarithm against the
// exponential, the residual of an exact measurement, the two analytic Jacobians against central differences of the retraction, and the
// 7x7 block operations.  The residual rotation of the Jacobian cases has the angles 0, 1e-9, 1e-3, 1, 3 and pi - 1e-6.
// Prints every figure; exit status 1 when one is over its bound.
//
// Bounds.  log(exp(w)) - w: both maps are a handful of operations on numbers of magnitude <= pi, the near-pi branch takes a square root
// of a difference of magnitude 1: 1e-9 leaves seven digits over the 1e-16 of the arithmetic.  Exact measurement: E is the identity up to
// products of numbers of magnitude <= 20 (t up to 5, s up to 2): 1e-12.  Central differences with h = 1e-7 (a step that keeps pi - 1e-6
// below pi): truncation h^2 |r'''| / 6 ~ 1e-14 |J|, rounding eps |r| / h ~ 1e-16 * 20 / 1e-7 = 2e-8; the bound is 1e-6 (1 + max |J|).
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../visual-slam_amd/csrc/posegraph.h"

static uint64_t rng_state = 0x1234567ull;
static double uni(double lo, double hi) { return lo + (hi - lo) * (double)(pnp_splitmix64(rng_state) >> 11) / 9007199254740992.0; }

static void rand_axis(double* a) {
    double n;
    do { for (int i = 0; i < 3; i++) a[i] = uni(-1, 1); n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); } while (n < 0.1 || n > 1.0);
    for (int i = 0; i < 3; i++) a[i] /= n;
}
static Sim3 rand_sim(double angle, double smin = 0.5, double smax = 2.0, double tmax = 5.0) {
    Sim3 S;
    double a[3];
    rand_axis(a);
    for (int i = 0; i < 3; i++) a[i] *= angle;
    pg_exp_so3(a, S.R);
    S.s = uni(smin, smax);
    for (int i = 0; i < 3; i++) S.t[i] = uni(-tmax, tmax);
    return S;
}

static int fails = 0;
static void report(const char* what, double got, double bound) {
    std::printf("%-58s %.3g (bound %.3g)%s\n", what, got, bound, got <= bound ? "" : "  FAIL");
    if (!(got <= bound)) fails++;
}

int main() {
    const double PI = 3.14159265358979323846;
    const double angles[6] = {0.0, 1e-9, 1e-3, 1.0, 3.0, PI - 1e-6};
    // log(exp(w)) = w
    double worst = 0.0;
    for (int a = 0; a < 6; a++)
        for (int rep = 0; rep < 200; rep++) {
            double w[3], R[9], v[3];
            rand_axis(w);
            for (int i = 0; i < 3; i++) w[i] *= angles[a];
            pg_exp_so3(w, R);
            pg_log_so3(R, v);
            for (int i = 0; i < 3; i++) worst = std::fmax(worst, std::fabs(v[i] - w[i]));
        }
    report("log_so3(exp_so3(w)) - w, six angles", worst, 1e-9);
    // the rotation by exactly pi about an axis: |log| = pi
    {
        const double R[9] = {-1, 0, 0, 0, 1, 0, 0, 0, -1};
        double v[3];
        pg_log_so3(R, v);
        report("log_so3 of the half turn about y", std::fabs(v[0]) + std::fabs(std::fabs(v[1]) - PI) + std::fabs(v[2]), 1e-15);
    }
    // compose / inverse / exact measurement
    worst = 0.0;
    for (int rep = 0; rep < 500; rep++) {
        const Sim3 Sa = rand_sim(uni(0, 3)), Sb = rand_sim(uni(0, 3));
        Sim3 M;
        pg_measure(Sa, Sb, M);
        double r[7];
        pg_residual(M, Sa, Sb, r);
        for (int k = 0; k < 7; k++) worst = std::fmax(worst, std::fabs(r[k]));
    }
    report("residual of an exact measurement", worst, 1e-12);
    // Jacobians against central differences, the residual rotation at each angle
    const double h = 1e-7;
    for (int a = 0; a < 6; a++) {
        double wr = 0.0, wj = 0.0;
        for (int rep = 0; rep < 100; rep++) {
            const Sim3 Sa = rand_sim(uni(0, 3)), Sb = rand_sim(uni(0, 3));
            const Sim3 Et = rand_sim(angles[a], 0.7, 1.4, 1.0);
            Sim3 Mx, M;   // M = E_target o S_b o S_a^-1, so that E = E_target
            pg_measure(Sa, Sb, Mx);
            pg_compose(Et, Mx, M);
            double r[7], Ja[49], Jb[49], r2[7];
            pg_linearize(M, Sa, Sb, r, Ja, Jb);
            pg_residual(M, Sa, Sb, r2);
            double jm = 0.0;
            for (int k = 0; k < 7; k++) wr = std::fmax(wr, std::fabs(r[k] - r2[k]));
            for (int k = 0; k < 49; k++) jm = std::fmax(jm, std::fmax(std::fabs(Ja[k]), std::fabs(Jb[k])));
            const double ang = std::sqrt(r[3] * r[3] + r[4] * r[4] + r[5] * r[5]);
            wr = std::fmax(wr, std::fabs(ang - angles[a]) > 1e-9 ? 1.0 : 0.0);   // (the case has the angle it was built for)
            for (int side = 0; side < 2; side++)
                for (int c = 0; c < 7; c++) {
                    double d[7] = {0, 0, 0, 0, 0, 0, 0}, rp[7], rm[7];
                    Sim3 P, Q;
                    d[c] = h; pg_retract(d, side ? Sb : Sa, P);
                    d[c] = -h; pg_retract(d, side ? Sb : Sa, Q);
                    if (side) { pg_residual(M, Sa, P, rp); pg_residual(M, Sa, Q, rm); }
                    else { pg_residual(M, P, Sb, rp); pg_residual(M, Q, Sb, rm); }
                    for (int k = 0; k < 7; k++) {
                        const double fd = (rp[k] - rm[k]) / (2.0 * h), an = (side ? Jb : Ja)[k * 7 + c];
                        wj = std::fmax(wj, std::fabs(fd - an) / (1.0 + jm));
                    }
                }
        }
        char name[96];
        std::snprintf(name, sizeof name, "residual rotation %.9g: linearize's residual - residual", angles[a]);
        report(name, wr, 0.0);
        std::snprintf(name, sizeof name, "residual rotation %.9g: |J - central difference| / (1 + max |J|)", angles[a]);
        report(name, wj, 1e-6);
    }
    // the 7x7 blocks: a Cholesky solve reproduces its right side; a block that is not positive definite is refused
    worst = 0.0;
    for (int rep = 0; rep < 200; rep++) {
        double A[49], H[49], L[49], b[7], x[7];
        for (int k = 0; k < 49; k++) A[k] = uni(-1, 1);
        for (int i = 0; i < 7; i++) {
            for (int j = 0; j < 7; j++) H[i * 7 + j] = pg_atb_entry(A, A, i, j) + (i == j ? 0.5 : 0.0);
            b[i] = uni(-1, 1);
        }
        if (!pg_chol7(H, 1.0, L)) { fails++; continue; }
        pg_chol7_solve(L, b, x);
        for (int i = 0; i < 7; i++) worst = std::fmax(worst, std::fabs(pg_mulv_entry(H, x, i, false) - b[i]));
    }
    report("H (chol7_solve b) - b", worst, 1e-11);
    {
        double H[49], L[49];
        for (int k = 0; k < 49; k++) H[k] = k % 8 == 0 ? 1.0 : 0.0;
        H[24] = -1.0;
        report("chol7 of an indefinite block is refused", pg_chol7(H, 1.0, L) ? 1.0 : 0.0, 0.0);
    }
    // the host order of a workgroup's sum equals the plain sum on integers
    report("tree sum of 0 .. 4999", std::fabs(pg_tree_sum(5000, [](int i) { return (double)i; }) - 12497500.0), 0.0);
    std::printf(fails ? "FAILED %d\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
