// Host build of visual-slam_amd/csrc/ba.h (the arithmetic of the bundle-adjustment kernels): analytic Jacobians against central
// differences, the 3x3 inverse and the Cholesky solve against known systems, one Schur step against the dense solve of the same damped
// system.  Prints "ok <name> <largest error>" per check; exit status 1 on a failure.  Driven by tests/test_ba_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../visual-slam_amd/csrc/ba.h"

static uint64_t rs = 12345;
static double rnd() { return (double)(pnp_splitmix64(rs) >> 11) / 9007199254740992.0; }
static double rndu(double a, double b) { return a + (b - a) * rnd(); }
static int fails = 0;
static void report(const char* name, double err, double bound) {
    printf("%s %s %.3e (bound %.1e)\n", err <= bound ? "ok" : "FAIL", name, err, bound);
    if (!(err <= bound)) fails++;
}

static const double K[9] = {500, 0, 320, 0, 480, 240, 0, 0, 1};

static void random_pose(double* T) {
    double w[3] = {rndu(-0.2, 0.2), rndu(-0.2, 0.2), rndu(-0.2, 0.2)}, E[9];
    pnp_exp_so3(w, E);
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T[i * 4 + j] = E[i * 3 + j]; T[i * 4 + 3] = rndu(-0.5, 0.5); }
}

static void project(const double* T, const double* X, double* uv) {
    double e[2], z;
    ba_residual(K, T, X, 0.0, 0.0, e, &z);
    uv[0] = -e[0]; uv[1] = -e[1];
}

static void check_jacobians() {
    double worst = 0.0;
    for (int it = 0; it < 200; it++) {
        double T[12], X[3] = {rndu(-2, 2), rndu(-2, 2), rndu(4, 10)}, Jc[12], Jp[6];
        random_pose(T);
        ba_jacobians(K, T, X, Jc, Jp);
        const double h = 1e-6;
        for (int k = 0; k < 6; k++) {
            double d[6] = {0, 0, 0, 0, 0, 0}, Ta[12], Tb[12], a[2], b[2];
            d[k] = h; ba_pose_update(d, T, Ta);
            d[k] = -h; ba_pose_update(d, T, Tb);
            project(Ta, X, a); project(Tb, X, b);
            for (int r = 0; r < 2; r++) worst = fmax(worst, fabs((a[r] - b[r]) / (2 * h) - Jc[r * 6 + k]) / (1.0 + fabs(Jc[r * 6 + k])));
        }
        for (int k = 0; k < 3; k++) {
            double Xa[3] = {X[0], X[1], X[2]}, Xb[3] = {X[0], X[1], X[2]}, a[2], b[2];
            Xa[k] += h; Xb[k] -= h;
            project(T, Xa, a); project(T, Xb, b);
            for (int r = 0; r < 2; r++) worst = fmax(worst, fabs((a[r] - b[r]) / (2 * h) - Jp[r * 3 + k]) / (1.0 + fabs(Jp[r * 3 + k])));
        }
    }
    report("jacobians_central_differences", worst, 1e-6);
}

static void check_inv3() {
    double worst = 0.0;
    for (int it = 0; it < 200; it++) {
        double B[9], V[6], Vi[6];
        for (double& v : B) v = rndu(-1, 1);
        int o = 0;
        for (int i = 0; i < 3; i++)
            for (int j = i; j < 3; j++) { V[o] = (i == j ? 0.1 : 0.0); for (int k = 0; k < 3; k++) V[o] += B[k * 3 + i] * B[k * 3 + j]; o++; }
        if (!ba_inv3(V, Vi)) { fails++; continue; }
        const double F[9] = {V[0], V[1], V[2], V[1], V[3], V[4], V[2], V[4], V[5]}, G[9] = {Vi[0], Vi[1], Vi[2], Vi[1], Vi[3], Vi[4], Vi[2], Vi[4], Vi[5]};
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                double s = 0.0;
                for (int k = 0; k < 3; k++) s += F[i * 3 + k] * G[k * 3 + j];
                worst = fmax(worst, fabs(s - (i == j)));
            }
    }
    report("inv3_times_matrix", worst, 1e-9);
    const double bad[6] = {1, 2, 0, 1, 0, 1}, nanv[6] = {NAN, 0, 0, 1, 0, 1};
    double Vi[6];
    report("inv3_refuses_indefinite", (ba_inv3(bad, Vi) ? 1.0 : 0.0) + (ba_inv3(nanv, Vi) ? 1.0 : 0.0), 0.0);
}

static void check_cholesky() {
    double worst = 0.0;
    for (int n : {1, 6, 42, 96}) {
        std::vector<double> B((size_t)n * n), A((size_t)n * (n + 1) / 2), x0(n), b(n), x(n);
        for (double& v : B) v = rndu(-1, 1);
        for (double& v : x0) v = rndu(-1, 1);
        for (int i = 0; i < n; i++)
            for (int j = 0; j <= i; j++) {
                double s = i == j ? 1.0 : 0.0;
                for (int k = 0; k < n; k++) s += B[(size_t)k * n + i] * B[(size_t)k * n + j];
                A[BA_TRI(i, j)] = s;
            }
        for (int i = 0; i < n; i++) {
            double s = 0.0;
            for (int j = 0; j < n; j++) s += A[i >= j ? BA_TRI(i, j) : BA_TRI(j, i)] * x0[j];
            b[i] = s;
        }
        if (!ba_chol_solve(n, A.data(), b.data(), x.data())) { fails++; continue; }
        for (int i = 0; i < n; i++) worst = fmax(worst, fabs(x[i] - x0[i]));
    }
    report("cholesky_known_solution", worst, 1e-9);
    double A2[3] = {1, 2, 1}, b2[2] = {1, 1}, x2[2];
    report("cholesky_refuses_indefinite", ba_chol_solve(2, A2, b2, x2) ? 1.0 : 0.0, 0.0);
}

// 3 free cameras + 1 fixed, 40 points seen by 2 - 4 of them; Schur step from ba.h's pieces against the dense damped system
static void check_schur() {
    const int NC = 4, NF = 3, NP = 40, D = 6 * NF + 3 * NP;
    const double lambda = 1e-3, huber2 = 5.991;
    double T[NC][12], X[NP][3];
    for (int c = 0; c < NC; c++) { random_pose(T[c]); T[c][3] += 0.4 * c; }
    struct Edge { int p, c; double x, y, info; };
    std::vector<Edge> edges;
    for (int p = 0; p < NP; p++) {
        X[p][0] = rndu(-2, 2); X[p][1] = rndu(-2, 2); X[p][2] = rndu(5, 10);
        const int first = (int)(rnd() * 3), cnt = 2 + (int)(rnd() * 3);
        for (int c = first; c < NC && c < first + cnt; c++) {
            double uv[2];
            project(T[c], X[p], uv);
            edges.push_back({p, c, uv[0] + rndu(-4, 4), uv[1] + rndu(-4, 4), ba_info(1.2, (int)(rnd() * 4))});
        }
    }
    auto fidx = [](int c) { return c - 1; };   // camera 0 fixed
    // dense
    std::vector<double> H((size_t)D * D, 0.0), g(D, 0.0);
    for (const Edge& e : edges) {
        double er[2], z, Jc[12], Jp[6];
        ba_residual(K, T[e.c], X[e.p], e.x, e.y, er, &z);
        ba_jacobians(K, T[e.c], X[e.p], Jc, Jp);
        const double e2 = e.info * (er[0] * er[0] + er[1] * er[1]), w = e.info * ba_weight(e2, huber2);
        int idx[9], n = 0;
        double J[2][9];
        if (fidx(e.c) >= 0) for (int k = 0; k < 6; k++) { idx[n] = 6 * fidx(e.c) + k; J[0][n] = Jc[k]; J[1][n] = Jc[6 + k]; n++; }
        for (int k = 0; k < 3; k++) { idx[n] = 6 * NF + 3 * e.p + k; J[0][n] = Jp[k]; J[1][n] = Jp[3 + k]; n++; }
        for (int a = 0; a < n; a++) {
            for (int b = 0; b < n; b++) H[(size_t)idx[a] * D + idx[b]] += w * (J[0][a] * J[0][b] + J[1][a] * J[1][b]);
            g[idx[a]] += w * (J[0][a] * er[0] + J[1][a] * er[1]);
        }
    }
    std::vector<double> A((size_t)D * (D + 1) / 2), xd(D);
    for (int i = 0; i < D; i++)
        for (int j = 0; j <= i; j++) A[BA_TRI(i, j)] = H[(size_t)i * D + j] * (i == j ? 1.0 + lambda : 1.0);
    if (!ba_chol_solve(D, A.data(), g.data(), xd.data())) { fails++; printf("FAIL dense system not positive definite\n"); return; }
    // Schur, the way the kernels compose it
    double Vi[NP][6], gp[NP][3];
    for (int p = 0; p < NP; p++) {
        double V[6] = {0, 0, 0, 0, 0, 0};
        gp[p][0] = gp[p][1] = gp[p][2] = 0.0;
        for (const Edge& e : edges) {
            if (e.p != p) continue;
            double er[2], z, Jc[12], Jp[6];
            ba_residual(K, T[e.c], X[p], e.x, e.y, er, &z);
            ba_jacobians(K, T[e.c], X[p], Jc, Jp);
            ba_point_terms(Jp, e.info * ba_weight(e.info * (er[0] * er[0] + er[1] * er[1]), huber2), er, V, gp[p]);
        }
        V[0] *= 1.0 + lambda; V[3] *= 1.0 + lambda; V[5] *= 1.0 + lambda;
        if (!ba_inv3(V, Vi[p])) { fails++; return; }
    }
    const int n = 6 * NF;
    std::vector<double> S((size_t)n * (n + 1) / 2, 0.0), b(n, 0.0), dc(n);
    for (int i = 0; i < NF; i++)
        for (int j = i; j < NF; j++) {
            double blk[36], bi[6] = {0, 0, 0, 0, 0, 0}, dA[6] = {0, 0, 0, 0, 0, 0};
            for (double& v : blk) v = 0.0;
            for (const Edge& a : edges) {
                if (fidx(a.c) != i) continue;
                double era[2], z, Jca[12], Jpa[6];
                ba_residual(K, T[a.c], X[a.p], a.x, a.y, era, &z);
                ba_jacobians(K, T[a.c], X[a.p], Jca, Jpa);
                const double wa = a.info * ba_weight(a.info * (era[0] * era[0] + era[1] * era[1]), huber2);
                if (i == j) {
                    ba_camera_terms(Jca, wa, era, blk, bi);
                    for (int k = 0; k < 6; k++) dA[k] += wa * (Jca[k] * Jca[k] + Jca[6 + k] * Jca[6 + k]);
                    ba_schur_rhs(Jca, Jpa, wa, Vi[a.p], gp[a.p], bi);
                }
                for (const Edge& e : edges) {
                    if (e.p != a.p || fidx(e.c) != j) continue;
                    double erb[2], Jcb[12], Jpb[6];
                    ba_residual(K, T[e.c], X[e.p], e.x, e.y, erb, &z);
                    ba_jacobians(K, T[e.c], X[e.p], Jcb, Jpb);
                    ba_schur_pair(Jca, Jpa, wa, Jcb, Jpb, e.info * ba_weight(e.info * (erb[0] * erb[0] + erb[1] * erb[1]), huber2), Vi[a.p], blk);
                }
            }
            for (int r = 0; r < 6; r++)
                for (int c = 0; c < 6; c++)
                    if (6 * j + c <= 6 * i + r || i != j) {
                        const int R = 6 * j + c, C = 6 * i + r;   // lower triangle: row of the later keyframe
                        if (i == j) { if (c <= r) S[BA_TRI(6 * i + r, 6 * i + c)] = blk[r * 6 + c] + (r == c ? lambda * dA[r] : 0.0); }
                        else S[BA_TRI(R, C)] = blk[r * 6 + c];
                    }
            if (i == j) for (int k = 0; k < 6; k++) b[6 * i + k] = bi[k];
        }
    if (!ba_chol_solve(n, S.data(), b.data(), dc.data())) { fails++; printf("FAIL reduced system not positive definite\n"); return; }
    double worst = 0.0;
    for (int k = 0; k < n; k++) worst = fmax(worst, fabs(dc[k] - xd[k]));
    for (int p = 0; p < NP; p++) {
        double gg[3] = {gp[p][0], gp[p][1], gp[p][2]}, dp[3];
        for (const Edge& e : edges) {
            if (e.p != p || fidx(e.c) < 0) continue;
            double er[2], z, Jc[12], Jp[6];
            ba_residual(K, T[e.c], X[p], e.x, e.y, er, &z);
            ba_jacobians(K, T[e.c], X[p], Jc, Jp);
            ba_back_edge(Jc, Jp, e.info * ba_weight(e.info * (er[0] * er[0] + er[1] * er[1]), huber2), dc.data() + 6 * fidx(e.c), gg);
        }
        ba_sym3_mul(Vi[p], gg, dp);
        for (int k = 0; k < 3; k++) worst = fmax(worst, fabs(dp[k] - xd[6 * NF + 3 * p + k]));
    }
    report("schur_step_equals_dense_solve", worst, 1e-9);
}

int main() {
    check_jacobians();
    check_inv3();
    check_cholesky();
    check_schur();
    return fails ? 1 : 0;
}
