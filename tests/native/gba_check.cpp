// Host build of visual-slam_amd/csrc/gba.h (the arithmetic of the global bundle adjustment's solve) on a 6-keyframe problem built here:
// the matrix-free operator S p against the dense S assembled from ba.h's Schur terms, the preconditioner blocks against the diagonal
// blocks of that S, the preconditioned conjugate gradient run to cg_tol 1e-14 against ba.h's dense Cholesky solve, and the scalar
// decisions.  Prints "ok <name> <largest error>" per check; exit status 1 on a failure.  Driven by tests/test_gba_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../visual-slam_amd/csrc/gba.h"

// the measured host differences (g++ -O2 -ffp-contract=off, x86-64) times 10
static const double SP_MEASURED = 2.26e-15, SP_BOUND = 10 * SP_MEASURED;     // |S p (matrix-free) - S p (dense)| / |S p|, largest of 20 random p
static const double PRECOND_MEASURED = 0.0, PRECOND_BOUND = 10 * PRECOND_MEASURED;   // |M_k - S_kk| / max |S_kk|: the same function in the same order, equal
static const double PCG_MEASURED = 5.67e-13, PCG_BOUND = 10 * PCG_MEASURED;   // |x (PCG, 27 iterations to cg_tol 1e-14) - x (Cholesky)| / |x|

static uint64_t rs = 777;
static double rnd() { return (double)(pnp_splitmix64(rs) >> 11) / 9007199254740992.0; }
static double rndu(double a, double b) { return a + (b - a) * rnd(); }
static int fails = 0;
static void report(const char* name, double err, double bound) {
    printf("%s %s %.3e (bound %.1e)\n", err <= bound ? "ok" : "FAIL", name, err, bound);
    if (!(err <= bound)) fails++;
}

static const double K[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1};
static const int N_KF = 6, N_FIX = 2, N_FREE = N_KF - N_FIX, N_PT = 150, DIM = 6 * N_FREE;
static const double CHI2 = 5.991, LAMBDA = 1e-4;

struct Edge { int kf, pt; double Jc[12], Jp[6], w, e[2]; };

struct Problem {
    std::vector<Edge> edges;                 // point by point
    std::vector<int> eoff;                   // [N_PT + 1]
    std::vector<double> Vi, gp;              // [N_PT][6], [N_PT][3]
    std::vector<std::vector<int>> klist;     // per free keyframe: its edges, ascending
    double Hd[N_FREE][36], b[DIM];
};

static int fidx(int kf) { return kf < N_FIX ? -1 : kf - N_FIX; }

static void build(Problem& P) {
    double T[N_KF][12];
    for (int k = 0; k < N_KF; k++) {
        double w[3] = {rndu(-0.02, 0.02), rndu(-0.03, 0.03), rndu(-0.02, 0.02)}, E[9];
        pnp_exp_so3(w, E);
        const double c[3] = {0.35 * k, 0.05 * sin((double)k), 0.0};
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) T[k][i * 4 + j] = E[i * 3 + j];
            T[k][i * 4 + 3] = -(E[i * 3] * c[0] + E[i * 3 + 1] * c[1] + E[i * 3 + 2] * c[2]);
        }
    }
    P.eoff.assign(1, 0);
    P.klist.assign(N_FREE, {});
    for (int p = 0; p < N_PT; p++) {
        const double X[3] = {rndu(-2.0, 4.0), rndu(-2.0, 2.0), rndu(3.0, 12.0)};
        const int first = (int)(rnd() * (N_KF - 2)), span = 3 + (int)(rnd() * 2);
        double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
        for (int k = first; k < N_KF && k < first + span; k++) {
            Edge e;
            e.kf = k; e.pt = p;
            double r0[2], z;
            ba_residual(K, T[k], X, 0.0, 0.0, r0, &z);
            // the keypoint: the projection with noise of a few pixels (some edges beyond the Huber width)
            const double x = -r0[0] + rndu(-3.0, 3.0), y = -r0[1] + rndu(-3.0, 3.0);
            ba_residual(K, T[k], X, x, y, e.e, &z);
            const double info = ba_info(1.2, (int)(rnd() * 4)), e2 = info * (e.e[0] * e.e[0] + e.e[1] * e.e[1]);
            e.w = info * ba_weight(e2, CHI2);
            ba_jacobians(K, T[k], X, e.Jc, e.Jp);
            ba_point_terms(e.Jp, e.w, e.e, V, g);
            if (fidx(k) >= 0) P.klist[fidx(k)].push_back((int)P.edges.size());
            P.edges.push_back(e);
        }
        P.eoff.push_back((int)P.edges.size());
        V[0] *= 1.0 + LAMBDA; V[3] *= 1.0 + LAMBDA; V[5] *= 1.0 + LAMBDA;
        double inv[6];
        if (!ba_inv3(V, inv)) { printf("FAIL a point block is not positive definite\n"); exit(1); }
        for (double v : inv) P.Vi.push_back(v);
        for (double v : g) P.gp.push_back(v);
    }
    for (int f = 0; f < N_FREE; f++) {
        double H[36] = {0}, g[6] = {0};
        for (int e : P.klist[f]) {
            const Edge& E = P.edges[e];
            ba_camera_terms(E.Jc, E.w, E.e, H, g);
            ba_schur_rhs(E.Jc, E.Jp, E.w, &P.Vi[E.pt * 6], &P.gp[E.pt * 3], g);
        }
        gba_damp6(H, LAMBDA, P.Hd[f]);
        for (int k = 0; k < 6; k++) P.b[6 * f + k] = g[k];
    }
}

// the dense S from ba.h: the damped diagonal blocks, less ba_schur_pair over every pair of free edges of every point
static void dense_S(const Problem& P, std::vector<double>& S) {
    S.assign(DIM * DIM, 0.0);
    for (int f = 0; f < N_FREE; f++)
        for (int r = 0; r < 6; r++)
            for (int c = 0; c < 6; c++) S[(6 * f + r) * DIM + 6 * f + c] = P.Hd[f][r * 6 + c];
    for (int p = 0; p < N_PT; p++)
        for (int a = P.eoff[p]; a < P.eoff[p + 1]; a++)
            for (int b = P.eoff[p]; b < P.eoff[p + 1]; b++) {
                const Edge &A = P.edges[a], &B = P.edges[b];
                const int fa = fidx(A.kf), fb = fidx(B.kf);
                if (fa < 0 || fb < 0) continue;
                double blk[36] = {0};
                ba_schur_pair(A.Jc, A.Jp, A.w, B.Jc, B.Jp, B.w, &P.Vi[p * 6], blk);
                for (int r = 0; r < 6; r++)
                    for (int c = 0; c < 6; c++) S[(6 * fa + r) * DIM + 6 * fb + c] += blk[r * 6 + c];
            }
}

// y = S p, matrix-free, in the two passes of the kernels
static void apply_S(const Problem& P, const double* p, double* y) {
    std::vector<double> q(N_PT * 3);
    for (int pt = 0; pt < N_PT; pt++) {
        double t[3] = {0, 0, 0};
        for (int e = P.eoff[pt]; e < P.eoff[pt + 1]; e++) {
            const Edge& E = P.edges[e];
            if (fidx(E.kf) >= 0) gba_wt_p(E.Jc, E.Jp, E.w, p + 6 * fidx(E.kf), t);
        }
        ba_sym3_mul(&P.Vi[pt * 6], t, &q[pt * 3]);
    }
    for (int f = 0; f < N_FREE; f++) {
        double a[6] = {0, 0, 0, 0, 0, 0};
        for (int e : P.klist[f]) { const Edge& E = P.edges[e]; gba_w_q(E.Jc, E.Jp, E.w, &q[E.pt * 3], a); }
        gba_block_mul(P.Hd[f], p + 6 * f, y + 6 * f);
        for (int k = 0; k < 6; k++) y[6 * f + k] -= a[k];
    }
}

static double norm(const double* v, int n) { double s = 0; for (int i = 0; i < n; i++) s += v[i] * v[i]; return sqrt(s); }

int main() {
    Problem P;
    build(P);
    std::vector<double> S;
    dense_S(P, S);
    // 1: the operator
    double worst = 0.0;
    for (int it = 0; it < 20; it++) {
        double p[DIM], y[DIM], yd[DIM], d[DIM];
        for (double& v : p) v = rndu(-1, 1);
        apply_S(P, p, y);
        for (int i = 0; i < DIM; i++) { yd[i] = 0; for (int j = 0; j < DIM; j++) yd[i] += S[i * DIM + j] * p[j]; d[i] = y[i] - yd[i]; }
        worst = fmax(worst, norm(d, DIM) / norm(yd, DIM));
    }
    report("matrix_free_Sp_against_dense", worst, SP_BOUND);
    // 2: the preconditioner blocks (no point is seen twice from one keyframe: same-edge terms are the whole diagonal block)
    double L[N_FREE][GBA_TRI_N];
    worst = 0.0;
    int how = 0;
    for (int f = 0; f < N_FREE; f++) {
        double M[36], big = 0.0;
        for (int k = 0; k < 36; k++) M[k] = P.Hd[f][k];
        for (int e : P.klist[f]) { const Edge& E = P.edges[e]; gba_precond_edge(E.Jc, E.Jp, E.w, &P.Vi[E.pt * 6], M); }
        for (int r = 0; r < 6; r++)
            for (int c = 0; c < 6; c++) big = fmax(big, fabs(S[(6 * f + r) * DIM + 6 * f + c]));
        for (int r = 0; r < 6; r++)
            for (int c = 0; c < 6; c++) worst = fmax(worst, fabs(M[r * 6 + c] - S[(6 * f + r) * DIM + 6 * f + c]) / big);
        how += gba_precond_factor(M, P.Hd[f], L[f]);
    }
    report("preconditioner_blocks_against_dense", worst, PRECOND_BOUND);
    report("preconditioner_blocks_factor", (double)how, 0.0);
    // 3: the conjugate gradient against the dense Cholesky solve
    std::vector<double> A(BA_TRI(DIM - 1, DIM - 1) + 1);
    for (int i = 0; i < DIM; i++)
        for (int j = 0; j <= i; j++) A[BA_TRI(i, j)] = S[i * DIM + j];
    double xd[DIM];
    if (!ba_chol_solve(DIM, A.data(), P.b, xd)) { printf("FAIL the dense system is not positive definite\n"); return 1; }
    double x[DIM], r[DIM], z[DIM], p[DIM], Sp[DIM];
    for (int i = 0; i < DIM; i++) { x[i] = 0.0; r[i] = P.b[i]; }
    for (int f = 0; f < N_FREE; f++) gba_solve6(L[f], r + 6 * f, z + 6 * f);
    for (int i = 0; i < DIM; i++) p[i] = z[i];
    double rz = 0.0;
    for (int i = 0; i < DIM; i++) rz += r[i] * z[i];
    const double rz0 = rz, tol2 = 1e-14 * 1e-14;
    int it = 0;
    if (gba_cg_start(rz0) == 1) {
        while (it < 500) {
            apply_S(P, p, Sp);
            double pSp = 0.0, alpha, beta;
            for (int i = 0; i < DIM; i++) pSp += p[i] * Sp[i];
            if (!gba_cg_alpha(rz, pSp, &alpha)) break;
            for (int i = 0; i < DIM; i++) { x[i] += alpha * p[i]; r[i] -= alpha * Sp[i]; }
            for (int f = 0; f < N_FREE; f++) gba_solve6(L[f], r + 6 * f, z + 6 * f);
            double rzn = 0.0;
            for (int i = 0; i < DIM; i++) rzn += r[i] * z[i];
            it++;
            if (!gba_cg_continue(rzn, tol2, rz0, rz, &beta)) break;
            for (int i = 0; i < DIM; i++) p[i] = z[i] + beta * p[i];
            rz = rzn;
        }
    }
    double d[DIM];
    for (int i = 0; i < DIM; i++) d[i] = x[i] - xd[i];
    printf("conjugate gradient: %d iterations on %d unknowns\n", it, DIM);
    report("pcg_against_dense_cholesky", norm(d, DIM) / norm(xd, DIM), PCG_BOUND);
    report("pcg_iterations_at_most_the_dimension_times_two", (double)it, 2.0 * DIM);
    // 4: the decisions
    double al = 0.0, be = 0.0;
    int bad = 0;
    bad += gba_cg_start(1.0) != 1; bad += gba_cg_start(0.0) != 0; bad += gba_cg_start(-1.0) != -1; bad += gba_cg_start(NAN) != -1; bad += gba_cg_start(INFINITY) != -1;
    bad += gba_cg_alpha(1.0, 0.0, &al); bad += gba_cg_alpha(1.0, -1.0, &al); bad += gba_cg_alpha(1.0, NAN, &al); bad += gba_cg_alpha(1.0, INFINITY, &al);
    bad += !gba_cg_alpha(1.0, 2.0, &al) || al != 0.5;
    bad += gba_cg_continue(1e-30, 1e-16, 1.0, 1.0, &be); bad += gba_cg_continue(NAN, 1e-16, 1.0, 1.0, &be);
    bad += !gba_cg_continue(0.25, 1e-16, 1.0, 0.5, &be) || be != 0.5;
    double I6[36] = {0}, N6[36] = {0}, Lf[GBA_TRI_N];
    for (int k = 0; k < 6; k++) { I6[k * 7] = 1.0; N6[k * 7] = k == 3 ? -1.0 : 1.0; }
    bad += gba_precond_factor(I6, I6, Lf) != 0; bad += gba_precond_factor(N6, I6, Lf) != 1; bad += gba_precond_factor(N6, N6, Lf) != 2;
    report("decisions", (double)bad, 0.0);
    return fails ? 1 : 0;
}
