// Host replay of mo_map_pose_graph's optimisation (visual-slam_amd/csrc/map_posegraph.hip) over the same header, posegraph.h, with the
// same orders of summation: the measurements from the given edge list (tests/posegraph_restatement.py builds it), then the
// Levenberg-Marquardt loop kernel by kernel - k_pg_edge, k_pg_vertex, k_pg_solve, k_pg_trial, k_pg_accept - as loops over what the
// device gives a thread.  Built twice by tests/posegraph_cases.py: plain, and with -DPG_LIBM_NUDGE (every libm result moved by two
// units in the last place, alternating): the spread between the two bounds what the device's libm may do to a result.
//
//   posegraph_replay run <in> <out>
// in:  int32 n_kf, n_edges, max_steps, max_cg; f64 cg_tol, step_tol; u8 fixed [n_kf] (padded to 8); f64 poses [n_kf][12], init [n_kf][13];
//      int32 ea [n_edges], eb [n_edges], kind [n_edges]
// out: f64 sim3 [n_kf][13], cost [2], lambda; int32 steps, accepted, cg_iters, 0; per step f64 c0, c1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../visual-slam_amd/csrc/posegraph.h"

struct Graph {
    int n_kf = 0, n_edges = 0, nf = 0;
    std::vector<uint8_t> fixed;
    std::vector<int> fidx, fpos, ea, eb, kind, rbase, cbase, clist;
    std::vector<double> M, r, Ja, Jb, W, ec, et, H, L, g;
    std::vector<uint8_t> pfix;
};

static void precond(const Graph& G, const std::vector<double>& r, std::vector<double>& z) {
    for (int f = 0; f < G.nf; f++) {
        double b[7], x[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 7; k++) b[k] = r[f * 7 + k];
        if (!G.pfix[f]) pg_chol7_solve(&G.L[(size_t)f * 49], b, x);
        for (int k = 0; k < 7; k++) z[f * 7 + k] = x[k];
    }
}

static void matvec(const Graph& G, const std::vector<double>& p, std::vector<double>& q) {
    for (int j = 0; j < 7 * G.nf; j++) {
        const int f = j / 7, k = j - f * 7, pos = G.fpos[f];
        double s = pg_mulv_entry(&G.H[(size_t)f * 49], &p[f * 7], k, false);
        for (int e = G.rbase[pos]; e < G.rbase[pos + 1]; e++) {
            const int fb = G.fidx[G.eb[e]];
            if (fb >= 0) s += pg_mulv_entry(&G.W[(size_t)e * 49], &p[fb * 7], k, false);
        }
        for (int c = G.cbase[pos]; c < G.cbase[pos + 1]; c++) {
            const int e = G.clist[c], fa = G.fidx[G.ea[e]];
            if (fa >= 0) s += pg_mulv_entry(&G.W[(size_t)e * 49], &p[fa * 7], k, true);
        }
        q[j] = s;
    }
}

static double dot(const std::vector<double>& a, const std::vector<double>& b) {
    return pg_tree_sum((int)a.size(), [&](int i) { return a[i] * b[i]; });
}

int main(int argc, char** argv) {
    if (argc != 4 || std::strcmp(argv[1], "run")) { std::fprintf(stderr, "usage: posegraph_replay run <in> <out>\n"); return 2; }
    FILE* fi = std::fopen(argv[2], "rb");
    if (!fi) return 2;
    int32_t hd[4];
    double tol[2];
    if (std::fread(hd, 4, 4, fi) != 4 || std::fread(tol, 8, 2, fi) != 2) return 2;
    Graph G;
    G.n_kf = hd[0]; G.n_edges = hd[1];
    const int max_steps = hd[2], max_cg = hd[3], n = G.n_kf, ne = G.n_edges;
    const double cg_tol2 = tol[0] * tol[0], step_tol = tol[1];
    G.fixed.resize((size_t)(n + 7) / 8 * 8);
    std::vector<double> poses((size_t)n * 12), init((size_t)n * 13);
    std::vector<int32_t> ea(ne), eb(ne), kind(ne);
    bool okr = std::fread(G.fixed.data(), 1, G.fixed.size(), fi) == G.fixed.size() && std::fread(poses.data(), 8, poses.size(), fi) == poses.size() &&
               std::fread(init.data(), 8, init.size(), fi) == init.size();
    if (ne) okr = okr && std::fread(ea.data(), 4, ne, fi) == (size_t)ne && std::fread(eb.data(), 4, ne, fi) == (size_t)ne && std::fread(kind.data(), 4, ne, fi) == (size_t)ne;
    std::fclose(fi);
    if (!okr) return 2;
    G.ea.assign(ea.begin(), ea.end()); G.eb.assign(eb.begin(), eb.end()); G.kind.assign(kind.begin(), kind.end());
    G.fidx.resize(n);
    for (int i = 0; i < n; i++) {
        G.fidx[i] = G.fixed[i] ? -1 : (int)G.fpos.size();
        if (!G.fixed[i]) G.fpos.push_back(i);
    }
    G.nf = (int)G.fpos.size();
    // the vertex CSR: the edges arrive ordered by (a, b); the as-b lists in ascending edge order
    G.rbase.assign(n + 1, 0); G.cbase.assign(n + 1, 0);
    for (int e = 0; e < ne; e++) { G.rbase[G.ea[e] + 1]++; G.cbase[G.eb[e] + 1]++; }
    for (int i = 0; i < n; i++) { G.rbase[i + 1] += G.rbase[i]; G.cbase[i + 1] += G.cbase[i]; }
    G.clist.resize(ne);
    {
        std::vector<int> cur(G.cbase.begin(), G.cbase.end() - 1);
        for (int e = 0; e < ne; e++) G.clist[cur[G.eb[e]]++] = e;
    }
    // k_pg_scatter's measurements
    G.M.resize((size_t)ne * 13);
    for (int e = 0; e < ne; e++) {
        Sim3 Sa, Sb, Me;
        if (G.kind[e] == 0) {
            pg_load(&init[(size_t)G.ea[e] * 13], Sa); pg_load(&init[(size_t)G.eb[e] * 13], Sb);
        } else {
            Sa.s = 1.0; Sb.s = 1.0;
            for (int j = 0; j < 3; j++) {
                for (int l = 0; l < 3; l++) { Sa.R[j * 3 + l] = poses[(size_t)G.ea[e] * 12 + j * 4 + l]; Sb.R[j * 3 + l] = poses[(size_t)G.eb[e] * 12 + j * 4 + l]; }
                Sa.t[j] = poses[(size_t)G.ea[e] * 12 + j * 4 + 3]; Sb.t[j] = poses[(size_t)G.eb[e] * 12 + j * 4 + 3];
            }
        }
        pg_measure(Sa, Sb, Me);
        pg_store(Me, &G.M[(size_t)e * 13]);
    }
    std::vector<double> S(init), St(init);
    G.r.resize((size_t)ne * 7); G.Ja.resize((size_t)ne * 49); G.Jb.resize((size_t)ne * 49); G.W.resize((size_t)ne * 49); G.ec.resize(ne); G.et.resize(ne);
    G.H.resize((size_t)G.nf * 49); G.L.resize((size_t)G.nf * 49); G.g.resize((size_t)G.nf * 7); G.pfix.resize(G.nf);
    double cost[2] = {0.0, 0.0}, lambda = 1e-4;
    int steps = 0, accepted = 0, cg_iters = 0;
    bool done = false;
    const bool run = ne > 0 && G.nf > 0;
    std::vector<double> margins;
    const int nv = 7 * G.nf;
    std::vector<double> x(nv), r(nv), z(nv), p(nv), q(nv);
    for (int s = 0; s < max_steps && run && !done; s++) {
        for (int e = 0; e < ne; e++) {   // k_pg_edge
            Sim3 Me, Sa, Sb;
            pg_load(&G.M[(size_t)e * 13], Me); pg_load(&S[(size_t)G.ea[e] * 13], Sa); pg_load(&S[(size_t)G.eb[e] * 13], Sb);
            double re[7], A[49], B[49];
            pg_linearize(Me, Sa, Sb, re, A, B);
            for (int k = 0; k < 7; k++) G.r[(size_t)e * 7 + k] = re[k];
            for (int k = 0; k < 49; k++) { G.Ja[(size_t)e * 49 + k] = A[k]; G.Jb[(size_t)e * 49 + k] = B[k]; }
            for (int i = 0; i < 7; i++)
                for (int j = 0; j < 7; j++) G.W[(size_t)e * 49 + i * 7 + j] = pg_atb_entry(A, B, i, j);
            G.ec[e] = pg_cost(re);
        }
        const double damp = 1.0 + lambda;
        for (int f = 0; f < G.nf; f++) {   // k_pg_vertex
            const int pos = G.fpos[f];
            double Hs[49];
            for (int k = 0; k < 49; k++) {
                const int i = k / 7, j = k - i * 7;
                double v = 0.0;
                for (int e = G.rbase[pos]; e < G.rbase[pos + 1]; e++) v += pg_atb_entry(&G.Ja[(size_t)e * 49], &G.Ja[(size_t)e * 49], i, j);
                for (int c = G.cbase[pos]; c < G.cbase[pos + 1]; c++) { const size_t e = (size_t)G.clist[c]; v += pg_atb_entry(&G.Jb[e * 49], &G.Jb[e * 49], i, j); }
                Hs[k] = v;
            }
            for (int i = 0; i < 7; i++) {
                double v = 0.0;
                for (int e = G.rbase[pos]; e < G.rbase[pos + 1]; e++) v += pg_atr_entry(&G.Ja[(size_t)e * 49], &G.r[(size_t)e * 7], i);
                for (int c = G.cbase[pos]; c < G.cbase[pos + 1]; c++) { const size_t e = (size_t)G.clist[c]; v += pg_atr_entry(&G.Jb[e * 49], &G.r[e * 7], i); }
                G.g[(size_t)f * 7 + i] = v;
            }
            for (int k = 0; k < 49; k++) G.H[(size_t)f * 49 + k] = (k % 8 == 0) ? Hs[k] * damp : Hs[k];
            G.pfix[f] = !pg_chol7(Hs, damp, &G.L[(size_t)f * 49]);
        }
        // k_pg_solve
        for (int j = 0; j < nv; j++) { x[j] = 0.0; r[j] = -G.g[j]; }
        precond(G, r, z);
        p = z;
        double rz = dot(r, z);
        const double rz0 = rz;
        int it = 0;
        if (rz0 > 0.0 && std::isfinite(rz0)) {
            while (it < max_cg) {
                matvec(G, p, q);
                const double pq = dot(p, q);
                if (!(pq > 0.0) || !std::isfinite(pq)) break;
                const double alpha = rz / pq;
                for (int j = 0; j < nv; j++) { x[j] += alpha * p[j]; r[j] -= alpha * q[j]; }
                precond(G, r, z);
                const double rzn = dot(r, z);
                it++;
                if (!(rzn > cg_tol2 * rz0)) break;
                const double beta = rzn / rz;
                for (int j = 0; j < nv; j++) p[j] = z[j] + beta * p[j];
                rz = rzn;
            }
        }
        double mu = 0.0;
        for (int f = 0; f < G.nf; f++) {
            const int pos = G.fpos[f];
            Sim3 Sc, T;
            pg_load(&S[(size_t)pos * 13], Sc);
            pg_retract(&x[f * 7], Sc, T);
            if (sim3_finite(T) && T.s > 0.0) {
                pg_store(T, &St[(size_t)pos * 13]);
                for (int k = 0; k < 7; k++) mu = std::fmax(mu, std::fabs(x[f * 7 + k]));
            }
        }
        cg_iters += it;
        for (int e = 0; e < ne; e++) {   // k_pg_trial
            Sim3 Me, Sa, Sb;
            pg_load(&G.M[(size_t)e * 13], Me); pg_load(&St[(size_t)G.ea[e] * 13], Sa); pg_load(&St[(size_t)G.eb[e] * 13], Sb);
            double re[7];
            pg_residual(Me, Sa, Sb, re);
            G.et[e] = pg_cost(re);
        }
        // k_pg_accept
        const double c0 = pg_tree_sum(ne, [&](int e) { return G.ec[e]; }), c1 = pg_tree_sum(ne, [&](int e) { return G.et[e]; });
        const bool ok = c1 < c0;
        const double lam = ok ? lambda / 10.0 : lambda * 10.0;
        if (steps == 0) cost[0] = c0;
        cost[1] = ok ? c1 : c0;
        lambda = lam;
        steps++;
        accepted += ok;
        if (mu < step_tol || lam > 1e8) done = true;
        if (ok) S = St; else St = S;
        margins.push_back(c0); margins.push_back(c1);
    }
    FILE* fo = std::fopen(argv[3], "wb");
    if (!fo) return 2;
    std::fwrite(S.data(), 8, S.size(), fo);
    std::fwrite(cost, 8, 2, fo);
    std::fwrite(&lambda, 8, 1, fo);
    const int32_t tail[4] = {steps, accepted, cg_iters, 0};
    std::fwrite(tail, 4, 4, fo);
    std::fwrite(margins.data(), 8, margins.size(), fo);
    std::fclose(fo);
    return 0;
}
