// The refit of mo_map_loop_confirm restated sequentially on the host (built with g++ -O2 -std=c++17 -ffp-contract=off): what k_cf_refit
// of visual-slam_amd/csrc/map_confirm.hip computes from the packed pairs and the given model, through the same sim3.h.  The sums of a
// Gauss-Newton step are taken in the device's order (lane l adds j = l, l + 64, ..., then the tree v[l] += v[l + d], d = 32 .. 1, of
// wave_sum in map_store.h), so libm's exp / sin / cos are the only difference to the device build.
//
//   confirm_replay <in> <out>
//     <in>  (little endian): f64 K[9], f64 chi2, i32 n_cand, i32 0; per candidate i32 takes_part, i32 m, f64 model[13] (s, R, t), then
//           m x Sim3Pair (12 f64: X1, X2, x1, y1, info1, x2, y2, info2) in row order.
//     <out>: i32 n_cand, i32 0, f64 margin of the selections (the smallest |e - chi2| / chi2 over both weighted errors of every pair
//           scored; +inf when chi2 = 0 or nothing was scored); per candidate i32 ninl, i32 rounds_run, f64 model[13], u8 flag[m].
//           A candidate that takes no part: 0, 0, NaN; one of fewer than 3 pairs: 0, 0, the model as given.
#include "../../visual-slam_amd/csrc/sim3.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

struct Cand { int32_t part, m; double model[13]; std::vector<Sim3Pair> c; };

static double g_margin = std::numeric_limits<double>::infinity();

static void note(double e, double chi2) {
    if (chi2 > 0.0) {
        const double d = std::fabs(e - chi2) / chi2;
        if (d < g_margin) g_margin = d;   // (a NaN error is on neither side of any threshold)
    }
}

static int select(const double* K, const Sim3& S, const Cand& c, double chi2, std::vector<uint8_t>& fl) {
    Sim3 I;
    sim3_inverse(S, I);
    int n = 0;
    for (int j = 0; j < c.m; j++) {
        double e1, e2;
        fl[j] = sim3_inlier(K, S, I, c.c[j], chi2, &e1, &e2);
        note(e1, chi2); note(e2, chi2);
        n += fl[j];
    }
    return n;
}

static double wave_sum(double (&v)[64]) {
    for (int d = 32; d; d >>= 1)
        for (int l = 0; l < d; l++) v[l] += v[l + d];
    return v[0];
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: confirm_replay <in> <out>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    double K[9], chi2;
    int32_t n_cand, pad;
    bool ok = std::fread(K, 8, 9, f) == 9 && std::fread(&chi2, 8, 1, f) == 1 && std::fread(&n_cand, 4, 1, f) == 1 && std::fread(&pad, 4, 1, f) == 1 &&
              n_cand >= 0 && n_cand <= 16;
    std::vector<Cand> cs(ok ? n_cand : 0);
    for (Cand& c : cs) {
        ok = ok && std::fread(&c.part, 4, 1, f) == 1 && std::fread(&c.m, 4, 1, f) == 1 && c.m >= 0 && std::fread(c.model, 8, 13, f) == 13;
        if (!ok) break;
        c.c.resize(c.m);
        ok = c.m == 0 || std::fread(c.c.data(), sizeof(Sim3Pair), c.m, f) == (size_t)c.m;
    }
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "malformed input %s\n", argv[1]); return 2; }
    struct Res { int32_t ninl = 0, rounds = 0; double model[13]; std::vector<uint8_t> fl; };
    std::vector<Res> res(n_cand);
    for (int ci = 0; ci < n_cand; ci++) {
        const Cand& c = cs[ci];
        Res& r = res[ci];
        r.fl.assign(c.m, 0);
        for (double& p : r.model) p = std::numeric_limits<double>::quiet_NaN();
        if (!c.part) continue;
        Sim3 S;
        S.s = c.model[0];
        for (int i = 0; i < 9; i++) S.R[i] = c.model[1 + i];
        for (int i = 0; i < 3; i++) S.t[i] = c.model[10 + i];
        int n = 0;
        if (c.m >= 3) {
            n = select(K, S, c, chi2, r.fl);
            for (int round = 0; round < 2 && n >= 3; round++) {
                for (int it = 0; it < 10; it++) {
                    Sim3 I;
                    sim3_inverse(S, I);
                    static double lane[35][64];
                    for (int l = 0; l < 64; l++) {
                        double H[28], g[7];
                        for (double& v : H) v = 0.0;
                        for (double& v : g) v = 0.0;
                        for (int j = l; j < c.m; j += 64) {
                            if (!r.fl[j]) continue;
                            sim3_gn_accumulate(K, S, I, c.c[j], chi2, H, g);
                        }
                        for (int i = 0; i < 28; i++) lane[i][l] = H[i];
                        for (int i = 0; i < 7; i++) lane[28 + i][l] = g[i];
                    }
                    double H[28], g[7], step;
                    for (int i = 0; i < 28; i++) H[i] = wave_sum(lane[i]);
                    for (int i = 0; i < 7; i++) g[i] = wave_sum(lane[28 + i]);
                    if (!sim3_gn_update(H, g, S, &step) || step < 1e-12) break;
                }
                n = select(K, S, c, chi2, r.fl);
                r.rounds++;
            }
        }
        r.ninl = n;
        r.model[0] = S.s;
        for (int i = 0; i < 9; i++) r.model[1 + i] = S.R[i];
        for (int i = 0; i < 3; i++) r.model[10 + i] = S.t[i];
    }
    const int32_t zero = 0;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::fwrite(&n_cand, 4, 1, o); std::fwrite(&zero, 4, 1, o); std::fwrite(&g_margin, 8, 1, o);
    for (int ci = 0; ci < n_cand; ci++) {
        const Res& r = res[ci];
        std::fwrite(&r.ninl, 4, 1, o); std::fwrite(&r.rounds, 4, 1, o);
        std::fwrite(r.model, 8, 13, o);
        if (!r.fl.empty()) std::fwrite(r.fl.data(), 1, r.fl.size(), o);
    }
    return std::fclose(o) ? 2 : 0;
}
