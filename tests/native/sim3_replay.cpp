// The geometry of mo_map_loop_sim3 restated sequentially on the host (built with g++ -O2 -std=c++17 -ffp-contract=off): what
// k_sim3_hyp, k_sim3_refine and k_sim3_finish of visual-slam_amd/csrc/map_sim3.hip compute from the gathered pairs, through the same
// sim3.h.  The sums of a Gauss-Newton step are taken in the device's order (lane l adds j = l, l + 64, ..., then the tree
// v[l] += v[l + d], d = 32 .. 1, of wave_sum in map_store.h), so libm's exp / sin / cos are the only difference to the device build.
//
//   sim3_replay run <in> <out>
//     <in>  (little endian): f64 K[9], f64 chi2, u64 seed, i32 n_hyp, i32 n_cand, i32 min_inliers, i32 0; per candidate i32 k (keyframe
//           position), i32 m, then m x Sim3Pair (12 f64: X1, X2, x1, y1, info1, x2, y2, info2) in row order.
//     <out>: i32 n_cand, i32 winner (candidate index, -1: none), i32 ok, i32 0, f64 margin of the hypothesis scoring, f64 margin of the
//           selections behind a Gauss-Newton round (the smallest |e - chi2| / chi2 over both weighted errors of every pair scored;
//           +inf when chi2 = 0 or nothing was scored); per candidate u64 best, i32 ninl, i32 m, i32 rounds_run, i32 0, f64 model[13]
//           (s, R, t), u8 flag[m]; then per candidate and hypothesis h < n_hyp: i32 idx[3], i32 has_model, i32 count, i32 0,
//           f64 model[13] (0 without a model; a candidate of fewer than 3 pairs has all-zero records).
//   sim3_replay seedsearch <m> <k> <n_hyp> <start> <tries> <i0> <i1> ...
//     the first seed >= start whose stream (seed, k) draws three of the given indices in exactly one hypothesis, the last one.
#include "../../visual-slam_amd/csrc/sim3.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

struct Cand { int32_t k, m; std::vector<Sim3Pair> c; };

static double g_margin_hyp = std::numeric_limits<double>::infinity(), g_margin_sel = std::numeric_limits<double>::infinity();

static void note(double e, double chi2, double* margin) {
    if (chi2 > 0.0) {
        const double d = std::fabs(e - chi2) / chi2;
        if (d < *margin) *margin = d;   // (a NaN error is on neither side of any threshold)
    }
}

static bool inlier(const double* K, const Sim3& S, const Sim3& I, const Sim3Pair& c, double chi2, double* margin) {
    double e1, e2;
    const bool in = sim3_inlier(K, S, I, c, chi2, &e1, &e2);
    note(e1, chi2, margin); note(e2, chi2, margin);
    return in;
}

static bool solve(const Cand& c, uint64_t seed, int h, int (&idx)[3], Sim3& S) {
    pnp_sample<3>(pnp_stream_seed(seed, c.k), h, c.m, idx);
    double P1[3][3], P2[3][3];
    for (int i = 0; i < 3; i++)
        for (int d = 0; d < 3; d++) { P1[i][d] = c.c[idx[i]].X1[d]; P2[i][d] = c.c[idx[i]].X2[d]; }
    return sim3_horn<3>(P1, P2, S);
}

static int select(const double* K, const Sim3& S, const Cand& c, double chi2, std::vector<uint8_t>& fl, double* margin) {
    Sim3 I;
    sim3_inverse(S, I);
    int n = 0;
    for (int j = 0; j < c.m; j++) {
        fl[j] = inlier(K, S, I, c.c[j], chi2, margin);
        n += fl[j];
    }
    return n;
}

static double wave_sum(double (&v)[64]) {
    for (int d = 32; d; d >>= 1)
        for (int l = 0; l < d; l++) v[l] += v[l + d];
    return v[0];
}

static void put_model(double* o, const Sim3& S) {
    o[0] = S.s;
    for (int i = 0; i < 9; i++) o[1 + i] = S.R[i];
    for (int i = 0; i < 3; i++) o[10 + i] = S.t[i];
}

static int run(const char* in_path, const char* out_path) {
    FILE* f = std::fopen(in_path, "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", in_path); return 2; }
    double K[9], chi2;
    uint64_t seed;
    int32_t n_hyp, n_cand, min_inliers, pad;
    bool ok = std::fread(K, 8, 9, f) == 9 && std::fread(&chi2, 8, 1, f) == 1 && std::fread(&seed, 8, 1, f) == 1 && std::fread(&n_hyp, 4, 1, f) == 1 &&
              std::fread(&n_cand, 4, 1, f) == 1 && std::fread(&min_inliers, 4, 1, f) == 1 && std::fread(&pad, 4, 1, f) == 1 && n_cand >= 0 &&
              n_cand <= 16 && n_hyp >= 1;
    std::vector<Cand> cs(ok ? n_cand : 0);
    for (Cand& c : cs) {
        ok = ok && std::fread(&c.k, 4, 1, f) == 1 && std::fread(&c.m, 4, 1, f) == 1 && c.m >= 0;
        if (!ok) break;
        c.c.resize(c.m);
        ok = c.m == 0 || std::fread(c.c.data(), sizeof(Sim3Pair), c.m, f) == (size_t)c.m;
    }
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "malformed input %s\n", in_path); return 2; }
    struct Res { uint64_t best = 0; int32_t ninl = 0, rounds = 0; double model[13]; std::vector<uint8_t> fl; };
    struct Hyp { int32_t idx[3], has, count, pad; double model[13]; };
    std::vector<Res> res(n_cand);
    std::vector<std::vector<Hyp>> dump(n_cand);
    for (int ci = 0; ci < n_cand; ci++) {
        const Cand& c = cs[ci];
        Res& r = res[ci];
        r.fl.assign(c.m, 0);
        for (double& p : r.model) p = std::numeric_limits<double>::quiet_NaN();
        dump[ci].resize(n_hyp);
        for (Hyp& d : dump[ci]) std::memset(&d, 0, sizeof(d));
        if (c.m < 3) continue;
        for (int h = 0; h < n_hyp; h++) {
            Hyp& d = dump[ci][h];
            int idx[3];
            Sim3 S, I;
            const bool has = solve(c, seed, h, idx, S);
            for (int i = 0; i < 3; i++) d.idx[i] = idx[i];
            d.has = has;
            if (!has) continue;
            sim3_inverse(S, I);
            int n = 0;
            for (int j = 0; j < c.m; j++) n += inlier(K, S, I, c.c[j], chi2, &g_margin_hyp);
            d.count = n;
            put_model(d.model, S);
            const uint64_t key = ((uint64_t)(uint32_t)n << 32) | (0xffffffffu - (uint32_t)h);
            if (key > r.best) r.best = key;
        }
        if (!r.best) continue;   // no sample with a model: 0 inliers, NaN model
        const int h = (int)(0xffffffffu - (uint32_t)(r.best & 0xffffffffu));
        int idx[3];
        Sim3 S;
        solve(c, seed, h, idx, S);
        double unused = std::numeric_limits<double>::infinity();
        int n = select(K, S, c, chi2, r.fl, &unused);   // (the hypothesis' own scoring: in margin_hyp already)
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
            n = select(K, S, c, chi2, r.fl, &g_margin_sel);
            r.rounds++;
        }
        r.ninl = n;
        put_model(r.model, S);
    }
    // the winner: a model and the most final inliers, ties to the earlier candidate (k_sim3_finish)
    int32_t win = -1;
    for (int ci = 0; ci < n_cand; ci++)
        if (res[ci].best && (win < 0 || res[ci].ninl > res[win].ninl)) win = ci;
    const int32_t okk = win >= 0 && res[win].ninl >= min_inliers, zero = 0;
    FILE* o = std::fopen(out_path, "wb");
    if (!o) { std::fprintf(stderr, "cannot write %s\n", out_path); return 2; }
    std::fwrite(&n_cand, 4, 1, o); std::fwrite(&win, 4, 1, o); std::fwrite(&okk, 4, 1, o); std::fwrite(&zero, 4, 1, o);
    std::fwrite(&g_margin_hyp, 8, 1, o); std::fwrite(&g_margin_sel, 8, 1, o);
    for (int ci = 0; ci < n_cand; ci++) {
        const Res& r = res[ci];
        std::fwrite(&r.best, 8, 1, o); std::fwrite(&r.ninl, 4, 1, o); std::fwrite(&cs[ci].m, 4, 1, o); std::fwrite(&r.rounds, 4, 1, o);
        std::fwrite(&zero, 4, 1, o);
        std::fwrite(r.model, 8, 13, o);
        if (!r.fl.empty()) std::fwrite(r.fl.data(), 1, r.fl.size(), o);
    }
    for (int ci = 0; ci < n_cand; ci++)
        for (const Hyp& d : dump[ci]) std::fwrite(&d, sizeof(d), 1, o);
    return std::fclose(o) ? 2 : 0;
}

static int seedsearch(int argc, char** argv) {
    const int m = std::atoi(argv[2]), k = std::atoi(argv[3]), n_hyp = std::atoi(argv[4]);
    const uint64_t start = std::strtoull(argv[5], 0, 10), tries = std::strtoull(argv[6], 0, 10);
    std::vector<char> in(m, 0);
    for (int i = 7; i < argc; i++) in[std::atoi(argv[i])] = 1;
    for (uint64_t s = start; s < start + tries; s++) {
        int hits = 0, last = -1;
        for (int h = 0; h < n_hyp; h++) {
            int idx[3];
            pnp_sample<3>(pnp_stream_seed(s, k), h, m, idx);
            if (in[idx[0]] && in[idx[1]] && in[idx[2]]) { hits++; last = h; }
        }
        if (hits == 1 && last == n_hyp - 1) { std::printf("%llu\n", (unsigned long long)s); return 0; }
    }
    std::printf("none\n");
    return 1;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    if (argc >= 10 && !std::strcmp(argv[1], "seedsearch")) return seedsearch(argc, argv);
    std::fprintf(stderr, "usage: sim3_replay run <in> <out> | seedsearch <m> <k> <n_hyp> <start> <tries> <indices...>\n");
    return 2;
}
