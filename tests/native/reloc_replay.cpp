// The geometry of mo_map_relocalize restated sequentially on the host (built with g++ -O2 -std=c++17 -ffp-contract=off): what
// k_reloc_hyp, k_reloc_refine and k_reloc_finish of visual-slam_amd/csrc/map_reloc.hip compute from the correspondence sets C_k,
// through the same pnp.h.  The sums of a Gauss-Newton step are taken in the device's order (lane l adds j = l, l + 64, ..., then the
// tree v[l] += v[l + d], d = 32 .. 1, of wave_sum in map_store.h), so libm's sin / cos are the only difference to the device build.
//
//   reloc_replay run <in> <out> [--variant NAME]
//     <in>  (little endian): f64 K[9], f64 thr_px, u64 seed, i32 n_hyp, i32 n_cand; per candidate i32 k (keyframe position), i32 m,
//           then m x (f32 X, Y, Z of the map point, f32 x, y of the query keypoint) in C_k order.  Candidates in rank order.
//     <out>: i32 n_cand, i32 winner (candidate index, -1: none), f64 margin of the hypothesis scoring, f64 margin of the selections
//           behind the two refinement rounds (the smallest |e2 - thr2| / thr2; +inf when thr2 = 0 or nothing was scored); per candidate
//           u64 best, i32 ninl, i32 m, i32 rounds_run, f64 pose[12], u8 flag[m]; then per candidate and hypothesis h < n_hyp:
//           i32 idx[3], i32 roots, i32 count[4], f64 R[4][9], f64 t[4][3] (entries past `roots` are 0).
//     --variant: one deliberately wrong reading of the header's rules (tests/test_reloc_replay_cpu.py lists what each must move):
//           ties_high, drop_last_block, drop_tail_lanes, no_depth_test, one_round, winner_by_score, root0.
//   reloc_replay seedsearch <m> <k> <n_hyp> <start> <tries> <i0> <i1> ...
//     the first seed >= start whose stream (seed, k) draws three of the given indices in exactly one hypothesis, the last one.
#include "../../visual-slam_amd/csrc/pnp.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

struct Corr { float X, Y, Z, x, y; };
struct Cand { int32_t k, m; std::vector<Corr> c; };
struct Variant { bool ties_high = false, drop_last_block = false, drop_tail_lanes = false, no_depth_test = false, one_round = false,
                      winner_by_score = false, root0 = false; };

static double g_margin_hyp = std::numeric_limits<double>::infinity(), g_margin_sel = std::numeric_limits<double>::infinity();

static bool inlier(const Variant& v, const double* P, const Corr& c, double thr2, double* margin) {
    double e2;
    const bool front = pnp_reproj2(P, c.X, c.Y, c.Z, c.x, c.y, &e2);
    if (thr2 > 0.0) {
        const double d = std::fabs(e2 - thr2) / thr2;
        if (d < *margin) *margin = d;   // (a NaN e2 is on neither side of any threshold)
    }
    return (front || v.no_depth_test) && e2 < thr2;
}

static int solve(const double* Kinv, const Cand& c, uint64_t seed, int h, int (&idx)[3], double (&R)[4][9], double (&t)[4][3]) {
    pnp_sample<3>(pnp_stream_seed(seed, c.k), h, c.m, idx);
    double X[3][3], b[3][3];
    for (int i = 0; i < 3; i++) {
        const Corr& s = c.c[idx[i]];
        X[i][0] = s.X; X[i][1] = s.Y; X[i][2] = s.Z;
        const double x = s.x, y = s.y;
        for (int r = 0; r < 3; r++) b[i][r] = Kinv[r * 3] * x + Kinv[r * 3 + 1] * y + Kinv[r * 3 + 2];
    }
    return pnp_p3p(X, b, R, t);
}

static int select(const Variant& v, const double* K, const double* R, const double* t, const Cand& c, double thr2, std::vector<uint8_t>& fl) {
    double P[12];
    pnp_projection(K, R, t, P);
    const int scored = v.drop_tail_lanes ? c.m - c.m % 64 : c.m;
    int n = 0;
    for (int j = 0; j < c.m; j++) {
        fl[j] = j < scored && inlier(v, P, c.c[j], thr2, &g_margin_sel);
        n += fl[j];
    }
    return n;
}

static double wave_sum(double (&v)[64]) {
    for (int d = 32; d; d >>= 1)
        for (int l = 0; l < d; l++) v[l] += v[l + d];
    return v[0];
}

int run(const char* in_path, const char* out_path, const Variant& v) {
    FILE* f = std::fopen(in_path, "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", in_path); return 2; }
    double K[9], thr_px;
    uint64_t seed;
    int32_t n_hyp, n_cand;
    bool ok = std::fread(K, 8, 9, f) == 9 && std::fread(&thr_px, 8, 1, f) == 1 && std::fread(&seed, 8, 1, f) == 1 &&
              std::fread(&n_hyp, 4, 1, f) == 1 && std::fread(&n_cand, 4, 1, f) == 1 && n_cand >= 0 && n_cand <= 64 && n_hyp >= 1;
    std::vector<Cand> cs(ok ? n_cand : 0);
    for (Cand& c : cs) {
        ok = ok && std::fread(&c.k, 4, 1, f) == 1 && std::fread(&c.m, 4, 1, f) == 1 && c.m >= 3;
        if (!ok) break;
        c.c.resize(c.m);
        ok = std::fread(c.c.data(), sizeof(Corr), c.m, f) == (size_t)c.m;
    }
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "malformed input %s\n", in_path); return 2; }
    // Kinv by the adjugate formula of reloc_run
    double Kinv[9];
    {
        const double* A = K;
        const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
        const double det = A[0] * c0 + A[1] * c1 + A[2] * c2;
        const double inv[9] = {c0, A[2] * A[7] - A[1] * A[8], A[1] * A[5] - A[2] * A[4],
                               c1, A[0] * A[8] - A[2] * A[6], A[2] * A[3] - A[0] * A[5],
                               c2, A[1] * A[6] - A[0] * A[7], A[0] * A[4] - A[1] * A[3]};
        for (int i = 0; i < 9; i++) Kinv[i] = inv[i] / det;
    }
    const double thr2 = thr_px * thr_px;
    const int hyp_run = v.drop_last_block ? n_hyp - n_hyp % 4 : n_hyp;
    FILE* o = std::fopen(out_path, "wb");
    if (!o) { std::fprintf(stderr, "cannot write %s\n", out_path); return 2; }
    struct Res { uint64_t best = 0; int32_t ninl = 0, rounds = 0; double pose[12]; std::vector<uint8_t> fl; };
    struct Hyp { int32_t idx[3], roots, count[4]; double R[4][9], t[4][3]; };
    std::vector<Res> res(n_cand);
    std::vector<std::vector<Hyp>> dump(n_cand);
    for (int ci = 0; ci < n_cand; ci++) {
        const Cand& c = cs[ci];
        Res& r = res[ci];
        r.fl.assign(c.m, 0);
        for (double& p : r.pose) p = std::numeric_limits<double>::quiet_NaN();
        dump[ci].resize(n_hyp);
        const int scored = v.drop_tail_lanes ? c.m - c.m % 64 : c.m;
        for (int h = 0; h < n_hyp; h++) {
            Hyp& d = dump[ci][h];
            std::memset(&d, 0, sizeof(d));
            int idx[3];
            double R[4][9], t[4][3];
            const int nr = solve(Kinv, c, seed, h, idx, R, t);
            for (int i = 0; i < 3; i++) d.idx[i] = idx[i];
            d.roots = nr;
            for (int root = 0; root < nr; root++) {
                double P[12];
                pnp_projection(K, R[root], t[root], P);
                int n = 0;
                for (int j = 0; j < scored; j++) n += inlier(v, P, c.c[j], thr2, &g_margin_hyp);
                d.count[root] = n;
                std::memcpy(d.R[root], R[root], sizeof(R[root]));
                std::memcpy(d.t[root], t[root], sizeof(t[root]));
                const uint32_t hr = (uint32_t)(h * 4 + root);
                const uint64_t key = ((uint64_t)(uint32_t)n << 32) | (v.ties_high ? hr : 0xffffffffu - hr);
                if (h < hyp_run && n > 0 && key > r.best) r.best = key;
            }
        }
        if (!r.best) continue;   // no pose with an inlier: 0 inliers, NaN pose
        const uint32_t low = (uint32_t)(r.best & 0xffffffffu), hr = v.ties_high ? low : 0xffffffffu - low;
        r.best = (r.best & 0xffffffff00000000ull) | (0xffffffffu - hr);   // (ties_high compared plain low words: reported in the key's form)
        int idx[3];
        double Rs[4][9], ts[4][3];
        solve(Kinv, c, seed, (int)(hr >> 2), idx, Rs, ts);
        const int root = v.root0 ? 0 : (int)(hr & 3);
        double R[9], t[3];
        for (int i = 0; i < 9; i++) R[i] = Rs[root][i];
        for (int i = 0; i < 3; i++) t[i] = ts[root][i];
        int n = select(v, K, R, t, c, thr2, r.fl);
        for (int round = 0; round < (v.one_round ? 1 : 2); round++) {
            for (int it = 0; it < 10; it++) {
                static double lane[27][64];
                for (int l = 0; l < 64; l++) {
                    double H[21], gr[6];
                    for (int i = 0; i < 21; i++) H[i] = 0.0;
                    for (int i = 0; i < 6; i++) gr[i] = 0.0;
                    for (int j = l; j < c.m; j += 64) {
                        if (!r.fl[j]) continue;
                        const Corr& s = c.c[j];
                        pnp_gn_accumulate(K, R, t, s.X, s.Y, s.Z, s.x, s.y, H, gr);
                    }
                    for (int i = 0; i < 21; i++) lane[i][l] = H[i];
                    for (int i = 0; i < 6; i++) lane[21 + i][l] = gr[i];
                }
                double H[21], gr[6], step;
                for (int i = 0; i < 21; i++) H[i] = wave_sum(lane[i]);
                for (int i = 0; i < 6; i++) gr[i] = wave_sum(lane[21 + i]);
                if (!pnp_gn_update(H, gr, R, t, &step) || step < 1e-12) break;
            }
            n = select(v, K, R, t, c, thr2, r.fl);
            r.rounds++;
        }
        r.ninl = n;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) r.pose[i * 4 + j] = R[i * 3 + j];
            r.pose[i * 4 + 3] = t[i];
        }
    }
    // the winner: most final inliers, ties to the lower position (k_reloc_finish)
    int32_t win = -1;
    for (int ci = 0; ci < n_cand; ci++) {
        if (v.winner_by_score) { if (win < 0) win = ci; continue; }   // rank order: the first candidate has the highest score
        if (win < 0 || res[ci].ninl > res[win].ninl || (res[ci].ninl == res[win].ninl && cs[ci].k < cs[win].k)) win = ci;
    }
    std::fwrite(&n_cand, 4, 1, o); std::fwrite(&win, 4, 1, o);
    std::fwrite(&g_margin_hyp, 8, 1, o); std::fwrite(&g_margin_sel, 8, 1, o);
    for (int ci = 0; ci < n_cand; ci++) {
        const Res& r = res[ci];
        std::fwrite(&r.best, 8, 1, o); std::fwrite(&r.ninl, 4, 1, o); std::fwrite(&cs[ci].m, 4, 1, o); std::fwrite(&r.rounds, 4, 1, o);
        std::fwrite(r.pose, 8, 12, o);
        std::fwrite(r.fl.data(), 1, r.fl.size(), o);
    }
    for (int ci = 0; ci < n_cand; ci++)
        for (const Hyp& d : dump[ci]) {
            std::fwrite(d.idx, 4, 3, o); std::fwrite(&d.roots, 4, 1, o); std::fwrite(d.count, 4, 4, o);
            std::fwrite(d.R, 8, 36, o); std::fwrite(d.t, 8, 12, o);
        }
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
    if (argc >= 4 && !std::strcmp(argv[1], "run")) {
        Variant v;
        if (argc >= 6 && !std::strcmp(argv[4], "--variant")) {
            const std::string n = argv[5];
            if (n == "ties_high") v.ties_high = true;
            else if (n == "drop_last_block") v.drop_last_block = true;
            else if (n == "drop_tail_lanes") v.drop_tail_lanes = true;
            else if (n == "no_depth_test") v.no_depth_test = true;
            else if (n == "one_round") v.one_round = true;
            else if (n == "winner_by_score") v.winner_by_score = true;
            else if (n == "root0") v.root0 = true;
            else { std::fprintf(stderr, "unknown variant %s\n", argv[5]); return 2; }
        } else if (argc != 4) {
            std::fprintf(stderr, "usage: reloc_replay run <in> <out> [--variant NAME]\n");
            return 2;
        }
        return run(argv[2], argv[3], v);
    }
    if (argc >= 8 && !std::strcmp(argv[1], "seedsearch")) return seedsearch(argc, argv);
    std::fprintf(stderr, "usage: reloc_replay run <in> <out> [--variant NAME] | seedsearch <m> <k> <n_hyp> <start> <tries> <indices...>\n");
    return 2;
}
