// Host check of the FAST arc network of k_fast (visual-slam_amd/csrc/fast_score.h, instantiated with std::min / std::max) against
// the oracle's corner test and cornerScore (oracle/orb_oracle.cpp).  Prints "circles <n> mismatches <m>" and, for the first
// mismatches, the circle.  Usage: fast_network_check <n random circles> <seed>
#include "../../oracle/orb_oracle.cpp"
#include "../../visual-slam_amd/csrc/fast_score.h"

#include <cstdio>
#include <random>

static long g_checked = 0, g_bad = 0;

static void check(int v, const int p[16], int t) {
    int d[25];
    for (int k = 0; k < 16; k++) d[k] = v - p[k];
    for (int k = 16; k < 25; k++) d[k] = d[k - 16];
    const bool corner = fast_is_corner(d, t);
    const int score = corner ? fast_corner_score(d, t) : -1;
    auto mn = [](int a, int b) { return std::min(a, b); };
    auto mx = [](int a, int b) { return std::max(a, b); };
    const int ld = v - fast_arc_extreme(p, mx, mn);  // darker arc
    const int lb = fast_arc_extreme(p, mn, mx) - v;  // brighter arc
    const int l = std::max(ld, lb);
    const bool c2 = l > t;
    const int s2 = c2 ? l - 1 : -1;
    g_checked++;
    if (c2 != corner || s2 != score) {
        if (g_bad++ < 5) {
            std::printf("mismatch t=%d v=%d p=", t, v);
            for (int k = 0; k < 16; k++) std::printf("%d ", p[k]);
            std::printf("oracle %d/%d network %d/%d\n", (int)corner, score, (int)c2, s2);
        }
    }
}

int main(int argc, char** argv) {
    const long n = argc > 1 ? std::atol(argv[1]) : 1000000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    const int ts[] = {0, 1, 7, 20, 254};
    int p[16];
    // random circles: uniform pixels, and centre-relative contrasts around the threshold (the cases that decide corner / score)
    for (long i = 0; i < n; i++) {
        const int t = ts[i % 5];
        const int v = (int)(rng() % 256);
        if (i & 1) {
            for (int k = 0; k < 16; k++) p[k] = (int)(rng() % 256);
        } else {
            for (int k = 0; k < 16; k++) {
                const int sgn = (int)(rng() % 3) - 1, dt = (int)(rng() % 5) - 2;
                p[k] = std::min(255, std::max(0, v + sgn * (t + dt)));
            }
        }
        check(v, p, t);
    }
    // edge cases at every threshold: all equal, every bright / dark circle mask at contrast t - 1, t, t + 1, 0 / 255 extremes
    for (int t : ts) {
        for (int v : {0, 1, 127, 128, 254, 255}) {
            for (int k = 0; k < 16; k++) p[k] = v;
            check(v, p, t);
        }
        for (int m = 0; m < 65536; m++) {
            for (int dt = -1; dt <= 1; dt++) {
                for (int v : {0, 128, 255}) {
                    for (int k = 0; k < 16; k++) p[k] = std::min(255, std::max(0, (m >> k) & 1 ? v + t + dt : v - t - dt));
                    check(v, p, t);
                }
                for (int k = 0; k < 16; k++) p[k] = (m >> k) & 1 ? 255 : 0;
                check(0, p, t);
                check(255, p, t);
            }
        }
    }
    std::printf("circles %ld mismatches %ld\n", g_checked, g_bad);
    return g_bad != 0;
}
