// Host check of the plan's table block (visual-slam_amd/csrc/plan_tables.h), built with g++ -fsanitize=address,undefined.
//   plan_check <w> <h> <nfeatures> <scale_factor> <nlevels> <edge_threshold> <max_batch>
// builds the plan and its block as fill_plan does and walks the block:
//   * every table starts on a 256-byte boundary and lies inside the block, no two tables overlap;
//   * the packed resize entries name source pixels inside the source level and agree with the unpacked ones;
//   * every blur tile, FAST strip and describe tile entry decodes to a level of the plan and to coordinates inside that level's tiling,
//     in level-major raster order; tile_cum is monotone and ends at the table's size;
//   * the launch constants hold for every level.
// Prints "plan <w>x<h> levels <n> words <block size> tables <count> dtiles <n> bad <failed checks>"; exit status 1 when bad > 0.
#include "../../visual-slam_amd/csrc/plan_tables.h"

#include <cstdio>
#include <cstdlib>
#include <utility>

static int bad = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { bad++; std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 8) {
        std::fprintf(stderr, "usage: plan_check w h nfeatures scale_factor nlevels edge_threshold max_batch\n");
        return 2;
    }
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), max_batch = std::atoi(argv[7]);
    mo_orb_params prm{};
    prm.nfeatures = std::atoi(argv[3]); prm.scale_factor = (float)std::atof(argv[4]); prm.nlevels = std::atoi(argv[5]);
    prm.edge_threshold = std::atoi(argv[6]); prm.wta_k = 2; prm.patch_size = 31; prm.fast_threshold = 7;
    const int fin_slack[MO_MAX_LEVELS] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    Plan P;
    PlanTables T;
    const char* why = "";
    if (int rc = plan_geometry(P, T, &prm, w, h, max_batch, fin_slack, &why)) {
        std::printf("refused %d %s\n", rc, why);
        return 3;
    }
    std::vector<uint32_t> blk;
    plan_build_tables(P, T, blk);
    const int nl = P.nlevels;

    // the tables as [start, end) word ranges, in the order they were appended
    std::vector<std::pair<size_t, size_t>> tabs;
    for (int L = 1; L < nl; L++) tabs.push_back({T.rs[L].xpk, (size_t)T.rs[L].yc1 + P.lv[L].h});
    for (int s = 0; s < 2; s++) tabs.push_back({T.tile_tab[s], (size_t)T.tile_tab[s] + T.tile_cum[s][nl]});
    tabs.push_back({T.strip_tab, (size_t)T.strip_tab + P.strips_per_frame});
    tabs.push_back({T.dtile_tab, (size_t)T.dtile_tab + T.n_dtiles});
    tabs.push_back({T.dtile_icw, (size_t)T.dtile_icw + 512});
    size_t prev_end = 0;
    for (const auto& t : tabs) {
        CHECK(t.first % 64 == 0);          // 256 bytes
        CHECK(t.first >= prev_end);        // no overlap
        CHECK(t.first - prev_end < 64);    // nothing but padding in between
        CHECK(t.second >= t.first && t.second <= blk.size());
        prev_end = t.second;
    }
    CHECK(prev_end == blk.size());

    // resize coefficients
    for (int L = 1; L < nl; L++) {
        const PlanTables::Resize& t = T.rs[L];
        const LevelInfo &s = P.lv[L - 1], &d = P.lv[L];
        const int wp = (int)(t.ypk - t.xpk), hp = (int)(t.xofs - t.ypk);
        CHECK(t.xpk % 64 == 0 && t.ypk % 64 == 0 && t.xofs % 64 == 0);  // (the packed tables are multiples of 64 entries)
        CHECK(wp >= d.w + 64 && hp >= d.h + 64);                        // a tiling that starts at a margin stays inside
        CHECK(t.xc1 == t.xofs + d.w && t.yofs == t.xc1 + d.w && t.yc1 == t.yofs + d.h);
        for (int axis = 0; axis < 2; axis++) {
            const int n = axis ? d.h : d.w, src = axis ? s.h : s.w, padded = axis ? hp : wp;
            const uint32_t* pk = &blk[axis ? t.ypk : t.xpk];
            const uint32_t* ofs = &blk[axis ? t.yofs : t.xofs];
            const uint32_t* c1 = &blk[axis ? t.yc1 : t.xc1];
            for (int i = 0; i < padded; i++) {
                const int j = std::min(i, n - 1), o = (int)(pk[i] & 0x7FFFu), step = (int)((pk[i] >> 15) & 1u), wgt = (int)(pk[i] >> 16);
                CHECK(o == (int)ofs[j] && wgt == (int)c1[j]);
                CHECK(o >= 0 && o + step < src && wgt >= 0 && wgt <= 256);
                CHECK(step == (o + 1 < src ? 1 : 0));
            }
        }
    }

    // blur tiles
    for (int slot = 0; slot < 2; slot++) {
        const int margin = slot ? mo_blur_margin(P.edge_threshold) : 0;
        const uint32_t* tab = &blk[T.tile_tab[slot]];
        CHECK(T.tile_cum[slot][0] == 0);
        for (int L = 0; L < nl; L++) {
            const int tx = (std::max(P.lv[L].w - 2 * margin, 1) + BT_W - 1) / BT_W, ty = (std::max(P.lv[L].h - 2 * margin, 1) + BT_H - 1) / BT_H;
            CHECK(T.tile_cum[slot][L + 1] >= T.tile_cum[slot][L]);
            CHECK(T.tile_cum[slot][L + 1] - T.tile_cum[slot][L] == tx * ty);
            for (int i = T.tile_cum[slot][L]; i < T.tile_cum[slot][L + 1]; i++) {
                const int k = i - T.tile_cum[slot][L];
                CHECK((int)(tab[i] & 0xFF) == L && (int)((tab[i] >> 8) & 0xFFF) == k % tx && (int)(tab[i] >> 20) == k / tx);
                // the tile's first pixel lies inside the level (or is the one tile of a level the margin swallows)
                CHECK(margin + (k % tx) * BT_W < std::max(P.lv[L].w - margin, margin + 1) && margin + (k / tx) * BT_H < std::max(P.lv[L].h - margin, margin + 1));
            }
        }
    }

    // FAST strips
    {
        const uint32_t* tab = &blk[T.strip_tab];
        int n = 0;
        for (int L = 0; L < nl; L++) {
            CHECK(P.lv[L].strip_base == n);
            for (int st = 0; st < P.lv[L].nstrips; st++, n++) {
                CHECK((int)(tab[n] & 0xFF) == L && (int)(tab[n] >> 8) == st);
                CHECK(st * P.lv[L].strip_rows < P.lv[L].bh);
            }
        }
        CHECK(P.strips_per_frame == std::max(n, 1));
        if (n == 0) CHECK(tab[0] >> 8 == 0xFFFFFFu);  // the one strip of a plan without strips: no level has that many, k_fast returns
    }

    // describe tiles and centroid weights
    {
        const uint32_t* tab = &blk[T.dtile_tab];
        int n = 0;
        for (int L = 0; L < nl; L++) {
            const int tx = (P.lv[L].bw + DT_W - 1) / DT_W, ty = (P.lv[L].bh + DT_H - 1) / DT_H;
            for (int k = 0; k < tx * ty; k++, n++) {
                CHECK(n < T.n_dtiles);
                if (n >= T.n_dtiles) break;
                CHECK((int)(tab[n] & 0xFF) == L && (int)((tab[n] >> 8) & 0xFFF) == k % tx && (int)(tab[n] >> 20) == k / tx);
                CHECK((k % tx) * DT_W < P.lv[L].bw && (k / tx) * DT_H < P.lv[L].bh);
            }
        }
        CHECK(n == T.n_dtiles);
        const uint32_t* icw = &blk[T.dtile_icw];
        CHECK(T.dtile_icw % 4 == 0);  // rows read as uint4
        for (int r = 0; r < 32; r++)
            for (int c4 = 0; c4 < 8; c4++)
                for (int b = 0; b < 4; b++) {
                    const int u = 4 * c4 - 15 + b, d = r < 31 ? P.umax[r < 15 ? 15 - r : r - 15] : -1;
                    const bool in = r < 31 && u >= -d && u <= d;
                    CHECK(((icw[r * 16 + c4] >> (8 * b)) & 0xFF) == (in ? (uint32_t)(u + 16) : 0u));
                    CHECK(((icw[r * 16 + 8 + c4] >> (8 * b)) & 0xFF) == (in ? 1u : 0u));
                }
    }

    // launch constants
    for (int L = 0; L < nl; L++) {
        const LevelInfo& v = P.lv[L];
        CHECK(T.score_bytes >= (size_t)(v.strip_rows + 2) * (v.bw + 2) && T.score_bytes % 16 == 0);
        CHECK(T.tw_need >= v.bw + 8 && T.max_rows >= v.strip_rows && T.max_strips >= v.nstrips);
    }
    CHECK(mo_fast_tw(T.tw_need) >= T.tw_need || T.tw_need > 4160);
    CHECK(T.max_strips <= SEL_MAXSTRIPS);
    CHECK(T.score_bytes + (size_t)(T.max_rows + 8) * mo_fast_tw(T.tw_need) + 16 <= 128 * 1024);

    std::printf("plan %dx%d levels %d words %zu tables %zu dtiles %d bad %d\n", w, h, nl, blk.size(), tabs.size(), T.n_dtiles, bad);
    return bad ? 1 : 0;
}
