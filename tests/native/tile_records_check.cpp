// Host check of the plan's tile records (visual-slam_amd/csrc/plan_tables.h: plan_build_tile_records), built once plain and once with
// g++ -fsanitize=address,undefined.  No arguments: it sweeps
//   widths 63 .. 693 in steps of 9 (71 values: every residue mod 16 and mod 64), each with a height out of the same set (rows and columns of a
//   record are independent), edge_threshold 19 .. 40, scale factors 1.1 / 1.2 / 1.5 / 2.0, 1 .. 12 levels and max_batch 1 / 256 (a plan of n
//   levels holds the records of every plan of fewer levels, and max_batch does not enter a record: both cycle with the other parameters)
// and checks for every plan, at the margins fill_plan passes:
//   * every resize/blur record against the prologue k_resize2's blurring form ran before the records existed, restated here from xpk / ypk;
//   * where the plan allows the fused form: the blur partitions cover [margin, size - margin) of level L-1 exactly once, the resize tiles
//     cover the produced region of level L, every window and partition fits RB_WR x RB_WP / RB_PH x RB_PW;
//   * the inside flag against the window's position in the level, the interior flag (the 16-byte staging form) against the position of the
//     bytes a value depends on; the former prologue's condition for that form implies the flag;
//   * (t * invq) >> 20 == t / nq for every t < npr * nq (each (nq, npr) pair once);
//   * the verdict of orb_plan_resize_blur, which reads the records, against the former one, restated here.
// Prints "tile records: plans <n> refused <n> levels <n> records <n> fused <n> interior <n> border <n> bad <failed checks>"; exit status 1 when bad > 0.
#include "../../visual-slam_amd/csrc/plan_tables.h"

#include <cstdio>
#include <cstdlib>

static long bad = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { if (bad++ < 40) std::fprintf(stderr, "line %d: %s  [%s]\n", __LINE__, #cond, g_case); } \
    } while (0)
static char g_case[160];

// the prologue of k_resize2<true> as it stood: every value a workgroup (bx, by) of the launch of level L derived from the kernel arguments
// and six wave-uniform reads of xpk / ypk
struct Old {
    int tx0, ty0, sy0, sy1, ab0, ax1, r0, r1, c0, c1, wy0, wy1, wx0, wx1, nwr, ndw, np16, nq, npr, nop;
    bool inside, interior;  // interior: the former condition of the 16-byte staging form
    uint32_t invq;
};
static Old old_prologue(const LevelInfo& s, const uint32_t* xpk, const uint32_t* ypk, int org, int bm, int bx, int by, int gx, int gy) {
    Old o;
    const int sw = s.w, sh = s.h, spitch = s.pitch;
    o.tx0 = org + bx * RS_TW; o.ty0 = org + by * RS_TH;
    const uint32_t ey0 = ypk[o.ty0], ey1 = ypk[o.ty0 + RS_TH - 1], ex1 = xpk[o.tx0 + RS_TW - 1];
    o.sy0 = (int)(ey0 & 0x7FFFu); o.sy1 = (int)(ey1 & 0x7FFFu) + (int)((ey1 >> 15) & 1u);
    o.ab0 = (int)(xpk[o.tx0] & 0x7FFCu); o.ax1 = (int)(ex1 & 0x7FFFu) + (int)((ex1 >> 15) & 1u) + 1;
    o.r0 = by == 0 ? bm : o.sy0; o.r1 = by == gy - 1 ? sh - bm : (int)(ypk[o.ty0 + RS_TH] & 0x7FFFu);
    o.c0 = bx == 0 ? bm : o.ab0; o.c1 = bx == gx - 1 ? (sw - bm + 3) & ~3 : (int)(xpk[o.tx0 + RS_TW] & 0x7FFCu);
    o.wy0 = std::min(o.r0 - 3, o.sy0); o.wy1 = std::max(o.r1 + 3, o.sy1 + 1);
    o.wx0 = std::min(o.c0 - 4, o.ab0); o.wx1 = std::max(o.c1 + 4, (o.ax1 + 3) & ~3);
    o.nwr = o.wy1 - o.wy0; o.ndw = (o.wx1 - o.wx0) >> 2;
    o.inside = o.wy0 >= 0 && o.wy1 <= sh && o.wx0 >= 0 && o.wx1 <= sw;
    o.np16 = (o.ndw + 3) >> 2;
    o.interior = o.inside && o.wx0 + 16 * o.np16 <= spitch;
    o.nq = (o.c1 - o.c0) >> 2; o.npr = (o.r1 - o.r0 + 7) >> 1; o.nop = (o.r1 - o.r0 + 1) >> 1;
    o.invq = 0x100000u / (uint32_t)std::max(o.nq, 1) + 1u;
    return o;
}

// orb_plan_resize_blur as it stood before it read the records
static bool old_verdict(const Plan& P, int L, const uint32_t* xp, size_t nx, const uint32_t* yp, size_t ny, int margin, int blur_margin) {
    const LevelInfo& s = P.lv[L - 1];
    const LevelInfo& d = P.lv[L];
    const int bm = blur_margin, org = (d.w > 2 * margin + 8 && d.h > 2 * margin + 8) ? margin : 0;
    if (bm < 0 || (bm & 3)) return false;
    const int gx = (d.w - 2 * org + RS_TW - 1) / RS_TW, gy = (d.h - 2 * org + RS_TH - 1) / RS_TH;
    if (gx < 1 || gy < 1 || (size_t)(org + gx * RS_TW + 1) > nx || (size_t)(org + gy * RS_TH + 1) > ny) return false;
    for (int by = 0; by < gy; by++) {
        const int ty0 = org + by * RS_TH;
        const uint32_t ey1 = yp[ty0 + RS_TH - 1];
        const int sy0 = (int)(yp[ty0] & 0x7FFFu), sy1 = (int)(ey1 & 0x7FFFu) + (int)((ey1 >> 15) & 1u);
        const int r0 = by == 0 ? bm : sy0, r1 = by == gy - 1 ? s.h - bm : (int)(yp[ty0 + RS_TH] & 0x7FFFu);
        const int wy0 = std::min(r0 - 3, sy0), wy1 = std::max(r1 + 3, sy1 + 1);
        if (r1 <= r0 || r1 - r0 > RB_PH || wy1 - wy0 > RB_WR || r1 + 4 - wy0 > RB_WR || sy1 >= s.h) return false;
    }
    for (int bx = 0; bx < gx; bx++) {
        const int tx0 = org + bx * RS_TW;
        const uint32_t ex1 = xp[tx0 + RS_TW - 1];
        const int ab0 = (int)(xp[tx0] & 0x7FFCu), ax1 = (int)(ex1 & 0x7FFFu) + (int)((ex1 >> 15) & 1u) + 1;
        const int c0 = bx == 0 ? bm : ab0, c1 = bx == gx - 1 ? (s.w - bm + 3) & ~3 : (int)(xp[tx0 + RS_TW] & 0x7FFCu);
        const int wx0 = std::min(c0 - 4, ab0), wx1 = std::max(c1 + 4, (ax1 + 3) & ~3);
        if (c1 <= c0 || c1 - c0 > RB_PW || wx1 - wx0 + 8 > RB_WP || ax1 > s.w) return false;
    }
    return true;
}

int main() {
    static bool seen_q[256][256];
    long plans = 0, refused = 0, levels = 0, records = 0, fused = 0, n_interior = 0, n_border = 0;
    const float scales[4] = {1.1f, 1.2f, 1.5f, 2.0f};
    const int fin_slack[MO_MAX_LEVELS] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    int seen_levels = 0, seen_batch = 0;
    for (int i = 0; i < 71; i++)
        for (int et = 19; et <= 40; et++)
            for (int si = 0; si < 4; si++) {
                const int w = 63 + 9 * i, h = 63 + 9 * ((i * 37 + 11) % 71);
                const int nl = 1 + (i + et + 5 * si) % 12, max_batch = ((i + et + si) & 1) ? 256 : 1;
                std::snprintf(g_case, sizeof g_case, "%dx%d et %d scale %.1f levels %d batch %d", w, h, et, scales[si], nl, max_batch);
                mo_orb_params prm{};
                prm.nfeatures = 500; prm.scale_factor = scales[si]; prm.nlevels = nl; prm.edge_threshold = et;
                prm.wta_k = 2; prm.patch_size = 31; prm.fast_threshold = 7;
                Plan P;
                PlanTables T;
                const char* why = "";
                if (plan_geometry(P, T, &prm, w, h, max_batch, fin_slack, &why)) { refused++; continue; }
                plans++;
                seen_levels |= 1 << nl; seen_batch |= max_batch == 1 ? 1 : 2;
                std::vector<uint32_t> blk, rec;
                plan_build_tables(P, T, blk);
                const int pm = mo_pyr_margin(et), bm = mo_blur_margin(et);
                plan_build_tile_records(P, T, blk, pm, bm, rec);
                CHECK(T.rb_margin == bm && T.rb_pyr_margin == pm);
                CHECK(rec.size() % RB_REC_WORDS == 0);
                size_t expect_words = 0;
                for (int L = 1; L < nl; L++) {
                    levels++;
                    const PlanTables::Resize& t = T.rs[L];
                    const PlanTables::RbLevel& rl = T.rb[L];
                    const LevelInfo &s = P.lv[L - 1], &d = P.lv[L];
                    const uint32_t *xpk = &blk[t.xpk], *ypk = &blk[t.ypk];
                    const size_t nx = t.ypk - t.xpk, ny = t.xofs - t.ypk;
                    const bool was = old_verdict(P, L, xpk, nx, ypk, ny, pm, bm);
                    const bool now = orb_plan_resize_blur(P, T, L, rec.data());
                    CHECK(was == now);
                    const int org = (d.w > 2 * pm + 8 && d.h > 2 * pm + 8) ? pm : 0;
                    const int gx = (d.w - 2 * org + RS_TW - 1) / RS_TW, gy = (d.h - 2 * org + RS_TH - 1) / RS_TH;
                    const bool tables_hold = gx >= 1 && gy >= 1 && (size_t)(org + gx * RS_TW + 1) <= nx && (size_t)(org + gy * RS_TH + 1) <= ny;
                    CHECK(rl.org == org);
                    if (!tables_hold) { CHECK(rl.gx == 0 && rl.gy == 0 && !now); continue; }
                    CHECK(rl.gx == gx && rl.gy == gy && rl.rec == expect_words && rl.rec % 16 == 0);
                    if (rl.gx != gx || rl.gy != gy || rl.rec + (size_t)gx * gy * RB_REC_WORDS > rec.size()) { bad++; continue; }
                    expect_words += (size_t)gx * gy * RB_REC_WORDS;
                    if (now) fused++;
                    std::vector<int> rows_seen((size_t)s.h, 0), cols_seen((size_t)s.pitch + 8, 0);
                    for (int by = 0; by < gy; by++)
                        for (int bx = 0; bx < gx; bx++) {
                            records++;
                            const uint32_t* r = &rec[rl.rec + (size_t)(by * gx + bx) * RB_REC_WORDS];
                            const Old o = old_prologue(s, xpk, ypk, org, bm, bx, by, gx, gy);
                            // the record against the former prologue
                            CHECK((int)r[RBR_TX0] == o.tx0 && (int)r[RBR_TY0] == o.ty0);
                            CHECK((int)(r[RBR_SRC0] & 0xFFFF) == o.sy0 && (int)(r[RBR_SRC0] >> 16) == o.ab0);
                            CHECK((int)(r[RBR_SRC1] & 0xFFFF) == o.sy1 && (int)(r[RBR_SRC1] >> 16) == o.ax1);
                            CHECK(rbr_lo(r[RBR_R]) == o.r0 && rbr_hi(r[RBR_R]) == o.r1 && rbr_lo(r[RBR_C]) == o.c0 && rbr_hi(r[RBR_C]) == o.c1);
                            const bool interior = ((r[RBR_FLG] >> 8) & 1u) != 0;
                            CHECK(!o.interior || interior);  // the flag is wider than the former condition, never narrower
                            CHECK(rbr_lo(r[RBR_W0]) == o.wy0 && rbr_hi(r[RBR_W0]) == o.wx0);
                            CHECK(rbr_lo(r[RBR_GEO]) == o.nwr && rbr_hi(r[RBR_GEO]) == o.ndw);
                            CHECK((int)(r[RBR_FLG] & 0xFF) == o.np16 && ((r[RBR_FLG] >> 9) & 1u) == (o.inside ? 1u : 0u));
                            CHECK((int)r[RBR_GOFF] == o.wy0 * s.pitch + o.wx0);
                            CHECK((int)r[RBR_LDS_RS] == -(o.wy0 * RB_WP + o.wx0));
                            CHECK((int)r[RBR_LDS_ROW] == (o.r0 - 3 - o.wy0) * RB_WP + (o.c0 - 4 - o.wx0));
                            CHECK((int)r[RBR_BOUT] == o.r0 * s.bpitch + o.c0);
                            if (now) {  // (a refused level's records are not read by the kernel; their packed counts may not hold the values)
                                CHECK((int)(r[RBR_Q] & 0xFF) == o.nq && (int)((r[RBR_Q] >> 8) & 0xFF) == o.npr && (int)(r[RBR_Q] >> 16) == o.nop);
                                CHECK(r[RBR_INVQ] == o.invq);
                                CHECK((int)(r[RBR_NT] & 0xFFFF) == o.npr * o.nq && (int)(r[RBR_NT] >> 16) == o.nop * o.nq);
                                // the windows and partitions inside the kernel's buffers; every LDS byte the phases touch inside s_px / s_row
                                CHECK(o.nwr >= 1 && o.nwr <= RB_WR && 4 * o.ndw + 8 <= RB_WP && 16 * o.np16 <= RB_WP);
                                CHECK(o.r1 > o.r0 && o.r1 - o.r0 <= RB_PH && o.c1 > o.c0 && o.c1 - o.c0 <= RB_PW && ((o.c0 | o.c1 | o.wx0) & 3) == 0);
                                CHECK((int)r[RBR_LDS_ROW] >= 0 && (o.r0 - 3 - o.wy0) + 2 * o.npr <= RB_WR && (o.c0 - 4 - o.wx0) + 4 * o.nq + 8 <= RB_WP);
                                CHECK(o.npr * RB_PW * 4 <= (RB_PH / 2 + 4) * RB_PW * 4 && o.nop + 3 <= o.npr);
                                CHECK(o.sy0 >= o.wy0 && o.sy1 < o.wy0 + o.nwr && o.ab0 >= o.wx0 && o.ax1 <= o.wx0 + 4 * o.ndw);
                                // the reciprocal
                                if (!seen_q[o.nq][o.npr]) {
                                    seen_q[o.nq][o.npr] = true;
                                    for (uint32_t t2 = 0; t2 < (uint32_t)(o.npr * o.nq); t2++) CHECK(((t2 * o.invq) >> 20) == t2 / (uint32_t)o.nq);
                                }
                                for (int y = o.r0; y < o.r1; y++) rows_seen[(size_t)y]++;
                                for (int x = o.c0; x < o.c1; x++) cols_seen[(size_t)x]++;
                            }
                            // the flags against the window's position in the level
                            const bool in = o.wy0 >= 0 && o.wy0 + o.nwr <= s.h && o.wx0 >= 0 && o.wx0 + 4 * o.ndw <= s.w;
                            CHECK(in == (((r[RBR_FLG] >> 9) & 1u) != 0));
                            // the 16-byte form: window rows are level rows, every piece ends inside the row's pitch, and the bytes a value depends
                            // on are pixels - the row pass reads columns [c0 - 3, c1 + 3) for its outputs [c0, c1), the resize [ab0, ax1)
                            const bool rows_in = o.wy0 >= 0 && o.wy0 + o.nwr <= s.h, pieces_in = o.wx0 >= 0 && o.wx0 + 16 * o.np16 <= s.pitch;
                            const bool used_in = o.c0 - 3 >= 0 && o.c1 + 3 <= s.w && o.ab0 >= 0 && o.ax1 <= s.w;
                            CHECK(interior == (rows_in && pieces_in && used_in));
                            if (bm == 0 && (bx == 0 || by == 0 || bx == gx - 1 || by == gy - 1)) CHECK(!o.inside);  // the halo of a border partition leaves the level
                            if (interior) n_interior++; else n_border++;
                        }
                    if (now) {
                        // every row / column of the blur region in gy x gx partitions: once per tile row / column, none outside it
                        for (int y = 0; y < s.h; y++) CHECK(rows_seen[(size_t)y] == (y >= bm && y < s.h - bm ? gx : 0));
                        for (int x = 0; x < s.pitch + 8; x++) {
                            if (x >= bm && x < s.w - bm) CHECK(cols_seen[(size_t)x] == gy);
                            else if (x < bm || x >= ((s.w - bm + 3) & ~3)) CHECK(cols_seen[(size_t)x] == 0);
                        }
                        CHECK(((s.w - bm + 3) & ~3) <= s.bpitch);  // the <= 3 columns past the region land in the row's padding
                        // the resize tiles: contiguous from org, none empty, the last one reaches the end of the produced region
                        CHECK(org + (gx - 1) * RS_TW < d.w - org && org + gx * RS_TW >= d.w - org);
                        CHECK(org + (gy - 1) * RS_TH < d.h - org && org + gy * RS_TH >= d.h - org);
                    }
                }
                CHECK(rec.size() == expect_words);
            }
    CHECK(seen_levels == 0x1FFE && seen_batch == 3);
    CHECK(fused > 0 && n_interior > 0 && n_border > 0);
    std::printf("tile records: plans %ld refused %ld levels %ld records %ld fused %ld interior %ld border %ld bad %ld\n", plans, refused, levels, records,
                fused, n_interior, n_border, bad);
    return bad ? 1 : 0;
}
