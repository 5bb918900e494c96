// plan_tables.h -- the host side of a plan: what one (image size, ORB parameters) pair fixes before any frame arrives.
//
// The plan holds everything the kernels need that OpenCV derives on the host inside ORB_Impl::detectAndCompute (level scales and
// sizes, per-level quotas, the circular-patch umax table, the INTER_LINEAR_EXACT coefficient tables, the quantised Gaussian taps), in
// the same float/double expressions cv2 uses (reference call site: src/orbslam2/extractor.py:38-48,65), and the tables and constants
// of this library's own launches.  plan_geometry fills the Plan (a kernel argument) and the launch constants, plan_build_tables
// appends every lookup table to ONE block of 32-bit words and records where each starts, plan_build_tile_records writes the per-tile
// records of the blurring k_resize2 into a second vector.  Plain C++ without a HIP call: fill_plan (ctx.hip) uploads the block with the
// records behind it, tests/native/plan_check.cpp and tests/native/tile_records_check.cpp walk them on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdint.h>
#include <vector>

#include "../../include/vslam_amd.h"

#define MO_MAX_LEVELS 12
#define MO_HALF_PATCH 15
#define MO_STRIP_ROWS 8
// rows per FAST strip in a context for one or two frames at a time (max_batch <= 2): such a call waits for the longest strip's chain, so
// shorter strips on more workgroups cut it (FAST stage of one 640x480 frame: 26.3 / 18.2 / 15.5 / 14.2 us at 8 / 4 / 3 / 2 rows; the
// selection's gather pays 2 us for the extra strips; 1 row: slower again; profiles/r04_ab_strip_rows_single.txt)
#ifndef MO_STRIP_ROWS_LATENCY
#define MO_STRIP_ROWS_LATENCY 2
#endif
#define SEL_MAXSTRIPS 2047  // strips of one level that k_select's prefix table (dynamic LDS, behind the record window) holds

// tile sizes of the kernels whose tile tables are built here (orb_kernels.hip)
#define BT_W 64
#define BT_H 58   // k_blur, output rows per tile: 58 + 6 halo rows = 32 row pairs, two passes of 16 (round 1: 26 rows; half the workgroups,
                  // 10 % instead of 23 % halo rows)
#ifndef DT_W
#define DT_W 128   // k_describe_tiles, measured on MI355X (profiles/r03_ab_describe.txt): 64 x 64 tiles of 128 threads 0.334 ms, 128 x 64 tiles of 256 threads 0.273 ms
#endif
#define DT_H 64
#ifndef DT_SPLIT_LATENCY
#define DT_SPLIT_LATENCY 4           // workgroups per describe tile in calls on one or two frames (a power of two)
#endif
#define RS_TW 64   // k_resize2 / k_resize: output tile of one workgroup
#define RS_TH 64
// the blurring form of k_resize2 (orb_kernels.hip): the partition of level L-1 one workgroup blurs and the window it stages
#define RB_PW 80                      // partition columns (multiple of 4)
#define RB_PH 80                      // partition rows
#define RB_WR 88                      // window rows
#define RB_WP 96                      // window pitch in bytes: window columns + 8 (the resize's third dword may run past it)

// One record per workgroup of the blurring k_resize2: what that kernel's prologue derived from its arguments and six dependent reads of
// xpk / ypk, for every (level L >= 1, tile by * gx + bx of the launch grid).  A function of the plan alone, so plan_build_tile_records states
// it once and the kernel fetches its record with one wave-uniform 64-byte load.  Words:
#define RB_REC_WORDS 16
enum {
    RBR_TX0, RBR_TY0,  // first output column / row of the resize tile
    RBR_GOFF,          // byte offset of the window's first pixel in level L-1: wy0 * pitch + wx0
    RBR_GEO,           // window rows nwr | window dwords per row ndw << 16
    RBR_FLG,           // 16-byte pieces per window row np16 | interior << 8 (the 16-byte staging form: see plan_build_tile_records) | inside << 9
                       // (the whole window inside the level: the dword staging form needs no REFLECT_101)
    RBR_LDS_RS,        // level pixel (y, x) lies at byte LDS_RS + y * RB_WP + x of the window buffer: -(wy0 * RB_WP + wx0)
    RBR_LDS_ROW,       // byte offset in the window buffer of the blur row pass' first dword: (r0 - 3 - wy0) * RB_WP + (c0 - 4 - wx0)
    RBR_R, RBR_C,      // blur partition rows r0 | r1 << 16 and columns c0 | c1 << 16 (signed halves: rbr_lo / rbr_hi)
    RBR_Q,             // quads per partition row nq | row pairs in npr << 8 | row pairs out nop << 16
    RBR_INVQ,          // 2^20 / nq + 1: (t * invq) >> 20 == t / nq for t < npr * nq
    RBR_W0,            // window origin wy0 | wx0 << 16 (signed halves)
    RBR_SRC0, RBR_SRC1,  // source rows / columns of the resize tile: sy0 | ab0 << 16, sy1 | ax1 << 16
    RBR_BOUT,          // byte offset of the partition's first output in the blurred level L-1: r0 * bpitch + c0
    RBR_NT             // work items of the row pass npr * nq | of the column pass nop * nq << 16
};
static inline int rbr_lo(uint32_t v) { return (int)(int16_t)(v & 0xFFFFu); }
static inline int rbr_hi(uint32_t v) { return (int)(int16_t)(v >> 16); }

// per-level geometry, uploaded by value as a kernel argument
struct LevelInfo {
    int w, h, pitch;      // level size and row pitch in bytes (level 0: pitch = w, aliases the input)
    int off;              // byte offset of the level inside one frame's raw pyramid slab (level 0: unused)
    int bpitch, boff;     // row pitch / byte offset inside one frame's blurred pyramid slab
    float scale;          // (float)pow((double)scale_factor, L)
    int quota;            // features wanted on this level
    int bx0, by0, bw, bh; // border region [bx0, bx0+bw) x [by0, by0+bh): keypoints allowed here
    uint32_t inv_bw;      // floor(2^32 / bw) + 1 for bw > 1: i / bw == mulhi(i, inv_bw) while i * bw < 2^32
    int strip_rows;       // rows per FAST strip
    int nstrips;          // strips covering the border region
    int strip_cap;        // entries per strip slot
    int strip_base;       // index of this level's first strip among one frame's strips
    int cand_off;         // entry offset of this level's first strip slot in one frame's candidate slab
    int cand_cap;         // total candidate capacity of the level (nstrips * strip_cap)
    int fin_off, fin_cap; // final-keypoint slot of the level in one frame's slab
    int scr_off;          // u64 offset of the level's overflow scratch inside one frame's scratch slab
};

struct Plan {
    int w, h, nlevels;
    int edge_threshold, fast_threshold, select_order, nfeatures;
    int pyr_stride;      // bytes per frame of the raw pyramid slab (levels 1..n-1)
    int blur_stride;     // bytes per frame of the blurred pyramid slab (levels 0..n-1)
    int strips_per_frame;
    int cand_stride;     // candidate entries (u32) per frame
    int fin_stride;      // final entries per frame
    int umax[MO_HALF_PATCH + 1];
    int gk[7];           // 7-tap Gaussian, 8 fractional bits
    LevelInfo lv[MO_MAX_LEVELS];
};

// margins of the levels nothing in the batched pipeline reads (see orb_launch_blur / orb_launch_pyramid)
inline int mo_blur_margin(int edge_threshold) { return (edge_threshold - 19) & ~3; }
inline int mo_pyr_margin(int edge_threshold) { return std::max(mo_blur_margin(edge_threshold) - 4, 0); }

static inline size_t mo_align(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }

// LDS pixel-tile pitch k_fast is instantiated with for a plan whose widest level needs tw_need columns
// (640-wide frames take 608: 8 workgroups per CU)
static inline int mo_fast_tw(int tw_need) { return tw_need <= 608 ? 608 : tw_need <= 704 ? 704 : tw_need <= 1344 ? 1344 : tw_need <= 2112 ? 2112 : 4160; }

// Where the tables start inside the plan's block (32-bit word offsets, every table on a 256-byte boundary), and the constants the
// launchers would otherwise derive from the levels on every call.
struct PlanTables {
    size_t scratch_stride = 0;     // u64 entries per frame of overflow scratch (k_select)
    size_t score_bytes = 0;        // k_fast: score plane of the largest strip; tw_need: columns of the widest level's LDS tile; max_rows: longest strip
    int tw_need = 0, max_rows = 1;
    int max_strips = 1;            // k_select: strips of the level that has most (its prefix table)
    // INTER_LINEAR_EXACT coefficients of level L >= 1, one table per level: xpk | ypk | xofs | xc1 | yofs | yc1.  Packed per output
    // column / row (k_resize2), padded to a multiple of 64 entries with the last one: source offset (15 bits) | (right / lower neighbour
    // offset - offset) << 15 | weight of that neighbour in 1/256 units << 16; then the same unpacked (k_resize)
    struct Resize {
        uint32_t xpk = 0, ypk = 0, xofs = 0, xc1 = 0, yofs = 0, yc1 = 0;
        bool two_pass_ok = true;   // k_resize2's 8-byte source window holds every group of 4 output columns
    } rs[MO_MAX_LEVELS];
    uint32_t tile_tab[2] = {};                 // k_blur: tile -> level | tile column << 8 | tile row << 20; [0]: whole levels, [1]: without the margin mo_blur_margin
    int tile_cum[2][MO_MAX_LEVELS + 1] = {};   // tiles of levels < L (the tables are level-major: a prefix blurs the first levels)
    uint32_t strip_tab = 0;                    // k_fast: strip of a frame -> level | strip of the level << 8
    uint32_t dtile_tab = 0, dtile_icw = 0;     // k_describe_tiles: tile -> level | column << 8 | row << 20; the intensity-centroid weights [32 rows][8 weight + 8 mask dwords]
    int n_dtiles = 0;
    // the tile records (plan_build_tile_records), uploaded behind the block: tile_rec is their word offset in that buffer, rb[L].rec the
    // word offset of level L's gx * gy resize/blur records among them (no records: gx = gy = 0), built for the margins rb_pyr_margin / rb_margin
    uint32_t tile_rec = 0;
    struct RbLevel { uint32_t rec = 0; int gx = 0, gy = 0, org = 0; } rb[MO_MAX_LEVELS];
    int rb_margin = -1, rb_pyr_margin = -1;
};

static inline int cv_round_f(float v) { return (int)lrintf(v); }
static inline int cv_round_d(double v) { return (int)lrint(v); }
static inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

// INTER_LINEAR_EXACT coefficient table of one axis (interpolationLinear<ufixedpoint16>::getCoeffs):
// offset + the weight of the right/lower neighbour in 1/256 units (left weight = 256 - c1).
inline void mo_linear_coeffs(int srcsize, int dstsize, std::vector<int>& ofs, std::vector<int>& c1) {
    ofs.assign(dstsize, 0);
    c1.assign(dstsize, 0);
    double inv_scale = (double)dstsize / (double)srcsize;
    double scale = 1.0 / inv_scale;
    int minofst = 0, maxofst = dstsize;
    for (int val = 0; val < dstsize; val++) {
        double fval = scale * ((double)val + 0.5) - 0.5;
        int ival = (int)std::floor(fval);
        if (ival >= 0 && srcsize > 1) {
            if (ival < srcsize - 1) {
                ofs[val] = ival;
                c1[val] = cv_round_d((fval - (double)ival) * 256.0);
            } else {
                ofs[val] = srcsize - 1;
                maxofst = std::min(maxofst, val);
            }
        } else {
            minofst = std::max(minofst, val + 1);
        }
    }
    for (int val = 0; val < dstsize; val++) {
        if (val < minofst) { ofs[val] = 0; c1[val] = 0; }
        if (val >= maxofst) { ofs[val] = srcsize - 1; c1[val] = 0; }
    }
}

// The Plan and the launch constants of an image size and parameter set that mo_build_plan has validated.  max_batch: the context's
// (one or two frames at a time: shorter strips); fin_slack: its per-level growth factors of the final-keypoint slots.  A geometry the
// kernels do not cover returns its error code and leaves the text in *why.
inline int plan_geometry(Plan& P, PlanTables& T, const mo_orb_params* p, int w, int h, int max_batch, const int* fin_slack, const char** why) {
    std::memset(&P, 0, sizeof(P));
    P.w = w; P.h = h; P.nlevels = p->nlevels;
    P.edge_threshold = p->edge_threshold;
    P.fast_threshold = std::min(std::max(p->fast_threshold, 0), 255);
    P.select_order = p->select_order;
    P.nfeatures = p->nfeatures;

    // per-level quotas (computeKeyPoints)
    int nl = p->nlevels;
    {
        float factor = (float)(1.0 / (double)p->scale_factor);
        float nd = p->nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nl));
        int sum = 0;
        for (int L = 0; L < nl - 1; L++) {
            P.lv[L].quota = cv_round_f(nd);
            sum += P.lv[L].quota;
            nd *= factor;
        }
        P.lv[nl - 1].quota = std::max(p->nfeatures - sum, 0);
    }
    // umax of the radius-15 disc
    {
        int umax[MO_HALF_PATCH + 2];
        int vmax = (int)std::floor(MO_HALF_PATCH * std::sqrt(2.f) / 2 + 1);
        int vmin = (int)std::ceil(MO_HALF_PATCH * std::sqrt(2.f) / 2);
        for (int v = 0; v <= vmax; ++v) umax[v] = cv_round_d(std::sqrt((double)MO_HALF_PATCH * MO_HALF_PATCH - v * v));
        for (int v = MO_HALF_PATCH, v0 = 0; v >= vmin; --v) {
            while (umax[v0] == umax[v0 + 1]) ++v0;
            umax[v] = v0;
            ++v0;
        }
        for (int v = 0; v <= MO_HALF_PATCH; v++) P.umax[v] = umax[v];
    }
    // Gaussian 7 taps, sigma 2, quantised to 8 fractional bits (sepFilter2D 8u path)
    {
        double k[7], sum = 0;
        for (int i = 0; i < 7; i++) {
            double x = 2.0 * i - 6.0;
            k[i] = std::exp(x * x * (-0.125 / 4.0));
            sum += k[i];
        }
        double mul1 = 1.0 / sum;
        for (int i = 0; i < 7; i++) P.gk[i] = cv_round_f((float)(k[i] * mul1) * 256.f);
    }

    int et = p->edge_threshold;
    int pyr_off = 0, blur_off = 0, strip_base = 0, cand_off = 0, fin_off = 0, scr_off = 0;
    for (int L = 0; L < nl; L++) {
        LevelInfo& v = P.lv[L];
        v.scale = (float)std::pow((double)p->scale_factor, (double)L);
        float inv_scale = 1.0f / v.scale;
        v.w = cv_round_f((float)w * inv_scale);
        v.h = cv_round_f((float)h * inv_scale);
        if (v.w < 1 || v.h < 1) { *why = "pyramid level collapses to zero size; reduce nlevels"; return MO_ERR_ARG; }
        if (L == 0) { v.pitch = w; v.off = 0; }
        else {
            v.pitch = align_up(v.w, 16);
            v.off = pyr_off;
            pyr_off += align_up(v.pitch * v.h, 256);
        }
        v.bpitch = align_up(v.w, 16);
        v.boff = blur_off;
        blur_off += align_up(v.bpitch * v.h, 256);
        if (v.w <= 2 * et || v.h <= 2 * et) { v.bx0 = v.by0 = et; v.bw = v.bh = 0; }
        else { v.bx0 = et; v.by0 = et; v.bw = v.w - 2 * et; v.bh = v.h - 2 * et; }
        v.inv_bw = v.bw > 1 ? 0xFFFFFFFFu / (uint32_t)v.bw + 1u : 0u;
        // (a context for one or two frames at a time: shorter strips, more workgroups - MO_STRIP_ROWS_LATENCY)
        v.strip_rows = max_batch <= 2 ? MO_STRIP_ROWS_LATENCY : MO_STRIP_ROWS;
        while (v.strip_rows > 1 && v.strip_rows * v.bw > 16384) v.strip_rows /= 2;
        // (short strips only while the level stays below the selection kernel's strip limit; mo_create caps frames at 4095 px = 2017 two-row
        //  strips, so this matters only if that cap is raised)
        while (v.strip_rows < MO_STRIP_ROWS && v.bh > 0 && (v.bh + v.strip_rows - 1) / v.strip_rows > SEL_MAXSTRIPS && 2 * v.strip_rows * v.bw <= 16384)
            v.strip_rows *= 2;
        if (v.bw > 16384) { *why = "level too wide"; return MO_ERR_UNSUPPORTED; }
        v.nstrips = v.bh > 0 ? (v.bh + v.strip_rows - 1) / v.strip_rows : 0;
        v.strip_cap = ((v.strip_rows + 1) / 2) * ((v.bw + 1) / 2);
        v.strip_base = strip_base;
        strip_base += v.nstrips;
        v.cand_off = cand_off;
        v.cand_cap = v.nstrips * v.strip_cap;
        cand_off += v.cand_cap;
        v.fin_off = fin_off;
        v.fin_cap = (int)std::max<long long>(1, std::min<long long>(v.cand_cap, (4ll * v.quota + 256) * fin_slack[L]));
        fin_off += v.fin_cap;
        v.scr_off = scr_off;
        // u64 records B + u32 records A + u16 partner positions + u64 ballots, in u64 units
        scr_off += v.cand_cap + (v.cand_cap + 1) / 2 + (v.cand_cap / 2 + 8) / 4 + 2 + v.cand_cap / 64 + 12;
    }
    P.pyr_stride = std::max(pyr_off, 256);
    P.blur_stride = blur_off;
    P.strips_per_frame = std::max(strip_base, 1);
    P.cand_stride = std::max(cand_off, 1);
    P.fin_stride = fin_off;
    T.scratch_stride = (size_t)scr_off;

    // launch constants of k_fast and k_select, and the geometries their LDS layouts do not hold
    T.score_bytes = 0; T.tw_need = 0; T.max_rows = 1; T.max_strips = 1;
    for (int L = 0; L < nl; L++) {
        const LevelInfo& v = P.lv[L];
        T.score_bytes = std::max(T.score_bytes, (((size_t)(v.strip_rows + 2) * (v.bw + 2) + 15) & ~(size_t)15));
        T.tw_need = std::max(T.tw_need, (v.bw + 2 + 6 + 15 + 15) & ~15);
        T.max_rows = std::max(T.max_rows, v.strip_rows);
        T.max_strips = std::max(T.max_strips, v.nstrips);
    }
    if (T.score_bytes + (size_t)(T.max_rows + 8) * mo_fast_tw(T.tw_need) + 16 > 128 * 1024) { *why = "level too wide for the FAST strip kernel"; return MO_ERR_UNSUPPORTED; }
    if (T.max_strips > SEL_MAXSTRIPS) { *why = "too many strips per level"; return MO_ERR_UNSUPPORTED; }
    return MO_OK;
}

// Every lookup table of the plan appended to blk, each on a 256-byte boundary (the centroid weight rows are read as uint4, the packed
// resize tables in 8-byte pieces), and its start recorded in T.
inline void plan_build_tables(const Plan& P, PlanTables& T, std::vector<uint32_t>& blk) {
    auto start = [&blk]() { blk.resize(mo_align(blk.size(), 64), 0u); return (uint32_t)blk.size(); };
    blk.clear();
    // resize coefficients
    for (int L = 1; L < P.nlevels; L++) {
        std::vector<int> xo, xc, yo, yc;
        mo_linear_coeffs(P.lv[L - 1].w, P.lv[L].w, xo, xc);
        mo_linear_coeffs(P.lv[L - 1].h, P.lv[L].h, yo, yc);
        const int dw = P.lv[L].w, dh = P.lv[L].h, wp = ((dw + 63) & ~63) + 64, hp = ((dh + 63) & ~63) + 64;  // + 64: the tiling may start at a margin
        auto pack = [](const std::vector<int>& o, const std::vector<int>& c1, int srcsize, int padded) {
            std::vector<uint32_t> t((size_t)padded);
            for (int i = 0; i < padded; i++) {
                const int j = std::min(i, (int)o.size() - 1), o1 = std::min(o[j] + 1, srcsize - 1);
                t[i] = (uint32_t)o[j] | ((uint32_t)(o1 - o[j]) << 15) | ((uint32_t)c1[j] << 16);
            }
            return t;
        };
        const std::vector<uint32_t> xp = pack(xo, xc, P.lv[L - 1].w, wp), yp = pack(yo, yc, P.lv[L - 1].h, hp);
        // k_resize2 takes the source bytes of 4 adjacent output columns from ONE 8-byte window: right neighbour of the last
        // column - offset of the first <= 7.  Always true below a level ratio of 2; rounded level widths can put the ratio a
        // little above it at scale_factor 2 (333 -> 166), and such a level keeps the gather kernel
        bool window_ok = true;
        for (int x = 0; x < dw && window_ok; x++) {
            const int xl = std::min(x + 3, dw - 1);
            window_ok = std::min(xo[xl] + 1, P.lv[L - 1].w - 1) - xo[x] <= 7;
        }
        PlanTables::Resize& t = T.rs[L];
        t.two_pass_ok = window_ok;
        // one table per level: xpk [wp] | ypk [hp] | xofs [dw] | xc1 [dw] | yofs [dh] | yc1 [dh]
        t.xpk = start(); t.ypk = t.xpk + wp;
        t.xofs = t.ypk + hp; t.xc1 = t.xofs + dw; t.yofs = t.xc1 + dw; t.yc1 = t.yofs + dh;
        blk.insert(blk.end(), xp.begin(), xp.end());
        blk.insert(blk.end(), yp.begin(), yp.end());
        for (const std::vector<int>* v : {&xo, &xc, &yo, &yc}) blk.insert(blk.end(), v->begin(), v->end());
    }
    // blur tiles: the tiling covers [margin, w - margin) x [margin, h - margin) of every level
    for (int slot = 0; slot < 2; slot++) {
        const int margin = slot ? mo_blur_margin(P.edge_threshold) : 0;
        const uint32_t t0 = T.tile_tab[slot] = start();
        for (int L = 0; L < P.nlevels; L++) {
            const int cw = std::max(P.lv[L].w - 2 * margin, 1), chh = std::max(P.lv[L].h - 2 * margin, 1);
            const int tx = (cw + BT_W - 1) / BT_W, ty = (chh + BT_H - 1) / BT_H;
            T.tile_cum[slot][L] = (int)(blk.size() - t0);
            for (int y = 0; y < ty; y++)
                for (int x = 0; x < tx; x++) blk.push_back((uint32_t)L | ((uint32_t)x << 8) | ((uint32_t)y << 20));
        }
        T.tile_cum[slot][P.nlevels] = (int)(blk.size() - t0);
    }
    // FAST strips (level-major: a level range is a strip range)
    T.strip_tab = start();
    blk.resize(blk.size() + (size_t)P.strips_per_frame, 0xFFFFFF00u);  // (no level has that many strips: the kernel returns)
    for (int L = 0; L < P.nlevels; L++)
        for (int st = 0; st < P.lv[L].nstrips; st++) blk[T.strip_tab + (size_t)P.lv[L].strip_base + st] = (uint32_t)L | ((uint32_t)st << 8);
    // describe tiles (level | tile column << 8 | tile row << 20, level-major), then the intensity-centroid weights
    // [32 rows][8 weight + 8 mask dwords]
    T.dtile_tab = start();
    for (int L = 0; L < P.nlevels; L++)
        for (int y = 0; y < (P.lv[L].bh + DT_H - 1) / DT_H; y++)
            for (int x = 0; x < (P.lv[L].bw + DT_W - 1) / DT_W; x++) blk.push_back((uint32_t)L | ((uint32_t)x << 8) | ((uint32_t)y << 20));
    T.n_dtiles = (int)(blk.size() - T.dtile_tab);
    T.dtile_icw = start();
    blk.resize(blk.size() + 512, 0u);
    for (int r = 0; r < 31; r++) {
        const int d = P.umax[r < 15 ? 15 - r : r - 15];
        for (int c4 = 0; c4 < 8; c4++) {
            uint32_t wv = 0, mv = 0;
            for (int b = 0; b < 4; b++) {
                const int u = 4 * c4 - 15 + b;
                if (u >= -d && u <= d) { wv |= (uint32_t)(u + 16) << (8 * b); mv |= 1u << (8 * b); }
            }
            blk[T.dtile_icw + r * 16 + c4] = wv;
            blk[T.dtile_icw + r * 16 + 8 + c4] = mv;
        }
    }
}

// margin: only [margin, w - margin) x [margin, h - margin) of levels 1.. is produced (a multiple of 4).  The pipeline passes
// the blur's margin - 4 (8 at edge_threshold 31): FAST stages from column 16 / row 27, the Harris and orientation windows stay
// 16 px inside, the blur tiling starts at 12 and reads from 8, and the next level's [8, ..) only needs this level's [9, ..).
// compute() with caller keypoints and the probes pass 0.
static inline int resize_org(const LevelInfo& d, int margin) { return (d.w > 2 * margin + 8 && d.h > 2 * margin + 8) ? margin : 0; }

// The resize/blur records of every level L >= 1 (RBR_* above) appended to out, level-major, tile by * gx + bx within a level, for a
// pipeline that produces the pyramid from pyr_margin and blurs from blur_margin; blk: the block of plan_build_tables (xpk / ypk).  Workgroup
// (bx, by) of the launch of level L owns rows [ypk[ty0] & 0x7FFF, the same for by + 1) and 4-aligned columns [xpk[tx0] & 0x7FFC, the same for
// bx + 1) of level L-1; the first and last row / column of workgroups stretch to the blur region, so the partitions tile it.  Its window is
// the union of the partition plus the blur halo (3 rows, 4 columns) and the source rows / columns of its resize tile.  Rows and columns are
// independent.  A level whose tables do not hold the tiling, or a margin the form does not take, gets no records.
inline void plan_build_tile_records(const Plan& P, PlanTables& T, const std::vector<uint32_t>& blk, int pyr_margin, int blur_margin,
                                    std::vector<uint32_t>& out) {
    out.clear();
    T.rb_margin = blur_margin; T.rb_pyr_margin = pyr_margin;
    const int bm = blur_margin;
    for (int L = 0; L < MO_MAX_LEVELS; L++) T.rb[L] = PlanTables::RbLevel();
    for (int L = 1; L < P.nlevels; L++) {
        const LevelInfo &s = P.lv[L - 1], &d = P.lv[L];
        const PlanTables::Resize& t = T.rs[L];
        const uint32_t *xp = &blk[t.xpk], *yp = &blk[t.ypk];
        const size_t nx = t.ypk - t.xpk, ny = t.xofs - t.ypk;
        PlanTables::RbLevel& rl = T.rb[L];
        const int org = rl.org = resize_org(d, pyr_margin);
        const int gx = (d.w - 2 * org + RS_TW - 1) / RS_TW, gy = (d.h - 2 * org + RS_TH - 1) / RS_TH;
        if (bm < 0 || (bm & 3) || gx < 1 || gy < 1 || (size_t)(org + gx * RS_TW + 1) > nx || (size_t)(org + gy * RS_TH + 1) > ny) continue;
        rl.rec = (uint32_t)out.size(); rl.gx = gx; rl.gy = gy;
        struct Axis { int t0, s0, s1, p0, p1, w0, w1; };  // tile start, source span [s0, s1], partition [p0, p1), window [w0, w1)
        std::vector<Axis> ys((size_t)gy), xs((size_t)gx);
        for (int by = 0; by < gy; by++) {
            Axis& a = ys[(size_t)by];
            a.t0 = org + by * RS_TH;
            const uint32_t ey1 = yp[a.t0 + RS_TH - 1];
            a.s0 = (int)(yp[a.t0] & 0x7FFFu); a.s1 = (int)(ey1 & 0x7FFFu) + (int)((ey1 >> 15) & 1u);
            a.p0 = by == 0 ? bm : a.s0; a.p1 = by == gy - 1 ? s.h - bm : (int)(yp[a.t0 + RS_TH] & 0x7FFFu);
            a.w0 = std::min(a.p0 - 3, a.s0); a.w1 = std::max(a.p1 + 3, a.s1 + 1);
        }
        for (int bx = 0; bx < gx; bx++) {
            Axis& a = xs[(size_t)bx];
            a.t0 = org + bx * RS_TW;
            const uint32_t ex1 = xp[a.t0 + RS_TW - 1];
            a.s0 = (int)(xp[a.t0] & 0x7FFCu); a.s1 = (int)(ex1 & 0x7FFFu) + (int)((ex1 >> 15) & 1u) + 1;  // [ab0, ax1)
            a.p0 = bx == 0 ? bm : a.s0; a.p1 = bx == gx - 1 ? (s.w - bm + 3) & ~3 : (int)(xp[a.t0 + RS_TW] & 0x7FFCu);
            a.w0 = std::min(a.p0 - 4, a.s0); a.w1 = std::max(a.p1 + 4, (a.s1 + 3) & ~3);
        }
        auto pack = [](int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); };
        for (int by = 0; by < gy; by++)
            for (int bx = 0; bx < gx; bx++) {
                const Axis &y = ys[(size_t)by], &x = xs[(size_t)bx];
                const int nwr = y.w1 - y.w0, ndw = (x.w1 - x.w0) >> 2, np16 = (ndw + 3) >> 2;
                const bool inside = y.w0 >= 0 && y.w1 <= s.h && x.w0 >= 0 && x.w1 <= s.w;
                // the 16-byte staging form copies level bytes as they lie: its rows must be rows of the level, its pieces end inside the row's
                // pitch, and every byte a value depends on - the taps of the partition's last column x.p1 - 1, the resize's source columns
                // below x.s1 - must be a pixel.  The window itself is rounded up to dwords and may run <= 3 bytes past the level's width
                // into the row's padding (the last tile column of a level whose width is no multiple of 4): bytes no value depends on.
                const bool interior = y.w0 >= 0 && y.w1 <= s.h && x.w0 >= 0 && x.w0 + 16 * np16 <= s.pitch && std::max(x.p1 + 3, x.s1) <= s.w;
                const int nq = (x.p1 - x.p0) >> 2, npr = (y.p1 - y.p0 + 7) >> 1, nop = (y.p1 - y.p0 + 1) >> 1;  // quads, row pairs in, row pairs out
                uint32_t r[RB_REC_WORDS];
                r[RBR_TX0] = (uint32_t)x.t0; r[RBR_TY0] = (uint32_t)y.t0;
                r[RBR_GOFF] = (uint32_t)(y.w0 * s.pitch + x.w0);
                r[RBR_GEO] = pack(nwr, ndw);
                r[RBR_FLG] = ((uint32_t)np16 & 0xFFu) | (interior ? 1u << 8 : 0u) | (inside ? 1u << 9 : 0u);
                r[RBR_LDS_RS] = (uint32_t)(-(y.w0 * RB_WP + x.w0));
                r[RBR_LDS_ROW] = (uint32_t)((y.p0 - 3 - y.w0) * RB_WP + (x.p0 - 4 - x.w0));
                r[RBR_R] = pack(y.p0, y.p1); r[RBR_C] = pack(x.p0, x.p1);
                r[RBR_Q] = ((uint32_t)nq & 0xFFu) | (((uint32_t)npr & 0xFFu) << 8) | ((uint32_t)nop << 16);
                r[RBR_INVQ] = 0x100000u / (uint32_t)std::max(nq, 1) + 1u;
                r[RBR_W0] = pack(y.w0, x.w0);
                r[RBR_SRC0] = pack(y.s0, x.s0); r[RBR_SRC1] = pack(y.s1, x.s1);
                r[RBR_BOUT] = (uint32_t)(y.p0 * s.bpitch + x.p0);
                r[RBR_NT] = pack(npr * nq, nop * nq);
                out.insert(out.end(), r, r + RB_REC_WORDS);
            }
    }
}

// Plan time: does the blurring form of k_resize2 cover level L - 1's blur region [rb_margin, size - rb_margin) at this geometry, with
// every window and partition inside RB_*?  Read from the records the kernel will read (rec: the vector of plan_build_tile_records); a
// level without records fails.
inline bool orb_plan_resize_blur(const Plan& P, const PlanTables& T, int L, const uint32_t* rec) {
    const LevelInfo& s = P.lv[L - 1];
    const PlanTables::RbLevel& rl = T.rb[L];
    if (rl.gx < 1 || rl.gy < 1) return false;
    for (int by = 0; by < rl.gy; by++) {  // (rows: the same in every record of a tile row)
        const uint32_t* r = rec + rl.rec + (size_t)by * rl.gx * RB_REC_WORDS;
        const int r0 = rbr_lo(r[RBR_R]), r1 = rbr_hi(r[RBR_R]), wy0 = rbr_lo(r[RBR_W0]), nwr = rbr_lo(r[RBR_GEO]), sy1 = rbr_lo(r[RBR_SRC1]);
        if (r1 <= r0 || r1 - r0 > RB_PH || nwr > RB_WR || r1 + 4 - wy0 > RB_WR || sy1 >= s.h) return false;
    }
    for (int bx = 0; bx < rl.gx; bx++) {
        const uint32_t* r = rec + rl.rec + (size_t)bx * RB_REC_WORDS;
        const int c0 = rbr_lo(r[RBR_C]), c1 = rbr_hi(r[RBR_C]), ndw = rbr_hi(r[RBR_GEO]), ax1 = rbr_hi(r[RBR_SRC1]);
        if (c1 <= c0 || c1 - c0 > RB_PW || 4 * ndw + 8 > RB_WP || ax1 > s.w) return false;
    }
    return true;
}
