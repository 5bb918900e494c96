// map_kernels.hip -- the device-resident LocalMapper (reference src/orbslam2/local_mapper.py): keyframe store, map store, the
// device-wide scan and the per-keyframe step add_keyframe runs (store -> growth of one keyframe pair -> cull of every map point ->
// per-keyframe lists and the counts _cull_keyframes reads), one synchronisation per keyframe.  The other users of the map have files
// of their own (map_reloc.hip, map_track.hip, map_ba.hip, map_obs.hip, map_io.hip); map_store.h is what they share.
//
// Stores (structure of arrays, grown by reallocation):
//   keyframes  slot s (creation order, never reused): kps [s][row][28 B], desc [s][row][32], count [s], P = K [R|t] [s][12] f64.
//              The reference indexes keyframes by list POSITION (local_mapper.py:223 self.keyframes[kf_id]); position -> slot is a
//              small table the host rewrites when keyframes are removed (_cull_keyframes pops them and renumbers the ids).
//   map points in the reference's list order: xyz f32 [n][3], colour u8 [n][3], id i32, descriptor reference (keyframe slot, row),
//              the life record {visible, found, born, 0} (map_store.h: map_life_new, map_point_copy; map_ptcull.hip reads and feeds it),
//              observations in CSR form (off [n + 1], keyframe id, keypoint index) in the dict's insertion order.  Two copies: the cull
//              compacts from one into the other, and the host flips them once the call has succeeded.
//
// Map sizes after the growth step are known on the device only: every kernel behind it is launched for an upper bound (the map before
// the step + the query keyframe's keypoints) and reads the live count from the status block, so nothing waits for the host.
//
// -ffp-contract=off (Makefile, every file): the reprojection test rounds each product and sum once, in the order numpy's P @ X_h does.
#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "common.h"
#include "map_rebuild.h"   // (map_store.h with it)

#define MAP_SCAN_BLOCK 256
#define MAP_SCAN_ITEMS 4
#define MAP_SCAN_TILE (MAP_SCAN_BLOCK * MAP_SCAN_ITEMS)
#define MAP_LIST_CHUNK 1024   // observation entries per one-wave block of the counting sort
#define MAP_MAX_KF 16384      // keyframes the counting sort's LDS cursors hold (64 KB)

// ---- device-wide exclusive scan of int32 (three launches: per-tile scan, one-block scan of the tile sums, add) ------------------
__global__ __launch_bounds__(MAP_SCAN_BLOCK) void k_scan_tiles(const int32_t* __restrict__ in, int32_t* __restrict__ out, int32_t* __restrict__ part, int n) {
    __shared__ int lw[40];
    const size_t base = (size_t)blockIdx.x * MAP_SCAN_TILE + (size_t)threadIdx.x * MAP_SCAN_ITEMS;
    int v[MAP_SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < MAP_SCAN_ITEMS; k++) { v[k] = base + k < (size_t)n ? in[base + k] : 0; s += v[k]; }
    int total;
    int e = block_excl_scan(s, lw, &total);
#pragma unroll
    for (int k = 0; k < MAP_SCAN_ITEMS; k++) { if (base + k < (size_t)n) out[base + k] = e; e += v[k]; }
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// one block: exclusive scan of the tile sums in place, the grand total into *total
__global__ __launch_bounds__(1024) void k_scan_parts(int32_t* __restrict__ part, int np, int32_t* __restrict__ total) {
    __shared__ int lw[40];
    int carry = 0;
    for (int b = 0; b < np; b += 1024) {
        const int i = b + threadIdx.x;
        const int v = i < np ? part[i] : 0;
        int t;
        const int e = block_excl_scan(v, lw, &t);
        if (i < np) part[i] = carry + e;
        carry += t;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(MAP_SCAN_BLOCK) void k_scan_add(int32_t* __restrict__ out, const int32_t* __restrict__ part, int n) {
    const size_t base = (size_t)blockIdx.x * MAP_SCAN_TILE;
    const int add = part[blockIdx.x];
    if (!add) return;
    for (int k = threadIdx.x; k < MAP_SCAN_TILE; k += MAP_SCAN_BLOCK)
        if (base + k < (size_t)n) out[base + k] += add;
}

int map_scan_excl(mo_map* m, const int32_t* in, int32_t* out, int n, int32_t* d_total) {
    mo_ctx* c = m->c;
    const int tiles = std::max(1, (n + MAP_SCAN_TILE - 1) / MAP_SCAN_TILE);
    int rc = m->part.reserve(c, (size_t)tiles);
    if (rc) return rc;
    hipLaunchKernelGGL(k_scan_tiles, dim3(tiles), dim3(MAP_SCAN_BLOCK), 0, c->stream, in, out, m->part, n);
    hipLaunchKernelGGL(k_scan_parts, dim3(1), dim3(1024), 0, c->stream, m->part, tiles, d_total);
    hipLaunchKernelGGL(k_scan_add, dim3(tiles), dim3(MAP_SCAN_BLOCK), 0, c->stream, out, m->part, n);
    HIPCHK(c, hipGetLastError());
    return MO_OK;
}

// ---- growth: the F-RANSAC inliers of one keyframe pair, in query order, onto the end of the map (local_mapper.py:150-187) --------
// One block of 1024 threads walks the query keypoints in tiles (ballot + block scan); the map's live counts come from the status block.
// midx: MatchBufs::idx of the one pair, midx[2 * q] the best neighbour of query q (the layout is emit_match's, match_kernels.hip).
__global__ __launch_bounds__(1024) void k_map_append(const uint8_t* __restrict__ inl, const int32_t* __restrict__ midx, const float* __restrict__ gpts,
                                                     const double* __restrict__ F, const mo_keypoint* __restrict__ qkps, const int32_t* __restrict__ qcnt,
                                                     const uint8_t* __restrict__ img, int w, int h, int ch, int prev_id, int cur_id, int prev_ord,
                                                     int born, MapPts dst, int32_t* __restrict__ st) {
    __shared__ int lw[40];
    const int nq = *qcnt;
    const int n0 = st[ST_NPTS], o0 = st[ST_NOBS];
    const bool model = !isnan(F[8]);
    int added = 0;
    for (int b = 0; b < nq; b += 1024) {
        const int q = b + threadIdx.x;
        const int take = (model && q < nq && inl[q]) ? 1 : 0;
        int t;
        const int r = block_excl_scan(take, lw, &t);
        if (take) {
            const int i = n0 + added + r;
            const float* X = gpts + (size_t)q * 3;
            dst.xyz[(size_t)i * 3 + 0] = X[0]; dst.xyz[(size_t)i * 3 + 1] = X[1]; dst.xyz[(size_t)i * 3 + 2] = X[2];
            const mo_keypoint kp = qkps[q];
            const int x = (int)kp.x, y = (int)kp.y;   // Python's int(): truncation toward zero
            uint8_t c0 = 0, c1 = 0, c2 = 255;
            if (x >= 0 && x < w && y >= 0 && y < h) {
                const uint8_t* px = img + ((size_t)y * w + x) * ch;
                c0 = px[0]; c1 = ch == 3 ? px[1] : px[0]; c2 = ch == 3 ? px[2] : px[0];
            }
            dst.col[(size_t)i * 3 + 0] = c0; dst.col[(size_t)i * 3 + 1] = c1; dst.col[(size_t)i * 3 + 2] = c2;
            dst.id[i] = i;                             // len(self.map_points) at creation
            dst.dkf[i] = prev_ord; dst.drow[i] = q;      // (the ordinal: the slot, except on an imported map)
            map_life_new(dst, i, born);
            const int o = o0 + 2 * (added + r);
            dst.off[i] = o;
            dst.okf[o] = prev_id; dst.okp[o] = q;
            dst.okf[o + 1] = cur_id; dst.okp[o + 1] = midx[(size_t)q * 2];
        }
        added += t;
    }
    if (threadIdx.x == 0) {
        map_store_end(dst, st, n0 + added, o0 + 2 * added);
        st[ST_NNEW] = added;
    }
}

// ---- cull (local_mapper.py:207-240): one thread per point, observations in insertion order --------------------------------------
// (for `bound` points at most, the live count in st: mv.n_pts is the map before the growth step and is not read)
__global__ __launch_bounds__(256) void k_map_cull(MapView mv, int bound, const mo_keypoint* __restrict__ kkps, const double* __restrict__ kP, int min_obs,
                                                  int32_t* __restrict__ keep, int32_t* __restrict__ kobs, int32_t* __restrict__ st) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= bound) return;
    const MapPts& src = mv.src;
    const int n = st[ST_NPTS];
    int k = 0;
    int nob = 0;
    if (i < n) {
        const int o0 = src.off[i], o1 = src.off[i + 1];
        nob = o1 - o0;
        if (nob >= min_obs) {
            k = 1;
            const double X = src.xyz[(size_t)i * 3], Y = src.xyz[(size_t)i * 3 + 1], Z = src.xyz[(size_t)i * 3 + 2];
            for (int o = o0; o < o1; o++) {
                int pos, s, kp;
                const int bad = map_obs(mv, o, &pos, &s, &kp);
                if (bad) { atomicOr(st + ST_ERR, bad); k = 0; break; }   // bit 1: keyframe, bit 2: keypoint
                const double* P = kP + (size_t)s * 12;
                const double u = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(P[0], X), __dmul_rn(P[1], Y)), __dmul_rn(P[2], Z)), P[3]);
                const double v = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(P[4], X), __dmul_rn(P[5], Y)), __dmul_rn(P[6], Z)), P[7]);
                const double z = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(P[8], X), __dmul_rn(P[9], Y)), __dmul_rn(P[10], Z)), P[11]);
                const mo_keypoint kq = kkps[(size_t)s * mv.row + kp];
                const double du = u / z - (double)kq.x, dv = v / z - (double)kq.y;
                const double err = sqrt(__dadd_rn(__dmul_rn(du, du), __dmul_rn(dv, dv)));
                if (err > 5.0) { k = 0; break; }
            }
        }
    }
    keep[i] = k;
    kobs[i] = k ? nob : 0;
}

// survivors in order through map_point_move (map_rebuild.h); the entry rule also writes ent_id[entry] = id of the entry's point (the
// counting sort's values)
struct CompactEdit : RebuildEdit {
    int32_t* ent_id;
    __device__ int entries(const MapPts& src, int i, int o0, int o1, const MapPts& dst, int ob) const {
        const int id = src.id[i];
        return map_entries_copy(src, o0, o1, dst, ob, [&](int at) { ent_id[at] = id; });
    }
};

// The chain's own kernel and not k_map_rebuild for two things: it runs over `bound` points at most, the live count being on the device,
// and an index error (ST_ERR) holds the end of the store back - the host then keeps the map it had (finish_chain).  map_store_end
// also writes the live counts ST_NPTS / ST_NOBS here; behind a chain without an error finish_chain uploads the same two words again.
// The upload is redundant since and is kept on purpose in this change (no later kernel of the chain reads the two words; with an error
// neither is written and the counts in front of the cull stand); dropping it is a change of its own.
__global__ __launch_bounds__(256) void k_map_compact(MapPts src, MapPts dst, int bound, const int32_t* __restrict__ keep, const int32_t* __restrict__ rank,
                                                     const int32_t* __restrict__ obase, int32_t* __restrict__ ent_id, int32_t* __restrict__ st) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int err = st[ST_ERR], kept = st[ST_KEPT], kobs = st[ST_KOBS];
    if (i == 0 && !err) map_store_end(dst, st, kept, kobs);
    if (i >= bound || !keep[i]) return;
    map_point_move(CompactEdit{{}, ent_id}, src, i, dst, rank[i], obase[i]);
}

// ---- per-keyframe lists (local_mapper.py:243-251): stable counting sort of (keyframe, map order) ----------------------------------
// A keyframe's list holds the ids of the points whose observation keys contain its id (= its position: ids are renumbered to positions).
// Pass 1: per chunk of MAP_LIST_CHUNK entries, a histogram over keyframes, stored keyframe-major (hist[kf][chunk]) so that ONE exclusive
// scan of it gives every (keyframe, chunk) its first output row.  Pass 2: the chunk's one wave walks its entries in order, 64 at a time,
// each lane's rank among the earlier lanes with the same key from one ballot per distinct key: the output keeps map order inside a list.
__global__ __launch_bounds__(64) void k_list_hist(const int32_t* __restrict__ okf, const int32_t* __restrict__ st, int n_kf, int n_chunks,
                                                  int32_t* __restrict__ hist) {
    extern __shared__ int cnt[];
    for (int j = threadIdx.x; j < n_kf; j += 64) cnt[j] = 0;
    __syncthreads();
    const int n = st[ST_KOBS];
    const int e0 = blockIdx.x * MAP_LIST_CHUNK, e1 = min(e0 + MAP_LIST_CHUNK, n);
    for (int e = e0 + threadIdx.x; e < e1; e += 64) {
        const int k = okf[e];
        if (k >= 0 && k < n_kf) atomicAdd(cnt + k, 1);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n_kf; j += 64) hist[(size_t)j * n_chunks + blockIdx.x] = cnt[j];
}

__global__ __launch_bounds__(64) void k_list_scatter(const int32_t* __restrict__ okf, const int32_t* __restrict__ ent_id, const int32_t* __restrict__ st,
                                                     int n_kf, int n_chunks, const int32_t* __restrict__ hbase, int32_t* __restrict__ lids) {
    extern __shared__ int cur[];
    for (int j = threadIdx.x; j < n_kf; j += 64) cur[j] = hbase[(size_t)j * n_chunks + blockIdx.x];
    __syncthreads();
    const int n = st[ST_KOBS];
    const int e0 = blockIdx.x * MAP_LIST_CHUNK, e1 = min(e0 + MAP_LIST_CHUNK, n);
    const int lane = threadIdx.x;
    for (int b = e0; b < e1; b += 64) {
        const int e = b + lane;
        int k = e < e1 ? okf[e] : -1;
        if (k >= n_kf) k = -1;
        int before = 0, same = 0;
        // one ballot per distinct key of the 64 entries (a wave's entries are a run of the map: few keyframes each)
        uint64_t todo = __ballot(k >= 0);
        while (todo) {
            const int key = __shfl(k, __ffsll((unsigned long long)todo) - 1, 64);
            const uint64_t mk = __ballot(k == key);
            if (k == key) { before = __popcll(mk & ((1ull << lane) - 1)); same = __popcll(mk); }
            todo &= ~mk;
        }
        int base = 0;
        if (k >= 0) base = cur[k];
        __syncthreads();
        if (k >= 0) {
            lids[base + before] = ent_id[e];
            if (before == same - 1) cur[k] = base + same;   // the group's last lane moves the cursor
        }
        __syncthreads();
    }
}

__global__ void k_list_offsets(const int32_t* __restrict__ hbase, int n_kf, int n_chunks, const int32_t* __restrict__ st, int32_t* __restrict__ loff) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n_kf) loff[j] = hbase[(size_t)j * n_chunks];
    if (j == n_kf) loff[j] = st[ST_NLIST];
}

// ---- the counts _cull_keyframes reads (local_mapper.py:270-285): per listed id, the FIRST map point with that id, its observation
// keys other than the keyframe's own id; >= 3 makes the entry redundant.  first[id] = lowest map index with that id.
__global__ __launch_bounds__(256) void k_first_index(const int32_t* __restrict__ id, const int32_t* __restrict__ st, int bound, int id_bound,
                                                     int32_t* __restrict__ first) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= bound || i >= st[ST_KEPT]) return;
    const int v = id[i];
    if (v >= 0 && v < id_bound) atomicMin(first + v, i);
}

__global__ __launch_bounds__(256) void k_kf_redundant(const int32_t* __restrict__ loff, const int32_t* __restrict__ lids, int n_kf, int bound,
                                                      const int32_t* __restrict__ st, const int32_t* __restrict__ first, const int32_t* __restrict__ off,
                                                      const int32_t* __restrict__ okf, int32_t* __restrict__ red) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool hit = false;
    int lo = 0;
    if (e < bound && e < st[ST_NLIST]) {
        int hi = n_kf;   // keyframe j of entry e: loff[j] <= e < loff[j + 1]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (loff[mid] <= e) lo = mid; else hi = mid; }
        const int p = first[lids[e]];
        int other = 0;
        for (int o = off[p]; o < off[p + 1]; o++) other += okf[o] != lo;
        hit = other >= 3;
    }
    // one atomic per (wave, keyframe): the lists are sorted by keyframe, so a wave's hits mostly share one keyframe (Guideline 12)
    uint64_t todo = __ballot(hit);
    while (todo) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const int key = __shfl(lo, leader, 64);
        const uint64_t same = __ballot(hit && lo == key);
        if (lane == leader) atomicAdd(red + key, __popcll(same));
        todo &= ~same;
    }
}

// ---- point_of (map_store.h's map_point_of): one thread per point; relocalization over every position, growth over its window ----
__global__ __launch_bounds__(256) void k_point_of(MapView v, int lo_pos, int32_t* __restrict__ tab) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < v.n_pts) map_point_of(v, i, lo_pos, tab);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
int map_launch_point_of(mo_map* m, int lo_pos, int n_tab_kf, int32_t* tab) {
    mo_ctx* c = m->c;
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)tab, INT_MAX, (size_t)n_tab_kf * m->row, c->stream));
    if (m->n_pts > 0) hipLaunchKernelGGL(k_point_of, dim3((unsigned)((m->n_pts + 255) / 256)), dim3(256), 0, c->stream, map_view(m), lo_pos, tab);
    HIPCHK(c, hipGetLastError());
    return MO_OK;
}

int map_pts_reserve(mo_map* m, int which, size_t pcap, size_t ocap, bool keep) {
    mo_ctx* c = m->c;
    MapPtsStore& p = m->P[which];
    const size_t np = keep ? (size_t)m->n_pts : 0, no = keep ? (size_t)m->n_obs : 0;
    int rc;
    if (!p.xyz || pcap > p.pcap) {
        pcap = std::max(pcap, p.pcap + p.pcap / 2);
        if ((rc = p.xyz.regrow(c, pcap * 3, np * 3)) || (rc = p.col.regrow(c, pcap * 3, np * 3)) || (rc = p.id.regrow(c, pcap, np)) ||
            (rc = p.dkf.regrow(c, pcap, np)) || (rc = p.drow.regrow(c, pcap, np)) || (rc = p.off.regrow(c, pcap + 1, np + 1)) ||
            (rc = p.life.regrow(c, pcap, np)))
            return rc;
        p.pcap = pcap;
    }
    if (!p.okf || ocap > p.ocap) {
        ocap = std::max(ocap, p.ocap + p.ocap / 2);
        if ((rc = p.okf.regrow(c, ocap, no)) || (rc = p.okp.regrow(c, ocap, no))) return rc;
        p.ocap = ocap;
    }
    return MO_OK;
}

// kkps / kdesc / kcnt hold one slot more than kslots: the spare slot (index kslots) mo_map_relocalize stages its query in, so that
// one counts array serves both sides of its keyframe matching
int kf_reserve(mo_map* m, int rows, int slots) {
    mo_ctx* c = m->c;
    int rc;
    const size_t kept = (size_t)m->n_slots;
    if (rows > m->row) {  // a wider row: every keyframe is moved to the new stride
        const int nr = (int)(((size_t)rows + 15) & ~(size_t)15);
        const int ns = std::max(slots, m->kslots);
        {
            DevBuf<mo_keypoint> k2; DevBuf<uint8_t> d2;
            if ((rc = k2.regrow(c, (size_t)(ns + 1) * nr, 0)) || (rc = d2.regrow(c, (size_t)(ns + 1) * nr * 32, 0))) return rc;
            if (m->n_slots && m->row) {
                HIPCHK(c, hipMemcpy2DAsync(k2, (size_t)nr * sizeof(mo_keypoint), m->kkps, (size_t)m->row * sizeof(mo_keypoint), (size_t)m->row * sizeof(mo_keypoint),
                                           m->n_slots, hipMemcpyDeviceToDevice, c->stream));
                HIPCHK(c, hipMemcpy2DAsync(d2, (size_t)nr * 32, m->kdesc, (size_t)m->row * 32, (size_t)m->row * 32, m->n_slots, hipMemcpyDeviceToDevice, c->stream));
            }
            HIPCHK(c, hipStreamSynchronize(c->stream));
            m->kkps.swap(k2); m->kdesc.swap(d2); m->row = nr;   // (the old blocks are freed here, behind the synchronisation)
        }
        if (ns > m->kslots) {
            if ((rc = m->kcnt.regrow(c, (size_t)ns + 1, kept)) || (rc = m->kP.regrow(c, (size_t)ns * 12, kept * 12))) return rc;
            m->kslots = ns;
        }
    }
    if (slots > m->kslots) {
        const int ns = std::max(slots, m->kslots * 2);
        if ((rc = m->kkps.regrow(c, (size_t)(ns + 1) * m->row, kept * m->row)) || (rc = m->kdesc.regrow(c, (size_t)(ns + 1) * m->row * 32, kept * m->row * 32)) ||
            (rc = m->kcnt.regrow(c, (size_t)ns + 1, kept)) || (rc = m->kP.regrow(c, (size_t)ns * 12, kept * 12)))
            return rc;
        m->kslots = ns;
    }
    return MO_OK;
}

int upload_pos_slot(mo_map* m) {
    mo_ctx* c = m->c;
    int rc = m->d_pos_slot.reserve(c, std::max<size_t>(m->pos_slot.size(), 1));
    if (rc) return rc;
    if (!m->pos_slot.empty())
        HIPCHK(c, hipMemcpyAsync(m->d_pos_slot, m->pos_slot.data(), m->pos_slot.size() * 4, hipMemcpyHostToDevice, c->stream));
    return MO_OK;
}

int map_poison(mo_map* m) {
    mo_ctx* c = m->c;
    if (int rc = mo_poison_scratch(c, *m)) return rc;
    for (const auto& f : m->features)
        if (int rc = f->poison(c)) return rc;
    return MO_OK;
}

extern "C" mo_map* mo_map_create(mo_ctx* c, int kf_slots, int kf_rows, int64_t pts_cap, int64_t obs_cap) {
    if (!c) return nullptr;
    if (hipSetDevice(c->device) != hipSuccess) { mo_fail(c, MO_ERR_HIP, "hipSetDevice"); return nullptr; }
    mo_map* m = new mo_map();
    m->c = c;
    int rc = MO_OK;
    if (!rc) rc = kf_reserve(m, std::max(kf_rows, 16), std::max(kf_slots, 2));
    if (!rc) rc = map_pts_reserve(m, 0, (size_t)std::max<int64_t>(pts_cap, 16), (size_t)std::max<int64_t>(obs_cap, 32), false);
    if (!rc) rc = map_pts_reserve(m, 1, (size_t)std::max<int64_t>(pts_cap, 16), (size_t)std::max<int64_t>(obs_cap, 32), false);
    if (!rc) rc = m->st.reserve(c, ST_NWORDS);
    if (!rc) rc = m->h_stat.reserve(c, ST_NWORDS);
    if (!rc && hipMemsetAsync(m->st, 0, ST_NWORDS * sizeof(int32_t), c->stream) != hipSuccess) rc = mo_fail(c, MO_ERR_HIP, "hipMemset");
    if (!rc && hipMemsetAsync(m->P[0].off, 0, 4, c->stream) != hipSuccess) rc = mo_fail(c, MO_ERR_HIP, "hipMemset");
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = mo_fail(c, MO_ERR_HIP, "sync");
    if (rc) { mo_map_destroy(m); return nullptr; }
    return m;
}

extern "C" void mo_map_destroy(mo_map* m) {
    if (!m) return;
    hipSetDevice(m->c->device);
    hipStreamSynchronize(m->c->stream);
    delete m;   // every buffer frees itself (DevBuf, PinnedBuf, the features)
}

// the list / cull / counts chain on the map in P[cur] with `bound_pts` points at most (status block live); results into P[cur ^ 1]
static int run_cull_chain(mo_map* m, int64_t bound_pts, int64_t bound_obs) {
    mo_ctx* c = m->c;
    const int n_kf = (int)m->pos_slot.size();
    if (n_kf > MAP_MAX_KF) return mo_fail(c, MO_ERR_UNSUPPORTED, "more keyframes than the per-keyframe list sort holds (16384)");
    if (bound_pts > INT32_MAX / 2 || bound_obs > INT32_MAX / 2) return mo_fail(c, MO_ERR_CAPACITY, "map larger than int32 indexing");
    int rc;
    const int bp = (int)std::max<int64_t>(bound_pts, 1), bo = (int)std::max<int64_t>(bound_obs, 1);
    if ((rc = rebuild_reserve(m, (size_t)bp, (size_t)bo)) || (rc = m->ent_id.reserve(c, (size_t)bo))) return rc;
    if ((rc = upload_pos_slot(m))) return rc;
    const MapPts src = m->P[m->cur].view(), dst = m->P[m->cur ^ 1].view();
    const unsigned gp = (unsigned)((bp + 255) / 256);
    hipLaunchKernelGGL(k_map_cull, dim3(gp), dim3(256), 0, c->stream, map_view(m), bp, m->kkps, m->kP, 2, m->keep, m->kobs, m->st);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, m->keep, m->rank, bp, m->st + ST_KEPT))) return rc;
    if ((rc = map_scan_excl(m, m->kobs, m->obase, bp, m->st + ST_KOBS))) return rc;
    hipLaunchKernelGGL(k_map_compact, dim3(gp), dim3(256), 0, c->stream, src, dst, bp, m->keep, m->rank, m->obase, m->ent_id, m->st);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "map_cull");
    // lists
    const int n_chunks = (bo + MAP_LIST_CHUNK - 1) / MAP_LIST_CHUNK;
    const size_t hn = (size_t)std::max(n_kf, 1) * n_chunks;
    if (hn > (size_t)INT32_MAX) return mo_fail(c, MO_ERR_CAPACITY, "list histogram too large");
    if ((rc = mo_reserve(c, m->hist, hn, m->hbase, hn))) return rc;
    const int ln = m->lcur ^ 1;
    if ((rc = m->loff[ln].reserve(c, (size_t)n_kf + 1))) return rc;
    if ((rc = m->lids[ln].reserve(c, (size_t)bo))) return rc;
    if ((rc = m->kf_red.reserve(c, (size_t)std::max(n_kf, 1)))) return rc;
    if (n_kf > 0) {
        const size_t lds = (size_t)n_kf * 4;
        hipLaunchKernelGGL(k_list_hist, dim3(n_chunks), dim3(64), lds, c->stream, dst.okf, m->st, n_kf, n_chunks, m->hist);
        HIPCHK(c, hipGetLastError());
        if ((rc = map_scan_excl(m, m->hist, m->hbase, (int)hn, m->st + ST_NLIST))) return rc;
        hipLaunchKernelGGL(k_list_scatter, dim3(n_chunks), dim3(64), lds, c->stream, dst.okf, m->ent_id, m->st, n_kf, n_chunks, m->hbase, m->lids[ln]);
        HIPCHK(c, hipGetLastError());
    } else {
        HIPCHK(c, hipMemsetAsync(m->st + ST_NLIST, 0, 4, c->stream));
    }
    hipLaunchKernelGGL(k_list_offsets, dim3((n_kf + 1 + 255) / 256), dim3(256), 0, c->stream, m->hbase, n_kf, n_chunks, m->st, m->loff[ln]);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "map_lists");
    // keyframe counts
    const int64_t idb = std::max<int64_t>(m->id_bound, 1);
    if (idb > INT32_MAX / 4) return mo_fail(c, MO_ERR_CAPACITY, "map point ids too large for the first-point table");
    if ((rc = m->first.reserve(c, (size_t)idb))) return rc;
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)m->first, 0x7fffffff, (size_t)idb, c->stream));
    HIPCHK(c, hipMemsetAsync(m->kf_red, 0, (size_t)std::max(n_kf, 1) * 4, c->stream));
    hipLaunchKernelGGL(k_first_index, dim3(gp), dim3(256), 0, c->stream, dst.id, m->st, bp, (int)idb, m->first);
    if (n_kf > 0)
        hipLaunchKernelGGL(k_kf_redundant, dim3((unsigned)((bo + 255) / 256)), dim3(256), 0, c->stream, m->loff[ln], m->lids[ln], n_kf, bo, m->st, m->first,
                           dst.off, dst.okf, m->kf_red);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "map_kf_counts");
    return MO_OK;
}

// after the chain's synchronisation: commit the compacted map unless an index error was raised
static int finish_chain(mo_map* m, int n_kf, int32_t* kf_len, int32_t* kf_red) {
    mo_ctx* c = m->c;
    const int32_t* s = m->h_stat;
    if (s[ST_ERR]) {
        m->n_pts = s[ST_NPTS]; m->n_obs = s[ST_NOBS];
        return mo_fail(c, MO_ERR_INDEX, s[ST_ERR] & 1 ? "list index out of range (keyframe)" : "list index out of range (keypoint)");
    }
    map_commit(m, s[ST_KEPT], s[ST_KOBS]);
    m->list_rows = n_kf;
    m->lcur ^= 1;
    // the next call's live counts
    int32_t w[2] = {s[ST_KEPT], s[ST_KOBS]};
    HIPCHK(c, hipMemcpyAsync(m->st + ST_NPTS, w, 8, hipMemcpyHostToDevice, c->stream));
    if (kf_len || kf_red) {
        std::vector<int32_t> lo((size_t)n_kf + 1);
        HIPCHK(c, hipMemcpyAsync(lo.data(), m->loff[m->lcur], lo.size() * 4, hipMemcpyDeviceToHost, c->stream));
        if (kf_red && n_kf) HIPCHK(c, hipMemcpyAsync(kf_red, m->kf_red, (size_t)n_kf * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (kf_len) for (int j = 0; j < n_kf; j++) kf_len[j] = lo[j + 1] - lo[j];
    } else {
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return MO_OK;
}

extern "C" int mo_map_add_keyframe(mo_map* m, const mo_frame_ref* f, const double P[12], const uint8_t* img, int w, int h, int ch,
                                   const mo_map_kf_params* prm, mo_map_kf_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!f || !P || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (img && (w < 1 || h < 1 || (ch != 1 && ch != 3))) return mo_fail(c, MO_ERR_ARG, "image must be h x w x ch u8 with ch 1 or 3");
    MAP_ENTER(m);
    HostClock clk(c);
    int rc;
    out->n_new = 0; out->from_token = 0;
    for (int i = 0; i < 9; i++) out->F[i] = NAN;
    // the frame: the resident result slot named by its token, else the host arrays
    int rs, n;
    if ((rc = mo_frame_lookup(c, f, "keyframe", &rs, &n))) return rc;
    const int slot = m->n_slots;
    if ((rc = kf_reserve(m, std::max(n, 1), slot + 1))) return rc;
    mo_stage_begin(c);
    if ((rc = mo_frame_copy_rows(c, f, rs, n, m->kkps + (size_t)slot * m->row, m->kdesc + (size_t)slot * m->row * 32))) return rc;
    out->from_token = rs >= 0;
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)(m->kcnt + slot), n, 1, c->stream));
    HIPCHK(c, hipMemcpyAsync(m->kP + (size_t)slot * 12, P, 96, hipMemcpyHostToDevice, c->stream));
    m->h_kcnt.push_back(n);
    m->kserial.resize((size_t)slot + 1, 0); m->kserial[slot]++;
    m->n_slots = slot + 1;
    m->slot_ord.resize((size_t)slot + 1); m->slot_ord[slot] = (int32_t)m->kf_stored++;
    m->pos_slot.push_back(slot);
    const int n_kf = (int)m->pos_slot.size();
    // the image of this keyframe (the colours of the points the NEXT keyframe grows)
    const int ib = m->img_cur ^ 1;
    if (img) {
        if ((rc = m->img[ib].reserve(c, (size_t)w * h * ch))) return rc;
        HIPCHK(c, hipMemcpyAsync(m->img[ib], img, (size_t)w * h * ch, hipMemcpyHostToDevice, c->stream));
    }
    m->img_w[ib] = img ? w : 0; m->img_h[ib] = img ? h : 0; m->img_ch[ib] = img ? ch : 1;
    m->img_cur = ib;
    mo_stage_mark(c, "map_store");
    // growth: previous keyframe (query) against this one (train)
    int64_t bound_new = 0;
    c->flags_cur = mo_host_flags(c);
    HIPCHK(c, hipMemsetAsync(mo_host_flags(c), 0, 4 * sizeof(int), c->stream));
    const int ps = n_kf >= 2 ? m->pos_slot[n_kf - 2] : -1;
    const int nq = ps >= 0 ? m->h_kcnt[ps] : 0;
    if (ps >= 0 && nq > 0 && n > 0) {
        if (prm->n_hyp < 1) return mo_fail(c, MO_ERR_ARG, "n_hyp must be >= 1");
        const size_t rows = (size_t)m->row;
        if ((rc = mo_reserve(c, m->match, rows, m->inl, rows, m->gpts, rows * 3, m->F, 9, m->gnp, 1))) return rc;
        bound_new = nq;
        if ((rc = map_pts_reserve(m, m->cur, (size_t)(m->n_pts + bound_new), (size_t)(m->n_obs + 2 * bound_new), true))) return rc;
        if ((rc = upload_pos_slot(m))) return rc;
        const int32_t* qf = m->d_pos_slot + (n_kf - 2);
        const int32_t* tf = m->d_pos_slot + (n_kf - 1);
        if ((rc = match_launch_pairs(c, m->kdesc, m->kdesc, rows * 32, rows * 32, m->kcnt, qf, tf, 0, 0, 1, (int)rows, prm->ratio, m->match.idx,
                                     m->match.dist, m->match.pass)))
            return rc;
        mo_stage_mark(c, "match_knn2_ratio");
        TwoViewArgs a = tv_fundamental(1, (int)rows, prm->n_hyp, prm->thr_px, prm->seed, prm->pair_index);
        a.d_kps = m->kkps; a.d_counts = m->kcnt; a.d_match_idx = m->match.idx; a.d_match_pass = m->match.pass;
        a.d_qf = qf; a.d_tf = tf; a.need_two = 1; a.d_P1 = m->kP + (size_t)ps * 12; a.d_P2 = m->kP + (size_t)slot * 12;
        a.d_E = m->F; a.d_points = m->gpts; a.d_n_points = m->gnp; a.d_inlier = m->inl;
        if ((rc = twoview_launch(c, a))) return rc;
        mo_stage_mark(c, "keyframe_f_ransac_triangulate");
        const int pi = m->img_cur ^ 1;  // the previous keyframe's image
        if (!m->img[pi]) { m->img_w[pi] = m->img_h[pi] = 0; }
        hipLaunchKernelGGL(k_map_append, dim3(1), dim3(1024), 0, c->stream, m->inl, m->match.idx, m->gpts, m->F, m->kkps + (size_t)ps * rows, m->kcnt + ps,
                           m->img[pi] ? m->img[pi].p : m->kdesc.p, m->img_w[pi], m->img_h[pi], m->img_ch[pi], n_kf - 2, n_kf - 1, m->slot_ord[ps], map_now(m),
                           m->P[m->cur].view(), m->st);
        HIPCHK(c, hipGetLastError());
        mo_stage_mark(c, "map_append");
        m->id_bound = std::max<int64_t>(m->id_bound, m->n_pts + bound_new);
    }
    HIPCHK(c, hipMemsetAsync(m->st + ST_ERR, 0, 4, c->stream));
    const bool cull = n_kf >= 2;  // (local_mapper.py:75: the map is updated from the second keyframe on)
    if (cull && (rc = run_cull_chain(m, m->n_pts + bound_new, m->n_obs + 2 * bound_new))) return rc;
    HIPCHK(c, hipMemcpyAsync(m->h_stat, m->st, ST_NWORDS * 4, hipMemcpyDeviceToHost, c->stream));
    if (bound_new) {
        if (out->match_idx) HIPCHK(c, hipMemcpyAsync(out->match_idx, m->match.idx, (size_t)nq * 8, hipMemcpyDeviceToHost, c->stream));
        if (out->match_pass) HIPCHK(c, hipMemcpyAsync(out->match_pass, m->match.pass, (size_t)nq, hipMemcpyDeviceToHost, c->stream));
        if (out->inlier) HIPCHK(c, hipMemcpyAsync(out->inlier, m->inl, (size_t)nq, hipMemcpyDeviceToHost, c->stream));
        if (out->points) HIPCHK(c, hipMemcpyAsync(out->points, m->gpts, (size_t)nq * 12, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(out->F, m->F, 72, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = map_sync(c, clk))) return rc;
    out->n_new = m->h_stat[ST_NNEW] * (bound_new ? 1 : 0);
    HIPCHK(c, hipMemsetAsync(m->st + ST_NNEW, 0, 4, c->stream));
    if (cull && (rc = finish_chain(m, n_kf, out->kf_len, out->kf_redundant))) return rc;
    out->n_points = m->n_pts; out->n_obs = m->n_obs;
    return MO_OK;
}

extern "C" int mo_map_add_points(mo_map* m, int n, const float* xyz, const uint8_t* col, const int32_t* id, const int32_t* obs_off, const int32_t* obs_kf,
                                 const int32_t* obs_kp, const int32_t* dref_kf, const int32_t* dref_row) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (n < 0 || (n > 0 && (!xyz || !col || !id || !obs_off || !dref_kf || !dref_row))) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    if (n == 0) return MO_OK;
    MAP_ENTER(m);
    const int64_t no = obs_off[n] - obs_off[0];
    if (no < 0 || (no > 0 && (!obs_kf || !obs_kp))) return mo_fail(c, MO_ERR_ARG, "bad observation offsets");
    int rc = map_pts_reserve(m, m->cur, (size_t)(m->n_pts + n), (size_t)(m->n_obs + no), true);
    if (rc) return rc;
    const MapPts p = m->P[m->cur].view();
    const size_t b = (size_t)m->n_pts;
    HIPCHK(c, hipMemcpyAsync(p.xyz + b * 3, xyz, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p.col + b * 3, col, (size_t)n * 3, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p.id + b, id, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p.dkf + b, dref_kf, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p.drow + b, dref_row, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    std::vector<int32_t> off((size_t)n + 1);
    int64_t mx = m->id_bound;
    for (int i = 0; i <= n; i++) off[i] = (int32_t)(m->n_obs + obs_off[i] - obs_off[0]);
    for (int i = 0; i < n; i++) {
        if (id[i] < 0) return mo_fail(c, MO_ERR_ARG, "map point ids must be >= 0");
        mx = std::max<int64_t>(mx, (int64_t)id[i] + 1);
    }
    HIPCHK(c, hipMemcpyAsync(p.off + b, off.data(), off.size() * 4, hipMemcpyHostToDevice, c->stream));
    const std::vector<int4> life((size_t)n, make_int4(1, 1, map_now(m), 0));   // (new points: map_life_new's record)
    HIPCHK(c, hipMemcpyAsync(p.life + b, life.data(), (size_t)n * sizeof(int4), hipMemcpyHostToDevice, c->stream));
    if (no) {
        HIPCHK(c, hipMemcpyAsync(p.okf + m->n_obs, obs_kf + obs_off[0], (size_t)no * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(p.okp + m->n_obs, obs_kp + obs_off[0], (size_t)no * 4, hipMemcpyHostToDevice, c->stream));
    }
    m->n_pts += n; m->n_obs += no; m->id_bound = mx;
    int32_t w[2] = {(int32_t)m->n_pts, (int32_t)m->n_obs};
    HIPCHK(c, hipMemcpyAsync(m->st + ST_NPTS, w, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MO_OK;
}

extern "C" int mo_map_remove_keyframes(mo_map* m, const int32_t* positions, int n) {
    if (!m) return MO_ERR_ARG;
    if (n < 0 || (n > 0 && !positions)) return mo_fail(m->c, MO_ERR_ARG, "NULL argument");
    std::vector<int32_t> pos(positions, positions + n);
    std::sort(pos.begin(), pos.end());
    pos.erase(std::unique(pos.begin(), pos.end()), pos.end());
    for (int i = (int)pos.size() - 1; i >= 0; i--) {
        if (pos[i] < 0 || pos[i] >= (int)m->pos_slot.size()) return mo_fail(m->c, MO_ERR_ARG, "keyframe position out of range");
        m->pos_slot.erase(m->pos_slot.begin() + pos[i]);
    }
    return MO_OK;
}

extern "C" int mo_map_sizes(mo_map* m, int64_t out[6]) {
    if (!m || !out) return MO_ERR_ARG;
    out[0] = (int64_t)m->pos_slot.size(); out[1] = m->n_pts; out[2] = m->n_obs; out[3] = m->list_rows;
    out[4] = m->list_rows ? -1 : 0;  // list entries: read with MO_MAP_LIST_OFF
    out[5] = m->n_slots;
    return MO_OK;
}

extern "C" int mo_map_download(mo_map* m, int field, void* dst, size_t bytes) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!dst && bytes) return mo_fail(c, MO_ERR_ARG, "NULL destination");
    MAP_ENTER(m);
    const MapPts p = m->P[m->cur].view();
    const void* src = nullptr; size_t have = 0;
    switch (field) {
        case MO_MAP_XYZ: src = p.xyz; have = (size_t)m->n_pts * 12; break;
        case MO_MAP_COLOR: src = p.col; have = (size_t)m->n_pts * 3; break;
        case MO_MAP_ID: src = p.id; have = (size_t)m->n_pts * 4; break;
        case MO_MAP_DREF_KF: src = p.dkf; have = (size_t)m->n_pts * 4; break;
        case MO_MAP_DREF_ROW: src = p.drow; have = (size_t)m->n_pts * 4; break;
        case MO_MAP_OBS_OFF: src = p.off; have = ((size_t)m->n_pts + 1) * 4; break;
        case MO_MAP_OBS_KF: src = p.okf; have = (size_t)m->n_obs * 4; break;
        case MO_MAP_OBS_KP: src = p.okp; have = (size_t)m->n_obs * 4; break;
        case MO_MAP_LIST_OFF: src = m->loff[m->lcur]; have = m->list_rows ? ((size_t)m->list_rows + 1) * 4 : 0; break;
        case MO_MAP_LIST_IDS: {
            if (!m->list_rows) { have = 0; break; }
            int32_t tot = 0;
            HIPCHK(c, hipMemcpyAsync(&tot, m->loff[m->lcur] + m->list_rows, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            src = m->lids[m->lcur]; have = (size_t)tot * 4; break;
        }
        default: return mo_fail(c, MO_ERR_ARG, "unknown map field");
    }
    if (bytes != have) return mo_fail(c, MO_ERR_CAPACITY, "download size must equal the field's size (" + std::to_string(have) + " bytes)");
    if (have) HIPCHK(c, hipMemcpyAsync(dst, src, have, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MO_OK;
}
