// map_correct.hip -- the correction of a confirmed loop on the device map (mo_map_loop_correct in include/vslam_amd.h): the first half of
// ORB-SLAM2's LoopClosing::CorrectLoop.  The similarity mo_map_loop_confirm refined is carried to the asking keyframe's neighbourhood
// (one transform A of the map frame, formed on the host in f64), the neighbourhood's points and poses move, and the loop side's points
// replace and absorb the duplicates the neighbourhood holds (SearchAndFuse): confirm's loop_point rows directly, every other loop point
// by mo_map_fuse's search under the corrected projections.  Writes the fused map into the other copy of the store.
//
// Chain (one synchronisation, the copy-out; every kernel behind the resolve reads cr_any(res) first and returns when nothing fuses):
//   uploads, fills, k_trk_rep over the group's keyframes (trk_launch_rep_mask: the loop points and their representatives)
//   k_cr_move      one thread per point: point_of of every keyframe (map_point_of), valid observations, the moved flag, A (X, 1) written
//                  over xyz of the moved points in the live copy, union-find and survivor tables reset; threads below the corrected count
//                  write kP = K [R' | t' / s] of their keyframe
//   k_trk_grid     one block per corrected keyframe (trk_launch_grid)
//   k_cr_direct    one thread per row of p: the row's loop point against the row's owner: a merge edge, or the point's claim on the free
//                  row (atomicMin of the row per point: the lower row wins)
//   k_cr_search    one thread per (point, corrected keyframe): k_fuse_search with the targets read through the position table
//   k_cr_resolve   one thread per (corrected keyframe, row): the winner of a claimed row against the row's owner (a row k_cr_direct gave
//                  to a loop point is owned by it)
//   k_cr_flatten, map_scan_excl + k_cr_members, k_cr_count, map_scan_excl x 2 + k_cr_scatter   map_fuse.hip's merge stages
// The merge stages are a second copy of map_fuse.hip's, not shared functions: that file reads its targets as lo_pos + t and its gains from
// the search alone; here the targets go through a position table, a component's key has the loop bit and a member may hold a direct gain.
// map_fuse.hip's device text stays the parent's (profiles/correct_isa.txt); NOTES.md says more.
// Integer atomics only: equal inputs give equal bytes.  -ffp-contract=off (Makefile): tests/correct_restatement.py rounds as this file does.
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"
#include "map_store.h"
#include "map_search.h"
#include "ba.h"    // ba_info
#include "pnp.h"   // pnp_projection

#define CR_BLOCK 256
#define FU_MAX_TARGETS 16384   // map_fuse.hip's bound on grid.y of the search

struct CrPrm {
    double K[9], A[12];
    double radius, sf, chi2;
    int32_t w, h, max_dist, p, n_p, nt;
};

struct CrRes {
    int32_t n_loop_points, n_moved, n_direct_edges, n_direct_gained, n_pairs, n_cand, n_proposals, n_gained, n_edges, n_absorbed;
    int32_t n_points, n_obs, n_members;
};

struct CorrectBufs : MapFeature {
    DevBuf<uint8_t> cmask, gmask;         // [n_kf] the corrected keyframes, the group
    DevBuf<int32_t> cpos, slots;          // [target] position (ascending) and slot of every corrected keyframe
    DevBuf<double> pose;                  // [target][12] the corrected [R' | t' / s]
    DevBuf<int32_t> lp;                   // [rows of p] loop_point
    DevBuf<uint8_t> rep;                  // [point][32] representative descriptors
    DevBuf<int32_t> oct;                  // [point] ref_octave (TK_NOT_LOCAL: no loop point)
    DevBuf<int32_t> cell, sorted;         // [target][TK_CELLS + 1], [target][row]: the keypoint grids
    DevBuf<int32_t> tab;                  // [position][row] point_of (INT_MAX: a free row)
    DevBuf<int32_t> drow;                 // [point] the row of p rule 4 gives the point (INT_MAX: none)
    DevBuf<unsigned long long> key;       // [target][row] (dist << 32) | point of the claim on each keypoint
    DevBuf<int32_t> prop;                 // [target][point] the row each pair proposed (-1: none)
    DevBuf<int32_t> parent, root, nval;   // [point] union-find, flattened root, valid observations
    DevBuf<unsigned long long> surv;      // [point] at a root: the survivor's key
    DevBuf<int32_t> mcnt, mbase, mcur, mem;   // [point] members per root, their first entry, scatter cursors, the member lists
    DevBuf<int32_t> into;                 // [point] new index of the point each old point now is
    DevBuf<uint8_t> moved;                // [point]
    ResBlock<CrRes> res;
    // all of it is scratch: every call's chain writes what it reads
    template <class F> void each_scratch(F f) {
        f(cmask); f(gmask); f(cpos); f(slots); f(pose); f(lp); f(rep); f(oct); f(cell); f(sorted); f(tab); f(drow); f(key); f(prop); f(parent); f(root);
        f(nval); f(surv); f(mcnt); f(mbase); f(mcur); f(mem); f(into); f(moved); f(res);
    }
    int poison(mo_ctx* c) override { return mo_poison_scratch(c, *this); }
};

// what the kernels read (by value): the map, and the call's own tables
struct CrView {
    MapView map;
    const int32_t* cpos; const int32_t* lp; const int32_t* drow;
    const int32_t* prop; const unsigned long long* key; const int32_t* tab;
    int p, n_p, nt;
};

__device__ __forceinline__ bool cr_any(const CrRes* res) { return res->n_proposals || res->n_direct_edges || res->n_direct_gained; }

// the owner of row r of the keyframe at position pos: point_of, else the loop point rule 4 gave the row to, else INT_MAX
__device__ __forceinline__ int cr_owner(const CrView& v, int pos, int r) {
    const int o = v.tab[(size_t)pos * v.map.row + r];
    if (o != INT_MAX || pos != v.p) return o;
    const int L = v.lp[r];
    return L >= 0 && L < v.map.n_pts && v.drow[L] == r ? L : INT_MAX;
}

// one thread per point: point_of, valid observations, the move, the tables of the later kernels reset; kP of the corrected keyframes
__global__ __launch_bounds__(CR_BLOCK) void k_cr_move(MapView v, CrPrm prm, const uint8_t* __restrict__ cmask, const uint8_t* __restrict__ gmask,
                                                       const int32_t* __restrict__ slots, const double* __restrict__ pose, double* __restrict__ kP,
                                                       int32_t* __restrict__ tab, int32_t* __restrict__ nval, int32_t* __restrict__ parent,
                                                       int32_t* __restrict__ mcnt, int32_t* __restrict__ mcur, unsigned long long* __restrict__ surv,
                                                       int32_t* __restrict__ drow, uint8_t* __restrict__ moved, CrRes* __restrict__ res) {
    const int i = blockIdx.x * CR_BLOCK + threadIdx.x;
    if (i < prm.nt) {
        double R[9], t[3], P[12];
        pose_split(pose + (size_t)i * 12, R, t);
        pnp_projection(prm.K, R, t, P);
        for (int k = 0; k < 12; k++) kP[(size_t)slots[i] * 12 + k] = P[k];
    }
    bool mv = false;
    if (i < v.n_pts) {
        nval[i] = map_point_of(v, i, 0, tab); parent[i] = i; mcnt[i] = 0; mcur[i] = 0; surv[i] = TK_NONE; drow[i] = INT_MAX;
        bool at_c = false, at_g = false;
        map_each_obs(v, i, [&](int, int pos, int, int) { at_c |= cmask[pos] != 0; at_g |= gmask[pos] != 0; return false; });
        mv = at_c && !at_g;
        moved[i] = mv;
        if (mv) {
            float* x = v.src.xyz + (size_t)i * 3;
            const double x0 = (double)x[0], x1 = (double)x[1], x2 = (double)x[2];
            for (int d = 0; d < 3; d++) x[d] = (float)(prm.A[d * 4] * x0 + prm.A[d * 4 + 1] * x1 + prm.A[d * 4 + 2] * x2 + prm.A[d * 4 + 3]);
        }
    }
    wave_count_add(mv, &res->n_moved);
}

__device__ __forceinline__ int cr_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// map_fuse.hip's lock-free union: the larger root under the smaller; the root of a finished component is its lowest index
__device__ __forceinline__ void cr_unite(int32_t* parent, int a, int b) {
    for (;;) {
        for (int p; (p = cr_load(parent + a)) != a;) a = p;
        for (int p; (p = cr_load(parent + b)) != b;) b = p;
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(parent + hi, hi, lo) == hi) return;
    }
}

// one thread per row of p: its loop point against the row's owner
__global__ __launch_bounds__(CR_BLOCK) void k_cr_direct(MapView v, int p, int n_p, const int32_t* __restrict__ lp, const int32_t* __restrict__ tab,
                                                         int32_t* __restrict__ parent, int32_t* __restrict__ drow, CrRes* __restrict__ res) {
    const int r = blockIdx.x * CR_BLOCK + threadIdx.x;
    bool edge = false, first = false;
    if (r < n_p) {
        const int L = lp[r];
        if (L >= 0 && L < v.n_pts) {
            const int o = tab[(size_t)p * v.row + r];
            if (o != INT_MAX) {
                edge = o != L;
                if (edge) cr_unite(parent, o, L);
            } else if (!map_observes(v, L, p)) {
                first = atomicMin(drow + L, r) == INT_MAX;   // (one first claim per point, whichever row makes it)
            }
        }
    }
    wave_count_add(edge, &res->n_direct_edges);
    wave_count_add(first, &res->n_direct_gained);
}

// one thread per (point, corrected keyframe): k_fuse_search, the target's position from the table
__global__ __launch_bounds__(CR_BLOCK) void k_cr_search(CrPrm prm, CrView v, const mo_keypoint* __restrict__ kkps, const uint8_t* __restrict__ kdesc,
                                                         const double* __restrict__ kP, const uint8_t* __restrict__ rep, const int32_t* __restrict__ oct,
                                                         const int32_t* __restrict__ cell, const int32_t* __restrict__ sorted,
                                                         unsigned long long* __restrict__ key, int32_t* __restrict__ prop, CrRes* __restrict__ res) {
    const int t = blockIdx.y, i = blockIdx.x * CR_BLOCK + threadIdx.x;
    const MapView& mv = v.map;
    const int pos = v.cpos[t], slot = mv.pos_slot[pos];
    const int ro = i < mv.n_pts ? oct[i] : TK_NOT_LOCAL;
    const bool pair = ro != TK_NOT_LOCAL && !map_observes(mv, i, pos);
    double uu = 0.0, vv = 0.0;
    const bool cand = pair && trk_project(kP + (size_t)slot * 12, mv.src.xyz[(size_t)i * 3], mv.src.xyz[(size_t)i * 3 + 1], mv.src.xyz[(size_t)i * 3 + 2],
                                          prm.w, prm.h, &uu, &vv);
    int bd = INT_MAX, bq = INT_MAX;
    if (cand) {
        const uint8_t* __restrict__ fdesc = kdesc + (size_t)slot * mv.row * 32;
        const uint8_t* d = rep + (size_t)i * 32;
        trk_window(uu, vv, prm.radius * trk_scale(prm.sf, ro), ro, prm.w, prm.h, cell + (size_t)t * (TK_CELLS + 1), sorted + (size_t)t * mv.row,
                   kkps + (size_t)slot * mv.row, [&](int q, const mo_keypoint& kp, double dx, double dy) {
                       if (!(ba_info(prm.sf, kp.octave) * (dx * dx + dy * dy) <= prm.chi2)) return;
                       trk_take(trk_ham(d, fdesc + (size_t)q * 32), q, bd, bq);
                   });
    }
    const bool acc = bd != INT_MAX && bd <= prm.max_dist;
    if (acc) atomicMin(key + (size_t)t * mv.row + bq, ((unsigned long long)(unsigned)bd << 32) | (unsigned)i);
    if (i < mv.n_pts) prop[(size_t)t * mv.n_pts + i] = acc ? bq : -1;
    wave_count_add(pair, &res->n_pairs);
    wave_count_add(cand, &res->n_cand);
    wave_count_add(acc, &res->n_proposals);
}

// one thread per (corrected keyframe, row): the row's winner against its owner
__global__ __launch_bounds__(CR_BLOCK) void k_cr_resolve(CrView v, const int32_t* __restrict__ slots, int32_t* __restrict__ parent, CrRes* __restrict__ res) {
    if (!res->n_proposals) return;
    const int t = blockIdx.y, r = blockIdx.x * CR_BLOCK + threadIdx.x;
    bool gain = false, edge = false;
    if (r < v.map.row && r < v.map.kcnt[slots[t]]) {
        const unsigned long long k = v.key[(size_t)t * v.map.row + r];
        if (k != TK_NONE) {
            const int owner = cr_owner(v, v.cpos[t], r);
            gain = owner == INT_MAX;
            edge = !gain;
            if (edge) cr_unite(parent, (int)(k & 0xffffffffu), owner);
        }
    }
    wave_count_add(gain, &res->n_gained);
    wave_count_add(edge, &res->n_edges);
}

// k_fuse_flatten with one more leading bit in the survivor's key: a loop point first, then the most observations, then the lowest index
__global__ __launch_bounds__(CR_BLOCK) void k_cr_flatten(int n_pts, const int32_t* __restrict__ parent, const int32_t* __restrict__ nval,
                                                          const int32_t* __restrict__ oct, int32_t* __restrict__ root, int32_t* __restrict__ mcnt,
                                                          unsigned long long* __restrict__ surv, const CrRes* __restrict__ res) {
    if (!cr_any(res)) return;
    const int i = blockIdx.x * CR_BLOCK + threadIdx.x;
    if (i >= n_pts) return;
    int r = i;
    for (int p; (p = parent[r]) != r;) r = p;
    root[i] = r;
    atomicAdd(mcnt + r, 1);
    const unsigned long long other = oct[i] == TK_NOT_LOCAL ? 1ull : 0ull;
    atomicMin(surv + r, (other << 63) | ((unsigned long long)(0x7fffffffu - (unsigned)nval[i]) << 32) | (unsigned)i);
}

__global__ __launch_bounds__(CR_BLOCK) void k_cr_members(int n_pts, const int32_t* __restrict__ root, const int32_t* __restrict__ mbase,
                                                          int32_t* __restrict__ mcur, int32_t* __restrict__ mem, const CrRes* __restrict__ res) {
    if (!cr_any(res)) return;
    const int i = blockIdx.x * CR_BLOCK + threadIdx.x;
    if (i >= n_pts) return;
    const int r = root[i];
    mem[mbase[r] + atomicAdd(mcur + r, 1)] = i;   // (arrival order: the survivor sorts its run)
}

// the gained observation of point j at target t by the search: the row it proposed, won, and that nothing owns
__device__ __forceinline__ bool cr_gained(const CrView& v, int j, int t, int* r) {
    const int pr = v.prop[(size_t)t * v.map.n_pts + j];
    if (pr < 0) return false;
    if ((int)(v.key[(size_t)t * v.map.row + pr] & 0xffffffffu) != j || cr_owner(v, v.cpos[t], pr) != INT_MAX) return false;
    *r = pr;
    return true;
}

// map_fuse.hip's fuse_walk: (0) the survivor's own valid entries, (1) those of the other members, (2) the gains of all members by member:
// the direct gain first, then the search's by position.  f(index, kind, position, row) -> true stops the walk.
template <class F> __device__ __forceinline__ void cr_walk(const CrView& v, int s, const int32_t* __restrict__ mem, int nm, F f) {
    int idx = 0, kp;
    bool stop = false;
    map_each_obs(v.map, s, [&](int, int pos, int, int r) { return stop = f(idx++, 0, pos, r); });
    for (int a = 0; a < nm && !stop; a++)
        if (mem[a] != s) map_each_obs(v.map, mem[a], [&](int, int pos, int, int r) { return stop = f(idx++, 1, pos, r); });
    for (int a = 0; a < nm && !stop; a++) {
        const int dr = v.drow[mem[a]];
        if (dr != INT_MAX && f(idx++, 2, v.p, dr)) return;
        for (int t = 0; t < v.nt; t++)
            if (cr_gained(v, mem[a], t, &kp) && f(idx++, 2, v.cpos[t], kp)) return;
    }
}

// map_fuse.hip's fuse_merge: an entry of kinds 1 and 2 is kept when no earlier candidate stands at its position
template <class E> __device__ __forceinline__ int cr_merge(const CrView& v, int s, const int32_t* __restrict__ mem, int nm, E emit) {
    int n = 0;
    cr_walk(v, s, mem, nm, [&](int idx, int kind, int pos, int kp) {
        if (kind == 0) return false;
        bool held = false;
        cr_walk(v, s, mem, nm, [&](int idx2, int, int pos2, int) {
            if (idx2 >= idx) return true;
            held = pos2 == pos;
            return held;
        });
        if (!held) { emit(pos, kp); n++; }
        return false;
    });
    return n;
}

// one thread per point: keep = it is its component's survivor; a survivor sorts its members and counts its merged list
__global__ __launch_bounds__(CR_BLOCK) void k_cr_count(CrView v, const int32_t* __restrict__ root, const unsigned long long* __restrict__ surv,
                                                        const int32_t* __restrict__ mcnt, const int32_t* __restrict__ mbase, int32_t* __restrict__ mem,
                                                        int32_t* __restrict__ keep, int32_t* __restrict__ cnt, CrRes* __restrict__ res) {
    if (!cr_any(res)) return;
    const int i = blockIdx.x * CR_BLOCK + threadIdx.x;
    bool gone = false;
    if (i < v.map.n_pts) {
        const int r = root[i];
        const bool k = (int)(surv[r] & 0xffffffffu) == i;
        gone = !k;
        int n = 0;
        if (k) {
            int32_t* run = mem + mbase[r];
            const int nm = mcnt[r];
            sort_run(run, nm);
            n = v.map.src.off[i + 1] - v.map.src.off[i] + cr_merge(v, i, run, nm, [](int, int) {});
        }
        keep[i] = k; cnt[i] = n;
    }
    wave_count_add(gone, &res->n_absorbed);
}

// every field of every survivor to its new index, its own entries as stored, the merged entries behind them
__global__ __launch_bounds__(CR_BLOCK) void k_cr_scatter(CrView v, MapPts dst, const int32_t* __restrict__ root, const unsigned long long* __restrict__ surv,
                                                          const int32_t* __restrict__ mcnt, const int32_t* __restrict__ mbase, const int32_t* __restrict__ mem,
                                                          const int32_t* __restrict__ keep, const int32_t* __restrict__ rank, const int32_t* __restrict__ obase,
                                                          int32_t* __restrict__ into, int32_t* __restrict__ st, const CrRes* __restrict__ res) {
    if (!cr_any(res)) return;
    const int i = blockIdx.x * CR_BLOCK + threadIdx.x;
    if (i == 0) { dst.off[res->n_points] = res->n_obs; st[ST_NPTS] = res->n_points; st[ST_NOBS] = res->n_obs; }   // (the next call's live counts)
    if (i >= v.map.n_pts) return;
    const int rt = root[i];
    into[i] = rank[(int)(surv[rt] & 0xffffffffu)];
    if (!keep[i]) return;
    const MapPts& src = v.map.src;
    const int r = rank[i], ob = obase[i];
    map_point_copy(src, i, dst, r);
    if (mcnt[rt] > 1) map_life_merge(src, i, mem + mbase[rt], mcnt[rt], dst, r);
    dst.off[r] = ob;
    const int o0 = src.off[i], o1 = src.off[i + 1];
    for (int o = o0; o < o1; o++) { dst.okf[ob + o - o0] = src.okf[o]; dst.okp[ob + o - o0] = src.okp[o]; }
    int at = ob + o1 - o0;
    cr_merge(v, i, mem + mbase[rt], mcnt[rt], [&](int pos, int kp) { dst.okf[at] = pos; dst.okp[at] = kp; at++; });
}

extern "C" int mo_map_loop_correct(mo_map* m, const double K[9], const double* poses, const mo_map_correct_params* prm, mo_map_correct_out* out) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!K || !prm || !out) return mo_fail(c, MO_ERR_ARG, "NULL argument");
    const int n_kf = (int)m->pos_slot.size();
    if (n_kf > 0 && !poses) return mo_fail(c, MO_ERR_ARG, "poses is NULL");
    if (prm->w <= 0 || prm->h <= 0) return mo_fail(c, MO_ERR_ARG, "w and h must be > 0");
    if (!(prm->scale > 0.0) || !std::isfinite(prm->scale)) return mo_fail(c, MO_ERR_ARG, "scale must be finite and > 0");
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(prm->R[i]) || !std::isfinite(K[i])) return mo_fail(c, MO_ERR_ARG, "R and K must be finite");
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(prm->t[i])) return mo_fail(c, MO_ERR_ARG, "t must be finite");
    if (!(prm->radius >= 0.0) || !std::isfinite(prm->radius)) return mo_fail(c, MO_ERR_ARG, "radius must be finite and >= 0");
    if (!(prm->scale_factor > 0.0) || !std::isfinite(prm->scale_factor)) return mo_fail(c, MO_ERR_ARG, "scale_factor must be finite and > 0");
    if (!(prm->chi2 >= 0.0)) return mo_fail(c, MO_ERR_ARG, "chi2 must be >= 0");
    for (size_t i = 0; i < (size_t)n_kf * 12; i++)
        if (!std::isfinite(poses[i])) return mo_fail(c, MO_ERR_ARG, "poses must be finite");
    out->n_corrected = out->n_moved = out->n_loop_points = out->n_direct_edges = out->n_direct_gained = out->n_pairs = out->n_cand = 0;
    out->n_proposals = out->n_gained = out->n_edges = out->n_absorbed = 0;
    out->n_points = m->n_pts; out->n_obs = m->n_obs;
    for (int i = 0; i < 12; i++) out->A[i] = i % 5 == 0 ? 1.0 : 0.0;
    out->A_scale = 1.0;
    if (out->into) for (int64_t i = 0; i < m->n_pts; i++) out->into[i] = (int32_t)i;
    if (out->moved && m->n_pts) std::memset(out->moved, 0, (size_t)m->n_pts);
    if (out->poses_out && n_kf) std::memcpy(out->poses_out, poses, (size_t)n_kf * 96);
    if (n_kf == 0 || m->n_pts == 0) return MO_OK;   // (nothing to correct: not an error)
    const int p = prm->kf_pos, q = prm->cand_pos;
    if (p < 0 || p >= n_kf || q < 0 || q >= n_kf) return mo_fail(c, MO_ERR_ARG, "kf_pos and cand_pos must be keyframe positions");
    if (!prm->corrected || !prm->corrected[p]) return mo_fail(c, MO_ERR_ARG, "corrected must hold kf_pos");
    std::vector<uint8_t> cmask((size_t)n_kf), gmask((size_t)n_kf, 0);
    std::vector<int32_t> cpos, slots;
    size_t rows_sum = 0;
    for (int k = 0; k < n_kf; k++) {
        cmask[k] = prm->corrected[k] != 0;
        if (prm->group) gmask[k] = prm->group[k] != 0;
        if (cmask[k] && gmask[k]) return mo_fail(c, MO_ERR_ARG, "a position is both corrected and of the group");
        if (cmask[k]) { cpos.push_back(k); slots.push_back(m->pos_slot[k]); rows_sum += (size_t)m->h_kcnt[m->pos_slot[k]]; }
    }
    const int nt = (int)cpos.size(), row = m->row, n_p = m->h_kcnt[m->pos_slot[p]];
    if (nt > FU_MAX_TARGETS) return mo_fail(c, MO_ERR_UNSUPPORTED, "more corrected keyframes than one call searches (16384)");
    // rule 1: A = S_cw'^-1 T_p with S_cw' = S_pc T_cand, f64, each row summed left to right
    const double s = prm->scale, *R = prm->R, *t = prm->t;
    double Rp[9], tp[3], Rc[9], tc[3], Rq[9], tq[3], d[3], RA[9], tA[3];
    pose_split(poses + (size_t)p * 12, Rp, tp);
    pose_split(poses + (size_t)q * 12, Rc, tc);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Rq[i * 3 + j] = R[i * 3] * Rc[j] + R[i * 3 + 1] * Rc[3 + j] + R[i * 3 + 2] * Rc[6 + j];
        const double u = R[i * 3] * tc[0] + R[i * 3 + 1] * tc[1] + R[i * 3 + 2] * tc[2];
        tq[i] = s * u + t[i];
        d[i] = tp[i] - tq[i];
    }
    const double inv = 1.0 / s;
    CrPrm g;
    std::memset(&g, 0, sizeof(g));
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            RA[i * 3 + j] = Rq[i] * Rp[j] + Rq[3 + i] * Rp[3 + j] + Rq[6 + i] * Rp[6 + j];
            g.A[i * 4 + j] = inv * RA[i * 3 + j];
        }
        tA[i] = Rq[i] * d[0] + Rq[3 + i] * d[1] + Rq[6 + i] * d[2];
        g.A[i * 4 + 3] = inv * tA[i];
    }
    // rule 2: S_iw' = T_i A^-1 = [s R_i RA^T | t_i - R_i RA^T tA]; the pose is [R_i RA^T | (t_i - R_i RA^T tA) / s]
    std::vector<double> pose((size_t)nt * 12);
    for (int e = 0; e < nt; e++) {
        double Ri[9], ti[3];
        pose_split(poses + (size_t)cpos[e] * 12, Ri, ti);
        double* o = pose.data() + (size_t)e * 12;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) o[i * 4 + j] = Ri[i * 3] * RA[j * 3] + Ri[i * 3 + 1] * RA[j * 3 + 1] + Ri[i * 3 + 2] * RA[j * 3 + 2];
            const double v = o[i * 4] * tA[0] + o[i * 4 + 1] * tA[1] + o[i * 4 + 2] * tA[2];
            o[i * 4 + 3] = (ti[i] - v) / s;
        }
    }
    MAP_ENTER(m);
    HostClock clk(c);
    const size_t np = (size_t)m->n_pts, trow = (size_t)nt * row, krow = (size_t)n_kf * row;
    const size_t gain_bound = rows_sum + (size_t)n_p;
    if (m->n_pts > INT32_MAX / 2 || (size_t)m->n_obs + gain_bound > (size_t)(INT32_MAX / 2) || np * (size_t)nt > (size_t)INT32_MAX ||
        krow > (size_t)INT32_MAX)
        return mo_fail(c, MO_ERR_CAPACITY, "map larger than int32 indexing");
    CorrectBufs& b = map_feature<CorrectBufs>(m);
    int rc;
    const size_t np1 = std::max(n_p, 1);
    if ((rc = mo_reserve(c, b.cmask, (size_t)n_kf, b.gmask, (size_t)n_kf, b.cpos, (size_t)nt, b.slots, (size_t)nt, b.pose, (size_t)nt * 12, b.lp, np1, b.rep,
                         np * 32, b.oct, np, b.cell, (size_t)nt * (TK_CELLS + 1), b.sorted, trow, b.tab, krow, b.drow, np, b.key, trow, b.prop, np * nt,
                         b.parent, np, b.root, np, b.nval, np, b.surv, np, b.mcnt, np, b.mbase, np, b.mcur, np, b.mem, np, b.into, np, b.moved, np, b.res,
                         m->keep, np, m->kobs, np, m->rank, np, m->obase, np)))
        return rc;
    if ((rc = map_pts_reserve(m, m->cur ^ 1, np, (size_t)m->n_obs + gain_bound, false)) || (rc = upload_pos_slot(m))) return rc;
    mo_stage_begin(c);
    HIPCHK(c, hipMemsetAsync(b.res, 0, sizeof(CrRes), c->stream));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)b.tab.p, INT_MAX, krow, c->stream));
    HIPCHK(c, hipMemsetAsync(b.key, 0xff, trow * 8, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.cmask, cmask.data(), (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.gmask, gmask.data(), (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.cpos, cpos.data(), (size_t)nt * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.slots, slots.data(), (size_t)nt * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.pose, pose.data(), (size_t)nt * 96, hipMemcpyHostToDevice, c->stream));
    if (prm->loop_point && n_p) HIPCHK(c, hipMemcpyAsync(b.lp, prm->loop_point, (size_t)n_p * 4, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(b.lp, 0xff, np1 * 4, c->stream));
    for (int i = 0; i < 9; i++) g.K[i] = K[i];
    g.radius = prm->radius; g.sf = prm->scale_factor; g.chi2 = prm->chi2;
    g.w = prm->w; g.h = prm->h; g.max_dist = prm->max_dist; g.p = p; g.n_p = n_p; g.nt = nt;
    const MapPts dst = m->P[m->cur ^ 1].view();
    const MapView mv = map_view(m);
    const CrView v{mv, b.cpos, b.lp, b.drow, b.prop, b.key, b.tab, p, n_p, nt};
    const unsigned pblocks = (unsigned)((std::max(np, (size_t)nt) + CR_BLOCK - 1) / CR_BLOCK);
    if ((rc = trk_launch_rep_mask(m, b.gmask, b.rep, b.oct, &b.res.p->n_loop_points))) return rc;
    hipLaunchKernelGGL(k_cr_move, dim3(pblocks), dim3(CR_BLOCK), 0, c->stream, mv, g, b.cmask, b.gmask, b.slots, b.pose, m->kP, b.tab, b.nval, b.parent, b.mcnt,
                       b.mcur, b.surv, b.drow, b.moved, b.res);
    HIPCHK(c, hipGetLastError());
    if ((rc = trk_launch_grid(m, b.slots, 0, nt, prm->w, prm->h, b.cell, b.sorted))) return rc;
    mo_stage_mark(c, "correct_move");
    hipLaunchKernelGGL(k_cr_direct, dim3((unsigned)((np1 + CR_BLOCK - 1) / CR_BLOCK)), dim3(CR_BLOCK), 0, c->stream, mv, p, n_p, b.lp, b.tab, b.parent, b.drow,
                       b.res);
    hipLaunchKernelGGL(k_cr_search, dim3(pblocks, (unsigned)nt), dim3(CR_BLOCK), 0, c->stream, g, v, m->kkps, m->kdesc, m->kP, b.rep, b.oct, b.cell, b.sorted,
                       b.key, b.prop, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "correct_search");
    hipLaunchKernelGGL(k_cr_resolve, dim3((unsigned)((row + CR_BLOCK - 1) / CR_BLOCK), (unsigned)nt), dim3(CR_BLOCK), 0, c->stream, v, b.slots, b.parent, b.res);
    hipLaunchKernelGGL(k_cr_flatten, dim3(pblocks), dim3(CR_BLOCK), 0, c->stream, (int)np, b.parent, b.nval, b.oct, b.root, b.mcnt, b.surv, b.res);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, b.mcnt, b.mbase, (int)np, &b.res.p->n_members))) return rc;
    hipLaunchKernelGGL(k_cr_members, dim3(pblocks), dim3(CR_BLOCK), 0, c->stream, (int)np, b.root, b.mbase, b.mcur, b.mem, b.res);
    hipLaunchKernelGGL(k_cr_count, dim3(pblocks), dim3(CR_BLOCK), 0, c->stream, v, b.root, b.surv, b.mcnt, b.mbase, b.mem, m->keep, m->kobs, b.res);
    HIPCHK(c, hipGetLastError());
    if ((rc = map_scan_excl(m, m->keep, m->rank, (int)np, &b.res.p->n_points)) || (rc = map_scan_excl(m, m->kobs, m->obase, (int)np, &b.res.p->n_obs))) return rc;
    hipLaunchKernelGGL(k_cr_scatter, dim3(pblocks), dim3(CR_BLOCK), 0, c->stream, v, dst, b.root, b.surv, b.mcnt, b.mbase, b.mem, m->keep, m->rank, m->obase,
                       b.into, m->st, b.res);
    HIPCHK(c, hipGetLastError());
    mo_stage_mark(c, "correct_merge");
    if ((rc = b.res.download(c))) return rc;
    // (into is read only after a call that fused: the kernel behind the flag leaves it unwritten otherwise, and the identity above stays)
    std::vector<int32_t> into;
    if (out->into) {
        into.resize(np);
        HIPCHK(c, hipMemcpyAsync(into.data(), b.into, np * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if (out->moved) HIPCHK(c, hipMemcpyAsync(out->moved, b.moved, np, hipMemcpyDeviceToHost, c->stream));
    if ((rc = map_sync(c, clk))) return rc;
    const CrRes& r = b.res.host();
    for (int i = 0; i < 12; i++) out->A[i] = g.A[i];
    out->A_scale = inv;
    if (out->poses_out)
        for (int e = 0; e < nt; e++) std::memcpy(out->poses_out + (size_t)cpos[e] * 12, pose.data() + (size_t)e * 12, 96);
    out->n_corrected = nt; out->n_moved = r.n_moved; out->n_loop_points = r.n_loop_points;
    out->n_direct_edges = r.n_direct_edges; out->n_direct_gained = r.n_direct_gained;
    out->n_pairs = r.n_pairs; out->n_cand = r.n_cand; out->n_proposals = r.n_proposals; out->n_gained = r.n_gained; out->n_edges = r.n_edges;
    if (!r.n_proposals && !r.n_direct_edges && !r.n_direct_gained) return MO_OK;   // (the move and kP are written in place; the store is not flipped)
    out->n_absorbed = r.n_absorbed;
    if (out->into) std::copy(into.begin(), into.end(), out->into);
    m->cur ^= 1;
    m->n_pts = r.n_points; m->n_obs = r.n_obs;
    out->n_points = m->n_pts; out->n_obs = m->n_obs;
    return MO_OK;
}
