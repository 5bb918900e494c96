// absorb.h -- the rules of mo_map_absorb (include/vslam_amd.h states them; map_absorb.hip launches them): what one point and one
// observation entry of the absorbed map become in the absorbing one, and the argument checks that run before anything is reserved.
// Plain C++, no HIP include: tests/native/absorb_check.cpp compiles it alone, the kernels of map_absorb.hip call the same functions.
//
// The checks, in the order made (mo_map_absorb returns MO_ERR_ARG with the text, MO_ERR_CAPACITY for ABSORB_INT32 and
// MO_ERR_UNSUPPORTED for ABSORB_KEYFRAMES):
//   ABSORB_NULL      dst, src, params or out is NULL.
//   ABSORB_SELF      src == dst (a map is not appended to itself: the kernels read src while they write dst).
//   ABSORB_SHIFT     dref_injected_shift outside 0 .. INT32_MAX (it is subtracted from an int32).
//   ABSORB_CONTEXT   the two maps belong to different contexts (one stream orders the chain, one device holds both).
//   ABSORB_INT32     a sum past what snapshot.h's SNAP_INT32 allows: n_pts, n_obs <= INT32_MAX / 2, id_bound <= 2^31, kf_stored <=
//                    INT32_MAX.  The absorbed map would otherwise be one that mo_map_import refuses.
//   ABSORB_KEYFRAMES more keyframes after the call than one launch of the snapshot kernels covers (65535): the result must stay
//                    exportable, and the row copies here are launched the same way.
#pragma once
#include <climits>
#include <cstdint>

#include "../../include/vslam_amd.h"

#if defined(__HIPCC__)
#define ABSORB_HD __host__ __device__ __forceinline__
#else
#define ABSORB_HD inline
#endif

#define ABSORB_NULL "NULL argument"
#define ABSORB_SELF "a map cannot absorb itself"
#define ABSORB_CONTEXT "the two maps belong to different contexts"
#define ABSORB_SHIFT "dref_injected_shift must be in 0 .. INT32_MAX"
#define ABSORB_INT32 "the absorbed map would be beyond int32 indexing"
#define ABSORB_KEYFRAMES "more keyframes than one launch of the snapshot kernels covers (65535)"

#define ABSORB_MAX_KF 65535

// the counters of one map that the sums are formed from
struct AbsorbSizes {
    int64_t n_kf, n_pts, n_obs, id_bound, kf_stored;
};

// what is added to the indices of the absorbed map: the absorbing map's counters in front of the call
struct AbsorbOffsets {
    int32_t kf;       // positions: n_kf of dst
    int32_t pt;       // point indices: n_pts of dst
    int32_t obs;      // entry offsets: n_obs of dst
    int32_t id;       // ids: id_bound of dst
    int32_t ord;      // ordinals (dref_kf >= 0, born): kf_stored of dst
    int32_t shift;    // injected references (dref_kf < 0): dref_injected_shift
    int32_t now;      // the ordinal of the last stored keyframe after the call (0 without one): no born lies past it
};

inline const char* absorb_args_violation(const void* dst, const void* src, const mo_map_absorb_params* prm, const void* out) {
    if (!dst || !src || !prm || !out) return ABSORB_NULL;
    if (dst == src) return ABSORB_SELF;
    if (prm->dref_injected_shift < 0 || prm->dref_injected_shift > INT32_MAX) return ABSORB_SHIFT;
    return nullptr;
}

// behind absorb_args_violation: the contexts and the sums
inline const char* absorb_sizes_violation(const void* dst_ctx, const void* src_ctx, const AbsorbSizes& d, const AbsorbSizes& s) {
    if (dst_ctx != src_ctx) return ABSORB_CONTEXT;
    if (d.n_pts + s.n_pts > INT32_MAX / 2 || d.n_obs + s.n_obs > INT32_MAX / 2 || d.id_bound + s.id_bound > (int64_t)INT32_MAX + 1 ||
        d.kf_stored + s.kf_stored > INT32_MAX)
        return ABSORB_INT32;
    if (d.n_kf + s.n_kf > ABSORB_MAX_KF) return ABSORB_KEYFRAMES;
    return nullptr;
}

// a map without live keyframes and without points has nothing to append: the call changes nothing, counters included
inline bool absorb_is_noop(const AbsorbSizes& s) { return s.n_kf == 0 && s.n_pts == 0; }

// ---- one point (A2).  xyz, col and dref_row keep their bytes; these change:
ABSORB_HD int32_t absorb_id(int32_t id, const AbsorbOffsets& o) { return (int32_t)((uint32_t)id + (uint32_t)o.id); }
// an ordinal moves behind dst's; a negative value is the host's index into its injected dicts (-(j + 1)) and moves behind dst's dicts
ABSORB_HD int32_t absorb_dref_kf(int32_t dkf, const AbsorbOffsets& o) {
    return dkf >= 0 ? (int32_t)((uint32_t)dkf + (uint32_t)o.ord) : (int32_t)((uint32_t)dkf - (uint32_t)o.shift);
}
// life {visible, found, born, 0} in and out as four int32.  born moves behind dst's history and is held at the new `now`: that binds
// only for a src that never stored a keyframe (its points carry born 0, its history is empty), whose points are then as old as
// dst's last keyframe; the snapshot rule born <= now (snapshot.h, SNAP_LIFE) holds either way.
ABSORB_HD void absorb_life(const int32_t in[4], const AbsorbOffsets& o, int32_t out[4]) {
    const int64_t born = (int64_t)in[2] + o.ord;
    out[0] = in[0]; out[1] = in[1]; out[2] = (int32_t)(born < o.now ? born : o.now); out[3] = 0;
}
// off[pt + i + 1] of dst from off[i + 1] of src
ABSORB_HD int32_t absorb_off(int32_t off_src, const AbsorbOffsets& o) { return o.obs + off_src; }

// ---- one observation entry (A3).  (kf, kp) is read as map_obs (map_store.h) reads it on src: negative values index from the end,
// count_of(pos) = the rows of src's keyframe at position pos.  An entry that names a row is written normalised and moved behind dst's
// positions; one that names nothing is written so that it names nothing in dst whatever is added later: no keyframe count reaches
// INT32_MIN + n_kf >= 0.
template <class CountOf> ABSORB_HD void absorb_entry(int32_t kf, int32_t kp, int32_t n_kf_src, CountOf count_of, const AbsorbOffsets& o, int32_t* kf_out,
                                                     int32_t* kp_out) {
    *kf_out = INT32_MIN; *kp_out = kp;
    if (kf < 0) kf += n_kf_src;
    if (kf < 0 || kf >= n_kf_src) return;
    const int32_t nk = count_of(kf);
    int32_t r = kp;
    if (r < 0) r += nk;
    if (r < 0 || r >= nk) return;
    *kf_out = o.kf + kf; *kp_out = r;
}
