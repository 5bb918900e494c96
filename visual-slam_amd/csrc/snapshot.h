// snapshot.h -- the rules a map snapshot (mo_map_snapshot, include/vslam_amd.h) must obey before mo_map_import uploads a byte of it.
// Plain C++ on host arrays, no HIP include: tests/native/snapshot_check.cpp compiles it alone.  One function, snapshot_violation,
// returns the text of the first rule the snapshot breaks (NULL: none); mo_map_import returns MO_ERR_ARG with that text.
//
// Every rule, in the order checked, with the reader that needs it (a reader that checks for itself needs no rule):
//   SNAP_NULL      the snapshot itself.
//   SNAP_COUNTS    n_kf, list_rows, kf_rows, n_pts, n_obs, list_ids, kf_stored, id_bound, st_live[2] >= 0: every one becomes a size_t.
//   SNAP_INT32     n_pts, n_obs, list_ids <= INT32_MAX / 2 (map_int32_guard: kernels form sums of two of them in int); kf_rows <=
//                  INT32_MAX (the row offsets of the pack / unpack kernels are int32); kf_stored <= INT32_MAX (ordinals are int32 in
//                  slot_ord, dref_kf and life.born); id_bound <= 2^31 (ids are int32).
//   SNAP_ARRAY     an array may be NULL only where its count is 0 (obs_off counts n_pts + 1: never; list_off counts list_rows + 1 with
//                  lists, 0 without).
//   SNAP_KF_CNT    kf_cnt[k] >= 0 (a count is a loop bound of every keyframe reader and the row capacity is sized by the largest).  There
//                  is no upper limit: the store has none either (place recognition refuses a keyframe above MO_BOW_MAX_ROWS when asked).
//   SNAP_KF_SUM    sum of kf_cnt == kf_rows (the packed arrays are indexed by the running sum: k_snap_rows).
//   SNAP_KF_ORD    kf_ord strictly increasing and within [0, kf_stored) (positions keep creation order; born <= now and the descriptor
//                  references of a caller rest on it).
//   SNAP_OBS_OFF   obs_off[0] == 0, never decreasing, obs_off[n_pts] == n_obs (every walk over a point's entries, map_each_obs, the
//                  rebuild's map_point_move: obs_kf / obs_kp are indexed by these offsets without a check).
//   SNAP_LIST_OFF  the same for list_off against list_ids; without lists (list_rows == 0) list_ids == 0 (mo_map_download's sizes).
//   SNAP_ID        0 <= id < id_bound (k_first_index's table has id_bound entries; mo_map_add_points refuses negative ids too).
//   SNAP_LIFE      visible and found >= 0 (map_life_merge sums them and clamps at INT32_MAX), 0 <= born <= now (the age now - born of
//                  mo_map_points_bad), now = kf_stored - 1, 0 without a stored keyframe.
//   SNAP_IMAGE     per image w, h >= 0, ch one of 1, 3 (0 only for an image without pixels), img_bytes == w * h * ch (k_map_append and
//                  k_grow_append index the image by (y * w + x) * ch inside [0, w) x [0, h)); img_cur 0 or 1.
//   SNAP_ST_LIVE   st_live[0] == n_pts and st_live[1] == n_obs (the kernels of a chain launched for a bound read the live counts from the
//                  status block and index off[i + 1] below them: k_map_cull, k_map_append).
// Not rules, because every reader checks: observation keys (map_obs skips what names nothing: stale entries are state), dref_kf /
// dref_row (never read), list_ids and kf_red (only copied back to the host), keypoint coordinates (the colour lookup checks them).
#pragma once
#include <climits>
#include <cstdint>

#include "../../include/vslam_amd.h"

#define SNAP_NULL "snapshot is NULL"
#define SNAP_COUNTS "a count of the snapshot is negative"
#define SNAP_INT32 "a count of the snapshot is beyond int32 indexing"
#define SNAP_ARRAY "an array of the snapshot is NULL with a count above 0"
#define SNAP_KF_CNT "kf_cnt must be >= 0"
#define SNAP_KF_SUM "kf_cnt must sum to kf_rows"
#define SNAP_KF_ORD "kf_ord must increase strictly inside [0, kf_stored)"
#define SNAP_OBS_OFF "obs_off must start at 0, never decrease and end at n_obs"
#define SNAP_LIST_OFF "list_off must start at 0, never decrease and end at list_ids"
#define SNAP_ID "every id must lie in [0, id_bound)"
#define SNAP_LIFE "life: visible and found must be >= 0, born in [0, now]"
#define SNAP_IMAGE "an image must have w, h >= 0, ch 1 or 3, img_bytes == w * h * ch, and img_cur must be 0 or 1"
#define SNAP_ST_LIVE "st_live must hold n_pts and n_obs"

// the ordinal of the last stored keyframe of a snapshot (mo_map_point_life's now)
inline int64_t snapshot_now(const mo_map_snapshot_dims_t& d) { return d.kf_stored > 0 ? d.kf_stored - 1 : 0; }

inline const char* snapshot_violation(const mo_map_snapshot* s) {
    if (!s) return SNAP_NULL;
    const mo_map_snapshot_dims_t& d = s->dims;
    if (d.n_kf < 0 || d.list_rows < 0 || d.kf_rows < 0 || d.n_pts < 0 || d.n_obs < 0 || d.list_ids < 0 || d.kf_stored < 0 || d.id_bound < 0 ||
        d.st_live[2] < 0)
        return SNAP_COUNTS;
    if (d.n_pts > INT32_MAX / 2 || d.n_obs > INT32_MAX / 2 || d.list_ids > INT32_MAX / 2 || d.kf_rows > INT32_MAX || d.kf_stored > INT32_MAX ||
        d.id_bound > (int64_t)INT32_MAX + 1)
        return SNAP_INT32;
    // images first among the arrays: their counts are part of what is checked
    if (d.img_cur != 0 && d.img_cur != 1) return SNAP_IMAGE;
    for (int i = 0; i < 2; i++) {
        const int32_t w = d.img_w[i], h = d.img_h[i], ch = d.img_ch[i];
        if (w < 0 || h < 0 || (ch != 0 && ch != 1 && ch != 3)) return SNAP_IMAGE;
        const int64_t px = (int64_t)w * h;
        if (px > 0 && ch == 0) return SNAP_IMAGE;
        if (ch ? (d.img_bytes[i] % ch != 0 || d.img_bytes[i] / ch != px) : d.img_bytes[i] != 0) return SNAP_IMAGE;   // (no product that could overflow)
    }
    const bool lists = d.list_rows > 0;
    if ((d.n_kf > 0 && (!s->kf_cnt || !s->kf_ord || !s->kf_P)) || (d.kf_rows > 0 && (!s->kf_kps || !s->kf_desc)) ||
        (d.n_pts > 0 && (!s->xyz || !s->col || !s->id || !s->dref_kf || !s->dref_row || !s->life)) || !s->obs_off ||
        (d.n_obs > 0 && (!s->obs_kf || !s->obs_kp)) || (lists && (!s->list_off || !s->kf_red)) || (d.list_ids > 0 && !s->list_ids) ||
        (d.img_bytes[0] > 0 && !s->img[0]) || (d.img_bytes[1] > 0 && !s->img[1]))
        return SNAP_ARRAY;
    int64_t sum = 0;
    for (int k = 0; k < d.n_kf; k++) {
        if (s->kf_cnt[k] < 0) return SNAP_KF_CNT;
        sum += s->kf_cnt[k];
    }
    if (sum != d.kf_rows) return SNAP_KF_SUM;
    for (int k = 0; k < d.n_kf; k++)
        if (s->kf_ord[k] < 0 || s->kf_ord[k] >= d.kf_stored || (k > 0 && s->kf_ord[k] <= s->kf_ord[k - 1])) return SNAP_KF_ORD;
    if (s->obs_off[0] != 0 || s->obs_off[d.n_pts] != d.n_obs) return SNAP_OBS_OFF;
    for (int64_t i = 0; i < d.n_pts; i++)
        if (s->obs_off[i + 1] < s->obs_off[i]) return SNAP_OBS_OFF;
    if (lists) {
        if (s->list_off[0] != 0 || s->list_off[d.list_rows] != d.list_ids) return SNAP_LIST_OFF;
        for (int j = 0; j < d.list_rows; j++)
            if (s->list_off[j + 1] < s->list_off[j]) return SNAP_LIST_OFF;
    } else if (d.list_ids != 0) {
        return SNAP_LIST_OFF;
    }
    const int64_t now = snapshot_now(d);
    for (int64_t i = 0; i < d.n_pts; i++) {
        if (s->id[i] < 0 || s->id[i] >= d.id_bound) return SNAP_ID;
        const int32_t* l = s->life + i * 4;
        if (l[0] < 0 || l[1] < 0 || l[2] < 0 || l[2] > now) return SNAP_LIFE;
    }
    if (d.st_live[0] != d.n_pts || d.st_live[1] != d.n_obs) return SNAP_ST_LIVE;
    return nullptr;
}
