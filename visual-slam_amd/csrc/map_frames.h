// map_frames.h -- the frames of a batch call (mo_map_track_batch, mo_map_relocalize_batch, mo_map_query_keyframes_batch) looked up and
// staged into [frame][stride] device buffers: host frames packed into pinned memory and uploaded in one copy per array, resident frames
// copied on the device.  The store's spare slot is not used.  The buffers are the caller's (its feature's scratch).  Private to the library.
#pragma once
#include <cstring>
#include <vector>

#include "common.h"

struct BatchFrames {
    std::vector<int> slot;                // by frame: its resident slot, -1: host arrays
    bool any_host = false, any_rows = false;
    int max_n = 0;                        // the widest frame
};

// every frame looked up, its row count into h_fcnt[i]: everything is known and checked before anything is written.  MO_ERR_ARG
// (limit_msg) for a frame of more than `limit` rows.
inline int batch_frames_lookup(mo_ctx* c, const mo_frame_ref* frames, int nf, int limit, const char* limit_msg, int32_t* h_fcnt, BatchFrames* bf) {
    bf->slot.assign((size_t)nf, -1);
    bf->any_host = bf->any_rows = false;
    bf->max_n = 0;
    for (int i = 0; i < nf; i++) {
        int n;
        if (int rc = mo_frame_lookup(c, &frames[i], "frame", &bf->slot[i], &n)) return rc;
        if (n > limit) return mo_fail(c, MO_ERR_ARG, limit_msg);
        h_fcnt[i] = n;
        bf->any_host |= bf->slot[i] < 0 && n > 0;
        bf->any_rows |= n > 0;
        bf->max_n = std::max(bf->max_n, n);
    }
    return MO_OK;
}

// the pinned sides of the host frames, reserved when there is one (rows = frames x stride)
inline int batch_frames_reserve_host(mo_ctx* c, const BatchFrames& bf, size_t rows, PinnedBuf<mo_keypoint>& h_fk, PinnedBuf<uint8_t>& h_fdesc) {
    if (!bf.any_host) return MO_OK;
    if (int rc = h_fk.reserve(c, rows)) return rc;
    return h_fdesc.reserve(c, rows * 32);
}

// the staging, enqueued on the context stream: the host frames in one upload per array, then the resident frames device to device
inline int batch_frames_stage(mo_ctx* c, const mo_frame_ref* frames, int nf, size_t stride, const BatchFrames& bf, const int32_t* h_fcnt,
                              mo_keypoint* h_fk, uint8_t* h_fdesc, mo_keypoint* fk, uint8_t* fdesc) {
    const size_t rows = (size_t)nf * stride;
    if (bf.any_host) {
        for (int i = 0; i < nf; i++) {
            if (bf.slot[i] >= 0 || h_fcnt[i] == 0) continue;
            const size_t at = (size_t)i * stride, n = (size_t)h_fcnt[i];
            std::memcpy(h_fk + at, frames[i].kps, n * sizeof(mo_keypoint));
            std::memcpy(h_fdesc + at * 32, frames[i].desc, n * 32);
        }
        HIPCHK(c, hipMemcpyAsync(fk, h_fk, rows * sizeof(mo_keypoint), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(fdesc, h_fdesc, rows * 32, hipMemcpyHostToDevice, c->stream));
    }
    for (int i = 0; i < nf; i++)
        if (bf.slot[i] >= 0)
            if (int rc = mo_frame_copy_rows(c, &frames[i], bf.slot[i], h_fcnt[i], fk + (size_t)i * stride, fdesc + (size_t)i * stride * 32)) return rc;
    return MO_OK;
}
