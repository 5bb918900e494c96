// bow.h -- place recognition on the device map (bow.hip): the binary vocabulary (mo_vocab), the keyframe database a map carries once a
// vocabulary is attached, and the preselection mo_map_relocalize_pre runs inside its own chain.  The rules are stated above
// mo_vocab_train in include/vslam_amd.h.  Private to the library.
#pragma once
#include <vector>

#include "common.h"
#include "map_store.h"

// a vocabulary: W words of 32 bytes and one weight per word, on the device and as the host copy mo_vocab_download hands out; rows and
// weights are padded to Wp (a multiple of 8: the database rows are read 16 bytes at a time), the padding weights are 0
struct mo_vocab {
    mo_ctx* c = nullptr;
    int W = 0, Wp = 0;
    DevBuf<uint8_t> words;       // [W][32]
    DevBuf<int32_t> weights;     // [Wp]
    std::vector<uint8_t> h_words;
    std::vector<int32_t> h_weights;
};

// What the preselection leaves on the device for the matching of mo_map_relocalize_pre (valid behind bow_select_enqueue, on the
// context stream): pair j < n_pre matches frame qf[j] against keyframe slot tf[j] with the row counts cnt; a pair past the selected
// keyframes names an empty query frame, so the matcher does nothing for it.  mrow[k] = the pair of keyframe position k, -1: not selected.
struct BowSel {
    const int32_t* cnt = nullptr;
    const int32_t* qf = nullptr;
    const int32_t* tf = nullptr;
    const int32_t* mrow = nullptr;
};

// MO_ERR_ARG unless a vocabulary is attached to the map
int bow_require(mo_map* m);
// the query chain of mo_map_query_keyframes for the frame staged in the spare slot (n rows), ranked to n_pre places, enqueued on the
// context stream inside the caller's stage set (marks bow_quantise, bow_hist, bow_score, bow_rank); no synchronisation
int bow_select_enqueue(mo_map* m, int n, int n_pre, BowSel* sel);

// The per-row words of the database (valid behind bow_words_enqueue on the context stream): word [slot][stride], the word of every row
// of every keyframe slot under the quantisation rule, and in the spare slot (m->kslots) those of the staged frame; W words.
struct BowWords {
    const uint16_t* word = nullptr;
    int stride = 0, W = 0;
};
// every stale row of the database and the row of the frame staged in the spare slot (n rows) brought up to date, as the query does,
// inside the caller's stage set with no stage mark of its own; enqueued, no synchronisation.  MO_ERR_UNSUPPORTED above MO_BOW_MAX_ROWS.
int bow_words_enqueue(mo_map* m, int n, BowWords* out);

// What the scoring of mo_map_loop_candidates (map_loop.hip) leaves on the device, valid behind bow_loop_score_enqueue on the context
// stream: cnt = the row counts by keyframe slot as the database update uploaded them (frame `empty` has 0 rows), score [n_kf] and
// common [n_kf] by keyframe position.
struct BowLoop {
    const int32_t* cnt = nullptr;
    const double* score = nullptr;
    const int32_t* common = nullptr;
    int empty = 0;
};
// every stale row of the database brought up to date, no frame staged: the spare slot's row is neither counted nor cleared, and with
// no stale keyframe nothing is launched (marks bow_quantise, bow_hist either way); enqueued, no synchronisation
int bow_update_enqueue(mo_map* m);
// mo_map_query_keyframes' D_k and score of every keyframe with the database row of the keyframe at position q_pos as the query, and in
// the same pass the common-word counts (0 for q_pos and for every k with wrow[k] >= min_w; wrow = row q_pos of the covisibility matrix,
// on the device); mark loop_score; behind bow_update_enqueue
int bow_loop_score_enqueue(mo_map* m, int q_pos, const int32_t* wrow, int min_w, BowLoop* out);
// mo_map_loop_candidates_among's one rule, behind bow_loop_score_enqueue: common[k] = 0 where among[k] == 0 (among [n_kf] on the device);
// mark loop_among
int bow_loop_among_enqueue(mo_map* m, const uint8_t* among);

// ---- a batch of query frames (mo_map_relocalize_batch, mo_map_query_keyframes_batch) ---------------------------------------------------
// The frames are staged by the caller in fdesc [frame][stride][32]; cnt is the matcher's combined count array, built by the caller:
// [0, S) the store's row counts by slot (S = kslots + 1), [S, S + nf) the frames', [S + nf] = W (the words as a train frame),
// [S + nf + 1] = 0 (the empty frame).  Frame f is query frame S + f of a matcher launch whose query base is bow_batch_qbase.
// Enqueued on the context stream inside the caller's stage set, no mark, no synchronisation: the database update of the stale keyframe
// slots (once), one quantisation launch (a pair per frame), one histogram and norm per frame in the batch's own rows (the database's
// spare row is not used), the scores over (frame, keyframe), the ranking with one workgroup per frame.  Valid behind it: pos / score
// [frame][n_best], n [frame]; with sel, qf / tf [frame][n_best] = frame f's slice of the matcher's pair list (pairs past the selected
// keyframes name the empty frame) and mrow [frame][n_kf] = the pair of (frame, position) inside its slice, -1: none.
struct BowBatch {
    const int32_t* pos = nullptr; const double* score = nullptr; const int32_t* n = nullptr;
    const int32_t* qf = nullptr; const int32_t* tf = nullptr; const int32_t* mrow = nullptr;
};
// the vocabulary's words (0 without one): what the caller writes at cnt[S + nf]
int bow_words(const mo_map* m);
// the query base that makes frame S + f of the matcher frame f of fdesc
inline const uint8_t* bow_batch_qbase(const uint8_t* fdesc, int S, size_t stride) { return (const uint8_t*)((uintptr_t)fdesc - (size_t)S * stride * 32); }
int bow_batch_enqueue(mo_map* m, const uint8_t* fdesc, const int32_t* cnt, const int32_t* h_fcnt, int nf, int stride, int n_best, bool sel, BowBatch* out);
