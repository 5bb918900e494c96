// absorb_check.cpp -- visual-slam_amd/csrc/absorb.h on the host (tests/test_absorb_cpu.py compiles it with AddressSanitizer and UBSan):
// every refusal of mo_map_absorb's argument checks with its text, valid arguments at the bounds, and the per-element rules on valid,
// negative, out-of-range and INT32_MIN values.  Prints one line per case, "<kind> <name> | <expected> | <got>", and returns the number
// of mismatches.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../visual-slam_amd/csrc/absorb.h"

static int n_bad = 0;
static void expect(const char* kind, const char* name, const char* got, const char* want) {
    const char* g = got ? got : "ok";
    std::printf("%s %s | %s | %s\n", kind, name, want, g);
    if (std::strcmp(g, want) != 0) n_bad++;
}
static void expect_pair(const char* name, int32_t kf, int32_t kp, int32_t want_kf, int32_t want_kp) {
    const std::string want = std::to_string(want_kf) + "," + std::to_string(want_kp), got = std::to_string(kf) + "," + std::to_string(kp);
    expect("rule", name, got.c_str(), want.c_str());
}
static void expect_int(const char* name, int64_t got, int64_t want) {
    expect("rule", name, std::to_string(got).c_str(), std::to_string(want).c_str());
}

int main() {
    int a = 0, b = 0, ctx1 = 0, ctx2 = 0;   // stand-ins: only their addresses are compared
    mo_map_absorb_params prm{0};
    mo_map_absorb_out out{};
    const AbsorbSizes small{3, 10, 20, 12, 4};
    const int64_t half = INT32_MAX / 2;

    // ---- the argument checks
    expect("valid", "plain", absorb_args_violation(&a, &b, &prm, &out), "ok");
    expect("broken", "null_dst", absorb_args_violation(nullptr, &b, &prm, &out), ABSORB_NULL);
    expect("broken", "null_src", absorb_args_violation(&a, nullptr, &prm, &out), ABSORB_NULL);
    expect("broken", "null_params", absorb_args_violation(&a, &b, nullptr, &out), ABSORB_NULL);
    expect("broken", "null_out", absorb_args_violation(&a, &b, &prm, nullptr), ABSORB_NULL);
    expect("broken", "self", absorb_args_violation(&a, &a, &prm, &out), ABSORB_SELF);
    prm.dref_injected_shift = -1;
    expect("broken", "negative_shift", absorb_args_violation(&a, &b, &prm, &out), ABSORB_SHIFT);
    prm.dref_injected_shift = (int64_t)INT32_MAX + 1;
    expect("broken", "shift_past_int32", absorb_args_violation(&a, &b, &prm, &out), ABSORB_SHIFT);
    prm.dref_injected_shift = INT32_MAX;
    expect("valid", "largest_shift", absorb_args_violation(&a, &b, &prm, &out), "ok");

    expect("valid", "small_maps", absorb_sizes_violation(&ctx1, &ctx1, small, small), "ok");
    expect("broken", "contexts", absorb_sizes_violation(&ctx1, &ctx2, small, small), ABSORB_CONTEXT);
    // each sum exactly at its bound passes, one past it is refused
    expect("valid", "points_at_bound", absorb_sizes_violation(&ctx1, &ctx1, AbsorbSizes{1, half - 10, 0, 1, 1}, small), "ok");
    expect("broken", "points_past_bound", absorb_sizes_violation(&ctx1, &ctx1, AbsorbSizes{1, half - 9, 0, 1, 1}, small), ABSORB_INT32);
    expect("valid", "entries_at_bound", absorb_sizes_violation(&ctx1, &ctx1, AbsorbSizes{1, 1, half - 20, 1, 1}, small), "ok");
    expect("broken", "entries_past_bound", absorb_sizes_violation(&ctx1, &ctx1, AbsorbSizes{1, 1, half - 19, 1, 1}, small), ABSORB_INT32);
    expect("valid", "ids_at_bound", absorb_sizes_violation(&ctx1, &ctx1, AbsorbSizes{1, 1, 1, (int64_t)INT32_MAX + 1 - 12, 1}, small), "ok");
    expect("broken", "ids_past_bound", absorb_sizes_violation(&ctx1, &ctx1, AbsorbSizes{1, 1, 1, (int64_t)INT32_MAX + 2 - 12, 1}, small), ABSORB_INT32);
    expect("valid", "ordinals_at_bound", absorb_sizes_violation(&ctx1, &ctx1, AbsorbSizes{1, 1, 1, 1, (int64_t)INT32_MAX - 4}, small), "ok");
    expect("broken", "ordinals_past_bound", absorb_sizes_violation(&ctx1, &ctx1, AbsorbSizes{1, 1, 1, 1, (int64_t)INT32_MAX - 3}, small), ABSORB_INT32);
    expect("valid", "keyframes_at_bound", absorb_sizes_violation(&ctx1, &ctx1, AbsorbSizes{ABSORB_MAX_KF - 3, 1, 1, 1, 70000}, small), "ok");
    expect("broken", "keyframes_past_bound", absorb_sizes_violation(&ctx1, &ctx1, AbsorbSizes{ABSORB_MAX_KF - 2, 1, 1, 1, 70000}, small), ABSORB_KEYFRAMES);
    expect_int("noop_empty", absorb_is_noop(AbsorbSizes{0, 0, 0, 0, 0}), 1);
    expect_int("noop_history_only", absorb_is_noop(AbsorbSizes{0, 0, 0, 9, 5}), 1);
    expect_int("noop_points_only", absorb_is_noop(AbsorbSizes{0, 1, 0, 1, 0}), 0);
    expect_int("noop_keyframes_only", absorb_is_noop(AbsorbSizes{1, 0, 0, 0, 1}), 0);

    // ---- the key rule: src has three keyframes of 8, 0 and 5 rows, dst had 7 keyframes
    const std::vector<int32_t> cnt{8, 0, 5};
    const AbsorbOffsets o{7, 100, 1000, 50, 9, 3, 12};
    auto key = [&](const char* name, int32_t kf, int32_t kp, int32_t want_kf, int32_t want_kp) {
        int32_t k2 = 12345, p2 = 12345;
        absorb_entry(kf, kp, (int32_t)cnt.size(), [&](int pos) { return cnt.at((size_t)pos); }, o, &k2, &p2);
        expect_pair(name, k2, p2, want_kf, want_kp);
    };
    key("valid_first", 0, 0, 7, 0);
    key("valid_last_row", 2, 4, 9, 4);
    key("negative_key", -1, 1, 9, 1);
    key("negative_key_first", -3, 7, 7, 7);
    key("negative_row", 0, -1, 7, 7);
    key("both_negative", -1, -5, 9, 0);
    key("key_past_end", 3, 0, INT32_MIN, 0);
    key("key_far_past_end", INT32_MAX, 2, INT32_MIN, 2);
    key("key_before_start", -4, 1, INT32_MIN, 1);
    key("key_int32_min", INT32_MIN, 6, INT32_MIN, 6);
    key("row_past_end", 2, 5, INT32_MIN, 5);
    key("row_before_start", 2, -6, INT32_MIN, -6);
    key("row_int32_min", 0, INT32_MIN, INT32_MIN, INT32_MIN);
    key("row_int32_max", 0, INT32_MAX, INT32_MIN, INT32_MAX);
    key("keyframe_of_0_rows", 1, 0, INT32_MIN, 0);
    key("keyframe_of_0_rows_negative", 1, -1, INT32_MIN, -1);
    {   // a src without keyframes: every entry names nothing and count_of is never asked
        int32_t k2 = 1, p2 = 1;
        absorb_entry(0, 0, 0, [&](int) -> int32_t { n_bad++; return 0; }, o, &k2, &p2);
        expect_pair("no_keyframes", k2, p2, INT32_MIN, 0);
    }

    // ---- the point rules
    expect_int("id", absorb_id(11, o), 61);
    expect_int("id_at_bound", absorb_id(INT32_MAX - 50, o), INT32_MAX);
    expect_int("dref_ordinal", absorb_dref_kf(0, o), 9);
    expect_int("dref_ordinal_last", absorb_dref_kf(3, o), 12);
    expect_int("dref_injected_first", absorb_dref_kf(-1, o), -4);
    expect_int("dref_injected", absorb_dref_kf(-20, o), -23);
    expect_int("dref_injected_wraps_without_trapping", absorb_dref_kf(INT32_MIN, AbsorbOffsets{0, 0, 0, 0, 0, INT32_MAX, 0}), 1);
    expect_int("off", absorb_off(20, o), 1020);
    {
        const int32_t in[4] = {5, 4, 3, 77};
        int32_t l[4];
        absorb_life(in, o, l);
        expect_int("life_visible", l[0], 5); expect_int("life_found", l[1], 4); expect_int("life_born", l[2], 12); expect_int("life_pad", l[3], 0);
        const int32_t first[4] = {1, 1, 0, 0};   // a src that never stored a keyframe, absorbed by a map that stored 9: born is held at now
        absorb_life(first, AbsorbOffsets{7, 100, 1000, 50, 9, 3, 8}, l);
        expect_int("life_born_held_at_now", l[2], 8);
    }
    std::printf("mismatches %d\n", n_bad);
    return n_bad;
}
