// Which of the commitment's 64 input-layer slices hold anything.  The input layer has 2^n entries of which the first n_used carry values and the tail is zero
// (vp_evaluate and vp_pc_load_input zero-fill it); a slice is N = 2^(n-6) consecutive entries, so slices >= live = ceil(n_used / N) are zero, and with them
// their coefficients, their l / h codewords, their virtual oracle and their share of every FRI level (lib/virgo/src/poly_commit.h:265-281 has the same
// special case, all_zero).  The transforms, products and folds run over the live slices only; the regions of the dead ones are kept as zero bytes for the
// hashes and openings, which read all 64.
// The real-pair encode of vp_commit_private carries slices p and p + pair_rows in one complex transform: pair_rows = ceil(live / 2) rows cover 0 .. live - 1
// (at odd live the last partner, slice 2 pair_rows - 1 = live, is a dead slice: read as zeros, written as the zeros the transform computes).
// Host only, no HIP types (tests/sanitize/pc_live_main.cpp checks the rule at every size, under plain g++).
#pragma once
#include <cstdint>

struct PcLive {
    unsigned live = 64, pair_rows = 32;
    PcLive() = default;
    // n: bit length of the input layer (>= 7), n_used: entries that may be non-zero (1 .. 2^n), enabled = 0: all 64 slices (VP_PC_LIVE=0)
    PcLive(int n, uint64_t n_used, bool enabled) {
        if (enabled && n >= 7) {
            const uint64_t N = (uint64_t) 1 << (n - 6), c = (n_used + N - 1) / N;
            live = c < 1 ? 1u : c > 64 ? 64u : (unsigned) c;
        }
        pair_rows = (live + 1) / 2;
    }
    unsigned pair_a(unsigned p) const { return p; }                     // the two slices of pair row p < pair_rows
    unsigned pair_b(unsigned p) const { return p + pair_rows; }
    unsigned pair_end() const { return 2 * pair_rows; }                 // slices below this are written by the paired encode (live or live + 1, <= 64)
};
