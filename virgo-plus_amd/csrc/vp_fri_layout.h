// Where a FRI level of the commitment lives: element offsets into the buffers that keep every level for the openings, as closed forms of
// (ln, lw, k).  ln = log2 of the values per coset of the committed codewords (N), lw = log2 of the ranks the commitment is sharded over (W;
// 0: the unsharded commitment), k = FRI level (the output of fold k; N >> (k + 1) values per coset, 16 of its leaves per value).  Every
// buffer holds its levels end to end and a level is half the one before it, so an offset is a geometric sum: c * (X - (X >> k)).
// Host only, no HIP types (tests/sanitize/fri_layout_main.cpp checks the forms against the recurrences they replace, under plain g++).
#pragma once
#include <cstddef>

struct FriLayout {
    int ln = 0, lw = 0;
    size_t N = 1, W = 1, Nl = 1;                          // values per coset of the committed codeword, ranks, values per coset a rank holds (N / W)
    FriLayout() = default;
    FriLayout(int ln_, int lw_) : ln(ln_), lw(lw_), N((size_t) 1 << ln_), W((size_t) 1 << lw_), Nl((size_t) 1 << (ln_ - lw_)) {}

    // sizes of level k (the whole level, whoever holds it)
    size_t per_coset(int k) const { return N >> (k + 1); }
    size_t leaves(int k) const { return 16 * per_coset(k); }

    // unsharded: codeword in pc_fri_all (64 x 32 rows), tree in pc_fri_tree (heap of 2 x leaves digests), mask slice in pc_fm (32 rows)
    size_t cw(int k) const { return 2048 * (N - (N >> k)); }
    size_t tree(int k) const { return 32 * (N - (N >> k)); }
    size_t mask(int k) const { return 32 * (N - (N >> k)); }
    size_t cw_total() const { return cw(ln); }            // (the last level has one value per coset: off(ln) is where a further level would start)
    size_t tree_total() const { return tree(ln); }
    size_t mask_total() const { return mask(ln); }

    // sharded: the first n_local folds pair positions of one rank; level k < n_local - 1 keeps >= 2 positions per coset on a rank and is hashed
    // there (local tree + replicated top tree); from level n_local - 1 on every rank holds the whole level (the replicated tail, index q)
    int n_local() const { return ln - lw; }
    bool is_tail(int k) const { return k >= n_local() - 1; }
    int tail_q(int k) const { return k - (n_local() - 1); }
    size_t loc_per_coset(int k) const { return Nl >> (k + 1); }
    size_t loc_in(int k) const { return 2048 * (2 * Nl - ((2 * Nl) >> k)); }   // fri_loc: input of local fold k (k = 0: the virtual oracle, at 0)
    size_t loc_cw(int k) const { return loc_in(k + 1); }                        // fri_loc: level k, k < n_local
    size_t loc_tree(int k) const { return 32 * (Nl - (Nl >> k)); }              // tree_f: local leaves + five levels of level k, k < n_local - 1
    size_t top(int k) const { return N - (N >> k); }                            // top_f: heap over the level's N >> (k + 2) level-5 nodes
    size_t tail_per_coset(int q) const { return W >> q; }
    size_t tail_leaves(int q) const { return 16 * tail_per_coset(q); }
    size_t tail_cw(int q) const { return 2048 * (2 * W - ((2 * W) >> q)); }     // tail
    size_t tail_tree(int q) const { return 32 * (2 * W - ((2 * W) >> q)); }     // tail_tree
    size_t loc_cw_total() const { return loc_in(n_local()) + 2048; }
    size_t loc_tree_total() const { return loc_tree(n_local() - 1); }
    size_t top_total() const { return top(n_local() - 1); }
    size_t tail_cw_total() const { return tail_cw(lw + 1); }
    size_t tail_tree_total() const { return tail_tree(lw + 1); }
    size_t tail_gather() const { return 2 * 2048 * W; }                         // tail: where the one-pass phase gathers the ranks' W x 2048 tail elements, behind the levels
};
