// The closed forms of virgo-plus_amd/csrc/vp_fri_layout.h against the incremental recurrences the FRI drivers used to keep in offset vectors
// (restated here, loop by loop), for every ln in 1..19 and every lw in 0..6 with ln - lw >= 1: each offset equal, consecutive levels of a buffer
// disjoint, each buffer's total within the size the commitment allocates for it (the allocation expressions restated here too).
// Prints the number of shapes and levels checked; exit status 1 and the first mismatches otherwise.  Built by tests/test_sanitizers.py under
// -fsanitize=address,undefined with plain g++.
#include <cstdio>
#include <vector>

#include "../../virgo-plus_amd/csrc/vp_fri_layout.h"

static int bad = 0;
static void expect(bool ok, const char *what, int ln, int lw, int k, size_t got, size_t want) {
    if (ok) return;
    if (bad++ < 20) std::printf("MISMATCH %s: ln %d lw %d level %d: %zu vs %zu\n", what, ln, lw, k, got, want);
}
#define EQ(what, k, got, want) expect((size_t) (got) == (size_t) (want), what, ln, lw, (k), (size_t) (got), (size_t) (want))
#define LE(what, k, a, b) expect((size_t) (a) <= (size_t) (b), what, ln, lw, (k), (size_t) (a), (size_t) (b))

int main() {
    long shapes = 0, levels = 0;
    for (int ln = 1; ln <= 19; ++ln)
        for (int lw = 0; lw <= 6 && ln - lw >= 1; ++lw) {
            const FriLayout fl(ln, lw);
            const size_t N = (size_t) 1 << ln, M = 32 * N, W = (size_t) 1 << lw, Nl = N >> lw;
            const int n_local = ln - lw;
            ++shapes;
            EQ("n_local", -1, fl.n_local(), n_local);

            // ---- unsharded (vp_fri_step / vp_fri_commit): cw_off += 64 * 32 * No, tree_used += 2 * n_leaves, m_off += 32 * No; No = N >> (k + 1)
            if (lw == 0) {
                size_t cw_off = 0, tree_used = 0, m_off = 0;
                for (int k = 0; k < ln; ++k, ++levels) {
                    const size_t No = (N >> k) >> 1, n_leaves = 16 * No;
                    EQ("per_coset", k, fl.per_coset(k), No);
                    EQ("leaves", k, fl.leaves(k), n_leaves);
                    EQ("cw", k, fl.cw(k), cw_off);
                    EQ("tree", k, fl.tree(k), tree_used);
                    EQ("mask", k, fl.mask(k), m_off);
                    cw_off += (size_t) 64 * 32 * No; tree_used += 2 * n_leaves; m_off += (size_t) 32 * No;
                    // the level ends where the next begins (or at the total): no overlap
                    LE("cw end", k, fl.cw(k) + 2048 * No, k + 1 < ln ? fl.cw(k + 1) : fl.cw_total());
                    LE("tree end", k, fl.tree(k) + 2 * n_leaves, k + 1 < ln ? fl.tree(k + 1) : fl.tree_total());
                    LE("mask end", k, fl.mask(k) + 32 * No, k + 1 < ln ? fl.mask(k + 1) : fl.mask_total());
                }
                EQ("cw_total", ln, fl.cw_total(), cw_off);
                EQ("tree_total", ln, fl.tree_total(), tree_used);
                EQ("mask_total", ln, fl.mask_total(), m_off);
                LE("pc_fri_all", ln, fl.cw_total(), (size_t) 64 * M);          // dalloc(pc_fri_all, 64 * M)
                LE("pc_fri_tree", ln, fl.tree_total(), M);                      // dalloc(pc_fri_tree, M)
                LE("pc_fm", ln, fl.mask_total(), M);                            // dalloc(pc_fm, M)
            }

            // ---- sharded, local levels (pcs_fri_commit stage 1 / pcs_fri_step): fri_off = {0}; per fold k < n_local: push(off), off += 64 * 32 * No with
            // off starting behind the level-0 input (64 * 32 * Nl); a level with No >= 2: tree_f_off.push(toff), toff += 2 * 16 * No;
            // top_f_off.push(top), top += 2 * ((No >> 1) << lw)
            std::vector<size_t> fri_off(1, 0), tree_f_off, top_f_off;
            size_t off = (size_t) 64 * 32 * Nl, toff = 0, top = 0;
            for (int k = 0; k < n_local; ++k, ++levels) {
                const size_t Nk = Nl >> k, No = Nk >> 1;
                fri_off.push_back(off);
                EQ("loc_in", k, fl.loc_in(k), fri_off[k]);
                EQ("loc_cw", k, fl.loc_cw(k), fri_off[k + 1]);
                EQ("loc_per_coset", k, fl.loc_per_coset(k), No);
                EQ("per_coset (global)", k, fl.per_coset(k), No << lw);
                LE("loc_in end", k, fl.loc_in(k) + 2048 * Nk, fl.loc_cw(k));
                off += (size_t) 64 * 32 * No;
                LE("loc_cw end", k, fl.loc_cw(k) + 2048 * No, k + 1 < n_local ? fl.loc_cw(k + 1) : fl.loc_cw_total());
                EQ("is_tail", k, fl.is_tail(k), !(No >= 2));
                if (No >= 2) {
                    const size_t n_leaves = 16 * No;
                    tree_f_off.push_back(toff); top_f_off.push_back(top);
                    EQ("loc_tree", k, fl.loc_tree(k), toff);
                    EQ("top", k, fl.top(k), top);
                    toff += 2 * n_leaves;
                    top += 2 * ((No >> 1) << lw);
                    const bool more = k + 1 < n_local - 1;
                    LE("loc_tree end", k, fl.loc_tree(k) + 2 * n_leaves, more ? fl.loc_tree(k + 1) : fl.loc_tree_total());
                    LE("top end", k, fl.top(k) + 2 * ((No >> 1) << lw), more ? fl.top(k + 1) : fl.top_total());
                }
            }
            EQ("loc_cw_total", n_local, fl.loc_cw_total(), off);
            EQ("loc_tree_total", n_local, fl.loc_tree_total(), toff);
            EQ("top_total", n_local, fl.top_total(), top);
            // pcs_alloc: fri_loc 2 * 64 * 32 * Nl, tree_f 32 * Nl, top_f N
            LE("fri_loc", n_local, fl.loc_cw_total(), (size_t) 2 * 64 * 32 * Nl);
            LE("tree_f", n_local, fl.loc_tree_total(), (size_t) 32 * Nl);
            LE("top_f", n_local, fl.top_total(), N);

            // ---- sharded, replicated tail (the tail loop of pcs_fri_commit / stages 2 and 3 of pcs_fri_step): levels k = n_local - 1 .. ln - 1, index q;
            // tail_cw_off = {0}, coff = 2048 << lw; per level: tail_tree_off.push(ttoff), ttoff += 2 * n_leaves (n_leaves = Nt >= 2 ? 16 Nt : 16);
            // then, while a level follows: tail_cw_off.push(coff), coff += 64 * 32 * (Nt >> 1), Nt >>= 1
            std::vector<size_t> tail_cw_off(1, 0), tail_tree_off;
            size_t coff = (size_t) 2048 << lw, ttoff = 0, Nt = W;
            for (int k = n_local - 1; k < ln; ++k, ++levels) {
                const int q = k - (n_local - 1);
                const size_t n_leaves = Nt >= 2 ? 16 * Nt : 16;
                tail_tree_off.push_back(ttoff);
                EQ("is_tail (tail)", k, fl.is_tail(k), true);
                EQ("tail_q", k, fl.tail_q(k), q);
                EQ("tail_per_coset", k, fl.tail_per_coset(q), Nt);
                EQ("per_coset (tail, global)", k, fl.per_coset(k), Nt);
                EQ("tail_leaves", k, fl.tail_leaves(q), n_leaves);
                EQ("leaves (tail, global)", k, fl.leaves(k), n_leaves);
                EQ("tail_cw", k, fl.tail_cw(q), tail_cw_off.back());
                EQ("tail_tree", k, fl.tail_tree(q), ttoff);
                ttoff += 2 * n_leaves;
                const bool more = k + 1 < ln;
                LE("tail_cw end", k, fl.tail_cw(q) + 2048 * Nt, more ? fl.tail_cw(q + 1) : fl.tail_cw_total());
                LE("tail_tree end", k, fl.tail_tree(q) + 2 * n_leaves, more ? fl.tail_tree(q + 1) : fl.tail_tree_total());
                if (more) { tail_cw_off.push_back(coff); coff += (size_t) 64 * 32 * (Nt >> 1); Nt >>= 1; }
            }
            EQ("tail levels", ln, tail_tree_off.size(), (size_t) lw + 1);
            EQ("tail_cw_total", ln, fl.tail_cw_total(), tail_cw_off.back() + 2048);
            EQ("tail_tree_total", ln, fl.tail_tree_total(), ttoff);
            // pcs_alloc: tail (4 * 2048) << lw, tail_tree (4 * 32) << lw
            LE("tail", ln, fl.tail_cw_total(), (size_t) 4 * 2048 << lw);
            LE("tail_tree", ln, fl.tail_tree_total(), (size_t) 4 * 32 << lw);
            // the one-pass phase gathers the W x 2048 tail elements at tail_gather() of the same buffer: behind the levels, inside the allocation
            LE("tail gather begin", ln, fl.tail_cw_total(), fl.tail_gather());
            LE("tail gather end", ln, fl.tail_gather() + 2048 * W, (size_t) 4 * 2048 << lw);
        }
    if (bad) { std::printf("fri_layout: %d mismatches\n", bad); return 1; }
    std::printf("fri_layout ok: %ld shapes, %ld levels\n", shapes, levels);
    return 0;
}
