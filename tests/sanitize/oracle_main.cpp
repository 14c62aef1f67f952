// TEST INFRASTRUCTURE ONLY.  Sanitizer leg of the CPU build (SURVEY.md §5 "ASan/UBSan CPU targets"): the oracle compiled with
// -fsanitize=address,undefined (make -C oracle asan -> oracle/_build/oracle_asan) and driven through every code path the parity tests use —
// loader + replication, randomize, custom circuits with every gate type, GKR proof, Fiat-Shamir proof, the full protocol with the
// commitment, FRI commit phase, the commitment with masks, primitives, fft_gkr and the GKR prover on caller's tapes.  Exit code 0 and no sanitizer report = pass (tests/test_sanitizers.py).
#include "../../oracle/vp_oracle.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fail(const char *what) { fprintf(stderr, "oracle_asan: %s\n", what); return 1; }

int main(int argc, char **argv) {
    std::vector<uint8_t> buf(1 << 20);
    orc_stats st;
    {   // synthetic circuit: GKR, FS, full protocol (input layer 2^9: the commitment's minimum meaningful size)
        orc_circuit *c = orc_circuit_randomize(4, 9, 3);
        if (!c) return fail("randomize");
        const int64_t n = orc_prove_gkr(c, buf.data(), (int64_t) buf.size(), &st);
        if (n <= 0 || !st.verified) return fail("prove_gkr");
        std::vector<uint8_t> fs(1 << 20);
        const int64_t m = orc_prove_fs(c, fs.data(), (int64_t) fs.size(), &st);
        if (m != n || !st.verified || !memcmp(fs.data(), buf.data(), (size_t) n)) return fail("prove_fs");
        const int64_t k = orc_prove_full(c, buf.data(), (int64_t) buf.size(), &st);
        if (k != n + 32 + 32 + 16 + 65 * 16) return fail("prove_full");
        uint8_t root[32];
        if (orc_commit_private(c, root) != 0 || memcmp(root, buf.data(), 32)) return fail("commit_private");
        const int nb = orc_circuit_layer_bitlen(c, 0);
        std::vector<orc_F> in(1u << nb), pub(1u << nb), r(nb - 6), fin(2048);
        orc_circuit_inputs(c, in.data());
        orc_f_random_seq(9, (int) pub.size(), pub.data());
        orc_f_random_next((int) r.size(), r.data());
        std::vector<uint8_t> roots(32 * r.size());
        if (orc_fri_commit(in.data(), pub.data(), nb, r.data(), roots.data(), fin.data()) != 0) return fail("fri_commit");
        {   // the same commitment with masks: a private mask of 100 elements (pads to 128, more than a slice's message of 8), a shorter public one, three
            // openings; with zero masks the bytes of the unmasked entry; the entry's refusals
            std::vector<orc_F> pm(100), qm(37), fm(32), fin2(2048), fm2(32), ov(3 * 130);
            orc_f_random_seq(11, 100, pm.data());
            orc_f_random_seq(12, 37, qm.data());
            uint8_t rl[32], rh[32], rl2[32], rh2[32];
            orc_F inner, alls[65], inner2, alls2[65];
            std::vector<uint8_t> roots2(roots.size());
            const int64_t at[6] = {0, 0, 1, (1 << (nb - 2)) - 1, 2 + nb - 7, 15};
            if (orc_commitment_array_masked_open(in.data(), in.size(), pub.data(), nb, r.data(), pm.data(), 100, qm.data(), 37, rl, &inner, alls, rh, roots.data(),
                                                 fin.data(), fm.data(), 3, at, ov.data()) != 0) return fail("commitment_array_masked_open");
            if (!alls[64].real && !alls[64].img) return fail("masked all_sum[64]");
            for (auto &x : pm) x = {0, 0};
            if (orc_commitment_array_masked(in.data(), in.size(), pub.data(), nb, r.data(), pm.data(), 100, pm.data(), 1, rl, &inner, alls, rh, roots.data(),
                                            fin.data(), fm.data()) != 0) return fail("commitment_array_masked, zero masks");
            if (orc_commitment_array(in.data(), in.size(), pub.data(), nb, r.data(), rl2, &inner2, alls2, rh2, roots2.data(), fin2.data()) != 0) return fail("commitment_array");
            if (memcmp(rl, rl2, 32) || memcmp(rh, rh2, 32) || memcmp(alls, alls2, sizeof alls) || roots != roots2 || memcmp(fin.data(), fin2.data(), 2048 * sizeof(orc_F)) ||
                memcmp(fm.data(), fm2.data(), 32 * sizeof(orc_F)) /* fm2 is zero */) return fail("zero masks differ from the unmasked entry");
            if (orc_commitment_array_masked(in.data(), in.size(), pub.data(), nb, r.data(), pm.data(), 3, pm.data(), 1, rl, &inner, alls, rh, roots.data(), fin.data(),
                                            fm.data()) != -1) return fail("a mask that pads to fewer than 8 elements");
            if (orc_commitment_array_masked(in.data(), in.size(), pub.data(), nb, r.data(), pm.data(), 100, qm.data(), 37, rl, &inner, alls, rh, roots.data(), fin.data(),
                                            fm.data()) != 0) return fail("commitment_array_masked");
            qm[36].img = 2305843009213693951ull;
            if (orc_commitment_array_masked(in.data(), in.size(), pub.data(), nb, r.data(), pm.data(), 100, qm.data(), 37, rl, &inner, alls, rh, roots.data(), fin.data(),
                                            fm.data()) != -1) return fail("non-canonical mask limb");
        }
        orc_circuit_free(c);
    }
    {   // tiny and ragged shapes: one-gate layers, single-entry tables
        for (int lg = 0; lg < 4; ++lg) {
            orc_circuit *c = orc_circuit_randomize(3, lg, 5 + lg);
            if (orc_prove_gkr(c, buf.data(), (int64_t) buf.size(), &st) <= 0 || !st.verified) return fail("tiny prove_gkr");
            if (orc_prove_fs(c, buf.data(), (int64_t) buf.size(), &st) <= 0 || !st.verified) return fail("tiny prove_fs");
            orc_circuit_free(c);
        }
    }
    if (argc > 1) {   // the reference's data file: loader, levelisation, subsetInit, two replicated blocks
        orc_circuit *c = orc_circuit_from_pws(argv[1], 2, 1);
        if (!c) return fail("from_pws");
        if (orc_prove_gkr(c, buf.data(), (int64_t) buf.size(), &st) <= 0 || !st.verified) return fail("pws prove_gkr");
        uint64_t h[2];
        orc_circuit_hash(c, h);
        orc_circuit_free(c);
    }
    {   // primitives
        orc_F a = {1234567890123456789ull, 987654321987654321ull}, b = {2305843009213693950ull, 1}, o, t;
        orc_f_mul(&a, &b, &o); orc_f_inv(&a, &t); orc_f_mul(&a, &t, &o);
        if (o.real != 1 || o.img != 0) return fail("inv");
        std::vector<orc_F> c8(8), ev(32), back(32);
        for (int i = 0; i < 8; ++i) c8[i] = {(uint64_t) i + 1, (uint64_t) 2 * i + 3};
        orc_fft(c8.data(), 8, 32, ev.data());
        if (ev[0].real != 36 || ev[0].img != 80) return fail("fft");
        orc_ifft(ev.data(), 32, back.data());
        for (int i = 0; i < 8; ++i) if (back[i].real != c8[i].real || back[i].img != c8[i].img) return fail("ifft");
        std::vector<orc_F> rr(5), tab(32);
        orc_f_random_seq(3396, 5, rr.data());
        orc_F one = {1, 0};
        orc_beta_table(rr.data(), 5, &one, tab.data());
        uint8_t z[64] = {0}, d[32];
        orc_sha3_256_64(z, d);
        if (d[0] != 0x07 || d[1] != 0x0f) return fail("sha3");
    }
    {   // fft_gkr at a small lg: the seeded entry, the tape entry on the same draws (same bytes), an edge-limb tape, and the tape entry's refusals
        const int lg = 3, nt = orc_fft_gkr_draws(lg);
        const uint64_t P = 2305843009213693951ull, edge[5] = {0, 1, 2, P - 2, P - 1};
        const int64_t want = 16 * (64 + 3 * (2 * lg * lg + 2 * lg + 6) + 2 + 2 * lg);
        std::vector<uint8_t> a(want), b(want);
        int ok = 0;
        if (orc_fft_gkr(lg, 3396, a.data(), want, nullptr, &ok) != want || !ok) return fail("fft_gkr seeded");
        std::vector<orc_F> tape(nt);
        orc_f_random_seq(3396, nt, tape.data());
        if (orc_fft_gkr_tape(lg, &tape[0].real, nt, b.data(), want, &ok) != want || !ok || memcmp(a.data(), b.data(), (size_t) want)) return fail("fft_gkr tape");
        for (int i = 0; i < nt; ++i) tape[i] = {edge[(7 * i + 3) % 5], edge[(3 * i + 1) % 5]};
        if (orc_fft_gkr_tape(lg, &tape[0].real, nt, b.data(), want, &ok) != want || !ok) return fail("fft_gkr edge tape");
        if (orc_fft_gkr_tape(lg, &tape[0].real, nt - 1, b.data(), want, &ok) != -3) return fail("fft_gkr tape length");
        if (orc_fft_gkr_tape(lg, &tape[0].real, nt, b.data(), want - 1, &ok) != -1) return fail("fft_gkr capacity");
        tape[nt - 1].img = P;
        if (orc_fft_gkr_tape(lg, &tape[0].real, nt, b.data(), want, &ok) != -4) return fail("fft_gkr non-canonical limb");
    }
    {   // the GKR prover on a caller's tape: the seeded draws (same bytes as orc_prove_gkr), an edge-limb tape, and the entry's refusals
        orc_circuit *c = orc_circuit_randomize(4, 6, 3);
        if (!c) return fail("randomize for the tape entry");
        const uint64_t P = 2305843009213693951ull, edge[8] = {0, 1, 2, (1ull << 31) - 1, (1ull << 31) + 1, 1ull << 60, P - 2, P - 1};
        const int64_t nt = orc_gkr_draws(c);
        const int64_t want = orc_prove_gkr(c, buf.data(), (int64_t) buf.size(), &st);
        if (nt <= 0 || want <= 0 || !st.verified) return fail("prove_gkr before the tape entry");
        std::vector<uint8_t> b(want);
        std::vector<orc_F> tape(nt);
        orc_f_random_seq(3396, (int) nt, tape.data());
        if (orc_prove_gkr_tape(c, &tape[0].real, nt, b.data(), want, &st) != want || !st.verified || memcmp(buf.data(), b.data(), (size_t) want)) return fail("prove_gkr_tape seeded");
        for (int64_t i = 0; i < nt; ++i) tape[i] = {edge[(7 * i + 3) % 8], edge[(3 * i + 1) % 8]};
        if (orc_prove_gkr_tape(c, &tape[0].real, nt, b.data(), want, &st) != want || !st.verified) return fail("prove_gkr_tape edge tape");
        if (orc_prove_gkr_tape(c, &tape[0].real, nt - 1, b.data(), want, &st) != -3) return fail("prove_gkr_tape length");
        if (orc_prove_gkr_tape(c, nullptr, nt, b.data(), want, &st) != -3) return fail("prove_gkr_tape null tape");
        if (orc_prove_gkr_tape(c, &tape[0].real, nt, b.data(), want - 1, &st) != -1) return fail("prove_gkr_tape capacity");
        tape[nt - 1].img = P;
        if (orc_prove_gkr_tape(c, &tape[0].real, nt, b.data(), want, &st) != -4) return fail("prove_gkr_tape non-canonical limb");
        orc_circuit_free(c);
    }
    puts("oracle_asan ok");
    return 0;
}
