// TEST INFRASTRUCTURE ONLY.  Sanitizer leg of the commitment-level verifier (vphost.h: vph_verify_commitment, vph_pc_mask_evals_host): the host library's
// sources compiled with -fsanitize=address,undefined (tests/test_masked_verifier_host.py builds tests/sanitize/_build/masked_verify_asan; libvpgpu.so is
// linked but no device call is made).  The case file holds one complete masked proof and a second answer block with one changed mask pair; every array is
// copied into exact-size heap storage, so one byte read past an end is a report.  Accept, two rejects by name, one malformed call.
#include "../../virgo-plus_amd/host/vphost.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int fail(const char *what, const char *why = "") { fprintf(stderr, "masked_verify_asan: %s (%s)\n", what, why); return 1; }
static std::vector<uint8_t> slurp(const char *p) {
    std::vector<uint8_t> v;
    FILE *f = fopen(p, "rb");
    if (!f) return v;
    uint8_t b[4096]; size_t n;
    while ((n = fread(b, 1, sizeof b, f)) > 0) v.insert(v.end(), b, b + n);
    fclose(f);
    return v;
}

// argv: case.bin = i32 n | i32 reps | u64 ms | u64 n_pub_mask | u64 answer bytes | pub[2^n] | pub_mask | claim | all_sum[65] | r[n - 6] | final_code[2048] |
// final_mask[32] | leaf0[reps] (u64) | root_l | root_h | fri_roots | answer | answer with a changed mask pair
int main(int argc, char **argv) {
    if (argc != 2) return fail("usage");
    const std::vector<uint8_t> file = slurp(argv[1]);
    size_t at = 0;
    bool short_file = false;
    auto take = [&](size_t bytes) {
        std::vector<uint8_t> v;
        if (bytes > file.size() - at) { short_file = true; return v; }
        v.assign(file.begin() + at, file.begin() + at + bytes);
        at += bytes;
        return v;
    };
    auto words = [&](size_t count) {
        const std::vector<uint8_t> b = take(8 * count);
        std::vector<uint64_t> w(b.size() / 8);
        if (!b.empty()) memcpy(w.data(), b.data(), b.size());
        return w;
    };
    if (file.size() < 32) return fail("case file too short");
    int32_t head[2];
    memcpy(head, file.data(), 8); at = 8;
    const int n = head[0], reps = head[1];
    const std::vector<uint64_t> lens = words(3);
    if (n < 7 || n > 12 || reps < 1 || reps > 64 || lens.size() != 3 || lens[1] > lens[0] || lens[0] > 4096) return fail("case header");
    const uint64_t ms = lens[0], n_pm = lens[1], nb = lens[2];
    if (nb != vph_pc_query_answer_bytes(n, reps)) return fail("answer size");
    const std::vector<uint64_t> pub = words(2ull << n), pm = words(2 * n_pm), claim = words(2), sums = words(130), r = words(2 * (size_t) (n - 6)), fc = words(4096),
                                fm = words(64), leaf0 = words((size_t) reps);
    const std::vector<uint8_t> root_l = take(32), root_h = take(32), roots = take(32 * (size_t) (n - 6)), ans = take(nb), ans_bad = take(nb);
    if (short_file || at != file.size()) return fail("case file size");
    char err[256] = "";
    auto run = [&](const std::vector<uint64_t> &mask, uint64_t ms_, const std::vector<uint8_t> &answer) {
        err[0] = 0;
        return vph_verify_commitment(n, nullptr, pub.data(), mask.data(), mask.size() / 2, ms_, claim.data(), root_l.data(), root_h.data(), sums.data(), r.data(), roots.data(),
                                     fc.data(), fm.data(), reps, leaf0.data(), answer.data(), answer.size(), -1, err, (int) sizeof err);
    };
    if (run(pm, ms, ans) != 0) return fail("the proof was not accepted", err);
    std::vector<uint64_t> pm2(pm);
    pm2[0] ^= 1;
    if (run(pm2, ms, ans) != 1 || std::string(err) != "Fri msk check consistency 0 round fail") return fail("a changed public mask", err);
    if (run(pm, ms, ans_bad) != 1 || std::string(err) != "commitment: Merkle opening rejected") return fail("a changed mask pair", err);
    std::vector<uint8_t> cut(ans.begin(), ans.end() - 1);
    if (run(pm, ms, cut) != -1) return fail("a truncated answer", err);
    if (run(pm, 3 * ms, ans) != -1) return fail("ms that is no power of two", err);
    // the mask row on its own: a full-length and a one-element mask, exact-size output
    std::vector<uint64_t> out(4 * (size_t) reps);
    if (vph_pc_mask_evals_host(n, pm.data(), n_pm, ms, reps, leaf0.data(), out.data()) != 0) return fail("mask row refused");
    if (vph_pc_mask_evals_host(n, pm.data(), 1, ms, reps, leaf0.data(), out.data()) != 0) return fail("one-element mask row refused");
    if (vph_pc_mask_evals_host(n, pm.data(), ms + 1, ms, reps, leaf0.data(), out.data()) == 0) return fail("over-long mask accepted");
    puts("masked_verify_asan ok");
    return 0;
}
