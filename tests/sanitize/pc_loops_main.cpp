// TEST INFRASTRUCTURE ONLY.  Sanitizer leg of the commitment verifier's two factored loops (vphost.h: vph_pc_public_evals_host,
// vph_pc_opening_digests_host): the host library's sources compiled with -fsanitize=address,undefined (tests/test_pc_verifier_loops_host.py builds
// tests/sanitize/_build/pc_loops_asan; libvpgpu.so is linked but no device call is made).  The digest loop runs over the openings of the committed
// record exactly as long as they are, and must refuse a truncated and an over-long block without reading either; the public evaluation runs in
// its three forms (point, one-transform, expanded vector), which must agree.
#include "../../virgo-plus_amd/host/vphost.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fail(const char *what, long at = -1) { fprintf(stderr, "pc_loops_asan: %s (%ld)\n", what, at); return 1; }
static std::vector<uint8_t> slurp(const char *p) {
    std::vector<uint8_t> v;
    FILE *f = fopen(p, "rb");
    if (!f) return v;
    uint8_t b[4096]; size_t n;
    while ((n = fread(b, 1, sizeof b, f)) > 0) v.insert(v.end(), b, b + n);
    fclose(f);
    return v;
}

// argv: record.bin  offset of its openings  n  leaf0 ...
int main(int argc, char **argv) {
    if (argc < 5) return fail("usage");
    const std::vector<uint8_t> rec = slurp(argv[1]);
    const long at = atol(argv[2]);
    const int n = atoi(argv[3]), nq = argc - 4;
    std::vector<uint64_t> leaf0;
    for (int i = 4; i < argc; ++i) leaf0.push_back(strtoull(argv[i], nullptr, 10));
    const uint64_t nb = vph_pc_query_answer_bytes(n, nq);
    if (at <= 0 || (uint64_t) at + nb != rec.size()) return fail("the openings do not end the record", at);
    // exact-size heap copies: one byte read past either end is a report
    std::vector<uint8_t> ans(rec.begin() + at, rec.end()), out((size_t) nq * (n - 4) * 64), out2(out.size());
    if (vph_pc_opening_digests_host(n, nq, leaf0.data(), ans.data(), ans.size(), out.data()) != 0) return fail("digest loop refused the record's openings");
    {
        size_t o = 0, i = 0;
        for (int q = 0; q < nq; ++q)
            for (int k = 0; k < n - 4; ++k, ++i) {
                const size_t plen = (size_t) (k < 2 ? n - 1 : n - 2 - (k - 2));
                if (memcmp(&out[64 * i], &ans[o + 2080 + 32 * (plen - 1)], 32) != 0) return fail("leaf digest differs from path[depth]", (long) i);
                o += 2080 + 32 * plen;
            }
    }
    {
        std::vector<uint8_t> cut(ans.begin(), ans.end() - 1), longer(ans);
        longer.push_back(0);
        if (vph_pc_opening_digests_host(n, nq, leaf0.data(), cut.data(), cut.size(), out2.data()) == 0) return fail("truncated answer accepted");
        if (vph_pc_opening_digests_host(n, nq, leaf0.data(), longer.data(), longer.size(), out2.data()) == 0) return fail("over-long answer accepted");
        if (vph_pc_opening_digests_host(n, nq - 1, leaf0.data(), ans.data(), ans.size(), out2.data()) == 0 && nq > 1) return fail("answer of another query count accepted");
    }
    // public evaluation: a point from the record's own bytes (limbs reduced below p), its three forms
    const uint64_t P = 2305843009213693951ull;
    std::vector<uint64_t> point(2 * (size_t) n);
    for (size_t i = 0; i < point.size(); ++i) { uint64_t w; memcpy(&w, &rec[64 + 8 * i], 8); point[i] = w % P; }
    std::vector<uint64_t> a((size_t) nq * 256), b(a.size()), c(a.size());
    if (vph_pc_public_evals_host(n, point.data(), nullptr, 0, nq, leaf0.data(), a.data()) != 0) return fail("public evaluation refused");
    if (vph_pc_public_evals_host(n, point.data(), nullptr, 1, nq, leaf0.data(), b.data()) != 0 || a != b) return fail("one-transform form differs");
    {
        // the expanded table through the same export: eq(point, .) by doubling, in exact-size storage
        std::vector<uint64_t> tab(2ull << n, 0);
        auto mulp = [&](uint64_t x, uint64_t y) { return (uint64_t) (((unsigned __int128) x * y) % P); };
        auto fmul = [&](const uint64_t *x, const uint64_t *y, uint64_t *o) {
            const uint64_t re = (mulp(x[0], y[0]) + P - mulp(x[1], y[1])) % P, im = (mulp(x[0], y[1]) + mulp(x[1], y[0])) % P;
            o[0] = re; o[1] = im;
        };
        tab[0] = 1;
        for (int k = 0; k < n; ++k)
            for (uint64_t j = 0; j < (1ull << k); ++j) {
                uint64_t t[2];
                fmul(&tab[2 * j], &point[2 * k], t);
                tab[2 * (j | (1ull << k))] = t[0]; tab[2 * (j | (1ull << k)) + 1] = t[1];
                tab[2 * j] = (tab[2 * j] + P - t[0]) % P; tab[2 * j + 1] = (tab[2 * j + 1] + P - t[1]) % P;
            }
        if (vph_pc_public_evals_host(n, nullptr, tab.data(), 0, nq, leaf0.data(), c.data()) != 0 || a != c) return fail("vector form differs");
    }
    {
        std::vector<uint64_t> bad(leaf0);
        bad[0] = 1ull << (n - 2);
        if (vph_pc_public_evals_host(n, point.data(), nullptr, 0, nq, bad.data(), b.data()) == 0) return fail("leaf out of range accepted");
        point[1] = P;
        if (vph_pc_public_evals_host(n, point.data(), nullptr, 0, nq, leaf0.data(), b.data()) == 0) return fail("non-canonical point accepted");
    }
    puts("pc_loops_asan ok");
    return 0;
}
