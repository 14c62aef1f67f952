// TEST INFRASTRUCTURE ONLY.  Sanitizer leg of the non-interactive commitment proof's parser and verifier: virgo-plus_amd/host/*.cpp compiled with
// -fsanitize=address,undefined (tests/test_pc_fs_host.py builds tests/sanitize/_build/pc_fs_asan; libvpgpu.so is linked but no device call is made) and
// driven through vph_verify_commitment_fs / vph_commitment_fs_challenges on the host: one good proof, then proofs damaged in every way a reader can be
// led astray — each heap copy is exactly as long as the proof it holds, so a read past the end is a report.
#include "../../virgo-plus_amd/host/vphost.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fail(const char *what, long at = -1) { fprintf(stderr, "pc_fs_asan: %s (%ld)\n", what, at); return 1; }
static std::vector<uint8_t> slurp(const char *p) {
    std::vector<uint8_t> v;
    FILE *f = fopen(p, "rb");
    if (!f) return v;
    uint8_t b[4096]; size_t n;
    while ((n = fread(b, 1, sizeof b, f)) > 0) v.insert(v.end(), b, b + n);
    fclose(f);
    return v;
}
// the verdict on an exact-size heap copy; the derivation runs on the same bytes
static int verdict(const std::vector<uint8_t> &p) {
    uint8_t *q = static_cast<uint8_t *>(malloc(p.size() ? p.size() : 1));
    if (!p.empty()) memcpy(q, p.data(), p.size());
    char err[256] = {0};
    const int rc = vph_verify_commitment_fs(q, p.size(), -1, err, sizeof err);
    std::vector<uint64_t> r(2 * 32), lf(4096);
    const int rd = vph_commitment_fs_challenges(q, p.size(), r.data(), lf.data());
    free(q);
    if ((rc == -1) != (rd == -1)) { fprintf(stderr, "pc_fs_asan: the derivation and the verifier disagree on what is well-formed\n"); return 99; }
    return rc;
}

// argv: a good proof (tests/pc_fs_ref.py)
int main(int argc, char **argv) {
    if (argc < 2) return fail("usage");
    const std::vector<uint8_t> good = slurp(argv[1]);
    if (good.size() < 32) return fail("no proof");
    if (verdict(good) != 0) return fail("the good proof is not accepted");
    uint32_t h32[4]; uint64_t h64[2];
    memcpy(h32, good.data(), 16); memcpy(h64, good.data() + 16, 16);
    const size_t n = h32[2], reps = h32[3], n_pub = h64[1];
    const size_t fixed = 32 + 16 * (n + n_pub + 1) + 64 + 65 * 16 + 32 * (n - 6) + (2048 + 32) * 16;
    if (fixed >= good.size()) return fail("the proof is shorter than its fixed sections");
    // one bit changed: every byte of the header, a stride through the fixed sections, a stride through the answer
    std::vector<size_t> at;
    for (size_t i = 0; i < 32; ++i) at.push_back(i);
    for (size_t i = 32; i < fixed; i += 61) at.push_back(i);
    for (size_t i = fixed; i < good.size(); i += (good.size() - fixed) / 40 + 1) at.push_back(i);
    at.push_back(good.size() - 1);
    for (size_t i : at) {
        std::vector<uint8_t> p = good;
        p[i] ^= 0x10;
        const int rc = verdict(p);
        if (rc != 1 && rc != -1) return fail("a changed byte is not rejected", (long) i);
    }
    // truncated everywhere a section ends, around those ends, and by single bytes; extended
    std::vector<size_t> cut = {0, 1, 15, 16, 31, 32, 33, fixed - 1, fixed, fixed + 1, good.size() - 1, good.size() - 32};
    size_t o = 32;
    for (size_t len : {16 * n, 16 * n_pub, (size_t) 16, (size_t) 32, (size_t) 32, (size_t) 65 * 16, 32 * (n - 6), (size_t) 2048 * 16, (size_t) 32 * 16}) {
        o += len;
        cut.push_back(o - 1); cut.push_back(o); cut.push_back(o + 7);
    }
    for (size_t len : cut) {
        if (len >= good.size()) continue;
        if (verdict(std::vector<uint8_t>(good.begin(), good.begin() + len)) != -1) return fail("a truncated proof is not malformed", (long) len);
    }
    for (size_t extra : {(size_t) 1, (size_t) 32, (size_t) 4096}) {
        std::vector<uint8_t> p = good;
        p.resize(good.size() + extra, 0);
        if (verdict(p) != -1) return fail("an extended proof is not malformed", (long) extra);
    }
    // header fields at their extremes: a size computed from them must not be trusted before it is bounded
    const uint32_t n_vals[] = {0, 1, 6, 31, 32, 63, 64, 0x7fffffffu, 0xffffffffu}, reps_vals[] = {0, 4097, 0x7fffffffu, 0xffffffffu};
    const uint64_t ms_vals[] = {0, 2, 3, 4, 12, 1ull << 17, 1ull << 32, 1ull << 63, ~0ull}, pub_vals[] = {h64[0] + 1, 1ull << 16, 1ull << 32, 1ull << 60, ~0ull};
    auto with = [&](int word, uint64_t v) {
        std::vector<uint8_t> p = good;
        if (word < 4) { const uint32_t x = (uint32_t) v; memcpy(p.data() + 4 * word, &x, 4); } else memcpy(p.data() + 16 + 8 * (word - 4), &v, 8);
        return verdict(p);
    };
    for (uint32_t v : n_vals) if (with(2, v) != -1) return fail("n", (long) v);
    for (uint32_t v : reps_vals) if (with(3, v) != -1) return fail("reps", (long) v);
    for (uint64_t v : ms_vals) if (with(4, v) != -1) return fail("ms", (long) v);
    for (uint64_t v : pub_vals) if (with(5, v) != -1) return fail("n_pub", (long) v);
    if (with(0, 0x52465056u) != -1 || with(1, 2) != -1 || with(1, 0) != -1) return fail("magic / version");
    // a non-canonical limb in every section of field elements
    const struct { size_t len; bool elems; } secs[] = {{16 * n, true}, {16 * n_pub, true}, {16, true}, {64, false}, {65 * 16, true}, {32 * (n - 6), false}, {2048 * 16, true}, {32 * 16, true}};
    size_t sec = 32;
    for (const auto &e : secs) {
        if (e.elems && e.len) {
            std::vector<uint8_t> p = good;
            const uint64_t big = (1ull << 61) - 1;
            memcpy(p.data() + sec + e.len - 8, &big, 8);
            if (verdict(p) != -1) return fail("a limb equal to p is not malformed", (long) sec);
        }
        sec += e.len;
    }
    (void) reps;
    printf("pc_fs_asan ok\n");
    return 0;
}
