// TEST INFRASTRUCTURE ONLY.  Sanitizer leg of the joined proof's parser and verifier: virgo-plus_amd/host/*.cpp compiled with -fsanitize=address,undefined
// (tests/test_full_fs_host.py builds tests/sanitize/_build/full_fs_asan; libvpgpu.so is linked but no device call is made) and driven through
// vph_verify_full_fs on the host: one good proof, then proofs damaged in every way a reader can be led astray — each heap copy is exactly as long as the proof it
// holds, so a read past the end is a report.  argv: the fixture's circuit (layers, log_size, seed of vph_circuit_randomize), the proof, the offset of its GKR
// section, the offset of root_h (tests/full_fs_ref.py: sections).
#include "../../virgo-plus_amd/host/vphost.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static vph_circuit *circ = nullptr;
static int fail(const char *what, long at = -1) { fprintf(stderr, "full_fs_asan: %s (%ld)\n", what, at); return 1; }
static std::vector<uint8_t> slurp(const char *p) {
    std::vector<uint8_t> v;
    FILE *f = fopen(p, "rb");
    if (!f) return v;
    uint8_t b[4096]; size_t n;
    while ((n = fread(b, 1, sizeof b, f)) > 0) v.insert(v.end(), b, b + n);
    fclose(f);
    return v;
}
static int verdict(const std::vector<uint8_t> &p) {
    uint8_t *q = static_cast<uint8_t *>(malloc(p.size() ? p.size() : 1));
    if (!p.empty()) memcpy(q, p.data(), p.size());
    char err[256] = {0};
    const int rc = vph_verify_full_fs(circ, q, p.size(), -1, nullptr, err, sizeof err);
    free(q);
    return rc;
}

int main(int argc, char **argv) {
    if (argc < 7) return fail("usage");
    circ = vph_circuit_randomize(atoi(argv[1]), atoi(argv[2]), atol(argv[3]));
    if (!circ) return fail("no circuit");
    const std::vector<uint8_t> good = slurp(argv[4]);
    const size_t gkr = (size_t) atol(argv[5]), root_h = (size_t) atol(argv[6]);
    if (good.size() < 32 || gkr >= root_h || root_h >= good.size()) return fail("no proof");
    if (verdict(good) != 0) return fail("the good proof is not accepted");
    // one bit changed: every byte of the header, a stride through the GKR part and through what follows it
    std::vector<size_t> at;
    for (size_t i = 0; i < 32; ++i) at.push_back(i);
    for (size_t i = 32; i < root_h; i += 37) at.push_back(i);
    for (size_t i = root_h; i < good.size(); i += (good.size() - root_h) / 60 + 1) at.push_back(i);
    at.push_back(good.size() - 1);
    for (size_t i : at) {
        std::vector<uint8_t> p = good;
        p[i] ^= 0x10;
        const int rc = verdict(p);
        if (rc != 1 && rc != -1) return fail("a changed byte is not rejected", (long) i);
    }
    // truncated: around every boundary this program knows, a stride through the GKR part (the reader runs out inside a sumcheck), by single bytes; extended
    std::vector<size_t> cut = {0, 1, 15, 16, 31, 32, 33, gkr - 1, gkr, gkr + 1, gkr + 15, gkr + 16, root_h - 1, root_h, root_h + 1, root_h + 31, root_h + 32, root_h + 47, root_h + 48,
                               good.size() - 1, good.size() - 32};
    for (size_t i = gkr; i < root_h; i += 101) cut.push_back(i);
    for (size_t i = root_h; i < good.size(); i += 997) cut.push_back(i);
    for (size_t len : cut) {
        if (len >= good.size()) continue;
        if (verdict(std::vector<uint8_t>(good.begin(), good.begin() + len)) != -1) return fail("a truncated proof is not malformed", (long) len);
    }
    for (size_t extra : {(size_t) 1, (size_t) 16, (size_t) 4096}) {
        std::vector<uint8_t> p = good;
        p.resize(good.size() + extra, 0);
        if (verdict(p) != -1) return fail("an extended proof is not malformed", (long) extra);
    }
    // header fields at their extremes: a size computed from them must not be trusted before it is bounded
    uint64_t h64[2];
    memcpy(h64, good.data() + 16, 16);
    const uint32_t n_vals[] = {0, 1, 6, 8, 30, 31, 32, 0x7fffffffu, 0xffffffffu}, reps_vals[] = {0, 4097, 0x7fffffffu, 0xffffffffu};
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
    if (with(0, 0x46435056u) != -1 || with(1, 2) != -1 || with(1, 0) != -1) return fail("magic / version");
    // a non-canonical limb in the GKR part and in every later section of field elements
    const uint64_t big = (1ull << 61) - 1;
    for (size_t off : {gkr + 8, root_h - 8, root_h + 32, root_h + 48 + 64 * 16, root_h + 48 + 65 * 16 + 16}) {
        std::vector<uint8_t> p = good;
        memcpy(p.data() + off, &big, 8);
        if (verdict(p) != -1) return fail("a limb equal to p is not malformed", (long) off);
    }
    vph_circuit_free(circ);
    printf("full_fs_asan ok\n");
    return 0;
}
