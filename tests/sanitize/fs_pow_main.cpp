// TEST INFRASTRUCTURE ONLY.  Sanitizer leg of the proof of work of the non-interactive proofs: virgo-plus_amd/host/*.cpp compiled with
// -fsanitize=address,undefined (tests/test_fs_pow_host.py builds tests/sanitize/_build/fs_pow_asan; libvpgpu.so is linked but no device call is made) and
// driven through vph_verify_commitment_fs_min / vph_commitment_fs_challenges / vph_fs_pow / vph_fs_grind_host on the host: one good version-2 proof, then every
// truncation class of the 48-byte header, the two new fields at their extremes and changed bytes — each heap copy is exactly as long as the proof it holds,
// so a read past the end is a report.
#include "../../virgo-plus_amd/host/vphost.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fail(const char *what, long at = -1) { fprintf(stderr, "fs_pow_asan: %s (%ld)\n", what, at); return 1; }
static std::vector<uint8_t> slurp(const char *p) {
    std::vector<uint8_t> v;
    FILE *f = fopen(p, "rb");
    if (!f) return v;
    uint8_t b[4096]; size_t n;
    while ((n = fread(b, 1, sizeof b, f)) > 0) v.insert(v.end(), b, b + n);
    fclose(f);
    return v;
}
// the verdict on an exact-size heap copy; the derivation and the header reader run on the same bytes
static int verdict(const std::vector<uint8_t> &p, int min_bits = 0) {
    uint8_t *q = static_cast<uint8_t *>(malloc(p.size() ? p.size() : 1));
    if (!p.empty()) memcpy(q, p.data(), p.size());
    char err[256] = {0};
    const int rc = vph_verify_commitment_fs_min(q, p.size(), -1, min_bits, err, sizeof err);
    std::vector<uint64_t> r(2 * 32), lf(4096);
    const int rd = vph_commitment_fs_challenges(q, p.size(), r.data(), lf.data());
    uint64_t bits = 0, nonce = 0;
    const int rp = vph_fs_pow(q, p.size(), &bits, &nonce);
    free(q);
    if ((rc == -1) != (rd == -1)) { fprintf(stderr, "fs_pow_asan: the derivation and the verifier disagree on what is well-formed\n"); return 99; }
    if (rc != -1 && rp != 0) { fprintf(stderr, "fs_pow_asan: vph_fs_pow refuses the header of a well-formed proof\n"); return 99; }
    return rc;
}

// argv: a good version-2 commitment proof (tests/fs_pow_ref.py)
int main(int argc, char **argv) {
    if (argc < 2) return fail("usage");
    const std::vector<uint8_t> good = slurp(argv[1]);
    if (good.size() < 48) return fail("no proof");
    uint32_t h32[4]; uint64_t h64[4];
    memcpy(h32, good.data(), 16); memcpy(h64, good.data() + 16, 32);
    if (h32[1] != 2) return fail("not a version-2 proof");
    const uint64_t bits = h64[2];
    if (verdict(good) != 0 || verdict(good, (int) bits) != 0) return fail("the good proof is not accepted");
    if (verdict(good, (int) bits + 1) != 1) return fail("a demand above the proof's bits is not rejected");
    // every length of the 48-byte header and one byte behind it
    for (size_t len = 0; len <= 49; ++len)
        if (verdict(std::vector<uint8_t>(good.begin(), good.begin() + len)) != -1) return fail("a truncated header is not malformed", (long) len);
    if (verdict(std::vector<uint8_t>(good.begin(), good.end() - 1)) != -1 || verdict(std::vector<uint8_t>(good.begin(), good.end() - 16)) != -1)
        return fail("a truncated proof is not malformed");
    { std::vector<uint8_t> p = good; p.resize(good.size() + 16, 0); if (verdict(p) != -1) return fail("an extended proof is not malformed"); }
    // the two fields at their extremes: pow_bits outside 1 .. 48 is malformed; inside, another value is a verdict (the work is met or not); any nonce is
    auto with = [&](int word, uint64_t v, int min_bits = 0) {
        std::vector<uint8_t> p = good;
        memcpy(p.data() + 32 + 8 * word, &v, 8);
        return verdict(p, min_bits);
    };
    const uint64_t bad_bits[] = {0, 49, 64, 65, 1ull << 31, 1ull << 32, 1ull << 63, ~0ull};
    for (uint64_t v : bad_bits) if (with(0, v) != -1) return fail("pow_bits", (long) v);
    for (uint64_t v = 1; v <= 48; ++v) {
        if (v == bits) continue;
        const int rc = with(0, v);
        if (rc != 1) return fail("changed pow_bits with the old answers is not rejected", (long) v);
    }
    const uint64_t nonces[] = {0, 1, 1ull << 32, 1ull << 63, ~0ull, h64[3] + 1, h64[3] - 1};
    for (uint64_t v : nonces) {
        if (v == h64[3]) continue;
        if (with(1, v) != 1) return fail("a changed nonce is not rejected", (long) v);
    }
    // the demand at its extremes
    for (int m : {-1, 0, 1, (int) bits}) if (verdict(good, m) != 0) return fail("min_pow_bits", m);
    for (int m : {(int) bits + 1, 48, 49, 0x7fffffff}) if (verdict(good, m) != 1) return fail("min_pow_bits", m);
    // the version word against the body: a version-2 body under version 1, and a version-1 body (the 16 bytes cut out) under version 2
    { std::vector<uint8_t> p = good; p[4] = 1; if (verdict(p) != -1) return fail("a version-2 body under a version-1 header"); }
    { std::vector<uint8_t> p = good; p.erase(p.begin() + 32, p.begin() + 48); if (verdict(p) != -1) return fail("a version-1 body under a version-2 header"); }
    { std::vector<uint8_t> p = good; p.erase(p.begin() + 32, p.begin() + 48); p[4] = 1; const int rc = verdict(p); if (rc != 1) return fail("the body without its work, as version 1, is not rejected", rc); }
    // one bit changed: every byte of the header, a stride through the rest
    std::vector<size_t> at;
    for (size_t i = 0; i < 48; ++i) at.push_back(i);
    for (size_t i = 48; i < good.size(); i += good.size() / 97 + 1) at.push_back(i);
    at.push_back(good.size() - 1);
    for (size_t i : at) {
        std::vector<uint8_t> p = good;
        p[i] ^= 0x10;
        const int rc = verdict(p);
        if (rc != 1 && rc != -1) return fail("a changed byte is not rejected", (long) i);
    }
    // the host search at the edges of its ranges
    uint8_t st[32], out[32];
    for (int i = 0; i < 32; ++i) st[i] = (uint8_t) (17 * i + 3);
    uint64_t nonce = 0;
    if (vph_fs_grind_host(st, 6, 0, 1ull << 20, &nonce, out) != 0) return fail("the search finds nothing");
    const uint64_t h = nonce;
    if (h > 0 && vph_fs_grind_host(st, 6, 0, h, &nonce, out) != -5) return fail("max_tries = h finds something");
    if (vph_fs_grind_host(st, 6, 0, h + 1, &nonce, out) != 0 || nonce != h) return fail("max_tries = h + 1 does not find h");
    if (vph_fs_grind_host(st, 3, ~0ull - 99, 100, &nonce, out) != 0 && vph_fs_grind_host(st, 3, ~0ull - 99, 100, &nonce, out) != -5) return fail("the last hundred nonces");
    if (vph_fs_grind_host(st, 3, ~0ull - 99, 101, &nonce, out) != -1 || vph_fs_grind_host(st, 3, ~0ull, 2, &nonce, out) != -1) return fail("a range past 2^64 is taken");
    if (vph_fs_grind_host(st, 0, 0, 8, &nonce, out) != -1 || vph_fs_grind_host(st, 49, 0, 8, &nonce, out) != -1 || vph_fs_grind_host(st, 64, 0, 8, &nonce, out) != -1 ||
        vph_fs_grind_host(st, 4, 0, 0, &nonce, out) != -1 || vph_fs_grind_host(nullptr, 4, 0, 8, &nonce, out) != -1 || vph_fs_grind_host(st, 4, 0, 8, nullptr, out) != -1 ||
        vph_fs_grind_host(st, 4, 0, 8, &nonce, nullptr) != -1)
        return fail("a refusal of the search");
    if (vph_fs_grind_host(st, 48, 0, 4, &nonce, out) != -5 && vph_fs_grind_host(st, 48, 0, 4, &nonce, out) != 0) return fail("48 bits");
    printf("fs_pow_asan ok\n");
    return 0;
}
