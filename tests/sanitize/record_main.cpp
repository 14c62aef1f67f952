// TEST INFRASTRUCTURE ONLY.  Sanitizer leg of the record replay (vphost.h: vph_verify_full_record): the host library's sources compiled with
// -fsanitize=address,undefined (tests/test_query_record_host.py builds tests/sanitize/_build/record_asan; libvpgpu.so is linked but no device
// call is made) and driven over the committed record of a complete-protocol run: accepted as it is; rejected with one byte flipped at each of
// the offsets given, truncated by one byte, extended by one byte, cut at every section boundary, and empty — never read out of bounds.
#include "../../virgo-plus_amd/host/vphost.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fail(const char *what, long at = -1) { fprintf(stderr, "record_asan: %s (%ld)\n", what, at); return 1; }
static std::vector<uint8_t> slurp(const char *p) {
    std::vector<uint8_t> v;
    FILE *f = fopen(p, "rb");
    if (!f) return v;
    uint8_t b[4096]; size_t n;
    while ((n = fread(b, 1, sizeof b, f)) > 0) v.insert(v.end(), b, b + n);
    fclose(f);
    return v;
}

// argv: circuit.bin (u64 n_layers | sizes | u64 gates | ty i32[] | l i32[] | u u64[] | v u64[] | c u64[2 x] | is_assert u8[])  record.bin  offset ...
int main(int argc, char **argv) {
    if (argc < 3) return fail("usage");
    const std::vector<uint8_t> cb = slurp(argv[1]);
    std::vector<uint8_t> rec = slurp(argv[2]);
    if (cb.size() < 16 || rec.size() < 1000) return fail("inputs missing");
    size_t at = 0;
    auto take = [&](void *dst, size_t k) { if (at + k > cb.size()) { fprintf(stderr, "record_asan: circuit file short\n"); exit(1); } memcpy(dst, cb.data() + at, k); at += k; };
    uint64_t nl = 0, G = 0;
    take(&nl, 8);
    if (nl < 2 || nl > 64) return fail("circuit file: layers");
    std::vector<uint64_t> sizes(nl);
    take(sizes.data(), 8 * nl);
    take(&G, 8);
    if (G > (1u << 24)) return fail("circuit file: gates");
    std::vector<int32_t> ty(G), l(G); std::vector<uint64_t> u(G), v(G), cp(2 * G); std::vector<uint8_t> as(G);
    take(ty.data(), 4 * G); take(l.data(), 4 * G); take(u.data(), 8 * G); take(v.data(), 8 * G); take(cp.data(), 16 * G); take(as.data(), G);
    vph_circuit *c = vph_circuit_custom((int) nl, sizes.data(), ty.data(), l.data(), u.data(), v.data(), cp.data(), as.data());
    if (!c) return fail("custom circuit");
    if (vph_verify_full_record(c, rec.data(), rec.size()) != 0) return fail("record rejected");
    for (int i = 3; i < argc; ++i) {
        const long o = atol(argv[i]);
        if (o < 0 || (size_t) o >= rec.size()) return fail("offset outside the record", o);
        rec[o] ^= 0x04;
        if (vph_verify_full_record(c, rec.data(), rec.size()) == 0) return fail("tampered record accepted", o);
        rec[o] ^= 0x04;
        if (vph_verify_full_record(c, rec.data(), (uint64_t) o) == 0) return fail("record cut short accepted", o);
    }
    if (vph_verify_full_record(c, rec.data(), rec.size() - 1) == 0) return fail("truncated record accepted");
    if (vph_verify_full_record(c, rec.data(), 0) == 0) return fail("empty record accepted");
    {
        std::vector<uint8_t> longer(rec);
        longer.push_back(0);
        if (vph_verify_full_record(c, longer.data(), longer.size()) == 0) return fail("extended record accepted");
    }
    if (vph_verify_full_record(c, rec.data(), rec.size()) != 0) return fail("record rejected at the end");
    vph_circuit_free(c);
    puts("record_asan ok");
    return 0;
}
