// TEST INFRASTRUCTURE ONLY.  Sanitizer leg of the GKR part's Fiat-Shamir derivation: virgo-plus_amd/host/*.cpp compiled with -fsanitize=address,undefined
// (tests/test_gkr_fs_host.py builds tests/sanitize/_build/gkr_fs_asan; libvpgpu.so is linked but no device call is made) and driven through vph_gkr_sizes and
// vph_gkr_fs_tape on the host: the recorded transcript, then transcripts of every length around it and with non-canonical limbs — each heap copy is exactly as
// long as what it holds, the tape buffer exactly vph_gkr_sizes' elements, so a read or write past an end is a report.  argv: the circuit (layers, log_size, seed
// of vph_circuit_randomize), the transcript, the 32-byte start state, the expected tape followed by the expected closing state, the expected number of draws.
#include "../../virgo-plus_amd/host/vphost.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static vph_circuit *circ = nullptr;
static uint64_t n_tape = 0, n_bytes = 0;
static int fail(const char *what, long at = -1) { fprintf(stderr, "gkr_fs_asan: %s (%ld)\n", what, at); return 1; }
static std::vector<uint8_t> slurp(const char *p) {
    std::vector<uint8_t> v;
    FILE *f = fopen(p, "rb");
    if (!f) return v;
    uint8_t b[4096]; size_t n;
    while ((n = fread(b, 1, sizeof b, f)) > 0) v.insert(v.end(), b, b + n);
    fclose(f);
    return v;
}
// the derivation on exact-size heap copies; tape | state copied out when asked for
static int derive(const std::vector<uint8_t> &tr, const uint8_t state[32], uint64_t *draws, std::vector<uint8_t> *out) {
    uint8_t *q = static_cast<uint8_t *>(malloc(tr.size() ? tr.size() : 1));
    if (!tr.empty()) memcpy(q, tr.data(), tr.size());
    uint64_t *tape = static_cast<uint64_t *>(malloc(n_tape ? 16 * n_tape : 1));
    uint8_t *st_in = static_cast<uint8_t *>(malloc(32)), *st_out = static_cast<uint8_t *>(malloc(32));
    memcpy(st_in, state, 32);
    uint64_t d = 0;
    const int rc = vph_gkr_fs_tape(circ, st_in, q, tr.size(), tape, &d, st_out);
    if (rc == 0) {
        if (draws) *draws = d;
        if (out) { out->assign(reinterpret_cast<uint8_t *>(tape), reinterpret_cast<uint8_t *>(tape) + 16 * n_tape); out->insert(out->end(), st_out, st_out + 32); }
    }
    free(q); free(tape); free(st_in); free(st_out);
    return rc;
}

int main(int argc, char **argv) {
    if (argc < 8) return fail("usage");
    circ = vph_circuit_randomize(atoi(argv[1]), atoi(argv[2]), atol(argv[3]));
    if (!circ) return fail("no circuit");
    const std::vector<uint8_t> good = slurp(argv[4]), state = slurp(argv[5]), want = slurp(argv[6]);
    const uint64_t want_draws = strtoull(argv[7], nullptr, 10);
    if (vph_gkr_sizes(circ, &n_tape, &n_bytes) != 0) return fail("vph_gkr_sizes");
    if (good.size() != n_bytes || state.size() != 32 || want.size() != 16 * n_tape + 32) return fail("the files do not fit the circuit");
    uint64_t draws = 0;
    std::vector<uint8_t> got;
    if (derive(good, state.data(), &draws, &got) != 0) return fail("the recorded transcript is refused");
    if (draws != want_draws || got != want) return fail("tape, count or state differ from the expected ones");
    // one changed bit: still a transcript (unless the limb leaves the field), another tape or state
    for (size_t i = 0; i < good.size(); i += 29) {
        std::vector<uint8_t> p = good, o;
        p[i] ^= 0x10;
        const int rc = derive(p, state.data(), &draws, &o);
        if (rc != 0 && rc != -1) return fail("a changed byte: neither derived nor refused", (long) i);
        if (rc == 0 && (o == want || draws != want_draws)) return fail("a changed byte leaves tape and state", (long) i);
    }
    // every length but the right one is refused: around both ends, a stride through the middle, extended
    std::vector<size_t> len = {0, 1, 15, 16, 17, 47, 48, 49, good.size() - 17, good.size() - 16, good.size() - 15, good.size() - 1, good.size() + 1, good.size() + 15,
                               good.size() + 16, good.size() + 4096, 2 * good.size()};
    for (size_t i = 64; i < good.size(); i += 101) len.push_back(i);
    for (size_t n : len) {
        if (n == good.size()) continue;
        std::vector<uint8_t> p = good;
        p.resize(n, 0);
        if (derive(p, state.data(), nullptr, nullptr) != -1) return fail("a transcript of another length is not refused", (long) n);
    }
    // non-canonical limbs anywhere: p, p + 1, 2^63, 2^64 - 1 in the first, a middle and the last element, either limb
    const uint64_t P = (1ull << 61) - 1, limbs[] = {P, P + 1, 1ull << 63, ~0ull};
    for (size_t off : {(size_t) 0, (size_t) 8, good.size() / 32 * 16, good.size() / 32 * 16 + 8, good.size() - 16, good.size() - 8})
        for (uint64_t v : limbs) {
            std::vector<uint8_t> p = good;
            memcpy(p.data() + off, &v, 8);
            if (derive(p, state.data(), nullptr, nullptr) != -1) return fail("a non-canonical limb is not refused", (long) off);
        }
    {   // p - 1 is an element
        std::vector<uint8_t> p = good;
        const uint64_t v = P - 1;
        memcpy(p.data() + 8, &v, 8);
        if (derive(p, state.data(), &draws, nullptr) != 0 || draws != want_draws) return fail("a limb of p - 1 is refused");
    }
    // null arguments
    {
        std::vector<uint64_t> tape(2 * n_tape + 2);
        uint8_t so[32];
        uint64_t d = 0;
        if (vph_gkr_fs_tape(nullptr, state.data(), good.data(), good.size(), tape.data(), &d, so) != -1 || vph_gkr_fs_tape(circ, nullptr, good.data(), good.size(), tape.data(), &d, so) != -1 ||
            vph_gkr_fs_tape(circ, state.data(), nullptr, good.size(), tape.data(), &d, so) != -1 || vph_gkr_fs_tape(circ, state.data(), good.data(), good.size(), nullptr, &d, so) != -1 ||
            vph_gkr_fs_tape(circ, state.data(), good.data(), good.size(), tape.data(), nullptr, so) != -1 ||
            vph_gkr_fs_tape(circ, state.data(), good.data(), good.size(), tape.data(), &d, nullptr) != -1 || vph_gkr_sizes(nullptr, &n_tape, &n_bytes) != -1)
            return fail("a null argument is not refused");
    }
    vph_circuit_free(circ);
    printf("gkr_fs_asan ok\n");
    return 0;
}
