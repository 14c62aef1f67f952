// The live-slice rule of virgo-plus_amd/csrc/vp_pc_live.h at every input-layer bit length 7 .. 25, with n_used on and beside every slice boundary:
// live against a slice-by-slice count, the real pairs cover 0 .. live - 1 once each, no index reaches 64, a partner beyond live - 1 is the one dead slice
// `live`, a full layer gives the 32 / 32 pairing the encode had before, and the switch restores 64 everywhere.  Plain g++ with the sanitizers, nothing but the
// header under test.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../virgo-plus_amd/csrc/vp_pc_live.h"

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++bad < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static void check(int n, uint64_t n_used) {
    const uint64_t N = (uint64_t) 1 << (n - 6);
    unsigned want = 0;                                   // slices that hold one of the first n_used entries
    for (unsigned s = 0; s < 64; ++s) if ((uint64_t) s * N < n_used) ++want;
    const PcLive v(n, n_used, true);
    CHECK(v.live == want, "n %d n_used %llu: live %u, counted %u", n, (unsigned long long) n_used, v.live, want);
    CHECK(v.live >= 1 && v.live <= 64, "n %d n_used %llu: live %u", n, (unsigned long long) n_used, v.live);
    CHECK(v.pair_rows == (v.live + 1) / 2, "n %d n_used %llu: pair_rows %u", n, (unsigned long long) n_used, v.pair_rows);
    CHECK(v.pair_end() <= 64 && v.pair_end() >= v.live && v.pair_end() <= v.live + 1, "n %d n_used %llu: pair_end %u", n, (unsigned long long) n_used, v.pair_end());
    std::vector<int> seen(64, 0);
    for (unsigned p = 0; p < v.pair_rows; ++p) {
        const unsigned a = v.pair_a(p), b = v.pair_b(p);
        CHECK(a < 64 && b < 64, "n %d n_used %llu: pair %u = (%u, %u)", n, (unsigned long long) n_used, p, a, b);
        if (a < 64) ++seen[a];
        if (b < 64) ++seen[b];
        CHECK(a < v.live, "n %d n_used %llu: first of pair %u is dead slice %u", n, (unsigned long long) n_used, p, a);
        CHECK(b <= v.live, "n %d n_used %llu: partner %u beyond the first dead slice", n, (unsigned long long) n_used, b);
    }
    for (unsigned s = 0; s < 64; ++s) {
        if (s < v.live) CHECK(seen[s] == 1, "n %d n_used %llu: slice %u covered %d times", n, (unsigned long long) n_used, s, seen[s]);
        else CHECK(seen[s] == ((s == v.live && (v.live & 1)) ? 1 : 0), "n %d n_used %llu: dead slice %u covered %d times", n, (unsigned long long) n_used, s, seen[s]);
    }
    if (v.live == 64) CHECK(v.pair_rows == 32 && v.pair_b(0) == 32 && v.pair_b(31) == 63, "n %d: full layer is not 32 / 32", n);
    const PcLive off(n, n_used, false);
    CHECK(off.live == 64 && off.pair_rows == 32, "n %d n_used %llu: switched off gives %u / %u", n, (unsigned long long) n_used, off.live, off.pair_rows);
}

int main() {
    long cases = 0;
    for (int n = 7; n <= 25; ++n) {
        const uint64_t N = (uint64_t) 1 << (n - 6), total = (uint64_t) 1 << n;
        for (unsigned s = 0; s <= 64; ++s)
            for (int d = -1; d <= 1; ++d) {
                const int64_t u = (int64_t) (s * N) + d;
                if (u < 1 || (uint64_t) u > total) continue;
                check(n, (uint64_t) u); ++cases;
            }
        if (n >= 13) { check(n, 7226ull << (n - 13)); ++cases; }      // the SHA-256 circuit's share of its layer: 7226 inputs per block
    }
    const PcLive d;                                      // the default: every slice
    CHECK(d.live == 64 && d.pair_rows == 32, "default %u / %u", d.live, d.pair_rows);
    const PcLive sha(23, 7226ull * 1024, true);          // 1024 SHA-256 blocks
    CHECK(sha.live == 57 && sha.pair_rows == 29, "sha256 x1024: %u / %u", sha.live, sha.pair_rows);
    if (bad) { std::printf("pc_live: %d mismatches\n", bad); return 1; }
    std::printf("pc_live ok: %ld cases\n", cases);
    return 0;
}
