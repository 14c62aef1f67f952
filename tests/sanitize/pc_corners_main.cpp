// pc_eq_corners of virgo-plus_amd/csrc/vp_pc_corners.h against the textbook eq table: eq(pt, j) = the product over ALL n bits k of j of pt[k] (bit set) or
// 1 - pt[k] (bit clear), written here with unsigned __int128 `%` arithmetic and none of the header's own multiply.  corner[i] must be entry i N, N = 2^(n-6),
// at n = 7, 8, 13 and 25: entry by entry at every n, and at n <= 13 also read out of the whole table built by doubling (initBetaTable's order).  Points: all 0,
// all 1, all p - 1, all (p - 1) + (p - 1) i, those mixed with i and random coordinates along the point, and random points.  Plain g++ with the sanitizers.
#include <cstdio>
#include <vector>

#include "../../virgo-plus_amd/csrc/vp_pc_corners.h"

using namespace vp;

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++bad < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static u64 mulmod(u64 a, u64 b) { return (u64) ((u128) a * b % P61); }
static F ref_mul(F a, F b) {                              // (a.re + a.im i)(b.re + b.im i), i^2 = -1
    const u64 rr = mulmod(a.re, b.re), ii = mulmod(a.im, b.im), ri = mulmod(a.re, b.im), ir = mulmod(a.im, b.re);
    return f_make((rr + P61 - ii) % P61, (ri + ir) % P61);
}
static F ref_one_minus(F x) { return f_make((1 + P61 - x.re) % P61, (P61 - x.im) % P61); }
static F ref_eq(const std::vector<F> &pt, u64 j) {
    F v = f_make(1, 0);
    for (size_t k = 0; k < pt.size(); ++k) v = ref_mul(v, ((j >> k) & 1) ? pt[k] : ref_one_minus(pt[k]));
    return v;
}

static u64 rng_state = 0x243f6a8885a308d3ull;
static u64 rnd64() {                                      // splitmix64
    u64 z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static F rnd_f() { return f_make(rnd64() % P61, rnd64() % P61); }

static long check(const char *what, const std::vector<F> &pt) {
    const int n = (int) pt.size();
    const u64 N = (u64) 1 << (n - 6);
    // guard elements around the output: the function writes corner[0 .. 63] and nothing else
    std::vector<F> out(66, f_make(7, 7));
    pc_eq_corners(pt.data(), n, out.data() + 1);
    CHECK(out[0].re == 7 && out[0].im == 7 && out[65].re == 7 && out[65].im == 7, "%s n %d: wrote outside corner[0 .. 63]", what, n);
    const F *corner = out.data() + 1;
    for (u64 i = 0; i < 64; ++i) {
        const F want = ref_eq(pt, i * N);
        CHECK(corner[i].re == want.re && corner[i].im == want.im, "%s n %d corner %llu: (%llu, %llu), textbook (%llu, %llu)", what, n, i, corner[i].re, corner[i].im,
              want.re, want.im);
        CHECK(corner[i].re < P61 && corner[i].im < P61, "%s n %d corner %llu not canonical", what, n, i);
    }
    if (n <= 13) {                                        // the whole table, by doubling: T[j + 2^k] = T[j] pt[k], T[j] = T[j] (1 - pt[k])
        std::vector<F> T((size_t) 1 << n);
        T[0] = f_make(1, 0);
        for (int k = 0; k < n; ++k)
            for (u64 j = 0; j < ((u64) 1 << k); ++j) { T[j + ((u64) 1 << k)] = ref_mul(T[j], pt[k]); T[j] = ref_mul(T[j], ref_one_minus(pt[k])); }
        for (u64 i = 0; i < 64; ++i)
            CHECK(corner[i].re == T[i * N].re && corner[i].im == T[i * N].im, "%s n %d corner %llu differs from table entry %llu", what, n, i, i * N);
    }
    return 64;
}

int main() {
    long cases = 0;
    const F zero = f_make(0, 0), one = f_make(1, 0), pm1 = f_make(P61 - 1, 0), top = f_make(P61 - 1, P61 - 1), iota = f_make(0, 1);
    for (int n : {7, 8, 13, 25}) {
        for (const F &c : {zero, one, pm1, top}) cases += check("constant", std::vector<F>((size_t) n, c));
        // the special coordinates at every place along the point, low (shared factor) and high (per-corner factors) alike
        const F special[6] = {zero, one, pm1, top, iota, f_make(P61 - 1, 1)};
        for (int shift = 0; shift < 7; ++shift) {
            std::vector<F> pt((size_t) n);
            for (int k = 0; k < n; ++k) { const int q = (k + shift) % 7; pt[(size_t) k] = q < 6 ? special[q] : rnd_f(); }
            cases += check("mixed", pt);
        }
        // no zero corner: every coordinate away from 0 and 1, the special ones among random ones
        for (int rep = 0; rep < 4; ++rep) {
            std::vector<F> pt((size_t) n);
            for (auto &x : pt) x = rnd_f();
            pt[(size_t) rep % pt.size()] = top; pt[pt.size() - 1 - (size_t) rep] = pm1;
            cases += check("random", pt);
        }
    }
    if (bad) { std::printf("pc_corners: %d mismatches\n", bad); return 1; }
    std::printf("pc_corners ok: %ld corners\n", cases);
    return 0;
}
