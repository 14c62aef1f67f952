// The 31-bit split forms of virgo-plus_amd/csrc/vp_field.h (MS = false, the instantiation a host compiler sees) at the EDGES of the operand ranges
// their comments state, against unsigned __int128 `%` arithmetic written here without the header's own multiply.  Uniform values in [0, p) reach
// these places with probability ~2^-58 per operation: an accumulator a few units below 2^64, a split half of all ones, the non-canonical zeros
// p and 2p, a weak result at its bound.  Strict forms must return exactly the canonical residue; WEAK forms must be congruent AND below 2^61 + 4.
// Prints the number of operand tuples per form; exit status 1 and the first offending tuples if a contract does not hold.
// Built by tests/test_field_edges_host.py, plain and under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../virgo-plus_amd/csrc/vp_field.h"

using namespace vp;

static const u64 P = P61, P2 = 2 * P61, B61 = 1ull << 61;
static const u64 WEAK_BOUND = B61 + 4;

// boundary sets per stated range
static const std::vector<u64> CANON = {0, 1, (1ull << 31) - 1, 1ull << 31, (1ull << 31) + 1, 1ull << 60, P - 1};
static std::vector<u64> lazy_set() {                    // [0, 2p]
    std::vector<u64> v = CANON;
    for (u64 x : {P, P + 1, B61 + 7, P2 - 1, P2}) v.push_back(x);
    return v;
}
static std::vector<u64> wide_set() {                    // < 2^62: [0, 2p] and the all-ones split (hi = lo = 2^31 - 1)
    std::vector<u64> v = lazy_set();
    v.push_back((1ull << 62) - 1);
    return v;
}
static const std::vector<u64> LAZY = lazy_set(), WIDE = wide_set();
static const std::vector<u64> ADD_P = {0, P - 1, P};                          // addend of the f_mad forms: [0, p]
static const std::vector<u64> ADD_W = {0, P - 1, P, B61 + 7};                 // addend of the dot forms: < 2^61 + 8
static std::vector<u64> canon_or_p() { std::vector<u64> v = CANON; v.push_back(P); return v; }      // a negated limb p - x reaches p itself
static const std::vector<u64> CANON_P = canon_or_p();

static u64 rng_state = 0x9e3779b97f4a7c15ull;
static u64 rnd64() {                                    // splitmix64
    u64 z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static u64 rnd_upto(u64 max_incl) { return (u64) (((u128) rnd64() * ((u128) max_incl + 1)) >> 64); }

static u64 mod_p(u128 x) { return (u64) (x % P); }
static u64 mulmod(u64 a, u64 b) { return mod_p((u128) a * b); }

struct Form {
    const char *name;
    unsigned long long checked = 0, failed = 0;
    explicit Form(const char *n) : name(n) {}
    // strict: got is the canonical residue.  weak: congruent and below `bound`.
    void check(u64 got, u64 exp, bool weak, u64 bound, const u64 *ops, int n_ops, bool second_limb = false) {
        if (!second_limb) ++checked;                    // a tuple is counted once, with its real limb
        const bool ok = weak ? (got < bound && got % P == exp) : got == exp;
        if (ok) return;
        if (failed++ < 5) {
            fprintf(stderr, "FAIL %s: got %llu (mod p %llu) expected %llu%s; operands", name, got, got % P, exp, weak && got >= bound ? " ABOVE THE BOUND" : "");
            for (int i = 0; i < n_ops; ++i) fprintf(stderr, " %llu", ops[i]);
            fprintf(stderr, "\n");
        }
    }
    bool report() const { printf("%-28s %10llu tuples%s\n", name, checked, failed ? "  FAILED" : ""); return failed == 0; }
};

static const int N_RANDOM = 4000;

// ---- dot2_31 / dot2_31c / dot1_31 / dot1_31c on split operands ----
template <bool WEAK> static void one_dot2(Form &f, u64 x, u64 y, u64 z, u64 w, u64 add) {
    const u64 ops[5] = {x, y, z, w, add};
    f.check(dot2_31<WEAK, false>(split31(x), split31(y), split31(z), split31(w), add), mod_p((u128) x * y + (u128) z * w + add), WEAK, WEAK_BOUND, ops, 5);
}
template <bool WEAK> static bool run_dot2() {           // x, y, z, w < 2^62, addend < 2^61 + 8
    Form f(WEAK ? "dot2_31<weak>" : "dot2_31<strict>");
    for (u64 x : WIDE) for (u64 y : WIDE) for (u64 z : WIDE) for (u64 w : WIDE) for (u64 c : ADD_W) one_dot2<WEAK>(f, x, y, z, w, c);
    const u64 top = (1ull << 62) - 1;
    for (int i = 0; i < N_RANDOM; ++i) one_dot2<WEAK>(f, rnd_upto(top), rnd_upto(top), rnd_upto(top), rnd_upto(top), rnd_upto(B61 + 7));
    return f.report();
}
template <bool WEAK> static void one_dot2c(Form &f, u64 x, u64 y, u64 z, u64 w, u64 add) {
    const u64 ops[5] = {x, y, z, w, add};
    f.check(dot2_31c<WEAK, false>(split31(x), split31(y), split31(z), split31(w), add), mod_p((u128) x * y + (u128) z * w + add), WEAK, WEAK_BOUND, ops, 5);
}
template <bool WEAK> static bool run_dot2c() {          // x, z canonical or p (high half < 2^30: the all-ones pattern with the largest hi), y, w < 2^62
    Form f(WEAK ? "dot2_31c<weak>" : "dot2_31c<strict>");
    for (u64 x : CANON_P) for (u64 y : WIDE) for (u64 z : CANON_P) for (u64 w : WIDE) for (u64 c : ADD_W) one_dot2c<WEAK>(f, x, y, z, w, c);
    const u64 top = (1ull << 62) - 1;
    for (int i = 0; i < N_RANDOM; ++i) one_dot2c<WEAK>(f, rnd_upto(P), rnd_upto(top), rnd_upto(P), rnd_upto(top), rnd_upto(B61 + 7));
    return f.report();
}
template <bool WEAK, bool CANON_X> static bool run_dot1() {     // x canonical (dot1_31c) or < 2^62 (dot1_31), y < 2^62
    Form f(CANON_X ? (WEAK ? "dot1_31c<weak>" : "dot1_31c<strict>") : (WEAK ? "dot1_31<weak>" : "dot1_31<strict>"));
    auto one = [&](u64 x, u64 y, u64 add) {
        const u64 ops[3] = {x, y, add};
        const u64 got = CANON_X ? dot1_31c<WEAK, false>(split31(x), split31(y), add) : dot1_31<WEAK, false>(split31(x), split31(y), add);
        f.check(got, mod_p((u128) x * y + add), WEAK, WEAK_BOUND, ops, 3);
    };
    const std::vector<u64> &xs = CANON_X ? CANON_P : WIDE;
    for (u64 x : xs) for (u64 y : WIDE) for (u64 c : ADD_W) one(x, y, c);
    const u64 top = (1ull << 62) - 1;
    for (int i = 0; i < N_RANDOM; ++i) one(rnd_upto(CANON_X ? P : top), rnd_upto(top), rnd_upto(B61 + 7));
    return f.report();
}

// ---- the F-level forms: a*b + c ----
static void expect_mad(const F &a, const F &b, const F &c, u64 &re, u64 &im) {
    re = mod_p((u128) mulmod(a.re, b.re) + (P - mulmod(a.im, b.im)) + c.re);
    im = mod_p((u128) mulmod(a.re, b.im) + mulmod(a.im, b.re) + c.im);
}
template <bool WEAK, bool CANON_A> static bool run_mad() {      // f_mad31: a, b in [0, 2p]; f_mad31c: a canonical, b in [0, 2p]; c in [0, p]
    Form f(CANON_A ? (WEAK ? "f_mad31c<weak>" : "f_mad31c<strict>") : (WEAK ? "f_mad31<weak>" : "f_mad31<strict>"));
    auto one = [&](const F &a, const F &b, const F &c) {
        const u64 ops[6] = {a.re, a.im, b.re, b.im, c.re, c.im};
        u64 re, im;
        expect_mad(a, b, c, re, im);
        const F got = CANON_A ? f_mad31c<WEAK, false>(a, b, c) : f_mad31<WEAK, false>(a, b, c);
        f.check(got.re, re, WEAK, WEAK_BOUND, ops, 6);
        f.check(got.im, im, WEAK, WEAK_BOUND, ops, 6, true);
    };
    const std::vector<u64> &as = CANON_A ? CANON : LAZY;
    for (u64 ar : as) for (u64 ai : as) for (u64 br : LAZY) for (u64 bi : LAZY) for (u64 cr : ADD_P) for (u64 ci : ADD_P)
        one(f_make(ar, ai), f_make(br, bi), f_make(cr, ci));
    const u64 at = CANON_A ? P - 1 : P2;
    for (int i = 0; i < N_RANDOM; ++i)
        one(f_make(rnd_upto(at), rnd_upto(at)), f_make(rnd_upto(P2), rnd_upto(P2)), f_make(rnd_upto(P), rnd_upto(P)));
    return f.report();
}
template <bool WEAK, bool CANON_A> static bool run_mad_rb() {   // a * (y, 0) + c: y in [0, 2p]
    Form f(CANON_A ? (WEAK ? "f_mad31c_rb<weak>" : "f_mad31c_rb<strict>") : (WEAK ? "f_mad31_rb<weak>" : "f_mad31_rb<strict>"));
    auto one = [&](const F &a, u64 y, const F &c) {
        const u64 ops[5] = {a.re, a.im, y, c.re, c.im};
        const F got = CANON_A ? f_mad31c_rb<WEAK, false>(a, y, c) : f_mad31_rb<WEAK, false>(a, y, c);
        f.check(got.re, mod_p((u128) a.re * y + c.re), WEAK, WEAK_BOUND, ops, 5);
        f.check(got.im, mod_p((u128) a.im * y + c.im), WEAK, WEAK_BOUND, ops, 5, true);
    };
    const std::vector<u64> &as = CANON_A ? CANON : LAZY;
    for (u64 ar : as) for (u64 ai : as) for (u64 y : LAZY) for (u64 cr : ADD_P) for (u64 ci : ADD_P) one(f_make(ar, ai), y, f_make(cr, ci));
    const u64 at = CANON_A ? P - 1 : P2;
    for (int i = 0; i < N_RANDOM; ++i) one(f_make(rnd_upto(at), rnd_upto(at)), rnd_upto(P2), f_make(rnd_upto(P), rnd_upto(P)));
    return f.report();
}

// ---- dot4_31cc: four canonical products in one sum; the second and fourth left factors are negated limbs p - x in [1, p] ----
static bool run_dot4() {
    Form f("dot4_31cc");
    auto one = [&](const u64 (&v)[8]) {
        const u128 s = (u128) v[0] * v[1] + (u128) v[2] * v[3] + (u128) v[4] * v[5] + (u128) v[6] * v[7];
        f.check(dot4_31cc<false>(split31(v[0]), split31(v[1]), split31(v[2]), split31(v[3]), split31(v[4]), split31(v[5]), split31(v[6]), split31(v[7])),
                mod_p(s), false, 0, v, 8);
    };
    for (u64 x0 : CANON) for (u64 y0 : CANON) for (u64 x1 : CANON_P) for (u64 y1 : CANON)
        for (u64 x2 : CANON) for (u64 y2 : CANON) for (u64 x3 : CANON_P) for (u64 y3 : CANON) {
            const u64 v[8] = {x0, y0, x1, y1, x2, y2, x3, y3};
            one(v);
        }
    for (int i = 0; i < N_RANDOM; ++i) {
        u64 v[8];
        for (int k = 0; k < 8; ++k) v[k] = rnd_upto(P - 1);
        v[2] = P - v[2]; v[6] = P - v[6];              // [1, p]
        one(v);
    }
    // the device branch of f_dot2cc, spelled with the same splits (on the host f_dot2cc itself takes the 128-bit branch)
    Form g("f_dot2cc (split wiring)");
    auto oneF = [&](const F &a, const F &b, const F &c, const F &d) {
        const Sp31 ar = split31(a.re), ai = split31(a.im), nai = split31(P61 - a.im), br = split31(b.re), bi = split31(b.im);
        const Sp31 cr = split31(c.re), ci = split31(c.im), nci = split31(P61 - c.im), dr = split31(d.re), di = split31(d.im);
        const u64 ops[8] = {a.re, a.im, b.re, b.im, c.re, c.im, d.re, d.im};
        u64 r1, i1, r2, i2;
        expect_mad(a, b, f_zero(), r1, i1);
        expect_mad(c, d, f_zero(), r2, i2);
        g.check(dot4_31cc<false>(ar, br, nai, bi, cr, dr, nci, di), mod_p((u128) r1 + r2), false, 0, ops, 8);
        g.check(dot4_31cc<false>(ar, bi, ai, br, cr, di, ci, dr), mod_p((u128) i1 + i2), false, 0, ops, 8, true);
    };
    const std::vector<u64> few = {0, 1, (1ull << 31) - 1, 1ull << 31, P - 1};
    for (u64 a0 : few) for (u64 a1 : few) for (u64 b0 : few) for (u64 b1 : few) for (u64 c0 : few) for (u64 c1 : few) for (u64 d0 : few) for (u64 d1 : few)
        oneF(f_make(a0, a1), f_make(b0, b1), f_make(c0, c1), f_make(d0, d1));
    for (int i = 0; i < N_RANDOM; ++i)
        oneF(f_make(rnd_upto(P - 1), rnd_upto(P - 1)), f_make(rnd_upto(P - 1), rnd_upto(P - 1)), f_make(rnd_upto(P - 1), rnd_upto(P - 1)), f_make(rnd_upto(P - 1), rnd_upto(P - 1)));
    const bool ok = f.report();
    return g.report() && ok;
}

// ---- c31_add<false>: C * 2^31 + base (mod p) for any middle word C; base + (C >> 30) + 2^61 < 2^64 is the caller's business ----
static bool run_c31() {
    Form f("c31_add<shift>");
    const std::vector<u64> Cs = {0, 1, (1ull << 30) - 1, 1ull << 30, (1ull << 30) + 1, (1ull << 31) - 1, 1ull << 33, 1ull << 63, ~0ull, 4 * ((1ull << 31) - 1) * ((1ull << 31) - 1)};
    const std::vector<u64> bases = {0, 1, P - 1, P, B61 + 7, 5 * B61};
    auto one = [&](u64 C, u64 base) {
        const u64 ops[2] = {C, base};
        f.check(c31_add<false>(C, base), mod_p(((u128) C << 31) + base), true, base + B61 + (1ull << 34), ops, 2);
    };
    for (u64 C : Cs) for (u64 b : bases) one(C, b);
    for (int i = 0; i < N_RANDOM; ++i) one(rnd64(), rnd_upto(5 * B61));
    return f.report();
}

// ---- canonical in, canonical out ----
static bool run_canonical() {
    bool ok = true;
    {
        Form f("m_add / m_sub"), h("f_half"), n("f_neg");
        const u64 inv2 = 1ull << 60;                    // 2 * 2^60 = 2^61 = 1 (mod p)
        auto pair = [&](u64 a, u64 b) {
            const u64 ops[2] = {a, b};
            f.check(m_add(a, b), mod_p((u128) a + b), false, 0, ops, 2);
            f.check(m_sub(a, b), mod_p((u128) a + P - b), false, 0, ops, 2, true);
        };
        auto single = [&](u64 a, u64 b) {
            const u64 ops[2] = {a, b};
            const F x = f_make(a, b), hx = f_half(x), nx = f_neg(x);
            h.check(hx.re, mulmod(a, inv2), false, 0, ops, 2); h.check(hx.im, mulmod(b, inv2), false, 0, ops, 2, true);
            n.check(nx.re, mod_p((u128) P - a), false, 0, ops, 2); n.check(nx.im, mod_p((u128) P - b), false, 0, ops, 2, true);
        };
        std::vector<u64> cs = CANON;
        for (u64 x : {2ull, P - 2, (P - 1) / 2, (P + 1) / 2}) cs.push_back(x);
        for (u64 a : cs) for (u64 b : cs) { pair(a, b); single(a, b); }
        for (int i = 0; i < N_RANDOM; ++i) { const u64 a = rnd_upto(P - 1), b = rnd_upto(P - 1); pair(a, b); single(a, b); }
        ok = f.report() && ok; ok = h.report() && ok; ok = n.report() && ok;
    }
    {
        Form f("m_red128");                            // x < 2^125
        auto one = [&](u128 x) {
            const u64 ops[2] = {(u64) (x >> 64), (u64) x};
            f.check(m_red128(x), mod_p(x), false, 0, ops, 2);
        };
        const u128 one128 = 1;
        std::vector<u128> xs = {0, 1, P - 1, P, (u128) P + 1, B61, (u128) P * P, (u128) (P - 1) * (P - 1), (u128) P2 * P2, (one128 << 122) - 1, one128 << 122,
                                (one128 << 125) - 1, ((u128) P << 61) * 2, ((u128) P << 61) * 3 + P - 1, (u128) P << 64, ((u128) P << 64) - 1};
        for (u128 x : xs) { one(x); if (x) one(x - 1); if (x + 1 < (one128 << 125)) one(x + 1); }
        for (u64 a : WIDE) for (u64 b : WIDE) one((u128) a * b);
        for (int i = 0; i < N_RANDOM; ++i) one((((u128) rnd64() << 64) | rnd64()) >> 3);
        ok = f.report() && ok;
    }
    {
        Form f("f_mul128 / f_mul_plain (host)");
        for (u64 ar : CANON) for (u64 ai : CANON) for (u64 br : CANON) for (u64 bi : CANON) {
            const F a = f_make(ar, ai), b = f_make(br, bi), got = f_mul_plain(a, b);
            const u64 ops[4] = {ar, ai, br, bi};
            u64 re, im;
            expect_mad(a, b, f_zero(), re, im);
            f.check(got.re, re, false, 0, ops, 4); f.check(got.im, im, false, 0, ops, 4, true);
        }
        ok = f.report() && ok;
    }
    return ok;
}

int main() {
    bool ok = true;
    ok = run_dot2<false>() && ok;       ok = run_dot2<true>() && ok;
    ok = run_dot2c<false>() && ok;      ok = run_dot2c<true>() && ok;
    ok = run_dot1<false, false>() && ok; ok = run_dot1<true, false>() && ok;
    ok = run_dot1<false, true>() && ok;  ok = run_dot1<true, true>() && ok;
    ok = run_mad<false, false>() && ok;  ok = run_mad<true, false>() && ok;
    ok = run_mad<false, true>() && ok;   ok = run_mad<true, true>() && ok;
    ok = run_mad_rb<false, false>() && ok; ok = run_mad_rb<true, false>() && ok;
    ok = run_mad_rb<false, true>() && ok;  ok = run_mad_rb<true, true>() && ok;
    ok = run_dot4() && ok;
    ok = run_c31() && ok;
    ok = run_canonical() && ok;
    printf(ok ? "field_edges ok\n" : "field_edges FAILED\n");
    return ok ? 0 : 1;
}
