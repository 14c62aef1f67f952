// SHA3-256 of one 64-byte block (the reference's my_hhash, lib/virgo/src/my_hhash.h:27-33, which calls XKCP's
// SHA3_256): host copy used by the verifier to recompute leaf chains and Merkle paths.  FIPS 202.
#pragma once
#include <cstdint>
#include <cstring>

namespace vph {

struct hhash_digest {
    uint64_t w[4];
    bool operator==(const hhash_digest &o) const { return !memcmp(w, o.w, 32); }
    bool operator!=(const hhash_digest &o) const { return !(*this == o); }
};

inline void keccak_f1600(uint64_t s[25]) {
    static const uint64_t rc[24] = {
        0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
        0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
        0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
        0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
        0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    static const int rot[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
    static const int pil[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
    for (int r = 0; r < 24; ++r) {
        uint64_t bc[5];
        for (int i = 0; i < 5; ++i) bc[i] = s[i] ^ s[i + 5] ^ s[i + 10] ^ s[i + 15] ^ s[i + 20];
        for (int i = 0; i < 5; ++i) {
            const uint64_t t = bc[(i + 4) % 5] ^ ((bc[(i + 1) % 5] << 1) | (bc[(i + 1) % 5] >> 63));
            for (int j = 0; j < 25; j += 5) s[j + i] ^= t;
        }
        uint64_t t = s[1];
        for (int i = 0; i < 24; ++i) {           // rho + pi along the single 24-cycle of the lane permutation
            const int j = pil[i];
            const uint64_t b = s[j];
            s[j] = (t << rot[i]) | (t >> (64 - rot[i]));
            t = b;
        }
        for (int j = 0; j < 25; j += 5) {
            uint64_t b[5];
            for (int i = 0; i < 5; ++i) b[i] = s[j + i];
            for (int i = 0; i < 5; ++i) s[j + i] = b[i] ^ (~b[(i + 1) % 5] & b[(i + 2) % 5]);
        }
        s[0] ^= rc[r];
    }
}

// digest of (m[0..4) || prev) — the 64-byte block of the leaf chains and of the Merkle nodes
inline hhash_digest hhash(const uint64_t m[4], const hhash_digest &prev) {
    uint64_t s[25] = {0};
    s[0] = m[0]; s[1] = m[1]; s[2] = m[2]; s[3] = m[3];
    s[4] = prev.w[0]; s[5] = prev.w[1]; s[6] = prev.w[2]; s[7] = prev.w[3];
    s[8] = 0x06; s[16] = 0x8000000000000000ull;
    keccak_f1600(s);
    hhash_digest d; d.w[0] = s[0]; d.w[1] = s[1]; d.w[2] = s[2]; d.w[3] = s[3];
    return d;
}

// The Fiat-Shamir chain of proveFS / checkFS and of the non-interactive commitment proof (its text: vphost.h, "The transcript chain"): every step is
// state = hhash(m, state) from the all-zero state.  One implementation for the prover's and the verifier's side.
struct fs_chain {
    hhash_digest s{};
    void step(uint64_t a, uint64_t b, uint64_t c, uint64_t d) { const uint64_t m[4] = {a, b, c, d}; s = hhash(m, s); }
    void param(uint64_t a, uint64_t b, uint64_t c, uint64_t d) { step(1, 0, 0, 0x50); step(a, b, c, d); }          // P(a, b, c, d)
    void elem(uint64_t re, uint64_t im) { step(re, im, 0, 0x4d); }                                                     // E(x)
    void digest(uint64_t label, const uint8_t d[32]) { uint64_t w[4]; memcpy(w, d, 32); step(label, 0, 0, 0x44); step(w[0], w[1], w[2], w[3]); }   // D(t, d)
    // a digest word -> a limb: the low 61 bits, p itself mapped to 0 (the bias is 2^-61)
    static uint64_t limb(uint64_t w) { const uint64_t P = 2305843009213693951ull; w &= P; return w == P ? 0 : w; }
    void challenge(uint64_t c, uint64_t &re, uint64_t &im) { step(c, 0, 0, 0x43); re = limb(s.w[0]); im = limb(s.w[1]); }   // C(c)
    // Q(q): a leaf in [2^(n-7), 2^(n-2)), the range pcVerifyCommitment accepts
    uint64_t position(uint64_t q, int n) { step(q, 0, 0, 0x51); const uint64_t lo = 1ull << (n - 7); return lo + s.w[0] % ((1ull << (n - 2)) - lo); }
    // W(b, nonce): the proof-of-work step; the work is met when the low b bits of the new state's first word are zero (b in 1 .. 48)
    bool work(uint64_t bits, uint64_t nonce) { step(nonce, bits, 0, 0x57); return (s.w[0] & ((1ull << bits) - 1)) == 0; }
};
// The smallest nonce in [first, first + max_tries) whose W(bits, nonce) on `from` meets the work: true and *nonce, or false (nothing is written).  The caller
// has checked bits in 1 .. 48, max_tries >= 1 and first + max_tries <= 2^64.
inline bool fs_grind(const hhash_digest &from, int bits, uint64_t first, uint64_t max_tries, uint64_t *nonce) {
    const uint64_t mask = (1ull << bits) - 1, m3 = 0x57;
    for (uint64_t i = 0; i < max_tries; ++i) {
        const uint64_t m[4] = {first + i, (uint64_t) bits, 0, m3};
        if ((hhash(m, from).w[0] & mask) == 0) { *nonce = first + i; return true; }
    }
    return false;
}

// Streaming SHA3-256 (FIPS 202 sponge, rate 136 bytes): the statement digest of the Fiat-Shamir mode absorbs the whole
// serialised circuit and its input values through it (verifier::fsInit).
class sha3_256 {
public:
    void update(const void *data, size_t n) {
        const uint8_t *p = static_cast<const uint8_t *>(data);
        while (n) {
            const size_t take = n < 136 - fill ? n : 136 - fill;
            memcpy(buf + fill, p, take);
            fill += take; p += take; n -= take;
            if (fill == 136) { absorb(); fill = 0; }
        }
    }
    void put64(uint64_t x) { update(&x, 8); }
    hhash_digest final() {
        memset(buf + fill, 0, 136 - fill);
        buf[fill] ^= 0x06; buf[135] ^= 0x80;
        absorb();
        hhash_digest d; memcpy(d.w, s, 32);
        return d;
    }
private:
    void absorb() {
        for (int i = 0; i < 17; ++i) { uint64_t w; memcpy(&w, buf + 8 * i, 8); s[i] ^= w; }
        keccak_f1600(s);
    }
    uint64_t s[25] = {0};
    uint8_t buf[136];
    size_t fill = 0;
};

}  // namespace vph
