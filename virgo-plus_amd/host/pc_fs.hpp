// The fixed parts of the non-interactive commitment proof's Fiat-Shamir chain (its text: vphost.h, "The transcript chain"), shared by prover::commitFS and
// pcParseCommitmentFS: one piece of code walks the chain on both sides.
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "circuit.hpp"
#include "field.hpp"
#include "sha3.hpp"

constexpr uint32_t PCFS_MAGIC = 0x46435056u, PCFS_VERSION = 1;      // the proof's header: "VPCF", version 1
constexpr uint32_t PCFS_VERSION_POW = 2;                             // version 2, of the commitment proof and of the joined proof alike: u64 pow_bits | u64 nonce behind the header
constexpr int PCFS_POW_MAX_BITS = 48, PCFS_POW_PROVER_BITS = 32;     // what a proof may carry; what the provers take

// steps 1 .. 7: the chain up to D(1, root_h), what both sides absorb before the commit phase
inline void pcFsAbsorbHead(vph::fs_chain &ch, int n, u64 reps, u64 ms, const std::vector<F> &point, const std::vector<F> &pub_mask, const F &claim, const uint8_t root_l[32],
                    const uint8_t root_h[32], const std::vector<F> &all_sum) {
    const u64 n_pub = ms == 1 ? 0 : pub_mask.size();
    ch.param((u64) n, reps, ms, n_pub);
    ch.digest(0, root_l);
    for (int i = 0; i < n; ++i) ch.elem(point[i].real, point[i].img);
    for (u64 i = 0; i < n_pub; ++i) ch.elem(pub_mask[i].real, pub_mask[i].img);
    ch.elem(claim.real, claim.img);
    for (int i = 0; i < 65; ++i) ch.elem(all_sum[i].real, all_sum[i].img);
    ch.digest(1, root_h);
}
// steps 8 and 9 on the host: r_0 = C(0); then per level D(2 + k, root_k) and, for k + 1 < ln, r_(k+1) = C(k + 1) (true: *next was drawn)
inline F pcFsFirstChallenge(vph::fs_chain &ch) { uint64_t a, b; ch.challenge(0, a, b); F r; r.real = a; r.img = b; return r; }
inline bool pcFsLevel(vph::fs_chain &ch, int k, int ln, const uint8_t root[32], F *next) {
    ch.digest(2 + (u64) k, root);
    if (k + 1 >= ln) return false;
    uint64_t a, b;
    ch.challenge((u64) k + 1, a, b);
    next->real = a; next->img = b;
    return true;
}
// The proof of work between the final codewords and the positions.  bits = 0: no step (a version-1 proof).  The prover sets `find`, which is handed the state
// the final codewords leave and returns the nonce; the verifier sets the proof's nonce.  met: whether W(bits, nonce) met the work.
struct PcFsWork {
    u64 bits = 0, nonce = 0;
    bool met = true;
    std::function<u64(const vph::hhash_digest &)> find;
};
// the second header of a version-2 proof: 1 .. 48 bits (0 has one encoding, version 1)
inline bool pcFsWorkHeader(const uint8_t *p, PcFsWork &w) {
    memcpy(&w.bits, p, 8); memcpy(&w.nonce, p + 8, 8);
    return w.bits >= 1 && w.bits <= (u64) PCFS_POW_MAX_BITS;
}
// steps 10 .. 12: the final codewords, W(bits, nonce) where the proof carries work, then the positions from the state it leaves
inline std::vector<u64> pcFsPositions(vph::fs_chain &ch, int n, u64 reps, const std::vector<F> &final_code, const std::vector<F> &final_mask, PcFsWork *w = nullptr) {
    for (const F &x : final_code) ch.elem(x.real, x.img);
    for (const F &x : final_mask) ch.elem(x.real, x.img);
    if (w && w->bits) {
        if (w->find) w->nonce = w->find(ch.s);
        w->met = ch.work(w->bits, w->nonce);
    }
    std::vector<u64> lf(reps);
    for (u64 q = 0; q < reps; ++q) lf[q] = ch.position(q, n);
    return lf;
}
