// The GKR part of the Fiat-Shamir chain (its text: vphost.h, "The GKR part on the device"): the tape vp_prove_gkr_fs draws on the device, derived on the host
// from the transcript it returned.  A walk over the bytes — no sumcheck is checked, no predicate summed.  One walk for the prover's cross-check
// (prover::proveGkrFS) and for a caller that holds only the circuit and the proof (vph_gkr_fs_tape).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "circuit.hpp"
#include "field.hpp"
#include "sha3.hpp"

namespace vph {

// Where each draw sits on the tape of vp_prove_gkr (verifier::drawTape's order) and how long tape and transcript are, from the circuit's shape alone.
struct GkrLayout {
    int n_layers = 0, max_bl = 0;
    uint64_t n_tape = 0, n_tr = 0;
    std::vector<uint64_t> ru, ar, rv, sig, rl;      // per layer i >= 1: r_u[max_bl], assert_random, r_v[maxDadBitLength] (if any), sig[n_layers], r_liu[max_bl]
    explicit GkrLayout(const layeredCircuit &C) {
        const int n = C.size;
        n_layers = n;
        for (int i = 0; i < n; ++i) max_bl = std::max(max_bl, C.circuit[i].bitLength);
        ru.assign(n, 0); ar.assign(n, 0); rv.assign(n, 0); sig.assign(n, 0); rl.assign(n, 0);
        if (n < 2) return;
        uint64_t at = (uint64_t) C.circuit[n - 1].bitLength;      // r_0 at slot 0
        n_tr = 1;                                                   // Vres
        for (int i = n - 1; i >= 1; --i) {
            const int mdb = C.circuit[i].maxDadBitLength, pbl = C.circuit[i - 1].bitLength;
            ru[i] = at; at += (uint64_t) max_bl;
            ar[i] = at; at += 1;
            if (mdb != -1) { rv[i] = at; at += (uint64_t) mdb; }
            sig[i] = at; at += (uint64_t) n;
            rl[i] = at; at += (uint64_t) max_bl;
            n_tr += 3 * (uint64_t) pbl + 1;
            if (mdb != -1) n_tr += 3 * (uint64_t) mdb + (uint64_t) i;
            n_tr += 3 * (uint64_t) pbl + 1;
        }
        n_tape = at;
    }
};

// From the chain's state in ch: tape[0 .. L.n_tape) from tr[0 .. L.n_tr) in vp_prove_gkr's layout, slots the schedule never draws zero; ch ends in the closing
// state.  Returns the number of draws (the counter runs from 0).
inline uint64_t gkrFsTape(const layeredCircuit &C, const GkrLayout &L, fs_chain &ch, const F *tr, F *tape) {
    for (uint64_t i = 0; i < L.n_tape; ++i) { tape[i].real = 0; tape[i].img = 0; }
    uint64_t ctr = 0, pos = 0;
    auto draw = [&](uint64_t slot) { uint64_t a, b; ch.challenge(ctr++, a, b); tape[slot].real = a; tape[slot].img = b; };
    auto absorb = [&](uint64_t k) { for (uint64_t i = 0; i < k; ++i, ++pos) ch.elem(tr[pos].real, tr[pos].img); };
    auto rounds = [&](uint64_t slot0, int k) { for (int j = 0; j < k; ++j) { absorb(3); draw(slot0 + (uint64_t) j); } };
    const int n = L.n_layers;
    if (n < 2) return 0;
    for (int j = 0; j < C.circuit[n - 1].bitLength; ++j) draw((uint64_t) j);
    absorb(1);                                                      // Vres
    for (int i = n - 1; i >= 1; --i) {
        const int mdb = C.circuit[i].maxDadBitLength, pbl = C.circuit[i - 1].bitLength;
        draw(L.ar[i]);
        rounds(L.ru[i], pbl);
        absorb(1);                                                  // claim_u
        if (mdb != -1) { rounds(L.rv[i], mdb); absorb((uint64_t) i); }
        for (int j = 0; j < n; ++j) draw(L.sig[i] + (uint64_t) j);
        rounds(L.rl[i], pbl);
        absorb(1);                                                  // vr
    }
    return ctr;
}

}  // namespace vph
