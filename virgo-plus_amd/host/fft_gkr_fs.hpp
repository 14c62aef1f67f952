// fft_gkr's part of the Fiat-Shamir chain (its text: vphost.h, "The transcript chain: fft_gkr"): the tape vp_fft_gkr_fs draws on the device, derived on the
// host from the messages it returned.  One walk for the prover's cross-check and for a verifier that holds only the messages.
#pragma once
#include <cstdint>

#include "fft_gkr_verify.hpp"
#include "field.hpp"
#include "sha3.hpp"

namespace vph {

// From the chain's state in ch: tape[0 .. n_tape) of FftGkrLayout(lg) from msgs[0 .. n_msgs) in vp_fft_gkr's layout; ch ends in the closing state.
inline void fftGkrFsTape(int lg, fs_chain &ch, const F *msgs, F *tape) {
    const FftGkrLayout L(lg);
    auto draw = [&](size_t slot) { uint64_t a, b; ch.challenge((uint64_t) slot, a, b); tape[slot].real = a; tape[slot].img = b; };
    auto absorb = [&](const F &x) { ch.elem(x.real, x.img); };
    size_t pos = 0;
    // rounds of one sumcheck (challenge k in slot slot0 + k), then its closing value
    auto sumcheck = [&](int rounds, size_t slot0) {
        for (int k = 0; k < rounds; ++k) {
            for (int t = 0; t < 3; ++t) absorb(msgs[pos++]);
            draw(slot0 + k);
        }
        absorb(msgs[pos++]);
    };
    for (size_t i = 0; i < (size_t) lg + 64; ++i) draw(L.r + i);                        // r, then x
    for (int i = 0; i < 64; ++i) absorb(msgs[pos++]);                                   // the outputs
    for (size_t i = 0; i < 2 * ((size_t) lg + 10); ++i) draw(L.r0 + i);                 // r_0, then r_1
    sumcheck(lg + 6, L.ru_a);                                                           // addition layer; its r_v multiply beta = 0 and are drawn all the same
    for (int k = 0; k < lg + 6; ++k) draw(L.rv_a + k);
    sumcheck(lg, L.ru_m);                                                               // multiplication layer
    for (int k = 0; k < lg; ++k) draw(L.rv_m + k);
    for (int d = 0; d < lg; ++d) {
        sumcheck(lg, L.ru_d(d));
        sumcheck(lg, L.rv_d(d));
        draw(L.alpha_d(d));
        draw(L.beta_d(d));
    }
}

}  // namespace vph
