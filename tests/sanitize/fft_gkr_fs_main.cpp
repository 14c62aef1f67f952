// TEST INFRASTRUCTURE ONLY.  Sanitizer leg of fft_gkr's part of the Fiat-Shamir chain: the host's derivation (virgo-plus_amd/host/fft_gkr_fs.hpp) and
// fft_gkr_check (fft_gkr_verify.hpp) compiled with -fsanitize=address,undefined into a program of its own (tests/test_fft_gkr_fs_host.py builds
// tests/sanitize/_build/fft_gkr_fs_asan from this file alone: both are header code).  Every array is a heap block of exactly its size, so a read or a write past
// an end is a report.  argv: in = u32 lg | 32-byte state | n_msgs x 16 bytes;  out = the derived tape | the closing state.
#include "../../virgo-plus_amd/host/fft_gkr_fs.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

static int fail(const char *what, long at = -1) { fprintf(stderr, "fft_gkr_fs_asan: %s (%ld)\n", what, at); return 1; }

int main(int argc, char **argv) {
    if (argc < 3) return fail("usage");
    FILE *f = fopen(argv[1], "rb");
    if (!f) return fail("no input");
    uint32_t lg = 0;
    uint8_t state[32];
    if (fread(&lg, 4, 1, f) != 1 || fread(state, 32, 1, f) != 1 || lg < 1 || lg > 19) return fail("header");
    const vph::FftGkrLayout L((int) lg);
    std::unique_ptr<F[]> msgs(new F[L.n_msgs]), tape(new F[L.n_tape]);
    if (fread(static_cast<void *>(msgs.get()), sizeof(F), L.n_msgs, f) != L.n_msgs || fgetc(f) != EOF) return fail("message count");
    fclose(f);
    const F inv_rou = F::getRootOfUnity((int) lg).inv();
    vph::fs_chain ch;
    memcpy(ch.s.w, state, 32);
    vph::fftGkrFsTape((int) lg, ch, msgs.get(), tape.get());
    if (!vph::fft_gkr_check<F>((int) lg, tape.get(), L.n_tape, msgs.get(), L.n_msgs, inv_rou)) return fail("the honest transcript is rejected");
    FILE *o = fopen(argv[2], "wb");
    if (!o || fwrite(static_cast<const void *>(tape.get()), sizeof(F), L.n_tape, o) != L.n_tape || fwrite(ch.s.w, 32, 1, o) != 1) return fail("output");
    fclose(o);
    // one element changed (kept canonical), a stride through the messages and the last one: the derived transcript is rejected, and so is the honest tape
    for (size_t i = 0; i < L.n_msgs; i += (i + 7 < L.n_msgs ? 7 : 1)) {
        std::unique_ptr<F[]> bad(new F[L.n_msgs]), t2(new F[L.n_tape]);
        memcpy(static_cast<void *>(bad.get()), static_cast<const void *>(msgs.get()), L.n_msgs * sizeof(F));
        bad[i].img = (bad[i].img + 1) % F::mod;
        vph::fs_chain c2;
        memcpy(c2.s.w, state, 32);
        vph::fftGkrFsTape((int) lg, c2, bad.get(), t2.get());
        if (!memcmp(c2.s.w, ch.s.w, 32)) return fail("a changed message leaves the closing state", (long) i);
        if (vph::fft_gkr_check<F>((int) lg, t2.get(), L.n_tape, bad.get(), L.n_msgs, inv_rou)) return fail("a changed message is accepted on its derived tape", (long) i);
        if (vph::fft_gkr_check<F>((int) lg, tape.get(), L.n_tape, bad.get(), L.n_msgs, inv_rou)) return fail("a changed message is accepted on the honest tape", (long) i);
    }
    // sizes that are not the layout's are refused before anything is read
    if (vph::fft_gkr_check<F>((int) lg, tape.get(), L.n_tape - 1, msgs.get(), L.n_msgs, inv_rou) || vph::fft_gkr_check<F>((int) lg, tape.get(), L.n_tape, msgs.get(), L.n_msgs - 1, inv_rou))
        return fail("a wrong size is accepted");
    printf("fft_gkr_fs_asan ok\n");
    return 0;
}
