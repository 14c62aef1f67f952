// vp_prove_gkr_fs: the GKR sumchecks with every challenge drawn on the device (the schedule: host/vphost.h, "The GKR part on the device").
// Part of the single translation unit vpgpu.hip.  The rounds are the per-round kernels of vp_kernels_round.h (round_main_body, round_final_tail) with one more
// step on the closing lane: it absorbs the polynomial it has just written and draws the challenge the NEXT round reads through RoundArgs::rp.  The chain is
// fft_gkr's (fg_fs_elem / fg_fs_challenge, vp_kernels_fftgkr.h: one dependent Keccak-f per step, one lane); what differs is the counter, which here runs from
// 0 over the draws of the call and lives beside the state in device memory.
#pragma once
#include "vp_kernels_fftgkr.h"
#include "vp_kernels_round.h"

namespace vp {

// chain of one vp_prove_gkr_fs call: the state and the counter of the next draw (one 64-byte block: it travels back with the transcript and the tape)
struct GkrFs { Dig s; unsigned long long ctr; unsigned long long pad[3]; };

// the closing lane of a round: E(a), E(b), E(c), *slot = C(counter)
__device__ __forceinline__ void gkr_fs_close(const F *poly, GkrFs *fs, F *slot) {
    Dig s = fs->s;
    const unsigned long long c = fs->ctr;
    for (int t = 0; t < 3; ++t) s = fg_fs_elem(s, poly[t]);
    F r; s = fg_fs_challenge(s, c, &r);
    *slot = r;
    fs->s = s; fs->ctr = c + 1;
}

// One lane: E(absorb[i]), i < n_absorb, then slot[k] = C(counter), k < n_draw.  Covers the opening r_liu draws, E(Vres) and assert_random, the claims behind
// k_finalize and the sig draws.
__global__ void k_gkr_fs_span(GkrFs *fs, const F *__restrict__ absorb, u32 n_absorb, F *__restrict__ slot, u32 n_draw) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Dig s = fs->s;
    unsigned long long c = fs->ctr;
    for (u32 i = 0; i < n_absorb; ++i) s = fg_fs_elem(s, absorb[i]);
    for (u32 k = 0; k < n_draw; ++k) { F r; s = fg_fs_challenge(s, c++, &r); slot[k] = r; }
    fs->s = s; fs->ctr = c;
}

// k_round_fused with the chain step behind its closing
__global__ void __launch_bounds__(VP_BLOCK) k_round_fused_fs(RoundArgs a, F *add_term, F *scalarV, F *poly_dev, GkrFs *fs, F *slot) {
    __shared__ F lds[12];
    F acc[3] = {f_zero(), f_zero(), f_zero()};
    round_main_body(a, 0, 1, acc, lds);
    if (threadIdx.x != 0) return;
    round_final_tail(a, acc, add_term, scalarV, poly_dev, nullptr, nullptr, 0);
    gkr_fs_close(poly_dev, fs, slot);
}
// k_round_final with the chain step
__global__ void __launch_bounds__(VP_BLOCK) k_round_final_fs(RoundArgs a, RoundOut o, GkrFs *fs, F *slot) {
    if (threadIdx.x != 0) return;
    const F z[3] = {f_zero(), f_zero(), f_zero()};
    round_final_tail(a, z, o.add_term, o.scalarV, o.poly_dev, nullptr, nullptr, 0);
    gkr_fs_close(o.poly_dev, fs, slot);
}
// k_round_main with the chain step: the arrival scheme is k_round_main's (see there for the ordering of the hand-off), and lane 0 of the workgroup that
// arrives last does the chain steps behind round_final_tail.  The challenge it stores is read by the next LAUNCH on the stream, never inside this one.
__global__ void __launch_bounds__(VP_BLOCK) k_round_main_fs(RoundArgs a, F *__restrict__ part, unsigned int *__restrict__ arrivals, RoundOut o, GkrFs *fs, F *slot) {
    __shared__ F lds[12];
    __shared__ int s_last;
    F acc[3] = {f_zero(), f_zero(), f_zero()};
    round_main_body(a, blockIdx.x, gridDim.x, acc, lds);
    if (threadIdx.x == 0) {
        unsigned long long *w = reinterpret_cast<unsigned long long *>(part + (size_t) blockIdx.x * 3);
        cf_st(w, acc[0].re); cf_st(w + 1, acc[0].im); cf_st(w + 2, acc[1].re); cf_st(w + 3, acc[1].im); cf_st(w + 4, acc[2].re); cf_st(w + 5, acc[2].im);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // the sums are out before they are counted
        s_last = __hip_atomic_fetch_add(arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;                                                       // uniform per workgroup
    F t[3] = {f_zero(), f_zero(), f_zero()};
    for (u32 i = threadIdx.x; i < gridDim.x; i += blockDim.x) {
        const unsigned long long *w = reinterpret_cast<const unsigned long long *>(part + (size_t) i * 3);
        t[0] = f_add(t[0], f_make(cf_ld(w), cf_ld(w + 1)));
        t[1] = f_add(t[1], f_make(cf_ld(w + 2), cf_ld(w + 3)));
        t[2] = f_add(t[2], f_make(cf_ld(w + 4), cf_ld(w + 5)));
    }
    __syncthreads();                                                           // lds is free again
    block_sum<3>(t, lds);
    if (threadIdx.x != 0) return;
    __hip_atomic_store(arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    round_final_tail(a, t, o.add_term, o.scalarV, o.poly_dev, nullptr, nullptr, 0);
    gkr_fs_close(o.poly_dev, fs, slot);
}

// The end of the call: transcript | tape | chain (state, counter) written side by side into pinned host memory, the one copy of the call (k_ship's way: the
// three live in different device arrays; the caller waits for the stream behind it).
__global__ void __launch_bounds__(VP_BLOCK) k_gkr_fs_ship(const F *__restrict__ tr, u32 n_tr, const F *__restrict__ tape, u32 n_tape, const GkrFs *__restrict__ fs, F *__restrict__ host) {
    const u32 n_fs = (u32) (sizeof(GkrFs) / sizeof(F)), total = n_tr + n_tape + n_fs;
    const F *fsw = reinterpret_cast<const F *>(fs);
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x)
        host[i] = i < n_tr ? tr[i] : i < n_tr + n_tape ? tape[i - n_tr] : fsw[i - n_tr - n_tape];
}

}  // namespace vp
