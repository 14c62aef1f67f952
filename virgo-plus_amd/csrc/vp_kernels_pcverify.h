// Kernels of the commitment VERIFIER's two heavy loops (host/verifier.cpp, verifyPoly): the public polynomials' values at the query points
// (vp_pc_public_evals) and the digests of every opening (vp_fri_query_digests).  Both return values; nothing here compares or decides.
#pragma once
#include "vp_kernels_pc.h"

namespace vp {

// ---- q_j(x), q_j(-x) for all query points --------------------------------------------------------------------------------------------
// q(x) = E(y) + x O(y) and q(-x) = E(y) - x O(y) with y = x^2, E = sum_p a[2p] y^p, O = sum_p a[2p + 1] y^p: one product per coefficient and
// point pair.  A workgroup takes a run of PEV_PAIRS coefficient pairs of one row; thread t holds pairs c PEV_PAIRS + t + 256 k, k < PEV_T
// (coalesced 32-byte loads, made ONCE and kept in registers for all points of the workgroup's query group), runs Horner in Y = y^256 over them
// and scales by y^(c PEV_PAIRS + t).  Both powers are one load from the root table: x = w^leaf, so y^e = w^(2 leaf e mod M).  Every product is the
// canonical multiply-add (f_mad_c: canonical first factor, second factor and addend canonical here); block_sum adds the 256 threads' canonical
// terms lazily, and the workgroup's (E, O) goes to part[((row n_q + q) chunks + c) 2 + {0, 1}] for the closing launch.
constexpr u32 PEV_T = 8, PEV_PAIRS = 256 * PEV_T;
struct PolyEvalArgs {
    const F *coef;               // rows x N coefficients
    const F *RT; u32 half_m;     // w^j, j < M / 2
    const u64 *leaf;             // n_q leaves, each < M / 2
    F *part;
    u32 ln, n_q, chunks, q_per_group;
};
__global__ void __launch_bounds__(VP_BLOCK) k_pc_poly_eval(PolyEvalArgs a) {
    __shared__ F lds[8];
    const u32 c = blockIdx.x, row = blockIdx.y, t = threadIdx.x;
    const u32 NP = (1u << a.ln) >> 1, M = 2 * a.half_m;
    const F *co = a.coef + ((size_t) row << a.ln);
    const u32 p0 = c * PEV_PAIRS + t;
    F ev[PEV_T], od[PEV_T];
#pragma unroll
    for (u32 k = 0; k < PEV_T; ++k) {
        const u32 p = p0 + 256 * k;
        ev[k] = f_zero(); od[k] = f_zero();
        if (p < NP) { ev[k] = co[2 * (size_t) p]; od[k] = co[2 * (size_t) p + 1]; }
    }
    const u32 q_end = min(a.n_q, (blockIdx.z + 1) * a.q_per_group);
    for (u32 q = blockIdx.z * a.q_per_group; q < q_end; ++q) {
        const u64 ey = (2 * a.leaf[q]) & (M - 1);                              // y = w^ey
        const F Y = root_pow(a.RT, a.half_m, (u32) ((ey * 256) & (M - 1)));
        const F S = root_pow(a.RT, a.half_m, (u32) ((ey * p0) & (M - 1)));     // y^p0
        F acc[2] = {ev[PEV_T - 1], od[PEV_T - 1]};
#pragma unroll
        for (int k = (int) PEV_T - 2; k >= 0; --k) { acc[0] = f_mad_c(Y, acc[0], ev[k]); acc[1] = f_mad_c(Y, acc[1], od[k]); }
        acc[0] = f_mad_c(S, acc[0], f_zero()); acc[1] = f_mad_c(S, acc[1], f_zero());
        block_sum<2>(acc, lds);
        if (t == 0) {
            F *dst = a.part + (((size_t) row * a.n_q + q) * a.chunks + c) * 2;
            dst[0] = acc[0]; dst[1] = acc[1];
        }
        __syncthreads();                                                       // block_sum's LDS words are free again
    }
}
// The closing launch: thread (q, j) adds the workgroups' partial sums of its row, forms q_j(x) = E + x O and q_j(-x) = E - x O with x = w^leaf, and — in
// the tensor form, where ONE row was evaluated — scales both by slice j's factor.  out[(q 2 + h) 64 + j], canonical.
__global__ void __launch_bounds__(VP_BLOCK) k_pc_poly_eval_fin(PolyEvalArgs a, const F *__restrict__ slice_scale /* 64, or null: 64 rows */, F *__restrict__ out) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n_q * 64) return;
    const u32 q = g >> 6, j = g & 63, row = slice_scale ? 0 : j;
    const F *src = a.part + ((size_t) row * a.n_q + q) * a.chunks * 2;
    F e = f_zero(), o = f_zero();
    for (u32 c = 0; c < a.chunks; ++c) { e = f_add(e, src[2 * c]); o = f_add(o, src[2 * c + 1]); }
    const F x = root_pow(a.RT, a.half_m, (u32) (a.leaf[q] & (2 * a.half_m - 1)));
    const F xo = f_mad_c(x, o, f_zero());
    F v0 = f_add(e, xo), v1 = f_sub(e, xo);
    if (slice_scale) { const F s = slice_scale[j]; v0 = f_mad_c(s, v0, f_zero()); v1 = f_mad_c(s, v1, f_zero()); }
    out[((size_t) q * 2) * 64 + j] = v0;
    out[((size_t) q * 2 + 1) * 64 + j] = v1;
}

// The closing launch of the mask row (vp_pc_mask_evals): k_pc_poly_eval ran over ONE row of 2^a.ln coefficients (the public mask polynomial; its length is
// independent of the domain 2 a.half_m), thread q adds that row's partial sums and writes out[2 q] = E + x O, out[2 q + 1] = E - x O, canonical.
__global__ void __launch_bounds__(VP_BLOCK) k_pc_mask_eval_fin(PolyEvalArgs a, F *__restrict__ out) {
    const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.n_q) return;
    const F *src = a.part + (size_t) q * a.chunks * 2;
    F e = f_zero(), o = f_zero();
    for (u32 c = 0; c < a.chunks; ++c) { e = f_add(e, src[2 * c]); o = f_add(o, src[2 * c + 1]); }
    const F x = root_pow(a.RT, a.half_m, (u32) (a.leaf[q] & (2 * a.half_m - 1)));
    const F xo = f_mad_c(x, o, f_zero());
    out[2 * (size_t) q] = f_add(e, xo);
    out[2 * (size_t) q + 1] = f_sub(e, xo);
}

// ---- digests of every opening of a query answer ------------------------------------------------------------------------------------------
// `buf` = leaf0[n_q] (8 bytes each) followed by the answer in vp_fri_query's layout: per query, oracle 0, oracle 1, level 0 .. ln - 1, each 130
// values (2080 bytes) + its path (n - 1 digests for the two first oracles, n - 2 - k for level k; the last one, the prover's copy of the leaf
// digest, is not read).  An opening is ONE chain of 65 + depth dependent Keccak-f: there is nothing to share between lanes, so a lane takes an
// opening (the compiler's block function, as k_leaf_hash_c) and the workgroups are single waves, so that the few hundred chains of a protocol
// run spread over as many SIMDs.  out: 64 bytes per opening — leaf-chain digest | root reached through path[0 .. depth).
constexpr u32 POD_THREADS = 64;
__global__ void __launch_bounds__(POD_THREADS) k_pc_opening_digests(const u64 *__restrict__ buf, u32 n, u32 n_q, u64 per_query /* bytes */, Dig *__restrict__ out) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 ln = n - 6, per = ln + 2;
    if (g >= n_q * per) return;
    const u32 q = g / per, o = g % per;
    u64 leaf = buf[q], off, depth;
    const u64 first = 2080 + 32ull * (n - 1);
    if (o < 2) { off = o * first; depth = n - 2; }
    else {
        const u64 k = o - 2;
        off = 2 * first + k * 2080 + 32 * (k * (n - 2) - k * (k - 1) / 2);
        depth = n - 3 - k;
        u64 D = 1ull << (n - 1);
        for (u64 i = 0; i <= k; ++i) { D >>= 1; leaf &= (D >> 1) - 1; }            // t mod (Dn / 2), level by level
    }
    const u64 *v = buf + n_q + (q * per_query + off) / 8;
    Dig h; h.w[0] = h.w[1] = h.w[2] = h.w[3] = 0;
    for (int s = 0; s < 65; ++s) h = hhash64(v[4 * s], v[4 * s + 1], v[4 * s + 2], v[4 * s + 3], h);
    out[2 * (size_t) g] = h;
    const u64 *path = v + 260;
    for (u64 k = 0; k < depth; ++k) {
        Dig sib; sib.w[0] = path[4 * k]; sib.w[1] = path[4 * k + 1]; sib.w[2] = path[4 * k + 2]; sib.w[3] = path[4 * k + 3];
        const bool odd = (leaf >> k) & 1;
        const Dig m = odd ? sib : h, st = odd ? h : sib;                          // node = H(left || right)
        h = hhash64(m.w[0], m.w[1], m.w[2], m.w[3], st);
    }
    out[2 * (size_t) g + 1] = h;
}

}  // namespace vp
