// fft_gkr on the device: the circuit and the sumcheck tables of lib/virgo's fft_circuit_gkr
// (lib/virgo/src/fft_circuit_GKR.cpp:22-849).  Part of the single translation unit vpgpu.hip.
//
// The circuit:  r[lg] -> E = eq-expansion of r (2^lg values, :24-32) -> lg butterfly layers of the inverse FFT (:34-65) -> scaling by
// 1/n (:66-71) -> 64 * 2^lg products S[j] * x_i^j (:79-90) -> 64 sums (:91-100).  Every layer is a dense array of F in HBM; all of them
// are kept (the layer below a butterfly layer is the V table of that depth's two sumchecks).  The sumchecks themselves run through the
// fold / segment / closing kernels of the GKR path (run_sumcheck_seg): what is specific to fft_gkr is only how the mult / add tables
// of each sumcheck are written — closed forms over the butterfly wiring, one element per thread, no gathers beyond the partner entry.
// All kernels: one thread per element, consecutive lanes on consecutive 16-byte elements.
#pragma once
#include <hip/hip_runtime.h>
#include "vp_field.h"
#include "vp_kernels_round.h"
#include "vp_kernels_pc.h"

namespace vp {

// E[g] = prod_i (bit (lg-1-i) of g ? 1 - r[i] : r[i])   (fft_circuit_GKR.cpp:24-32: level i appends its bit at the bottom, 0 <-> r[i])
__global__ void __launch_bounds__(VP_BLOCK) k_fg_expand(const F *__restrict__ r, int lg, F *__restrict__ out) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (1u << lg)) return;
    F acc = f_one();
    for (int i = 0; i < lg; ++i) {
        const F ri = r[i];
        acc = f_mul(acc, ((g >> (lg - 1 - i)) & 1u) ? f_sub(f_one(), ri) : ri);
    }
    out[g] = acc;
}

// out[t] = w^t for t < n, given sq[b] = w^(2^b): the powers the butterflies (x_k = w^(k 2^dep)) and the table inits use
__global__ void __launch_bounds__(VP_BLOCK) k_fg_pows(const F *__restrict__ sq, int nbits, u32 n, F *__restrict__ out) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    F acc = f_one();
    for (int b = 0; b < nbits; ++b) if ((t >> b) & 1u) acc = f_mul(acc, sq[b]);
    out[t] = acc;
}

// One butterfly layer (:44-64): pair p = (k, j), j < 2^dep:  l = pre[k << (dep+1) | j], rr = w^(k 2^dep) * pre[k << (dep+1) | 2^dep | j];
// cur[k << dep | j] = l + rr, cur[(k + half) << dep | j] = l - rr.  winv[t] = inv_rou^t, t < N/2.  `scaled` (last layer only): cur * inv_n.
__global__ void __launch_bounds__(VP_BLOCK) k_fg_butterfly(const F *__restrict__ pre, F *__restrict__ cur, const F *__restrict__ winv, int lg, int dep,
                                                          F *__restrict__ scaled, F inv_n) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x, halfN = 1u << (lg - 1);
    if (p >= halfN) return;
    const u32 J = 1u << dep, j = p & (J - 1), k = p >> dep, half = halfN >> dep;
    const F l = pre[(k << (dep + 1)) | j];
    const F rr = f_mul(winv[k << dep], pre[(k << (dep + 1)) | J | j]);
    const F a = f_add(l, rr), b = f_sub(l, rr);
    cur[(k << dep) | j] = a;
    cur[((k + half) << dep) | j] = b;
    if (scaled) { scaled[(k << dep) | j] = f_mul(a, inv_n); scaled[((k + half) << dep) | j] = f_mul(b, inv_n); }
}

// xsq[i * lg + b] = x_i^(2^b), i < 64
__global__ void k_fg_xsq(const F *__restrict__ xs, int lg, F *__restrict__ xsq) {
    const int i = threadIdx.x;
    if (i >= 64) return;
    F x = xs[i];
    for (int b = 0; b < lg; ++b) { xsq[i * lg + b] = x; x = f_mul(x, x); }
}
__device__ __forceinline__ F fg_xpow(const F *__restrict__ xsq_i, int lg, u32 j) {       // x_i^j from the squarings
    F acc = f_one();
    for (int b = 0; b < lg; ++b) if ((j >> b) & 1u) acc = f_mul(acc, xsq_i[b]);
    return acc;
}
// Powers of the 64 points by table (round 4): x_i^j = Q_i[j >> lb] * P_i[j & (2^lb - 1)], lb = min(lg, 9) — two multiplications per power instead of one per
// set bit of j.  xt: [64][2^lb] P then [64][2^(lg - lb)] Q.
__device__ __forceinline__ int fg_lb(int lg) { return lg < 9 ? lg : 9; }
__global__ void __launch_bounds__(VP_BLOCK) k_fg_xtab(const F *__restrict__ xsq, int lg, F *__restrict__ xt) {
    const int lb = fg_lb(lg), hb = lg - lb;
    const u32 nP = 64u << lb, nQ = 64u << hb, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nP) { const u32 i = t >> lb, b = t & ((1u << lb) - 1); xt[t] = fg_xpow(xsq + i * lg, lg, b); }
    else if (t < nP + nQ) { const u32 q = t - nP, i = q >> hb, a = q & ((1u << hb) - 1); xt[t] = fg_xpow(xsq + i * lg, lg, a << lb); }
}
__device__ __forceinline__ F fg_xpow_tab(const F *__restrict__ xt, int lg, u32 i, u32 j) {
    const int lb = fg_lb(lg), hb = lg - lb;
    const F p = xt[((size_t) i << lb) | (j & ((1u << lb) - 1))];
    return hb ? f_mul(xt[((size_t) 64 << lb) + ((size_t) i << hb) + (j >> lb)], p) : p;
}
// Pm[i << lg | j] = S[j] * x_i^j (:79-90), and the block's share of O[i] = sum_j Pm[i << lg | j] (:91-100): grid (ceil(N / 256), 64)
__global__ void __launch_bounds__(VP_BLOCK) k_fg_polyeval(const F *__restrict__ S, const F *__restrict__ xt, int lg, F *__restrict__ Pm, F *__restrict__ part) {
    __shared__ F lds[4];
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, N = 1u << lg;
    F v[1] = {f_zero()};
    if (j < N) { v[0] = f_mul(S[j], fg_xpow_tab(xt, lg, i, j)); Pm[((size_t) i << lg) | j] = v[0]; }
    block_sum<1>(v, lds);
    if (threadIdx.x == 0) part[(size_t) i * gridDim.x + blockIdx.x] = v[0];
}
__global__ void __launch_bounds__(VP_BLOCK) k_fg_rowsum(const F *__restrict__ part, u32 nb, F *__restrict__ O) {      // one block per output
    __shared__ F lds[4];
    F v[1] = {f_zero()};
    for (u32 b = threadIdx.x; b < nb; b += blockDim.x) v[0] = f_add(v[0], part[(size_t) blockIdx.x * nb + b]);
    block_sum<1>(v, lds);
    if (threadIdx.x == 0) O[blockIdx.x] = v[0];
}

// g[x] = alpha * eq(r0, x) + beta * eq(r1, x), x < 2^n, bit b of x set <-> r[b] (the beta_g half tables, :193-216).  alpha / beta are device
// pointers into the tape; NULL alpha = 1, NULL beta = 0 (engage_gkr starts with alpha = 1, beta = 0, :775-776: the r1 term is then absent).
__global__ void __launch_bounds__(VP_BLOCK) k_fg_gtab(const F *__restrict__ r0, const F *__restrict__ r1, int n, const F *__restrict__ alpha,
                                                     const F *__restrict__ beta, F *__restrict__ out) {
    const u32 x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= (1u << n)) return;
    F a = alpha ? *alpha : f_one();
    for (int b = 0; b < n; ++b) { const F rb = r0[b]; a = f_mul(a, ((x >> b) & 1u) ? rb : f_sub(f_one(), rb)); }
    if (beta) {
        F c = *beta;
        for (int b = 0; b < n; ++b) { const F rb = r1[b]; c = f_mul(c, ((x >> b) & 1u) ? rb : f_sub(f_one(), rb)); }
        a = f_add(a, c);
    }
    out[x] = a;
}

// addition layer (:231-236): mult[j] = g6[j >> lg] over the 64 * 2^lg products; the add table is identically zero (has_a = 0)
__global__ void __launch_bounds__(VP_BLOCK) k_fg_add_init(const F *__restrict__ g6, int lg, F *__restrict__ M) {
    const size_t j = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ((size_t) 64 << lg)) return;
    M[j] = g6[j >> lg];
}
// multiplication layer (:347-359) with alpha = 1, beta = 0:  mult[i] = sum_j g(j 2^lg + i) x_j^i = lo[i] * sum_j hi[j] x_j^i, g = eq(r0, .) split
// into lo = eq(r0[0..lg), .) and hi = eq(r0[lg..lg+6), .)
__global__ void __launch_bounds__(VP_BLOCK) k_fg_mul_init(const F *__restrict__ lo, const F *__restrict__ hi, const F *__restrict__ xt, int lg, F *__restrict__ M) {
    __shared__ F s_hi[64];
    if (threadIdx.x < 64) s_hi[threadIdx.x] = hi[threadIdx.x];
    __syncthreads();
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << lg)) return;
    F acc = f_zero();
    for (int j = 0; j < 64; ++j) acc = f_add(acc, f_mul(s_hi[j], fg_xpow_tab(xt, lg, (u32) j, i)));
    M[i] = f_mul(lo[i], acc);
}

// inverse-FFT depth `dep`, phase 1 (:516-539): for the pair p = (k, j): u = k << (dep+1) | j, v = u | 2^dep, g1 = k << dep | j, g2 = (k + half) << dep | j;
//   mult[u] = g[g1] + g[g2],  add[u] = (g[g1] - g[g2]) * w^(k 2^dep) * pre[v],  mult[v] = add[v] = 0
__global__ void __launch_bounds__(VP_BLOCK) k_fg_ifft_p1(const F *__restrict__ g, const F *__restrict__ pre, const F *__restrict__ winv, int lg, int dep,
                                                        F *__restrict__ M, F *__restrict__ A) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x, halfN = 1u << (lg - 1);
    if (p >= halfN) return;
    const u32 J = 1u << dep, j = p & (J - 1), k = p >> dep, half = halfN >> dep;
    const u32 u = (k << (dep + 1)) | j, v = u | J;
    const F t1 = g[(k << dep) | j], t2 = g[((k + half) << dep) | j];
    M[u] = f_add(t1, t2);
    A[u] = f_mul(f_mul(f_sub(t1, t2), winv[k << dep]), pre[v]);
    M[v] = f_zero(); A[v] = f_zero();
}
// phase 2 (:574-606): mult[v] = (g[g1] - g[g2]) * eq(r_u, u) * w^(k 2^dep),  add[v] = (g[g1] + g[g2]) * eq(r_u, u) * v_u,  mult[u] = add[u] = 0.
// v_u = the claim phase 1 ended with (device pointer: the closing kernel of that sumcheck wrote it).
__global__ void __launch_bounds__(VP_BLOCK) k_fg_ifft_p2(const F *__restrict__ g, const F *__restrict__ eu, const F *__restrict__ vu, const F *__restrict__ winv,
                                                        int lg, int dep, F *__restrict__ M, F *__restrict__ A) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x, halfN = 1u << (lg - 1);
    if (p >= halfN) return;
    const u32 J = 1u << dep, j = p & (J - 1), k = p >> dep, half = halfN >> dep;
    const u32 u = (k << (dep + 1)) | j, v = u | J;
    const F t1 = g[(k << dep) | j], t2 = g[((k + half) << dep) | j], e = eu[u];
    M[v] = f_mul(f_mul(f_sub(t1, t2), e), winv[k << dep]);
    A[v] = f_mul(f_mul(f_add(t1, t2), e), *vu);
    M[u] = f_zero(); A[u] = f_zero();
}

// ---- the 2 lg sumchecks of the inverse FFT as ONE batch (round 4) ------------------------------------------------------------------------------
// Given the tape they are independent of each other: depth d's tables come from the layer values (all kept), from eq tables of tape entries, and — phase 2 —
// from v_u = the layer's extension at r_u, which is an inner product with eq(r_u, .) instead of phase 1's last fold.  The kernels above, one job per blockIdx.y:
struct FgTabJob { const F *r0, *r1, *alpha, *beta; F *out; };
__global__ void __launch_bounds__(VP_BLOCK) k_fg_gtab_multi(const FgTabJob *__restrict__ jobs, int n) {
    const FgTabJob j = jobs[blockIdx.y];
    const u32 x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= (1u << n)) return;
    F a = j.alpha ? *j.alpha : f_one();
    for (int b = 0; b < n; ++b) { const F rb = j.r0[b]; a = f_mul(a, ((x >> b) & 1u) ? rb : f_sub(f_one(), rb)); }
    if (j.beta) {
        F c = *j.beta;
        for (int b = 0; b < n; ++b) { const F rb = j.r1[b]; c = f_mul(c, ((x >> b) & 1u) ? rb : f_sub(f_one(), rb)); }
        a = f_add(a, c);
    }
    j.out[x] = a;
}
struct FgDotJob { const F *x, *y; F *out; };
__global__ void __launch_bounds__(VP_BLOCK) k_fg_dot_multi(const FgDotJob *__restrict__ jobs, u32 n) {      // one workgroup per inner product (2^lg <= 2^20 terms)
    __shared__ F lds[4];
    const FgDotJob j = jobs[blockIdx.x];
    F v[1] = {f_zero()};
    for (u32 i = threadIdx.x; i < n; i += blockDim.x) v[0] = f_add(v[0], f_mul(j.x[i], j.y[i]));
    block_sum<1>(v, lds);
    if (threadIdx.x == 0) *j.out = v[0];
}
struct FgIfftJob { const F *g, *pre, *eu, *vu; F *M, *A; int dep, phase; };
__global__ void __launch_bounds__(VP_BLOCK) k_fg_ifft_multi(const FgIfftJob *__restrict__ jobs, const F *__restrict__ winv, int lg) {
    const FgIfftJob jb = jobs[blockIdx.y];
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x, halfN = 1u << (lg - 1);
    if (p >= halfN) return;
    const int dep = jb.dep;
    const u32 J = 1u << dep, j = p & (J - 1), k = p >> dep, half = halfN >> dep;
    const u32 u = (k << (dep + 1)) | j, v = u | J;
    const F t1 = jb.g[(k << dep) | j], t2 = jb.g[((k + half) << dep) | j];
    if (jb.phase == 1) {                                                   // k_fg_ifft_p1
        jb.M[u] = f_add(t1, t2);
        jb.A[u] = f_mul(f_mul(f_sub(t1, t2), winv[k << dep]), jb.pre[v]);
        jb.M[v] = f_zero(); jb.A[v] = f_zero();
    } else {                                                               // k_fg_ifft_p2
        const F e = jb.eu[u];
        jb.M[v] = f_mul(f_mul(f_sub(t1, t2), e), winv[k << dep]);
        jb.A[v] = f_mul(f_mul(f_add(t1, t2), e), *jb.vu);
        jb.M[u] = f_zero(); jb.A[u] = f_zero();
    }
}

// ---- vp_fft_gkr_fs: the sumchecks with every challenge drawn on the device (the chain's text: host/vphost.h) -------------------------------------
// A challenge depends on the polynomial before it, so the rounds cannot share a launch the way k_sumfold3b / k_seg share them: a round is one launch on
// every workgroup (k_fg_fs_round: fold by the challenge in its tape slot, sum the round's (a, b, c) into per-workgroup partials) and a closing launch on one
// workgroup (k_fg_fs_close: sum the partials, write the polynomial, absorb it, draw), until the tables fit LDS; from there one launch of one workgroup runs
// every round that is left (k_fg_fs_tail).  The chain itself is one lane's work (fs_absorb_draw's form: a dependent Keccak-f per step).
constexpr int fg_fs_log2_floor(size_t x) { return x <= 1 ? 0 : 1 + fg_fs_log2_floor(x >> 1); }
constexpr int FG_FS_TABLES = 3;                                                   // V, M and (inverse-FFT layers) A
constexpr size_t FG_FS_LDS = 160 * 1024;                                          // per workgroup on gfx950
constexpr int FG_FS_TAIL_LOG = fg_fs_log2_floor((FG_FS_LDS - 1024) / (FG_FS_TABLES * sizeof(F)));      // 1 KB kept for the reduction scratch and the challenge
#ifdef VP_FFT_GKR_FS_TAIL_LOG
static_assert(FG_FS_TAIL_LOG == VP_FFT_GKR_FS_TAIL_LOG, "include/vpgpu.h: VP_FFT_GKR_FS_TAIL_LOG");
#endif
constexpr u32 FG_FS_TAIL_N = 1u << FG_FS_TAIL_LOG;
constexpr int FG_FS_TAIL_PER = (int) (FG_FS_TAIL_N / 2 / VP_BLOCK) > 0 ? (int) (FG_FS_TAIL_N / 2 / VP_BLOCK) : 1;      // fold outputs per thread and table

__device__ __noinline__ Dig fg_fs_step(u64 m0, u64 m1, u64 m2, u64 m3, Dig s) { return hhash64(m0, m1, m2, m3, s); }
__device__ __forceinline__ Dig fg_fs_elem(const Dig &s, const F &x) { return fg_fs_step(x.re, x.im, 0, 0x4d, s); }                 // E(x)
__device__ __forceinline__ Dig fg_fs_challenge(const Dig &s, u64 counter, F *out) {                                                // C(counter)
    const Dig t = fg_fs_step(counter, 0, 0, 0x43, s);
    *out = f_make(fs_limb(t.w[0]), fs_limb(t.w[1]));
    return t;
}
// One lane: E(absorb[i]), i < n_absorb, then tape[slot] = C(slot) for first <= slot < first + count.
__global__ void k_fg_fs_draw(Dig *state, const F *__restrict__ absorb, u32 n_absorb, F *__restrict__ tape, u32 first, u32 count) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Dig s = *state;
    for (u32 i = 0; i < n_absorb; ++i) s = fg_fs_elem(s, absorb[i]);
    for (u32 k = first; k < first + count; ++k) { F r; s = fg_fs_challenge(s, k, &r); tape[k] = r; }
    *state = s;
}
// one pair of one round: (m0 + t dm)(v0 + t dv) + a0 + t da, summed into acc = (a, b, c) of a t^2 + b t + c
template <bool HAS_A>
__device__ __forceinline__ void fg_fs_pair(const F &v0, const F &v1, const F &m0, const F &m1, const F &a0, const F &a1, F (&acc)[3]) {
    const F dv = f_sub(v1, v0), dm = f_sub(m1, m0);
    acc[0] = f_add(acc[0], f_mul(dm, dv));
    F b = f_dot2cc<VP_MADSHIFT != 0>(dm, v0, m0, dv), c = f_mul(m0, v0);
    if (HAS_A) { b = f_add(b, f_sub(a1, a0)); c = f_add(c, a0); }
    acc[1] = f_add(acc[1], b);
    acc[2] = f_add(acc[2], c);
}
// A round above the tail.  fold = 0 (round 1): the tables are read as they are, n entries each.  fold = 1: entry i of the out tables is the pair (2 i, 2 i + 1) of
// the in tables folded by *r (the challenge of the round before, in its tape slot), n entries come out.  Either way the n / 2 pairs of the n entries are summed:
// part[3 b .. 3 b + 3) = workgroup b's share of (a, b, c).
struct FgFsRound { const F *inV, *inM, *inA; F *outV, *outM, *outA; const F *r; F *part; u32 n; int fold; };
template <bool HAS_A>
__global__ void __launch_bounds__(VP_BLOCK) k_fg_fs_round(FgFsRound a) {
    __shared__ F lds[12];
    F acc[3] = {f_zero(), f_zero(), f_zero()};
    const u32 pairs = a.n >> 1;
    const F r = a.fold ? *a.r : f_zero();
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += gridDim.x * blockDim.x) {
        F v0, v1, m0, m1, a0 = f_zero(), a1 = f_zero();
        if (a.fold) {
            const size_t q = (size_t) 4 * i;
            v0 = fold_entry(a.inV[q], a.inV[q + 1], r); v1 = fold_entry(a.inV[q + 2], a.inV[q + 3], r);
            m0 = fold_entry(a.inM[q], a.inM[q + 1], r); m1 = fold_entry(a.inM[q + 2], a.inM[q + 3], r);
            a.outV[2 * (size_t) i] = v0; a.outV[2 * (size_t) i + 1] = v1;
            a.outM[2 * (size_t) i] = m0; a.outM[2 * (size_t) i + 1] = m1;
            if (HAS_A) {
                a0 = fold_entry(a.inA[q], a.inA[q + 1], r); a1 = fold_entry(a.inA[q + 2], a.inA[q + 3], r);
                a.outA[2 * (size_t) i] = a0; a.outA[2 * (size_t) i + 1] = a1;
            }
        } else {
            const size_t q = (size_t) 2 * i;
            v0 = a.inV[q]; v1 = a.inV[q + 1]; m0 = a.inM[q]; m1 = a.inM[q + 1];
            if (HAS_A) { a0 = a.inA[q]; a1 = a.inA[q + 1]; }
        }
        fg_fs_pair<HAS_A>(v0, v1, m0, m1, a0, a1, acc);
    }
    block_sum<3>(acc, lds);
    if (threadIdx.x == 0) { a.part[3 * blockIdx.x] = acc[0]; a.part[3 * blockIdx.x + 1] = acc[1]; a.part[3 * blockIdx.x + 2] = acc[2]; }
}
// The round's closing step, one workgroup: the polynomial = the sum of the nb partials -> poly[0..3); E(a), E(b), E(c); tape[slot] = C(slot).
__global__ void __launch_bounds__(VP_BLOCK) k_fg_fs_close(const F *__restrict__ part, u32 nb, F *__restrict__ poly, Dig *state, F *__restrict__ tape, u32 slot) {
    __shared__ F lds[12];
    F acc[3] = {f_zero(), f_zero(), f_zero()};
    for (u32 b = threadIdx.x; b < nb; b += blockDim.x) { acc[0] = f_add(acc[0], part[3 * b]); acc[1] = f_add(acc[1], part[3 * b + 1]); acc[2] = f_add(acc[2], part[3 * b + 2]); }
    block_sum<3>(acc, lds);
    if (threadIdx.x == 0) {
        Dig s = *state;
        for (int t = 0; t < 3; ++t) { poly[t] = acc[t]; s = fg_fs_elem(s, acc[t]); }
        F r; s = fg_fs_challenge(s, slot, &r);
        tape[slot] = r;
        *state = s;
    }
}
// The tail of a sumcheck (or all of it), one workgroup, tables of n = 2^rounds <= 2^FG_FS_TAIL_LOG entries in LDS.  r_fold null: the tables are read as they are;
// else entry i is the pair (2 i, 2 i + 1) of the in tables folded by *r_fold.  Per round k < rounds: (a, b, c) -> poly[3 k ..), E(a), E(b), E(c),
// tape[slot0 + k] = C(slot0 + k), the workgroup folds by it.  Then v = V[0] -> poly[3 rounds], E(v), and tape[slot] = C(slot) for the n_extra slots from extra0
// (the one-phase layers' r_v; alpha and beta behind a depth's second phase).
// Launch contract: ONE workgroup of VP_BLOCK threads (block_sum and the in-place fold are written for it), n = 2^rounds <= 2^FG_FS_TAIL_LOG, dynamic LDS of
// FG_FS_TABLES * sizeof(F) * n bytes; a launch outside it does nothing.
static_assert(FG_FS_TAIL_PER * VP_BLOCK * 2 >= (int) FG_FS_TAIL_N, "k_fg_fs_tail: a thread folds FG_FS_TAIL_PER pairs per table");
struct FgFsTail { const F *inV, *inM, *inA, *r_fold; F *poly; Dig *state; F *tape; u32 n, slot0, extra0, n_extra; int rounds; };
template <bool HAS_A>
__global__ void __launch_bounds__(VP_BLOCK) k_fg_fs_tail(FgFsTail a) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    __shared__ F lds[12];
    __shared__ F s_r;
    if (blockDim.x != VP_BLOCK || blockIdx.x != 0 || a.n > FG_FS_TAIL_N || a.n != (1u << a.rounds)) return;      // the launch contract above
    F *V = reinterpret_cast<F *>(smem_raw), *M = V + a.n, *A = M + a.n;
    const F rf = a.r_fold ? *a.r_fold : f_zero();
    for (u32 i = threadIdx.x; i < a.n; i += blockDim.x) {
        if (a.r_fold) {
            V[i] = fold_entry(a.inV[2 * (size_t) i], a.inV[2 * (size_t) i + 1], rf);
            M[i] = fold_entry(a.inM[2 * (size_t) i], a.inM[2 * (size_t) i + 1], rf);
            if (HAS_A) A[i] = fold_entry(a.inA[2 * (size_t) i], a.inA[2 * (size_t) i + 1], rf);
        } else {
            V[i] = a.inV[i]; M[i] = a.inM[i];
            if (HAS_A) A[i] = a.inA[i];
        }
    }
    __syncthreads();
    Dig s;
    if (threadIdx.x == 0) s = *a.state;
    u32 len = a.n;
    for (int k = 0; k < a.rounds; ++k, len >>= 1) {
        const u32 pairs = len >> 1;
        F acc[3] = {f_zero(), f_zero(), f_zero()};
        for (u32 i = threadIdx.x; i < pairs; i += blockDim.x)
            fg_fs_pair<HAS_A>(V[2 * i], V[2 * i + 1], M[2 * i], M[2 * i + 1], HAS_A ? A[2 * i] : f_zero(), HAS_A ? A[2 * i + 1] : f_zero(), acc);
        block_sum<3>(acc, lds);
        if (threadIdx.x == 0) {
            for (int t = 0; t < 3; ++t) { a.poly[3 * k + t] = acc[t]; s = fg_fs_elem(s, acc[t]); }
            F r; s = fg_fs_challenge(s, a.slot0 + k, &r);
            a.tape[a.slot0 + k] = r;
            s_r = r;
        }
        __syncthreads();
        const F r = s_r;
        // in place: every thread reads its pairs, the workgroup meets, every thread writes
        F o[FG_FS_TABLES][FG_FS_TAIL_PER];
#pragma unroll
        for (int j = 0; j < FG_FS_TAIL_PER; ++j) {
            const u32 i = threadIdx.x + j * VP_BLOCK;
            if (i < pairs) {
                o[0][j] = fold_entry(V[2 * i], V[2 * i + 1], r); o[1][j] = fold_entry(M[2 * i], M[2 * i + 1], r);
                if (HAS_A) o[2][j] = fold_entry(A[2 * i], A[2 * i + 1], r);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < FG_FS_TAIL_PER; ++j) {
            const u32 i = threadIdx.x + j * VP_BLOCK;
            if (i < pairs) { V[i] = o[0][j]; M[i] = o[1][j]; if (HAS_A) A[i] = o[2][j]; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const F v = V[0];
        a.poly[3 * a.rounds] = v;
        s = fg_fs_elem(s, v);
        for (u32 q = a.extra0; q < a.extra0 + a.n_extra; ++q) { F r; s = fg_fs_challenge(s, q, &r); a.tape[q] = r; }
        *a.state = s;
    }
}

}  // namespace vp
