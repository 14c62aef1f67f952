// Transforms of 2^18 and 2^19 points (the commitment at input layers of 2^24 / 2^25 wires: slices of N = 2^(n-6) coefficients).  Part of the single
// translation unit vpgpu.hip (included by vp_kernels_pc.h after vp_kernels_ntt8.h).
//
//   N = N0 x N', N0 = 2^l0 (2 or 4), N' = 2^17: one radix-N0 step by decimation in time around the tuned 2^17-point pair of vp_kernels_ntt8.h, unchanged.
//   k_ntt_long_split: D_j0[k'] = in[j0 + N0 k'] — the N0 interleaved sub-sequences of each row, each contiguous (N0 x N' elements per row).
//   The sub-transforms: forward — P(x) = sum_j0 x^j0 Q_j0(x^N0), and x^N0 runs over the order-M/N0 points with the same coset pattern, so each Q_j0 is encoded by
//       the existing 2^17-point path (32 cosets or one) on the root table of order M / N0; inverse — the existing 2^17-point inverse of each D_j0.
//   k_ntt_long_merge: per (row, coset) and a' < N', the N0 outputs a' + N' t are one radix-N0 DFT of the sub-transforms' values at a', each multiplied first by
//       w_M^(j0 (b + a' M / N)) = w_N^(j0 a') w_M^(j0 b) (forward, coset b) or w_N^(-j0 a') (inverse; the sub-transforms scaled by 1/N', this pass by 1/N0):
//       out[a' + N' t] = sum_j0 w_N0^(+-t j0) w^(j0 ...) C_j0[a'].   Natural order out, canonical limbs.
// Both passes stream: every element is read once and written once, whole lines per wave.  Lazy arithmetic as in vp_kernels_ntt8.h: products and the
// radix-N0 butterflies stay weakly reduced, the store canonicalises.
#pragma once

namespace vp {

constexpr u32 NTTL_THREADS = 256;

// D[(row N0 + j0) N' + k'] = in[row in_stride + j0 + N0 k'].  grid (N' / 256, rows)
template <int L0>
__global__ void __launch_bounds__(NTTL_THREADS) k_ntt_long_split(const F *__restrict__ in, F *__restrict__ out, u32 in_stride, int lsub) {
    constexpr u32 N0 = 1u << L0;
    const u32 kp = blockIdx.x * NTTL_THREADS + threadIdx.x, row = blockIdx.y;
    const F *src = in + (size_t) row * in_stride + ((size_t) kp << L0);
    F v[N0];
#pragma unroll
    for (u32 j0 = 0; j0 < N0; ++j0) v[j0] = src[j0];
    F *dst = out + ((size_t) row << (lsub + L0)) + kp;
#pragma unroll
    for (u32 j0 = 0; j0 < N0; ++j0) dst[(size_t) j0 << lsub] = v[j0];
}

struct NttLongArgs {
    const F *in;        // sub-transform outputs: row r' = row N0 + j0, coset b at ((r' ncoset + b) << lsub)
    F *out;             // [(row ncoset + b)][N], natural order; may be `in` itself when ncoset = 1 (every thread rewrites exactly the positions it read)
    const F *W;         // w_N^e, e < N (full circle of order N)
    const F *RT; u32 half_m;        // half table of order M: the coset factors w_M^(j0 b)
    int lsub; u32 ncoset;
    F scale;            // inverse: 1 / N0 (pre-split for lz_mul_ps); forward: unused
};
// grid (N' / 256, rows x ncoset)
template <int L0, bool INV>
__global__ void __launch_bounds__(NTTL_THREADS) k_ntt_long_merge(NttLongArgs a) {
    constexpr u32 N0 = 1u << L0;
    const u32 ap = blockIdx.x * NTTL_THREADS + threadIdx.x, rt = blockIdx.y, row = rt / a.ncoset, b = rt - row * a.ncoset;
    const u32 N = 1u << (a.lsub + L0), M = 2 * a.half_m;
    F u[N0];
#pragma unroll
    for (u32 j0 = 0; j0 < N0; ++j0) u[j0] = a.in[((((size_t) row * N0 + j0) * a.ncoset + b) << a.lsub) + ap];
    F w[N0];
#pragma unroll
    for (u32 j0 = 1; j0 < N0; ++j0) { const u32 e = (j0 * ap) & (N - 1); w[j0] = a.W[INV ? (N - e) & (N - 1) : e]; }
    loads_first();
    if (!INV && b) {                                            // uniform per workgroup: the coset's share w_M^(j0 b)
#pragma unroll
        for (u32 j0 = 1; j0 < N0; ++j0) u[j0] = lz_mul(root_pow(a.RT, a.half_m, (j0 * b) & (M - 1)), u[j0]);
    }
#pragma unroll
    for (u32 j0 = 1; j0 < N0; ++j0) u[j0] = lz_mul(w[j0], u[j0]);
    if constexpr (L0 == 1) lz_dft2(u);                      // w_2 = -1 both ways
    else lz_dft4<INV>(u);
    F *dst = a.out + ((size_t) rt << (a.lsub + L0)) + ap;
#pragma unroll
    for (u32 t = 0; t < N0; ++t) dst[(size_t) t << a.lsub] = lz_canon(INV ? lz_mul_ps(a.scale, u[t]) : u[t]);
}

}  // namespace vp
