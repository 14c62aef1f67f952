// The 64 slice corners of an eq table.  The commitment cuts a public vector of 2^n entries into 64 slices of N = 2^(n-6); of the eq table of a point
// (initBetaTable, src/utils.cpp:8-45: eq(pt, j) is a product of n factors, pt[k] for a set bit k of j and 1 - pt[k] otherwise) the entries at the slice
// starts, corner[i] = eq(pt, i N), need only the n - 6 low factors at bit 0 and the six high ones by the bits of i.  vp_commit_public_eq forms them on the
// host, sharded or not, instead of reading them back from the device: the tensor decision and the 64 scalars corner[i] / corner[0] come from them.
// Host only, nothing but vp_field.h (tests/sanitize/pc_corners_main.cpp checks it against the product over all n bits, under plain g++).
#pragma once
#include "vp_field.h"

namespace vp {

// pt: n canonical coordinates, 7 <= n
inline void pc_eq_corners(const F *pt, int n, F corner[64]) {
    F low = f_one();
    for (int k = 0; k < n - 6; ++k) low = f_mul(low, f_sub(f_one(), pt[k]));
    for (int i = 0; i < 64; ++i) {
        F v = low;
        for (int k = 0; k < 6; ++k) v = f_mul(v, ((i >> k) & 1) ? pt[n - 6 + k] : f_sub(f_one(), pt[n - 6 + k]));
        corner[i] = v;
    }
}

}  // namespace vp
