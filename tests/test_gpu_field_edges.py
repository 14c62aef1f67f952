"""GPU (-m gpu): the lazy field forms and butterflies at the EDGES of the operand ranges their comments state ("Operand contracts").

The product kernels no longer compute with the canonical f_add / f_sub / f_mul but with forms whose correctness rests on operand ranges: limbs in
[0, 2p], weak results below 2^61 + 4 summed unreduced, butterflies on limbs below 2^61 + 8 with offsets 2p / 4p.  Uniform values in [0, p) and the
0/1 wires of SHA-256 land near those edges with probability ~2^-58 per operation, so the transcript tests never visit them.  Here every form runs
through vp_test_field (ops 4 .. 38: raw words in, raw words out, the template arguments of the product kernels) on boundary operands of its STATED
range, against Python integers.  Strict forms must return the canonical residue; weak forms and butterflies a congruent word below their bound.
The host leg (tests/test_field_edges_host.py) runs the exhaustive cross products on the MS = false forms; the multiplier-shift form of c31_add
exists on the device only and is compared here, word for word, with the shift form.

Then structured inputs through the real kernels: transforms of constant / single-spike / alternating / real / imaginary vectors (every butterfly
sees differences of exactly 2p and the non-canonical zero), forward and inverse against the oracle on the SAME input, and sumchecks over circuits
whose inputs and constants come from {0, 1, 2, p - 2, p - 1}."""
import ctypes
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = (1 << 61) - 1
B61 = 1 << 61
WEAK = B61 + 4            # bound of a weakly reduced product (vp_field.h)
LZ = B61 + 8              # bound of a limb travelling through the lazy butterflies (vp_kernels_ntt8.h)
VP_EINVAL = -1

# op codes of vp_test_field (include/vpgpu.h)
MAD_LAZY, MAD_LAZY_W, MAD_C, MAD_C_W, MAD_RB_W, MADC_RB, MADC_RB_W, MUL_PLAIN, HALF, NEG = range(4, 14)
OTHER_MS = 10             # ops 4 .. 10 in the other form of c31_add
MUL_MS, LZ_MUL, LZ_MUL_PS, W8_F, W8_I, W4_F_P2, W4_I_P2, W4_F_P4, W4_I_P4, LZ_CANON, M_FOLD = range(21, 32)
DFT8_F, DFT8_I, DFT4_F, DFT4_I, DFT2, WAVE_SUM, BLOCK_SUM = range(32, 39)


@pytest.fixture(scope="module")
def ctx(vp):
    lib = vp.lib_gpu()
    h = ctypes.c_void_p()
    assert lib.vp_create(0, ctypes.byref(h)) == 0, "vp_create failed: the HIP extension must run on the GPU box"
    yield h
    lib.vp_destroy(h)


def boundary(top):
    """Boundary values of the range [0, top]."""
    s = {0, 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, 1 << 60, P - 1, P, P + 1, B61 + 7, 2 * P - 1, 2 * P, (1 << 62) - 1, top - 1, top}
    return sorted(x for x in s if x <= top)


def corners(top):
    return [0, (1 << 31) - 1, top - 1, top]


def tuples(tops, seed, n_sampled=3000, n_random=2000):
    """Operand tuples, one limb per entry of `tops` (the largest value that limb may take): the cross product of four corner values per limb
    (all-maximal and all-minimal tuples among them), tuples with every limb drawn from its full boundary set, and uniform draws over the whole range."""
    rng = np.random.default_rng(seed)
    out = list(itertools.product(*[corners(t) for t in tops]))
    sets = [boundary(t) for t in tops]
    out += [tuple(s[int(rng.integers(0, len(s)))] for s in sets) for _ in range(n_sampled)]
    out += [tuple(int(rng.integers(0, t, endpoint=True, dtype=np.uint64)) for t in tops) for _ in range(n_random)]
    return out


def u64(rows):
    return np.array(rows, dtype=np.uint64).reshape(-1, 2)


def run(vp, ctx, op, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, dtype=np.uint64)
    out = np.full_like(a, 0x5a5a5a5a5a5a5a5a)
    assert vp.lib_gpu().vp_test_field(ctx, op, a.ctypes.data, b.ctypes.data, out.ctypes.data, a.shape[0]) == 0
    return out


def ints(arr):
    return [(int(x), int(y)) for x, y in arr]


def check_words(got, exp, bound, what, operands):
    """got: (re, im) words of the device; exp: canonical residues.  bound None: strict (the word IS the residue); else congruent and below bound."""
    assert len(got) == len(exp)
    for k, (g, e) in enumerate(zip(got, exp)):
        for limb in (0, 1):
            if bound is None:
                assert g[limb] == e[limb], (what, "limb", limb, "operands", operands[k], "got", g, "expected", e)
            else:
                assert g[limb] < bound, (what, "limb", limb, "above its bound by", g[limb] - bound + 1, "operands", operands[k])
                assert g[limb] % P == e[limb], (what, "limb", limb, "operands", operands[k], "got", g, "expected", e)


# ---------------------------------------------------------------------------------------------------------------------------------
# a*b + c: element 2k carries (a, b) of tuple k, element 2k + 1 carries c (vp_test_field takes the addend from the next element)
# ---------------------------------------------------------------------------------------------------------------------------------
MAD_FORMS = {   # op: (name, top of a's limbs, real second factor, weak result)
    MAD_LAZY: ("f_mad_lazy<false>", 2 * P, False, False), MAD_LAZY_W: ("f_mad_lazy<true>", 2 * P, False, True),
    MAD_C: ("f_mad_c<false>", P - 1, False, False), MAD_C_W: ("f_mad_c<true>", P - 1, False, True),
    MAD_RB_W: ("f_mad31_rb<true>", 2 * P, True, True), MADC_RB: ("f_mad31c_rb<false>", P - 1, True, False),
    MADC_RB_W: ("f_mad31c_rb<true>", P - 1, True, True)}


def mad_operands(op):
    _, top_a, real_b, _ = MAD_FORMS[op]
    # limbs of b in [0, 2p] (a real factor y in [0, 2p]), of c in [0, p]
    tops = [top_a, top_a, 2 * P] + ([] if real_b else [2 * P]) + [P, P]
    t = tuples(tops, seed=op)
    a = np.zeros((2 * len(t), 2), dtype=np.uint64)
    b = np.zeros_like(a)
    for k, v in enumerate(t):
        a[2 * k] = v[0:2]
        b[2 * k] = (v[2], 0) if real_b else v[2:4]
        a[2 * k + 1] = v[-2:]
    return t, a, b


def mad_expected(op, t):
    exp = []
    for v in t:
        if MAD_FORMS[op][2]:
            ar, ai, y, cr, ci = v
            exp.append(((ar * y + cr) % P, (ai * y + ci) % P))
        else:
            ar, ai, br, bi, cr, ci = v
            exp.append(((ar * br - ai * bi + cr) % P, (ar * bi + ai * br + ci) % P))
    return exp


@pytest.mark.parametrize("op", sorted(MAD_FORMS))
def test_multiply_add_forms_at_range_edges(vp, ctx, op):
    """f_mad_lazy / f_mad_c / f_mad31_rb / f_mad31c_rb as the GKR kernels instantiate them, and the same op in the other form of c31_add: both
    against Python integers, and equal to each other word for word (c31_add<true> is compared with nothing else anywhere)."""
    name, _, _, weak = MAD_FORMS[op]
    t, a, b = mad_operands(op)
    exp = mad_expected(op, t)
    got = run(vp, ctx, op, a, b)
    other = run(vp, ctx, op + OTHER_MS, a, b)
    check_words(ints(got[0::2]), exp, WEAK if weak else None, name, t)
    check_words(ints(other[0::2]), exp, WEAK if weak else None, name + " (other c31_add form)", t)
    assert np.array_equal(got[0::2], other[0::2]), name + ": the two forms of c31_add give different words"
    if not weak:
        assert int(got[0::2].max()) < P


def test_canonical_forms_at_range_edges(vp, ctx):
    """f_mul_plain, f_mad31c<false, true>(a, b, 0) (the GKR kernels' f_mul), f_half, f_neg: canonical in, canonical out."""
    t = tuples([P - 1] * 4, seed=11)
    a, b = u64([v[0:2] for v in t]), u64([v[2:4] for v in t])
    exp = [((ar * br - ai * bi) % P, (ar * bi + ai * br) % P) for ar, ai, br, bi in t]
    plain, ms, canonical = run(vp, ctx, MUL_PLAIN, a, b), run(vp, ctx, MUL_MS, a, b), run(vp, ctx, 2, a, b)
    check_words(ints(plain), exp, None, "f_mul_plain", t)
    check_words(ints(ms), exp, None, "f_mad31c<false, true>", t)
    assert np.array_equal(plain, ms) and np.array_equal(plain, canonical)
    inv2 = 1 << 60
    check_words(ints(run(vp, ctx, HALF, a)), [(ar * inv2 % P, ai * inv2 % P) for ar, ai, _, _ in t], None, "f_half", t)
    check_words(ints(run(vp, ctx, NEG, a)), [(-ar % P, -ai % P) for ar, ai, _, _ in t], None, "f_neg", t)


def test_lazy_transform_products_at_range_edges(vp, ctx):
    """lz_mul (canonical root x data limbs in [0, 2p]) and the pre-split form lz_mul_ps(lz_presplit(root), x): weak results (congruent, not the same words: the two negate different factors).
    The data range of lz_mul is f_mad31c's [0, 2p] and ends there: its real limb negates x.im as 2p - x.im, and at x.im = 2^62 - 1 that wraps (this test, run
    with limbs up to 2^62 - 1 as the comment used to allow, gave 6442450941 for root (0, 2^31 - 1), x = (0, 2^62 - 1)).  No caller reaches it: the transforms
    pass limbs below 2^61 + 8.  lz_mul_ps negates the root's limb instead and takes every x below 2^62: second leg."""
    t = tuples([P - 1, P - 1, 2 * P, 2 * P], seed=22)
    a, b = u64([v[0:2] for v in t]), u64([v[2:4] for v in t])
    exp = [((ar * br - ai * bi) % P, (ar * bi + ai * br) % P) for ar, ai, br, bi in t]
    m, ps = run(vp, ctx, LZ_MUL, a, b), run(vp, ctx, LZ_MUL_PS, a, b)
    check_words(ints(m), exp, WEAK, "lz_mul", t)
    check_words(ints(ps), exp, WEAK, "lz_mul_ps", t)
    t = tuples([P - 1, P - 1, (1 << 62) - 1, (1 << 62) - 1], seed=23)
    a, b = u64([v[0:2] for v in t]), u64([v[2:4] for v in t])
    exp = [((ar * br - ai * bi) % P, (ar * bi + ai * br) % P) for ar, ai, br, bi in t]
    check_words(ints(run(vp, ctx, LZ_MUL_PS, a, b)), exp, WEAK, "lz_mul_ps (limbs < 2^62)", t)


@pytest.mark.parametrize("op,name,top,fac", [
    (W8_F, "lz_mul_w8<false>", LZ - 1, (1 << 30, P - (1 << 30))), (W8_I, "lz_mul_w8<true>", LZ - 1, (1 << 30, 1 << 30)),
    (W4_F_P2, "lz_mul_w4<false, 2p>", 2 * P, (0, P - 1)), (W4_I_P2, "lz_mul_w4<true, 2p>", 2 * P, (0, 1)),
    (W4_F_P4, "lz_mul_w4<false, 4p>", 4 * P, (0, P - 1)), (W4_I_P4, "lz_mul_w4<true, 4p>", 4 * P, (0, 1))])
def test_free_roots_at_range_edges(vp, ctx, op, name, top, fac):
    """The multiplications by w_8 = 2^30 (1 -+ i) and w_4 = -+i that cost no multiplier: limbs up to the offset K (w_4) / below 2^61 + 8 (w_8).
    Results congruent and at most 2p (w_8: what level 3 of lz_dft8 subtracts from 2p) / at most K (w_4)."""
    s = boundary(top) + ([3 * B61 - 1, 4 * P - 1] if top == 4 * P else [])
    t = list(itertools.product(s, s)) + tuples([top, top], seed=op, n_sampled=0)
    got = ints(run(vp, ctx, op, u64(t)))
    exp = [((x * fac[0] - y * fac[1]) % P, (x * fac[1] + y * fac[0]) % P) for x, y in t]
    check_words(got, exp, (2 * P if op in (W8_F, W8_I) else top) + 1, name, t)


def test_folds_on_arbitrary_words(vp, ctx):
    """m_fold: any 64-bit word -> [0, p) (eight canonical limbs added before it, unreduced sums of weak products).  lz_canon: words < 2^62."""
    rng = np.random.default_rng(31)
    edge = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, (1 << 62) - 1, 1 << 62, 4 * P, 8 * (P - 1), 8 * P - 1, 8 * P, 8 * P + 7, (1 << 63) - 1, 1 << 63,
            (1 << 64) - 1, (1 << 64) - 2, 7 * B61 - 1, 7 * B61, 7 * (B61 + 7)]
    t = list(itertools.product(edge, edge)) + [tuple(int(x) for x in rng.integers(0, (1 << 64) - 1, size=2, endpoint=True, dtype=np.uint64)) for _ in range(4000)]
    check_words(ints(run(vp, ctx, M_FOLD, u64(t))), [(x % P, y % P) for x, y in t], None, "m_fold", t)
    t = list(itertools.product(boundary((1 << 62) - 1), repeat=2)) + tuples([(1 << 62) - 1] * 2, seed=32, n_sampled=0)
    check_words(ints(run(vp, ctx, LZ_CANON, u64(t))), [(x % P, y % P) for x, y in t], None, "lz_canon", t)


# ---------------------------------------------------------------------------------------------------------------------------------
# butterflies
# ---------------------------------------------------------------------------------------------------------------------------------
def fmul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def root_powers(ob, order, inverse):
    """w^0 .. w^(order - 1) for the reference's root of unity of that order (its inverse for the inverse transform)."""
    w = np.zeros(2, dtype=np.uint64)
    ob.lib().orc_f_root_of_unity(order.bit_length() - 1, w.ctypes.data)
    if inverse:
        wi = np.zeros(2, dtype=np.uint64)
        ob.lib().orc_f_inv(w.ctypes.data, wi.ctypes.data)
        w = wi
    w = (int(w[0]), int(w[1]))
    pw = [(1, 0)]
    for _ in range(order - 1):
        pw.append(fmul(pw[-1], w))
    assert fmul(pw[-1], w) == (1, 0) and pw[order // 2] == (P - 1, 0)
    return pw


def dft_groups(g, seed):
    """Groups of g elements with limbs below 2^61 + 8: every 0 / maximum pattern over the group, the non-canonical zeros, boundary and random draws."""
    top = LZ - 1
    rng = np.random.default_rng(seed)
    groups = []
    for hi, lo in ((top, 0), (top, top - 1), (P, 0), (P, P - 1), (P - 1, 1), (top, P)):
        for mask in range(1 << g):
            groups.append([(hi, hi) if mask >> m & 1 else (lo, lo) for m in range(g)])
    for hi, lo in ((top, 0), (P, 0)):           # real against imaginary limbs
        for mask in range(1 << g):
            groups.append([(hi, lo) if mask >> m & 1 else (lo, hi) for m in range(g)])
    s = boundary(top)
    for _ in range(1500):
        groups.append([(s[int(rng.integers(0, len(s)))], s[int(rng.integers(0, len(s)))]) for _ in range(g)])
    for _ in range(1000):
        groups.append([tuple(int(x) for x in rng.integers(0, top, size=2, endpoint=True, dtype=np.uint64)) for _ in range(g)])
    return groups


@pytest.mark.parametrize("op,name,g,inverse", [(DFT8_F, "lz_dft8<false>", 8, False), (DFT8_I, "lz_dft8<true>", 8, True), (DFT4_F, "lz_dft4<false>", 4, False),
                                               (DFT4_I, "lz_dft4<true>", 4, True), (DFT2, "lz_dft2", 2, False)])
def test_lazy_butterflies_at_range_edges(vp, ob, ctx, op, name, g, inverse):
    """u[k] <- sum_m u[m] w_g^(m k) on limbs up to 2^61 + 7: the plain sum over Python integers with the oracle's root of unity, raw outputs congruent
    and below 2^61 + 8.  (Level 1 differences reach 3 * 2^61, level 2 sums 7 * 2^61; the offsets 2p / 4p must dominate what they subtract.)"""
    pw = root_powers(ob, g, inverse)
    groups = dft_groups(g, seed=op)
    got = ints(run(vp, ctx, op, u64([e for grp in groups for e in grp])))
    exp, operands = [], []
    for grp in groups:
        for k in range(g):
            acc = (0, 0)
            for m in range(g):
                t = fmul(grp[m], pw[m * k % g])
                acc = (acc[0] + t[0], acc[1] + t[1])
            exp.append((acc[0] % P, acc[1] % P))
            operands.append((k, grp))
    check_words(got, exp, LZ, name, operands)


# ---------------------------------------------------------------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------------------------------------------------------------
def sum_inputs():
    rng = np.random.default_rng(41)
    full = np.full((1024, 2), P - 1, dtype=np.uint64)                      # every lane holds (p - 1, p - 1)
    one = np.zeros((1024, 2), dtype=np.uint64); one[300] = (P - 1, P - 1)  # a single lane does
    ragged = rng.integers(0, P, size=(5 * 256 + 77, 2), dtype=np.uint64)   # the last block is cut short by n
    ragged_full = np.full((256 + 65, 2), P - 1, dtype=np.uint64)
    tiny = np.full((1, 2), P - 1, dtype=np.uint64)
    return [("all p-1", full, full), ("single lane", one, np.roll(one, 17, axis=0)), ("ragged random", ragged, np.roll(ragged, 5, axis=0)),
            ("ragged p-1", ragged_full, ragged_full), ("n = 1", tiny, tiny)]


def test_wave_and_block_sums_at_range_edges(vp, ctx):
    """wave_sum63 adds eight canonical limbs before its first fold and eight folded values before its last ("8 (2^61 - 1) < 2^64"); block_sum<3> adds the
    waves' totals canonically.  Totals against Python integers, canonical."""
    for what, a, b in sum_inputs():
        n = a.shape[0]
        ai, bi = ints(a), ints(b)
        w = run(vp, ctx, WAVE_SUM, a, b)
        for first in range(0, n - 63, 64):
            exp = (sum(x for x, _ in ai[first:first + 64]) % P, sum(y for _, y in ai[first:first + 64]) % P)
            assert (int(w[first + 63][0]), int(w[first + 63][1])) == exp, ("wave_sum63", what, "wave", first // 64)
        s = run(vp, ctx, BLOCK_SUM, a, b)
        for first in range(0, n, 256):
            xs, ys = ai[first:first + 256], bi[first:first + 256]
            exp = [(sum(x for x, _ in xs) % P, sum(y for _, y in xs) % P), (sum(x for x, _ in ys) % P, sum(y for _, y in ys) % P),
                   (sum(y for _, y in xs) % P, sum(x for x, _ in ys) % P)]
            for k in range(min(3, n - first)):
                assert (int(s[first + k][0]), int(s[first + k][1])) == exp[k], ("block_sum<3>", what, "block", first // 256, "sum", k)
            assert not s[first + 3:first + 256].any(), ("block_sum<3>", what, "stray words in block", first // 256)


def test_field_entry_point_refuses_what_it_cannot_run(vp, ctx):
    lib = vp.lib_gpu()
    a = np.zeros((8, 2), dtype=np.uint64)
    out = np.zeros_like(a)
    assert lib.vp_test_field(ctx, 39, a.ctypes.data, a.ctypes.data, out.ctypes.data, 8) == VP_EINVAL
    assert lib.vp_test_field(ctx, -1, a.ctypes.data, a.ctypes.data, out.ctypes.data, 8) == VP_EINVAL
    for op, n in ((DFT8_F, 7), (DFT8_I, 4), (DFT4_F, 6), (DFT4_I, 2), (DFT2, 1)):        # the butterflies take whole groups
        assert lib.vp_test_field(ctx, op, a.ctypes.data, a.ctypes.data, out.ctypes.data, n) == VP_EINVAL
    assert lib.vp_test_field(ctx, DFT8_F, a.ctypes.data, a.ctypes.data, out.ctypes.data, 0) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# structured inputs through the real kernels
# ---------------------------------------------------------------------------------------------------------------------------------
FFT_PATTERNS = ["zero", "all p-1", "spike at 0", "spike at n-1", "spike at n/2", "constant one", "alternating 0 / p-1", "real random", "imaginary random"]


def fft_pattern(name, n, seed):
    c = np.zeros((n, 2), dtype=np.uint64)
    rng = np.random.default_rng(seed)
    if name == "all p-1":
        c[:] = P - 1
    elif name == "spike at 0":
        c[0] = (P - 1, 0)
    elif name == "spike at n-1":
        c[n - 1] = (P - 1, 0)
    elif name == "spike at n/2":
        c[n // 2] = (P - 1, 0)
    elif name == "constant one":
        c[:, 0] = 1
    elif name == "alternating 0 / p-1":
        c[1::2] = P - 1
    elif name == "real random":
        c[:, 0] = rng.integers(0, P, size=n, dtype=np.uint64)
    elif name == "imaginary random":
        c[:, 1] = rng.integers(0, P, size=n, dtype=np.uint64)
    else:
        assert name == "zero"
    return c


def structured_fft_case(vp, ob, ctx, ln, mode):
    """mode: 1 / 32 = forward transform at that ratio, 0 = inverse.  Expected: orc_fft, and orc_ifft ON THE SAME INPUT."""
    lib, L = vp.lib_gpu(), ob.lib()
    L.orc_fft.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.orc_ifft.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    n = 1 << ln
    for k, name in enumerate(FFT_PATTERNS):
        c = fft_pattern(name, n, seed=100 * ln + k)
        m = n * (mode or 1)
        out = np.full((m, 2), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
        exp = np.zeros_like(out)
        if mode:
            assert lib.vp_test_fft(ctx, c.ctypes.data, n, m, 0, out.ctypes.data) == 0
            L.orc_fft(c.ctypes.data, n, m, exp.ctypes.data)
        else:
            assert lib.vp_test_fft(ctx, c.ctypes.data, n, n, 1, out.ctypes.data) == 0
            L.orc_ifft(c.ctypes.data, n, exp.ctypes.data)
        assert int(out.max()) < P, (name, "non-canonical output")
        bad = np.flatnonzero((out != exp).any(axis=1))
        assert bad.size == 0, (name, "2^%d" % ln, "mode", mode, "first differing index", int(bad[0]), out[bad[0]], exp[bad[0]], "of", bad.size)


@pytest.mark.parametrize("mode", [1, 32, 0])
@pytest.mark.parametrize("ln", [3, 12, 13, 17])
def test_fft_structured_inputs_vs_oracle(vp, ob, ctx, ln, mode):
    """One size per code path below 2^18 (2^3 and 2^12: the LDS kernels; 2^13 and 2^17: the radix-8 pair, smallest and largest; 2^18 / 2^19 are in
    test_gpu_large_inputs.py).  Equal sub-sequences make the level-1 differences exactly 2p and the sums 2p - 2 in every butterfly."""
    structured_fft_case(vp, ob, ctx, ln, mode)


EDGE_VALUES = (0, 1, 2, P - 2, P - 1)


@pytest.mark.parametrize("real_consts", [True, False])
@pytest.mark.parametrize("seed,sizes", [(11, [1500, 2100, 900, 4100, 700]), (12, [40, 33, 50, 17]), (13, [4096, 1024, 3000])])
def test_sumcheck_over_edge_valued_circuits_vs_oracle(vp, ob, seed, sizes, real_consts):
    """Inputs and Mulc / Addc constants from {0, 1, 2, p - 2, p - 1}: the lazy differences v1 + p - v0 of round 1 sit at 1, p, 2p - 1 and the sums of
    products of p - 1 at the top of the unreduced accumulators.  Real constants keep every value real (the half-price real x complex products of
    round 1, sf_pair_step_rv); constants with the same set in both limbs take the general products.  Layers of >= 2^10 gates reach the three-round
    fold kernel; the small ragged circuit the closing kernels alone.  Both proving modes against the oracle's transcript of the same circuit."""
    import custom_circuits as cc
    from test_gpu_parity import _both_modes
    args = cc.make(seed, sizes, values=EDGE_VALUES, real_consts=real_consts)
    assert set(int(x) for x in args[3][:sizes[0]]) <= set(EDGE_VALUES) and set(int(x) for x in args[5].ravel()) <= set(EDGE_VALUES)
    assert bool(args[5][:, 1].any()) != real_consts
    c = vp.Circuit.custom(*args)
    oc = ob.Circuit.custom(*args)
    assert c.hash() == oc.hash()
    gold, st = oc.prove_gkr()
    assert st["verified"] == 1
    _both_modes(vp, c, gold)
    c.close(); oc.close()
