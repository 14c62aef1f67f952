"""Definition-level reference of the commitment's mask slice (lib/virgo/src/poly_commit.h:55-86, 138-161, 187-262 and the mask slice's part of fri.cpp) in Python
integers: no transform code, polynomials as coefficient lists, for padded mask lengths up to 256.

  L, Q      the polynomials of degree < ms through the zero-padded masks on the ms-th roots of unity, by the inverse DFT's sum
  L Q       a schoolbook product; G its lower half (degree < ms), H its upper half — the reference's lq_coef / h_coef — and S0 = (L Q)[0] + H[0]
  all_sum   ms S0, which is also sum_i pri[i] pub[i] (asserted: the sum of L Q over the ms-th roots, where x^ms = 1, is the sum of G + H)
  oracle    l q - (x^ms - 1) h = G + H on the whole domain, so the virtual oracle (.. - S0) ms / x is the polynomial ms ((G + H)(x) - S0) / x
  fold      f(x) = e(x^2) + x o(x^2) gives ((f(x) + f(-x)) + r / x (f(x) - f(-x))) / 2 = e(y) + r o(y), y = x^2: c'_i = c_2i + r c_(2i+1)
  values    Horner's rule at the opened positions

The only datum taken from elsewhere is w_M, the oracle's root of unity of order M = 2^(n-1) (orc_f_root_of_unity), checked here: w^(M/2) = -1.  Field elements
are (re, im) pairs of ints below p = 2^61 - 1, i^2 = -1."""
P = (1 << 61) - 1
ZERO, ONE = (0, 0), (1, 0)


def add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def power(a, e):
    out = ONE
    while e:
        if e & 1:
            out = mul(out, a)
        a = mul(a, a)
        e >>= 1
    return out


def inv(a):
    d = pow((a[0] * a[0] + a[1] * a[1]) % P, P - 2, P)          # 1 / (re + i im) = (re - i im) / (re^2 + im^2)
    return (a[0] * d % P, -a[1] * d % P)


def horner(c, x):
    out = ZERO
    for k in reversed(c):
        out = add(mul(out, x), k)
    return out


def interpolate(values, w):
    """coefficients of the polynomial of degree < len(values) with p(w^j) = values[j], w a primitive root of that order: c_k = 1/n sum_j v_j w^(-jk)"""
    n = len(values)
    wi = inv(w)
    pw = [ONE]
    for _ in range(n - 1):
        pw.append(mul(pw[-1], wi))
    n_inv = (pow(n, P - 2, P), 0)
    out = []
    for k in range(n):
        re = im = 0
        for j, v in enumerate(values):
            t = pw[j * k % n]
            re += v[0] * t[0] - v[1] * t[1]
            im += v[0] * t[1] + v[1] * t[0]
        out.append(mul((re % P, im % P), n_inv))
    return out


def product(a, b):
    re, im = [0] * (len(a) + len(b)), [0] * (len(a) + len(b))
    for i, x in enumerate(a):
        if x == ZERO:
            continue
        for j, y in enumerate(b):
            re[i + j] += x[0] * y[0] - x[1] * y[1]
            im[i + j] += x[0] * y[1] + x[1] * y[0]
    return [(u % P, v % P) for u, v in zip(re, im)]


class MaskSlice:
    """the mask slice of one commitment at input bit length n: pri / pub the mask vectors as given (lists of (re, im)), r the n - 6 fold challenges"""

    def __init__(self, n, pri, pub, r, w_M):
        self.n, self.M, self.N, self.w = n, 1 << (n - 1), 1 << (n - 6), w_M
        assert power(w_M, self.M // 2) == (P - 1, 0), "w_M is no primitive root of order M"
        gap = 1 << ((self.M // len(pri)).bit_length() - 1)                   # the largest power of two <= M / len (poly_commit.h:55-61)
        self.ms = ms = self.M // gap
        assert 8 <= ms <= 256 and gap >= 2 and len(pub) <= ms and len(r) == n - 6
        pri = list(pri) + [ZERO] * (ms - len(pri))
        pub = list(pub) + [ZERO] * (ms - len(pub))
        w_ms = power(w_M, gap)
        self.L, self.Q = interpolate(pri, w_ms), interpolate(pub, w_ms)
        LQ = product(self.L, self.Q)                                         # 2 ms entries, the last one zero
        G, self.H = LQ[:ms], LQ[ms:]
        S0 = add(LQ[0], self.H[0])
        self.all_sum = mul(S0, (ms, 0))
        direct = ZERO
        for a, b in zip(pri, pub):
            direct = add(direct, mul(a, b))
        assert self.all_sum == direct, "the reference of the mask slice contradicts itself: ms S0 != <pri, pub>"
        GH = [add(a, b) for a, b in zip(G, self.H)]
        c = [mul(x, (ms, 0)) for x in GH[1:]]                                # ms ((G + H)(x) - S0) / x
        self.levels = []                                                     # levels[k]: coefficients after k + 1 folds, on the domain of w^(2^(k+1))
        for rk in r:
            c = c + [ZERO] * (len(c) & 1)
            c = [add(c[2 * i], mul(rk, c[2 * i + 1])) for i in range(len(c) // 2)]
            self.levels.append(c)

    def pair(self, oracle, leaf):
        """the mask slice's pair of an opening: oracle 0 = l, 1 = h, 2 + k = FRI level k; positions leaf and leaf + half the codeword"""
        if oracle < 2:
            c, lg = (self.L, self.H)[oracle], 0
        else:
            c, lg = self.levels[oracle - 2], oracle - 1
        size = self.M >> lg
        assert 0 <= leaf < size // 2
        g = power(self.w, 1 << lg)
        return horner(c, power(g, leaf)), horner(c, power(g, leaf + size // 2))

    def final_mask(self):
        """the 32 values of vp_fri_final_mask: the last level's codeword, [i << 1 | hi] = position i + 16 hi"""
        out = [None] * 32
        for i in range(16):
            out[2 * i], out[2 * i + 1] = self.pair(2 + self.n - 7, i)
        return out
