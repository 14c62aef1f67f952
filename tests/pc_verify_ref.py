"""Reference, in Python integers and hashlib, of the two values the commitment verifier's heavy loops return (host/verifier.cpp: pcPublicEvalsHost,
pcOpeningDigestsHost; device: vp_pc_public_evals, vp_fri_query_digests).  Written from the definitions, not from the code under test:

  * the public vector eq(point, .) is the PRODUCT over the coordinates; slice j is its entries [j N, (j + 1) N), N = 2^(n-6);
  * q_j is the polynomial of degree < N with q_j(omega^i) = slice_j[i], omega the root of unity of order N, evaluated through the barycentric form
        q_j(x) = ((x^N - 1) / N) sum_i s[i] omega^i / (x - omega^i)        (x = omega^i itself: s[i])
    — no inverse transform, no Horner;
  * a digest is hashlib.sha3_256 over block || state (host/sha3.hpp), 65 blocks from the zero state for a leaf chain, then up the Merkle path.

F_p^2 = F_p[i] / (i^2 + 1), p = 2^61 - 1, elements as (re, im) tuples of Python ints."""
import hashlib
import struct

P = (1 << 61) - 1
ROOT_2_62 = (2147483648, 1033321771269002680)       # generator of the 2^62-th roots of unity (fieldElement.cpp:237-249)
VAL = 130 * 16


def add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], P - 2, P)
    return (a[0] * d % P, -a[1] * d % P)


def fpow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = mul(r, a)
        a = mul(a, a)
        e >>= 1
    return r


def root_of_unity(log_order):
    r = ROOT_2_62
    for _ in range(62 - log_order):
        r = mul(r, r)
    return r


def eq_table(point):
    """eq(point, i) = prod_k (bit k of i ? point[k] : 1 - point[k])."""
    n = len(point)
    out = []
    for i in range(1 << n):
        e = (1, 0)
        for k in range(n):
            e = mul(e, point[k] if (i >> k) & 1 else sub((1, 0), point[k]))
        out.append(e)
    return out


def interpolant_at(s, x):
    """q(x) for the q of degree < len(s) with q(omega^i) = s[i]."""
    N = len(s)
    ln = N.bit_length() - 1
    om = root_of_unity(ln)
    pw = [(1, 0)]
    for _ in range(N - 1):
        pw.append(mul(pw[-1], om))
    for i in range(N):
        if pw[i] == x:
            return s[i]
    acc = (0, 0)
    for i in range(N):
        acc = add(acc, mul(mul(s[i], pw[i]), inv(sub(x, pw[i]))))
    return mul(mul(sub(fpow(x, N), (1, 0)), inv((N % P, 0))), acc)


def public_evals(n, pub, leaf0):
    """[q][h][j] = q_j(+-w^leaf0[q]) for the public vector pub (2^n elements), w the root of unity of order 2^(n-1)."""
    N = 1 << (n - 6)
    w = root_of_unity(n - 1)
    out = []
    for lf in leaf0:
        x0 = fpow(w, lf)
        x1 = sub((0, 0), x0)
        out.append([[interpolant_at(pub[j * N:(j + 1) * N], x) for j in range(64)] for x in (x0, x1)])
    return out


def hhash(block, state):
    return hashlib.sha3_256(block + state).digest()


def query_leaves(n, leaf0):
    """(oracle, leaf, path digests) of every opening of one repetition, in vp_fri_query's order."""
    out = [(0, leaf0, n - 1), (1, leaf0, n - 1)]
    D, t = 1 << (n - 1), leaf0
    for k in range(n - 6):
        Dn = D // 2
        t = t % (Dn // 2)
        out.append((2 + k, t, n - 2 - k))
        D = Dn
    return out


def answer_bytes(n, n_queries):
    return n_queries * sum(VAL + 32 * plen for _, _, plen in query_leaves(n, 0))


def opening_digest(leaf, values, path, depth):
    """(leaf-chain digest of the 2080 value bytes, root reached through path[0 .. depth))."""
    h = bytes(32)
    for s in range(65):
        h = hhash(values[32 * s:32 * s + 32], h)
    leaf_digest = h
    pos = leaf
    for k in range(depth):
        sib = path[32 * k:32 * k + 32]
        h = hhash(sib, h) if pos & 1 else hhash(h, sib)
        pos >>= 1
    return leaf_digest, h


def opening_digests(n, leaf0, answer):
    """64 bytes per opening of an answer block in vp_fri_query's layout."""
    assert len(answer) == answer_bytes(n, len(leaf0))
    out, at = [], 0
    for lf in leaf0:
        for _, leaf, plen in query_leaves(n, lf):
            a, b = opening_digest(leaf, answer[at:at + VAL], answer[at + VAL:at + VAL + 32 * plen], plen - 1)
            out.append(a + b)
            at += VAL + 32 * plen
    return b"".join(out)


def pack(elems):
    return b"".join(struct.pack("<QQ", e[0], e[1]) for e in elems)
