"""The commitment's verifier from its definition, in Python integers and hashlib: what Circuit.verify_commitment must decide, and which check must say so.

Written from the protocol (lib/virgo/src/vpd_verifier.cpp:76-328), not from host/verifier.cpp.  The commitment holds 64 witness slices and one mask
slice.  For slice j the prover commits l_j (the slice's low-degree extension) and h_j on the domain of w, the root of unity of order M = 2^(n-1), and claims

        l_j(x) q_j(x) - (x^N - 1) h_j(x) = g_j(x),   deg g_j < N,   N g_j(0) = all_sum[j]                      (N = 2^(n-6); the mask slice: ms for N)

with q_j the polynomial of degree < N through the j-th slice of the public vector on the N-th roots of unity.  v_j(x) = (N g_j(x) - all_sum[j]) / x then has
degree < N - 1, and FRI proves that: level k holds e(y) + r_k o(y) of the level before, v = e(x^2) + x o(x^2), which at x = w_D^t, from the pair (a, b) at
t and t + D / 2 (b is the value at -x), is

        ((a + b) + (w_D^t)^-1 r_k (a - b)) / 2,             w_D = w^(2^k) the generator of level k's input domain (D = M / 2^k points).

It sits at index t of the next domain (D / 2 points), whose leaves hold the pairs (i, i + D / 4): leaf t mod D / 4, second element iff t >= D / 4.  After n - 6
levels 32 points are left and the codeword must be a constant; the last opened pair must be that constant.

verify(..) takes the arguments of Circuit.verify_commitment and returns (accepted, name, repetition, slice), name in the strings of host/verifier.cpp.  Order:
slice sums; constancy of the final codewords (64 slices x 32 entries, then the mask's 32); then per repetition the Merkle openings of l and h, and per level the
level's Merkle opening, then its fold relation over slices 0 .. 64; then the last pair.  q_j(x) is pc_verify_ref.interpolant_at (barycentric: no transform, no
Horner), the mask polynomial pc_mask_ref.interpolate / horner.  Values that depend only on (slice, position) or on an opening's bytes are kept between calls: a
table of forgeries verifies the same openings over and over."""
import hashlib

import numpy as np

import pc_mask_ref as mref
import pc_verify_ref as ref

P = ref.P
SUMS = "commitment: slice sums do not match the inner product"
MERKLE = "commitment: Merkle opening rejected"
RS, RS_MSK = "Fri rs code check fail", "Fri msk rs code check fail"
FINAL, FINAL_MSK = "Fri final codeword mismatch", "Fri msk final codeword mismatch"


def round_name(k, mask=False):
    return ("Fri msk check consistency %d round fail" if mask else "Fri check consistency %d round fail") % k


def level_merkle(k):
    return "commitment: FRI Merkle opening rejected (level %d)" % k


_Q, _MERKLE, _MASKQ, _REP = {}, {}, {}, {}


def _elems(a):
    return [(int(x[0]), int(x[1])) for x in np.ascontiguousarray(a, np.uint64).reshape(-1, 2)]


def _q_at(slice_bytes, s, n, s0):
    """(q(x0), q(-x0)) of one slice of the public vector, x0 = w^s0"""
    key = (slice_bytes, n, s0)
    if key not in _Q:
        x0 = ref.fpow(ref.root_of_unity(n - 1), s0)
        _Q[key] = (ref.interpolant_at(s, x0), ref.interpolant_at(s, ref.sub((0, 0), x0)))
    return _Q[key]


def _mask_q_at(pub_mask, ms, n, s0):
    if ms == 1:
        return (0, 0), (0, 0)
    pm = _elems(pub_mask) if pub_mask is not None else []
    key = (tuple(pm), ms, n, s0)
    if key not in _MASKQ:
        w = ref.root_of_unity(n - 1)
        coef = mref.interpolate(pm + [mref.ZERO] * (ms - len(pm)), mref.power(w, (1 << (n - 1)) // ms))
        x0 = mref.power(w, s0)
        _MASKQ[key] = (mref.horner(coef, x0), mref.horner(coef, mref.sub(mref.ZERO, x0)))
    return _MASKQ[key]


def _opening_ok(root, leaf, blob, plen):
    """the chain of the 130 values is the path's last digest and the path leads from it to the root"""
    key = (root, leaf, blob)
    if key not in _MERKLE:
        d, top = ref.opening_digest(leaf, blob[:ref.VAL], blob[ref.VAL:], plen - 1)
        _MERKLE[key] = d == blob[ref.VAL + 32 * (plen - 1):] and top == root
    return _MERKLE[key]


def verify(n, claim, root_l, root_h, all_sum, r, fri_roots, final_code, final_mask, leaf0, answer, point=None, pub=None, pub_mask=None, ms=1):
    assert (point is None) != (pub is None) and len(answer) == ref.answer_bytes(n, len(leaf0))
    ln, N, M = n - 6, 1 << (n - 6), 1 << (n - 1)
    sums, r, fc, fm = _elems(all_sum), _elems(r), _elems(final_code), _elems(final_mask)
    claim = _elems(claim)[0]
    # 1. the witness slices' sums are the claimed inner product (the mask slice's is no part of it)
    tot = (0, 0)
    for j in range(64):
        tot = ref.add(tot, sums[j])
    if tot != claim:
        return False, SUMS, None, None
    # 2. the final codewords are constants: entry (i, hi) of slice s is the codeword's value at position i + 16 hi
    for s in range(64):
        if any(fc[(i << 7) | (s << 1) | hi] != fc[s << 1] for i in range(16) for hi in range(2)):
            return False, RS, None, s
    if any(x != fm[0] for x in fm):
        return False, RS_MSK, None, 64
    const = [fc[s << 1] for s in range(64)] + [fm[0]]
    # 3. the repetitions
    pubv = ref.eq_table(_elems(point)) if pub is None else _elems(pub)
    slices = [pubv[j * N:(j + 1) * N] for j in range(64)]
    keys = [ref.pack(s) for s in slices]
    roots = [root_l, root_h] + [fri_roots[32 * k:32 * k + 32] for k in range(ln)]
    w = ref.root_of_unity(n - 1)
    inv2 = ref.inv((2, 0))
    size = [N] * 64 + [ms]

    def algebra(s0, blobs):
        """(level of the first failed relation — n - 6: the last pair —, name, slice) of one repetition's opened values, or None"""
        vl, vh = (_elems(np.frombuffer(b[:ref.VAL], np.uint64)) for _, _, _, b in blobs[:2])
        x = [ref.fpow(w, s0), ref.fpow(w, s0 + M // 2)]
        assert ref.add(x[0], x[1]) == (0, 0)
        cur = []
        for j in range(65):
            q = _q_at(keys[j], slices[j], n, s0) if j < 64 else _mask_q_at(pub_mask, ms, n, s0)
            pair = []
            for h in range(2):
                g = ref.sub(ref.mul(vl[2 * j + h], q[h]), ref.mul(ref.sub(ref.fpow(x[h], size[j]), (1, 0)), vh[2 * j + h]))
                pair.append(ref.mul(ref.sub(ref.mul(g, (size[j] % P, 0)), sums[j]), ref.inv(x[h])))
            cur.append(pair)
        D, t = M, s0
        for k in range(ln):
            _, leaf, _, b = blobs[2 + k]
            assert leaf == t % (D // 4)
            nxt = _elems(np.frombuffer(b[:ref.VAL], np.uint64))
            c = ref.mul(ref.inv(ref.fpow(ref.fpow(w, 1 << k), t)), r[k])
            second = t >= D // 4
            for j in range(65):
                a, bb = cur[j]
                if ref.mul(inv2, ref.add(ref.add(a, bb), ref.mul(c, ref.sub(a, bb)))) != nxt[2 * j + second]:
                    return k, round_name(k, j == 64), j
            cur = [[nxt[2 * j], nxt[2 * j + 1]] for j in range(65)]
            D, t = D // 2, leaf
        for j in range(65):
            if cur[j][0] != const[j] or cur[j][1] != const[j]:
                return ln, (FINAL if j < 64 else FINAL_MSK), j
        return None

    ctx = hashlib.sha256(b"".join([bytes([n]), ref.pack(sums), ref.pack(r), ref.pack(const), b"".join(keys),
                                   repr((ms, None if pub_mask is None else _elems(pub_mask))).encode()])).digest()
    at = 0
    for rep, s0 in enumerate(leaf0):
        blobs = []
        for o, leaf, plen in ref.query_leaves(n, s0):
            blobs.append((o, leaf, plen, answer[at:at + ref.VAL + 32 * plen]))
            at += ref.VAL + 32 * plen
        key = (ctx, s0, b"".join(b[:ref.VAL] for _, _, _, b in blobs))
        if key not in _REP:
            _REP[key] = algebra(s0, blobs)
        alg = _REP[key]
        if not all([_opening_ok(roots[o], leaf, b, plen) for o, leaf, plen, b in blobs[:2]]):
            return False, MERKLE, rep, None
        for k in range(ln):
            o, leaf, plen, b = blobs[2 + k]
            if not _opening_ok(roots[o], leaf, b, plen):
                return False, level_merkle(k), rep, None
            if alg is not None and alg[0] == k:
                return False, alg[1], rep, alg[2]
        if alg is not None:
            return False, alg[1], rep, alg[2]
    return True, "", None, None


def verify_p(p, **change):
    """verify() on a proof dict of masked_verifier_cases (pub / pub_mask / ms from the dict; point= replaces pub)"""
    a = dict(p, **change)
    if a.get("point") is not None:
        a["pub"] = None
    return verify(a["n"], a["claim"], a["root_l"], a["root_h"], a["all_sum"], a["r"], a["fri_roots"], a["final_code"], a["final_mask"], a["leaf0"], a["answer"],
                  point=a.get("point"), pub=a["pub"], pub_mask=a["pub_mask"], ms=a["ms"])
