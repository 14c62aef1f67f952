"""The GKR prover of one proof in plain Python integers, written from the definitions on top of tests/verifier_sums.py: the reference the oracle's tape
entry (orc_prove_gkr_tape) is compared with byte for byte in tests/test_gkr_tape_host.py.  No numpy arithmetic on field values; folds use plain %.

Every sumcheck is the sum over the cube of  sum_j [ M_j(y) V_j(y) + A_j(y) ]  for a list of table triples; a triple shorter than the cube (the subsets of
phase 2 have their own bit lengths) is the function of its own low variables times prod (1 - y_b) over the variables above them.  The round polynomial is
summed at 0, 1, 2 over the remaining cube and interpolated; nothing is derived from the previous claim.

    phase 1 of layer i   one triple over layer i-1: V its values; a gate g of layer i with weight eq(r_g, g) (times assert_random on an assert gate) and value
                         m x_u + a (m, a from its type and its second operand) adds weight*m to M[u] and weight*a to A[u]
    phase 2 of layer i   one triple per layer j < i over the subset of layer j: V the subset's values; a binary gate with weight eq(r_g, g) eq(r_u, u) and value
                         m y + a at x_u = claim_u adds to M[lv], A[lv]; the unary gates' values go to A[0] of the triple of layer i-1
    Liu of layer i       one triple over layer i-1: V its values, M = sig[0] eq(r_u, .) + sum over later layers k of sig[k-i+1] eq(r_v[k], slot) on the wires of
                         their subsets, A = 0

The prover checks itself as it goes (a failed check raises): q(0) + q(1) = claim in every round, claim_u = layer_mle(V_{i-1}, r_u), claims_v[j] against the
subset values at r_v, vr = layer_mle(V_{i-1}, r_liu), the closing value of phases 1 + 2 from predicates(), vr * liu_gr = claim, and the input layer's MLE at
the last r_liu."""
import verifier_sums as vs
from custom_circuits import MUL, ADD, SUB, ANTISUB, NAAB, ANTINAAB, MULC, ADDC, XOR, NOT, COPY, P, BINARY

ZERO, ONE, TWO = vs.ZERO, vs.ONE, (2, 0)
add, sub, mul = vs.add, vs.sub, vs.mul
HALF = ((P + 1) // 2, 0)


def neg(a):
    return sub(ZERO, a)


def _as_function_of_u(t, y, c):
    """The gate's value as m x + a in its first operand x, y the value of the second operand, c its constant."""
    if t == ADD: return ONE, y
    if t == SUB: return ONE, neg(y)
    if t == ANTISUB: return neg(ONE), y
    if t == MUL: return y, ZERO
    if t == NAAB: return neg(y), y                       # y - x y
    if t == ANTINAAB: return sub(ONE, y), ZERO           # x - x y
    if t == XOR: return sub(ONE, mul(TWO, y)), y         # x + y - 2 x y
    if t == ADDC: return ONE, c
    if t == MULC: return c, ZERO
    if t == COPY: return ONE, ZERO
    if t == NOT: return neg(ONE), ONE
    raise ValueError("gate type %d" % t)


def _as_function_of_v(t, x):
    """A binary gate's value as m y + a in its second operand y, x the value of the first."""
    if t == ADD: return ONE, x
    if t == SUB: return neg(ONE), x
    if t == ANTISUB: return ONE, neg(x)
    if t == MUL: return x, ZERO
    if t == NAAB: return sub(ONE, x), ZERO
    if t == ANTINAAB: return neg(x), x
    if t == XOR: return sub(ONE, mul(TWO, x)), x
    raise ValueError("gate type %d" % t)


def _unary_value(t, x, c):
    m, a = _as_function_of_u(t, ZERO, c)
    return add(mul(m, x), a)


class Triple:
    """M, V, A over 2^bits entries (shorter lists are zero above their end)."""

    def __init__(self, bits, M, V, A):
        n = 1 << bits
        pad = lambda t: list(t) + [ZERO] * (n - len(t))
        self.M, self.V, self.A = pad(M), pad(V), pad(A)
        self.tail = None                                 # once the triple is down to one entry: its value times prod (1 - r_b) over the later variables

    def at(self, t):
        """Its share of q(t): the sum over the remaining cube with the current variable at t."""
        if self.tail is not None or len(self.M) == 1:
            c = self.tail if self.tail is not None else add(mul(self.M[0], self.V[0]), self.A[0])
            return mul(c, sub(ONE, t))
        acc = ZERO
        for i in range(len(self.M) // 2):
            m = add(self.M[2 * i], mul(sub(self.M[2 * i + 1], self.M[2 * i]), t))
            v = add(self.V[2 * i], mul(sub(self.V[2 * i + 1], self.V[2 * i]), t))
            a = add(self.A[2 * i], mul(sub(self.A[2 * i + 1], self.A[2 * i]), t))
            acc = add(acc, add(mul(m, v), a))
        return acc

    def fix(self, r):
        if self.tail is not None or len(self.M) == 1:
            c = self.tail if self.tail is not None else add(mul(self.M[0], self.V[0]), self.A[0])
            self.tail = mul(c, sub(ONE, r))
            return
        fold = lambda T: [add(T[2 * i], mul(sub(T[2 * i + 1], T[2 * i]), r)) for i in range(len(T) // 2)]
        self.M, self.V, self.A = fold(self.M), fold(self.V), fold(self.A)

    def value(self):
        return self.tail if self.tail is not None else add(mul(self.M[0], self.V[0]), self.A[0])


def sumcheck(triples, rounds, challenges, claim, out, what):
    """`rounds` round polynomials (a, b, c of a x^2 + b x + c) appended to out; returns the closing claim.  Every triple ends with one entry."""
    for k in range(rounds):
        q0, q1, q2 = (ZERO, ZERO, ZERO)
        for T in triples:
            q0, q1, q2 = add(q0, T.at(ZERO)), add(q1, T.at(ONE)), add(q2, T.at(TWO))
        if add(q0, q1) != claim:
            raise AssertionError("%s, round %d: q(0) + q(1) is not the claim" % (what, k + 1))
        a = mul(HALF, add(sub(q2, mul(TWO, q1)), q0))
        b = sub(sub(q1, q0), a)
        out += [a, b, q0]
        r = challenges[k]
        claim = add(mul(add(mul(a, r), b), r), q0)
        for T in triples:
            T.fix(r)
    total = ZERO
    for T in triples:
        assert len(T.V) == 1
        total = add(total, T.value())
    if total != claim:
        raise AssertionError("%s: the closing claim is not the value of the folded tables" % what)
    return claim


def prove(w, off, tape):
    """The transcript (list of (re, im) in the golden layout) of the proof of wiring `w` (verifier_sums.Wiring) on `tape` (a sequence of (re, im) pairs laid out
    as `off`, gkr_tape_cases.Offsets)."""
    tp = [(int(a), int(b)) for a, b in tape]
    take = lambda slot: tp[slot[0]:slot[0] + slot[1]]
    val = vs.evaluate(w)
    n = w.n
    out = []
    r_liu = take(off.r0)
    claim = vs.layer_mle(val[n - 1], r_liu)
    out.append(claim)
    r_v = {}
    claims_v = {}
    for i in range(n - 1, 0, -1):
        L = w.layers[i]
        r_u, ar, sig, r_l = take(off.ru[i]), take(off.ar[i])[0], take(off.sig[i]), take(off.rl[i])
        r_v[i] = take(off.rv[i])
        size, psize, pbits = w.size[i], w.size[i - 1], w.bl[i - 1]
        beta_g = vs.eq_table(r_liu)
        weight = [mul(beta_g[g], ar) if L["a"][g] else beta_g[g] for g in range(size)]
        # phase 1
        M, A = [ZERO] * psize, [ZERO] * psize
        for g in range(size):
            t, u = L["ty"][g], L["u"][g]
            y = val[L["l"][g]][L["v"][g]] if t in BINARY else ZERO
            m, a = _as_function_of_u(t, y, L["c"][g])
            M[u] = add(M[u], mul(weight[g], m))
            A[u] = add(A[u], mul(weight[g], a))
        T = Triple(pbits, M, val[i - 1], A)
        claim = sumcheck([T], pbits, r_u, claim, out, "layer %d, phase 1" % i)
        claim_u = T.V[0]
        if claim_u != vs.layer_mle(val[i - 1], r_u):
            raise AssertionError("layer %d: claim_u is not V_{i-1}(r_u)" % i)
        out.append(claim_u)
        # phase 2
        have_p2 = w.max_dad_bl[i] != -1
        if have_p2:
            beta_u = vs.eq_table(r_u)
            Ms = [[ZERO] * max(1, w.dad_size[i][j]) for j in range(i)]
            As = [[ZERO] * max(1, w.dad_size[i][j]) for j in range(i)]
            for g in range(size):
                t = L["ty"][g]
                x = mul(weight[g], beta_u[L["u"][g]])
                if t in BINARY:
                    m, a = _as_function_of_v(t, claim_u)
                    j, k = L["l"][g], L["lv"][g]
                    Ms[j][k] = add(Ms[j][k], mul(x, m))
                    As[j][k] = add(As[j][k], mul(x, a))
                else:
                    As[i - 1][0] = add(As[i - 1][0], mul(x, _unary_value(t, claim_u, L["c"][g])))
            subset = [[val[j][wire] for wire in w.dad_id[i][j]] for j in range(i)]
            Ts = [Triple(w.dad_bl[i][j], Ms[j], subset[j], As[j]) for j in range(i)]
            claim = sumcheck(Ts, w.max_dad_bl[i], r_v[i], claim, out, "layer %d, phase 2" % i)
            claims_v[i] = [T.V[0] for T in Ts]
            for j in range(i):
                if claims_v[i][j] != vs.layer_mle(subset[j], r_v[i][:w.dad_bl[i][j]]):
                    raise AssertionError("layer %d: claims_v[%d] is not the subset's values at r_v" % (i, j))
            out += claims_v[i]
        else:
            claims_v[i] = [ZERO] * i
        # the closing value of phases 1 + 2 from the wiring predicates
        pr = vs.predicates(w, i, r_liu, ar, r_u, r_v[i])
        bv0 = ONE
        for r in r_v[i]:
            bv0 = mul(bv0, sub(ONE, r))
        cu = claim_u
        final = mul(bv0, add(add(mul(pr[1], sub(ONE, cu)), mul(add(add(pr[0], pr[2]), pr[3]), cu)), pr[4]))
        if have_p2:
            for j in range(i):
                cv = claims_v[i][j]
                uv = mul(cu, cv)
                terms = {ADD: add(cu, cv), SUB: sub(cu, cv), ANTISUB: sub(cv, cu), MUL: uv, NAAB: sub(cv, uv), ANTINAAB: sub(cu, uv),
                         XOR: sub(add(cu, cv), mul(TWO, uv))}
                for t, x in terms.items():
                    final = add(final, mul(pr[5 + vs.R_SLOT[t] * i + j], x))
        if final != claim:
            raise AssertionError("layer %d: the closing claim of phases 1 + 2 is not the value the wiring predicates give" % i)
        # Liu
        claim = mul(sig[0], claim_u)
        for k in range(i, n):
            claim = add(claim, mul(sig[k - i + 1], claims_v[k][i - 1]))
        M = [mul(sig[0], x) for x in vs.eq_table(r_u)[:psize]]
        for k in range(i, n):
            ids = w.dad_id[k][i - 1]
            if ids:
                bg = vs.eq_table(r_v[k][:w.dad_bl[k][i - 1]])
                for slot, wire in enumerate(ids):
                    M[wire] = add(M[wire], mul(sig[k - i + 1], bg[slot]))
        T = Triple(pbits, M, val[i - 1], [ZERO] * psize)
        claim = sumcheck([T], pbits, r_l, claim, out, "layer %d, Liu" % i)
        vr = T.V[0]
        if vr != vs.layer_mle(val[i - 1], r_l):
            raise AssertionError("layer %d: vr is not V_{i-1}(r_liu)" % i)
        if mul(vr, vs.liu_gr(w, i, r_u, r_v, sig, r_l)) != claim:
            raise AssertionError("layer %d: vr * gr is not the closing claim of the Liu sumcheck" % i)
        out.append(vr)
        claim, r_liu = vr, r_l
    if claim != vs.layer_mle(w.inputs, r_liu):
        raise AssertionError("the last claim is not the input layer's MLE at r_liu")
    assert len(out) == off.n_tr
    return out


def to_bytes(elements):
    return b"".join(int(a).to_bytes(8, "little") + int(b).to_bytes(8, "little") for a, b in elements)
