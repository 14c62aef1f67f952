"""The GKR verifier of an unlayered circuit in Python integers, written from the protocol on tests/verifier_sums.py (predicates, liu_gr, layer_mle) — not from
host/verifier.cpp — and the two places its challenges can come from.  The verdict the host verifier (and its device loops) is held to on forged transcripts
(tests/gkr_forge.py, tests/gkr_forged_cases.py).

The protocol, per layer i from the output layer down.  The running claim S starts as Vres, the prover's value of the output layer's extension at r_g.
  phase 1   bl[i-1] rounds over the wire u of layer i - 1: p(0) + p(1) = S, then S = p(r_u[j]).                                         fails as (phase1, i, j)
            claim_u = V_(i-1)(r_u).
  phase 2   where the layer has binary gates: maxDadBitLength rounds over the subset slot v, the same test.                               fails as (phase2, i, j)
            claims_v[l] = the extension of layer i's subset of layer l at r_v, one for every l < i.
  closing   S = sum over the gates g of eq(r_g, g) [assert_random if g is an assert gate] eq(r_u, u_g) eq(r_v, slot_g) gate_g(claim_u, claims_v[l_g]): the sum
            vp_predicates returns grouped by gate type (a unary gate sits in slot 0 of r_v).                                              fails as (semi_final, i, -1)
  Liu       every claim about layer i - 1 made so far — claim_u and claims_v[j][i-1] of every layer j >= i that reads it — joined with sig:
            S = sig[0] claim_u + sum_j sig[j-i+1] claims_v[j][i-1]; bl[i-1] rounds over the wires of layer i - 1.                          fails as (liu, i, j)
            vr = V_(i-1)(r_liu); S = vr * gr with gr the joined eq polynomial at r_liu (liu_gr).                                           fails as (liu_semi_final, i, -1)
            S = vr, r_g = r_liu.
  input     S = the input layer's extension at r_g (left to the commitment in the whole protocol: input_check=False).                     fails as (input, 0, -1)

verify() returns None or the first failed check (kind, layer, round).  Field elements are (re, im) pairs of Python ints; no numpy arithmetic on them."""
import numpy as np

import verifier_sums as vs
from verifier_sums import add, mul, sub, ZERO, ONE

P = vs.P
KINDS = ("phase1", "phase2", "semi_final", "liu", "liu_semi_final", "input")


def elements(tr):
    return [(int(a), int(b)) for a, b in np.frombuffer(bytes(tr), np.uint64).reshape(-1, 2)]


def to_bytes(el):
    return np.array(el, np.uint64).reshape(-1, 2).tobytes()


def poly_at(q, r):
    """q = (a, b, c): a x^2 + b x + c"""
    return add(mul(add(mul(q[0], r), q[1]), r), q[2])


def poly_sum(q):
    """p(0) + p(1)"""
    return add(add(q[0], q[1]), add(q[2], q[2]))


# ---- where the challenges come from ------------------------------------------------------------------------------------------------------------------------------
class Tape:
    """A tape given up front in gkr_tape_cases.Offsets layout: a challenge is read from its slot, whatever the prover sent."""

    def __init__(self, off, tape):
        assert len(tape) == off.n
        self.t = [(int(a), int(b)) for a, b in tape]

    def draw(self, slot):
        return self.t[slot]

    def absorb(self, x):
        pass


class Chained:
    """The Fiat-Shamir chain (pc_fs_ref.Chain) from `state`, in full_fs_ref.gkr_schedule's order: every element the prover sends is absorbed, every challenge is the
    next C(counter).  The caller draws in the schedule's order; .tape records each draw in its Offsets slot, .ch.s is the state."""

    def __init__(self, off, state):
        import pc_fs_ref as fs
        self.ch, self.ctr = fs.Chain(state), 0
        self.tape = np.zeros((off.n, 2), np.uint64)

    def draw(self, slot):
        x = self.ch.C(self.ctr)
        self.ctr += 1
        self.tape[slot] = x
        return x

    def absorb(self, x):
        self.ch.E(x)


# ---- the verifier's own sums, computed once per point -------------------------------------------------------------------------------------------------------------
_memo = {}


def _cached(key, f):
    if key not in _memo:
        if len(_memo) > 20000:
            _memo.clear()
        _memo[key] = f()
    return _memo[key]


def closing_terms(w, layer, r_g, ar, r_u, r_v):
    """(k0, ku, [(kv_l, kuv_l)]): the layer's closing value is k0 + ku cu + sum_l (kv_l cv[l] + kuv_l cu cv[l]).  From vp_predicates' groups: Copy, Not, Addc,
    Mulc, the Addc constants (all times eq(r_v, 0) = prod (1 - r_v[j])), then per earlier layer Add, Sub, AntiSub, Mul, Naab, AntiNaab, Xor."""
    def make():
        out = vs.predicates(w, layer, r_g, ar, r_u, r_v)
        slot0 = ONE
        for r in r_v:
            slot0 = mul(slot0, sub(ONE, r))
        copy, no, addc, mulc, bias = (mul(x, slot0) for x in out[:5])
        k0 = add(no, bias)                                               # Not: 1 - u;  Addc: u + c
        ku = add(sub(add(copy, addc), no), mulc)
        per = []
        for l in range(layer):
            a, s, asb, m, na, ana, x = (out[5 + t * layer + l] for t in range(7))
            ku = add(ku, add(add(a, s), add(sub(ana, asb), x)))            # u + v, u - v, v - u, u v, v - u v, u - u v, u + v - 2 u v
            kv = add(add(sub(a, s), asb), add(na, x))
            kuv = sub(sub(sub(m, na), ana), add(x, x))
            per.append((kv, kuv))
        return k0, ku, per
    return _cached(("closing", id(w), layer, tuple(r_g), ar, tuple(r_u), tuple(r_v)), make)


def closing_value(w, layer, r_g, ar, r_u, r_v, cu, cv):
    k0, ku, per = closing_terms(w, layer, r_g, ar, r_u, r_v)
    s = add(k0, mul(ku, cu))
    for l, (kv, kuv) in enumerate(per):
        s = add(s, mul(add(kv, mul(kuv, cu)), cv[l]))
    return s


def liu_start(w, layer, sig, cu, claims):
    """claims[j]: claims_v of layer j (a layer without phase 2 makes none)"""
    s = mul(sig[0], cu)
    for j in range(layer, w.n):
        if w.dad_size[j][layer - 1]:
            s = add(s, mul(sig[j - layer + 1], claims[j][layer - 1]))
    return s


def liu_gr(w, layer, r_u, r_v, sig, r_liu):
    """r_v: {layer j: its r_v}"""
    rv = [r_v.get(j, []) for j in range(w.n)]
    return _cached(("gr", id(w), layer, tuple(r_u), tuple(tuple(x) for x in rv[layer:]), tuple(sig), tuple(r_liu)), lambda: vs.liu_gr(w, layer, r_u, rv, sig, r_liu))


def input_value(w, r):
    return _cached(("input", id(w), tuple(r)), lambda: vs.layer_mle(w.inputs, r))


def checks(off):
    """every check of a verification, in the order it is made"""
    out = []
    for i in range(off.n_layers - 1, 0, -1):
        out += [("phase1", i, j) for j in range(off.bl[i - 1])]
        out += [("phase2", i, j) for j in range(max(0, off.mdb[i]))]
        out.append(("semi_final", i, -1))
        out += [("liu", i, j) for j in range(off.bl[i - 1])]
        out.append(("liu_semi_final", i, -1))
    return out + [("input", 0, -1)]


# ---- the verifier ---------------------------------------------------------------------------------------------------------------------------------------------------
def verify(w, off, src, tr, skip_predicates=False, input_check=True, state=None):
    """tr: the transcript as elements or bytes (off.n_tr elements).  src: Tape or Chained.  state: a dict that receives what the walk ended with ("claim", "point")."""
    el = tr if isinstance(tr, list) else elements(tr)
    assert len(el) == off.n_tr and w.n == off.n_layers and [w.bl[i] for i in range(w.n)] == off.bl
    pos = [0]

    def take(k=1):
        x = el[pos[0]:pos[0] + k]
        pos[0] += k
        for e in x:
            src.absorb(e)
        return x

    def rounds(kind, layer, slot, k, s):
        r = []
        for j in range(k):
            q = take(3)
            if poly_sum(q) != s:
                return None, (kind, layer, j)
            r.append(src.draw(slot + j))
            s = poly_at(q, r[-1])
        return (r, s), None

    n = off.n_layers
    r_g = [src.draw(off.r0[0] + j) for j in range(off.bl[n - 1])]
    s = take()[0]
    r_v, claims = {}, {}
    for i in range(n - 1, 0, -1):
        ar = src.draw(off.ar[i][0])
        got, fail = rounds("phase1", i, off.ru[i][0], off.bl[i - 1], s)
        if fail:
            return fail
        r_u, s = got
        cu = take()[0]
        r_v[i], claims[i] = [], [ZERO] * i
        if off.mdb[i] != -1:
            got, fail = rounds("phase2", i, off.rv[i][0], off.mdb[i], s)
            if fail:
                return fail
            r_v[i], s = got
            claims[i] = take(i)
        if not skip_predicates and closing_value(w, i, r_g, ar, r_u, r_v[i], cu, claims[i]) != s:
            return ("semi_final", i, -1)
        sig = [src.draw(off.sig[i][0] + j) for j in range(n)]
        s = liu_start(w, i, sig, cu, claims)
        got, fail = rounds("liu", i, off.rl[i][0], off.bl[i - 1], s)
        if fail:
            return fail
        r_l, s = got
        vr = take()[0]
        if mul(vr, liu_gr(w, i, r_u, r_v, sig, r_l)) != s:
            return ("liu_semi_final", i, -1)
        s, r_g = vr, r_l
    assert pos[0] == off.n_tr
    if state is not None:
        state.update(claim=s, point=r_g)
    if input_check and input_value(w, r_g) != s:
        return ("input", 0, -1)
    return None
