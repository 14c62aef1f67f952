"""A cheating GKR prover in Python integers, on tests/verifier_sums.py through tests/gkr_verifier_ref.py's sums: transcripts that pass every check but the one the
forger leaves standing, which it declares.  A changed element under an otherwise honest transcript breaks the first check that reads it; here the prover repairs
what follows its lie, so that only one named check can tell.

It walks the verifier's schedule once, with the verifier's running claim S in hand, and sends each message either as the honest transcript has it or forged:
  re-made rounds   a round polynomial (a, b, (S - a - b) / 2) with seeded random a, b: p(0) + p(1) = S holds, and S becomes p(r);
  solved claims    a layer's closing value is affine in each claim: evaluated at 0 and at 1 and solved for S.  claim_u on a layer without phase 2; otherwise
                   claim_u is sent first (random, or the honest one where the layers below are to stay honest) and one claims_v[k] is solved, k the nearest
                   non-empty subset or a far one (k < layer - 1);
  Liu              the start sum is the verifier's own, from the claims sent; the rounds are re-made; vr is S / gr, the honest one, or the input layer's true value;
  pair change      a + 1, b - 1 in one round of an otherwise honest transcript: the same p(0) + p(1), another p(r) unless r is 0 or 1.
The challenges come from a gkr_verifier_ref.Tape (given up front) or a gkr_verifier_ref.Chained (Fiat-Shamir, drawn as the forger goes).  Messages in front of the
lie, and messages meant to be honest, are the elements of `honest`: the oracle's transcript on that tape, or the honest proof's old bytes on the chain.

A plan is a dict:
  {"pair": (kind, layer, round)}                                                   kind: phase1 / phase2 / liu
  {"lie": "vres" or (layer, round of its phase 1), "stop": (layer, how), "k": "near" / "far"}
The lie is carried from where it starts down to the stop layer — by re-made rounds, a random claim_u, a solved near claim, a re-made Liu sumcheck and vr = S / gr in
every layer above it — and ends there as `how` says:
  claims    rounds re-made, honest claims                                            -> (semi_final, layer)
  solved    rounds re-made, honest claim_u, claims_v[k] solved, honest below         -> Liu round 0 of layer k + 1, which joins the claims about layer k
  liu_vr    claims solved, Liu re-made, honest vr                                    -> (liu_semi_final, layer)
  vr_div    claims solved, Liu re-made, vr = S / gr, honest below                    -> the next check there is (at layer 1: input)
  true_vr   (layer 1) the same with vr = the input layer's true extension at r_liu   -> (liu_semi_final, 1)
forge() returns (elements, declared check); the declared check is None where the forged transcript is honest in value (a pair change at a challenge of 0 or 1; a far
claim whose sig weight on the tape is zero).  When a coefficient the forger must divide by is zero — gr, or the slope of the closing value — it raises DeadEnd
naming the layer: the lie cannot be carried past that layer's own closing check."""
import random

import gkr_verifier_ref as gv
from verifier_sums import add, mul, sub, ZERO, ONE

P = gv.P


class DeadEnd(Exception):
    def __init__(self, layer, what):
        Exception.__init__(self, "layer %d: %s is zero" % (layer, what))
        self.layer, self.what = layer, what


def inv(a):
    n = pow((a[0] * a[0] + a[1] * a[1]) % P, P - 2, P)
    return (a[0] * n % P, (P - a[1]) * n % P)


def subsets(w, layer, which="near"):
    """the non-empty subsets of the layer in the order the forger tries them: from the nearest down, or — far — from the farthest up among those below layer - 1"""
    full = [l for l in range(layer) if w.dad_size[layer][l]]
    return full[::-1] if which == "near" else [l for l in full if l < layer - 1 and l != full[-1]]


def next_check(off, check):
    order = gv.checks(off)
    return order[order.index(tuple(check)) + 1]


def forge(w, off, src, honest, plan, seed=0):
    n = off.n_layers
    chained = isinstance(src, gv.Chained)
    rng = random.Random(seed)
    rnd = lambda: (rng.randrange(P), rng.randrange(P))
    half = inv((2, 0))
    out = []
    pair = tuple(plan["pair"]) if "pair" in plan else None
    lie = plan.get("lie")
    stop_layer, how = plan.get("stop", (0, None))
    assert pair or (lie == "vres" or off.bl[lie[0] - 1] > lie[1]) and how in ("claims", "solved", "liu_vr", "vr_div", "true_vr")
    assert how != "true_vr" or stop_layer == 1
    st = {"lying": False, "done": False, "declared": None}

    def send(x=None):
        x = honest[len(out)] if x is None else x
        out.append(x)
        src.absorb(x)
        return x

    def forging():
        return st["lying"] and not st["done"]

    def rounds(kind, layer, slot, k, s):
        r = []
        for j in range(k):
            if kind == "phase1" and lie == (layer, j):
                st["lying"] = True
            if forging():
                a, b = rnd(), rnd()
                q = (send(a), send(b), send(mul(sub(sub(s, a), b), half)))
            else:
                q = (send(), send(), send())
            r.append(src.draw(slot + j))
            if pair == (kind, layer, j):                                # a r^2 + b r moves by r^2 - r
                st["declared"] = None if r[-1] in (ZERO, ONE) else next_check(off, pair)
            s = gv.poly_at(q, r[-1])
        return r, s

    if pair:
        at = {"phase1": "phase 1", "phase2": "phase 2", "liu": "Liu"}[pair[0]]
        i0 = [p for p in off.parts if p[0] == at and p[1] == pair[1]][0][2] + 3 * pair[2]
        honest = list(honest)
        honest[i0], honest[i0 + 1] = add(honest[i0], ONE), sub(honest[i0 + 1], ONE)

    r_g = [src.draw(off.r0[0] + j) for j in range(off.bl[n - 1])]
    if lie == "vres":
        st["lying"] = True
        s = send(rnd())
    else:
        s = send()
    r_v, claims = {}, {}
    for i in range(n - 1, 0, -1):
        last = forging() and i == stop_layer
        ar = src.draw(off.ar[i][0])
        r_u, s = rounds("phase1", i, off.ru[i][0], off.bl[i - 1], s)
        last = last or (forging() and i == stop_layer)                 # a lie that starts in this layer's phase 1
        phase2 = off.mdb[i] != -1
        solve = forging() and not (last and how == "claims")
        keep_u = not forging() or (last and how in ("claims", "solved"))
        r_v[i], claims[i] = [], [ZERO] * i
        if not phase2:
            if solve:
                v0 = gv.closing_value(w, i, r_g, ar, r_u, [], ZERO, claims[i])
                slope = sub(gv.closing_value(w, i, r_g, ar, r_u, [], ONE, claims[i]), v0)
                if slope == ZERO:
                    raise DeadEnd(i, "the slope of the closing value in claim_u")
                cu = send(mul(sub(s, v0), inv(slope)))
                k = i - 1
            else:
                cu = send()
        else:
            cu = send() if keep_u else send(rnd())
            r_v[i], s = rounds("phase2", i, off.rv[i][0], off.mdb[i], s)
            cv = [honest[len(out) + l] for l in range(i)]
            if solve:
                order = subsets(w, i, plan.get("k", "near") if last else "near")
                assert order
                for k in order:                                          # the first subset in whose claim the closing value moves
                    old = cv[k]
                    cv[k] = ZERO
                    v0 = gv.closing_value(w, i, r_g, ar, r_u, r_v[i], cu, cv)
                    cv[k] = ONE
                    slope = sub(gv.closing_value(w, i, r_g, ar, r_u, r_v[i], cu, cv), v0)
                    if slope != ZERO:
                        break
                    cv[k] = old
                else:
                    raise DeadEnd(i, "the slope of the closing value in each of claims_v%r" % (order,))
                cv[k] = mul(sub(s, v0), inv(slope))
            claims[i] = [send(x) for x in cv]
        sig = [src.draw(off.sig[i][0] + j) for j in range(n)]
        if last and how == "claims":
            st["done"], st["declared"] = True, ("semi_final", i, -1)
        if last and how == "solved":
            st["done"] = True
            if chained:
                # The old bytes behind the claims meet new challenges: sig is new, so Liu's start sum is, and its first check fails.  One exception: a Liu sumcheck
                # without a round, all of whose claims are honest (k is a far layer), tests vr gr = S, which holds for every sig; S = vr is then the old one, round
                # 0 of the next phase 1 compares old with old, and the first check that reads a challenge drawn behind the lie is the one behind it.
                st["declared"] = next_check(off, ("semi_final", i, -1))
                if st["declared"] == ("liu_semi_final", i, -1) and k != i - 1:
                    assert next_check(off, st["declared"]) == ("phase1", i - 1, 0)
                    st["declared"] = next_check(off, ("phase1", i - 1, 0))
            else:
                weight = src.draw(off.sig[k + 1][0] + (i - k)) if k + 1 != i else sig[1 if phase2 else 0]
                st["declared"] = None if weight == ZERO else ("liu", k + 1, 0) if off.bl[k] else ("liu_semi_final", k + 1, -1)
        s = gv.liu_start(w, i, sig, cu, claims)
        r_l, s = rounds("liu", i, off.rl[i][0], off.bl[i - 1], s)
        if forging():
            if last and how == "liu_vr":
                vr = send()
                st["done"], st["declared"] = True, ("liu_semi_final", i, -1)
            elif last and how == "true_vr":
                vr = send(gv.input_value(w, r_l))
                st["done"], st["declared"] = True, ("liu_semi_final", 1, -1)
            else:
                gr = gv.liu_gr(w, i, r_u, r_v, sig, r_l)
                if gr == ZERO:
                    raise DeadEnd(i, "gr")
                vr = send(mul(s, inv(gr)))
                if last:
                    st["done"], st["declared"] = True, next_check(off, ("liu_semi_final", i, -1))
        else:
            vr = send()
        s, r_g = vr, r_l
    assert len(out) == off.n_tr and (pair or st["done"])
    return out, st["declared"]
