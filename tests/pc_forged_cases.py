"""The table of forged commitments shared by tests/test_pc_forged_host.py (CPU) and tests/test_gpu_forged_commitments.py (device loops): WHAT is forged, and
what the protocol says must come of it.  The expected verdict and name of every case are asked of the definition-level verifier (tests/pc_verifier_ref.py) by the
tests; `must` below is the condition the table was built to meet (the check that has to fire), asserted of that reference — None only at the one corner where
the protocol cannot see the change (CORNER).

A case: {"id", "family" (FAMILIES), "q": the (re-committed) proof, "kw": replaced arguments of the verifier, "must": name or None, "rep": the repetition that must reject or None,
"control": (proof, kw) made by the same machinery with no value changed}."""
import numpy as np

import masked_verifier_cases as mvc
import pc_array_inputs as pai
import pc_forge as forge
import pc_masked_inputs as pmi
import pc_verifier_ref as vref
import pc_verify_ref as ref

SLICES = (0, 1, 31, 63)
D = (3, 5)                                           # what a changed value moves by: non-zero in both limbs
CORNER = 64                                          # a position s0 that is a multiple of 32: x0^N = x1^N = 1 there and h drops out of the relation
MID, CORNER_REP = 11, 16
FINAL_ENTRIES = ((0, 0), (0, 1), (15, 1), (7, 0))    # (i, hi); (0, 0) is the entry all others are compared with
FAMILIES = ("arguments", "final", "lh", "levels")
PROOFS = [(9, "zero"), (9, "uniform"), (10, "zero"), (10, "uniform")]
_CACHE = {}


def proof(ob, n, kind):
    """kind: "zero" (ms = 1), "uniform" (ms = 8), "point" (zero mask, the public vector is eq(point, .): p["point"])"""
    if (n, kind) in _CACHE:
        return _CACHE[(n, kind)]
    x = dict(pai.inputs("uniform", n))
    point = None
    if kind == "point":
        point = np.random.default_rng(77 + n).integers(0, ref.P, size=(n, 2), dtype=np.uint64)
        x["pub"] = np.array(ref.eq_table([(int(a), int(b)) for a, b in point]), dtype=np.uint64)
    if kind == "uniform":
        f = pmi.family("uniform", n, 8)
    else:
        f = {"pri_mask": np.zeros((8, 2), np.uint64), "pub_mask": np.zeros((1, 2), np.uint64), "r": x["r"]}
    p = mvc.build(ob.lib(), n, x, f, seed=4200 + n)
    if kind != "uniform":
        p["ms"] = 1
    for seed in range(4300 + 100 * n, 4400 + 100 * n):         # the first seed whose positions open the forged leaves of l and h once (33 of at most 248 repeat often)
        lf = mvc.positions(n, seed)
        lf[CORNER_REP] = CORNER
        if lf.count(lf[0]) == lf.count(lf[-1]) == lf.count(CORNER) == lf.count(lf[MID]) == 1 and lf[MID] % 32:
            break
    else:
        raise AssertionError("no seed gives usable positions")
    p = forge.with_positions(p, lf)
    p["point"] = point
    _CACHE[(n, kind)] = p
    return p


def host_verify(vp, q, device=None, **kw):
    """Circuit.verify_commitment on q with some arguments replaced; point= takes pub's place"""
    a = dict(q, **kw)
    use_point = "point" in kw
    return vp.Circuit.verify_commitment(a["n"], a["claim"], a["root_l"], a["root_h"], a["all_sum"], a["r"], a["fri_roots"], a["final_code"], a["final_mask"],
                                        a["leaf0"], a["answer"], point=a["point"] if use_point else None, pub=None if use_point else a["pub"],
                                        pub_mask=a["pub_mask"], ms=a["ms"], device=device)


def ref_verify(q, **kw):
    a = dict(q, **kw)
    if "point" not in kw:
        a["point"] = None
    return vref.verify_p(a)


def _moved(arr, idx, d=D):
    out = np.array(arr, dtype=np.uint64, copy=True)
    out[idx] = forge.f_add(out[idx], d)
    return out


def level_reps(p):
    """{(k, upper): repetition} — for every level one repetition that compares its fold with the first and one with the second element of the pair, each the first
    to open its leaf of that level (so that the reject comes at that repetition)"""
    out = {}
    for rep in range(len(p["leaf0"])):
        for o, leaf, up in forge.opened(p, rep)[2:]:
            if (o - 2, up) not in out and forge.first_opener(p, o, leaf) == rep:
                out[(o - 2, up)] = rep
    return out


def cases(p):
    n, ln, N = p["n"], p["n"] - 6, 1 << (p["n"] - 6)
    R0 = vref.round_name(0)
    last = len(p["leaf0"]) - 1
    out, family = [], [None]

    def add(id_, must, q=p, kw=None, rep=None, control=None):
        out.append({"id": id_, "family": family[0], "q": q, "kw": kw or {}, "must": must, "rep": rep, "control": control or (p, {})})

    # ---- no re-hash needed ----
    family[0] = "arguments"
    for j in SLICES:
        j2 = (j + 1) % 64
        sums = _moved(_moved(p["all_sum"], j), j2, (ref.P - D[0], ref.P - D[1]))
        add("all_sum[%d] + d, all_sum[%d] - d" % (j, j2), R0, kw={"all_sum": sums}, rep=0, control=(p, {"all_sum": p["all_sum"].copy()}))
        for i in (j * N, j * N + N - 1):
            add("pub[%d] of slice %d" % (i, j), R0, kw={"pub": _moved(p["pub"], i)}, rep=0, control=(p, {"pub": p["pub"].copy()}))
    add("the claim alone", vref.SUMS, kw={"claim": np.array(forge.f_add(p["claim"], D), np.uint64)}, control=(p, {"claim": p["claim"].copy()}))
    for k in range(ln):
        add("r[%d] replaced" % k, vref.round_name(k), kw={"r": _moved(p["r"], k)}, rep=0, control=(p, {"r": p["r"].copy()}))
    if p["point"] is not None:
        for c in (0, ln - 1, ln, n - 1):
            add("point[%d]" % c, R0, kw={"point": _moved(p["point"], c)}, rep=0, control=(p, {"point": p["point"].copy()}))
    # ---- final codeword ----
    family[0] = "final"
    for s in SLICES:
        for i, hi in FINAL_ENTRIES:
            add("final entry (%d, %d) of slice %d" % (i, hi, s), vref.RS, kw={"final_code": _moved(p["final_code"], (i << 7) | (s << 1) | hi)},
                control=(p, {"final_code": p["final_code"].copy()}))
        fc = p["final_code"].copy()
        other = forge.f_add(fc[s << 1], D)
        for i in range(16):
            for hi in range(2):
                fc[(i << 7) | (s << 1) | hi] = other
        add("another constant as final codeword of slice %d" % s, vref.FINAL, kw={"final_code": fc}, rep=0)
    # ---- l and h, re-committed ----
    family[0] = "lh"
    for rep in (0, MID, CORNER_REP, last):
        s0 = p["leaf0"][rep]
        assert forge.first_opener(p, 0, s0) == rep
        for j in SLICES:
            for o in (0, 1):
                for h in (0, 1):
                    e = 2 * j + h
                    corner = o == 1 and s0 % 32 == 0
                    add("%s[%d] of repetition %d (s0 = %d)" % ("lh"[o], e, rep, s0), None if corner else R0,
                        q=forge.forge(p, [(o, s0, e, forge.f_add(p["vals"][o][s0, e], D))]), rep=None if corner else rep,
                        control=(forge.forge(p, [(o, s0, e, tuple(int(v) for v in p["vals"][o][s0, e]))]), {}))
    # ---- FRI level k, re-committed ----
    family[0] = "levels"
    for (k, up), rep in sorted(level_reps(p).items()):
        o, leaf, _ = forge.opened(p, rep)[2 + k]
        for j in SLICES:
            for which, must in (("compared", vref.round_name(k)), ("other", vref.round_name(k + 1) if k + 1 < ln else vref.FINAL)):
                e = 2 * j + (int(up) if which == "compared" else 1 - int(up))
                add("level %d, %s element %d of repetition %d (upper: %s)" % (k, which, e, rep, up), must,
                    q=forge.forge(p, [(o, leaf, e, forge.f_add(p["vals"][o][leaf, e], D))]), rep=rep,
                    control=(forge.forge(p, [(o, leaf, e, tuple(int(v) for v in p["vals"][o][leaf, e]))]), {}))
    return out
