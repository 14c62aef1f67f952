"""The circuits and point sets of tests/test_verifier_sums_host.py (CPU: the Python reference against the oracle's loops) and tests/test_gpu_verifier_sums.py
(GPU: the device entry points against both).  One list, so that the GPU file adds no expectation the CPU suite has not checked.  Everything is seeded; a
circuit, its wiring and every reference value are computed once per process and never modified."""
import functools

import numpy as np

import custom_circuits as cc
import verifier_sums as vs

P = cc.P
EDGE = (0, 1, 2, P - 2, P - 1)
SEED = 2024
CIRCUITS = {"ladder": cc.make_ladder, "unary_mid": cc.make_unary_mid, "zero_var": cc.make_zero_var, "dot": cc.make_dot_layers}
DEEP = (64, 3, 5)               # Circuit.randomize(64, 3, seed=5): 5 + 7 * 63 = 446 buckets at the top layer, the most the bucket key allows


@functools.lru_cache(maxsize=None)
def arrays(name):
    return CIRCUITS[name](SEED)


@functools.lru_cache(maxsize=None)
def oracle_circuit(name):
    import oracle_binding as ob
    return ob.Circuit.randomize(*DEEP[:2], seed=DEEP[2]) if name == "deep" else ob.Circuit.custom(*arrays(name))


@functools.lru_cache(maxsize=None)
def wiring(name):
    return vs.wiring_from(oracle_circuit(name), None if name == "deep" else arrays(name))


@functools.lru_cache(maxsize=None)
def values(name):
    return vs.evaluate(wiring(name))


def bits(x, n):
    return [((x >> i) & 1, 0) for i in range(n)]


def uniform(rng, n):
    return [(int(rng.integers(0, P)), int(rng.integers(0, P))) for _ in range(n)]


def edgy(rng, n):
    return [(EDGE[int(rng.integers(0, 5))], EDGE[int(rng.integers(0, 5))]) for _ in range(n)]


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def corner_gates(w, layer):
    """One gate of every (type, assert flag) pair the layer holds, and its first and last gate."""
    L = w.layers[layer]
    seen, out = set(), []
    for g in range(w.size[layer]):
        k = (L["ty"][g], L["a"][g])
        if k not in seen:
            seen.add(k)
            out.append(g)
    for g in (0, w.size[layer] - 1):
        if g not in out:
            out.append(g)
    return out


def corner_expectation(w, layer, g, assert_random):
    """vp_predicates at the corner of gate g, known without field arithmetic: one entry (Addc: two) is non-zero."""
    L = w.layers[layer]
    t, c = L["ty"][g], L["c"][g]
    f = assert_random if L["a"][g] else vs.ONE
    out = [vs.ZERO] * (5 + 7 * layer)
    if t in vs.R_SLOT:
        out[5 + vs.R_SLOT[t] * layer + L["l"][g]] = f
    elif t == cc.ADDC:
        assert not L["a"][g]                             # x + c = 0 cannot be made legal by construction: no Addc assert gate
        out[2] = vs.ONE
        out[4] = c
    elif t == cc.MULC:
        out[3] = c if not L["a"][g] else vs.mul(c, f)    # the one product a Mulc assert gate needs
    else:
        out[vs.HEAD[t]] = f
    return out


def filled_slots(w, layer):
    """The output slots of vp_predicates that at least one gate of the layer feeds; every other slot is a bucket the circuit leaves empty."""
    L = w.layers[layer]
    out = {5 + vs.R_SLOT[t] * layer + l for t, l in zip(L["ty"], L["l"]) if t in vs.R_SLOT}
    return out | {vs.HEAD[t] for t in L["ty"] if t in vs.HEAD} | ({4} if cc.ADDC in L["ty"] else set())


def dot_launches(size, n):
    """The launch table of one inner product <eq(r, .), table> over `size` entries at n variables, from the shapes include/vpgpu.h and the kernels' comments
    state: the two half tables (2^(n >> 1) + 2^(n - (n >> 1)) entries, one thread each, 256 per workgroup), k_dot_multi on one workgroup per 256 entries but
    at most 128, one k_dotfin_multi workgroup.  [(kernel, workgroups)]"""
    half = (1 << (n >> 1)) + (1 << (n - (n >> 1)))
    return [("k_beta_half_direct", -(-half // 256)), ("k_dot_multi", max(1, min(-(-size // 256), 128))), ("k_dotfin_multi", 1)]


@functools.lru_cache(maxsize=None)
def predicate_points(name, layer):
    """[(label, r_g, assert_random, r_u, r_v)]: two uniform points; assert_random 0, 1, p - 1 on the first; coordinates from {0, 1, 2, p - 2, p - 1} in both limbs,
    the all-(p - 1) and the all-zero point; the corners of corner_gates()."""
    w = wiring(name)
    ng, nu, nv = w.bl[layer], w.bl[layer - 1], w.n_v(layer)
    out = []
    for k in range(2):
        r = _rng(1, layer, k)
        out.append(("uniform%d" % k, uniform(r, ng), uniform(r, 1)[0], uniform(r, nu), uniform(r, nv)))
    _, g0, _, u0, v0 = out[0]
    for label, ar in (("assert_random=0", (0, 0)), ("assert_random=1", (1, 0)), ("assert_random=p-1", (P - 1, 0))):
        out.append((label, g0, ar, u0, v0))
    for k in range(2):
        r = _rng(2, layer, k)
        out.append(("edge%d" % k, edgy(r, ng), edgy(r, 1)[0], edgy(r, nu), edgy(r, nv)))
    m1 = (P - 1, P - 1)
    out.append(("all p-1", [m1] * ng, m1, [m1] * nu, [m1] * nv))
    out.append(("all zero", [(0, 0)] * ng, uniform(_rng(3, layer), 1)[0], [(0, 0)] * nu, [(0, 0)] * nv))
    L = w.layers[layer]
    ar = uniform(_rng(4, layer), 1)[0]
    for g in corner_gates(w, layer):
        lv = L["lv"][g] if L["ty"][g] in cc.BINARY else 0
        out.append(("corner gate %d" % g, bits(g, ng), ar, bits(L["u"][g], nu), bits(lv, nv)))
    return out


@functools.lru_cache(maxsize=None)
def predicate_reference(name, layer):
    w = wiring(name)
    return [vs.predicates(w, layer, rg, ar, ru, rv) for _, rg, ar, ru, rv in predicate_points(name, layer)]


@functools.lru_cache(maxsize=None)
def liu_points(name, layer):
    """[(label, r_u, r_v, sig, r_liu)], r_v[j] = the maxDadBitLength(j) phase-2 challenges of layer j >= layer (None below)."""
    w = wiring(name)
    n, nb = w.n, w.bl[layer - 1]

    def rv(draw):
        return [draw(w.n_v(j)) if j >= layer else None for j in range(n)]
    out = []
    for k in range(2):
        r = _rng(5, layer, k)
        out.append(("uniform%d" % k, uniform(r, nb), rv(lambda m: uniform(r, m)), uniform(r, n - layer + 1), uniform(r, nb)))
    r = _rng(6, layer)
    out.append(("edge", edgy(r, nb), rv(lambda m: edgy(r, m)), edgy(r, n - layer + 1), edgy(r, nb)))
    m1 = (P - 1, P - 1)
    out.append(("all p-1", [m1] * nb, rv(lambda m: [m1] * m), [m1] * (n - layer + 1), [m1] * nb))
    out.append(("all zero", [(0, 0)] * nb, rv(lambda m: [(0, 0)] * m), [(0, 0)] * (n - layer + 1), [(0, 0)] * nb))
    r = _rng(7, layer)
    wire = w.size[layer - 1] - 1
    out.append(("corner", bits(wire, nb), rv(lambda m: bits(0, m)), uniform(r, n - layer + 1), bits(wire, nb)))
    return out


@functools.lru_cache(maxsize=None)
def liu_reference(name, layer):
    w = wiring(name)
    return [vs.liu_gr(w, layer, ru, rv, sig, rl) for _, ru, rv, sig, rl in liu_points(name, layer)]


@functools.lru_cache(maxsize=None)
def mle_points(name, layer):
    w = wiring(name)
    n = w.bl[layer]
    out = [("uniform%d" % k, uniform(_rng(8, layer, k), n)) for k in range(2)]
    out.append(("edge", edgy(_rng(9, layer), n)))
    out.append(("all p-1", [(P - 1, P - 1)] * n))
    out.append(("all zero", [(0, 0)] * n))
    out.append(("corner last", bits(w.size[layer] - 1, n)))
    return out


@functools.lru_cache(maxsize=None)
def mle_reference(name, layer):
    val = values(name)[layer]
    return [vs.layer_mle(val, r) for _, r in mle_points(name, layer)]


# which layers each entry point is checked on
PREDICATE_LAYERS = [("ladder", i) for i in range(1, 6)] + [("unary_mid", i) for i in range(1, 5)] + [("zero_var", 1), ("zero_var", 2)] + [("deep", 63), ("deep", 1)]
LIU_LAYERS = [("ladder", 1), ("ladder", 4), ("ladder", 5), ("unary_mid", 1), ("unary_mid", 2), ("unary_mid", 3), ("unary_mid", 4), ("zero_var", 2)]
MLE_LAYERS = [("dot", i) for i in range(8)] + [("ladder", 5), ("unary_mid", 2)]
