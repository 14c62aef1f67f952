"""The verifier's O(|C|) loops (src/verifier.cpp:50-113 wiring predicates, :311-323 the Liu `gr`, :363-389 a layer's multilinear extension) in plain
Python integers: the reference the device entry points vp_predicates / vp_liu_gr / vp_layer_mle are compared with, value by value.  No numpy arithmetic on
field values: F_p^2 is a pair (re, im) of Python ints, p = 2^61 - 1, i^2 = -1.  Written as the sums of oracle/vp_oracle.cpp (VerifierSums), not as its code:
no half tables, no in-place scaling of beta_g, one loop per layer."""
from custom_circuits import MUL, ADD, SUB, ANTISUB, NAAB, ANTINAAB, INPUT, MULC, ADDC, XOR, NOT, COPY, P, BINARY

ZERO, ONE = (0, 0), (1, 0)
COEFF_R_ORDER = (ADD, SUB, ANTISUB, MUL, NAAB, ANTINAAB, XOR)          # include/vpgpu.h: out[5 + t * layer + l]
R_SLOT = {t: k for k, t in enumerate(COEFF_R_ORDER)}
HEAD = {COPY: 0, NOT: 1, ADDC: 2, MULC: 3}                             # out[0..4), out[4] = bias


def add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def eq_table(r):
    """Entry j = prod over the bits of j: r[i] for a set bit i, 1 - r[i] otherwise (bit 0 of j goes with r[0])."""
    t = [ONE]
    for ri in r:
        ri = (int(ri[0]), int(ri[1]))
        no = sub(ONE, ri)
        t = [mul(x, no) for x in t] + [mul(x, ri) for x in t]
    return t


def ceil_log2(x):
    b = 0
    while (1 << b) < x:
        b += 1
    return b


class Wiring:
    """A layered circuit as plain lists, with the subset numbering of subsetInit (src/circuit.cpp:43-80) taken from the gates' lv and rebuilt into dadId.
    layers[i] = dict(ty, l, u, v, lv, c, a) of lists (c: (re, im) pairs); inputs = the layer-0 values."""

    def __init__(self, layers, inputs):
        self.layers = layers
        self.inputs = [(int(x) % P, 0) for x in inputs]
        self.n = len(layers)
        self.size = [len(inputs)] + [len(L["ty"]) for L in layers[1:]]
        self.bl = [ceil_log2(s) for s in self.size]
        self.dad_id, self.dad_size, self.dad_bl, self.max_dad_bl = [None], [None], [None], [None]
        for i in range(1, self.n):
            L = layers[i]
            ids = [dict() for _ in range(i)]
            for g in range(self.size[i]):
                if L["ty"][g] in BINARY:
                    slot = ids[L["l"][g]].setdefault(L["lv"][g], L["v"][g])
                    assert slot == L["v"][g], "two wires in one subset slot"
            for j in range(i):
                assert sorted(ids[j]) == list(range(len(ids[j]))), "subset slots are not 0 .. size-1"
            self.dad_id.append([[ids[j][k] for k in range(len(ids[j]))] for j in range(i)])
            self.dad_size.append([len(ids[j]) for j in range(i)])
            self.dad_bl.append([ceil_log2(len(ids[j])) if ids[j] else 0 for j in range(i)])          # empty subset: size 0, bit length 0 (oracle: subset_init)
            self.max_dad_bl.append(max([ceil_log2(len(ids[j])) for j in range(i) if ids[j]], default=-1))

    def n_v(self, layer):
        return max(0, self.max_dad_bl[layer])


def wiring_from(oc, arrays=None):
    """oc: the oracle's circuit (its export carries lv).  arrays: the seven arrays the circuit was built from (constants and assert flags come from them, and
    ty / l / u / v must agree with the export); None for a circuit without constants and assert gates (randomize), whose inputs the oracle gives."""
    import numpy as np
    n = oc.layers
    sizes = [oc.layer_size(i) for i in range(n)]
    off = np.concatenate([[0], np.cumsum(sizes)])
    layers = [None]
    for i in range(1, n):
        e = oc.export_layer(i)
        L = {k: [int(x) for x in e[k]] for k in ("ty", "l", "u", "v", "lv")}
        if arrays is not None:
            lo, hi = int(off[i]), int(off[i + 1])
            assert L["ty"] == [int(x) for x in arrays[1][lo:hi]] and L["u"] == [int(x) for x in arrays[3][lo:hi]]
            assert all(L["l"][g] == int(arrays[2][lo + g]) and L["v"][g] == int(arrays[4][lo + g]) for g in range(sizes[i]) if L["ty"][g] in BINARY)
            L["c"] = [(int(a), int(b)) for a, b in arrays[5][lo:hi]]
            L["a"] = [int(x) for x in arrays[6][lo:hi]]
        else:
            assert all(t in BINARY or t in (NOT, COPY) for t in L["ty"])
            L["c"] = [ZERO] * sizes[i]
            L["a"] = [0] * sizes[i]
        layers.append(L)
    if arrays is not None:
        inputs = [int(x) for x in arrays[3][:sizes[0]]]
    else:
        e = oc.export_layer(0)
        inputs = [int(x) for x in e["u"]]
    return Wiring(layers, inputs)


def predicates(w, layer, r_g, assert_random, r_u, r_v):
    """The 5 + 7 * layer values of vp_predicates: coeff_l[Copy], [Not], [Addc], [Mulc], bias (without the beta_v[0] factor), then coeff_r[t][l]."""
    L = w.layers[layer]
    assert len(r_g) == w.bl[layer] and len(r_u) == w.bl[layer - 1] and len(r_v) == w.n_v(layer)
    bg, bu, bv = eq_table(r_g), eq_table(r_u), eq_table(r_v)
    ar = (int(assert_random[0]), int(assert_random[1]))
    out = [ZERO] * (5 + 7 * layer)
    ty, ll, uu, lv, cc, aa = L["ty"], L["l"], L["u"], L["lv"], L["c"], L["a"]
    for g in range(w.size[layer]):
        x = bg[g]
        if x == ZERO:
            continue
        x = mul(x, bu[uu[g]])
        if aa[g]:
            x = mul(x, ar)
        t = ty[g]
        if t in R_SLOT:
            k = 5 + R_SLOT[t] * layer + ll[g]
            out[k] = add(out[k], mul(x, bv[lv[g]]))
        elif t == ADDC:
            out[2] = add(out[2], x)
            out[4] = add(out[4], mul(x, cc[g]))
        elif t == MULC:
            out[3] = add(out[3], mul(x, cc[g]))
        else:
            out[HEAD[t]] = add(out[HEAD[t]], x)
    return out


def liu_gr(w, layer, r_u, r_v, sig, r_liu):
    """gr of verifyLiu(layer): sig[0] * sum_g eq(r_u, g) eq(r_liu, g) over layer - 1, plus for every later layer j >= layer
    sig[j - layer + 1] * sum_k eq(r_v[j][:dadBitLength[j][layer - 1]], k) eq(r_liu, dadId[j][layer - 1][k]).  An empty subset adds nothing."""
    pre = layer - 1
    assert len(r_u) == w.bl[pre] and len(r_liu) == w.bl[pre]
    bl_, bu = eq_table(r_liu), eq_table(r_u)
    s0 = (int(sig[0][0]), int(sig[0][1]))
    acc = ZERO
    for g in range(w.size[pre]):
        acc = add(acc, mul(bu[g], bl_[g]))
    gr = mul(s0, acc)
    for j in range(layer, w.n):
        ids = w.dad_id[j][pre]
        if not ids:
            continue
        bg = eq_table(list(r_v[j])[:w.dad_bl[j][pre]])
        acc = ZERO
        for k, wire in enumerate(ids):
            acc = add(acc, mul(bg[k], bl_[wire]))
        s = sig[j - pre]
        gr = add(gr, mul((int(s[0]), int(s[1])), acc))
    return gr


def layer_mle(values, r):
    assert len(values) <= 1 << len(r)
    b = eq_table(r)
    acc = ZERO
    for g, x in enumerate(values):
        if b[g] != ZERO:
            acc = add(acc, mul(b[g], x))
    return acc


def evaluate(w):
    """prover::evaluate (src/prover.cpp:27-91): the values of every layer."""
    val = [w.inputs]
    two = (2, 0)
    for i in range(1, w.n):
        L = w.layers[i]
        pre = val[i - 1]
        cur = []
        for g in range(w.size[i]):
            t, x = L["ty"][g], pre[L["u"][g]]
            if t in BINARY:
                y = val[L["l"][g]][L["v"][g]]
                if t == ADD: z = add(x, y)
                elif t == SUB: z = sub(x, y)
                elif t == ANTISUB: z = sub(y, x)
                elif t == MUL: z = mul(x, y)
                elif t == NAAB: z = sub(y, mul(x, y))
                elif t == ANTINAAB: z = sub(x, mul(x, y))
                else: z = sub(add(x, y), mul(two, mul(x, y)))
            elif t == ADDC: z = add(x, L["c"][g])
            elif t == MULC: z = mul(x, L["c"][g])
            elif t == COPY: z = x
            elif t == NOT: z = sub(ONE, x)
            else: raise ValueError("gate type %d" % t)
            cur.append(z)
        val.append(cur)
    return val
