"""Random layered circuits that use EVERY gate type of the reference's enum gateType (src/inputCircuit.hpp:13-15),
including the ones its .pws loader never produces (Addc, Mulc, Copy, AntiNaab, AntiSub) and assert gates
(src/prover.cpp:18-21,209-212), for parity tests between the oracle and the device."""
import numpy as np

MUL, ADD, SUB, ANTISUB, NAAB, ANTINAAB, INPUT, MULC, ADDC, XOR, NOT, COPY = range(12)
P = (1 << 61) - 1


def make(seed, layer_sizes, with_asserts=True, values=None, real_consts=False):
    """values: draw the inputs and the Mulc / Addc constants from this sequence instead of uniformly from [0, p) (edge values: tests/test_gpu_field_edges.py);
    real_consts: constants (c, 0), so that a circuit with real inputs has real values throughout.  The defaults leave every seed's circuit as it was."""
    rng = np.random.default_rng(seed)

    def draw():
        return int(rng.integers(0, P)) if values is None else int(values[int(rng.integers(0, len(values)))])
    ty, l, u, v, c, a = [], [], [], [], [], []
    for i, n in enumerate(layer_sizes):
        for g in range(n):
            if i == 0:
                ty.append(INPUT); l.append(-1); u.append(draw()); v.append(0); c.append((0, 0)); a.append(0)
                continue
            if with_asserts and g == n - 1:
                # x - x == 0: a legal assert gate (both operands the same wire of layer i-1)
                w = int(rng.integers(0, layer_sizes[i - 1]))
                ty.append(SUB); l.append(i - 1); u.append(w); v.append(w); c.append((0, 0)); a.append(1)
                continue
            t = int(rng.choice([MUL, ADD, SUB, ANTISUB, NAAB, ANTINAAB, MULC, ADDC, XOR, NOT, COPY]))
            ty.append(t)
            u.append(int(rng.integers(0, layer_sizes[i - 1])))
            if t in (MULC, ADDC, NOT, COPY):
                l.append(-1); v.append(0)
            else:
                ll = int(rng.integers(0, i))
                l.append(ll); v.append(int(rng.integers(0, layer_sizes[ll])))
            c.append(((draw(), 0) if real_consts else (draw(), draw())) if t in (MULC, ADDC) else (0, 0))
            a.append(0)
    return (np.array(layer_sizes, np.uint64), np.array(ty, np.int32), np.array(l, np.int32), np.array(u, np.uint64),
            np.array(v, np.uint64), np.array(c, np.uint64).reshape(-1, 2), np.array(a, np.uint8))


# ---- skewed circuits: fan-outs, subset sizes and row placements fixed by construction ---------------------------------------------
BINARY = (MUL, ADD, SUB, ANTISUB, NAAB, ANTINAAB, XOR)
UNARY = (MULC, ADDC, NOT, COPY)
ALL_TYPES = BINARY + UNARY
SKEWED_SIZES = [12001, 16383, 9001, 16384, 49153, 16001]      # layers 0-3 have bit length 14 (two of them odd-sized); layer 4 can put > 32768 gates on one wire
SKEWED_SINGLE_SIZES = [12001, 16383, 16384, 9001]             # only_type: three layers of bit length 14 below the gate layers
HEAVY = 16                                                    # VP_LIGHT_MAX: a row with more contributions is summed by the chunk kernels
HUGE = 33000                                                  # > 64 chunks of 512 contributions
P2_MIDS = {2: (4, 1000, 41), 3: (6, 100, 21), 5: (0, 600, 17)}    # distance below the gate layer -> (first wire, wires, contributions of the first wire)


def skewed_p1_pins(n, m):
    """Row (wire of the layer below, m wires) -> the number of gates, of a layer of n, that read it as u.  Heavy / heavy pair at rows 0 and 1; heavy even row 6 and
    heavy odd row 9 with light partners; heavy rows 4 and 10 beside empty rows; heavy rows on both sides of the 2^13 slice edge; the last valid row heavy (no partner
    when m is odd); in a layer that is large enough, row 2 with more than 64 chunks."""
    pins = {0: 1025, 1: 1024, 4: 513, 5: 0, 6: 512, 7: 1, 8: 16, 9: 511, 10: 17, 11: 0, m - 1: 100}
    if m > 8194:
        pins[8191] = 40; pins[8192] = 33
    if n >= 45000:
        pins[2] = HUGE; pins[3] = 3
    return pins


def skewed_p2_pins(n_asserts):
    """Wire of layer i-1 -> the number of BINARY gates of layer i that read it as v (wire w is slot w of the subset: the gates are ordered for that).  Wire 0 is
    the slot that also takes every unary gate of the layer (src/prover.cpp:314), its count is set by the caller."""
    return {1: 1025, 2: 1024, 3: 513, 4: 1, 5: 16, 6: 512, 7: 511, 8: 17}


def make_skewed(seed, layer_sizes=None, only_type=None, real_consts=False):
    """The same seven arrays as make(), with the contribution lists of the device inits shaped by construction (tests/test_skewed_circuits_host.py asserts it all
    from the arrays):
      phase 1 (gates of a layer sharing u): skewed_p1_pins; every other gate reads a wire outside the pinned rows;
      phase 2 (gates sharing an (l, v) slot): skewed_p2_pins on layer i-1, whose subset is as long as the layer's binary gates allow, up to 8200 wires (bit length
          14); P2_MIDS on layers i-2, i-3 and i-5 (subsets of 1000, 100 and 600 wires, the first wire heavy); no subset on layer i-4;
      Liu lists (the later layers' subsets that hold a wire): the subsets above overlap, so wires sit in none, one, or up to four of them — a list is at most as
          long as there are later layers;
      types: all eleven in every phase-1 row of >= 512 gates, all seven binary ones in every phase-2 slot of >= 512, all eleven in slot 0 of subset i-1;
      assert gates: Sub(w0, w0) as the last gate of each layer and AntiSub(w1, w1), inside the heavy rows 0 / 1 of phase 1 and the heavy slots 0 / 1 of phase 2.
    only_type = T: every gate of type T, and the Sub assert gate alone."""
    rng = np.random.default_rng(seed)
    sizes = list(layer_sizes if layer_sizes is not None else (SKEWED_SINGLE_SIZES if only_type is not None else SKEWED_SIZES))
    n_as = 1 if only_type is not None else 2
    ty = [np.full(sizes[0], INPUT, np.int32)]; l = [np.full(sizes[0], -1, np.int32)]
    u = [rng.integers(0, P, sizes[0]).astype(np.uint64)]; v = [np.zeros(sizes[0], np.uint64)]
    c = [np.zeros((sizes[0], 2), np.uint64)]; a = [np.zeros(sizes[0], np.uint8)]
    for i in range(1, len(sizes)):
        n, m, body = sizes[i], sizes[i - 1], sizes[i] - n_as
        pins = skewed_p1_pins(n, m)
        cnt = dict(pins); cnt[0] -= 1
        if n_as == 2:
            cnt[1] -= 1
        fixed = np.repeat(np.array(list(cnt.keys())), np.array(list(cnt.values())))
        assert len(fixed) <= body, "layer %d is too small for the pinned rows" % i
        free_rows = np.setdiff1d(np.arange(m), np.array(list(pins.keys())))
        uu = np.concatenate([fixed, rng.choice(free_rows, body - len(fixed))])
        if only_type is not None:
            tt = np.full(body, only_type, np.int32)
        else:
            tt = rng.choice(np.array(ALL_TYPES), size=body, p=[0.88 / 7] * 7 + [0.03] * 4).astype(np.int32)
            for row, k in cnt.items():
                if k >= 512:
                    tt[np.flatnonzero(uu == row)[:11]] = np.roll(np.array(ALL_TYPES), row)
        ll = np.full(body, -1, np.int32); vv = np.zeros(body, np.int64)
        is_bin = np.isin(tt, BINARY)
        n_bin, n_un = int(is_bin.sum()), int(body - is_bin.sum())
        if n_bin:
            pools = {t: list(rng.permutation(np.flatnonzero(tt == t))) for t in BINARY}
            order = rng.permutation(np.flatnonzero(is_bin)); used = np.zeros(body, bool); pos = [0]

            def take(k, cover):
                out = []
                for t in (BINARY if cover else ()):
                    while pools[t] and len(out) < k:
                        g = pools[t].pop()
                        if not used[g]:
                            used[g] = True; out.append(g); break
                while len(out) < k:
                    g = order[pos[0]]; pos[0] += 1
                    if not used[g]:
                        used[g] = True; out.append(g)
                return out

            def put(lay, wire, k, cover=False):
                g = take(k, cover or k >= 512)
                ll[g] = lay; vv[g] = wire
            put(i - 1, 0, (HUGE - n_un if n >= 45000 else 20) - 1, cover=True)
            p2 = skewed_p2_pins(n_as)
            for w, k in p2.items():
                put(i - 1, w, k - (1 if w == 1 and n_as == 2 else 0))
            for d, (w0, nw, k0) in P2_MIDS.items():
                if i - d >= 0:
                    put(i - d, w0, k0)
                    for w in range(w0 + 1, w0 + nw):
                        put(i - d, w, 1)
            left = n_bin - int(used.sum())
            D = min(8200 - 9, left)
            for w in range(9, 9 + D):
                put(i - 1, w, 1)
            rest = np.flatnonzero(is_bin & ~used)
            assert D > 0 or not len(rest)
            ll[rest] = i - 1; vv[rest] = rng.integers(9, 9 + max(D, 1), len(rest))
        cc = np.zeros((body, 2), np.uint64)
        isc = np.isin(tt, (MULC, ADDC))
        cc[isc, 0] = rng.integers(0, P, int(isc.sum()))
        if not real_consts:
            cc[isc, 1] = rng.integers(0, P, int(isc.sum()))
        aa = np.zeros(body, np.uint8)
        # gate order: the gates reading layer i-1 come last, by descending v, so that wire w is slot w of that subset (subsetInit numbers the wires by their
        # first use, walking the layer backwards: src/circuit.cpp:58-70); the Sub assert gate closes the layer
        key = np.where(ll == i - 1, m - vv, -1)
        if n_as == 2:
            tt = np.append(tt, ANTISUB); ll = np.append(ll, i - 1); uu = np.append(uu, 1); vv = np.append(vv, 1); key = np.append(key, m - 1)
            cc = np.vstack([cc, [[0, 0]]]); aa = np.append(aa, 1)
        pre = rng.permutation(len(tt))
        perm = pre[np.argsort(key[pre], kind="stable")]
        for arr, x, last in ((ty, tt, SUB), (l, ll, i - 1), (u, uu, 0), (v, vv, 0), (a, aa, 1)):
            arr.append(np.append(x[perm], last).astype(arr[0].dtype))
        c.append(np.vstack([cc[perm], [[0, 0]]]).astype(np.uint64))
    return (np.array(sizes, np.uint64), np.concatenate(ty), np.concatenate(l), np.concatenate(u), np.concatenate(v), np.concatenate(c), np.concatenate(a))


# ---- bucketed circuits: the size of every (type, operand layer) bucket of the verifier's wiring predicates fixed by construction -------------------------
def make_bucketed(seed, n_inputs, layer_buckets, v_wires=None, asserts=None):
    """The same seven arrays as make().  layer_buckets[i - 1] = {(type, operand layer; -1 for a unary type): number of gates} for gate layer i: the layer is
    exactly these gates, shuffled, so a bucket's members are scattered over it; u is uniform over layer i - 1.
    v_wires[(i, l)] = the number of distinct wires of layer l that layer i's binary gates read (default: as many as there are gates and wires), so the subset's
    size, and with it dadBitLength[i][l], is fixed too (tests/test_verifier_sums_host.py asserts all of it from the arrays).
    asserts[i] = the buckets of layer i that get ONE assert gate each: binary, unary (Copy) or unary with a constant (Mulc).  They are legal by construction:
    one input is 0, one Copy gate per layer (taken from its Copy bucket) carries that 0 upwards as far as the assert gates need it, and an assert gate reads
    nothing else (x op 0-wire pairs: 0 + 0, 0 * 0, 0 xor 0, ...; Copy(0); c * 0)."""
    rng = np.random.default_rng(seed)
    v_wires, asserts = v_wires or {}, asserts or {}
    sizes = [n_inputs]
    inp = rng.integers(0, P, n_inputs).astype(np.uint64)
    zero = [int(rng.integers(0, n_inputs))]
    inp[zero[0]] = 0
    ty = [np.full(n_inputs, INPUT, np.int32)]; l = [np.full(n_inputs, -1, np.int32)]; u = [inp]; v = [np.zeros(n_inputs, np.uint64)]
    c = [np.zeros((n_inputs, 2), np.uint64)]; a = [np.zeros(n_inputs, np.uint8)]
    chain_to = max(asserts, default=0) - 1
    for i, buckets in enumerate(layer_buckets, start=1):
        m = sizes[i - 1]
        for (t, lay) in buckets:
            assert (lay == -1) == (t in UNARY) and lay < i and t in ALL_TYPES
        keys = [k for k, cnt in buckets.items() if cnt]
        tt = np.concatenate([np.full(buckets[k], k[0], np.int32) for k in keys])
        ll = np.concatenate([np.full(buckets[k], k[1], np.int32) for k in keys])
        start = dict(zip(keys, np.concatenate([[0], np.cumsum([buckets[k] for k in keys])])[:-1]))
        n = len(tt)
        uu = rng.integers(0, m, n).astype(np.int64)
        vv = np.zeros(n, np.int64); aa = np.zeros(n, np.uint8)
        taken = {k: 0 for k in keys}

        def pin(key):
            g = int(start[key]) + taken[key]
            taken[key] += 1
            assert taken[key] <= buckets[key], "bucket %r of layer %d is too small for its pinned gates" % (key, i)
            uu[g] = zero[i - 1]
            return g
        carrier = pin((COPY, -1)) if i <= chain_to else None
        forced = {}
        for key in asserts.get(i, ()):
            g = pin(key)
            aa[g] = 1
            if key[1] >= 0:
                forced.setdefault(key[1], []).append(g)
        for lay in range(i):
            idx = np.flatnonzero(ll == lay)
            if not len(idx):
                continue
            k = min(v_wires.get((i, lay), sizes[lay]), sizes[lay], len(idx))
            f = np.array(forced.get(lay, []), np.int64)
            if len(f):
                others = np.setdiff1d(np.arange(sizes[lay]), [zero[lay]])
                wires = np.concatenate([[zero[lay]], rng.choice(others, k - 1, replace=False)])
                vv[f] = zero[lay]
                rest = rng.permutation(np.setdiff1d(idx, f))
                vv[rest[:k - 1]] = wires[1:]
                vv[rest[k - 1:]] = wires[rng.integers(0, k, max(len(rest) - (k - 1), 0))]
            else:
                wires = rng.choice(sizes[lay], k, replace=False)
                rest = rng.permutation(idx)
                vv[rest[:k]] = wires
                vv[rest[k:]] = wires[rng.integers(0, k, len(rest) - k)]
        cc = np.zeros((n, 2), np.uint64)
        isc = np.isin(tt, (MULC, ADDC))
        cc[isc] = rng.integers(0, P, (int(isc.sum()), 2))
        perm = rng.permutation(n)
        if carrier is not None:
            zero.append(int(np.flatnonzero(perm == carrier)[0]))
        else:
            zero.append(None)
        ty.append(tt[perm]); l.append(ll[perm]); u.append(uu[perm].astype(np.uint64)); v.append(vv[perm].astype(np.uint64)); c.append(cc[perm]); a.append(aa[perm])
        sizes.append(n)
    return (np.array(sizes, np.uint64), np.concatenate(ty), np.concatenate(l), np.concatenate(u), np.concatenate(v), np.concatenate(c), np.concatenate(a))


# The ladder circuit: gate layer 4 has four layers below it and carries every bucket size at which the device sums change shape (a wave strides a piece of
# <= 512 gates by 64 lanes; a bucket's pieces are added with a 64-lane stride, so HUGE = 65 pieces takes a second trip).  Naab and AntiNaab are empty for
# operand layer 3 and filled for layer 2; Sub is empty for layer 2; five types are empty for layer 1, whose subset (3 wires, bit length 2) is far shorter than
# the longest (600 wires of layer 0, bit length 10 = maxDadBitLength).  n_g = 16, n_u = 9, n_v = 10.  Addc feeds two sums (coeff_l[Addc] and bias): 513 gates
# here, 65 in layer 1.  Layer 1 (113 gates, bit length 7) holds an assert gate of each flag class, layer 4 too (inside HUGE, the 513-gate Xor bucket, Copy and
# Mulc).  Layer 5 is a small top layer.
LADDER_LAYER = 4
LADDER_INPUTS = 600
LADDER_BUCKETS = [
    {**{(t, 0): 5 for t in BINARY}, (COPY, -1): 4, (NOT, -1): 3, (MULC, -1): 6, (ADDC, -1): 65},
    {**{(t, 1): 20 for t in BINARY}, **{(t, 0): 17 for t in BINARY}, (COPY, -1): 11, (NOT, -1): 10, (MULC, -1): 10, (ADDC, -1): 10},
    {**{(t, 2): 40 for t in BINARY}, **{(t, 0): 20 for t in BINARY}, (MUL, 1): 30, (COPY, -1): 10, (NOT, -1): 10, (MULC, -1): 10, (ADDC, -1): 20},
    {(ADD, 3): HUGE, (MUL, 3): 1025, (SUB, 3): 1024, (XOR, 3): 513, (NAAB, 3): 0, (ANTINAAB, 3): 0, (ANTISUB, 3): 1,
     (NAAB, 2): 512, (ANTINAAB, 2): 511, (ANTISUB, 2): 65, (MUL, 2): 64, (ADD, 2): 63, (SUB, 2): 0, (XOR, 2): 1,
     (MUL, 1): 3, (XOR, 1): 2, (ADD, 1): 0, (SUB, 1): 0, (ANTISUB, 1): 0, (NAAB, 1): 0, (ANTINAAB, 1): 0,
     (MUL, 0): 513, (NAAB, 0): 1, (ANTINAAB, 0): 64, (SUB, 0): 511, (ADD, 0): 0, (XOR, 0): 65, (ANTISUB, 0): 512,
     (COPY, -1): 63, (NOT, -1): 1, (ADDC, -1): 513, (MULC, -1): 1024},
    {(ADD, 4): 6, (MUL, 4): 5, (XOR, 3): 2, (SUB, 0): 3, (NAAB, 2): 1, (COPY, -1): 1, (ADDC, -1): 1, (MULC, -1): 1},
]
LADDER_V_WIRES = {(4, 1): 3, (4, 0): 600, (4, 3): 400, (4, 2): 100}
LADDER_ASSERTS = {1: [(ADD, 0), (COPY, -1), (MULC, -1)], 4: [(ADD, 3), (XOR, 3), (COPY, -1), (MULC, -1)]}


def make_ladder(seed):
    return make_bucketed(seed, LADDER_INPUTS, LADDER_BUCKETS, LADDER_V_WIRES, LADDER_ASSERTS)


# A layer of unary gates only (layer 2) in the middle of a circuit: maxDadBitLength -1, no phase 2, vp_predicates with n_v = 0.  Layers 3 and 4 read it and the
# layers below it; layer 2's subset of layers 0 and 1 is empty, which the Liu sums of layers 1 and 2 meet.
UNARY_MID_LAYER = 2
UNARY_MID_INPUTS = 600      # > 512 inputs: the real reference's commitment needs them (tests/golden/make_golden.py)
UNARY_MID_BUCKETS = [
    {**{(t, 0): 4 for t in BINARY}, (COPY, -1): 2},
    {(COPY, -1): 7, (NOT, -1): 6, (ADDC, -1): 7, (MULC, -1): 5},
    {**{(t, 2): 3 for t in BINARY}, (ADD, 1): 4, (MUL, 0): 5, (XOR, 1): 2, (NOT, -1): 2},
    {(MUL, 3): 4, (ADD, 2): 3, (SUB, 1): 2, (XOR, 0): 3, (ANTINAAB, 2): 2, (ADDC, -1): 1},
]
UNARY_MID_ASSERTS = {2: [(COPY, -1), (MULC, -1)]}


def make_unary_mid(seed):
    return make_bucketed(seed, UNARY_MID_INPUTS, UNARY_MID_BUCKETS, None, UNARY_MID_ASSERTS)


# Zero-variable layers: layer 1 is one gate (n_g = 0, n_u = 3), layer 2 is one gate above a layer of one wire (n_g = n_u = 0; its one-wire subset has bit length 0).
ZERO_VAR_INPUTS = 8
ZERO_VAR_BUCKETS = [{(MUL, 0): 1}, {(XOR, 0): 1}]


def make_zero_var(seed):
    return make_bucketed(seed, ZERO_VAR_INPUTS, ZERO_VAR_BUCKETS)


# Layers for the inner products <eq(r, .), values>: bit lengths 17, 17, 16, 15, 7, 2, 1, 0.  n >= 16 takes the whole-runs branch of the dot kernel (half table of
# 2^(n >> 1) >= 256 entries) and the sizes 2^16 + 3 and 2^16 - 5 leave the last run partial; both have more than 128 x 256 entries, so the 128 workgroups loop.
# Mostly Mulc / Addc with complex constants, so every layer above the inputs holds complex values.
DOT_INPUTS = (1 << 16) + 3
DOT_SIZES = [(1 << 16) + 3, (1 << 16) - 5, (1 << 15) - 7, 100, 3, 2, 1]


def _dot_buckets():
    out = []
    for i, n in enumerate(DOT_SIZES, start=1):
        nb = n // 8 if n >= 8 else (1 if n > 1 else 0)
        b = {(MULC, -1): (n - nb + 1) // 2, (ADDC, -1): (n - nb) // 2}
        if nb:
            b[(MUL, i - 1)] = nb - nb // 2
            if nb // 2:
                b[(ADD, 0)] = nb // 2
        out.append(b)
    return out


DOT_BUCKETS = _dot_buckets()


def make_dot_layers(seed):
    return make_bucketed(seed, DOT_INPUTS, DOT_BUCKETS)


def from_golden(entry):
    """The circuit of a custom case of tests/golden/golden.json (its "custom" entry: generator, seed, sizes)."""
    if entry.get("generator") == "make_skewed":
        return make_skewed(entry["seed"], entry["sizes"])
    if entry.get("generator") == "make_unary_mid":
        return make_unary_mid(entry["seed"])
    return make(entry["seed"], entry["sizes"])
