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


def from_golden(entry):
    """The circuit of a custom case of tests/golden/golden.json (its "custom" entry: generator, seed, sizes)."""
    if entry.get("generator") == "make_skewed":
        return make_skewed(entry["seed"], entry["sizes"])
    return make(entry["seed"], entry["sizes"])
