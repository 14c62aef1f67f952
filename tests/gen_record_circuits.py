"""A circuit whose contribution lists have every row shape the row records of the fused inits distinguish (csrc/vp_kernels_batch.h, GenP1R / GenLiuR /
GenP2R): the same seven arrays as custom_circuits.make().

    layer 0   1500 inputs (bit length 11)
    layer 1   1027 gates over layer 0: an odd length of two whole 512-entry fold chunks and a partial third
    layer 2   the shaped layer: its gates read layer 1 as u with P1_PATTERN fan-outs (rows with 0, 1, 2, VP_LIGHT_MAX and VP_LIGHT_MAX + 1 contributions;
              the last row, 1026, is even, so that its partner falls past the end), its binary gates read layer 1 as v with P2_PATTERN fan-outs (a subset of
              more than 512 wires that leaves wires out: Liu rows without a list) and 100 wires of layer 0 (a subset shorter than a fold chunk); every
              unary gate lands in slot 0 of the subset of layer 1 (a heavy slot); assert gates Sub(w, w) in a row of one, of two and of 17 contributions
    layer 3   700 gates over layer 2 with operands in layers 0, 1 and 2: Liu lists of two terms
shape() counts what the lists hold, so that a test can assert the shapes from the arrays."""
import numpy as np

from custom_circuits import ADD, ADDC, ALL_TYPES, BINARY, COPY, INPUT, MUL, MULC, NOT, P, SUB, UNARY

LIGHT_MAX = 16                                      # VP_LIGHT_MAX
SIZES0, SIZES1 = 1500, 1027
P1_PATTERN = (0, 1, 2, LIGHT_MAX, LIGHT_MAX + 1, 1, 3, 1)
P2_PATTERN = (1, 1, 2, 1, 1, 0, 1, LIGHT_MAX, 1, 1, 1, LIGHT_MAX + 1, 1, 1, 1, 1)
ASSERT_ROWS = (8, 9, 11)                            # P1_PATTERN 0, 1 and 16 -> rows of 1, 2 and 17 contributions


def make_rows(seed, real=True):
    """real: constants (c, 0), so that every circuit value is real (the inputs are); otherwise the Mulc / Addc constants are complex."""
    rng = np.random.default_rng(seed)

    def consts(tt):
        cc = np.zeros((len(tt), 2), np.uint64)
        isc = np.isin(tt, (MULC, ADDC))
        cc[isc, 0] = rng.integers(0, P, int(isc.sum()))
        if not real:
            cc[isc, 1] = rng.integers(0, P, int(isc.sum()))
        return cc

    def random_layer(n, below, i):
        tt = rng.choice(np.array(ALL_TYPES), n).astype(np.int32)
        un = np.isin(tt, UNARY)
        ll = np.where(un, -1, rng.integers(0, i, n)).astype(np.int32)
        uu = rng.integers(0, below[i - 1], n)
        vv = np.where(un, 0, rng.integers(0, np.array(below)[np.maximum(ll, 0)]))
        return tt, ll, uu, vv, consts(tt), np.zeros(n, np.uint8)

    sizes = [SIZES0, SIZES1]
    layers = [(np.full(SIZES0, INPUT, np.int32), np.full(SIZES0, -1, np.int32), rng.integers(0, P, SIZES0), np.zeros(SIZES0, np.int64),
               np.zeros((SIZES0, 2), np.uint64), np.zeros(SIZES0, np.uint8))]
    layers.append(random_layer(SIZES1, sizes, 1))
    # ---- layer 2 ----
    m = SIZES1
    u_cnt = np.array([P1_PATTERN[w % len(P1_PATTERN)] for w in range(m)])
    u_cnt[m - 1] = 2
    uu = rng.permutation(np.repeat(np.arange(m), u_cnt))
    v_cnt = np.array([P2_PATTERN[w % len(P2_PATTERN)] for w in range(m)])
    v1 = np.repeat(np.arange(m), v_cnt)
    v0 = np.arange(200, 300)
    n_bin, n = len(v1) + len(v0), len(uu)
    assert n_bin < n
    tt = np.concatenate([rng.choice(np.array(BINARY), n_bin), rng.choice(np.array(UNARY), n - n_bin)]).astype(np.int32)
    ll = np.concatenate([np.full(len(v1), 1), np.full(len(v0), 0), np.full(n - n_bin, -1)]).astype(np.int32)
    vv = np.concatenate([v1, v0, np.zeros(n - n_bin, np.int64)])
    aa = np.zeros(n, np.uint8)
    order = rng.permutation(n)
    tt, ll, vv = tt[order], ll[order], vv[order]
    # assert gates x - x = 0 on wires of layer 1
    na = len(ASSERT_ROWS)
    tt = np.append(tt, [SUB] * na).astype(np.int32); ll = np.append(ll, [1] * na).astype(np.int32)
    uu = np.append(uu, ASSERT_ROWS); vv = np.append(vv, ASSERT_ROWS); aa = np.append(aa, [1] * na).astype(np.uint8)
    layers.append((tt, ll, uu, vv, consts(tt), aa))
    sizes.append(len(tt))
    # ---- layer 3 ----
    sizes.append(700)
    layers.append(random_layer(700, sizes, 3))
    cat = lambda k, dt: np.concatenate([np.asarray(L[k]) for L in layers]).astype(dt)
    return (np.array(sizes, np.uint64), cat(0, np.int32), cat(1, np.int32), cat(2, np.uint64), cat(3, np.uint64),
            np.concatenate([L[4] for L in layers]).astype(np.uint64).reshape(-1, 2), cat(5, np.uint8))


def shape(args, layer=2):
    """Of gate layer `layer`: (set of phase-1 row lengths over the wires of the layer below, set of phase-2 slot lengths of its binary gates, number of
    unary gates, number of assert gates, set of operand layers)."""
    sizes, ty, l, u, v, c, a = args
    lo = int(sizes[:layer].sum()); hi = lo + int(sizes[layer])
    ty, l, u, v, a = ty[lo:hi], l[lo:hi], u[lo:hi].astype(np.int64), v[lo:hi].astype(np.int64), a[lo:hi]
    rows = set(np.bincount(u, minlength=int(sizes[layer - 1])).tolist())
    binary = l >= 0
    key = l[binary].astype(np.int64) * (1 << 32) + v[binary]
    slots = set(np.unique(key, return_counts=True)[1].tolist())
    return rows, slots, int((~binary).sum()), int(a.sum()), set(l[binary].tolist())
