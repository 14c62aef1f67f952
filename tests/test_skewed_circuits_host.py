"""CPU: custom_circuits.make_skewed promises the shapes that send every gate type through the fused inits, the chunk kernels and the row-range jobs of a
sharded proof (tests/test_gpu_gate_paths.py).  Everything it promises is asserted here from the seven arrays alone, and the oracle proves and verifies
each circuit."""
import numpy as np
import pytest

import custom_circuits as cc

BOUNDARY = (1, 16, 17, 511, 512, 513, 1024, 1025)
NAMES = {cc.MUL: "mul", cc.ADD: "add", cc.SUB: "sub", cc.ANTISUB: "antisub", cc.NAAB: "naab", cc.ANTINAAB: "antinaab", cc.MULC: "mulc", cc.ADDC: "addc",
         cc.XOR: "xor", cc.NOT: "not", cc.COPY: "copy"}


def _bl(n):
    return int(n - 1).bit_length() if n > 1 else 0


def _layers(args):
    sizes, ty, l, u, v, c, a = args
    off = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    return [dict(ty=ty[off[i]:off[i + 1]], l=l[off[i]:off[i + 1]], u=u[off[i]:off[i + 1]].astype(np.int64), v=v[off[i]:off[i + 1]].astype(np.int64),
                 c=c[off[i]:off[i + 1]], a=a[off[i]:off[i + 1]]) for i in range(len(sizes))]


def _subsets(L, i):
    """dadId of layer i as layeredCircuit::subsetInit builds it: per source layer, the wires in the order of their first use walking the gates backwards."""
    out = {}
    for j in range(i):
        vs = L["v"][L["l"] == j][::-1]
        uniq, first = np.unique(vs, return_index=True)
        out[j] = uniq[np.argsort(first)]
    return out


def _check(args, only_type=None):
    sizes = [int(s) for s in args[0]]
    lay = _layers(args)
    n_layers = len(sizes)
    assert (lay[0]["ty"] == cc.INPUT).all() and sizes[0] > 512
    p1_layers = [i for i in range(1, n_layers) if _bl(sizes[i - 1]) == 14]
    assert len(p1_layers) >= (3 if only_type is not None else 4)
    assert sum(sizes[i - 1] % 2 for i in p1_layers) >= 2, "two odd-sized tables of bit length 14"
    subsets = {i: _subsets(lay[i], i) for i in range(1, n_layers)}
    four_kinds = long_subsets = huge1 = huge2 = 0
    for i in range(1, n_layers):
        L, n, m = lay[i], sizes[i], sizes[i - 1]
        un = np.isin(L["ty"], cc.UNARY)
        assert (L["l"][un] == -1).all() and (L["l"][~un] >= 0).all() and (L["l"] < i).all() and (L["u"] < m).all()
        for j in range(i):
            assert (L["v"][L["l"] == j] < sizes[j]).all()
        asserts = np.flatnonzero(L["a"])
        assert len(asserts) == (1 if only_type is not None else 2) and L["a"][n - 1] == 1
        for g in asserts:      # value 0 whatever the witness: x - x
            assert L["ty"][g] in (cc.SUB, cc.ANTISUB) and L["l"][g] == i - 1 and L["u"][g] == L["v"][g]
        if only_type is not None:
            assert (np.delete(L["ty"], asserts) == only_type).all()
        else:
            assert (L["c"][np.isin(L["ty"], (cc.MULC, cc.ADDC))] != 0).any(axis=0).tolist() == [True, True], "complex constants"
        # ---- phase 1: gates per u
        f1 = np.bincount(L["u"], minlength=m)
        pins = cc.skewed_p1_pins(n, m)
        for row, k in pins.items():
            assert f1[row] == k, (i, row)
        assert set((0,) + BOUNDARY) <= set(f1.tolist())
        H = cc.HEAVY
        assert f1[0] > H and f1[1] > H                                        # heavy / heavy pair
        assert f1[6] > H and 0 < f1[7] <= H and f1[9] > H and 0 < f1[8] <= H  # heavy even / odd row, light partner
        assert f1[4] > H and f1[5] == 0 and f1[10] > H and f1[11] == 0        # beside an empty row
        assert f1[m - 1] > H                                                  # last valid row (no partner when m is odd)
        if _bl(m) >= 14:
            assert f1[8191] > H and f1[8192] > H                              # both sides of the slice edge of a split over two ranks
        if f1.max() > 64 * 512:
            huge1 += 1
            assert f1[2] == f1.max() and 0 < f1[3] <= H
        for row in np.flatnonzero(f1 >= 512):
            kinds = set(L["ty"][L["u"] == row].tolist())
            assert kinds >= (set(cc.ALL_TYPES) if only_type is None else {only_type}), (i, row)
        assert all(f1[L["u"][g]] > H for g in asserts), "an assert gate inside a heavy phase-1 row"
        # ---- phase 2: gates per (l, v) slot; the unary gates all land on slot 0 of subset i-1 (src/prover.cpp:314)
        sub = subsets[i]
        slot_counts = []
        for j in range(i):
            ids = sub[j]
            if not len(ids):
                continue
            cnt = np.bincount(L["v"][L["l"] == j], minlength=sizes[j])[ids]
            if j == i - 1:
                cnt = cnt.copy(); cnt[0] += int(un.sum())
            slot_counts.append((j, ids, cnt))
        top = [s for s in slot_counts if s[0] == i - 1][0]
        assert top[1][0] == 0 and top[2][0] > H and all(L["v"][g] in (0, 1) for g in asserts), "an assert gate inside a heavy phase-2 slot"
        if only_type is None or only_type in cc.BINARY:
            ids, cnt = top[1], top[2]
            assert (ids == np.arange(len(ids))).all(), "wire w of layer i-1 is slot w"
            for w, k in cc.skewed_p2_pins(len(asserts)).items():
                assert cnt[w] == k, (i, w)
            assert set(BOUNDARY) <= set(cnt.tolist())
            assert cnt[0] > H and cnt[1] > H and cnt[6] > H and cnt[7] > H and 0 < cnt[5] <= H and 0 < cnt[4] <= H
            for j, ids_j, cnt_j in slot_counts:
                for w in ids_j[cnt_j >= 512]:
                    kinds = set(L["ty"][(L["l"] == j) & (L["v"] == w)].tolist())
                    if j == i - 1 and w == 0:
                        kinds |= set(L["ty"][un].tolist())
                        assert kinds >= (set(cc.ALL_TYPES) if only_type is None else {only_type})
                    else:
                        assert kinds >= (set(cc.BINARY) if only_type is None else {only_type}), (i, j, w)
                if j != i - 1:
                    by_wire = cnt_j[np.argsort(ids_j)]
                    assert by_wire[0] == dict((w0, k0) for w0, _, k0 in cc.P2_MIDS.values())[ids_j.min()] > H and (by_wire[1:] == 1).all()      # mid subsets: the lowest wire heavy, single gates on the others (their slots follow the gate order)
            if top[2].max() > 64 * 512:
                huge2 += 1
            tl = {j: (1 << _bl(len(ids_j))) for j, ids_j, _ in slot_counts}
            long_subsets += len(top[1]) > 8192 and any(512 <= t <= 2048 for t in tl.values())
            if (len(top[1]) > 8192 and any(512 <= t <= 2048 for t in tl.values()) and any(t < 512 for t in tl.values()) and any(j not in tl for j in range(i))):
                four_kinds += 1
        else:
            assert len(slot_counts) == 1 and len(top[1]) == 1 and top[2][0] == n      # unary types: one slot takes the whole layer
    # ---- Liu rows: the later layers' subsets that hold a wire of layer i-1
    if only_type is None or only_type in cc.BINARY:
        assert long_subsets >= 1 and (only_type is not None or four_kinds >= 1)      # the single-type circuits have too few layers for all four kinds at once
        seen = set()
        for j in range(n_layers - 1):
            k = np.zeros(sizes[j], np.int64)
            for i in range(j + 1, n_layers):
                k[subsets[i][j]] += 1
            seen |= set(k.tolist())
            assert k.min() == 0 and k.max() >= 1
        assert seen >= {0, 1, 2, 3} and (only_type is not None or 4 in seen)
    if only_type is None:
        assert huge1 == 1 and huge2 == 1
        assert max(sizes) < 50000 and sum(sizes) <= 130000


def _oracle_accepts(ob, args):
    oc = ob.Circuit.custom(*args)
    tr, st = oc.prove_gkr()
    oc.close()
    assert st["verified"] == 1 and len(tr) > 0


@pytest.mark.parametrize("seed,real", [(103, False), (104, True)])
def test_skewed_circuit_has_the_promised_shape_and_the_oracle_proves_it(ob, seed, real):
    args = cc.make_skewed(seed, real_consts=real)
    if not real:
        _check(args)
    else:
        assert not args[5][:, 1].any()
        lay = _layers(args)
        assert all(set(np.bincount(L["u"]).tolist()) >= set(BOUNDARY) for L in lay[1:])
    _oracle_accepts(ob, args)


@pytest.mark.parametrize("t", sorted(NAMES), ids=lambda t: NAMES[t])
def test_single_type_circuit_has_the_promised_shape_and_the_oracle_proves_it(ob, t):
    args = cc.make_skewed(200 + t, only_type=t)
    _check(args, only_type=t)
    _oracle_accepts(ob, args)


def test_make_is_untouched_by_the_second_generator():
    """make()'s circuits for the existing seeds are pinned by golden files and circuit hashes: the digest of one of them, taken before make_skewed existed."""
    import hashlib
    h = hashlib.sha256()
    for x in cc.make(102, [1500, 2100, 900, 4100, 700]):
        h.update(np.ascontiguousarray(x).tobytes())
    assert h.hexdigest() == MAKE_102_DIGEST


MAKE_102_DIGEST = "9b234a60b1a4199dbd6937570e15168072e6895e1fd777e64b7ecf1a1049a78c"
