"""CPU: the references the device's verifier-side entry points are compared with (tests/test_gpu_verifier_sums.py) are checked here first.
  * custom_circuits.make_bucketed keeps its promises: the bucket histogram, the bit lengths and the unary-only layer, asserted from the arrays;
  * tests/verifier_sums.py (Python integers) equals the oracle's own loops (orc_predicates / orc_liu_gr / orc_layer_mle), element by element, on every
    circuit and point set of tests/verifier_sums_cases.py — the list the GPU file uses;
  * at corner points both equal a vector known without field arithmetic;
  * the circuit with a unary-only layer is proved by the oracle, accepted by the host verifier, and pinned to the real reference's transcript
    (tests/test_oracle_golden.py)."""
import numpy as np
import pytest

import custom_circuits as cc
import verifier_sums as vs
import verifier_sums_cases as cases
from test_skewed_circuits_host import _bl, _layers, _subsets

P = cc.P


def _histogram(L):
    h = {}
    for t, l in zip(L["ty"].tolist(), L["l"].tolist()):
        h[(t, l)] = h.get((t, l), 0) + 1
    return h


@pytest.mark.parametrize("name,inputs,buckets,v_wires,asserts", [
    ("ladder", cc.LADDER_INPUTS, cc.LADDER_BUCKETS, cc.LADDER_V_WIRES, cc.LADDER_ASSERTS),
    ("unary_mid", cc.UNARY_MID_INPUTS, cc.UNARY_MID_BUCKETS, {}, cc.UNARY_MID_ASSERTS),
    ("zero_var", cc.ZERO_VAR_INPUTS, cc.ZERO_VAR_BUCKETS, {}, {}),
    ("dot", cc.DOT_INPUTS, cc.DOT_BUCKETS, {}, {})])
def test_bucketed_generator_keeps_its_promises(name, inputs, buckets, v_wires, asserts):
    args = cases.arrays(name)
    sizes = [int(x) for x in args[0]]
    lay = _layers(args)
    assert sizes[0] == inputs and (lay[0]["ty"] == cc.INPUT).all() and len(sizes) == len(buckets) + 1
    for i in range(1, len(sizes)):
        L, want = lay[i], {k: n for k, n in buckets[i - 1].items() if n}
        assert _histogram(L) == want, "bucket histogram of layer %d" % i
        assert sizes[i] == sum(want.values())
        un = np.isin(L["ty"], cc.UNARY)
        assert (L["u"] < sizes[i - 1]).all() and (L["l"][un] == -1).all()
        sub = _subsets(L, i)
        for j in range(i):
            assert (L["v"][L["l"] == j] < sizes[j]).all()
            n_read = int((L["l"] == j).sum())
            assert len(sub[j]) == min(v_wires.get((i, j), sizes[j]), sizes[j], n_read), "subset (%d, %d)" % (i, j)
        flagged = sorted((int(L["ty"][g]), int(L["l"][g])) for g in np.flatnonzero(L["a"]))
        assert flagged == sorted(asserts.get(i, [])), "assert gates of layer %d" % i
        # scattered: no bucket of >= 63 gates sits in one run of consecutive gates
        for (t, l), n in want.items():
            if 63 <= n < sizes[i]:
                idx = np.flatnonzero((L["ty"] == t) & (L["l"] == l))
                assert idx[-1] - idx[0] >= n, "bucket %r of layer %d is not scattered" % ((t, l), i)
    # the assert gates evaluate to 0 (the oracle would refuse the circuit otherwise; here from the Python evaluation)
    w = cases.wiring(name)
    if asserts:
        vals = cases.values(name)
        for i in asserts:
            for g in np.flatnonzero(lay[i]["a"]):
                assert vals[i][int(g)] == (0, 0)
    assert [w.bl[i] for i in range(len(sizes))] == [_bl(s) for s in sizes]


def test_ladder_layer_shapes():
    """What tests/test_gpu_verifier_sums.py relies on: the ladder of bucket sizes, the empty buckets, odd and even bit lengths, a short subset."""
    w = cases.wiring("ladder")
    i = cc.LADDER_LAYER
    b = cc.LADDER_BUCKETS[i - 1]
    assert i >= 3 and sorted(set(b.values())) == [0, 1, 2, 3, 63, 64, 65, 511, 512, 513, 1024, 1025, cc.HUGE]
    assert cc.HUGE > 64 * 512
    assert b[(cc.ADDC, -1)] == 513 and cc.LADDER_BUCKETS[0][(cc.ADDC, -1)] == 65                 # Addc feeds coeff_l[Addc] and bias: two ladder sizes
    empty_then_filled = [t for t in cc.BINARY if any(b.get((t, l), 0) == 0 for l in range(i)) and any(b.get((t, l), 0) > 0 for l in range(i))]
    assert len(empty_then_filled) >= 2
    n_g, n_u, n_v = w.bl[i], w.bl[i - 1], w.max_dad_bl[i]
    assert (n_g, n_u, n_v) == (16, 9, 10) and {x % 2 for x in (n_g, n_u, n_v)} == {0, 1}
    assert w.dad_bl[i] == [10, 2, 7, 9] and min(w.dad_bl[i]) + 5 < n_v
    for k in (1, i):           # assert gates of each flag class: binary, unary, unary with a constant
        L = w.layers[k]
        kinds = {("binary" if L["ty"][g] in cc.BINARY else "const" if L["ty"][g] in (cc.MULC, cc.ADDC) else "unary") for g in range(w.size[k]) if L["a"][g]}
        assert kinds == {"binary", "unary", "const"}


def test_unary_only_and_zero_variable_layers():
    w = cases.wiring("unary_mid")
    i = cc.UNARY_MID_LAYER
    assert w.max_dad_bl[i] == -1 and w.n_v(i) == 0 and all(t in cc.UNARY for t in w.layers[i]["ty"])
    assert all(m >= 0 for k, m in enumerate(w.max_dad_bl) if k >= 1 and k != i)
    for k in (i + 1, i + 2):                                  # the layers above read it and the layers below it
        assert w.dad_size[k][i] > 0 and any(w.dad_size[k][j] > 0 for j in range(i))
    assert w.dad_size[i] == [0, 0]                            # the Liu sums of layers 1 and 2 meet an empty subset
    z = cases.wiring("zero_var")
    assert z.bl == [3, 0, 0] and z.max_dad_bl[1:] == [0, 0]
    d = cases.wiring("dot")
    assert d.bl == [17, 17, 16, 15, 7, 2, 1, 0]
    assert d.size[1] % (1 << 8) and d.size[2] % (1 << 8) and d.size[1] > 128 * 256 and d.size[2] > 128 * 256     # a partial last run; the 128 workgroups loop
    val = cases.values("dot")
    assert all(any(x[1] for x in val[k]) for k in range(1, 8)), "complex values in every gate layer"
    # the launch shapes the GPU file asserts: the 128-workgroup cap is reached by layers 0-3 and not by the small ones
    assert [cases.dot_launches(d.size[k], d.bl[k])[1][1] for k in range(8)] == [128, 128, 128, 128, 1, 1, 1, 1]
    assert [cases.dot_launches(d.size[k], d.bl[k])[0][1] for k in (0, 2, 3, 4, 7)] == [3, 2, 2, 1, 1]


@pytest.mark.parametrize("name", ["ladder", "unary_mid", "zero_var", "dot", "deep"])
def test_subset_numbering_is_the_oracles(name):
    """dadId rebuilt from the export's lv equals the oracle's own subset sizes and bit lengths."""
    w, oc = cases.wiring(name), cases.oracle_circuit(name)
    for i in range(1, w.n):
        ds, db, mx = oc.subsets(i)
        assert (w.dad_size[i], w.dad_bl[i], w.max_dad_bl[i]) == (ds, db, mx), i
        assert w.bl[i] == oc.layer_bitlen(i)


def test_eq_table_is_the_oracles_beta_table(ob):
    for n in (0, 1, 2, 5, 9):
        r = cases.uniform(np.random.default_rng(n), n) if n != 5 else cases.edgy(np.random.default_rng(5), 5)
        rr = np.array(r, dtype=np.uint64).reshape(-1, 2)
        one = np.array([1, 0], dtype=np.uint64)
        exp = np.zeros((1 << n, 2), np.uint64)
        ob.lib().orc_beta_table(rr.ctypes.data, n, one.ctypes.data, exp.ctypes.data)
        assert vs.eq_table(r) == [(int(a), int(b)) for a, b in exp]


@pytest.mark.parametrize("name,layer", cases.PREDICATE_LAYERS)
def test_predicates_reference_equals_oracle(name, layer):
    w, oc = cases.wiring(name), cases.oracle_circuit(name)
    ref = cases.predicate_reference(name, layer)
    for (label, rg, ar, ru, rv), mine in zip(cases.predicate_points(name, layer), ref):
        assert len(mine) == 5 + 7 * layer and all(0 <= x < P and 0 <= y < P for x, y in mine)
        assert oc.predicates(layer, rg, ar, ru, rv) == mine, label
        if label.startswith("corner gate"):
            assert mine == cases.corner_expectation(w, layer, int(label.split()[-1]), ar), label
    # buckets the circuit leaves empty are exactly zero at every point
    filled = cases.filled_slots(w, layer)
    for mine in ref:
        assert all(mine[k] == (0, 0) for k in range(5 + 7 * layer) if k not in filled)


def test_corner_points_cover_every_type_and_assert_class():
    w = cases.wiring("ladder")
    for layer in (1, cc.LADDER_LAYER):
        L = w.layers[layer]
        picked = cases.corner_gates(w, layer)
        assert {(L["ty"][g], L["a"][g]) for g in picked} == {(t, a) for t, a in zip(L["ty"], L["a"])}
        assert 0 in picked and w.size[layer] - 1 in picked
        assert {L["ty"][g] for g in picked} == set(cc.ALL_TYPES)


@pytest.mark.parametrize("name,layer", cases.LIU_LAYERS)
def test_liu_gr_reference_equals_oracle(name, layer):
    oc = cases.oracle_circuit(name)
    for (label, ru, rv, sig, rl), mine in zip(cases.liu_points(name, layer), cases.liu_reference(name, layer)):
        assert oc.liu_gr(layer, ru, [x or [] for x in rv], sig, rl) == mine, label


def test_liu_gr_corner_and_empty_subsets():
    """r_u = r_liu = the bits of one wire: the first sum is sig[0] exactly.  With all later sig zero nothing else is added, and a layer whose subset is empty adds
    nothing whatever its sig."""
    w = cases.wiring("unary_mid")
    layer, wire = 1, 17
    n, nb = w.n, w.bl[0]
    rng = np.random.default_rng(11)
    rv = [cases.uniform(rng, w.n_v(j)) if j >= layer else None for j in range(n)]
    s0 = cases.uniform(rng, 1)[0]
    sig = [s0] + [(0, 0)] * (n - layer)
    assert vs.liu_gr(w, layer, cases.bits(wire, nb), rv, sig, cases.bits(wire, nb)) == s0
    assert w.dad_size[2][0] == 0
    sig2 = list(sig); sig2[2 - layer + 1] = (12345, 678)       # layer 2's subset of layer 0 is empty
    assert vs.liu_gr(w, layer, cases.bits(wire, nb), rv, sig2, cases.bits(wire, nb)) == s0
    assert cases.oracle_circuit("unary_mid").liu_gr(layer, cases.bits(wire, nb), [x or [] for x in rv], sig2, cases.bits(wire, nb)) == s0


@pytest.mark.parametrize("name,layer", cases.MLE_LAYERS)
def test_layer_mle_reference_equals_oracle(name, layer):
    oc = cases.oracle_circuit(name)
    val = cases.values(name)[layer]
    for (label, r), mine in zip(cases.mle_points(name, layer), cases.mle_reference(name, layer)):
        assert oc.layer_mle(layer, r) == mine, label
        if label == "corner last":
            assert mine == val[-1]
        if label == "all zero":
            assert mine == val[0]


def test_unary_only_circuit_is_proved_and_verified(vp, ob):
    """A layer without binary gates has no phase 2: the oracle proves the circuit and its own verifier accepts; the host verifier of the product accepts
    the oracle's transcript (with its own predicate loops) and rejects it with the last claim flipped."""
    args = cases.arrays("unary_mid")
    oc = cases.oracle_circuit("unary_mid")
    tr, st = oc.prove_gkr()
    assert st["verified"] == 1
    c = vp.Circuit.custom(*args)
    assert c.hash() == oc.hash()
    assert c.verify_transcript(tr)
    bad = bytearray(tr); bad[-16] ^= 1
    assert not c.verify_transcript(bytes(bad))
    c.close()
