"""CPU: tests/upload_desc.py keeps its promises before tests/test_gpu_circuit_upload.py relies on them.
  * build() follows the reference's subset rule: lv, dadSize, dadBitLength and the wire behind every subset slot equal the oracle's own export after subsetInit;
  * validate() accepts every unmutated description and refuses every row of CASES with the code and text the row is named for;
  * every row changes the description where its name says, and nowhere else (a diff of the arrays)."""
import numpy as np
import pytest

import custom_circuits as cc
import upload_desc as ud


def _circuits():
    return {
        "base": ud.base_arrays(),
        "wide": ud.wide_arrays(),
        "no_const": ud.no_const_arrays(),
        "bucketed_unary_mid": cc.make_unary_mid(104),      # an empty subset and a layer of unary gates only
        "zero_var": cc.make_zero_var(21),
    }


@pytest.mark.parametrize("name", ["base", "wide", "no_const", "bucketed_unary_mid", "zero_var", "randomize"])
def test_build_equals_the_oracles_export(ob, name):
    if name == "randomize":
        oc = ob.Circuit.randomize(3, 6, seed=5)
        n = oc.layers
        ex = [oc.export_layer(i) for i in range(n)]
        sizes = [oc.layer_size(i) for i in range(n)]
        cat = lambda k, dt: np.concatenate([e[k] for e in ex]).astype(dt)
        total = sum(sizes)
        a = (np.array(sizes, np.uint64), cat("ty", np.int32), cat("l", np.int32), cat("u", np.uint64), cat("v", np.uint64), np.zeros((total, 2), np.uint64),
             np.zeros(total, np.uint8))
    else:
        a = _circuits()[name]
        oc = ob.Circuit.custom(*a)
    desc = ud.build(*a)
    assert len(desc) == oc.layers
    saw_empty = saw_unary_only = False
    for i in range(oc.layers):
        assert desc[i]["size"] == oc.layer_size(i) and desc[i]["bit_length"] == oc.layer_bitlen(i)
        if i == 0:
            continue
        e, d = oc.export_layer(i), desc[i]
        ds, db, mx = oc.subsets(i)
        binary = np.isin(e["ty"], cc.BINARY)
        assert np.array_equal(d["ty"], e["ty"]) and np.array_equal(d["u"], e["u"])
        assert np.array_equal(d["l"][binary], e["l"][binary]) and (d["l"][~binary] == -1).all()
        assert np.array_equal(d["v"][binary], e["v"][binary]) and np.array_equal(d["lv"][binary], e["lv"][binary])
        assert [int(x) for x in d["dad_size"]] == ds
        for j in range(i):
            if ds[j]:
                assert int(d["dad_bitlen"][j]) == db[j]
                m = binary & (e["l"] == j)
                # dadId of the reference, slot by slot: the wire every gate's lv points at
                assert np.array_equal(d["dad_id"][j][e["lv"][m].astype(np.int64)], e["v"][m].astype(np.uint32))
                assert len(np.unique(d["dad_id"][j])) == ds[j] == int(e["lv"][m].max()) + 1
            else:
                saw_empty = True
        assert mx == max([db[j] for j in range(i) if ds[j]], default=-1)
        saw_unary_only = saw_unary_only or not binary.any()
        assert (d["c"] is None) == (not np.isin(e["ty"], (cc.MULC, cc.ADDC)).any())
    if name == "bucketed_unary_mid":
        assert saw_empty and saw_unary_only
    assert ud.validate(desc) == (ud.VP_OK, None)
    oc.close()


@pytest.fixture(scope="module")
def bases():
    return {k: ud.build(*f()) for k, f in ud.BASES.items()}


def test_base_circuit_has_what_the_table_needs(bases):
    d = bases["base"]
    assert [x["size"] for x in d] == ud.BASE_SIZES and all((1 << x["bit_length"]) > x["size"] for x in d if x["size"] != 64)      # a padded region in every layer the rows point into
    types = set(int(t) for x in d[1:] for t in x["ty"])
    assert types == set(cc.ALL_TYPES)
    assert all(x["is_assert"] is not None and x["is_assert"].sum() == 1 for x in d[1:])
    i, j = ud.empty_subset(d)
    assert i == len(d) - 1
    assert set(int(t) for t in d[3]["ty"]) >= set(ud.UNARY) and int(d[3]["dad_size"][1]) >= 3
    assert len(bases["wide"][1]["dad_id"][0]) == 300
    assert all(x["c"] is None and x["is_assert"] is None for x in bases["no_const"][1:])
    for b in bases.values():
        assert ud.validate(b) == (ud.VP_OK, None)


def test_case_names_are_unique_and_every_check_has_a_row():
    names = [c.name for c in ud.CASES]
    assert len(set(names)) == len(names)
    texts = {c.want[1] for c in ud.CASES}
    assert texts >= {"bad gate type", "gate.u out of range", "unary gate with l != -1", "gate.v out of range", "gate.lv inconsistent with dadId", "dadId out of range",
                     "dadSize too large", "dadBitLength mismatch", "bad layer size", "layer arrays missing", "Addc/Mulc gates without constants", "too many layers"}
    assert set(ud.GROUPS) == {"arguments", "layer size", "type", "u", "unary l", "v / l", "lv", "dadId", "subsets", "constants", "placement", "precedence"}


@pytest.mark.parametrize("case", ud.CASES, ids=lambda c: c.name)
def test_validate_refuses_each_row_for_its_reason(bases, case):
    base = bases[case.base]
    snapshot = ud.build(*ud.BASES[case.base]())
    d = case.mutate(base)
    assert ud.differences(base, snapshot) == [], "the mutation wrote into the shared description"
    got = ud.validate(None if case.null_desc else d, case.n_layers)
    assert got == case.want, "%s: validate says %r" % (case.name, got)


# where each row may differ from its base: (layer, field) pairs; layer -1 is the last layer
_TOUCHES = {
    "size_0": {(2, "size")}, "size_2p30_plus_1": {(-1, "size"), (-1, "bit_length")}, "bit_length_above_layer_0": {(0, "bit_length")},
    "lv_swapped": {(2, "lv")}, "lv_eq_dad_size": {(3, "lv")}, "lv_u32_max": {(3, "lv")}, "lv_into_empty_subset": {(-1, "l"), (-1, "v"), (-1, "lv")},
    "dad_id_eq_size": {(3, "dad_id[1]")}, "dad_size_above_layer": {(3, "dad_size"), (3, "dad_bitlen"), (3, "dad_id[1]")},
    "dad_bitlen_above": {(3, "dad_bitlen")}, "dad_bitlen_below": {(3, "dad_bitlen")}, "empty_subset_bitlen_int_min_ok": {(-1, "dad_bitlen")},
    "c_null_one_addc": {(3, "ty"), (3, "c")}, "c_null_one_mulc": {(3, "ty"), (3, "c")},
    "lower_gate_wins_u_before_v": {(2, "u"), (2, "v")}, "lower_gate_wins_v_before_u": {(2, "u"), (2, "v")}, "one_gate_u_before_v": {(2, "u"), (2, "v")},
    "lower_layer_wins": {(1, "ty"), (3, "u")}, "v_eq_size": {(3, "v")}, "v_in_padding": {(3, "v")},
    "desc_null": set(), "one_layer": set(), "c_and_assert_null_unused_ok": set(),
}


def _touches(case, n):
    if case.name in _TOUCHES:
        return {(i if i >= 0 else n - 1, k) for i, k in _TOUCHES[case.name]}
    nm = case.name
    if nm.startswith("null_"):
        k = nm[len("null_"):nm.index("_layer_")]
        return {(1 if nm.endswith("_1") else n - 1, k)}
    if nm.startswith("bit_length_"):
        return {(1, "bit_length")}
    if nm.startswith("type_"):
        return {(2, "ty")}
    if nm.startswith("u_"):
        return {(2, "u")}
    if nm.startswith("unary_") or nm.startswith("binary_l_"):
        return {(3, "l")}
    if nm.startswith("dad_id_bad_"):
        return {(1, "dad_id[0]")}
    if nm.startswith("bad_u_layer_"):
        return {(1 if "_layer_1_" in nm else n - 1, "u")}
    if nm == "dad_id_before_the_gate_it_breaks":
        return None                                 # one entry of one subset of layer 3, whichever the first binary gate points at
    raise KeyError(nm)


@pytest.mark.parametrize("case", ud.CASES, ids=lambda c: c.name)
def test_each_row_changes_the_place_it_names(bases, case):
    base = bases[case.base]
    d = case.mutate(base)
    diff = ud.differences(base, d)
    if case.name == "layers_65":
        assert diff == [(i, "layer") for i in range(len(base), 65)]
        return
    want = _touches(case, len(base))
    if want is None:
        assert len(diff) == 1 and diff[0][0] == 3 and diff[0][1].startswith("dad_id[")
    else:
        assert set(diff) == want, "%s changed %r" % (case.name, diff)
    # one element per changed array, where the row is about one element (the type rewrites of the constants rows and the new list of dad_size_above_layer aside)
    if case.group in ("type", "u", "unary l", "v / l", "dadId", "placement") or case.name in ("lv_eq_dad_size", "lv_u32_max"):
        for i, k in diff:
            a, b = (base[i]["dad_id"][int(k[7:-1])], d[i]["dad_id"][int(k[7:-1])]) if k.startswith("dad_id[") else (base[i][k], d[i][k])
            assert int((np.asarray(a) != np.asarray(b)).sum()) == 1
