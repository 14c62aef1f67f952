"""CPU: the GKR verifier's checks held to a cheating prover (tests/gkr_forge.py).  A changed element under an otherwise honest transcript shows that SOME check reads
it; these transcripts are repaired behind the lie, so that exactly one check stands between each of them and acceptance, and the test knows which.

For every row of tests/gkr_forged_cases.py three answers must agree: the check the forger declares it left standing; the first failed check of the verifier written
from the protocol in Python integers (tests/gkr_verifier_ref.py); the host verifier's verdict and the check it names (vph_last_gkr_failure).  A rejection at any other
check — earlier or later — fails the row, and so does an acceptance.

  table        every (circuit, family, plan) on a tape given up front, through Circuit.verify_transcript_tape; the honest transcript accepted, nothing recorded
  skip         with skip_predicates the closing values are not computed: the "honest claims" forgeries are accepted by design, every other row keeps its verdict
  dead end     on uv_corners the forger cannot pass the first layer whose challenges are corners
  Fiat-Shamir  on the chain (Circuit.verify_fs): the challenges move with the forger's messages, and the bytes behind the repaired stretch are the honest proof's
  joined       tests/golden/full_fs_rand3_7.bin with its GKR section forged: rejected at the hand-over of the claim, and — with the true last vr — inside the GKR part
  record       tests/golden/full_record_custom_a.bin with its GKR section forged on the record's own challenges: rejected at claim != input_0

Corners in which a forged transcript is honest in value, so that the definition, the host and the device must all ACCEPT it (the row's declared check is None):
a pair change a + 1, b - 1 moves p(r) by r^2 - r, which is zero at a challenge of 0 or 1 (sprinkle and edge_limbs_complex have them); a solved claim is weighed into
the Liu sumcheck of the layer it is about by one sig element, which sprinkle and sig_first_only set to zero in places."""
import os
import re
import subprocess

import pytest

import full_fs_ref as ff
import gkr_fs_cases as gfc
import gkr_forge as gf
import gkr_forged_cases as fc
import gkr_tape_cases as gc
import gkr_verifier_ref as gv
import verifier_sums as vs
from conftest import GOLDEN, ROOT

# plans per circuit, from its shape (gkr_forged_cases.plans): pair changes + the eleven (ten without a far subset, fewer where top, middle and bottom coincide) lies
N_PLANS = {"S": 38, "tiny": 23, "zero_var": 15, "unary_mid": 35, "edge_small": 38}


@pytest.fixture(scope="module")
def host_circuits(vp):
    made = {}

    def get(name):
        if name not in made:
            made[name] = gc.build(vp, name)
            assert made[name].hash() == gc.oracle_circuit(name).hash()
        return made[name]
    yield get
    for c in made.values():
        c.close()


def test_plans_cover_what_the_table_promises():
    for name in gc.SMALL_CIRCUITS:
        off, pl = gc.offsets(name), fc.plans(name)
        assert len(pl) == N_PLANS[name] and len({label for label, _ in pl}) == len(pl), name
        pairs = [p["pair"] for _, p in pl if "pair" in p]
        for i in fc.layers_of(off):
            for kind, k in (("phase1", off.bl[i - 1]), ("phase2", max(0, off.mdb[i])), ("liu", off.bl[i - 1])):
                assert [j for kk, ii, j in pairs if (kk, ii) == (kind, i)] == fc.three(k)
        hows = [(p["stop"][1], p["stop"][0]) for _, p in pl if "stop" in p]
        assert {h for h, _ in hows} == {"claims", "solved", "liu_vr", "vr_div", "true_vr"} and ("vr_div", 1) in hows and ("true_vr", 1) in hows
    # far subsets on S: the top layer reads layers 0 and 1 as well as layer 2
    assert gf.subsets(fc.wiring("S"), 3, "far") == [0, 1] and any(p.get("k") == "far" for _, p in fc.plans("S"))
    assert gc.offsets("unary_mid").mdb[2] == -1 and gc.offsets("zero_var").bl[1:] == [0, 0]
    # the next check from every place a lie can end
    off = gc.offsets("unary_mid")
    assert gf.next_check(off, ("phase1", 2, 4)) == ("semi_final", 2, -1) and gf.next_check(off, ("liu_semi_final", 1, -1)) == ("input", 0, -1)
    off = gc.offsets("zero_var")
    assert gv.checks(off) == [("semi_final", 2, -1), ("liu_semi_final", 2, -1)] + [("phase1", 1, j) for j in range(3)] + [("semi_final", 1, -1)] + \
        [("liu", 1, j) for j in range(3)] + [("liu_semi_final", 1, -1), ("input", 0, -1)]


@pytest.mark.parametrize("name", gc.SMALL_CIRCUITS)
def test_every_forgery_is_rejected_at_its_declared_check(vp, host_circuits, name):
    c, off = host_circuits(name), gc.offsets(name)
    accepted = []
    for fam in fc.FAMILIES:
        tape, tr = gc.tape(name, fam), gc.oracle(name, fam)[0]
        assert fc.reference(name, fam, tr) is None, fam
        assert c.verify_transcript_tape(tape, tr) and vp.last_gkr_failure() is None, fam
        rows = fc.rows(name, fam)
        dead = [(label, str(d)) for label, _, bad, d in rows if bad is None]
        assert not dead and len(rows) == N_PLANS[name], "%s / %s: %d rows, the forger stopped at %r" % (name, fam, len(rows), dead)
        seen = set()
        for label, plan, bad, declared in rows:
            what = "%s / %s / %s" % (name, fam, label)
            assert bad != tr and len(bad) == len(tr) and bad not in seen, what
            seen.add(bad)
            assert fc.reference(name, fam, bad) == declared, what + ": the definition"
            assert c.verify_transcript_tape(tape, bad) == (declared is None), what + ": the host's verdict"
            assert vp.last_gkr_failure() == declared, what + ": the check the host names"
            if declared is None:
                accepted.append((fam, label))
            # without the closing values: honest claims under re-made rounds pass (by design); everything else keeps its verdict, unless that was a closing value
            skipped = fc.reference(name, fam, bad, skip_predicates=True)
            assert c.verify_transcript_tape(tape, bad, skip_predicates=True) == (skipped is None) and vp.last_gkr_failure() == skipped, what + ": skip_predicates"
            if "stop" in plan and plan["stop"][1] == "claims":
                assert declared == ("semi_final", plan["stop"][0], -1) and skipped is None, what
            elif declared is not None and declared[0] != "semi_final":
                assert skipped == declared, what
        assert c.verify_transcript_tape(tape, tr) and vp.last_gkr_failure() is None, fam + ": a failure recorded before stays behind an accepted replay"
    print(name, "accepted as honest in value:", accepted)
    # honest in value: only the two corners of the module's text, and few of them
    assert all(("pair change" in label and fam in ("sprinkle", "edge_limbs_complex")) or ("claim solved" in label and fam in ("sprinkle", "sig_first_only"))
               for fam, label in accepted) and len(accepted) <= 6


@pytest.mark.parametrize("name", ["M", "R"])
def test_rows_of_the_larger_gpu_circuits(vp, host_circuits, name):
    """the rows tests/test_gpu_gkr_forged.py sends through the device loops on M and R: definition, declared check and host agree here first"""
    c, off = host_circuits(name), gc.offsets(name)
    for fam in fc.GPU_TABLE[name]:
        tape, tr = gc.tape(name, fam), gc.oracle(name, fam)[0]
        assert fc.reference(name, fam, tr) is None and c.verify_transcript_tape(tape, tr) and vp.last_gkr_failure() is None, fam
        rows = fc.rows(name, fam)
        assert len(rows) == 38 and all(bad is not None for _, _, bad, _ in rows), (name, fam)
        for label, plan, bad, declared in rows:
            what = "%s / %s / %s" % (name, fam, label)
            assert fc.reference(name, fam, bad) == declared, what + ": the definition"
            assert c.verify_transcript_tape(tape, bad) == (declared is None) and vp.last_gkr_failure() == declared, what + ": the host"
        assert sum(declared is None for _, _, _, declared in rows) <= 3, (name, fam)
    assert all(set(fc.GPU_TABLE[k]) <= set(fc.FAMILIES) for k in fc.GPU_TABLE) and set(fc.GPU_TABLE) - set(gc.SMALL_CIRCUITS) == {"M", "R"}


def test_declared_checks_are_all_kinds_at_all_places():
    """what the table reaches: every kind of check, first, middle and last rounds, top, middle and bottom layers, zero-round Liu sumchecks, far claims"""
    declared = {}
    for name in gc.SMALL_CIRCUITS:
        declared[name] = {d for fam in fc.FAMILIES for _, _, _, d in fc.rows(name, fam) if d is not None}
    every = set().union(*declared.values())
    assert {d[0] for d in every} == set(gv.KINDS)
    s = declared["S"]                                                  # layers 3, 2, 1; six rounds over layers 2, 1, 0
    assert {("liu", 3, 0), ("liu", 2, 0), ("liu", 1, 0)} <= s, "near and far claims: the Liu sumchecks about layers 2, 1 and 0"
    assert {("phase2", i, 0) for i in (3, 2, 1)} <= s and {("semi_final", i, -1) for i in (3, 2, 1)} <= s and {("liu_semi_final", i, -1) for i in (3, 2, 1)} <= s
    assert ("phase1", 2, 0) in s and ("phase1", 1, 0) in s and ("input", 0, -1) in s
    assert ("liu_semi_final", 2, -1) in declared["zero_var"] and ("semi_final", 2, -1) in declared["zero_var"]
    u = declared["unary_mid"]                                           # layer 2 has no phase 2: phase 1's last round hands over to the closing value
    assert ("semi_final", 2, -1) in u and not any(d[:2] == ("phase2", 2) for d in u)


def test_the_corner_tape_is_a_dead_end(vp, host_circuits):
    """uv_corners: r_u and r_v are 0 / 1 patterns, the closing value's slope in every claim is zero, the lie cannot leave the first layer that has such challenges
    (the top layer; on zero_var layer 2 has no round and no challenge of its own, so layer 1).  What is left to the forger there is rejected by that layer's closing value."""
    for name in gc.SMALL_CIRCUITS:
        off, c = gc.offsets(name), host_circuits(name)
        first = max(i for i in range(1, off.n_layers) if off.bl[i - 1] + max(0, off.mdb[i]) > 0)
        assert first == (off.n_layers - 1 if name != "zero_var" else 1)
        rows = fc.rows(name, fc.DEAD_END)
        stuck = [d for _, plan, bad, d in rows if bad is None]
        assert stuck and all(d.layer == first for d in stuck), name
        carried = [label for label, plan, bad, _ in rows if bad is None]
        assert "everything re-made" in carried and "everything re-made, true last vr" in carried
        tape = gc.tape(name, fc.DEAD_END)
        for label, plan, bad, declared in rows:
            if bad is not None:
                assert fc.reference(name, fc.DEAD_END, bad) == declared and c.verify_transcript_tape(tape, bad) == (declared is None) and vp.last_gkr_failure() == declared, label
        if first == off.n_layers - 1:
            label, plan, bad, declared = [r for r in rows if r[0] == "false Vres, honest claims"][0]
            assert declared == ("semi_final", first, -1) and bad is not None


# ---- the Fiat-Shamir form -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.FS_CIRCUITS)
def test_forgeries_on_the_chain(vp, host_circuits, name):
    c, oc, off, w, a = host_circuits(name), gc.oracle_circuit(name), gc.offsets(name), fc.wiring(name), gc.arrays(name)
    state = gfc.statement_state(oc, True, consts=a[5], asserts=a[6])
    proof = fc.honest_fs(oc, off, state)
    assert gv.verify(w, off, gv.Chained(off, state), proof) is None
    assert c.verify_fs(proof) and vp.last_gkr_failure() is None
    plans = fc.plans(name, fs=True)
    labels = [label for label, _ in plans]
    assert sum("pair change" in x for x in labels) == 3 and "near claim solved at the top layer" in labels and "everything re-made" in labels
    assert ("far claim solved at the top layer" in labels) == (name != "zero_var") and "everything re-made, true last vr" in labels
    for label, plan, bad, declared, _, tape in fc.rows_fs(w, off, state, proof, plans):
        what = "%s / %s" % (name, label)
        assert declared is not None and bad != proof
        assert gv.verify(w, off, gv.Chained(off, state), bad) == declared, what + ": the definition"
        assert not c.verify_fs(bad) and vp.last_gkr_failure() == declared, what + ": the host"
        assert c.gkr_fs_tape(bad, state)[0].tobytes() == tape.tobytes(), what + ": the forger's challenges are the chain's"
    assert c.verify_fs(proof) and vp.last_gkr_failure() is None


# ---- the joined proof and the record --------------------------------------------------------------------------------------------------------------------------------
def test_joined_proof_with_a_forged_gkr_section(vp, ob):
    _, layers, log_size, seed, _ = ff.FIXTURE
    proof = ff.fixture()
    oc = ob.Circuit.randomize(layers, log_size, seed=seed)
    c = vp.Circuit.randomize(layers, log_size, seed=seed)
    try:
        w, off, s = vs.wiring_from(oc), gc.Offsets.of(oc), ff.sections(proof)
        n = off.bl[0]
        state, gkr = gfc.full_fs_head_state(oc, proof)
        ok, why, point = c.verify_full_fs(proof, return_point=True)
        assert ok and vp.last_gkr_failure() is None
        assert gv.verify(w, off, gv.Chained(off, state), gkr, input_check=False) is None
        (remade, d0, tape0), (true_vr, d1, tape1) = fc.joined_forgeries(w, off, state, gkr)
        # every check of the GKR part holds: only the hand-over of the claim to the commitment is left, and the point has moved with the lie
        end = {}
        assert gv.verify(w, off, gv.Chained(off, state), remade, input_check=False, state=end) is None and gv.verify(w, off, gv.Chained(off, state), remade) == d0
        ok, why, moved = c.verify_full_fs(proof[:s["gkr"]] + remade + proof[s["root_h"]:], return_point=True)
        assert not ok and "final input check" in why and vp.last_gkr_failure() == d0
        at = off.rl[1][0]
        assert moved.tobytes() == tape0[at:at + n].tobytes() != point.tobytes() and [tuple(int(x) for x in r) for r in moved] == end["point"]
        # the true value of the input layer at the moved point: now the Liu sumcheck's own closing test is all that stands
        assert gv.elements(true_vr)[-1] == vs.layer_mle(w.inputs, [tuple(int(x) for x in r) for r in tape1[at:at + n]])
        assert gv.verify(w, off, gv.Chained(off, state), true_vr, input_check=False) == d1
        ok, why = c.verify_full_fs(proof[:s["gkr"]] + true_vr + proof[s["root_h"]:])
        assert not ok and "GKR" in why and "liu_semi_final, layer 1, round -1" in why and vp.last_gkr_failure() == d1
        assert c.verify_full_fs(proof)[0] and vp.last_gkr_failure() is None
    finally:
        c.close()


def test_record_with_a_forged_gkr_section(vp, golden):
    import custom_circuits as cc
    g = golden["custom_a"]
    args = cc.make(g["custom"]["seed"], g["custom"]["sizes"])
    rec = open(os.path.join(GOLDEN, "full_record_custom_a.bin"), "rb").read()
    c = vp.Circuit.custom(*args)
    try:
        assert c.verify_full_record(rec) and vp.last_gkr_failure() is None
        bad, old, new = fc.record_forgery(args, rec)
        assert old != new and old[-16:] != new[-16:]
        assert not c.verify_full_record(bad) and vp.last_gkr_failure() == ("input", 0, -1), "claim != input_0"
        # the GKR section alone is a transcript every check of which holds but the input's
        assert not c.verify_transcript(new) and vp.last_gkr_failure() == ("input", 0, -1)
        assert c.verify_full_record(rec) and vp.last_gkr_failure() is None
    finally:
        c.close()


def test_accessor_is_declared_and_exported(vp):
    hdr = open(os.path.join(ROOT, "virgo-plus_amd", "host", "vphost.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", vp.LIB_HOST], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "int vph_last_gkr_failure(int *layer, int *round);" in hdr and re.search(r" T vph_last_gkr_failure$", nm, flags=re.M)
    assert vp.GKR_CHECKS == (None,) + gv.KINDS and callable(vp.last_gkr_failure)
    assert vp.lib_host().vph_last_gkr_failure(None, None) in range(7)
