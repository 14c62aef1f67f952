"""The GKR sumcheck off the seeded tapes, CPU side: the Python-integer prover (gkr_ref.py) against the oracle's tape entry (orc_prove_gkr_tape) byte for
byte on every tape family (gkr_tape_cases.py) on the small circuits; the oracle's own verifier and the host verifier (its getFinalValue, predicate and Liu
code is this project's own) on every (circuit, family) tests/test_gpu_gkr_tapes.py hands to the device — completeness holds for any challenges, so a rejected
tape is a broken test input or a verifier defect; the host verifier rejecting a transcript with one element changed; and the condition on the inputs that
makes a byte-for-byte match evidence: the transcripts of the value families are at most half zero.  tests/test_oracle_golden.py pins the tape entry itself."""
import numpy as np
import pytest

import gkr_ref as ref
import gkr_tape_cases as gc
import verifier_sums as vs

P = gc.P


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


def test_offsets_and_families_are_what_they_say(ob):
    for name in ("S", "M", "unary_mid", "zero_var"):
        off, oc, u = gc.offsets(name), gc.oracle_circuit(name), gc.tape(name, "uniform")
        n = off.n_layers
        assert off.n == oc.gkr_draws() and 16 * off.n_tr == len(oc.prove_gkr()[0])
        # the slots tile the tape in draw order
        at = off.r0[2]
        for i in range(n - 1, 0, -1):
            for slot in (off.ru[i], off.ar[i], off.rv[i], off.sig[i], off.rl[i]):
                assert slot[0] == at and slot[1] <= slot[2]
                at += slot[2]
            assert off.ru[i][1] == off.rl[i][1] == oc.layer_bitlen(i - 1) and off.sig[i][1] == n - i + 1 and off.rv[i][2] == max(0, oc.subsets(i)[2])
        assert at == off.n
        assert (u == ob.random_seq(gc.SEED, off.n)).all()
        assert not gc.tape(name, "zero").any() and (gc.tape(name, "one") == [1, 0]).all() and (gc.tape(name, "minus_one_limbs") == P - 1).all()
        assert (gc.tape(name, "minus_one") == [P - 1, 0]).all() and set(np.unique(gc.tape(name, "corner_pattern"))) <= {0, 1}
        assert set(np.unique(gc.tape(name, "edge_limbs_complex"))) <= set(gc.EDGE_LIMBS) and not gc.tape(name, "edge_limbs_real")[:, 1].any()
        sp = gc.tape(name, "sprinkle")
        hit = (sp != u).any(axis=1)
        assert 0 < hit.sum() < off.n and {tuple(int(x) for x in e) for e in sp[hit]} <= set(gc.SPRINKLE)
        in_vec = np.zeros(off.n, bool)
        for s, _, drawn in off.vectors():
            in_vec[s:s + drawn] = True
        for k in range(3):
            for vname, val in gc.STRIPE_VALUES.items():
                t = gc.tape(name, "stripes_%d_%s" % (k, vname))
                moved = (t != u).any(axis=1)
                assert not moved[~in_vec].any() and {tuple(int(x) for x in e) for e in t[moved]} == {val}
                for s, _, drawn in off.vectors():
                    assert all((tuple(int(x) for x in t[s + j]) == val) for j in range(k, drawn, 3))
                    assert all((t[s + j] == u[s + j]).all() for j in range(drawn) if j % 3 != k)
        uv = gc.tape(name, "uv_corners")
        for i in range(1, n):
            for s, _, drawn in (off.ru[i], off.rv[i]):
                assert set(np.unique(uv[s:s + drawn])) <= {0, 1}
            assert (uv[off.rl[i][0]:off.rl[i][0] + off.rl[i][2]] == u[off.rl[i][0]:off.rl[i][0] + off.rl[i][2]]).all()
        mid = gc._mid(off)
        s, _, drawn = off.sig[mid]
        assert 1 <= mid < n and not gc.tape(name, "sig_zero_mid")[s:s + drawn].any() and gc.tape(name, "sig_first_only")[s].any()
        assert not gc.tape(name, "sig_first_only")[s + 1:s + drawn].any()
        for fam, val in (("assert_0", (0, 0)), ("assert_1", (1, 0)), ("assert_m1", (P - 1, 0))):
            assert all(tuple(int(x) for x in gc.tape(name, fam)[off.ar[i][0]]) == val for i in range(1, n))
        moved = np.flatnonzero((gc.tape(name, "dont_care") != u).any(axis=1))
        assert len(off.unused()) > 0 and sorted(moved.tolist()) == sorted(off.unused().tolist())
    off = gc.offsets("S")                                    # bit lengths 6, 6, 6, 5; maxDadBitLength 5, 5, 3
    assert off.locate(0).startswith("Vres") and off.locate(1) == "layer 3, phase 1, round 1 of 6, coefficient a"
    assert off.locate(19) == "layer 3, phase 1, claim 0 of 1" and off.locate(20) == "layer 3, phase 2, round 1 of 3, coefficient a"
    assert off.locate(29 + 2) == "layer 3, phase 2, claim 2 of 3" and off.locate(32) == "layer 3, Liu, round 1 of 6, coefficient a"
    assert off.locate(off.n_tr - 1) == "layer 1, Liu, claim 0 of 1" and off.claim_index("phase 1", 3) == 19 and off.claim_index("phase 2", 3) == 29
    with pytest.raises(IndexError):
        off.locate(off.n_tr)


@pytest.mark.parametrize("name", gc.SMALL_CIRCUITS)
def test_python_prover_vs_oracle_on_every_family(ob, name):
    """Byte for byte, whole transcript; the Python prover's own checks (gkr_ref.py lists them) run inside prove() and raise."""
    w, off = vs.wiring_from(gc.oracle_circuit(name), gc.arrays(name)), gc.offsets(name)
    for fam in gc.FAMILIES:
        got = ref.to_bytes(ref.prove(w, off, gc.tape(name, fam)))
        want, ok = gc.oracle(name, fam)
        assert ok == 1, fam
        assert gc.first_difference(name, fam, got, want) is None, gc.first_difference(name, fam, got, want)
        assert got == gc.expected(name, fam)


def test_small_circuits_have_the_shapes_they_are_there_for():
    assert gc.offsets("zero_var").bl == [3, 0, 0] and gc.offsets("zero_var").mdb[1:] == [0, 0]          # zero-variable layers, zero-round phase 2
    assert gc.offsets("unary_mid").mdb[2] == -1                                                        # no phase 2
    assert gc.offsets("tiny").bl == [3, 2, 1, 0]
    a = gc.arrays("edge_small")
    assert max(int(x) for x in a[0]) <= 64 and set(int(x) for x in a[3][:int(a[0][0])]) <= set(gc.EDGE_VALUES) and a[5][:, 1].any()
    assert set(int(x) for x in a[5].ravel()) <= set(gc.EDGE_VALUES)


@pytest.mark.parametrize("name", gc.GPU_CIRCUITS + gc.SMALL_CIRCUITS)
def test_both_verifiers_accept_every_tape_and_value_families_are_not_mostly_zero(ob, host_circuits, name):
    c = host_circuits(name)
    shares = {}
    for fam in gc.FAMILIES:
        tr, ok = gc.oracle(name, fam)
        assert ok == 1, "%s / %s: the oracle's verifier rejects the oracle's proof" % (name, fam)
        assert c.verify_transcript_tape(gc.tape(name, fam), tr), "%s / %s: the host verifier rejects the oracle's proof" % (name, fam)
        shares[fam] = gc.zero_share(tr)
    print(name, {k: round(v, 2) for k, v in shares.items()})
    for fam in gc.VALUE:
        assert shares[fam] <= gc.MAX_ZERO_SHARE, "%s / %s: %.2f of the transcript is zero" % (name, fam, shares[fam])
    assert gc.oracle(name, "dont_care")[0] == gc.oracle(name, "uniform")[0], "the oracle's messages moved with a draw they do not depend on"


@pytest.mark.parametrize("name", ["S", "M", "unary_mid", "R"])
def test_host_verifier_rejects_one_changed_element(host_circuits, name):
    """On an edge tape and on the uniform one: the first limb of one NON-ZERO element is changed by one — Vres, a round coefficient of every sumcheck kind, every
    kind of claim, the last element.  (A zero element can be a don't-care: with sig = 0 a whole Liu sumcheck is.)  The tape with one used element changed is
    rejected as well, and the tape's refusals are errors, not verdicts."""
    c, off = host_circuits(name), gc.offsets(name)
    top = off.n_layers - 1
    for fam in ("sprinkle", "uniform"):
        tape, tr = gc.tape(name, fam), gc.oracle(name, fam)[0]
        assert c.verify_transcript_tape(tape, tr) and c.verify_transcript_tape(tape, tr, skip_predicates=True)
        el = gc.elements(tr)
        spots = [0, 1, 2, 3, off.claim_index("phase 1", top), off.claim_index("Liu", top) - 2, off.claim_index("Liu", top), off.claim_index("phase 1", 1) - 1, off.n_tr - 1]
        if off.mdb[top] != -1:
            spots += [off.claim_index("phase 2", top) - 3, off.claim_index("phase 2", top), off.claim_index("phase 2", top) + top - 1]
        changed = 0
        for at in spots:
            if el[at] == (0, 0):
                continue
            bad = bytearray(tr)
            bad[16 * at:16 * at + 8] = ((el[at][0] + 1) % P).to_bytes(8, "little")
            assert not c.verify_transcript_tape(tape, bytes(bad)), "%s / %s: accepted with element %d (%s) changed" % (name, fam, at, off.locate(at))
            changed += 1
        assert changed >= 8
        assert not c.verify_transcript_tape(tape, tr[:-16]) and not c.verify_transcript_tape(tape, tr + tr[-16:])
        t = np.array(tape)
        s = off.ru[top][0]
        t[s, 0] = (int(t[s, 0]) + 1) % P
        assert not c.verify_transcript_tape(t, tr), "accepted on another tape"
        for t in (tape[:-1], np.concatenate([tape, tape[:1]])):
            with pytest.raises(ValueError):
                c.verify_transcript_tape(t, tr)
        t = np.array(tape)
        t[off.n - 1, 1] = P
        with pytest.raises(ValueError):
            c.verify_transcript_tape(t, tr)


@pytest.mark.parametrize("name", ["S", "M", "R", "tiny", "zero_var", "unary_mid", "K_skewed"])
def test_corner_claims_are_looked_up_witness_values(ob, name):
    """gkr_tape_cases.corner_claims — the expectation the GPU file holds the device's claims to on the uv_corners tape — against the oracle's transcript, with the
    values from verifier_sums.evaluate (Python integers) where the circuit is small and from the oracle's layer MLE at one-hot points elsewhere."""
    oc, off = gc.oracle_circuit(name), gc.offsets(name)
    if name in gc.SMALL_CIRCUITS:
        values = vs.evaluate(vs.wiring_from(oc, gc.arrays(name)))
    else:
        class OneHot:                                       # values[i][w]: the layer's MLE at the corner that is the index w
            def __init__(self, i):
                self.i, self.n = i, oc.layer_size(i)
            def __len__(self):
                return self.n
            def __getitem__(self, w):
                return oc.layer_mle(self.i, [((w >> b) & 1, 0) for b in range(off.bl[self.i])])
        values = [OneHot(i) for i in range(off.n_layers - 1)]
    want = gc.corner_claims(name, values)
    got = gc.elements(gc.oracle(name, "uv_corners")[0])
    assert len(want) == sum(claims for ph, _, _, _, claims in off.parts if ph in ("phase 1", "phase 2"))
    for at, v in want.items():
        assert got[at] == v, (name, at, off.locate(at))
    assert any(v != (0, 0) for v in want.values())
