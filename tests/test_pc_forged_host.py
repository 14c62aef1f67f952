"""CPU: the host verifier's ALGEBRA (PcSliceCheck through pcVerifyCommitment's loop, host/verifier.cpp) held to forgeries that pass every Merkle check.

Every other rejection test of the 64 witness slices changes bytes under a root that stays as it was, and is caught before any algebra runs.  Here the values are
changed and then re-committed (tests/pc_forge.py), or they are arguments no tree covers, and for every case of tests/pc_forged_cases.py

  (i)   the definition-level verifier (tests/pc_verifier_ref.py) gives the verdict, the name of the check and the repetition — and it must be the check the case
        was built for (a condition on the table, not a measurement);
  (ii)  Circuit.verify_commitment returns exactly that verdict and name;
  (iii) the control — the same machinery, no value changed — is the honest proof byte for byte and is accepted.

n = 9 (N = 8, 3 levels) and n = 10 (4 levels), the zero mask (ms = 1) and a uniform one (ms = 8), 33 repetitions with both ends of the position range; slices
0, 1, 31, 63; the first, a middle and the last repetition.

The corner.  One position is s0 = 64 on purpose, a multiple of 32: x0 = w^s0 has x0^N = 1, and so has x1 = -x0 (N is even), so the term (x^N - 1) h(x) vanishes
at both points and a re-committed change of h there is invisible: the protocol's own relation does not involve h at the N-th roots of unity.  The reference
verifier ACCEPTS those four-per-slice forgeries of h (asserted below: accepted by the definition, so accepted by the host), and rejects the same change of l at
that position at round 0.  This is no hole: h's values there are pinned by the low-degree test of the virtual oracle through every other position."""
import numpy as np
import pytest

import masked_verifier_cases as mvc
import pc_forge as forge
import pc_forged_cases as fc
import pc_verifier_ref as vref
import test_masked_verifier_host as mvh


def _ids(cs):
    return [c["id"] for c in cs]


@pytest.mark.parametrize("n,kind", fc.PROOFS + [(9, "point"), (10, "point")])
def test_forgeries_are_rejected_by_the_check_they_break(vp, ob, n, kind):
    p = fc.proof(ob, n, kind)
    assert fc.ref_verify(p) == (True, "", None, None) and fc.host_verify(vp, p) == (True, "")
    if kind == "point":
        assert fc.ref_verify(p, point=p["point"]) == (True, "", None, None) and fc.host_verify(vp, p, point=p["point"]) == (True, "")
    if kind == "uniform":
        assert p["ms"] == 8 and p["all_sum"][64].any() and p["final_mask"].any()
    assert forge.forge(p, [])["answer"] == p["answer"] and forge.forge(p, [])["root_l"] == p["root_l"]
    cs = fc.cases(p)
    kinds = {(k, up) for (k, up) in fc.level_reps(p)}
    assert kinds == {(k, up) for k in range(n - 6) for up in (False, True)}, "both kinds of position at every level"
    seen, accepted_corner = set(), 0
    for c in cs:
        q, kw = c["q"], c["kw"]
        cq, ckw = c["control"]
        for key in ("root_l", "root_h", "fri_roots", "answer"):
            assert cq[key] == p[key], "the control of %s is not the honest proof" % c["id"]
        for key, v in ckw.items():
            assert np.array_equal(v, p[key])
        if cq is not p or ckw:
            assert fc.host_verify(vp, cq, **ckw) == (True, ""), "control of " + c["id"]
        ok, name, rep, _ = fc.ref_verify(q, **kw)
        if c["must"] is None:                        # the corner: what the definition decides is the expectation
            assert q["leaf0"][fc.CORNER_REP] == fc.CORNER and "h[" in c["id"] and q["root_h"] != p["root_h"]
            assert ok, "the definition rejects a change of h where x^N = 1: " + c["id"]
            accepted_corner += 1
        else:
            assert not ok and name == c["must"], (c["id"], name)
            assert c["rep"] is None or rep == c["rep"], (c["id"], rep)
        assert fc.host_verify(vp, q, **kw) == (ok, name), c["id"]
        seen.add(name)
    assert accepted_corner == 2 * len(fc.SLICES)
    want = {"", vref.SUMS, vref.RS, vref.FINAL} | {vref.round_name(k) for k in range(n - 6)}
    assert seen == want, "every algebraic verdict of the witness slices occurs, and no other"
    assert len(set(_ids(cs))) == len(cs)


@pytest.mark.parametrize("n,kind", fc.PROOFS)
def test_a_forgery_in_one_repetition_is_rejected_at_that_repetition(vp, ob, n, kind):
    """consistent at every queried position of every repetition but one: without that repetition the forged commitment is accepted"""
    p = fc.proof(ob, n, kind)
    for rep in (0, fc.MID, len(p["leaf0"]) - 1):
        s0 = p["leaf0"][rep]
        q = forge.forge(p, [(0, s0, 2 * 31, forge.f_add(p["vals"][0][s0, 62], fc.D))])
        assert q["root_l"] != p["root_l"]
        assert fc.ref_verify(q) == (False, vref.round_name(0), rep, 31)
        assert fc.host_verify(vp, q) == (False, vref.round_name(0))
        rest = forge.with_positions(q, p["leaf0"][:rep] + p["leaf0"][rep + 1:])
        assert fc.ref_verify(rest) == (True, "", None, None) and fc.host_verify(vp, rest) == (True, "")


def test_the_reference_verifier_decides_the_recorded_cases(vp, ob):
    """tests/pc_verifier_ref.py on the proofs of tests/test_masked_verifier_host.py: its accept set, and every rejection that file asserts by name"""
    R = lambda p, **kw: vref.verify_p(p, **kw)[:2]
    for n, ms in mvh.ACCEPT:
        for fam in mvh.pmi.FAMILIES:
            assert R(mvh.proof(ob, n, ms, fam)) == (True, "")
        p = mvh.proof(ob, n, ms, "short_pub")
        fail = vref.round_name(0, mask=True)
        pm = p["pub_mask"].copy(); pm[0, 0] ^= np.uint64(1)
        assert R(p, pub_mask=pm) == (False, fail)
        if ms >= 16:
            assert R(p, ms=ms // 2) == (False, fail)
        sums = p["all_sum"].copy(); sums[64] = mvc.f_add(sums[64], (5, 7))
        assert R(p, claim=mvc.f_add(p["claim"], (5, 7)), all_sum=sums) == (False, vref.SUMS)
        assert R(p, all_sum=sums) == (False, fail)
        p = mvh.proof(ob, n, ms, "edges")
        fm = p["final_mask"].copy(); fm[:] = mvc.f_add(fm[0], (1, 0))
        assert R(p, final_mask=fm) == (False, vref.FINAL_MSK)
        fm = p["final_mask"].copy(); fm[31] = mvc.f_add(fm[31], (0, 1))
        assert R(p, final_mask=fm) == (False, vref.RS_MSK)
    for n in (9, 10):
        p = mvh.proof(ob, n, 1, "zero")
        assert R(p) == (True, "") and R(p, pub_mask=None) == (True, "")
        sums = p["all_sum"].copy(); sums[64] = mvc.f_add(sums[64], (1, 0))
        assert R(p, claim=mvc.f_add(p["claim"], (1, 0)), all_sum=sums) == (False, vref.SUMS)
        assert R(p, all_sum=sums) == (False, vref.round_name(0, mask=True))
        fm = p["final_mask"].copy(); fm[:, 0] = 3
        assert R(p, final_mask=fm) == (False, vref.FINAL_MSK)
    for n, mult in [(9, 2), (9, 4), (10, 2), (10, 4)]:
        assert R(mvh.proof(ob, n, mult << (n - 6), "uniform")) == (False, vref.RS_MSK)
    p = mvh.proof(ob, 10, 16, "uniform")
    for oracle in (0, 1, 2, 4):
        _, leaf, _ = mvh.ref.query_leaves(10, p["leaf0"][3])[oracle]
        vals = [v.copy() for v in p["vals"]]
        vals[oracle][leaf, 128 + (oracle & 1), 1] ^= np.uint64(4)
        assert R(p, answer=mvc.answer(p, vals)) == (False, vref.MERKLE if oracle < 2 else vref.level_merkle(oracle - 2))
