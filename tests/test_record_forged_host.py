"""CPU: verifier::verifyPoly's own loop (checkFull / verify_full_record) held to re-committed forgeries of a complete-protocol record.

tests/test_query_record_host.py flips bytes under roots that stay as they were: every flip in an opening is a Merkle rejection, and a flipped entry of the final
codeword only reaches the constancy check.  Here an oracle of tests/golden/full_record_custom_a.bin (n = 10, 4 FRI levels, 2 repetitions) gets a FRESH tree
(tests/pc_forge.py: recommit) — filler leaves, the opened values at their recovered positions, a new root and new paths in the record — so that the Merkle checks
pass and the verdict is the algebra's.  The control of every family is the same machinery with the recorded values: accepted.  The name of the failed check is
what the verifier prints on stderr (captured at the file descriptor).  The record's challenges are drawn by the verifier's own generator and cannot be had in
Python, so the names are compared with the strings of host/verifier.cpp, not with tests/pc_verifier_ref.py (which decides the same forgeries at commitment
level, tests/test_pc_forged_host.py)."""
import numpy as np
import pytest

import pc_forge as forge
import pc_verifier_ref as vref
from test_query_record_host import case  # noqa: F401  (the fixture: circuit, record, offsets)

D = (3, 5)


def verdict(c, rec, capfd):
    capfd.readouterr()
    ok = c.verify_full_record(rec)
    err = capfd.readouterr().err.strip().splitlines()
    return ok, err[-1] if err else ""


def elem(rec, off):
    return tuple(int(x) for x in np.frombuffer(rec[off:off + 16], np.uint64))


def put(rec, off, value):
    return rec[:off] + np.array(value, np.uint64).tobytes() + rec[off + 16:]


@pytest.fixture(scope="module")
def parsed(case):
    sec = forge.sections(case["rec"])
    assert {k: sec[k] for k in ("fft_gkr", "roots", "final", "openings")} == {k: case["sec"][k] for k in ("fft_gkr", "roots", "final", "openings")}
    ops = forge.openings(case["rec"], sec)
    assert len(ops) == 2 and ops[0][0]["leaf"] != ops[1][0]["leaf"]
    return sec, ops


@pytest.mark.parametrize("s", [0, 1, 31, 63])
def test_another_final_constant_is_a_last_pair_rejection(case, parsed, capfd, s):
    sec, _ = parsed
    rec = same = case["rec"]
    other = forge.f_add(elem(rec, sec["final"] + 16 * (s << 1)), D)
    for i in range(16):
        for hi in range(2):
            off = sec["final"] + 16 * ((i << 7) | (s << 1) | hi)
            same = put(same, off, elem(same, off))
            rec = put(rec, off, other)
    assert same == case["rec"] and verdict(case["c"], same, capfd) == (True, "")
    assert verdict(case["c"], rec, capfd) == (False, vref.FINAL)


@pytest.mark.parametrize("j", [0, 1, 31, 63])
def test_slice_sums_moved_against_each_other_are_a_round_0_rejection(case, parsed, capfd, j):
    sec, _ = parsed
    rec, j2 = case["rec"], (j + 1) % 64
    a, b = sec["all_sum"] + 16 * j, sec["all_sum"] + 16 * j2
    bad = put(put(rec, a, forge.f_add(elem(rec, a), D)), b, forge.f_add(elem(rec, b), (vref.P - D[0], vref.P - D[1])))
    assert put(put(rec, a, elem(rec, a)), b, elem(rec, b)) == rec
    assert verdict(case["c"], bad, capfd) == (False, vref.round_name(0))
    alone = put(rec, a, forge.f_add(elem(rec, a), D))          # (one sum alone: off the claim)
    assert verdict(case["c"], alone, capfd) == (False, vref.SUMS)


@pytest.mark.parametrize("oracle", range(6))
def test_recommitted_openings(case, parsed, capfd, oracle):
    """l, h and every FRI level: the fresh-tree control is accepted; one compared value changed in repetition 0, and separately in repetition 1, is rejected by
    the round that compares it, and the pair's other element (of a level) by the round after, the last level's by the last pair"""
    sec, ops = parsed
    c, rec, ln = case["c"], case["rec"], sec["n"] - 6
    fresh = forge.recommit(rec, sec, oracle)
    ro = forge.root_offset(sec, oracle)
    assert fresh != rec and fresh[ro:ro + 32] != rec[ro:ro + 32] and len(fresh) == len(rec)
    assert [[e["vals"].tobytes() for e in row] for row in forge.openings(fresh, sec)] == [[e["vals"].tobytes() for e in row] for row in ops]
    assert verdict(c, fresh, capfd) == (True, "")
    for rep in (0, 1):
        shared = [r for r in (0, 1) if ops[r][oracle]["leaf"] == ops[rep][oracle]["leaf"]]
        up = 0 if oracle < 2 else int(forge.upper(ops, rep, oracle - 2))
        for j in (0, 63):
            for which in ("compared", "other"):
                if oracle < 2:                       # l and h: both elements enter round 0
                    e, want = 2 * j + (which == "other"), vref.round_name(0)
                else:
                    k = oracle - 2
                    e = 2 * j + (up if which == "compared" else 1 - up)
                    want = vref.round_name(k) if which == "compared" else vref.round_name(k + 1) if k + 1 < ln else vref.FINAL
                v = ops[rep][oracle]["vals"].copy()
                v[e] = forge.f_add(v[e], D)
                bad = forge.recommit(rec, sec, oracle, {r: v for r in shared})
                if len(shared) == 1 or rep == 0:
                    assert verdict(c, bad, capfd) == (False, want), (oracle, rep, j, which)
                else:                                # a leaf both repetitions open: repetition 0 meets the change first, maybe with the other element
                    ok, name = verdict(c, bad, capfd)
                    assert not ok and name.startswith("Fri "), (oracle, rep, j, which, name)


def test_positions_recovered_from_the_paths_have_both_kinds(parsed):
    sec, ops = parsed
    n = sec["n"]
    for row in ops:
        assert 1 << (n - 7) <= row[0]["leaf"] < 1 << (n - 2)
    ups = [forge.upper(ops, rep, k) for rep in (0, 1) for k in range(n - 6)]
    assert any(ups) and not all(ups)
