"""CPU: the joined non-interactive proof of the whole protocol (vph_verify_full_fs; chain and layout: host/vphost.h, "The joined proof") without a device.

The reference is tests/full_fs_ref.py: assemble() builds the record from the ORACLE alone — orc_prove_gkr_tape, orc_commitment_array_masked, orc_fft_gkr_tape — stage
by stage on challenges derived with hashlib from the text in vphost.h (statement digest computed in Python from the oracle's gate tables, head, the GKR part's schedule,
the commitment head, fft_gkr's tape, the fold challenges, the positions), and by induction over the chain a candidate that every stage reproduces is the unique joined
proof.  The candidates are tests/golden/full_fs_rand3_7.bin (Circuit.randomize(3, 7, seed=11): the smallest circuit with an input layer of 2^7 wires, 3 repetitions, the
zero mask) and full_fs_rand3_9_ms8.bin (randomize(3, 9, seed=12), ms = 8 with a shorter public mask: n = 9 is the smallest size whose verifier accepts ms = 8),
written by tests/golden/make_full_fs.py, which runs the same assemble().

  reference       assemble(oracle, fixture) is the fixture, byte for byte, zero mask and ms = 8; the reference notices a changed GKR element, root, all_sum or fft_gkr
                  element itself (the stage that fails is named); the Python statement digest with the input values is the one orc_prove_fs's proof starts from
  honest          a verifier holding only the circuit accepts both; the derived point is the reference's; the record's sections add up to its length
  another circuit the same bytes under a circuit that differs in a gate, in depth or in input size: rejected or malformed — the statement is bound
  tampered        one bit in every section in turn (field elements kept canonical): rejected, the reason names the failed check; root_l or a GKR element moves
                  the derived point; a changed later section leaves it
  malformed       truncated, extended, non-canonical limbs, wrong headers: ValueError
  sanitizers      tests/sanitize/full_fs_main.cpp: the host sources under ASan / UBSan as a stand-alone program over the good proof and damaged ones
  symbols         declared, exported"""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import full_fs_ref as ff
from conftest import ROOT


@pytest.fixture(scope="module")
def fixture(vp):
    _, layers, log_size, seed, reps = ff.FIXTURE
    c = vp.Circuit.randomize(layers, log_size, seed=seed)
    yield c, ff.fixture()
    c.close()


def verdict(c, proof):
    try:
        return c.verify_full_fs(proof, return_point=True)
    except ValueError as e:
        return "malformed", str(e), None


def test_the_recorded_proof_is_accepted_by_the_circuit_alone(vp, fixture):
    c, proof = fixture
    magic, version, n, reps, ms, n_pub = struct.unpack_from("<4I2Q", proof)
    assert (magic, version, n, reps, ms, n_pub) == (ff.MAGIC, ff.VERSION, c.layer_bitlen(0), ff.FIXTURE[4], 1, 0) and n == 7
    assert ff.sections(proof)["end"] == len(proof)
    ok, why, pt = c.verify_full_fs(proof, return_point=True)
    assert (ok, why) == (True, "") and pt.shape == (n, 2) and int(pt.max()) < ff.P and len({bytes(x) for x in pt}) == n
    assert c.verify_full_fs(proof) == (True, "")


def test_the_statement_is_bound_and_the_input_values_are_not_in_it(vp, fixture):
    c, proof = fixture
    _, layers, log_size, seed, _ = ff.FIXTURE
    other_inputs = vp.Circuit.randomize(layers, log_size, seed=seed)      # the same draws ...
    assert other_inputs.hash() == c.hash()
    assert other_inputs.verify_full_fs(proof) == (True, "")
    other_inputs.close()
    for what, c2 in {"another seed": vp.Circuit.randomize(layers, log_size, seed=seed + 1), "one more layer": vp.Circuit.randomize(layers + 1, log_size, seed=seed),
                     "a larger input layer": vp.Circuit.randomize(layers, log_size + 1, seed=seed)}.items():
        assert verdict(c2, proof)[0] in (False, "malformed"), what
        c2.close()


def test_one_changed_bit_in_any_section_is_rejected_with_the_failed_check_named(vp, fixture):
    c, proof = fixture
    _, _, honest = c.verify_full_fs(proof, return_point=True)
    s = ff.sections(proof)
    for what, (bad, word) in ff.tampered(proof).items():
        ok, why, pt = verdict(c, bad)
        assert ok is False and why, what
        assert word in why, (what, why)
        moved = pt.tobytes() != honest.tobytes()
        if what in ("root_l", "the first GKR element", "a GKR element in the middle"):
            assert moved and "GKR" in why, what + ": the point must move"
        elif what != "the last GKR element":
            assert not moved, what + ": nothing behind the GKR part reaches the point"
    for field, off in {"magic": 1, "version": 4, "n": 8, "reps": 12, "ms": 16, "n_pub": 24}.items():
        bad = bytearray(proof); bad[off] ^= 0x04
        assert verdict(c, bytes(bad))[0] in (False, "malformed"), field
    assert s["gkr"] == 64


def test_malformed_proofs_are_refused(vp, fixture):
    c, proof = fixture
    for what, x in ff.malformed(proof).items():
        ok, why, _ = verdict(c, x)
        assert ok == "malformed" and why, (what, ok, why)


def test_new_symbols_are_declared_and_exported(vp):
    host_hdr = open(os.path.join(ROOT, "virgo-plus_amd", "host", "vphost.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", vp.LIB_HOST], stdout=subprocess.PIPE, text=True, check=True).stdout
    for s in ("vph_prove_full_fs", "vph_verify_full_fs"):
        assert re.search(r"\b%s\s*\(" % s, host_hdr), s + " is not declared"
        assert re.search(r" T %s$" % s, out, flags=re.M), s + " is not exported"
    assert "The joined proof" in host_hdr
    assert hasattr(vp.Session, "prove_full_fs") and hasattr(vp.Circuit, "verify_full_fs")


def test_parser_and_verifier_under_asan_ubsan(vp, fixture, tmp_path):
    """tests/sanitize/full_fs_main.cpp with the host sources, -fsanitize=address,undefined: the recorded proof accepted, then changed bytes, every truncation class,
    header fields at their extremes, non-canonical limbs — each must end in a verdict, none in a report"""
    _, proof = fixture
    good = tmp_path / "proof.bin"
    good.write_bytes(proof)
    out_dir = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "full_fs_asan")
    host = os.path.join(ROOT, "virgo-plus_amd", "host")
    csrc = os.path.join(ROOT, "virgo-plus_amd", "csrc")
    src = [os.path.join(host, f) for f in ("circuit.cpp", "prover.cpp", "verifier.cpp", "vphost.cpp")] + [os.path.join(ROOT, "tests", "sanitize", "full_fs_main.cpp")]
    deps = src + [os.path.join(host, f) for f in os.listdir(host) if f.endswith((".hpp", ".h"))]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-pthread"] + san + ["-o", exe] + src + ["-L" + csrc, "-lvpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    s = ff.sections(proof)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    args = [str(v) for v in ff.FIXTURE[1:4]] + [str(good), str(s["gkr"]), str(s["root_h"])]
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "full_fs_asan ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_the_record_assembled_from_the_oracle_is_the_fixture(vp, ob, masked):
    _, layers, log_size, seed, reps = ff.FIXTURE_MASKED if masked else ff.FIXTURE
    proof = ff.fixture(masked)
    f = ff.masked_family()
    kw = {"pri_mask": f["pri_mask"], "oracle_pub_mask": f["pub_mask"]} if masked else {}
    oc = ob.Circuit.randomize(layers, log_size, seed=seed)
    want, d = ff.assemble(oc, proof, **kw)
    assert want == proof, "the oracle's joined proof on the hashlib-derived challenges is not the recorded one"
    c = vp.Circuit.randomize(layers, log_size, seed=seed)
    assert c.hash() == oc.hash()
    ok, why, pt = c.verify_full_fs(proof, return_point=True)
    assert (ok, why) == (True, "") and pt.tobytes() == d["point"].tobytes(), "the verifier's derived point is not the reference's"
    magic, version, n, r, ms, n_pub = struct.unpack_from("<4I2Q", proof)
    assert (n, r, ms) == (log_size, reps, 8 if masked else 1) and n_pub == (f["pub_mask"].shape[0] if masked else 0)
    if masked:
        s = ff.sections(proof)
        assert n_pub < 8 and np.frombuffer(proof, np.uint64, 64, s["final_mask"]).any() and np.frombuffer(proof, np.uint64, 2, s["all_sum"] + 64 * 16).any(), "a vacuous masked case"
    c.close()


def test_the_reference_itself_notices_a_changed_section(ob):
    """the induction's premise is checked stage by stage: a candidate with one changed element is not reproduced by the oracle, and the stage says where"""
    _, layers, log_size, seed, _ = ff.FIXTURE
    proof = ff.fixture()
    oc = ob.Circuit.randomize(layers, log_size, seed=seed)
    s = ff.sections(proof)
    for what, off, stage in (("a GKR element", s["gkr"] + 160, "stage 3"), ("root_l", s["root_l"], "stage 3"), ("all_sum", s["all_sum"] + 32, "stage 5"),
                             ("an fft_gkr element", s["fft_gkr"] + 64, "stage 5"), ("a FRI root", s["fri_roots"] + 3, "stage 6"), ("root_h", s["root_h"] + 1, "stage 5")):
        bad = bytearray(proof); bad[off] ^= 0x04
        with pytest.raises(AssertionError, match=stage):
            ff.assemble(oc, bytes(bad))
            pytest.fail(what)
    for what, off in (("the final codeword", s["final_code"] + 99), ("an opened value", s["answer"] + 7)):      # not inputs of a challenge the oracle is handed:
        bad = bytearray(proof); bad[off] ^= 0x04                                                                    # the oracle's own bytes come back
        assert ff.assemble(oc, bytes(bad))[0] == proof, what


def test_the_python_statement_digest_with_inputs_is_the_one_of_the_oracles_fs_proof(vp, ob):
    """The digest code of full_fs_ref is held to something outside this change: with the input values in, it is the statement vph_prove_fs / orc_prove_fs bind —
    the oracle's FS proof of the fixture's circuit, replayed with hashlib from that digest, derives the challenges on which orc_prove_gkr_tape returns it."""
    import gkr_tape_cases as gc
    import pc_fs_ref as fs
    _, layers, log_size, seed, _ = ff.FIXTURE
    oc = ob.Circuit.randomize(layers, log_size, seed=seed)
    proof, _ = oc.prove_fs()
    assert vp.Circuit.randomize(layers, log_size, seed=seed).verify_fs(proof)
    with_in, without = ff.statement_digest(oc, True), ff.statement_digest(oc, False)
    assert with_in != without
    other = ob.Circuit.randomize(layers, log_size, seed=seed + 1)
    assert ff.statement_digest(other, False) != without
    ch = fs.Chain()
    ch.step(*struct.unpack("<4Q", with_in))
    ch.step(oc.layers, 0, 0, 0x53)
    off = gc.Offsets.of(oc)
    tape = ff.gkr_schedule(ch, off, np.frombuffer(proof, np.uint64).reshape(-1, 2)[:off.n_tr])
    assert oc.prove_gkr_tape(tape)[0] == proof[:16 * off.n_tr]
