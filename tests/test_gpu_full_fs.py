"""Session.prove_full_fs / Circuit.verify_full_fs on the device: the joined non-interactive proof of the whole protocol (host/vphost.h, "The joined proof").

  circuits     the CPU tests' circuits (Circuit.randomize(3, 7, seed=11) with the zero mask, randomize(3, 9, seed=12) with ms = 8: the bytes of the fixtures under
               tests/golden/), custom_a (n = 10; every gate type, constants, assert gates) with the zero mask and with ms = 8 and a shorter public mask, SHA-256 x1
  reference    tests/full_fs_ref.py, assemble(): the record built from the ORACLE alone, stage by stage on the hashlib-derived challenges — so for every circuit here
               the GKR slice equals orc_prove_gkr_tape on the derived challenges, the commitment sections (root_l, root_h, input_0, all_sum, FRI roots, final
               codewords, every opening) equal orc_commitment_array_masked on the derived point and fold challenges, the fft_gkr section equals orc_fft_gkr_tape on
               the derived tape, and the whole record is compared byte for byte; the prover's derived point is the reference's
  checks       accepted on the host and with device=0; two runs give the same bytes; the record's sections add up; every tampered section (tests/full_fs_ref.py) is
               rejected in both verifier modes with the same reason; malformed proofs are refused
  refusals     a session with a sharded commitment; the session goes on working"""
import struct

import numpy as np
import pytest

import full_fs_ref as ff
import pc_masked_inputs as pmi

pytestmark = pytest.mark.gpu


def verdict(c, proof, device=None):
    try:
        return c.verify_full_fs(proof, device=device)
    except ValueError as e:
        return "malformed", str(e)


def check_proof(c, s, reps, oc=None, consts=None, asserts=None, **kw):
    """oc: the oracle's copy of the circuit — the proof must be the record full_fs_ref.assemble builds from it"""
    proof, pt = s.prove_full_fs(reps=reps, return_point=True, **kw)
    if oc is not None:
        assert oc.hash() == c.hash()
        okw = {"pri_mask": kw["mask"], "oracle_pub_mask": kw["pub_mask"]} if kw else {}
        want, d = ff.assemble(oc, proof, consts=consts, asserts=asserts, **okw)
        assert want == proof, "not the record the oracle assembles on the derived challenges"
        assert d["point"].tobytes() == pt.tobytes()
    assert s.prove_full_fs(reps=reps, **kw) == proof, "a second run gives other bytes"
    n = c.layer_bitlen(0)
    assert struct.unpack_from("<4I", proof) == (ff.MAGIC, ff.VERSION, n, reps) and ff.sections(proof)["end"] == len(proof)
    ok, why, pt_v = c.verify_full_fs(proof, return_point=True)
    assert (ok, why) == (True, "") and pt_v.tobytes() == pt.tobytes()
    assert c.verify_full_fs(proof, device=0) == (True, "")
    return proof


@pytest.fixture(scope="module")
def small(vp):
    _, layers, log_size, seed, reps = ff.FIXTURE
    c = vp.Circuit.randomize(layers, log_size, seed=seed)
    s = vp.Session(c, device=0)
    yield c, s, reps
    s.close()
    c.close()


def test_the_cpu_tests_circuits_give_the_recorded_bytes(vp, ob, small):
    c, s, reps = small
    _, layers, log_size, seed, _ = ff.FIXTURE
    oc = ob.Circuit.randomize(layers, log_size, seed=seed)
    assert check_proof(c, s, reps, oc=oc) == ff.fixture()
    other = check_proof(c, s, reps + 2, oc=oc)
    _, layers, log_size, seed, reps_m = ff.FIXTURE_MASKED
    f = ff.masked_family()
    cm = vp.Circuit.randomize(layers, log_size, seed=seed)
    sm = vp.Session(cm, device=0)
    try:
        assert check_proof(cm, sm, reps_m, oc=ob.Circuit.randomize(layers, log_size, seed=seed), mask=f["pri_mask"], pub_mask=f["pub_mask"]) == ff.fixture(masked=True)
    finally:
        sm.close()
        cm.close()
    assert other[64:96] != ff.fixture()[64:96], "reps is in the chain in front of the GKR part"


def test_tampered_and_malformed_proofs_in_both_verifier_modes(small):
    c, s, reps = small
    proof = s.prove_full_fs(reps=reps)
    for what, (bad, word) in ff.tampered(proof).items():
        host, dev = verdict(c, bad), verdict(c, bad, device=0)
        assert host[0] is False and host[1] and word in host[1], (what, host)
        assert dev == host, (what, host, dev)
    for what, x in list(ff.malformed(proof).items())[::3]:
        assert verdict(c, x)[0] == "malformed" and verdict(c, x, device=0)[0] == "malformed", what


def test_custom_a_zero_mask_and_masked(vp, ob, golden):
    import custom_circuits as cc
    g = golden["custom_a"]
    arrays = cc.make(g["custom"]["seed"], g["custom"]["sizes"])
    c = vp.Circuit.custom(*arrays)
    ref = {"oc": ob.Circuit.custom(*arrays), "consts": arrays[5], "asserts": arrays[6]}
    n = c.layer_bitlen(0)
    s = vp.Session(c, device=0)
    try:
        plain = check_proof(c, s, 5, **ref)
        assert struct.unpack_from("<2Q", plain, 16) == (1, 0)
        f = pmi.family("short_pub", n, 8)
        masked = check_proof(c, s, 5, mask=f["pri_mask"], pub_mask=f["pub_mask"], **ref)
        ms, n_pub = struct.unpack_from("<2Q", masked, 16)
        assert ms == 8 and n_pub == f["pub_mask"].shape[0] < 8
        sec = ff.sections(masked)
        assert np.frombuffer(masked, np.uint64, 32 * 2, sec["final_mask"]).any(), "a vacuous masked case"
        for what, off in {"the public mask": sec["pub_mask"] + 3, "all_sum[64]": sec["all_sum"] + 64 * 16 + 8, "the final mask": sec["final_mask"] + 16}.items():
            bad = bytearray(masked); bad[off] ^= 0x04
            assert verdict(c, bytes(bad))[0] is False and verdict(c, bytes(bad), device=0)[0] is False, what
        assert check_proof(c, s, 5) == plain, "the zero mask after a masked run"
    finally:
        s.close()
        c.close()


def test_sha256_x1(vp, ob, pws_path):
    c = vp.Circuit.from_pws(pws_path, 1, seed=1)
    s = vp.Session(c, device=0)
    try:
        proof = check_proof(c, s, 4, oc=ob.Circuit.from_pws(pws_path, 1, seed=1))      # (the .pws gates carry no constants and no assert flags)
        bad = bytearray(proof); bad[ff.sections(proof)["gkr"] + 16 * 50] ^= 0x04
        assert verdict(c, bytes(bad))[0] is False
    finally:
        s.close()
        c.close()


def test_a_sharded_session_refuses(vp):
    c = vp.Circuit.randomize(8, 12, seed=1)
    s = vp.Session(c, devices=[0] * 2, round_shard_min_log=2, shard_commitment=True)
    try:
        with pytest.raises(RuntimeError, match="not built for a sharded session"):
            s.prove_full_fs(reps=3)
        tr, ok, _ = s.prove_and_verify_full(reps=3)                        # the session goes on working
        assert ok
    finally:
        s.close()
        c.close()
