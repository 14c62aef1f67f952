"""CPU: the oracle (oracle/vp_oracle.cpp) against the fixtures made from the REAL reference
(tests/golden/make_golden.py) and the known answers recorded in SURVEY.md §8c."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

P = (1 << 61) - 1
SURVEY_SHA256 = {
    "sha256_x1": "7d56df550455f8e32dcda3ea158e2606b23f4e8bac761ca6a081b8caeee65047",
    "sha256_x16": "d9c442312561023d237a0c8ea1a40f26273c8d5a967028ab3f1bfeafe22d179f",
    "sha256_x64": "69974a97b58f46102549d723b24f5cd6677f7c1102347f979aa4d26483274682",
    "randomize_8_12": "6caa064a89e026000f352b1919b88e0735b67e7c760f752b9e4c23828c6919c0",
}


def F(re, im):
    return np.array([re, im], dtype=np.uint64)


def call2(ob, fn, a, b):
    out = np.zeros(2, dtype=np.uint64)
    getattr(ob.lib(), fn)(a.ctypes.data, b.ctypes.data, out.ctypes.data)
    return tuple(int(x) for x in out)


def call1(ob, fn, a):
    out = np.zeros(2, dtype=np.uint64)
    getattr(ob.lib(), fn)(a.ctypes.data, out.ctypes.data)
    return tuple(int(x) for x in out)


def test_fixture_digests_match_survey(golden):
    from conftest import GOLDEN
    for name, g in golden.items():
        data = open(os.path.join(GOLDEN, g["transcript"]), "rb").read()
        assert hashlib.sha256(data).hexdigest() == g["sha256"]
        if name in SURVEY_SHA256:
            assert g["sha256"] == SURVEY_SHA256[name]
        assert len(data) == g["bytes"]


def test_field_known_answers(ob):
    # values captured from the compiled reference, SURVEY.md §8c
    a = F(1234567890123456789, 987654321987654321)
    b = F(P - 1, 1)
    assert call2(ob, "orc_f_mul", a, b) == (83620797102582841, 246913568135802468)
    assert call2(ob, "orc_f_mul", a, a) == (2249395553658566880, 1358570223080517404)
    assert call1(ob, "orc_f_inv", a) == (665622733565594987, 969236709710989493)
    assert call1(ob, "orc_f_neg", a) == (1071275119090237162, 1318188687226039630)
    assert call1(ob, "orc_f_inv", F(2, 0)) == (1152921504606846976, 0)


def test_roots_of_unity(ob):
    exp = {1: (P - 1, 0), 2: (0, P - 1), 3: (1073741824, 2305843008139952127),
           10: (1311084444718765561, 829995604607609521), 22: (1662087499102352953, 1029856169172585086)}
    for k, v in exp.items():
        out = np.zeros(2, dtype=np.uint64)
        ob.lib().orc_f_root_of_unity(k, out.ctypes.data)
        assert tuple(int(x) for x in out) == v


def test_verifier_random_stream(ob):
    out = np.zeros((3, 2), dtype=np.uint64)
    ob.lib().orc_f_random_seq(3396, 3, out.ctypes.data)
    assert [tuple(int(x) for x in r) for r in out] == [
        (69318801402563806, 1662776802730791352), (1980605035210677997, 152700460719136691),
        (1923425296405918794, 2135854949068199597)]


def test_field_against_python_bigint(ob):
    rng = np.random.default_rng(1)
    edge = [0, 1, 2, P - 1, P - 2, (1 << 60), (1 << 32) - 1, 1 << 32]
    vals = [(int(x), int(y)) for x in edge for y in edge[:4]]
    vals += [(int(rng.integers(0, P)), int(rng.integers(0, P))) for _ in range(200)]
    for (a0, a1), (b0, b1) in zip(vals, vals[7:] + vals[:7]):
        a, b = F(a0, a1), F(b0, b1)
        assert call2(ob, "orc_f_mul", a, b) == ((a0 * b0 - a1 * b1) % P, (a0 * b1 + a1 * b0) % P)
        assert call2(ob, "orc_f_add", a, b) == ((a0 + b0) % P, (a1 + b1) % P)
        assert call2(ob, "orc_f_sub", a, b) == ((a0 - b0) % P, (a1 - b1) % P)


def test_first_messages_x1(gold_gkr):
    # Vres and the first round polynomial of the single-block proof
    t = np.frombuffer(gold_gkr("sha256_x1"), dtype=np.uint64)
    assert tuple(int(x) for x in t[0:2]) == (724662900143931110, 476060367020167324)
    assert tuple(int(x) for x in t[2:8]) == (2211877472072237705, 669034324121346583, 1128696917772413940,
                                              606831994937767933, 2150808768970180659, 1905940033194220355)


@pytest.mark.parametrize("name,blocks", [("sha256_x1", 1), ("sha256_x16", 16), ("sha256_x64", 64)])
def test_oracle_transcript_sha256(ob, golden, gold_gkr, pws_path, name, blocks):
    c = ob.Circuit.from_pws(pws_path, blocks, seed=1)       # glibc's default seed is 1
    g = golden[name]
    assert c.layers == g["layers"] and c.gates == g["gates"]
    assert c.hash() == g["circuit_hash"]
    tr, st = c.prove_gkr()
    assert st["verified"] == 1
    assert tr == gold_gkr(name)
    assert st["mult_count"] == g["mult_counter"] and st["add_count"] == g["add_counter"]
    assert st["rounds"] == g["rounds"]
    assert abs(st["proof_kb"] - g["proof_kb"]) < 1e-9
    c.close()


def test_oracle_transcript_randomize(ob, golden, gold_gkr):
    c = ob.Circuit.randomize(8, 12, seed=1)
    g = golden["randomize_8_12"]
    assert c.hash() == g["circuit_hash"]
    tr, st = c.prove_gkr()
    assert st["verified"] == 1 and tr == gold_gkr("randomize_8_12")
    assert (st["mult_count"], st["add_count"], st["rounds"]) == (g["mult_counter"], g["add_counter"], g["rounds"])
    c.close()


# ---- Virgo polynomial commitment, commit side (oracle/vp_oracle.cpp second half) ---------------------------------
def test_oracle_sha3_is_fips202(ob):
    rng = np.random.default_rng(3)
    L = ob.lib()
    L.orc_sha3_256_64.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    msgs = [bytes(64), bytes(range(64)), b"\xff" * 64] + [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(50)]
    for m in msgs:
        out = ctypes.create_string_buffer(32)
        L.orc_sha3_256_64(m, out)
        assert out.raw == hashlib.sha3_256(m).digest()
    # my_hhash(64 zero bytes) as computed by the compiled reference (libXKCP)
    assert hashlib.sha3_256(bytes(64)).hexdigest() == "070fa1ab6fcc557ed14d42941f1967693048551eb9042a8d0a057afbd75e81e0"


def test_oracle_fft_known_answer_and_round_trip(ob):
    L = ob.lib()
    L.orc_fft.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.orc_ifft.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    c = np.array([[i + 1, 2 * i + 3] for i in range(8)], dtype=np.uint64)
    o = np.zeros((32, 2), dtype=np.uint64)
    L.orc_fft(c.ctypes.data, 8, 32, o.ctypes.data)              # values from the compiled reference, SURVEY.md §8c
    assert tuple(int(x) for x in o[0]) == (36, 80)
    assert tuple(int(x) for x in o[1]) == (617377187976651873, 1655836513184006865)
    assert tuple(int(x) for x in o[31]) == (107673715198561662, 1973828267175406033)
    rng = np.random.default_rng(9)
    x = rng.integers(0, P, size=(64, 2), dtype=np.uint64)
    e = np.zeros_like(x); back = np.zeros_like(x)
    L.orc_fft(x.ctypes.data, 64, 64, e.ctypes.data)
    L.orc_ifft(e.ctypes.data, 64, back.ctypes.data)
    assert np.array_equal(back, x)
    # definition check on a small size: out[k] = sum_j c_j w^(jk)
    w = np.zeros(2, dtype=np.uint64); L.orc_f_root_of_unity(3, w.ctypes.data)
    def fmul(a, b): return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)
    o8 = np.zeros((8, 2), dtype=np.uint64)
    L.orc_fft(c.ctypes.data, 8, 8, o8.ctypes.data)
    wk = (1, 0)
    for k in range(8):
        acc, p = (0, 0), (1, 0)
        for j in range(8):
            t = fmul((int(c[j][0]), int(c[j][1])), p)
            acc = ((acc[0] + t[0]) % P, (acc[1] + t[1]) % P)
            p = fmul(p, wk)
        assert tuple(int(v) for v in o8[k]) == acc
        wk = fmul(wk, (int(w[0]), int(w[1])))


@pytest.mark.parametrize("name,blocks", [("sha256_x1", 1), ("sha256_x16", 16)])
def test_oracle_commit_private_root(ob, golden, pws_path, name, blocks):
    from conftest import GOLDEN
    L = ob.lib()
    L.orc_commit_private.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    c = ob.Circuit.from_pws(pws_path, blocks, seed=1)
    r = ctypes.create_string_buffer(32)
    assert L.orc_commit_private(c.h, r) == 0
    assert r.raw == open(os.path.join(GOLDEN, golden[name]["transcript"]), "rb").read()[:32]
    if blocks == 1:
        assert r.raw.hex() == "b8b3a141ac9144df9ff7f837784044d9832101b76a72de58a92d359918586efc"
    c.close()


def test_oracle_commit_private_root_randomize(ob, golden):
    from conftest import GOLDEN
    L = ob.lib()
    L.orc_commit_private.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    c = ob.Circuit.randomize(8, 12, seed=1)
    r = ctypes.create_string_buffer(32)
    assert L.orc_commit_private(c.h, r) == 0
    assert r.raw == open(os.path.join(GOLDEN, golden["randomize_8_12"]["transcript"]), "rb").read()[:32]
    c.close()


def _fri_case(ob, golden, name, c):
    """Oracle full proof + FRI commit phase against the real reference's recorded FRI steps."""
    from conftest import GOLDEN
    L = ob.lib()
    L.orc_fri_commit.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.orc_prove_full.restype = ctypes.c_int64
    L.orc_prove_full.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.orc_last_point.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    g = golden[name]
    buf = ctypes.create_string_buffer(1 << 20)
    n = L.orc_prove_full(c.h, buf, len(buf), None)
    gold = open(os.path.join(GOLDEN, g["transcript"]), "rb").read()
    assert buf.raw[:n] == gold and hashlib.sha256(buf.raw[:n]).hexdigest() == SURVEY_SHA256[name]
    nb = L.orc_circuit_layer_bitlen(c.h, 0)
    pt = np.zeros((nb, 2), np.uint64)
    assert L.orc_last_point(c.h, pt.ctypes.data, nb) == 0
    one = np.array([1, 0], np.uint64)
    pub = np.zeros((1 << nb, 2), np.uint64)
    L.orc_beta_table(pt.ctypes.data, nb, one.ctypes.data, pub.ctypes.data)
    inp = np.zeros((1 << nb, 2), np.uint64)
    L.orc_circuit_inputs(c.h, inp.ctypes.data)
    fri = open(os.path.join(GOLDEN, g["fri"]), "rb").read()
    st = g["fri_steps"]
    assert st == nb - 6
    rec = np.frombuffer(fri[:48 * st], dtype=np.uint64).reshape(st, 6)
    r = np.ascontiguousarray(rec[:, :2])
    # The reference's FRI challenges are the verifier's NEXT draws after the ones fft_gkr consumes (vpd_verifier.cpp:92,56):
    # continuing the glibc stream where orc_prove_full left it must reproduce the recorded challenges.
    L.orc_f_random_next.argtypes = [ctypes.c_int, ctypes.c_void_p]
    skip = L.orc_fft_gkr_draws(nb - 6)
    assert skip == 2 * (nb - 6) ** 2 + 9 * (nb - 6) + 96
    nxt = np.zeros((skip + st, 2), np.uint64)
    L.orc_f_random_next(skip + st, nxt.ctypes.data)
    assert np.array_equal(nxt[skip:], r), "fft_gkr draw count does not lead to the reference's FRI challenges"
    roots = ctypes.create_string_buffer(32 * st)
    fin = np.zeros((2048, 2), np.uint64)
    assert L.orc_fri_commit(inp.ctypes.data, pub.ctypes.data, nb, r.ctypes.data, roots, fin.ctypes.data) == 0
    assert roots.raw == b"".join(rec[i, 2:].tobytes() for i in range(st))
    assert np.array_equal(fin, np.frombuffer(fri[48 * st:48 * st + 2048 * 16], dtype=np.uint64).reshape(2048, 2))
    assert not np.frombuffer(fri[48 * st + 2048 * 16:], dtype=np.uint64).any()      # mask codeword is zero


def test_oracle_full_transcript_and_fri_x1(ob, golden, pws_path):
    c = ob.Circuit.from_pws(pws_path, 1, seed=1)
    _fri_case(ob, golden, "sha256_x1", c)
    c.close()


def test_oracle_full_transcript_and_fri_randomize(ob, golden):
    c = ob.Circuit.randomize(8, 12, seed=1)
    _fri_case(ob, golden, "randomize_8_12", c)
    c.close()


def test_oracle_commitment_array_vs_reference_x1(ob, golden, pws_path):
    """orc_commitment_array (commit_private, commit_public and the FRI commit phase on caller-supplied arrays, in one pass) on sha256_x1's input layer, the eq
    table of its opening point and the challenges the real reference recorded: every output is what the reference's golden transcript and FRI record hold."""
    import pc_array_inputs as pai
    from conftest import GOLDEN
    L = ob.lib()
    L.orc_prove_full.restype = ctypes.c_int64
    L.orc_prove_full.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.orc_last_point.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    g = golden["sha256_x1"]
    gold = open(os.path.join(GOLDEN, g["transcript"]), "rb").read()
    fri = open(os.path.join(GOLDEN, g["fri"]), "rb").read()
    c = ob.Circuit.from_pws(pws_path, 1, seed=1)
    buf = ctypes.create_string_buffer(1 << 20)
    assert L.orc_prove_full(c.h, buf, len(buf), None) == len(gold)           # (leaves the opening point behind)
    nb = L.orc_circuit_layer_bitlen(c.h, 0)
    st = g["fri_steps"]
    assert st == nb - 6
    pt = np.zeros((nb, 2), np.uint64)
    assert L.orc_last_point(c.h, pt.ctypes.data, nb) == 0
    one = np.array([1, 0], np.uint64)
    pub = np.zeros((1 << nb, 2), np.uint64)
    L.orc_beta_table(pt.ctypes.data, nb, one.ctypes.data, pub.ctypes.data)
    inp = np.zeros((1 << nb, 2), np.uint64)
    L.orc_circuit_inputs(c.h, inp.ctypes.data)
    rec = np.frombuffer(fri[:48 * st], dtype=np.uint64).reshape(st, 6)
    r = np.ascontiguousarray(rec[:, :2])
    assert c.layer_size(0) < 1 << nb                                         # the inner product stops before the padding
    out = pai.split_record(pai.oracle_record(L, inp, c.layer_size(0), pub, nb, r), nb)
    tail = 16 + 65 * 16
    assert out["root_l"] == gold[:32]
    assert out["root_h"] == gold[-tail - 32:-tail]
    assert out["public"] == gold[-tail:]                                     # input_0 | all_sum[65]
    assert out["roots"] == [rec[k, 2:].tobytes() for k in range(st)]
    assert out["final"] == fri[48 * st:48 * st + 2048 * 16]
    c.close()


@pytest.mark.parametrize("name", ["custom_a", "custom_b", "custom_c", "custom_d"])
def test_oracle_on_all_gate_types_and_asserts_vs_reference(ob, golden, name):
    """Circuits using every gate type + assert gates, proved by the REAL reference (ref_run --custom): the oracle must
    reproduce transcript, field-op counters, commitment and FRI data.  custom_c is the skewed circuit of custom_circuits.make_skewed
    (heavy rows of up to 33000 gates, subsets of bit length 14, two assert gates per layer); custom_d is custom_circuits.make_unary_mid
    (a layer of unary gates only, so no phase 2 there, and assert flags on a Copy and a Mulc gate)."""
    import custom_circuits as cc
    g = golden[name]
    c = ob.Circuit.custom(*cc.from_golden(g["custom"]))
    assert c.hash() == g["circuit_hash"]
    tr, st = c.prove_gkr()
    from conftest import GOLDEN
    gold = open(os.path.join(GOLDEN, g["transcript"]), "rb").read()
    assert tr == gold[g["gkr_slice"][0]:g["gkr_slice"][1]]
    assert (st["mult_count"], st["add_count"], st["rounds"]) == (g["mult_counter"], g["add_counter"], g["rounds"])
    # full transcript + FRI (reuses the helper above without the SURVEY digest table)
    L = ob.lib()
    L.orc_prove_full.restype = ctypes.c_int64
    L.orc_prove_full.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    buf = ctypes.create_string_buffer(1 << 20)
    n = L.orc_prove_full(c.h, buf, len(buf), None)
    assert buf.raw[:n] == gold and hashlib.sha256(gold).hexdigest() == g["sha256"]
    c.close()


def test_oracle_fiat_shamir_proof_equals_the_committed_device_proof(ob):
    """Second opinion for the Fiat-Shamir mode: tests/golden/fs_proof_randomize_6_8_seed5.bin was produced on the GPU box by
    the product (host/verifier.cpp::proveFS driving vp_round).  The oracle derives the same challenges with its OWN SHA3 sponge, its own
    statement serialiser and its own CPU prover (orc_prove_fs) and must arrive at the same 5 936 proof bytes — challenges and messages
    are interlocked, so one differing challenge or one differing field element anywhere changes everything after it."""
    from conftest import GOLDEN
    c = ob.Circuit.randomize(6, 8, seed=5)
    proof, st = c.prove_fs()
    assert st["verified"] == 1
    assert proof == open(os.path.join(GOLDEN, "fs_proof_randomize_6_8_seed5.bin"), "rb").read()
    tr, _ = c.prove_gkr()
    assert len(tr) == len(proof) and tr != proof            # same layout, other challenges (random() instead of the hash chain)
    c.close()
    other = ob.Circuit.randomize(6, 8, seed=6)              # another witness: another statement digest, other challenges from the start
    p2, _ = other.prove_fs()
    assert p2 != proof and p2[:16] != proof[:16]
    other.close()


@pytest.mark.parametrize("name", ["sha256_x1024", "randomize_16_20"])
def test_full_size_oracle_fixtures_equal_the_real_reference(golden, name):
    """BASELINE configs[2]/[3] and [4] were pinned through the oracle port in rounds 1-2 (fixtures made by the oracle on the GPU box's host);
    round 3 ran the REAL reference at those sizes in the build container (x1024 with the commitment: 183 s + 576 s, 63 GB).  The
    oracle's fixtures must be byte-identical to the reference's records wherever they overlap — GKR slice, both Merkle roots, input_0,
    all_sum, the FRI challenges the reference's verifier drew (after fft_gkr's draws), all FRI roots, the final codeword — and the
    oracle's 64-bit field-op counts must be what the reference's wrapping `int` counters printed (mod 2^32)."""
    from conftest import GOLDEN
    g = golden[name]
    assert g["origin"].startswith("real reference")
    ref = open(os.path.join(GOLDEN, g["transcript"]), "rb").read()
    assert len(ref) == g["bytes"] and hashlib.sha256(ref).hexdigest() == g["sha256"]
    orc = open(os.path.join(GOLDEN, g["oracle_fixture"]["transcript"]), "rb").read()
    assert hashlib.sha256(orc).hexdigest() == g["oracle_fixture"]["sha256"]
    assert ref[g["gkr_slice"][0]:g["gkr_slice"][1]] == orc
    fri = open(os.path.join(GOLDEN, g["fri"]), "rb").read()
    st = g["fri_steps"]
    assert len(fri) == 48 * st + (2048 + 32) * 16 and hashlib.sha256(fri).hexdigest() == g["fri_sha256"]
    if name == "sha256_x1024":
        assert (g["mult_counter"] - g["mult_counter_printed_int32"]) % (1 << 32) == 0 and g["mult_counter"] > 1 << 31
        assert (g["add_counter"] - g["add_counter_printed_int32"]) % (1 << 32) == 0
        full = open(os.path.join(GOLDEN, "oracle_sha256_x1024_full.bin"), "rb").read()     # the oracle's run of the COMPLETE protocol
        n = len(ref)
        assert full[:n] == ref
        roots, fin, ch = full[n:n + 32 * st], full[n + 32 * st:n + 32 * st + 2048 * 16], full[n + 32 * st + 2048 * 16:]
        assert b"".join(fri[48 * k:48 * k + 16] for k in range(st)) == ch
        assert b"".join(fri[48 * k + 16:48 * k + 48] for k in range(st)) == roots
        assert fri[48 * st:48 * st + 2048 * 16] == fin
        pc = open(os.path.join(GOLDEN, "oracle_sha256_x1024_pc.bin"), "rb").read()
        assert pc[:32] == ref[:32]                                                       # merkle_root_l (the rest used another public vector)


def _orc_fft_gkr(ob, lg, seed):
    L = ob.lib()
    L.orc_fft_gkr.restype = ctypes.c_int64
    L.orc_fft_gkr.argtypes = [ctypes.c_int, ctypes.c_long, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    buf = ctypes.create_string_buffer(1 << 20)
    ok = ctypes.c_int(0)
    n = L.orc_fft_gkr(lg, seed, buf, len(buf), None, ctypes.byref(ok))
    assert n > 0
    return buf.raw[:n], ok.value


@pytest.mark.parametrize("lg", [7, 13, 17])
def test_oracle_fft_gkr_vs_reference_record(ob, lg):
    """lib/virgo's fft_gkr (fft_circuit_GKR.cpp:22-849) restated in the oracle (orc_fft_gkr) against the REAL reference's
    record of the same call — `ref_run --fft-gkr LG --dump-fft` after F::init(): the circuit's 64 outputs, every round polynomial of the
    2 + 2 lg sumchecks and every claimed table value, taken at link time (ld --wrap on quadratic_poly::eval / linear_poly::eval, no
    reference line edited).  lg = 7 / 13 / 17 are the sizes of the x1 / x64 / x1024 SHA-256 commitments."""
    from conftest import GOLDEN
    rec, ok = _orc_fft_gkr(ob, lg, 3396)
    assert ok == 1
    assert len(rec) == 16 * (64 + 3 * (2 * lg * lg + 2 * lg + 6) + 2 + 2 * lg)
    assert rec == open(os.path.join(GOLDEN, "fftgkr_lg%d.bin" % lg), "rb").read()


@pytest.mark.parametrize("lg", [7, 13])
def test_oracle_fft_gkr_on_a_tape_vs_reference_record(ob, lg):
    """orc_fft_gkr_tape (the same prover with its draws taken from the caller's tape) fed the reference's own draw sequence: the real reference's record.
    (lg 17 and the entry's other properties: tests/test_fft_gkr_host.py.)"""
    from conftest import GOLDEN
    rec, ok = ob.fft_gkr_tape(lg, ob.random_seq(3396, ob.lib().orc_fft_gkr_draws(lg)))
    assert ok == 1 and rec == open(os.path.join(GOLDEN, "fftgkr_lg%d.bin" % lg), "rb").read()


def test_oracle_fft_gkr_on_the_protocols_own_draws(ob, golden):
    """... and fed the draws the stream holds where the reference's complete run calls fft_gkr (after commit_public): its record from inside that run."""
    from conftest import GOLDEN
    c = ob.Circuit.randomize(8, 12, seed=1)
    L = ob.lib()
    L.orc_prove_full.restype = ctypes.c_int64
    L.orc_prove_full.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    buf = ctypes.create_string_buffer(1 << 20)
    n = L.orc_prove_full(c.h, buf, len(buf), None)
    assert buf.raw[:n] == open(os.path.join(GOLDEN, golden["randomize_8_12"]["transcript"]), "rb").read()
    L.orc_f_random_next.argtypes = [ctypes.c_int, ctypes.c_void_p]
    tape = np.zeros((L.orc_fft_gkr_draws(6), 2), dtype=np.uint64)
    L.orc_f_random_next(tape.shape[0], tape.ctypes.data)
    rec, ok = ob.fft_gkr_tape(6, tape)
    assert ok == 1 and rec == open(os.path.join(GOLDEN, "fftgkr_randomize_8_12.bin"), "rb").read()
    c.close()


@pytest.mark.parametrize("name,lg", [("sha256_x1", 7), ("randomize_8_12", 6)])
def test_oracle_fft_gkr_inside_the_protocol(ob, golden, pws_path, name, lg):
    """The same record taken INSIDE the reference's complete run (verify_poly_commitment, vpd_verifier.cpp:92): the oracle proves up to
    commit_public and then runs fft_gkr from wherever the glibc stream stands — equality pins the stream position too (the draw-count
    replay of round 2, 2 lg^2 + 9 lg + 96 draws, is now a consequence)."""
    from conftest import GOLDEN
    c = ob.Circuit.from_pws(pws_path, 1, seed=1) if name == "sha256_x1" else ob.Circuit.randomize(8, 12, seed=1)
    L = ob.lib()
    L.orc_prove_full.restype = ctypes.c_int64
    L.orc_prove_full.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    buf = ctypes.create_string_buffer(1 << 20)
    n = L.orc_prove_full(c.h, buf, len(buf), None)
    assert buf.raw[:n] == open(os.path.join(GOLDEN, golden[name]["transcript"]), "rb").read()
    rec, ok = _orc_fft_gkr(ob, lg, -1)
    assert ok == 1 and rec == open(os.path.join(GOLDEN, "fftgkr_%s.bin" % name), "rb").read()
    # ... and the FRI challenges the reference drew next are the next draws of the stream
    L.orc_f_random_next.argtypes = [ctypes.c_int, ctypes.c_void_p]
    st = golden[name]["fri_steps"]
    nxt = np.zeros((st, 2), dtype=np.uint64)
    L.orc_f_random_next(st, nxt.ctypes.data)
    fri = open(os.path.join(GOLDEN, golden[name]["fri"]), "rb").read()
    assert nxt.tobytes() == b"".join(fri[48 * k:48 * k + 16] for k in range(st))
    c.close()


def test_masked_commitment_goldens_are_the_recorded_files():
    """tests/golden/pc_masked_*.bin (the REAL reference's commit_private_array / commit_public_array / commit_phase with non-zero masks, make_pc_masked.py): the files are
    the ones the index was written for, the inputs regenerate deterministically, and the record has the layout the GPU test walks."""
    import hashlib
    import json
    import pc_masked_inputs as pmi
    from conftest import GOLDEN
    meta = json.load(open(os.path.join(GOLDEN, "pc_masked.json")))
    assert set(meta) == set(pmi.CASES)
    for name, m in meta.items():
        rec = open(os.path.join(GOLDEN, m["record"]), "rb").read()
        fri = open(os.path.join(GOLDEN, m["fri"]), "rb").read()
        assert hashlib.sha256(rec).hexdigest() == m["record_sha256"] and hashlib.sha256(fri).hexdigest() == m["fri_sha256"]
        assert len(rec) == 64 + 65 * 16 + 8 * 130 * 16 and len(fri) == 48 * m["fri_steps"] + 2048 * 16 + 32 * 16
        x = pmi.inputs(name)
        assert x["values"].shape == (1 << m["n"], 2) and x["pri_mask"].shape == (m["m"], 2) and int(x["values"].max()) < (1 << 61) - 1
        M = 1 << (m["n"] - 1)
        assert M % m["mask_position_gap"] == 0
        if name.endswith("_zero"):
            assert fri[-32 * 16:] == bytes(32 * 16) and rec[64 + 64 * 16:64 + 65 * 16] == bytes(16)          # zero mask: all_sum[64] = 0, mask codeword 0
        else:
            assert fri[-32 * 16:] != bytes(32 * 16) and rec[64 + 64 * 16:64 + 65 * 16] != bytes(16)


def test_commitment_array_goldens_are_the_recorded_files():
    """tests/golden/pc_array_n18.bin / _n20.bin (the oracle's orc_commitment_array on the uniform input set, make_pc_array.py): the files are the ones the index
    was written for, they have the record's layout, and the inputs the GPU test regenerates are the ones they were recorded with."""
    import json
    import pc_array_inputs as pai
    from conftest import GOLDEN
    meta = json.load(open(os.path.join(GOLDEN, "pc_array.json")))
    assert sorted(meta) == ["n18", "n20"]
    for m in meta.values():
        rec = open(os.path.join(GOLDEN, m["record"]), "rb").read()
        assert hashlib.sha256(rec).hexdigest() == m["record_sha256"] and len(rec) == pai.record_bytes(m["n"])
        assert m["seed"] == pai.seed_of(m["set"], m["n"])
        x = pai.inputs(m["set"], m["n"], seed=m["seed"])
        assert x["n_used"] == m["n_used"] == (1 << m["n"]) - 3
        for k, v in pai.digests(x).items():
            assert m[k] == v, "input generator differs: " + k
        f = pai.split_record(rec, m["n"])
        assert len(set(f["roots"] + [f["root_l"], f["root_h"]])) == m["n"] - 4 and f["public"][-16:] == bytes(16)      # all_sum[64]: the zero mask


def test_commitment_array_input_sets_have_their_edges():
    """the three input sets of the commitment ladder are what its cases name: canonical limbs, the unused tail, the all-zero slices, the five-wire witness"""
    import pc_array_inputs as pai
    for n in (7, 12):
        sl = 1 << (n - 6)
        a, b, c = (pai.inputs(k, n) for k in pai.SETS)
        assert a["n_used"] == (1 << n) - 3 and not a["values"][-3:].any() and a["values"][-4].any() and a["values"][:, 1].any()
        assert b["n_used"] == 1 << n and set(np.unique(b["values"])) <= set(pai.EDGES) and set(np.unique(b["pub"])) <= set(pai.EDGES)
        assert not b["values"][5 * sl:6 * sl].any() and not b["values"][63 * sl:].any() and not b["pub"][7 * sl:8 * sl].any() and not b["pub"][0].any()
        assert b["values"][4 * sl:5 * sl].any() and b["values"][62 * sl:63 * sl].any() and b["pub"][6 * sl:7 * sl].any()
        assert c["n_used"] == 5 and c["values"][:5, 0].all() and not c["values"][5:].any() and not c["values"][:, 1].any()
        for x in (a, b, c):
            assert x["r"].shape == (n - 6, 2) and int(max(x["values"].max(), x["pub"].max(), x["r"].max())) < pai.P61


@pytest.mark.parametrize("name", ["n13_m5", "n13_m64", "n16_m100", "n13_m300", "n13_m2000"])
def test_reference_verifier_on_the_references_own_masked_commitments(name, tmp_path):
    """Pins what `accepted` means for the mask slice: the reference's own verify_poly_commitment (vpd_verifier.cpp:76-328) on the reference's own
    commit_private_array / commit_public_array with the masks of the goldens (oracle/_ref/ref_run --pc-masked IN --verify).  Masks up to a slice's message length are
    accepted; longer ones — which the reference's prover commits without complaint, and which the device reproduces byte for byte — are REJECTED by its own verifier
    at the last check (the mask slice's final codeword is not constant).  The GPU suite asks the same verdicts of the device prover."""
    import subprocess
    import pc_masked_inputs as pmi
    from conftest import ROOT
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_run")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_run not built (needs the reference tree at build time)")
    inp = tmp_path / "in.bin"
    pmi.write_case_file(name, str(inp))
    r = subprocess.run([exe, "--pc-masked", str(inp), "--verify"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    want = pmi.REFERENCE_VERIFIER_ACCEPTS[name]
    assert ("verify_poly_commitment ACCEPT" in r.stdout) == want and ("verify_poly_commitment REJECT" in r.stdout) == (not want), (r.stdout[-400:], r.stderr[-400:])
    assert r.returncode == (0 if want else 1)
    if not want:
        assert "Fri msk rs code check fail" in r.stderr


# ---- the GKR prover on a caller's tape (orc_prove_gkr_tape): the entry tests/test_gpu_gkr_tapes.py takes its expected bytes from ---------------------------
def _gkr_tape_circuits(ob, golden, pws_path):
    import custom_circuits as cc
    yield "sha256_x1", ob.Circuit.from_pws(pws_path, 1, seed=1)
    yield "randomize_8_12", ob.Circuit.randomize(8, 12, seed=1)
    for name in ("custom_a", "custom_b", "custom_c", "custom_d"):
        yield name, ob.Circuit.custom(*cc.from_golden(golden[name]["custom"]))


def test_oracle_gkr_on_the_seeded_tape_vs_reference_records(ob, golden, gold_gkr, pws_path):
    """Fed the draws of F::init()'s stream, orc_prove_gkr_tape returns the REAL reference's recorded GKR slice (and with it orc_prove_gkr's bytes), consuming
    exactly orc_gkr_draws elements — the layout of include/vpgpu.h: r_0, then per layer r_u[max_bl], assert_random, r_v, sig[n_layers], r_liu[max_bl].  Another
    seed gives other bytes."""
    for name, c in _gkr_tape_circuits(ob, golden, pws_path):
        n = c.gkr_draws()
        bl = [c.layer_bitlen(i) for i in range(c.layers)]
        assert n == bl[-1] + sum(2 * max(bl) + 1 + c.layers + max(0, c.subsets(i)[2]) for i in range(1, c.layers)), name
        tr, st = c.prove_gkr_tape(ob.random_seq(3396, n))
        assert st["verified"] == 1 and tr == gold_gkr(name), name
        if name in ("randomize_8_12", "custom_d"):
            assert (tr, 1) == (c.prove_gkr()[0], c.prove_gkr()[1]["verified"])
            other, st = c.prove_gkr_tape(ob.random_seq(77, n))
            assert st["verified"] == 1 and other != tr and len(other) == len(tr)
        c.close()


def test_oracle_gkr_tape_refusals_and_dont_care_draws(ob):
    import custom_circuits as cc
    P = (1 << 61) - 1
    c = ob.Circuit.custom(*cc.make(4, [5, 3, 2, 1]))            # bit lengths 3, 2, 1, 0: every r_u and r_liu vector has drawn entries nobody reads
    n, max_bl, layers = c.gkr_draws(), 3, 4
    t = ob.random_seq(3396, n)
    full = len(c.prove_gkr()[0])
    assert c.prove_gkr_tape_rc(t)[0] == full
    assert c.prove_gkr_tape_rc(t, n_tape=n - 1)[0] == -3 and c.prove_gkr_tape_rc(np.concatenate([t, t[:1]]))[0] == -3      # a short count, a long count
    assert ob.lib().orc_prove_gkr_tape(c.h, None, n, None, 0, None) == -3
    assert c.prove_gkr_tape_rc(t, capacity=full - 1)[0] == -1 and c.prove_gkr_tape_rc(t, capacity=full)[0] == full
    dont_care = c.layer_bitlen(3) + c.layer_bitlen(2)          # the first entry of r_u past the bit length of layer 2 (1 < max_bl = 3): drawn, never read
    assert c.layer_bitlen(2) < max_bl
    for at, limb, v in ((0, 0, P), (n - 1, 1, P), (n // 2, 0, 2 ** 64 - 1), (dont_care, 1, P)):       # a don't-care position is checked too
        bad = t.copy()
        bad[at, limb] = v
        assert c.prove_gkr_tape_rc(bad)[0] == -4
        bad[at, limb] = P - 1
        assert c.prove_gkr_tape_rc(bad)[0] == full
    # draws the prover never reads (r_u / r_liu past bit_length(i - 1), sig past n_layers - i + 1) do not move a byte; a draw it reads does
    want = c.prove_gkr_tape(t)[0]
    moved = t.copy()
    at = c.layer_bitlen(3)
    for i in range(layers - 1, 0, -1):
        used = c.layer_bitlen(i - 1)
        moved[at + used:at + max_bl] = [5, 7]; at += max_bl + 1 + max(0, c.subsets(i)[2])
        moved[at + layers - i + 1:at + layers] = [P - 1, P - 1]; at += layers
        moved[at + used:at + max_bl] = [0, 1]; at += max_bl
    assert at == n and (moved != t).any() and c.prove_gkr_tape(moved)[0] == want
    moved[n - max_bl + c.layer_bitlen(0) - 1, 0] ^= 1          # the last challenge of the last Liu sumcheck: only the closing claim follows it
    got = c.prove_gkr_tape(moved)[0]
    assert got != want and got[:-16] == want[:-16]
    c.close()


# ---- the oracle's masked commitment (orc_commitment_array_masked) against the REAL reference ------------------------------------------------------------------

def _masked_oracle_vs_record(ob, n, values, pub, pri_mask, pub_mask, rec, fri):
    """orc_commitment_array_masked_open on the reference's own challenges (read from its FRI record) against a `--dump` / `--dump-fri` pair of
    `ref_run --pc-masked`: both roots, all_sum[65], the eight openings (3 leaves of l, 3 of h, leaf 3 of FRI levels 0 and 2; 65 pairs each), every FRI root, the
    final codeword and the mask slice's final codeword, byte for byte"""
    import pc_masked_inputs as pmi
    st, M = n - 6, 1 << (n - 1)
    assert len(rec) == 64 + 65 * 16 + 8 * 130 * 16 and len(fri) == 48 * st + 2048 * 16 + 32 * 16
    r = np.frombuffer(b"".join(fri[48 * k:48 * k + 16] for k in range(st)), dtype=np.uint64).reshape(st, 2).copy()
    opens = [(0, 0), (0, 5), (0, M // 2 - 1), (1, 0), (1, 5), (1, M // 2 - 1), (2, 3), (4, 3)]
    got, vals = pmi.oracle_masked(ob.lib(), values, 1 << n, pub, n, r, pri_mask, pub_mask, opens)
    f = pmi.split_masked_record(got, n)
    assert f["root_l"] == rec[:32], "merkle_root_l"
    assert f["root_h"] == rec[32:64], "merkle_root_h"
    assert f["public"][16:] == rec[64:64 + 65 * 16], "all_sum[65]"
    for i, (o, lf) in enumerate(opens):
        assert vals[i].tobytes() == rec[64 + 65 * 16 + 130 * 16 * i:64 + 65 * 16 + 130 * 16 * (i + 1)], "opening of oracle %d at leaf %d" % (o, lf)
    for k in range(st):
        assert f["roots"][k] == fri[48 * k + 16:48 * k + 48], "FRI root %d" % k
    assert f["final"] == fri[48 * st:48 * st + 2048 * 16], "final codeword"
    assert f["final_mask"] == fri[48 * st + 2048 * 16:], "final mask codeword"


@pytest.mark.parametrize("name", ["n13_zero", "n13_m5", "n13_m64", "n16_m100", "n19_m3000", "n13_m300", "n13_m2000", "n13_m128", "n13_m100_p37", "n13_m200", "n13_m1000"])
def test_masked_oracle_reproduces_the_real_references_records(ob, name):
    """All eleven records of the real reference's commitment with masks (tests/golden/pc_masked_*.bin): ms = 8, 64, 128 (= N), 512, 2048 at n = 13, 128 at
    n = 16, 4096 at n = 19; 2, 4, 8 and 16 blocks of a slice's message; a public mask of 37 elements under a private one of 100.  n13_zero is the protocol's
    one-element zero mask, which the entry refuses as the device does (it pads to one element): there the entry gets eight zeros, the same polynomial, and
    orc_commitment_array — the same code on the one-element zero masks — must return the same bytes."""
    import json
    import pc_array_inputs as pai
    import pc_masked_inputs as pmi
    from conftest import GOLDEN
    m = json.load(open(os.path.join(GOLDEN, "pc_masked.json")))[name]
    x = pmi.inputs(name)
    n = x["n"]
    assert m.get("n_pub", x["m"]) == x["n_pub"] and not x["pub_mask"][x["n_pub"]:].any()
    rec, fri = open(os.path.join(GOLDEN, m["record"]), "rb").read(), open(os.path.join(GOLDEN, m["fri"]), "rb").read()
    pm, qm = x["pri_mask"], x["pub_mask"][:x["n_pub"]]
    if name == "n13_zero":
        assert pmi.oracle_masked_rc(ob.lib(), x["values"], 1 << n, x["pub"], n, np.zeros((n - 6, 2), np.uint64), pm, qm)[0] == -1
        pm = qm = np.zeros((8, 2), np.uint64)
        st = n - 6
        r = np.frombuffer(b"".join(fri[48 * k:48 * k + 16] for k in range(st)), dtype=np.uint64).reshape(st, 2).copy()
        f = pai.split_record(pai.oracle_record(ob.lib(), x["values"], 1 << n, x["pub"], n, r), n)
        assert (f["root_l"], f["root_h"], f["public"][16:]) == (rec[:32], rec[32:64], rec[64:64 + 65 * 16])
        assert b"".join(f["roots"]) == b"".join(fri[48 * k + 16:48 * k + 48] for k in range(st)) and f["final"] == fri[48 * st:48 * st + 2048 * 16]
    _masked_oracle_vs_record(ob, n, x["values"], x["pub"], pm, qm, rec, fri)


@pytest.mark.parametrize("fam,ms", [("uniform", 8), ("edges", 16), ("short_pub", 32), ("one_hot", 64), ("pub_zero", 128), ("edges", 256)])
@pytest.mark.parametrize("n", [10, 11])
def test_masked_oracle_vs_the_real_reference_live(ob, tmp_path, n, fam, ms):
    """Where oracle/_ref/ref_run exists: the oracle against `ref_run --pc-masked` on the mask families at n = 10 and 11 (slices of 16 and 32 elements: every
    transform of the reference has at least the 8 points below which it reads stale scratch, tests/pc_masked_inputs.py).  The reference's output there is a
    function of its inputs — run twice here, equal bytes asserted — so both lengths stay."""
    import subprocess
    import pc_array_inputs as pai
    import pc_masked_inputs as pmi
    from conftest import ROOT
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_run")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_run not built (needs the reference tree at build time)")
    x, f = pai.inputs("uniform", n), pmi.family(fam, n, ms)
    inp = str(tmp_path / "in.bin")
    pmi.write_in_file(inp, n, x["values"], x["pub"], f["pri_mask"], f["pub_mask"])
    runs = []
    for k in range(2):
        rec, fri = str(tmp_path / ("rec%d.bin" % k)), str(tmp_path / ("fri%d.bin" % k))
        subprocess.run([exe, "--pc-masked", inp, "--dump", rec, "--dump-fri", fri], stdout=subprocess.PIPE, check=True, timeout=600)
        runs.append((open(rec, "rb").read(), open(fri, "rb").read()))
    assert runs[0] == runs[1], "the reference's masked commitment is not a function of its inputs here"
    _masked_oracle_vs_record(ob, n, x["values"], x["pub"], f["pri_mask"], f["pub_mask"], *runs[0])
