"""CPU: the proof of work of the non-interactive proofs (host/vphost.h, "The proof of work") without a device.  The reference is tests/fs_pow_ref.py: the
step and the smallest-nonce search with hashlib, version-2 proofs assembled from the oracle alone.

  search       vph_fs_grind_host equals the hashlib search for bits 1 .. 12 on eight states (all zero and all 0xff among them); first = found + 1 gives the
               next hit; max_tries = h - first is exhausted and h - first + 1 finds h; the range rule at 2^64; the refusals
  commitment   version-2 proofs at n = 9, 10, the zero mask and ms = 8, pow_bits 8 and 12: accepted; positions differ from the version-1 proof of the same
               commitment; vph_commitment_fs_challenges equals the Python derivation; vph_fs_pow reads the pair
  rejected     a nonce hashlib says fails (the reason names the work), pow_bits changed with the nonce kept, min_pow_bits = pow_bits + 1, a version-1 proof under
               min_pow_bits = 1 — each verdict predicted with hashlib first, each proof answered honestly at the positions it derives, so that nothing but the
               work can reject it
  malformed    version 2 with pow_bits 0, 49, 2^63; 47 header bytes; a version-1 body under a version-2 header
  joined       one version-2 proof on the circuit of tests/golden/full_fs_rand3_7.* at pow_bits = 8: accepted; a failing nonce rejected, naming the work;
               rejected under min_pow_bits = 9
  symbols      declared in both headers, exported; vp_options still twelve fields
  sanitizers   tests/sanitize/fs_pow_main.cpp under ASan / UBSan as a stand-alone program"""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fs_pow_ref as pw
import full_fs_ref as ff
import pc_fs_ref as fs
from conftest import ROOT

REPS = 5
STATES = [bytes(32), b"\xff" * 32] + [bytes(np.random.default_rng(4100 + i).integers(0, 256, 32, dtype=np.uint8)) for i in range(6)]
# (n, mask family or None, ms)
CASES = [(9, None, 1), (10, None, 1), (9, "uniform", 8), (10, "short_pub", 8)]
_PROOFS = {}


def proof(ob, n, fam, ms, bits):
    if (n, fam, ms, bits) not in _PROOFS:
        x, point, f = fs.case("uniform", n, fam, ms if fam else None)
        _PROOFS[(n, fam, ms, bits)] = pw.expected_proof(ob.lib(), n, x, point, f, REPS, bits)[:2]
    return _PROOFS[(n, fam, ms, bits)]


def verdict(vp, b, **kw):
    try:
        return vp.Circuit.verify_commitment_fs(b, **kw)
    except ValueError as e:
        return "malformed", str(e)


# ---- the search ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(STATES)))
def test_the_host_search_is_the_hashlib_search(vp, i):
    st = STATES[i]
    for bits in range(1, 13):
        h = pw.grind(st, bits)
        assert h is not None
        nonce, out = vp.fs_grind_host(st, bits)
        assert (nonce, out) == (h, pw.step(st, bits, h)) and pw.met(out, bits), bits
        # the next hit; the two max_tries edges around it
        h2 = pw.grind(st, bits, h + 1)
        assert vp.fs_grind_host(st, bits, first=h + 1)[0] == h2
        first = h + 1
        if h2 > first:
            with pytest.raises(RuntimeError):
                vp.fs_grind_host(st, bits, first=first, max_tries=h2 - first)
        assert vp.fs_grind_host(st, bits, first=first, max_tries=h2 - first + 1) == (h2, pw.step(st, bits, h2))


def test_the_range_rule_at_two_to_the_64_and_the_refusals(vp):
    import ctypes
    L = vp.lib_host()
    st, out, nonce = ctypes.create_string_buffer(STATES[2], 32), ctypes.create_string_buffer(b"\x11" * 32, 32), ctypes.c_uint64(77)
    call = lambda bits, first, tries, s=st, nn=ctypes.byref(nonce), o=out: L.vph_fs_grind_host(ctypes.cast(s, ctypes.c_void_p) if s else None, bits, first, tries, nn,
                                                                                                ctypes.cast(o, ctypes.c_void_p) if o else None)
    top = (1 << 64) - 200
    h = pw.grind(STATES[2], 3, top, 200)
    assert h is not None
    assert call(3, top, 200) == 0 and nonce.value == h and out.raw == pw.step(STATES[2], 3, h)            # first + max_tries = 2^64: the last nonce is 2^64 - 1
    assert call(3, top, 201) == -1 and call(3, (1 << 64) - 1, 2) == -1 and call(3, 1, (1 << 64) - 1) == 0
    nonce.value, keep = 77, out.raw
    for bits, first, tries in ((0, 0, 10), (49, 0, 10), (-1, 0, 10), (4, 0, 0)):
        assert call(bits, first, tries) == -1
    assert call(4, 0, 10, s=None) == -1 and call(4, 0, 10, nn=None) == -1 and call(4, 0, 10, o=None) == -1
    empty = next((f, t) for f in range(0, 4000, 7) for t in (5,) if pw.grind(STATES[2], 12, f, t) is None)
    assert call(12, *empty) == -5 and nonce.value == 77 and out.raw == keep, "an exhausted range leaves the outputs"
    with pytest.raises(ValueError):
        vp.fs_grind_host(STATES[0], 49)
    with pytest.raises(ValueError):
        vp.fs_grind_host(STATES[0], 4, first=1 << 64)
    assert call(48, 0, 1) in (0, -5)                                                                       # 48 bits is inside the limits


# ---- the commitment proof --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 12])
@pytest.mark.parametrize("n,fam,ms", CASES)
def test_version_2_commitment_proofs_are_accepted_and_derived(vp, ob, n, fam, ms, bits):
    b, p = proof(ob, n, fam, ms, bits)
    n_pub = 0 if ms == 1 else p["chain_pub_mask"].shape[0]
    assert struct.unpack_from("<4I2Q2Q", b) == (fs.MAGIC, 2, n, REPS, ms, n_pub, bits, p["nonce"]) and len(b) == fs.sections(n, REPS, n_pub)["end"] + 16
    assert pw.grind(p["state_before_work"], bits) == p["nonce"] and pw.met(pw.step(p["state_before_work"], bits, p["nonce"]), bits)
    assert vp.Circuit.fs_pow(b) == (bits, p["nonce"])
    # the same commitment without work: the same bytes up to the answer, other positions
    x, point, f = fs.case("uniform", n, fam, ms if fam else None)
    b1, p1 = fs.expected_proof(ob.lib(), n, x, point, f, reps=REPS)
    sec = fs.sections(n, REPS, n_pub)
    assert b1[32:sec["answer"]] == b[48:sec["answer"] + 16] and p1["leaf0"] != p["leaf0"]
    assert vp.Circuit.fs_pow(b1) == (0, 0)
    r, lf = vp.Circuit.commitment_fs_challenges(b)
    r_py, lf_py = pw.derive(b)
    assert r.tobytes() == r_py.tobytes() == vp.Circuit.commitment_fs_challenges(b1)[0].tobytes() and lf == lf_py == p["leaf0"]
    assert verdict(vp, b) == (True, "") and verdict(vp, b, min_pow_bits=bits) == (True, "") and verdict(vp, b, min_pow_bits=1) == (True, "")
    assert verdict(vp, b1) == (True, "")


def test_rejections_are_the_ones_hashlib_predicts(vp, ob):
    for key in ((9, None, 1), (10, "short_pub", 8)):
        bits = 8
        b, p = proof(ob, *key, bits)
        st = p["state_before_work"]
        # a nonce that fails, answered honestly at the positions it leads to: only the work is wrong
        bad_nonce = next(v for v in range(p["nonce"] + 1, p["nonce"] + 50) if not pw.met(pw.step(st, bits, v), bits))
        ok, why = verdict(vp, pw.proof_of(pw.reanswered(p, bits, bad_nonce)))
        assert ok is False and "proof of work" in why, why
        ok, why = verdict(vp, pw.proof_of(p, nonce=bad_nonce))                           # ... and with the old answers
        assert ok is False and "proof of work" in why, why
        # pow_bits changed, the nonce kept: the step absorbs the bits, so the state is another one; hashlib says whether the work is met
        for other in (bits - 1, bits + 1, 1, 48):
            q = pw.reanswered(p, other, p["nonce"])
            ok, why = verdict(vp, pw.proof_of(q))
            if pw.met(pw.step(st, other, p["nonce"]), other):
                assert (ok, why) == (True, ""), other
            else:
                assert ok is False and "proof of work" in why, (other, why)
            ok, why = verdict(vp, pw.proof_of(p, pow_bits=other))                        # with the old answers: rejected either way
            assert ok is False and why, other
        # the verifier's demand
        ok, why = verdict(vp, b, min_pow_bits=bits + 1)
        assert ok is False and str(bits) in why and str(bits + 1) in why and "proof of work" in why, why
        x, point, f = fs.case("uniform", key[0], key[1], key[2] if key[1] else None)
        b1, _ = fs.expected_proof(ob.lib(), key[0], x, point, f, reps=REPS)
        ok, why = verdict(vp, b1, min_pow_bits=1)
        assert ok is False and "proof of work" in why and "0 bits" in why and "demands 1" in why, why
        assert verdict(vp, b1, min_pow_bits=0) == (True, "")


def test_malformed_version_2_headers(vp, ob):
    b, p = proof(ob, 9, "uniform", 8, 8)
    x, point, f = fs.case("uniform", 9, "uniform", 8)
    b1, _ = fs.expected_proof(ob.lib(), 9, x, point, f, reps=REPS)
    bad = {"pow_bits = 0": pw.proof_of(p, pow_bits=0), "pow_bits = 49": pw.proof_of(p, pow_bits=49), "pow_bits = 2^63": pw.proof_of(p, pow_bits=1 << 63),
           "pow_bits = 2^64 - 1": pw.proof_of(p, pow_bits=(1 << 64) - 1), "47 header bytes": b[:47], "the header alone": b[:48], "33 bytes": b[:33],
           "a version-1 body under a version-2 header": b1[:4] + struct.pack("<I", 2) + b1[8:], "a version-2 body under a version-1 header": b[:4] + struct.pack("<I", 1) + b[8:],
           "version 3": b[:4] + struct.pack("<I", 3) + b[8:], "short by one": b[:-1], "long by one": b + b"\0"}
    # the version-1 body under a version-2 header, with the 16 bytes behind the header made a valid pair: 16 bytes short of its answer
    forged = bytearray(b1[:4] + struct.pack("<I", 2) + b1[8:]); forged[32:48] = struct.pack("<2Q", 8, 0)
    bad["a version-1 body whose first 16 bytes read as a valid pair"] = bytes(forged)
    for what, x in bad.items():
        ok, why = verdict(vp, x)
        assert ok == "malformed" and why, (what, ok, why)
        with pytest.raises(ValueError):
            vp.Circuit.commitment_fs_challenges(x)
    for what in ("pow_bits = 0", "pow_bits = 49", "pow_bits = 2^63", "47 header bytes", "version 3"):
        with pytest.raises(ValueError):
            vp.Circuit.fs_pow(bad[what])
    with pytest.raises(ValueError):
        vp.Circuit.fs_pow(b"")


# ---- the joined proof ------------------------------------------------------------------------------------------------------------------------------------------
def test_a_version_2_joined_proof_on_the_fixture_circuit(vp, ob):
    _, layers, log_size, seed, reps = ff.FIXTURE
    oc = ob.Circuit.randomize(layers, log_size, seed=seed)
    c = vp.Circuit.randomize(layers, log_size, seed=seed)
    v1 = ff.fixture()
    bits = 8
    b, d = pw.assemble_full(oc, v1, bits)
    st = d["state_before_work"]
    assert struct.unpack_from("<4I2Q2Q", b) == (ff.MAGIC, 2, log_size, reps, 1, 0, bits, d["nonce"]) and len(b) == len(v1) + 16
    assert pw.grind(st, bits) == d["nonce"] and c.fs_pow(b) == (bits, d["nonce"]) and c.fs_pow(v1) == (0, 0)
    s1 = ff.sections(v1)
    assert b[48:s1["answer"] + 16] == v1[32:s1["answer"]] and b[s1["answer"] + 16:] != v1[s1["answer"]:], "the work moves the positions and nothing in front of them"
    ok, why, pt = c.verify_full_fs(b, return_point=True)
    assert (ok, why) == (True, "") and pt.tobytes() == d["point"].tobytes()
    assert c.verify_full_fs(b, min_pow_bits=bits) == (True, "")
    ok, why = c.verify_full_fs(b, min_pow_bits=bits + 1)
    assert ok is False and "proof of work" in why and "8" in why and "9" in why, why
    ok, why = c.verify_full_fs(v1, min_pow_bits=1)
    assert ok is False and "proof of work" in why, why
    # a nonce that fails, the openings answered at the positions it leads to
    bad_nonce = next(v for v in range(d["nonce"] + 1, d["nonce"] + 50) if not pw.met(pw.step(st, bits, v), bits))
    forged, _ = pw.assemble_full(oc, v1, bits, nonce=bad_nonce)
    ok, why = c.verify_full_fs(forged)
    assert ok is False and "proof of work" in why, why
    for what, x in {"pow_bits = 0": b[:32] + struct.pack("<Q", 0) + b[40:], "pow_bits = 49": b[:32] + struct.pack("<Q", 49) + b[40:], "47 bytes": b[:47],
                    "a version-1 body under a version-2 header": v1[:4] + struct.pack("<I", 2) + v1[8:]}.items():
        with pytest.raises(ValueError):
            c.verify_full_fs(x)
    c.close()


# ---- symbols, the sanitizer leg --------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported(vp):
    gpu_hdr = open(os.path.join(ROOT, "include", "vpgpu.h")).read()
    host_hdr = open(os.path.join(ROOT, "virgo-plus_amd", "host", "vphost.h")).read()
    for lib, hdr, names in ((vp.LIB_GPU, gpu_hdr, ("vp_fs_grind",)),
                            (vp.LIB_HOST, host_hdr, ("vph_fs_grind_host", "vph_commit_fs_pow", "vph_prove_full_fs_pow", "vph_verify_commitment_fs_min", "vph_verify_full_fs_min",
                                                     "vph_fs_pow"))):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in names:
            assert re.search(r"\b%s\s*\(" % s, hdr), s + " is not declared"
            assert re.search(r" T %s$" % s, out, flags=re.M), s + " is not exported"
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", gpu_hdr, flags=re.S))
    assert "int vp_fs_grind(vp_ctx *, const uint8_t state_in[32], int bits, uint64_t first, uint64_t max_tries, uint64_t *nonce, uint8_t state_out[32]);" in flat
    assert "The proof of work" in host_hdr
    import ctypes
    body = re.sub(r"/\*.*?\*/", "", gpu_hdr[gpu_hdr.index("typedef struct {\n    uint32_t struct_size;"):gpu_hdr.index("} vp_options;")], flags=re.S)
    public = [f for f in re.findall(r"(?<!u)int32_t\s+(\w+)\s*(?:\[\d+\])?;", body) if f != "reserved"]
    assert len(public) == 12 and ctypes.sizeof(vp.Options) == 4 * (2 + 12 + 4), public
    for name in ("fs_grind", "commit_fs", "prove_full_fs"):
        assert hasattr(vp.Session, name)
    assert hasattr(vp, "fs_grind_host") and hasattr(vp.Circuit, "fs_pow")


def test_parser_and_verifier_under_asan_ubsan(vp, ob, tmp_path):
    """tests/sanitize/fs_pow_main.cpp with the host sources, -fsanitize=address,undefined, run as a program: one good version-2 proof (n = 9, ms = 8, 8 bits)
    accepted, then every truncation class of the 48-byte header, the field extremes, changed bytes, the host search at its range edges — each must end in a
    verdict, none in a report"""
    b, _ = proof(ob, 9, "uniform", 8, 8)
    good = tmp_path / "proof.bin"
    good.write_bytes(b)
    out_dir = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "fs_pow_asan")
    host = os.path.join(ROOT, "virgo-plus_amd", "host")
    csrc = os.path.join(ROOT, "virgo-plus_amd", "csrc")
    src = [os.path.join(host, f) for f in ("circuit.cpp", "prover.cpp", "verifier.cpp", "vphost.cpp")] + [os.path.join(ROOT, "tests", "sanitize", "fs_pow_main.cpp")]
    deps = src + [os.path.join(host, f) for f in os.listdir(host) if f.endswith((".hpp", ".h"))]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-pthread"] + san + ["-o", exe] + src + ["-L" + csrc, "-lvpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(good)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "fs_pow_asan ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
