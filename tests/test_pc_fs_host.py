"""CPU: the non-interactive commitment proof (vph_verify_commitment_fs, vph_commitment_fs_challenges; chain and layout: host/vphost.h) on proofs assembled in
Python without a device — tests/pc_fs_ref.py: the chain with hashlib, the commitment by a fixed point over the oracle, the openings of masked_verifier_cases.

  derivation       the C ABI's challenges and positions equal the Python chain's on every proof below; 10 000 positions of the chain lie in [2^(n-7), 2^(n-2))
  honest           n = 7, 8, 9, 10 with the zero mask, ms = 8 at n = 9 and 10 (a shorter public mask at 10): accepted
  non-interactive  a proof that Circuit.verify_commitment accepts with seeded challenges and positions, packed as a proof: rejected; the chain's challenges with
                   answers at other positions: rejected; one byte changed in every section and header field: rejected or malformed; a changed FRI root k, with the
                   openings answered again at the positions the changed proof derives (what a forger would do — on the plain flip the moved positions already
                   fail the openings of l): the reason names a check at level k or later; short, long, another version or magic, a limb >= p, ms or n_pub
                   outside the rules: malformed
  recorded sizes   tests/golden/pc_fs.json is consistent with the chain: the recorded roots give the recorded challenges and closing state
  symbols          declared in both headers, exported
  sanitizers       tests/sanitize/pc_fs_main.cpp: the host sources under ASan / UBSan parse and verify one good proof and a set of damaged ones"""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import masked_verifier_cases as mvc
import pc_array_inputs as pai
import pc_fs_ref as fs
import pc_masked_inputs as pmi
from conftest import ROOT

REPS = 7
_PROOFS = {}
# (n, mask family or None, ms)
HONEST = [(7, None, 1), (8, None, 1), (9, None, 1), (10, None, 1), (9, "uniform", 8), (10, "short_pub", 8)]


def proof(ob, n, fam, ms):
    if (n, fam, ms) not in _PROOFS:
        x, point, f = fs.case("uniform", n, fam, ms if fam else None)
        _PROOFS[(n, fam, ms)] = fs.expected_proof(ob.lib(), n, x, point, f, reps=REPS)
    return _PROOFS[(n, fam, ms)]


def verdict(vp, proof_bytes):
    """(accepted, reason), or ("malformed", reason) for the return code -1"""
    try:
        return vp.Circuit.verify_commitment_fs(proof_bytes)
    except ValueError as e:
        return "malformed", str(e)


@pytest.mark.parametrize("n,fam,ms", HONEST)
def test_honest_proofs_are_accepted_and_the_derivation_is_the_chains(vp, ob, n, fam, ms):
    b, p = proof(ob, n, fam, ms)
    assert p["ms"] == ms and struct.unpack_from("<4I2Q", b) == (fs.MAGIC, fs.VERSION, n, REPS, ms, 0 if ms == 1 else p["chain_pub_mask"].shape[0])
    if fam == "short_pub":
        assert p["chain_pub_mask"].shape[0] < p["pri_mask"].shape[0]
    if ms > 1:
        assert p["all_sum"][64].any() and p["final_mask"].any(), "a vacuous masked case"
    assert len(b) == fs.sections(n, REPS, 0 if ms == 1 else p["chain_pub_mask"].shape[0])["end"]
    r, lf = vp.Circuit.commitment_fs_challenges(b)
    r_py, lf_py = fs.derive(b)
    assert r.tobytes() == r_py.tobytes() == np.ascontiguousarray(p["r"], np.uint64).tobytes() and lf == lf_py == p["leaf0"]
    assert verdict(vp, b) == (True, "")


@pytest.mark.parametrize("n", [7, 10, 25])
def test_ten_thousand_positions_lie_in_the_accepted_range(n):
    ch = fs.Chain(bytes(range(32)))
    lf = [ch.Q(q, n) for q in range(10000)]
    assert min(lf) >= 1 << (n - 7) and max(lf) < 1 << (n - 2)
    assert len(set(lf)) > 1 and (n > 7 or len(set(lf)) == (1 << 5) - 1), "n = 7: every one of the 31 leaves is reached"


def test_the_reduction_maps_p_to_zero():
    assert [fs.limb(w) for w in (0, fs.P - 1, fs.P, 1 << 61, (1 << 64) - 1)] == [0, fs.P - 1, 0, 0, 0]


def test_an_interactive_proof_packed_as_a_proof_is_rejected(vp, ob):
    """seeded challenges and positions: Circuit.verify_commitment accepts it, nothing binds it to its own roots"""
    n = 9
    x, point, _ = fs.case("uniform", n)
    seeded = mvc.build(ob.lib(), n, dict(x, pub=fs.eq_table(point)), {"pri_mask": np.zeros((8, 2), np.uint64), "pub_mask": np.zeros((1, 2), np.uint64), "r": x["r"]}, seed=5)
    seeded["ms"] = 1
    seeded["leaf0"] = seeded["leaf0"][:REPS]
    seeded["answer"] = mvc.answer(seeded)
    assert mvc.verify(vp, seeded) == (True, "")
    seeded["point"], seeded["chain_pub_mask"] = point, np.zeros((0, 2), np.uint64)
    ok, why = verdict(vp, fs.proof_of(seeded))
    assert ok is False and why


def test_the_chains_challenges_with_answers_at_other_positions_are_rejected(vp, ob):
    for key in ((9, None, 1), (9, "uniform", 8)):
        b, p = proof(ob, *key)
        other = dict(p, leaf0=mvc.positions(key[0], 11, REPS))
        assert other["leaf0"] != p["leaf0"]
        other["answer"] = mvc.answer(other)
        assert mvc.verify(vp, other) == (True, ""), "openings of the committed trees"
        ok, why = verdict(vp, fs.proof_of(other))
        assert ok is False and "Merkle opening rejected" in why


def _level_of(why, ln):
    """the FRI level a reason names; ln for the checks behind the last level"""
    m = re.search(r"consistency (\d+) round|\(level (\d+)\)", why)
    if m:
        return int(m.group(1) or m.group(2))
    return ln if re.search(r"final codeword|rs code check", why) else -1


@pytest.mark.parametrize("key", [(10, None, 1), (10, "short_pub", 8)])
def test_one_changed_byte_in_any_section_is_rejected(vp, ob, key):
    n, ln = key[0], key[0] - 6
    b, p = proof(ob, *key)
    sec = fs.sections(n, REPS, 0 if key[2] == 1 else p["chain_pub_mask"].shape[0])
    flips = {"magic": 1, "version": 4, "n": 8, "reps": 12, "ms": 16, "n_pub": 24, "point": sec["point"] + 3, "claim": sec["claim"] + 9, "root_l": sec["root_l"] + 31,
             "root_h": sec["root_h"], "all_sum[0]": sec["all_sum"] + 2, "all_sum[64]": sec["all_sum"] + 64 * 16 + 8, "final_code": sec["final_code"] + 1000,
             "final_mask": sec["final_mask"] + 17, "a value": sec["answer"] + 40, "a mask pair": sec["answer"] + 129 * 16 + 2, "a path": sec["end"] - 1}
    if key[2] > 1:
        flips["pub_mask"] = sec["pub_mask"] + 5
    for k in range(ln):
        flips["fri root %d" % k] = sec["fri_roots"] + 32 * k + 7
    for what, off in flips.items():
        bad = bytearray(b); bad[off] ^= 0x04
        ok, why = verdict(vp, bytes(bad))
        assert ok in (False, "malformed") and why, what
    # a changed FRI root k moves every later challenge and every position; answered again at the positions the changed proof derives, the verdict names level k or later
    for k in range(ln):
        roots = bytearray(p["fri_roots"]); roots[32 * k + 7] ^= 0x04
        forged = dict(p, fri_roots=bytes(roots))
        r_new, lf_new = fs.derive(fs.proof_of(forged))
        assert r_new[:k + 1].tobytes() == np.ascontiguousarray(p["r"], np.uint64)[:k + 1].tobytes() and lf_new != p["leaf0"]
        assert k + 1 == ln or r_new[k + 1:].tobytes() != np.ascontiguousarray(p["r"], np.uint64)[k + 1:].tobytes()
        forged["leaf0"] = lf_new
        forged["answer"] = mvc.answer(forged)
        ok, why = verdict(vp, fs.proof_of(forged))
        assert ok is False and _level_of(why, ln) >= k, (k, why)


def test_malformed_proofs_are_refused(vp, ob):
    n = 9
    b, p = proof(ob, n, "uniform", 8)
    sec = fs.sections(n, REPS, p["chain_pub_mask"].shape[0])
    head = lambda **kw: struct.pack("<4I2Q", *[kw.get(k, v) for k, v in zip(("magic", "version", "n", "reps", "ms", "n_pub"), struct.unpack_from("<4I2Q", b))]) + b[32:]
    limb = bytearray(b); limb[sec["claim"]:sec["claim"] + 8] = struct.pack("<Q", fs.P)
    limb2 = bytearray(b); limb2[sec["final_mask"] + 8:sec["final_mask"] + 16] = struct.pack("<Q", (1 << 64) - 1)
    bad = {"empty": b"", "header only": b[:32], "short by one": b[:-1], "long by one": b + b"\0", "cut inside a section": b[:sec["final_code"] + 100],
           "without the answer": b[:sec["answer"]], "version 2": head(version=2), "version 0": head(version=0), "magic": head(magic=0x52465056), "n = 6": head(n=6),
           "n = 31": head(n=31), "n = 2^32 - 1": head(n=0xFFFFFFFF), "reps = 0": head(reps=0), "reps = 4097": head(reps=4097), "ms = 0": head(ms=0), "ms = 4": head(ms=4),
           "ms = 12": head(ms=12), "ms = 2^(n-1)": head(ms=1 << (n - 1)), "ms = 2^63": head(ms=1 << 63), "n_pub = ms + 1": head(n_pub=9), "n_pub = 2^64 - 1": head(n_pub=(1 << 64) - 1),
           "ms = 1 with a public mask": head(ms=1), "a limb = p": bytes(limb), "a limb = 2^64 - 1": bytes(limb2)}
    for what, x in bad.items():
        ok, why = verdict(vp, x)
        assert ok == "malformed" and why, what
        with pytest.raises(ValueError):
            vp.Circuit.commitment_fs_challenges(x)


def test_the_recorded_sizes_are_consistent_with_the_chain():
    rec = json.load(open(fs.GOLDEN))
    assert set(rec) == set(fs.RECORDED)
    for name, (kind, n, fam, ms) in fs.RECORDED.items():
        g, ln = rec[name], n - 6
        roots = bytes.fromhex(g["roots"])
        ch = fs.Chain(bytes.fromhex(g["state_in"]))
        r = fs.commit_phase(ch, [roots[32 * k:32 * k + 32] for k in range(ln)])
        assert np.array(r, np.uint64).tobytes().hex() == g["r"] and ch.s.hex() == g["state_out"], name
        assert g["ms"] == (1 if fam is None else ms) and len(g["leaf0"]) == 33 and all(1 << (n - 7) <= v < 1 << (n - 2) for v in g["leaf0"])


def test_new_symbols_are_declared_and_exported(vp):
    gpu_hdr = open(os.path.join(ROOT, "include", "vpgpu.h")).read()
    host_hdr = open(os.path.join(ROOT, "virgo-plus_amd", "host", "vphost.h")).read()
    for lib, hdr, names in ((vp.LIB_GPU, gpu_hdr, ("vp_fri_commit_fs", "vp_test_fs_draw")),
                            (vp.LIB_HOST, host_hdr, ("vph_commit_fs", "vph_verify_commitment_fs", "vph_commitment_fs_challenges", "vph_last_commit_fs_times"))):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in names:
            assert re.search(r"\b%s\s*\(" % s, hdr), s + " is not declared"
            assert re.search(r" T %s$" % s, out, flags=re.M), s + " is not exported"
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", gpu_hdr, flags=re.S))
    assert "int vp_fri_commit_fs(vp_ctx *, const uint8_t state_in[32], uint8_t *roots , vp_F *r_out , uint8_t state_out[32]);" in flat
    assert "enum { VPH_FS_HOST_DRAWS = 1 };" in host_hdr and "The transcript chain" in host_hdr
    for name in ("commit_fs",):
        assert hasattr(vp.Session, name)
    assert hasattr(vp.Circuit, "verify_commitment_fs") and hasattr(vp.Circuit, "commitment_fs_challenges")


def test_parser_and_verifier_under_asan_ubsan(vp, ob, tmp_path):
    """tests/sanitize/pc_fs_main.cpp with the host sources, -fsanitize=address,undefined: one good proof (n = 9, ms = 8) accepted, then changed bytes, every
    truncation class, header fields at their extremes — each must end in a verdict, none in a report"""
    b, _ = proof(ob, 9, "uniform", 8)
    good = tmp_path / "proof.bin"
    good.write_bytes(b)
    out_dir = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "pc_fs_asan")
    host = os.path.join(ROOT, "virgo-plus_amd", "host")
    csrc = os.path.join(ROOT, "virgo-plus_amd", "csrc")
    src = [os.path.join(host, f) for f in ("circuit.cpp", "prover.cpp", "verifier.cpp", "vphost.cpp")] + [os.path.join(ROOT, "tests", "sanitize", "pc_fs_main.cpp")]
    deps = src + [os.path.join(host, f) for f in os.listdir(host) if f.endswith((".hpp", ".h"))]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-pthread"] + san + ["-o", exe] + src + ["-L" + csrc, "-lvpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    # (libvpgpu.so is linked, since the prover class forwards to it, and never initialised; the ROCm libraries behind it keep process-lifetime allocations)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(good)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "pc_fs_asan ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
