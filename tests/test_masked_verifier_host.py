"""CPU: the host verifier of masked commitments at commitment level (vph_verify_commitment = verifier.cpp's pcVerifyCommitment, the algebra verifyPoly itself
runs), on complete proofs assembled in Python from the oracle's openings of every leaf (tests/masked_verifier_cases.py).  Every comparison is a verdict, the
name of the failed check, or bytes.

  accept       n = 9 (N = 8 = ms, the smallest accepted mask) and n = 10 (ms = 8, 16), the four non-zero mask families — all_sum[64] != 0 and a final mask
               codeword that is not all zero, asserted — and pub_zero, pri_zero, and the zero mask through the same entry (ms = 1)
  reject       by name: ms = 2 N and 4 N at the final mask codeword (the reference's "Fri msk rs code check fail"); a changed public mask element, ms halved and
               all_sum[64] moved by d (on a masked and on the zero-mask proof) at the mask slice's fold consistency; claim and all_sum[64] moved by the same d at the
               slice sums — the claim is the witness slots' sum alone, all_sum[64] is no part of it (a sum over 65 slots would reject every honest masked proof);
               a changed mask pair in an l, an h and a level opening at the Merkle check; another constant as final mask codeword at the last level
  reference    where oracle/_ref/ref_run exists, the real reference's verifier on its own commitments of the eleven CASES: REFERENCE_VERDICTS below
  mask row     vph_pc_mask_evals_host against interpolate / horner of tests/pc_mask_ref.py at ms = 8 .. 256"""
import os
import re
import subprocess

import numpy as np
import pytest

import masked_verifier_cases as mvc
import pc_array_inputs as pai
import pc_mask_ref as mref
import pc_masked_inputs as pmi
import pc_verify_ref as ref
from conftest import ROOT

NONZERO = pmi.NONZERO_FAMILIES
_PROOFS = {}

REFERENCE_VERDICTS = mvc.REFERENCE_VERDICTS


def proof(ob, n, ms, fam):
    if (n, ms, fam) not in _PROOFS:
        x = pai.inputs("uniform", n)
        if fam == "zero":                            # zero masks of any accepted length are the unmasked commitment (tests/test_pc_masked_host.py)
            f = {"pri_mask": np.zeros((8, 2), np.uint64), "pub_mask": np.zeros((1, 2), np.uint64), "r": x["r"]}
        else:
            f = pmi.family(fam, n, ms)
        p = mvc.build(ob.lib(), n, x, f, seed=100 * n + ms)
        if fam == "zero":
            p["ms"] = 1
        _PROOFS[(n, ms, fam)] = p
    return _PROOFS[(n, ms, fam)]


ACCEPT = [(n, ms) for n in (9, 10) for ms in pmi.accepted_ms(n) if ms <= 1 << (n - 6)]


def test_the_accept_cases_are_every_mask_up_to_a_slice():
    assert ACCEPT == [(9, 8), (10, 8), (10, 16)]


@pytest.mark.parametrize("fam", pmi.FAMILIES)
@pytest.mark.parametrize("n,ms", ACCEPT)
def test_masked_commitments_are_accepted(vp, ob, n, ms, fam):
    p = proof(ob, n, ms, fam)
    assert p["ms"] == ms
    if fam in NONZERO:
        assert p["all_sum"][64].any() and p["final_mask"].any(), "a vacuous case"
    assert mvc.verify(vp, p) == (True, "")


@pytest.mark.parametrize("n", [9, 10])
def test_the_zero_mask_is_accepted_through_the_same_entry(vp, ob, n):
    p = proof(ob, n, 1, "zero")
    assert not p["all_sum"][64].any() and not p["final_mask"].any()
    assert mvc.verify(vp, p) == (True, "")
    assert mvc.verify(vp, p, pub_mask=None) == (True, "")


@pytest.mark.parametrize("n,mult", [(9, 2), (9, 4), (10, 2), (10, 4)])
def test_a_mask_longer_than_a_slice_is_rejected_at_the_final_mask_codeword(vp, ob, n, mult):
    p = proof(ob, n, mult << (n - 6), "uniform")
    assert mvc.verify(vp, p) == (False, "Fri msk rs code check fail")


@pytest.mark.parametrize("n,ms", ACCEPT)
def test_the_mask_slices_own_checks_reject(vp, ob, n, ms):
    p = proof(ob, n, ms, "short_pub")
    fail = "Fri msk check consistency 0 round fail"
    pm = p["pub_mask"].copy(); pm[0, 0] ^= np.uint64(1)
    assert mvc.verify(vp, p, pub_mask=pm) == (False, fail), "one element of the public mask"
    if ms >= 16:                                     # (ms / 2 = 4 is no padded length of a commitment: malformed, below)
        assert p["pub_mask"].shape[0] <= ms // 2
        assert mvc.verify(vp, p, ms=ms // 2) == (False, fail), "ms halved"
    # The claim is <witness, pub> alone and all_sum[64] = <private mask, public mask> comes on top of it (asserted), so the sum the verifier compares with the claim
    # runs over the 64 witness slots: a claim moved by d is off that sum whatever all_sum[64] does, and all_sum[64] moved by d meets the mask slice's own check.
    tot = (0, 0)
    for j in range(64):
        tot = mvc.f_add(tot, p["all_sum"][j])
    assert tuple(tot) == tuple(p["claim"]) and p["all_sum"][64].any()
    d = (5, 7)
    sums = p["all_sum"].copy(); sums[64] = mvc.f_add(sums[64], d)
    assert mvc.verify(vp, p, claim=mvc.f_add(p["claim"], d), all_sum=sums) == (False, "commitment: slice sums do not match the inner product"), "claim and all_sum[64] moved together"
    assert mvc.verify(vp, p, all_sum=sums) == (False, fail), "all_sum[64] moved"


@pytest.mark.parametrize("n", [9, 10])
def test_the_zero_mask_slot_is_constrained(vp, ob, n):
    """what the verifier did not check before: with the reference's zero mask, a claim moved off the inner product together with all_sum[64]"""
    p = proof(ob, n, 1, "zero")
    d = (1, 0)
    sums = p["all_sum"].copy(); sums[64] = mvc.f_add(sums[64], d)
    assert mvc.verify(vp, p, claim=mvc.f_add(p["claim"], d), all_sum=sums) == (False, "commitment: slice sums do not match the inner product")
    assert mvc.verify(vp, p, all_sum=sums) == (False, "Fri msk check consistency 0 round fail")
    fm = p["final_mask"].copy(); fm[:, 0] = 3
    assert mvc.verify(vp, p, final_mask=fm) == (False, "Fri msk final codeword mismatch")


@pytest.mark.parametrize("oracle", [0, 1, 2, 4])
def test_a_changed_mask_pair_is_a_merkle_rejection(vp, ob, oracle):
    n = 10
    p = proof(ob, n, 16, "uniform")
    _, leaf, _ = ref.query_leaves(n, p["leaf0"][3])[oracle]
    vals = [v.copy() for v in p["vals"]]
    vals[oracle][leaf, 128 + (oracle & 1), 1] ^= np.uint64(4)
    ok, why = mvc.verify(vp, p, answer=mvc.answer(p, vals))
    assert not ok and why == ("commitment: Merkle opening rejected" if oracle < 2 else "commitment: FRI Merkle opening rejected (level %d)" % (oracle - 2))


@pytest.mark.parametrize("n,ms", ACCEPT)
def test_another_constant_as_final_mask_codeword_is_a_last_level_rejection(vp, ob, n, ms):
    p = proof(ob, n, ms, "edges")
    fm = p["final_mask"].copy(); fm[:] = mvc.f_add(fm[0], (1, 0))
    assert mvc.verify(vp, p, final_mask=fm) == (False, "Fri msk final codeword mismatch")
    fm = p["final_mask"].copy(); fm[31] = mvc.f_add(fm[31], (0, 1))
    assert mvc.verify(vp, p, final_mask=fm) == (False, "Fri msk rs code check fail")


def test_malformed_arguments_are_no_verdict(vp, ob):
    p = proof(ob, 10, 16, "uniform")
    bad = p["all_sum"].copy(); bad[64, 0] = ref.P
    for change in ({"ms": 4}, {"ms": 24}, {"ms": 512}, {"ms": 8}, {"leaf0": p["leaf0"][:-1]}, {"answer": p["answer"][:-1]}, {"all_sum": bad},
                   {"leaf0": [1] + p["leaf0"][1:]}):
        with pytest.raises(ValueError):
            mvc.verify(vp, p, **change)
    with pytest.raises(ValueError):                  # both of point and pub
        vp.Circuit.verify_commitment(10, p["claim"], p["root_l"], p["root_h"], p["all_sum"], p["r"], p["fri_roots"], p["final_code"], p["final_mask"], p["leaf0"],
                                     p["answer"], pub=p["pub"], point=p["pub"][:10], pub_mask=p["pub_mask"], ms=16)


def test_a_non_canonical_opened_value_is_rejected(vp, ob):
    n = 9
    p = proof(ob, n, 8, "uniform")
    a = bytearray(p["answer"])
    a[128 * 16:128 * 16 + 8] = int(ref.P).to_bytes(8, "little")
    ok, why = mvc.verify(vp, p, answer=bytes(a))
    assert not ok and "non-canonical" in why


@pytest.mark.parametrize("name", [k for k, v in pmi.CASES.items() if v[0] in (13, 16)])       # (n19_m3000: pmi.REFERENCE_VERIFIER_ACCEPTS holds its recorded verdict)
def test_verdicts_equal_the_real_references(name, tmp_path):
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_run")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_run not built (needs the reference tree at build time)")
    n, m, _ = pmi.CASES[name]
    inp = tmp_path / "in.bin"
    pmi.write_case_file(name, str(inp))
    r = subprocess.run([exe, "--pc-masked", str(inp), "--verify"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    got = "verify_poly_commitment ACCEPT" in r.stdout
    assert got != ("verify_poly_commitment REJECT" in r.stdout), (r.stdout[-400:], r.stderr[-400:])
    want = pmi.REFERENCE_VERIFIER_ACCEPTS.get(name, pmi.padded_length(n, m)[1] <= 1 << (n - 6))
    assert got == want == REFERENCE_VERDICTS[name]
    if not got:
        assert "Fri msk rs code check fail" in r.stderr


def test_the_observed_table_is_the_rule():
    assert set(REFERENCE_VERDICTS) == set(pmi.CASES)
    for name, (n, m, _) in pmi.CASES.items():
        assert REFERENCE_VERDICTS[name] == (pmi.padded_length(n, m)[1] <= 1 << (n - 6)), name
        assert pmi.REFERENCE_VERIFIER_ACCEPTS.get(name, REFERENCE_VERDICTS[name]) == REFERENCE_VERDICTS[name]


@pytest.mark.parametrize("ms", [8, 16, 32, 64, 128, 256])
def test_mask_evals_host_equal_the_definition(vp, ms):
    n = max(9, ms.bit_length() + 1)                  # ms <= 2^(n-2)
    rng = np.random.default_rng(4000 + ms)
    for m in (ms, ms - ms // 4, 1):
        pm = rng.integers(0, ref.P, size=(m, 2), dtype=np.uint64)
        if m == ms:
            pm[0], pm[-1] = (ref.P - 1, ref.P - 1), (0, 1)
        lf = mvc.positions(n, ms, reps=5)
        got = vp.Circuit.pc_mask_evals_host(n, lf, pm, ms)
        w = ref.root_of_unity(n - 1)
        coef = mref.interpolate([(int(a), int(b)) for a, b in pm] + [mref.ZERO] * (ms - m), mref.power(w, (1 << (n - 1)) // ms))
        for q, leaf in enumerate(lf):
            x = mref.power(w, leaf)
            assert tuple(int(v) for v in got[q, 0]) == mref.horner(coef, x) and tuple(int(v) for v in got[q, 1]) == mref.horner(coef, mref.sub(mref.ZERO, x)), (ms, m, q)
    for args in ((n, lf, pm, 3 * ms // 2), (n, lf, np.zeros((ms + 1, 2), np.uint64), ms), (n, [0], pm, ms), (n, lf, np.full((1, 2), ref.P, np.uint64), ms)):
        with pytest.raises(ValueError):
            vp.Circuit.pc_mask_evals_host(*args)


def test_new_symbols_are_declared_and_exported_and_the_old_ones_unchanged(vp):
    gpu_hdr = open(os.path.join(ROOT, "include", "vpgpu.h")).read()
    host_hdr = open(os.path.join(ROOT, "virgo-plus_amd", "host", "vphost.h")).read()
    for lib, hdr, names in ((vp.LIB_GPU, gpu_hdr, ("vp_pc_mask_evals",)),
                            (vp.LIB_HOST, host_hdr, ("vph_verify_commitment", "vph_prove_and_verify_full_masked", "vph_pc_mask_evals_host", "vph_pc_mask_evals"))):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in names:
            assert re.search(r"\b%s\s*\(" % s, hdr), s + " is not declared"
            assert re.search(r" T %s$" % s, out, flags=re.M), s + " is not exported"
    flat = lambda h: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", h, flags=re.S))
    g, h = flat(gpu_hdr), flat(host_hdr)
    assert "int vp_pc_mask_evals(vp_ctx *, int n, const vp_F *pub_mask, uint64_t n_pub_mask, uint64_t ms, int n_queries, const uint64_t *leaf0, vp_F *out );" in g
    assert "int vp_pc_public_evals(vp_ctx *, int n, const vp_F *point , const vp_F *pub , int n_queries, const uint64_t *leaf0, vp_F *out );" in g
    assert "int vp_fri_query_digests(vp_ctx *, int n, int n_queries, const uint64_t *leaf0, const uint8_t *answer, uint64_t n_bytes, uint8_t *out );" in g
    assert ("int vph_prove_and_verify_full_ex(vph_session *, int reps, int flags, uint8_t *transcript, uint64_t capacity, uint64_t *n_written, double *gkr_prove_sec, "
            "double *pc_prove_sec, double *verify_sec, char *err, int errlen);") in h
    assert ("int vph_prove_and_verify_full(vph_session *, int reps, uint8_t *transcript, uint64_t capacity, uint64_t *n_written, double *gkr_prove_sec, "
            "double *pc_prove_sec, double *verify_sec, char *err, int errlen);") in h
    assert "int vph_verify_full_record(vph_circuit *, const uint8_t *record, uint64_t n);" in h
    assert "int vph_verify_full_record_dev(vph_circuit *, int device, const uint8_t *record, uint64_t n, char *err, int errlen);" in h
    kinds = [k.strip() for k in re.search(r"enum \{ (VP_K_BETA = 0.*?), VP_K_COUNT \}", gpu_hdr, flags=re.S).group(1).replace(" = 0", "").split(",")]
    assert kinds.index("VP_K_PC_OPEN_MANY") == len(kinds) - 1
    for m in ("pc_mask_evals",):
        assert hasattr(vp.Session, m)
    for m in ("pc_mask_evals_host", "verify_commitment"):
        assert hasattr(vp.Circuit, m)
    import inspect
    sig = inspect.signature(vp.Session.prove_and_verify_full)
    assert list(sig.parameters)[-2:] == ["mask", "pub_mask"] and sig.parameters["mask"].default is None


def test_masked_verifier_under_asan_ubsan(vp, ob, tmp_path):
    """tests/sanitize/masked_verify_main.cpp — a program of its own, built with -fsanitize=address,undefined from the host sources and run directly: the
    commitment-level verifier on an accepted proof, on one with a changed public mask and on one whose answer holds a changed mask pair."""
    from test_sanitizers import ENV, SAN
    out_dir = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "masked_verify_asan")
    host = os.path.join(ROOT, "virgo-plus_amd", "host")
    csrc = os.path.join(ROOT, "virgo-plus_amd", "csrc")
    src = [os.path.join(host, f) for f in ("circuit.cpp", "prover.cpp", "verifier.cpp", "vphost.cpp")] + [os.path.join(ROOT, "tests", "sanitize", "masked_verify_main.cpp")]
    deps = src + [os.path.join(host, f) for f in os.listdir(host) if f.endswith((".hpp", ".h"))]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-pthread"] + SAN + ["-o", exe] + src +
                       ["-L" + csrc, "-lvpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    n = 9
    p = proof(ob, n, 8, "short_pub")
    vals = [v.copy() for v in p["vals"]]
    vals[0][p["leaf0"][0], 129, 0] ^= np.uint64(1)
    case = tmp_path / "case.bin"
    with open(case, "wb") as f:                      # i32 n, i32 reps, u64 ms, u64 n_pub_mask, u64 answer bytes, then the arrays in verify_commitment's order
        f.write(np.array([n, len(p["leaf0"])], np.int32).tobytes())
        f.write(np.array([p["ms"], p["pub_mask"].shape[0], len(p["answer"])], np.uint64).tobytes())
        for a in (p["pub"], p["pub_mask"], p["claim"], p["all_sum"], p["r"], p["final_code"], p["final_mask"], np.array(p["leaf0"], np.uint64)):
            f.write(np.ascontiguousarray(a, np.uint64).tobytes())
        f.write(p["root_l"] + p["root_h"] + p["fri_roots"] + p["answer"] + mvc.answer(p, vals))
    env = dict(ENV, ASAN_OPTIONS="detect_leaks=0:exitcode=99")
    r = subprocess.run([exe, str(case)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "masked_verify_asan ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
