"""CPU: the two heavy loops of the commitment's verifier (host/verifier.cpp: pcPublicEvalsHost, pcOpeningDigestsHost — the functions verifyPoly itself
calls), read by value through vphost.h and compared with a reference written from the definitions in Python integers (tests/pc_verify_ref.py:
the eq table as a product, the interpolant in barycentric form, hashlib's SHA3-256).  Every comparison is equality of bytes: the arithmetic is exact.

What is here and why:
  n = 7 .. 10                         slices of 2, 4, 8, 16 entries: the smallest the commitment takes, and the fixture's size
  points                              uniform | the 0/1 corners (unit vectors) | edge limbs (p - 1, 2^60, 2^31 +- 1) | one general vector (no tensor)
  leaves                              N / 2 (smallest; at n = 10 not yet a multiple of 32) | M / 2 - 1 | one drawn | M / 4 + 1 and M / 8 + 3
                                      (upper half at one FRI level, lower at another)
  tests/golden/full_record_custom_a   real openings: the digest loop must reproduce every path[depth] and every committed root; flips move exactly
                                      the digests they should; the record is still accepted, and still rejected with the flips of
                                      tests/test_query_record_host.py (the factoring changed nothing)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pc_verify_cases as cases
import pc_verify_ref as ref
from conftest import GOLDEN, ROOT
from test_query_record_host import NAME, _offsets, case  # noqa: F401  (the fixture record and the flips of that file)

VAL = ref.VAL


def _tuples(a):
    return [(int(x[0]), int(x[1])) for x in np.asarray(a).reshape(-1, 2)]


def _ref_bytes(n, pub, lf):
    return b"".join(ref.pack(row) for q in ref.public_evals(n, pub, lf) for row in q)


@pytest.mark.parametrize("n", [7, 8, 9, 10])
def test_public_evals_equal_the_definition(vp, n):
    lf = cases.leaves(n)
    for name, pt in cases.points(n).items():
        want = _ref_bytes(n, ref.eq_table(_tuples(pt)), lf)
        got = vp.Circuit.pc_public_evals_host(n, lf, point=pt)
        assert got.shape == (len(lf), 2, 64, 2) and int(got.max()) < ref.P
        assert got.tobytes() == want, (n, name)
        # the one-transform form (what the GPU test's host side uses at n = 24) and the vector form on the expanded table: the same values
        assert vp.Circuit.pc_public_evals_host(n, lf, point=pt, tensor=True).tobytes() == want, (n, name, "tensor")
        tab = np.array(ref.eq_table(_tuples(pt)), dtype=np.uint64)
        assert vp.Circuit.pc_public_evals_host(n, lf, pub=tab).tobytes() == want, (n, name, "pub")
    vec = cases.general_vector(n)
    assert vp.Circuit.pc_public_evals_host(n, lf, pub=vec).tobytes() == _ref_bytes(n, _tuples(vec), lf), (n, "general vector")


def test_public_evals_at_a_slice_root_and_with_repeats(vp):
    """A leaf that is a multiple of 32 makes x an N-th root of unity: q_j(x) is then the slice's own entry.  Repeated leaves repeat their rows."""
    n = 10
    N = 1 << (n - 6)
    vec = cases.general_vector(n)
    lf = [32, 64, 32, 33]
    got = vp.Circuit.pc_public_evals_host(n, lf, pub=vec)
    assert got.tobytes() == _ref_bytes(n, _tuples(vec), lf)
    for j in range(64):
        assert tuple(got[0, 0, j]) == tuple(vec[j * N + 1]) and tuple(got[1, 0, j]) == tuple(vec[j * N + 2])     # w^32 = omega, w^64 = omega^2
    assert got[0].tobytes() == got[2].tobytes() != got[3].tobytes()


def test_public_evals_refusals(vp):
    n = 8
    pt = cases.points(n)["uniform"]
    ok = cases.leaves(n)
    f = vp.Circuit.pc_public_evals_host
    f(n, ok, point=pt)
    bad = pt.copy(); bad[3, 1] = ref.P
    for kw, lf in (({"point": bad}, ok), ({"point": pt}, [1]), ({"point": pt}, [1 << (n - 2)]), ({"point": pt}, []), ({}, ok),
                   ({"point": pt, "pub": cases.general_vector(n)}, ok), ({"pub": cases.general_vector(n), "tensor": True}, ok)):
        with pytest.raises(ValueError):
            f(n, lf, **kw)
    with pytest.raises(ValueError):
        f(6, [1], point=pt[:6])


def _leaf0_of_record(c):
    """The positions the record's openings were made at: the record does not store them (the replay redraws them), so they are found from the definition
    — the leaf under which opening 0's path leads to root_l."""
    rec, sec, n, reps = c["rec"], c["sec"], c["n"], c["meta"]["reps"]
    root_l = rec[sec["transcript"]:sec["transcript"] + 32]
    out = []
    for q in range(reps):
        at = sec["openings"] + q * c["per_query"]
        vals, path = rec[at:at + VAL], rec[at + VAL:at + VAL + 32 * (n - 1)]
        hits = [lf for lf in range(1 << (n - 7), 1 << (n - 2)) if ref.opening_digest(lf, vals, path, n - 2)[1] == root_l]
        assert len(hits) == 1
        out.append(hits[0])
    return out


def _roots_of_record(c):
    rec, sec, n = c["rec"], c["sec"], c["n"]
    tr, gl = sec["transcript"], len(c["gold"])
    return [rec[tr:tr + 32], rec[tr + gl - (32 + 16 + 65 * 16):tr + gl - (16 + 65 * 16)]] + [rec[sec["roots"] + 32 * k:sec["roots"] + 32 * k + 32] for k in range(n - 6)]


def test_digest_loop_reproduces_the_records_leaf_digests_and_roots(vp, case):
    n, sec, rec = case["n"], case["sec"], case["rec"]
    lf = _leaf0_of_record(case)
    ans = rec[sec["openings"]:sec["end"]]
    assert len(ans) == vp.Circuit.pc_query_answer_bytes(n, len(lf)) == ref.answer_bytes(n, len(lf))
    dig = vp.Circuit.pc_opening_digests_host(n, lf, ans)
    assert dig == ref.opening_digests(n, lf, ans) and len(dig) == len(lf) * (n - 4) * 64
    roots, at, i = _roots_of_record(case), 0, 0
    for l0 in lf:
        for o, _, plen in ref.query_leaves(n, l0):
            assert dig[64 * i:64 * i + 32] == ans[at + VAL + 32 * (plen - 1):at + VAL + 32 * plen], (i, "path[depth]")
            assert dig[64 * i + 32:64 * i + 64] == roots[o], (i, "root")
            at += VAL + 32 * plen; i += 1


def test_digest_loop_flips_move_exactly_their_digests(vp, case):
    n, sec, rec = case["n"], case["sec"], case["rec"]
    lf = _leaf0_of_record(case)
    ans = rec[sec["openings"]:sec["end"]]
    base = vp.Circuit.pc_opening_digests_host(n, lf, ans)
    n_open = len(lf) * (n - 4)
    at, starts = 0, []
    for l0 in lf:
        for _, _, plen in ref.query_leaves(n, l0):
            starts.append((at, plen)); at += VAL + 32 * plen

    def changed(off):
        bad = bytearray(ans); bad[off] ^= 0x20
        got = vp.Circuit.pc_opening_digests_host(n, lf, bytes(bad))
        assert got == ref.opening_digests(n, lf, bytes(bad))
        return [k for k in range(2 * n_open) if got[32 * k:32 * k + 32] != base[32 * k:32 * k + 32]]

    for i in (0, n_open // 2, n_open - 1):
        s, plen = starts[i]
        assert changed(s + 7) == [2 * i, 2 * i + 1] and changed(s + VAL - 1) == [2 * i, 2 * i + 1]          # a value byte: both digests of that opening
        for k in (0, plen - 2):
            assert changed(s + VAL + 32 * k + 5) == [2 * i + 1], (i, k)                                      # a path byte at height k: its root only
        assert changed(s + VAL + 32 * (plen - 1)) == []                                                      # path[depth] is the prover's copy: not read


def test_digest_loop_refuses_other_sizes(vp, case):
    n, sec, rec = case["n"], case["sec"], case["rec"]
    lf = _leaf0_of_record(case)
    ans = rec[sec["openings"]:sec["end"]]
    for bad in (ans[:-1], ans + b"\0", ans[:-32], b""):
        with pytest.raises(ValueError):
            vp.Circuit.pc_opening_digests_host(n, lf, bad)
    with pytest.raises(ValueError):
        vp.Circuit.pc_opening_digests_host(n, lf[:1], ans)
    with pytest.raises(ValueError):
        vp.Circuit.pc_opening_digests_host(n, [lf[0], 1 << (n - 2)], ans)


def test_factoring_changed_nothing_for_the_record(case):
    c, rec = case["c"], case["rec"]
    assert c.verify_full_record(rec)
    for what, off in _offsets(case).items():
        for bit in (0x01, 0x80):
            bad = bytearray(rec); bad[off] ^= bit
            assert not c.verify_full_record(bytes(bad)), what
    assert not c.verify_full_record(rec[:-1]) and not c.verify_full_record(rec + b"\0")


def test_new_symbols_are_declared_and_exported(vp):
    gpu_hdr = open(os.path.join(ROOT, "include", "vpgpu.h")).read()
    host_hdr = open(os.path.join(ROOT, "virgo-plus_amd", "host", "vphost.h")).read()
    for lib, hdr, names in ((vp.LIB_GPU, gpu_hdr, ("vp_pc_public_evals", "vp_fri_query_digests")),
                            (vp.LIB_HOST, host_hdr, ("vph_pc_public_evals_host", "vph_pc_opening_digests_host", "vph_pc_query_answer_bytes", "vph_pc_public_evals",
                                                     "vph_fri_query_digests", "vph_verify_full_record_dev", "vph_last_verify_split"))):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in names:
            assert re.search(r"\b%s\s*\(" % s, hdr), s + " is not declared"
            assert re.search(r" T %s$" % s, out, flags=re.M), s + " is not exported"
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", gpu_hdr, flags=re.S))
    assert "int vp_pc_public_evals(vp_ctx *, int n, const vp_F *point , const vp_F *pub , int n_queries, const uint64_t *leaf0, vp_F *out );" in flat
    assert "int vp_fri_query_digests(vp_ctx *, int n, int n_queries, const uint64_t *leaf0, const uint8_t *answer, uint64_t n_bytes, uint8_t *out );" in flat
    assert "VPH_VERIFY_DEVICE_LOOPS = 2" in host_hdr
    kinds = [k.strip() for k in re.search(r"enum \{ (VP_K_BETA = 0.*?), VP_K_COUNT \}", gpu_hdr, flags=re.S).group(1).replace(" = 0", "").split(",")]
    lib = vp.lib_gpu()
    for kind, name in (("VP_K_PC_POLY_EVAL", b"k_pc_poly_eval"), ("VP_K_PC_POLY_EVAL_FIN", b"k_pc_poly_eval_fin"), ("VP_K_PC_OPENING_DIGESTS", b"k_pc_opening_digests"),
                       ("VP_K_PC_OPEN_MANY", b"k_pc_open_many")):
        assert lib.vp_kernel_name(kinds.index(kind)) == name
    assert kinds.index("VP_K_PC_OPEN_MANY") == len(kinds) - 1
    for m in ("pc_public_evals", "fri_query_digests"):
        assert hasattr(vp.Session, m)
    for m in ("pc_public_evals_host", "pc_opening_digests_host"):
        assert hasattr(vp.Circuit, m)


def test_factored_loops_under_asan_ubsan(case):
    """tests/sanitize/pc_loops_main.cpp — a program of its own, built with -fsanitize=address,undefined from the host sources and run directly: the two
    factored loops on the fixture's openings, on a truncated and an over-long answer block, and the three forms of the public evaluation against each other."""
    from test_sanitizers import ENV, SAN
    out_dir = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "pc_loops_asan")
    host = os.path.join(ROOT, "virgo-plus_amd", "host")
    csrc = os.path.join(ROOT, "virgo-plus_amd", "csrc")
    src = [os.path.join(host, f) for f in ("circuit.cpp", "prover.cpp", "verifier.cpp", "vphost.cpp")] + [os.path.join(ROOT, "tests", "sanitize", "pc_loops_main.cpp")]
    deps = src + [os.path.join(host, f) for f in os.listdir(host) if f.endswith((".hpp", ".h"))]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-pthread"] + SAN + ["-o", exe] + src +
                       ["-L" + csrc, "-lvpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    lf = _leaf0_of_record(case)
    env = dict(ENV, ASAN_OPTIONS="detect_leaks=0:exitcode=99")
    r = subprocess.run([exe, os.path.join(GOLDEN, "full_record_%s.bin" % NAME), str(case["sec"]["openings"]), str(case["n"])] + [str(x) for x in lf],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "pc_loops_asan ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
