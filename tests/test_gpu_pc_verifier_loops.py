"""GPU: the commitment verifier's two heavy loops on the device — vp_pc_public_evals (k_pc_poly_eval + k_pc_poly_eval_fin behind the existing eq
builders and inverse transforms) and vp_fri_query_digests (k_pc_opening_digests) — against the host loops verifyPoly itself runs (which
tests/test_pc_verifier_loops_host.py pins to the definitions), and the verifier that uses them (verifier::poly_dev, VPH_VERIFY_DEVICE_LOOPS,
vph_verify_full_record_dev).  Every comparison is equality of bytes.

Sizes, and what each is there for (N = 2^(n-6) coefficients per slice, M = 2^(n-1)):
  public evaluation
    n = 7 .. 12    N = 2 .. 64: k_ntt_lds below one wave's worth of points; N = 2 is ONE coefficient pair (a single live thread in the workgroup)
    n = 14, 16     N = 256, 1024: several pairs per thread, still one workgroup per row
    n = 19         N = 2^13: the largest in-LDS transform; two workgroups per row (a run boundary inside a row)
    n = 20         N = 2^14: the radix-8 pair
    n = 24         N = 2^18: the long transform, 64 workgroups per row, leaf exponents beyond 2^32 before reduction — once, with a single query
    queries        1, 2, 5 (the leaf families of pc_verify_cases) and 33 with repeats: one and several query groups per launch
  opening digests
    n = 7 .. 12, 15, 19   paths of 5 .. 17 digests, the last FRI level's 16 leaves at every size; 1 position and 33 (more than one wave of openings)"""
import ctypes
import os

import numpy as np
import pytest

import pc_verify_cases as cases
import test_gpu_query_phase as qp
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
P = (1 << 61) - 1
VP_EINVAL, VP_ELIMIT = -1, -5
VAL = 130 * 16


def _evals(vp, ctx, n, lf, point=None, pub=None, n_queries=None):
    """(rc, (nq, 2, 64, 2) uint64) of the raw call on a vp_ctx*."""
    lf = np.ascontiguousarray(lf, dtype=np.uint64)
    nq = len(lf) if n_queries is None else n_queries
    out = np.zeros((max(nq, 1), 2, 64, 2), dtype=np.uint64)
    rc = vp.lib_gpu().vp_pc_public_evals(ctx, n, None if point is None else point.ctypes.data, None if pub is None else pub.ctypes.data, nq,
                                         lf.ctypes.data if len(lf) else None, out.ctypes.data)
    return rc, out[:max(nq, 0)]


def _digests(vp, ctx, n, lf, answer, n_bytes=None):
    lf = np.ascontiguousarray(lf, dtype=np.uint64)
    buf = ctypes.create_string_buffer(bytes(answer), max(len(answer), 1))
    out = ctypes.create_string_buffer(max(len(lf) * (n - 4) * 64, 64))
    rc = vp.lib_gpu().vp_fri_query_digests(ctx, n, len(lf), lf.ctypes.data, ctypes.cast(buf, ctypes.c_void_p), len(answer) if n_bytes is None else n_bytes,
                                           ctypes.cast(out, ctypes.c_void_p))
    return rc, out.raw[:len(lf) * (n - 4) * 64]


def _table(vp, ctx):
    L = vp.lib_gpu()
    k = ctypes.c_int(0)
    L.vp_get_launch_stats(ctx, None, 0, ctypes.byref(k))
    arr = (vp.LaunchStat * max(k.value, 1))()
    L.vp_get_launch_stats(ctx, arr, k.value, ctypes.byref(k))
    return [L.vp_kernel_name(e.kind).decode() for e in arr[:k.value]]


@pytest.fixture(scope="module")
def bare(vp):
    """A context with no circuit, no witness and no commitment: all the two calls need."""
    ctx = qp._ctx(vp)
    yield ctx
    vp.lib_gpu().vp_destroy(ctx)


# ---- 1. vp_pc_public_evals = the host loop --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 8, 9, 10, 11, 12, 14, 16])
def test_public_evals_equal_the_host_loop_small(vp, bare, n):
    L = vp.lib_gpu()
    L.vp_set_profiling(bare, 1)
    lf = cases.leaves(n)
    for name, pt in cases.points(n).items():
        want = vp.Circuit.pc_public_evals_host(n, lf, point=pt)
        rc, got = _evals(vp, bare, n, lf, point=pt)
        assert rc == 0, L.vp_last_error(bare)
        assert int(got.max()) < P and got.tobytes() == want.tobytes(), (n, name)
        t = _table(vp, bare)
        assert t.count("k_pc_poly_eval") == 1 and t.count("k_pc_poly_eval_fin") == 1 and t[-2:] == ["k_pc_poly_eval", "k_pc_poly_eval_fin"], t
    vec = cases.general_vector(n)
    for nq in (1, 2, len(lf)):
        rc, got = _evals(vp, bare, n, lf[:nq], pub=vec)
        assert rc == 0, L.vp_last_error(bare)
        assert got.tobytes() == vp.Circuit.pc_public_evals_host(n, lf[:nq], pub=vec).tobytes(), (n, "general vector", nq)
    t = _table(vp, bare)
    assert t.count("k_pc_poly_eval") == 1 and t.count("k_pc_poly_eval_fin") == 1, t
    l33 = cases.leaves_33(n)
    pt = cases.points(n)["uniform"]
    rc, got = _evals(vp, bare, n, l33, point=pt)
    assert rc == 0 and got.tobytes() == vp.Circuit.pc_public_evals_host(n, l33, point=pt).tobytes(), (n, "33 queries, point")
    assert got[7].tobytes() == got[3].tobytes() and got[32].tobytes() == got[0].tobytes()
    rc, got = _evals(vp, bare, n, l33, pub=vec)
    assert rc == 0 and got.tobytes() == vp.Circuit.pc_public_evals_host(n, l33, pub=vec).tobytes(), (n, "33 queries, vector")
    L.vp_set_profiling(bare, 0)


@pytest.mark.parametrize("n", [19, 20])
def test_public_evals_equal_the_host_loop_large(vp, bare, n):
    L = vp.lib_gpu()
    lf = cases.leaves(n)
    pts = cases.points(n)
    for name, pt in pts.items():                                        # every point family, with the leaf families (the plain host loop)
        rc, got = _evals(vp, bare, n, lf, point=pt)
        assert rc == 0, L.vp_last_error(bare)
        assert got.tobytes() == vp.Circuit.pc_public_evals_host(n, lf, point=pt).tobytes(), (n, name)
    vec = cases.general_vector(n)
    l33 = cases.leaves_33(n)
    rc, got = _evals(vp, bare, n, l33, pub=vec)
    assert rc == 0, L.vp_last_error(bare)
    assert got.tobytes() == vp.Circuit.pc_public_evals_host(n, l33, pub=vec).tobytes(), (n, "general vector, 33 queries")
    for nq in (1, 2):
        rc, got = _evals(vp, bare, n, lf[:nq], pub=vec)
        assert rc == 0 and got.tobytes() == vp.Circuit.pc_public_evals_host(n, lf[:nq], pub=vec).tobytes(), (n, "general vector", nq)
    for name in ("uniform", "edge limbs"):
        rc, got = _evals(vp, bare, n, l33, point=pts[name])
        assert rc == 0 and got.tobytes() == vp.Circuit.pc_public_evals_host(n, l33, point=pts[name], tensor=True).tobytes(), (n, name, "33 queries")


def test_public_evals_long_transform_single_query(vp, bare):
    """n = 24: slices of 2^18 coefficients (the long transform).  The host side takes the one-transform form, which the CPU file pins to the plain loop;
    the vector form is given the point's own eq table (built by the device's eq builder, vp_test_beta), so its 64 transforms must give the same values."""
    n = 24
    L = vp.lib_gpu()
    L.vp_set_profiling(bare, 1)
    for name, leaf in (("uniform", cases.leaves(n)[2]), ("edge limbs", (1 << (n - 2)) - 1)):
        pt = cases.points(n)[name]
        want = vp.Circuit.pc_public_evals_host(n, [leaf], point=pt, tensor=True)
        rc, got = _evals(vp, bare, n, [leaf], point=pt)
        assert rc == 0, L.vp_last_error(bare)
        assert got.tobytes() == want.tobytes(), name
    t = _table(vp, bare)
    assert "k_ntt_long_merge" in t and t.count("k_pc_poly_eval") == 1, t
    tab = np.zeros((1 << n, 2), dtype=np.uint64)
    one = np.array([1, 0], dtype=np.uint64)
    assert L.vp_test_beta(bare, pt.ctypes.data, n, one.ctypes.data, tab.ctypes.data) == 0
    rc, got = _evals(vp, bare, n, [leaf], pub=tab)
    assert rc == 0, L.vp_last_error(bare)
    assert got.tobytes() == want.tobytes()
    t = _table(vp, bare)
    assert "k_ntt_long_merge" in t and t.count("k_pc_poly_eval") == 1 and t.count("k_pc_poly_eval_fin") == 1, t
    L.vp_set_profiling(bare, 0)


# ---- 2. vp_fri_query_digests on real answers --------------------------------------------------------------------------------------------------
def _commit_with_roots(vp, ctx, n, seed):
    """qp._commit, keeping the roots: [root_l, root_h, FRI roots ...]."""
    L = vp.lib_gpu()
    vals = qp._seeded(n, seed)
    assert L.vp_pc_load_input(ctx, vals.ctypes.data, vals.shape[0], n) == 0, L.vp_last_error(ctx)
    rl, rh = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    assert L.vp_commit_private(ctx, ctypes.cast(rl, ctypes.c_void_p)) == 0, L.vp_last_error(ctx)
    pub = qp._seeded(n, seed + 1)
    inner, alls = np.zeros(2, np.uint64), np.zeros((65, 2), np.uint64)
    assert L.vp_commit_public(ctx, pub.ctypes.data, pub.shape[0], inner.ctypes.data, alls.ctypes.data, ctypes.cast(rh, ctypes.c_void_p)) == 0, L.vp_last_error(ctx)
    r = qp._seeded(n, seed + 2, n - 6)
    roots = ctypes.create_string_buffer(32 * (n - 6))
    assert L.vp_fri_commit(ctx, r.ctypes.data, n - 6, ctypes.cast(roots, ctypes.c_void_p)) == 0, L.vp_last_error(ctx)
    return [rl.raw, rh.raw] + [roots.raw[32 * k:32 * k + 32] for k in range(n - 6)]


def _openings(n, nq):
    """(start, path digests) of every opening of an answer block."""
    out, at = [], 0
    for _ in range(nq):
        for o in range(n - 4):
            plen = n - 1 if o < 2 else n - 2 - (o - 2)
            out.append((at, plen))
            at += VAL + 32 * plen
    return out


@pytest.mark.parametrize("n", [7, 8, 9, 10, 11, 12, 15, 19])
def test_query_digests_on_real_answers(vp, bare, n):
    L = vp.lib_gpu()
    ctx = qp._ctx(vp)
    try:
        roots = _commit_with_roots(vp, ctx, n, 700 + n)
        for lf in ([cases.leaves(n)[2]], cases.leaves_33(n)):
            rc, ans = vp.fri_query(ctx, lf)
            assert rc == 0 and len(ans) == vp.Circuit.pc_query_answer_bytes(n, len(lf))
            host = vp.Circuit.pc_opening_digests_host(n, lf, ans)
            L.vp_set_profiling(ctx, 1)
            rc, dev = _digests(vp, ctx, n, lf, ans)
            assert rc == 0, L.vp_last_error(ctx)
            assert _table(vp, ctx) == ["k_pc_opening_digests"]
            L.vp_set_profiling(ctx, 0)
            assert dev == host
            ops = _openings(n, len(lf))
            for i, (at, plen) in enumerate(ops):
                assert dev[64 * i:64 * i + 32] == ans[at + VAL + 32 * (plen - 1):at + VAL + 32 * plen], (i, "leaf digest")
                assert dev[64 * i + 32:64 * i + 64] == roots[i % (n - 4)], (i, "root")
            rc, dev2 = _digests(vp, bare, n, lf, ans)                    # a context with no commitment: the same answer
            assert rc == 0 and dev2 == host

            def changed(off):
                bad = bytearray(ans); bad[off] ^= 0x10
                rc, d = _digests(vp, bare, n, lf, bytes(bad))
                assert rc == 0 and d == vp.Circuit.pc_opening_digests_host(n, lf, bytes(bad))
                return [k for k in range(2 * len(ops)) if d[32 * k:32 * k + 32] != host[32 * k:32 * k + 32]]

            for i in (0, len(ops) // 2, len(ops) - 1):
                at, plen = ops[i]
                assert changed(at + 9) == [2 * i, 2 * i + 1], (i, "value byte")
                assert changed(at + VAL + 1) == [2 * i + 1], (i, "path byte, lowest height")
                assert changed(at + VAL + 32 * (plen - 2) + 31) == [2 * i + 1], (i, "path byte, highest height")
                assert changed(at + VAL + 32 * (plen - 1)) == [], (i, "path[depth] is not read")
    finally:
        L.vp_destroy(ctx)


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch_and_leave_a_commitment_alone(vp):
    L = vp.lib_gpu()
    n = 12
    ctx, undisturbed = qp._ctx(vp), qp._ctx(vp)
    try:
        L.vp_set_profiling(ctx, 1)
        pt = cases.points(n)["uniform"]
        vec = cases.general_vector(n)
        lf = cases.leaves(n)
        N, M = 1 << (n - 6), 1 << (n - 1)
        bad_pt = pt.copy(); bad_pt[n - 1, 0] = P
        bad_vec = vec.copy(); bad_vec[-1, 1] = (1 << 64) - 1
        refused = [
            (_evals(vp, ctx, n, lf, point=bad_pt)[0], (VP_EINVAL,), "non-canonical point limb"),
            (_evals(vp, ctx, n, lf, pub=bad_vec)[0], (VP_EINVAL,), "non-canonical vector limb"),
            (_evals(vp, ctx, n, [N // 2 - 1], point=pt)[0], (VP_EINVAL,), "leaf below N / 2"),
            (_evals(vp, ctx, n, lf[:2] + [M // 2], point=pt)[0], (VP_EINVAL,), "leaf at M / 2"),
            (_evals(vp, ctx, n, lf, point=pt, pub=vec)[0], (VP_EINVAL,), "both point and pub"),
            (_evals(vp, ctx, n, lf)[0], (VP_EINVAL,), "neither point nor pub"),
            (_evals(vp, ctx, 6, [1], point=pt)[0], (VP_EINVAL, VP_ELIMIT), "n = 6"),
            (_evals(vp, ctx, 26, [1 << 20], point=np.zeros((26, 2), dtype=np.uint64))[0], (VP_EINVAL, VP_ELIMIT), "n = 26"),
            (_evals(vp, ctx, n, lf, point=pt, n_queries=0)[0], (VP_EINVAL,), "no query"),
            (_evals(vp, ctx, n, [lf[0]] * 4097, point=pt)[0], (VP_EINVAL,), "4097 queries"),
        ]
        size = vp.Circuit.pc_query_answer_bytes(n, 2)
        blk = bytes(size)
        refused += [
            (_digests(vp, ctx, n, lf[:2], blk[:-32])[0], (VP_EINVAL,), "n_bytes short"),
            (_digests(vp, ctx, n, lf[:2], blk + bytes(32), n_bytes=size + 32)[0], (VP_EINVAL,), "n_bytes long"),
            (_digests(vp, ctx, n, lf[:1], blk)[0], (VP_EINVAL,), "n_bytes of another query count"),
            (_digests(vp, ctx, n, [lf[0], M // 2], blk)[0], (VP_EINVAL,), "leaf out of range"),
            (_digests(vp, ctx, 6, [1], bytes(64), n_bytes=64)[0], (VP_EINVAL, VP_ELIMIT), "n = 6"),
            (_digests(vp, ctx, 26, [1 << 20], bytes(64), n_bytes=64)[0], (VP_EINVAL, VP_ELIMIT), "n = 26"),
        ]
        for rc, allowed, what in refused:
            assert rc in allowed, (what, rc)
        assert _table(vp, ctx) == [], "a refused call launched something"
        # a commitment in progress on the same context: refusals and good calls between its steps, the same roots and openings as an undisturbed one
        vals = qp._seeded(n, 900)
        roots = {}
        for c in (ctx, undisturbed):
            out = []
            assert L.vp_pc_load_input(c, vals.ctypes.data, vals.shape[0], n) == 0
            rl, rh = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
            assert L.vp_commit_private(c, ctypes.cast(rl, ctypes.c_void_p)) == 0
            if c is ctx:
                assert _evals(vp, c, n, lf, point=bad_pt)[0] == VP_EINVAL
                rc, got = _evals(vp, c, n, lf, point=pt)
                assert rc == 0 and got.tobytes() == vp.Circuit.pc_public_evals_host(n, lf, point=pt).tobytes()
                rc, got = _evals(vp, c, 9, cases.leaves(9), pub=cases.general_vector(9))           # another size than the commitment's
                assert rc == 0 and got.tobytes() == vp.Circuit.pc_public_evals_host(9, cases.leaves(9), pub=cases.general_vector(9)).tobytes()
            pub = qp._seeded(n, 901)
            inner, alls = np.zeros(2, np.uint64), np.zeros((65, 2), np.uint64)
            assert L.vp_commit_public(c, pub.ctypes.data, pub.shape[0], inner.ctypes.data, alls.ctypes.data, ctypes.cast(rh, ctypes.c_void_p)) == 0
            if c is ctx:
                rc, got = _evals(vp, c, n, lf, pub=vec)
                assert rc == 0 and got.tobytes() == vp.Circuit.pc_public_evals_host(n, lf, pub=vec).tobytes()
                assert _digests(vp, c, n, lf[:2], blk[:-32])[0] == VP_EINVAL
                assert _digests(vp, c, n, lf[:2], blk)[0] == 0
            r = qp._seeded(n, 902, n - 6)
            fr = ctypes.create_string_buffer(32 * (n - 6))
            assert L.vp_fri_commit(c, r.ctypes.data, n - 6, ctypes.cast(fr, ctypes.c_void_p)) == 0
            rc, ans = vp.fri_query(c, lf)
            assert rc == 0
            roots[c is ctx] = (rl.raw, rh.raw, fr.raw, inner.tobytes(), alls.tobytes(), ans)
        assert roots[True] == roots[False]
    finally:
        L.vp_destroy(ctx); L.vp_destroy(undisturbed)


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------------
def _end_to_end(vp, c, reps, gold, flips):
    s = vp.Session(c)
    try:
        tr0, ok0, t0 = s.prove_and_verify_full(reps=reps)
        rec0 = s.last_full_record()
        tr1, ok1, _ = s.prove_and_verify_full(reps=reps, batched_openings=True)
        rec1 = s.last_full_record()
        s.set_profiling(1)
        tr2, ok2, t2 = s.prove_and_verify_full(reps=reps, device_verifier=True)
        rec2 = s.last_full_record()
        launches = s.verifier_launch_stats()
        s.set_profiling(0)
        assert ok0 and ok1 and ok2
        assert tr0 == tr1 == tr2 == gold and rec0 == rec1 == rec2
        names = [e["kernel"] for e in launches]
        # the predicate sums show through their bracketed half-table launch (the bucket kernels behind it carry no launch kind)
        assert names.count("k_pc_poly_eval") == 1 and names.count("k_pc_opening_digests") == 1 and "k_beta_half_direct" in names, names
        assert names.index("k_beta_half_direct") < names.index("k_pc_poly_eval") < names.index("k_pc_opening_digests")
        assert t0["verify_public_eval_sec"] > 0 and t0["verify_digests_sec"] > 0 and t2["verify_public_eval_sec"] > 0 and t2["verify_digests_sec"] > 0
    finally:
        s.close()
    assert c.verify_full_record(rec2) and c.verify_full_record(rec2, device=0)
    for what, off in flips(rec2).items():
        bad = bytearray(rec2); bad[off] ^= 0x04
        assert not c.verify_full_record(bytes(bad)), what
        assert not c.verify_full_record(bytes(bad), device=0), what
    assert not c.verify_full_record(rec2[:-1], device=0) and not c.verify_full_record(rec2 + b"\0", device=0)
    return rec2


def test_device_verifier_end_to_end_custom_a(vp, golden):
    import custom_circuits as cc
    import test_query_record_host as rh
    g = golden["custom_a"]
    c = vp.Circuit.custom(*cc.make(g["custom"]["seed"], g["custom"]["sizes"]))
    gold = open(os.path.join(GOLDEN, g["transcript"]), "rb").read()
    fixture = open(os.path.join(GOLDEN, "full_record_custom_a.bin"), "rb").read()
    n, lg, reps = 10, 4, 2
    per_query = 2 * (VAL + 32 * (n - 1)) + sum(VAL + 32 * (n - 2 - k) for k in range(lg))
    sec = {"header": 0, "transcript": 16, "fft_gkr": 16 + len(gold)}
    sec["roots"] = sec["fft_gkr"] + 16 * (64 + 3 * (2 * lg * lg + 2 * lg + 6) + 2 + 2 * lg)
    sec["final"] = sec["roots"] + 32 * lg
    sec["openings"] = sec["final"] + 2048 * 16
    sec["end"] = sec["openings"] + reps * per_query
    case = {"sec": sec, "g": g, "n": n, "gold": gold}
    rec = _end_to_end(vp, c, reps, gold, lambda r: rh._offsets(case))          # the flips of tests/test_query_record_host.py
    assert rec == fixture
    c.close()


def test_device_verifier_end_to_end_sha256(vp, golden, pws_path):
    c = vp.Circuit.from_pws(pws_path, 1, seed=1)
    n = c.layer_bitlen(0)
    lg = n - 6
    gold = open(os.path.join(GOLDEN, golden["sha256_x1"]["transcript"]), "rb").read()
    fft = 16 + len(gold)
    roots = fft + 16 * (64 + 3 * (2 * lg * lg + 2 * lg + 6) + 2 + 2 * lg)
    final = roots + 32 * lg
    openings = final + 2048 * 16

    def flips(rec):
        return {"gkr": 16 + len(gold) // 2, "fft_gkr": fft + 5, "fri root": roots + 4, "final": final + 8, "value": openings + 40, "path leaf digest": len(rec) - 1}
    _end_to_end(vp, c, 33, gold, flips)
    c.close()


def test_cli_checks_a_record_with_the_device_verifier(vp, pws_path, tmp_path):
    """virgo_plus_run --check-record FILE circuit.pws --device-verifier: the replay with the device loops accepts the record the command line wrote
    and rejects a copy with one byte of an opened value, and one byte of a path, changed."""
    import subprocess
    f = tmp_path / "cli_record.bin"
    out = subprocess.run([vp.CLI, pws_path, "--record", str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0 and "Verification pass" in out.stderr, out.stderr[-1500:]
    rec = f.read_bytes()
    chk = subprocess.run([vp.CLI, "--check-record", str(f), pws_path, "--device-verifier", "--device", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert chk.returncode == 0 and "Verification pass" in chk.stderr, chk.stderr[-1500:]
    for off in (len(rec) - 40, len(rec) - 33 * vp.Circuit.pc_query_answer_bytes(13, 1) + 24):
        bad = bytearray(rec); bad[off] ^= 1
        g = tmp_path / "cli_record_bad.bin"
        g.write_bytes(bytes(bad))
        chk = subprocess.run([vp.CLI, "--check-record", str(g), pws_path, "--device-verifier"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert chk.returncode == 1 and "Verification fail" in chk.stderr, (off, chk.stderr[-500:])
