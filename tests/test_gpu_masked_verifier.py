"""GPU (-m gpu): masked commitments verified.  Every comparison is a verdict, the name of the failed check, or bytes.

  commitment level   every case of pc_masked_inputs.CASES committed through the C ABI (vp_pc_load_input, the masked commits, vp_fri_commit, vp_fri_final(_mask),
                     vp_fri_query at 33 seeded positions), then Circuit.verify_commitment on the host loops and with device=0: the reference verifier's verdicts
                     (masked_verifier_cases.REFERENCE_VERDICTS), rejects at the final mask codeword.  n19_m3000: ms = 4096, one full chunk of k_pc_poly_eval
  batched openings   n = 13, masked: vp_fri_query and vp_fri_open_many return vp_fri_open's bytes, vp_fri_query_digests the host loop's
  vp_pc_mask_evals   against its host twin at ms = 8, 64, 2048, 4096, 2^13, 2^14, 2^16 with ms < N, = N and > N (n = 9 .. 22): a partly filled chunk, one and several
                     full chunks, the transform's three paths; a short and an edge-limb mask; 1 and 33 queries with both ends of the leaf range; every refusal,
                     with a commitment in progress on the context unchanged; one k_pc_poly_eval over one row in the launch table
  protocol level     randomize(8, 12) and a custom circuit: prove_and_verify_full(mask=, pub_mask=) in the three verifier modes — one transcript (prove_protocol's),
                     one version-2 record, replayed on the host and with device=0, a flipped byte in every section rejected, a mask longer than a slice rejected,
                     and the unmasked run's version-1 record unchanged"""
import ctypes
import struct

import numpy as np
import pytest

import masked_verifier_cases as mvc
import pc_array_inputs as pai
import pc_masked_inputs as pmi
from test_gpu_masked_fast_path import Ctx

pytestmark = pytest.mark.gpu
VP_EINVAL, VP_ELIMIT = -1, -5
P = pmi.P61
VAL = mvc.VAL


def _seeded(seed, count):
    return np.random.default_rng(seed).integers(0, P, size=(count, 2), dtype=np.uint64)


def _proof_on_device(vp, c, x, r, lf):
    """masked commits, commit phase, final codewords and the answer to `lf` on the context c: the arguments of Circuit.verify_commitment"""
    n = x["n"]
    if x["pri_mask"].any():
        c.commit_private(x["pri_mask"])
        c.commit_public(x["pub"], x["pub_mask"][:x["n_pub"]])
    else:                                            # the protocol's own one-element zero mask: the unmasked entry points
        c.commit_private()
        c.commit_public(x["pub"])
    roots = c.fri_commit(r)
    fin, fm = c.finals()
    rc, ans = vp.fri_query(c.ctx, lf)
    assert rc == 0, c.err()
    root_l, root_h, inner, alls = c.state()
    return {"n": n, "claim": np.frombuffer(inner, np.uint64).copy(), "root_l": root_l, "root_h": root_h, "all_sum": np.frombuffer(alls, np.uint64).reshape(65, 2).copy(),
            "r": r, "fri_roots": roots, "final_code": np.frombuffer(fin, np.uint64).reshape(2048, 2).copy(), "final_mask": np.frombuffer(fm, np.uint64).reshape(32, 2).copy(),
            "leaf0": lf, "answer": ans, "pub": x["pub"], "pub_mask": x["pub_mask"][:x["n_pub"]], "ms": pmi.padded_length(n, x["m"])[1]}


# ---- 1. commitment level ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pmi.CASES))
def test_commitment_verdicts_are_the_references(vp, name):
    x = pmi.inputs(name)
    n = x["n"]
    c = Ctx(vp, x["values"], n)
    try:
        p = _proof_on_device(vp, c, x, _seeded(500 + n, n - 6), mvc.positions(n, 600 + n))
    finally:
        c.close()
    zero = name.endswith("_zero")                    # zero masks commit as the unmasked commitment: the verifier's ms = 1
    if zero:
        assert not p["all_sum"][64].any() and not p["final_mask"].any()
        p["ms"] = 1
    else:
        assert p["all_sum"][64].any() and p["final_mask"].any()
    want = (True, "") if mvc.REFERENCE_VERDICTS[name] else (False, "Fri msk rs code check fail")
    assert want[0] == (p["ms"] <= 1 << (n - 6))
    assert mvc.verify(vp, p) == want, "host loops"
    assert mvc.verify(vp, p, device=0) == want, "device loops"
    if want[0] and not zero:                         # the device's mask row is what decides: a changed public mask is rejected through it as well
        pm = p["pub_mask"].copy(); pm[-1, 1] ^= np.uint64(2)
        for dev in (None, 0):
            assert mvc.verify(vp, p, device=dev, pub_mask=pm) == (False, "Fri msk check consistency 0 round fail")


def test_accepts_and_rejects_both_occur():
    v = [mvc.REFERENCE_VERDICTS[k] for k in pmi.CASES]
    assert any(v) and not all(v)


# ---- 2. the batched openings on a masked commitment -------------------------------------------------------------------------------------------------------------
def test_batched_openings_of_a_masked_commitment_are_the_single_ones(vp):
    import pc_verify_ref as ref
    name = "n13_m64"
    x = pmi.inputs(name)
    n = x["n"]
    lf = mvc.positions(n, 77)
    c = Ctx(vp, x["values"], n)
    try:
        p = _proof_on_device(vp, c, x, _seeded(78, n - 6), lf)
        ans, at, reqs, singles = p["answer"], 0, [], []
        for l0 in lf:
            for o, leaf, plen in ref.query_leaves(n, l0):
                v, path = c.open1(o, leaf)
                assert len(path) == 32 * plen and ans[at:at + VAL + 32 * plen] == v + path, "vp_fri_query against vp_fri_open, oracle %d leaf %d" % (o, leaf)
                assert any(v[128 * 16:]), "the mask pair of a masked commitment"
                reqs.append((o, leaf)); singles.append((v, path))
                at += VAL + 32 * plen
        assert at == len(ans)
        v, pth, pl = c.open_many(reqs)
        for i, (sv, sp) in enumerate(singles):
            assert v[i].tobytes() == sv and pth[i, :32 * pl[i]].tobytes() == sp, "vp_fri_open_many against vp_fri_open, request %d" % i
        out = ctypes.create_string_buffer(len(lf) * (n - 4) * 64)
        la = np.array(lf, np.uint64)
        buf = ctypes.create_string_buffer(ans, len(ans))
        assert c.L.vp_fri_query_digests(c.ctx, n, len(lf), la.ctypes.data, ctypes.cast(buf, ctypes.c_void_p), len(ans), ctypes.cast(out, ctypes.c_void_p)) == 0, c.err()
        assert out.raw == vp.Circuit.pc_opening_digests_host(n, lf, ans)
    finally:
        c.close()


# ---- 3. vp_pc_mask_evals ---------------------------------------------------------------------------------------------------------------------------------------
def _mask_evals(vp, ctx, n, lf, pm, ms, n_pm=None):
    L = vp.lib_gpu()
    lf = np.ascontiguousarray(lf, dtype=np.uint64)
    pm = np.ascontiguousarray(pm, dtype=np.uint64)
    out = np.full((max(len(lf), 1), 2, 2), 0xEE, dtype=np.uint64)
    rc = L.vp_pc_mask_evals(ctx, n, pm.ctypes.data if pm.shape[0] else None, pm.shape[0] if n_pm is None else n_pm, ms, len(lf), lf.ctypes.data if len(lf) else None,
                            out.ctypes.data)
    return rc, out[:len(lf)]


def _table(vp, ctx):
    L = vp.lib_gpu()
    k = ctypes.c_int(0)
    L.vp_get_launch_stats(ctx, None, 0, ctypes.byref(k))
    arr = (vp.LaunchStat * max(k.value, 1))()
    L.vp_get_launch_stats(ctx, arr, k.value, ctypes.byref(k))
    return [(L.vp_kernel_name(e.kind).decode(), e.jobs, e.workgroups) for e in arr[:k.value]]


@pytest.fixture(scope="module")
def bare(vp):
    ctx = ctypes.c_void_p()
    assert vp.lib_gpu().vp_create(0, ctypes.byref(ctx)) == 0
    yield ctx
    vp.lib_gpu().vp_destroy(ctx)


# (n, ms): N = 2^(n-6); ms < N, = N, > N at the chunk edges of k_pc_poly_eval (4096 coefficients a chunk) and on the transform's paths (LDS up to 2^12, radix-8 from 2^13)
MASK_SIZES = [(9, 8), (12, 8), (10, 64), (12, 64), (13, 64), (14, 2048), (17, 2048), (19, 2048), (14, 4096), (18, 4096), (22, 4096), (15, 1 << 13), (19, 1 << 13),
              (21, 1 << 13), (16, 1 << 14), (20, 1 << 14), (22, 1 << 14), (18, 1 << 16), (22, 1 << 16)]


def test_the_mask_sizes_cover_every_relation_to_a_slice():
    for ms in (8, 64, 2048, 4096, 1 << 13, 1 << 14, 1 << 16):
        rel = {(ms > 1 << (n - 6)) - (ms < 1 << (n - 6)) for n, m in MASK_SIZES if m == ms}
        # (8 > N would be n < 9, where no mask is accepted; 2^16 < N would be n = 23 and more: nothing new for one row)
        assert rel == ({-1, 0} if ms == 8 else {0, 1} if ms == 1 << 16 else {-1, 0, 1}), ms
    assert all(8 <= ms <= min(1 << 16, 1 << (n - 2)) and 9 <= n <= 22 for n, ms in MASK_SIZES)


@pytest.mark.parametrize("n,ms", MASK_SIZES)
def test_mask_evals_equal_the_host_twin(vp, bare, n, ms):
    L = vp.lib_gpu()
    lf33 = mvc.positions(n, 900 + n + ms)
    masks = {"short": _seeded(901 + ms, max(1, ms // 3)), "edges": pai.EDGES[np.random.default_rng(902 + ms).integers(0, len(pai.EDGES), size=(ms, 2))],
             "one element": _seeded(903, 1)}
    L.vp_set_profiling(bare, 1)
    for what, pm in masks.items():
        for lf in (lf33, lf33[:1], lf33[-1:]):
            rc, got = _mask_evals(vp, bare, n, lf, pm, ms)
            assert rc == 0, L.vp_last_error(bare)
            assert int(got.max()) < P and got.tobytes() == vp.Circuit.pc_mask_evals_host(n, lf, pm, ms).tobytes(), (n, ms, what, len(lf))
            t = _table(vp, bare)
            ev = [e for e in t if e[0] == "k_pc_poly_eval"]
            assert len(ev) == 1 and ev[0][1] == 1 and [e[0] for e in t[-2:]] == ["k_pc_poly_eval", "k_pc_poly_eval_fin"], t
    L.vp_set_profiling(bare, 0)


def test_mask_evals_refusals_leave_the_context_unchanged(vp):
    name = "n13_m64"
    x = pmi.inputs(name)
    n = x["n"]
    lf = mvc.positions(n, 31)
    c = Ctx(vp, x["values"], n)
    try:
        p = _proof_on_device(vp, c, x, _seeded(32, n - 6), lf)
        pm = _seeded(33, 64)
        bad = pm.copy(); bad[5, 1] = P
        ok = (n, lf, pm, 64)
        refusals = [((6, [1], pm[:8], 8), VP_EINVAL, "at least 2^7"), ((26, lf, pm, 64), VP_ELIMIT, "above 2^25"), ((n, [], pm, 64), VP_EINVAL, "queries"),
                    ((n, lf * 125, pm, 64), VP_EINVAL, "queries"), ((n, [lf[0], (1 << (n - 7)) - 1], pm, 64), VP_EINVAL, "leaf"),
                    ((n, [1 << (n - 2)], pm, 64), VP_EINVAL, "leaf"), ((n, lf, bad, 64), VP_EINVAL, "non-canonical"), ((n, lf, pm[:4], 4), VP_EINVAL, "power of two"),
                    ((n, lf, pm, 96), VP_EINVAL, "power of two"), ((n, lf, pm, 1 << (n - 1)), VP_EINVAL, "power of two"), ((22, mvc.positions(22, 1), pm, 1 << 17), VP_EINVAL, "power of two"),
                    ((n, lf, pm, 32), VP_EINVAL, "1 .. ms"), ((n, lf, pm[:0], 64), VP_EINVAL, "1 .. ms")]
        assert len(lf * 125) > 4096
        for args, rc_want, word in refusals:
            rc, got = _mask_evals(vp, c.ctx, *args)
            assert rc == rc_want and word in c.err(), (args[0], args[3], rc, c.err())
            assert not len(got) or (int(got.min()), int(got.max())) == (0xEE, 0xEE), "a refused call wrote its output"
        assert _mask_evals(vp, c.ctx, n, lf, pm, 64, n_pm=0)[0] == VP_EINVAL
        L = c.L
        out = np.zeros((len(lf), 2, 2), np.uint64)
        la = np.array(lf, np.uint64)
        assert L.vp_pc_mask_evals(c.ctx, n, pm.ctypes.data, 64, 64, len(lf), None, out.ctypes.data) == VP_EINVAL
        assert L.vp_pc_mask_evals(c.ctx, n, pm.ctypes.data, 64, 64, len(lf), la.ctypes.data, None) == VP_EINVAL
        assert L.vp_pc_mask_evals(None, n, pm.ctypes.data, 64, 64, len(lf), la.ctypes.data, out.ctypes.data) == VP_EINVAL
        rc, got = _mask_evals(vp, c.ctx, *ok)
        assert rc == 0 and got.tobytes() == vp.Circuit.pc_mask_evals_host(*ok).tobytes()
        rc, got = _mask_evals(vp, c.ctx, 16, mvc.positions(16, 2), pm, 1 << 13)                      # another size than the commitment's, on its context
        assert rc == 0 and got.tobytes() == vp.Circuit.pc_mask_evals_host(16, mvc.positions(16, 2), pm, 1 << 13).tobytes()
        # the commitment in progress is as it was: the same openings, the same final codewords
        rc, ans = vp.fri_query(c.ctx, lf)
        assert rc == 0 and ans == p["answer"]
        fin, fm = c.finals()
        assert fin == p["final_code"].tobytes() and fm == p["final_mask"].tobytes()
    finally:
        c.close()


# ---- 4. protocol level -----------------------------------------------------------------------------------------------------------------------------------------
def _sections(rec, n, reps, n_pub):
    lg = n - 6
    per_query = 2 * (VAL + 32 * (n - 1)) + sum(VAL + 32 * (n - 2 - k) for k in range(lg))
    mask_len = 8 + 16 * n_pub + 32 * 16
    openings = len(rec) - reps * per_query
    mask = openings - mask_len
    final = mask - 2048 * 16
    roots = final - 32 * lg
    fft = roots - 16 * (64 + 3 * (2 * lg * lg + 2 * lg + 6) + 2 + 2 * lg)
    return {"header": 0, "transcript": 16, "fft_gkr": fft, "roots": roots, "final": final, "mask": mask, "openings": openings}


def _protocol(vp, c, reps):
    n = c.layer_bitlen(0)
    N = 1 << (n - 6)
    f = pmi.family("short_pub", n, N)
    pri, pub = f["pri_mask"], f["pub_mask"]
    s = vp.Session(c)
    try:
        tr_plain, ok_plain, _ = s.prove_and_verify_full(reps=reps)
        rec_plain = s.last_full_record()
        assert ok_plain and struct.unpack_from("<4I", rec_plain) == (0x52465056, 1, n, reps)
        runs = []
        for kw in ({}, {"batched_openings": True}, {"device_verifier": True}):
            if kw.get("device_verifier"):
                s.set_profiling(1)
            tr, ok, _ = s.prove_and_verify_full(reps=reps, mask=pri, pub_mask=pub, **kw)
            assert ok, kw
            runs.append((tr, s.last_full_record()))
        launches = [e["kernel"] for e in s.verifier_launch_stats()]
        s.set_profiling(0)
        assert launches.count("k_pc_poly_eval") == 2 and launches.count("k_pc_poly_eval_fin") == 2 and launches.count("k_pc_opening_digests") == 1, launches
        assert runs[0] == runs[1] == runs[2]
        tr, rec = runs[0]
        assert tr != tr_plain and tr[32:-(32 + 16 + 65 * 16)] == tr_plain[32:-(32 + 16 + 65 * 16)], "the same GKR slice under another commitment"
        assert any(tr[-16:]), "all_sum[64] of a masked run"
        assert struct.unpack_from("<4I", rec) == (0x52465056, 2, n, reps)
        sec = _sections(rec, n, reps, pub.shape[0])
        assert rec[16:16 + len(tr)] == tr and sec["fft_gkr"] == 16 + len(tr)
        assert struct.unpack_from("<2I", rec, sec["mask"]) == (N, pub.shape[0]) and rec[sec["mask"] + 8:sec["mask"] + 8 + 16 * pub.shape[0]] == pub.tobytes()
        assert any(rec[sec["openings"] - 32 * 16:sec["openings"]]), "the final mask codeword of a masked run"
        # the one-pass prover writes the same transcript
        s.draw_protocol_tape()
        assert s.prove_protocol(mask=pri, pub_mask=pub)[0] == tr
        # a zero mask is the run without one, and the unmasked record is what it was
        tr0, ok0, _ = s.prove_and_verify_full(reps=reps, mask=np.zeros_like(pri), pub_mask=pub)
        assert ok0 and tr0 == tr_plain and s.last_full_record() == rec_plain
        tr1, ok1, _ = s.prove_and_verify_full(reps=reps)
        assert ok1 and tr1 == tr_plain and s.last_full_record() == rec_plain
        # a mask longer than a slice's message: proved as the reference proves it, rejected as the reference rejects it
        long_mask = pmi.family("uniform", n, 2 * N)
        _, ok2, _ = s.prove_and_verify_full(reps=reps, mask=long_mask["pri_mask"], pub_mask=long_mask["pub_mask"], batched_openings=True)
        assert not ok2
        with pytest.raises(RuntimeError, match="vp_commit_private_masked"):                            # a refusal is no verdict
            s.prove_and_verify_full(reps=reps, mask=_seeded(5, 3), pub_mask=pub)
    finally:
        s.close()
    assert c.verify_full_record(rec) and c.verify_full_record(rec, device=0)
    assert c.verify_full_record(rec_plain) and c.verify_full_record(rec_plain, device=0)
    flips = {"version": 4, "gkr": 16 + len(tr) // 2, "all_sum[64]": 16 + len(tr) - 3, "fft_gkr": sec["fft_gkr"] + 5, "fri root": sec["roots"] + 4, "final": sec["final"] + 8,
             "ms": sec["mask"] + 1, "public mask length": sec["mask"] + 4, "public mask": sec["mask"] + 8 + 3, "final mask": sec["openings"] - 9,
             "value": sec["openings"] + 40, "mask pair": sec["openings"] + 129 * 16 + 2, "path leaf digest": len(rec) - 1}
    for what, off in flips.items():
        bad = bytearray(rec); bad[off] ^= 0x04
        assert not c.verify_full_record(bytes(bad)), what
        assert not c.verify_full_record(bytes(bad), device=0), what
    for bad in (rec[:-1], rec + b"\0", rec[:sec["mask"]] + rec[sec["openings"]:]):
        assert not c.verify_full_record(bad) and not c.verify_full_record(bad, device=0)


def test_protocol_with_masks_randomize_8_12(vp):
    c = vp.Circuit.randomize(8, 12, seed=1)
    _protocol(vp, c, 33)
    c.close()


def test_protocol_with_masks_custom_circuit(vp, golden):
    import custom_circuits as cc
    g = golden["custom_a"]
    c = vp.Circuit.custom(*cc.make(g["custom"]["seed"], g["custom"]["sizes"]))
    _protocol(vp, c, 5)
    c.close()
