"""GPU (-m gpu): the commitment leaves the input layer's all-zero slices out of its transforms, products and folds (csrc/vp_pc_live.h: live = ceil(n_used / N)
of the 64 slices) and keeps their regions as zero bytes for the hashes and openings, which read all 64.  Inputs go in through vp_pc_load_input(values, n_used,
n); expectations are the oracle's orc_commitment_array, byte for byte — root_l, root_h, inner, all 65 all_sum, every FRI root, the final codeword — and every
opening (l, h, every level; a leaf carries one value pair of each slice, live and dead) verifies against the ORACLE's root with zeros in the dead slices.  At the
flagship's kernels (n = 21) the default is compared with VP_PC_LIVE=0, and on the SHA-256 x64 circuit (a real witness: the paired encode at stride 29) with the
reference's goldens, the launch table showing that the skip ran."""
import ctypes
import os

import numpy as np
import pytest

import pc_array_inputs as pai
from conftest import GOLDEN
from test_gpu_commitment_ladder import Ctx, _compare, _run
from test_gpu_sharded_dropin_commitment import _fri_golden, _opening_ok

pytestmark = pytest.mark.gpu

# live -> n_used in slices of N entries: inside the last live slice, except the two that sit on and just behind a slice boundary
_LIVE = {1: lambda N: 1, 2: lambda N: N + 1, 3: lambda N: 2 * N + N // 2, 33: lambda N: 32 * N + N // 2 + 1, 57: lambda N: 56 * N + N // 4 + 1,
         63: lambda N: 63 * N - 1, 64: lambda N: 64 * N, "57N": lambda N: 57 * N, "57N+1": lambda N: 57 * N + 1}
_WANT_LIVE = {"57N": 57, "57N+1": 58}


def _inputs(n, n_used, seed, real=False):
    """random values in the first n_used entries (complex, or real), zero behind them; a public vector that is no tensor; n - 6 fold challenges"""
    rng = np.random.default_rng(seed)
    size = 1 << n
    uni = lambda cnt: rng.integers(0, pai.P61, size=(cnt, 2), dtype=np.uint64)
    values = uni(size)
    if real:
        values[:, 1] = 0
    values[n_used:] = 0
    return {"n": n, "n_used": n_used, "values": np.ascontiguousarray(values), "pub": uni(size), "r": uni(n - 6)}


_ORACLE = {}          # (n, n_used, seed) -> the oracle's record, computed once and shared


def _expected(ob, x, seed):
    key = (x["n"], x["n_used"], seed)
    if key not in _ORACLE:
        _ORACLE[key] = pai.oracle_record(ob.lib(), x["values"], x["n_used"], x["pub"], x["n"], x["r"])
    return pai.split_record(_ORACLE[key], x["n"])


def _live_of(x):
    N = 1 << (x["n"] - 6)
    return min(64, (x["n_used"] + N - 1) // N)


def _check_openings(cx, want, live, what):
    """l, h and every level at the first leaf, the last and one inside: the device's values and path verify against the oracle's root; the pairs of the dead
    slices are zero (a leaf's 65 pairs are one per slice and the mask's), those of the live slices of l are not"""
    n, ln = cx.n, cx.ln
    for oracle in range(2 + ln):
        n_leaves = 1 << (n - 2) if oracle < 2 else 16 << (ln - 1 - (oracle - 2))
        root = want["root_l"] if oracle == 0 else want["root_h"] if oracle == 1 else want["roots"][oracle - 2]
        for leaf in (0, n_leaves - 1, n_leaves // 3 + 1):
            rc, vals, path = cx.open(oracle, leaf)
            assert rc == 0, (what, oracle, leaf, cx.err())
            assert _opening_ok(root, leaf, vals, path), "%s: opening of oracle %d at leaf %d" % (what, oracle, leaf)
            assert not vals[2 * live:].any(), "%s: oracle %d, leaf %d: a dead slice's pair is not zero" % (what, oracle, leaf)
            if oracle == 0:
                assert all(vals[2 * s:2 * s + 2].any() for s in range(live)), "%s: l, leaf %d: a live slice's pair is zero" % (what, leaf)


def _case(vp, ob, x, seed, passes, what):
    want = _expected(ob, x, seed)
    live = _live_of(x)
    alls = np.frombuffer(want["public"][16:], np.uint64).reshape(65, 2)
    assert not alls[live:].any() and alls[:live].any(axis=1).all()           # the oracle agrees about which slices are dead
    for one_pass in passes:
        got, cx = _run(vp, x, lambda c: c.commit_public(x["pub"]), one_pass)
        try:
            _compare(got, want, "%s, %d challenges in one pass" % (what, one_pass))
            _check_openings(cx, want, live, "%s, %d challenges in one pass" % (what, one_pass))
        finally:
            cx.close()


@pytest.mark.parametrize("case", list(_LIVE))
@pytest.mark.parametrize("n", [9, 12])
def test_live_boundaries_vs_oracle(vp, ob, n, case):
    """live = 1, 2, 3, 33, 57, 63, 64, and n_used on the boundary 57 N and one behind it (live 58): k_ntt_lds over `live` rows, k_fri_fold0_vo and k_fri_fold with a
    partial group of four slices at live = 1, 2, 3, 33, 57 and 63 — the one-pass phase, and 2 (and at n = 12 also 3) challenges in one pass with vp_fri_step for the rest."""
    N = 1 << (n - 6)
    x = _inputs(n, _LIVE[case](N), 7000 + n)
    assert _live_of(x) == _WANT_LIVE.get(case, case)
    _case(vp, ob, x, 7000 + n, [n - 6, 2] + ([3] if n == 12 else []), "n=%d live=%s" % (n, case))


@pytest.mark.parametrize("live", [57, 5])
def test_three_fold_kernel_and_split_transforms_vs_oracle(vp, ob, live):
    """n = 15: k_fri_fold0_vo3<false, 1> (a partial group at both counts) and the transforms of 2^9 points, one pass."""
    n, N = 15, 1 << 9
    x = _inputs(n, (live - 1) * N + 3, 7100 + live)
    assert _live_of(x) == live
    _case(vp, ob, x, 7100 + live, [n - 6], "n=15 live=%d" % live)


def test_reloaded_context_keeps_no_stale_data(vp, ob):
    """One context: live = 64 through the whole commit phase, then vp_pc_load_input with live = 5, then live = 40.  After each load everything equals the
    oracle's (and so a fresh context's): a dead region that kept values of the larger commitment would change the roots and the final codeword."""
    n, N = 12, 1 << 6
    sets = [_inputs(n, u, 7200 + i) for i, u in enumerate((64 * N, 4 * N + 1, 39 * N + 7))]
    assert [_live_of(x) for x in sets] == [64, 5, 40]
    cx = Ctx(vp, sets[0])
    try:
        for i, x in enumerate(sets):
            if i:
                assert cx.L.vp_pc_load_input(cx.c, x["values"].ctypes.data, x["n_used"], n) == 0, cx.err()
            got = {"root_l": cx.commit_private()}
            got["root_h"], got["public"] = cx.commit_public(x["pub"])
            got["roots"] = cx.fri_commit(x["r"])
            rc, got["final"] = cx.fri_final_rc()
            assert rc == 0, cx.err()
            want = _expected(ob, x, 7200 + i)
            _compare(got, want, "load %d (live %d)" % (i, _live_of(x)))
            _check_openings(cx, want, _live_of(x), "load %d (live %d)" % (i, _live_of(x)))
    finally:
        cx.close()


def test_masked_then_unmasked_commitment_on_one_context(vp, ob):
    """A commitment with a mask slice runs over all 64 slices and leaves the "zero from slice" marks at 64; the unmasked commitment that follows on the SAME
    context (no reload: the buffers stay) zeroes the gap above its live count in buffers it keeps.  Everything equals the oracle's, and so a fresh context's —
    a gap zeroed at the wrong place or length would wipe live slices or miss dead ones."""
    n, N = 12, 1 << 6
    x = _inputs(n, 32 * N + 9, 7500)
    assert _live_of(x) == 33
    L = vp.lib_gpu()
    VP = ctypes.c_void_p
    L.vp_commit_private_masked.argtypes = [VP, VP, ctypes.c_uint64, VP]
    L.vp_commit_public_masked.argtypes = [VP, VP, ctypes.c_uint64, VP, ctypes.c_uint64, VP, VP, VP]
    rng = np.random.default_rng(7501)
    pm, qm = (rng.integers(0, pai.P61, size=(k, 2), dtype=np.uint64) for k in (40, 40))
    cx = Ctx(vp, x)
    try:
        rl, rh, sums = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32), np.zeros((66, 2), np.uint64)
        assert L.vp_commit_private_masked(cx.c, pm.ctypes.data, pm.shape[0], ctypes.cast(rl, VP)) == 0, cx.err()
        assert L.vp_commit_public_masked(cx.c, x["pub"].ctypes.data, x["pub"].shape[0], qm.ctypes.data, qm.shape[0], sums.ctypes.data, sums.ctypes.data + 16,
                                         ctypes.cast(rh, VP)) == 0, cx.err()
        cx.fri_commit(x["r"])
        assert sums[1:34].any(axis=1).all() and not sums[34:65].any() and sums[65].any()       # all_sum: 33 live slices, 31 dead ones, the mask's
        got = {"root_l": cx.commit_private()}
        assert got["root_l"] != rl.raw
        got["root_h"], got["public"] = cx.commit_public(x["pub"])
        got["roots"] = cx.fri_commit(x["r"])
        rc, got["final"] = cx.fri_final_rc()
        assert rc == 0, cx.err()
        want = _expected(ob, x, 7500)
        _compare(got, want, "unmasked behind masked, live 33")
        _check_openings(cx, want, 33, "unmasked behind masked, live 33")
    finally:
        cx.close()


def _tuning(vp, cx, name):
    v = ctypes.c_int32(-1)
    L = vp.lib_gpu()
    L.vp_tuning_get.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32)]
    assert L.vp_tuning_get(cx.c, name, ctypes.byref(v)) == 0
    return v.value


def test_toggle_equality_at_the_flagship_kernels(vp, monkeypatch):
    """n = 21 (N = 2^15: k_ntt8_colsx<6>, the grouped k_fri_fold0_vo3, the 1024-thread leaf hash), live = 57, seeded real values, the protocol's tensor public
    vector (vp_commit_public_eq): the default and VP_PC_LIVE=0 give the same roots, all_sum, FRI roots and final codeword."""
    n, N = 21, 1 << 15
    x = _inputs(n, 56 * N + 1234, 7300, real=True)
    assert _live_of(x) == 57
    point = np.random.default_rng(7301).integers(0, pai.P61, size=(n, 2), dtype=np.uint64)
    out = []
    for live_on in (1, 0):
        monkeypatch.setenv("VP_PC_LIVE", str(live_on))            # read once per vp_create
        got, cx = _run(vp, x, lambda c: c.commit_public_eq(point), n - 6)
        try:
            assert _tuning(vp, cx, b"pc_live") == live_on
            rc, vals, path = cx.open(0, 12345)
            assert rc == 0 and _opening_ok(got["root_l"], 12345, vals, path) and not vals[2 * 57:].any() and vals[:2 * 57].any()
        finally:
            cx.close()
        out.append(got)
    alls = np.frombuffer(out[0]["public"][16:], np.uint64).reshape(65, 2)
    assert alls[:57].any(axis=1).all() and not alls[57:].any()
    _compare(out[0], out[1], "n=21 live=57, default against VP_PC_LIVE=0")


def test_real_pair_encode_at_stride_29_vs_reference(vp, golden, pws_path):
    """SHA-256 x64 (n = 19, 7226 x 64 inputs: live = 57; a real witness, so vp_commit_private pairs slices p and p + 29): the complete pass against the real
    reference's transcript, FRI roots and final codeword, and the launch table's forward encodes run 29 x 32 (l) and 57 x 32 (h) transforms."""
    c = vp.Circuit.from_pws(pws_path, 64, seed=1)
    s = vp.Session(c)
    try:
        n = c.layer_bitlen(0)
        assert n == 19 and -(-c.layer_size(0) // (1 << (n - 6))) == 57
        gold = open(os.path.join(GOLDEN, golden["sha256_x64"]["transcript"]), "rb").read()
        s.set_profiling(1)
        root, _ = s.commit_private()
        enc = sorted(e["jobs"] for e in s.launch_stats() if e["kernel"] in ("k_ntt8_cols", "k_ntt8_rows"))
        assert enc == [29, 29, 29 * 32, 29 * 32], enc             # 29 paired inverse transforms, 29 x 32 paired forward ones (both passes of each)
        s.set_profiling(0)
        assert root == gold[:32]
        full, ok = s.prove_full(batched=True)
        assert ok
        assert full == gold
        r, roots_gold, fin_gold = _fri_golden(golden, "sha256_x64")
        roots, fin = s.fri_commit(r)
        assert roots == b"".join(roots_gold)
        assert np.array_equal(fin, fin_gold)
        # the h encode, from a profiled vp_commit_public on a vector that is no tensor: q and the products' inverses run over 57 slices as well
        pub = np.random.default_rng(7400).integers(0, pai.P61, size=(1 << n, 2), dtype=np.uint64)
        s.set_profiling(1)
        s.commit_public(pub)
        enc = sorted(e["jobs"] for e in s.launch_stats() if e["kernel"] in ("k_ntt8_cols", "k_ntt8_rows"))
        assert enc == [57, 57, 2 * 57, 2 * 57, 57 * 32, 57 * 32, 57 * 32, 57 * 32], enc
        s.set_profiling(0)
    finally:
        s.close(); c.close()
