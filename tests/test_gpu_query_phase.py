"""The commitment's query phase in one device pass: vp_fri_open_many (k_pc_open_many: one launch, one copy, one synchronise for a list of
openings), vp_fri_query (the complete answer to the verifier's repetitions in a fixed layout), the verifier's batched_openings path, and the
record of a complete-protocol run that the host verifier replays without a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_parity as parity
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
P = (1 << 61) - 1
VP_EINVAL, VP_ELIMIT = -1, -5
VAL = 130 * 16                      # bytes of one opening's values


def _ctx(vp):
    h = ctypes.c_void_p()
    assert vp.lib_gpu().vp_create(0, ctypes.byref(h)) == 0, "vp_create failed: the HIP extension must run on the GPU box"
    return h


def _seeded(n, seed, count=None):
    rng = np.random.default_rng(seed)
    return rng.integers(0, P, size=((1 << n) if count is None else count, 2), dtype=np.uint64)


def _commit(vp, ctx, n, seed, upto="fri"):
    """A commitment on seeded values through vp_pc_load_input: private, public, commit phase (or only up to `upto`).  Returns the fold challenges."""
    L = vp.lib_gpu()
    vals = _seeded(n, seed)
    assert L.vp_pc_load_input(ctx, vals.ctypes.data, vals.shape[0], n) == 0, L.vp_last_error(ctx)
    del vals
    root = ctypes.create_string_buffer(32)
    if upto == "load":
        return None
    assert L.vp_commit_private(ctx, ctypes.cast(root, ctypes.c_void_p)) == 0, L.vp_last_error(ctx)
    if upto == "private":
        return None
    pub = _seeded(n, seed + 1)
    inner, alls = np.zeros(2, np.uint64), np.zeros((65, 2), np.uint64)
    assert L.vp_commit_public(ctx, pub.ctypes.data, pub.shape[0], inner.ctypes.data, alls.ctypes.data, ctypes.cast(root, ctypes.c_void_p)) == 0, L.vp_last_error(ctx)
    del pub
    if upto == "public":
        return None
    r = _seeded(n, seed + 2, n - 6)
    roots = ctypes.create_string_buffer(32 * (n - 6))
    assert L.vp_fri_commit(ctx, r.ctypes.data, n - 6, ctypes.cast(roots, ctypes.c_void_p)) == 0, L.vp_last_error(ctx)
    return r


def _n_leaves(n, oracle):
    return 1 << (n - 2) if oracle < 2 else 1 << (n - 3 - (oracle - 2))


def _requests(n, count, seed):
    """Every oracle and level, each one's leaf 0 and last leaf, random leaves, and repeated requests; `count` in all, shuffled."""
    rng = np.random.default_rng(seed)
    oracles = list(range(2 + n - 6))
    req = []
    for o in oracles:
        req += [(o, 0), (o, _n_leaves(n, o) - 1)]
    while len(req) < count - count // 8:
        o = int(rng.choice(oracles))
        req.append((o, int(rng.integers(0, _n_leaves(n, o)))))
    while len(req) < count:
        req.append(req[int(rng.integers(0, len(req)))])        # repeated requests
    order = rng.permutation(len(req))
    return [req[i] for i in order]


def _open_one(vp, ctx, oracle, leaf, cap=32 * 40):
    vals = np.zeros((130, 2), np.uint64)
    path = ctypes.create_string_buffer(max(cap, 1))
    plen = ctypes.c_int(0)
    rc = vp.lib_gpu().vp_fri_open(ctx, oracle, leaf, vals.ctypes.data, ctypes.cast(path, ctypes.c_void_p), cap, ctypes.byref(plen))
    return rc, vals, path.raw[:32 * plen.value], plen.value


def _assert_many_equals_one_by_one(vp, ctx, req):
    rc, values, paths, plen = vp.fri_open_many(ctx, req)
    assert rc == 0, vp.lib_gpu().vp_last_error(ctx)
    for i, (o, lf) in enumerate(req):
        rc1, v1, p1, n1 = _open_one(vp, ctx, o, lf)
        assert rc1 == 0
        assert plen[i] == n1, ("path_len", i, o, lf)
        assert values[i].tobytes() == v1.tobytes(), ("values", i, o, lf)
        assert paths[i, :32 * n1].tobytes() == p1, ("path", i, o, lf)


# ---- 1. many = one by one ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,blocks,n", [("sha256_x1", 1, 13), ("sha256_x16", 16, 17)])
def test_open_many_equals_one_by_one_sha256(vp, golden, pws_path, name, blocks, n):
    """After a complete commitment of the SHA-256 circuit's input layer: >= 600 requests over every oracle and level (each one's first and last
    leaf, repeats) answered in ONE vp_fri_open_many call are byte for byte what vp_fri_open answers one at a time."""
    c = vp.Circuit.from_pws(pws_path, blocks, seed=1)
    assert c.layer_bitlen(0) == n
    s = vp.Session(c)
    _, ok = s.prove_full(batched=True)
    assert ok
    r, _, _ = parity._fri_golden(golden, name)
    s.fri_commit(r)
    req = _requests(n, 640, 11 + n)
    assert len(req) >= 600 and {o for o, _ in req} == set(range(2 + n - 6))
    _assert_many_equals_one_by_one(vp, s.gpu_ctx(), req)
    v, p, pl = s.fri_open_many(req[:5])                                    # the Session wrapper
    assert v.shape == (5, 130, 2) and [int(x) for x in pl] == [(n - 1 if o < 2 else n - 2 - (o - 2)) for o, _ in req[:5]]
    s.close(); c.close()


@pytest.mark.parametrize("n,count", [(20, 640), (24, 64)])
def test_open_many_equals_one_by_one_loaded_input(vp, n, count):
    """The same on seeded values loaded with vp_pc_load_input at n = 20 and n = 24 (leaf indices up to 2^22, byte offsets beyond 2^32)."""
    ctx = _ctx(vp)
    try:
        _commit(vp, ctx, n, 500 + n)
        _assert_many_equals_one_by_one(vp, ctx, _requests(n, count, 21 + n))
    finally:
        vp.lib_gpu().vp_destroy(ctx)


# ---- 2. the real reference's openings ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n13_zero", "n13_m5", "n13_m64", "n16_m100", "n19_m3000", "n13_m300", "n13_m2000"])
def test_open_many_vs_real_reference_with_mask_slices(vp, name):
    """The eight openings of tests/golden/pc_masked_*.bin (the REAL reference's, mask slice's pair included: oracles 0 and 1 at leaves 0, 5,
    M/2 - 1, FRI levels 0 and 2 at leaf 3), asked in ONE call after the commit phase."""
    x, meta, rec, fri = parity._pc_masked_record(name)
    L = vp.lib_gpu()
    n, st = x["n"], meta["fri_steps"]
    M = 1 << (n - 1)
    ctx = _ctx(vp)
    try:
        vals = np.ascontiguousarray(x["values"])
        assert L.vp_pc_load_input(ctx, vals.ctypes.data, vals.shape[0], n) == 0
        root_l, root_h = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
        inner, alls = np.zeros(2, np.uint64), np.zeros((65, 2), np.uint64)
        pub = np.ascontiguousarray(x["pub"])
        if name.endswith("_zero"):
            assert L.vp_commit_private(ctx, ctypes.cast(root_l, ctypes.c_void_p)) == 0
            assert L.vp_commit_public(ctx, pub.ctypes.data, pub.shape[0], inner.ctypes.data, alls.ctypes.data, ctypes.cast(root_h, ctypes.c_void_p)) == 0
        else:
            L.vp_commit_private_masked.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
            L.vp_commit_public_masked.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
            pm, qm = np.ascontiguousarray(x["pri_mask"]), np.ascontiguousarray(x["pub_mask"])
            assert L.vp_commit_private_masked(ctx, pm.ctypes.data, pm.shape[0], ctypes.cast(root_l, ctypes.c_void_p)) == 0, L.vp_last_error(ctx)
            assert L.vp_commit_public_masked(ctx, pub.ctypes.data, pub.shape[0], qm.ctypes.data, qm.shape[0], inner.ctypes.data, alls.ctypes.data,
                                             ctypes.cast(root_h, ctypes.c_void_p)) == 0, L.vp_last_error(ctx)
        assert root_l.raw == rec[:32] and root_h.raw == rec[32:64]
        rr = np.frombuffer(b"".join(fri[48 * k:48 * k + 16] for k in range(st)), dtype=np.uint64).reshape(st, 2).copy()
        roots = ctypes.create_string_buffer(32 * st)
        assert L.vp_fri_commit(ctx, rr.ctypes.data, st, ctypes.cast(roots, ctypes.c_void_p)) == 0, L.vp_last_error(ctx)
        req = [(o, lf) for o in (0, 1) for lf in (0, 5, M // 2 - 1)] + [(2, 3), (4, 3)]
        rc, values, _, plen = vp.fri_open_many(ctx, req)
        assert rc == 0, L.vp_last_error(ctx)
        at = 64 + 65 * 16
        for i, q in enumerate(req):
            assert values[i].tobytes() == rec[at:at + VAL], ("opening", q)
            at += VAL
        assert at == len(rec)
        assert [int(v) for v in plen] == [n - 1] * 6 + [n - 2, n - 4]
    finally:
        L.vp_destroy(ctx)


# ---- 3. vp_fri_query's layout --------------------------------------------------------------------------------------------------------------
def _leaf_chain(n, leaf0):
    """(oracle, leaf) of one repetition, derived as host/verifier.cpp does."""
    out = [(0, leaf0), (1, leaf0)]
    D, t = 1 << (n - 1), leaf0
    for k in range(n - 6):
        Dn = D // 2
        leaf = t % (Dn // 2)
        out.append((2 + k, leaf))
        t, D = leaf, Dn
    return out


def _query_formula(n):
    return 2 * (VAL + 32 * (n - 1)) + sum(VAL + 32 * (n - 2 - k) for k in range(n - 6))


def test_query_bytes_formula_at_n23():
    assert _query_formula(23) == 48000


@pytest.mark.parametrize("name,blocks,n", [("sha256_x1", 1, 13), ("sha256_x16", 16, 17)])
def test_fri_query_is_the_concatenation_of_single_openings(vp, golden, pws_path, name, blocks, n):
    """vp_fri_query for 33 seeded positions = vp_fri_open's answers along the derived leaf chains, in the documented order and at the true path
    lengths; n_written = vp_fri_query_bytes = 33 x the formula."""
    c = vp.Circuit.from_pws(pws_path, blocks, seed=1)
    s = vp.Session(c)
    _, ok = s.prove_full(batched=True)
    assert ok
    r, _, _ = parity._fri_golden(golden, name)
    s.fri_commit(r)
    ctx = s.gpu_ctx()
    rng = np.random.default_rng(77 + n)
    leaf0 = rng.integers(0, 1 << (n - 2), size=33, dtype=np.uint64)
    leaf0[0], leaf0[1] = 0, (1 << (n - 2)) - 1
    out = s.fri_query(leaf0)
    rc, nb = vp.fri_query_bytes(ctx, 33)
    assert rc == 0 and nb == len(out) == 33 * _query_formula(n)
    exp = b""
    for l0 in leaf0:
        for o, lf in _leaf_chain(n, int(l0)):
            rc1, v1, p1, n1 = _open_one(vp, ctx, o, lf)
            assert rc1 == 0 and n1 == (n - 1 if o < 2 else n - 2 - (o - 2))
            exp += v1.tobytes() + p1
    assert out == exp
    assert vp.fri_query(ctx, np.zeros(0, np.uint64)) == (0, b"")
    s.close(); c.close()


# ---- 4. sharded ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [13, 17])
@pytest.mark.parametrize("world", [2, 4, 8])
def test_open_many_on_a_sharded_commitment(vp, n, world):
    """W contexts on one GPU: vp_fri_open_many asked of every rank and merged by path_len equals the unsharded context's bytes; a request for a
    position-sharded oracle is answered by exactly one rank (its owner), a tail-level request by all of them identically."""
    L = vp.lib_gpu()
    ctx = _ctx(vp)
    sc = None
    try:
        r = _commit(vp, ctx, n, 900 + n)
        req = _requests(n, 300, 31 + n + world)
        rc, values, paths, plen = vp.fri_open_many(ctx, req)
        assert rc == 0, L.vp_last_error(ctx)
        sc = vp.ShardedCommitment(_seeded(n, 900 + n), n, world)
        sc.commit_private(); sc.commit_public(_seeded(n, 901 + n)); sc.fri_commit(r)
        mv, mp, mpl, answered = sc.open_many(req)
        assert np.array_equal(mpl, plen) and np.array_equal(mv, values)
        for i in range(len(req)):
            assert mp[i, :32 * plen[i]].tobytes() == paths[i, :32 * plen[i]].tobytes(), ("path", i, req[i])
        lw = world.bit_length() - 1
        first_tail = 2 + (n - 6 - lw) - 1                                   # oracle of the first replicated level
        n_tail = 0
        for i, (o, lf) in enumerate(req):
            if o >= first_tail:
                assert answered[:, i].all(), ("tail level: every rank", o, lf)
                n_tail += 1
            else:
                assert answered[:, i].sum() == 1 and answered[(lf >> 5) % world, i], ("owner", o, lf)
        assert 0 < n_tail < len(req)
        # every rank's own answer: untouched sentinel bytes where it does not own, identical bytes on the tail levels
        for rk in range(world):
            rc, v, p, pl = vp.fri_open_many(sc.ctx[rk], req, fill=0xA5)
            assert rc == 0
            for i, (o, lf) in enumerate(req):
                if answered[rk, i]:
                    assert pl[i] == plen[i] and v[i].tobytes() == values[i].tobytes() and p[i, :32 * pl[i]].tobytes() == paths[i, :32 * plen[i]].tobytes()
                else:
                    assert pl[i] == 0 and (v[i].view(np.uint8) == 0xA5).all() and (p[i] == 0xA5).all()
        assert vp.fri_query(sc.ctx[0], np.zeros(3, np.uint64))[0] == VP_EINVAL     # vp_fri_query: unsharded contexts only
    finally:
        if sc is not None:
            sc.close()
        L.vp_destroy(ctx)


# ---- 5. the protocol -----------------------------------------------------------------------------------------------------------------------
def _protocol_case(vp, golden, c, name, reps):
    s = vp.Session(c)
    tr0, ok0, _ = s.prove_and_verify_full(reps=reps)                        # the default path, one vp_fri_open per opening
    assert ok0
    rec0 = s.last_full_record()
    tr, ok, times = s.prove_and_verify_full(reps=reps, batched_openings=True)
    assert ok
    gold = open(os.path.join(GOLDEN, golden[name]["transcript"]), "rb").read()
    assert tr == gold and tr0 == gold
    r_gold, roots_gold, fin_gold = parity._fri_golden(golden, name)
    roots, fin, r = s.last_fri()
    assert np.array_equal(r, r_gold), "FRI fold challenges differ from the reference's"
    assert roots == roots_gold and np.array_equal(fin, fin_gold)
    rec = s.last_full_record()
    assert rec == rec0, "the batched run's record differs from the one-by-one run's (positions or openings)"
    n = c.layer_bitlen(0)
    lg = n - 6
    fft_msgs = 64 + 3 * (2 * lg * lg + 2 * lg + 6) + 2 + 2 * lg
    assert rec[16:16 + len(gold)] == gold and len(rec) == 16 + len(gold) + 16 * fft_msgs + 32 * lg + 2048 * 16 + reps * _query_formula(n)
    assert rec[16 + len(gold) + 16 * fft_msgs:16 + len(gold) + 16 * fft_msgs + 32 * lg] == roots
    assert rec[-reps * _query_formula(n) - 2048 * 16:-reps * _query_formula(n)] == fin.tobytes()
    assert times["pc_query_answer_sec"] > 0
    s.close()
    return rec


@pytest.mark.parametrize("name,blocks", [("sha256_x1", 1), ("sha256_x16", 16)])
def test_complete_protocol_with_batched_openings(vp, golden, pws_path, name, blocks):
    """verifier::verify() end to end with the query phase answered in one device pass: accepted; transcript, FRI roots, challenges and final
    codeword equal the real reference's records; the record equals the one the default one-by-one run of the same session leaves."""
    c = vp.Circuit.from_pws(pws_path, blocks, seed=1)
    _protocol_case(vp, golden, c, name, 33)
    c.close()


def test_complete_protocol_with_batched_openings_custom_gates(vp, golden):
    import custom_circuits as cc
    g = golden["custom_b"]
    c = vp.Circuit.custom(*cc.make(g["custom"]["seed"], g["custom"]["sizes"]))
    _protocol_case(vp, golden, c, "custom_b", 8)
    c.close()


# ---- 6. one launch -------------------------------------------------------------------------------------------------------------------------
def test_query_phase_is_one_launch(vp, pws_path):
    """With profiling on, the query phase of a 33-repetition batched run is exactly ONE k_pc_open_many entry whose bytes are what
    vp_fri_query_bytes reports; a list of 4097 requests is two entries (pieces of 4096)."""
    c = vp.Circuit.from_pws(pws_path, 1, seed=1)
    s = vp.Session(c)
    s.set_profiling(1)
    _, ok, _ = s.prove_and_verify_full(reps=33, batched_openings=True)
    assert ok
    st = s.launch_stats()                                                   # the table of the last profiled call: vp_fri_query
    assert [e["kernel"] for e in st] == ["k_pc_open_many"], st
    rc, nb = vp.fri_query_bytes(s.gpu_ctx(), 33)
    assert rc == 0 and st[0]["bytes"] == nb == 33 * _query_formula(13) and st[0]["workgroups"] == 33 * 9 and st[0]["us"] > 0
    n = 13
    req = _requests(n, 4097, 5)
    v, p, pl = s.fri_open_many(req)
    st = s.launch_stats()
    assert [e["kernel"] for e in st] == ["k_pc_open_many"] * 2 and [e["workgroups"] for e in st] == [4096, 1]
    assert sum(e["bytes"] for e in st) == sum(VAL + 32 * int(x) for x in pl)
    for i in (0, 4095, 4096):                                               # both sides of the seam
        rc1, v1, p1, n1 = _open_one(vp, s.gpu_ctx(), *req[i])
        assert rc1 == 0 and v[i].tobytes() == v1.tobytes() and p[i, :32 * n1].tobytes() == p1 and pl[i] == n1
    s.set_profiling(0)
    s.close(); c.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def _assert_refused_like_single(vp, ctx, req, bad_index, path_stride=32 * 26):
    """The whole list is refused with the status vp_fri_open gives the bad request, and the sentinel-filled outputs are untouched."""
    L = vp.lib_gpu()
    o, lf = req[bad_index]
    rc1, _, _, _ = _open_one(vp, ctx, o, lf, cap=path_stride)
    assert rc1 < 0
    n0 = ctypes.c_int(0)
    L.vp_get_launch_stats(ctx, None, 0, ctypes.byref(n0))
    rc, v, p, pl = vp.fri_open_many(ctx, req, path_stride=path_stride, fill=0xA5)
    assert rc == rc1, (rc, rc1, req[bad_index])
    assert (v.view(np.uint8) == 0xA5).all() and (p == 0xA5).all() and (pl.view(np.uint8) == 0xA5).all()
    n1 = ctypes.c_int(0)
    L.vp_get_launch_stats(ctx, None, 0, ctypes.byref(n1))
    assert n1.value == n0.value                                             # no launch: the profiled table of the last good call still stands


def test_refused_lists(vp):
    """Argument checks on the host, before anything is launched: one bad request among good ones fails the whole call like vp_fri_open fails
    that request; 2^16 + 1 requests are VP_ELIMIT; vp_fri_query before the last FRI step is VP_EINVAL; a good list is answered afterwards."""
    L = vp.lib_gpu()
    n = 13
    ctx = _ctx(vp)
    try:
        L.vp_set_profiling(ctx, 1)
        _commit(vp, ctx, n, 40, upto="private")
        good0 = [(0, 3), (0, 77)]
        rc, _, _, _ = vp.fri_open_many(ctx, good0)
        assert rc == 0
        _assert_refused_like_single(vp, ctx, good0 + [(1, 3)] + good0, 2)                    # oracle 1 before commit_public
        _commit(vp, ctx, n, 40, upto="public")
        good1 = [(0, 3), (1, 77), (1, 0)]
        assert vp.fri_open_many(ctx, good1)[0] == 0
        _assert_refused_like_single(vp, ctx, good1 + [(2, 0)], 3)                             # a level not committed yet
        assert vp.fri_query(ctx, np.zeros(2, np.uint64))[0] == VP_EINVAL                      # vp_fri_query before the last FRI step
        assert vp.fri_query_bytes(ctx, 2)[0] == VP_EINVAL
        _commit(vp, ctx, n, 40)
        good = [(0, 3), (1, 77), (2, 5), (2 + n - 7, 15), (3, 0)]
        assert vp.fri_open_many(ctx, good)[0] == 0
        _assert_refused_like_single(vp, ctx, good[:2] + [(0, _n_leaves(n, 0))] + good[2:], 2)  # leaf = n_leaves
        _assert_refused_like_single(vp, ctx, good[:3] + [(4, _n_leaves(n, 4))] + good[3:], 3)
        _assert_refused_like_single(vp, ctx, [(-1, 0)] + good, 0)                             # oracle < 0
        _assert_refused_like_single(vp, ctx, good + [(2 + n - 6, 0)], len(good))              # a level beyond the last
        _assert_refused_like_single(vp, ctx, good, 0, path_stride=32 * (n - 1) - 32)          # path_stride one digest short of the longest path
        assert vp.fri_open_many(ctx, good, path_stride=32 * (n - 1))[0] == 0                  # ... and exactly long enough
        rc, _, _, _ = vp.fri_open_many(ctx, [(0, 1)] * ((1 << 16) + 1), path_stride=32 * (n - 1))
        assert rc == VP_ELIMIT
        assert vp.fri_open_many(ctx, [])[0] == 0                                              # n == 0: VP_OK, nothing done
        _assert_many_equals_one_by_one(vp, ctx, good + _requests(n, 50, 3))                   # the context still answers
        rc, out = vp.fri_query(ctx, np.array([5, 2047], np.uint64))
        assert rc == 0 and len(out) == 2 * _query_formula(n)
    finally:
        L.vp_destroy(ctx)


# ---- 8. record round trip ------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
sys.path.insert(0, %r)
import vp_loader
vp = vp_loader.load()
c = vp.Circuit.from_pws(sys.argv[1], 1, seed=1)          # the circuit only: no session, no device
rec = open(sys.argv[2], "rb").read()
bad = bytearray(rec); bad[int(sys.argv[3])] ^= 0x10
print("VERDICT", c.verify_full_record(rec), c.verify_full_record(bytes(bad)), flush=True)
"""


def test_record_of_a_gpu_run_verifies_in_a_process_without_a_session(vp, pws_path, tmp_path):
    """The record of a complete-protocol run at x1 is accepted by Circuit.verify_full_record in a fresh child process that builds the circuit and
    creates no session, and rejected there with one byte of an opening flipped."""
    c = vp.Circuit.from_pws(pws_path, 1, seed=1)
    s = vp.Session(c)
    _, ok, _ = s.prove_and_verify_full(reps=33, batched_openings=True)
    assert ok
    rec = s.last_full_record()
    s.close(); c.close()
    f = tmp_path / "record.bin"
    f.write_bytes(rec)
    flip = len(rec) - 5 * _query_formula(13) + 1000                         # a value of repetition 28's first opening
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, pws_path, str(f), str(flip)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "VERDICT True False" in r.stdout, (r.stdout[-300:], r.stderr[-1500:])


def test_cli_writes_and_checks_a_record(vp, pws_path, tmp_path):
    """virgo_plus_run --record FILE writes the record of its run; virgo_plus_run --check-record FILE <circuit.pws> verifies it with the host
    verifier alone and rejects a tampered copy."""
    f = tmp_path / "cli_record.bin"
    out = subprocess.run([vp.CLI, pws_path, "--record", str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0 and "Verification pass" in out.stderr, out.stderr[-1500:]
    rec = f.read_bytes()
    assert len(rec) > 33 * _query_formula(13)
    chk = subprocess.run([vp.CLI, "--check-record", str(f), pws_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert chk.returncode == 0 and "Verification pass" in chk.stderr, chk.stderr[-1500:]
    bad = bytearray(rec); bad[-40] ^= 1
    g = tmp_path / "cli_record_bad.bin"
    g.write_bytes(bytes(bad))
    chk = subprocess.run([vp.CLI, "--check-record", str(g), pws_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert chk.returncode == 1 and "Verification fail" in chk.stderr


# ---- the -DVP_CHECKED flavour ----------------------------------------------------------------------------------------------------------------
_CHECKED_CHILD = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import vp_loader
vp = vp_loader.load()
vp.lib_host()
assert vp.lib_gpu().vp_checked_build() == 1, "VP_LIBGPU did not select the checked library"
import test_gpu_query_phase as t
ctx = t._ctx(vp)
n = 13
r = t._commit(vp, ctx, n, 60)
req = t._requests(n, 200, 9)
t._assert_many_equals_one_by_one(vp, ctx, req)
rc, values, paths, plen = vp.fri_open_many(ctx, req)
sc = vp.ShardedCommitment(t._seeded(n, 60), n, 4)
sc.commit_private(); sc.commit_public(t._seeded(n, 61)); sc.fri_commit(r)
mv, mp, mpl, answered = sc.open_many(req)
assert rc == 0 and np.array_equal(mv, values) and np.array_equal(mpl, plen)
sc.close()
vp.lib_gpu().vp_destroy(ctx)
print("CHECKED OK", flush=True)
"""


def test_checked_build_answers_open_many_without_a_violated_check(vp):
    """k_pc_open_many in the -DVP_CHECKED flavour (csrc/vp_check.h sites 7 and 9: the request and the positions it leads to): the same bytes as
    vp_fri_open on an unsharded and a sharded commitment, and no check fires (a violated one would fail the call with VP_EHIP)."""
    assert os.path.exists(vp.LIB_GPU_CHECKED), "vp.build() did not produce the checked library"
    env = dict(os.environ, VP_LIBGPU=vp.LIB_GPU_CHECKED)
    r = subprocess.run([sys.executable, "-c", _CHECKED_CHILD % (ROOT, os.path.join(ROOT, "tests"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0 and "CHECKED OK" in r.stdout, (r.stdout[-800:], r.stderr[-2000:])
