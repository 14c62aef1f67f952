"""GPU (-m gpu): the commit phase of the non-interactive commitment drawn on the device (vp_fri_commit_fs) and the proof around it (Session.commit_fs).

  against the CPU reference   tests/pc_fs_ref.py — the Python chain over the oracle's commitment, a fixed point of ln + 1 runs (recorded for the sizes at which
                              that takes the CPU too long: tests/golden/pc_fs.json) — compared with roots, r_out, state_out, the final codeword and the final mask:
                              n = 7 (one fold, k_fri_fold0_vo_p; the 16-leaf last level), 8 (the first k_fri_fold_p), 9 and 12 (k_ntt_lds edges, trees of one
                              k_merkle_top), 14 (the radix-8 transforms), 15 and 16 (ln >= 9, where the one-pass phase takes the fused three-level fold and this one
                              must not); uniform, edges and sparse inputs (five wires: live < 64, VP_PC_LIVE=0 the same bytes); masks: n = 10 ms = 8 (uniform,
                              pub_zero, a shorter public mask), n = 13 ms = 128 = N and 256 = 2 N (k_mask_combine)
  device against device       a fresh commitment of the same input through vp_fri_commit(r_out): the same roots and final codewords, vp_fri_query the same bytes
  Session.commit_fs           device_draws True and False: the same proof; accepted on the host and with device=0; a tampered section rejected in both
  launch table                ln k_fri_fold rows of the per-level grids (none of the fused fold's), ln k_leaf_hash rows, one drawing tree top per level
  draw hook                   D + C against hashlib; the reduction on 0, p - 1, p, 2^61, 2^64 - 1 in each limb
  refusals                    null arguments, before vp_commit_public, after vp_fri_step / vp_fri_commit / vp_fri_commit_fs, a sharded commitment — and an honest
                              run on the same context afterwards gives the expected bytes
  other contexts              vp_pc_hash_late 1 and 2: the same bytes; one context through n = 8, 12 (masked), 9, 9 (masked), 12"""
import ctypes
import hashlib
import struct

import numpy as np
import pytest

import pc_fs_ref as fs
import pc_masked_inputs as pmi
from test_gpu_masked_fast_path import Ctx

pytestmark = pytest.mark.gpu
VP_EINVAL = -1
P = fs.P
_cp = lambda b: ctypes.cast(b, ctypes.c_void_p)
_REF = {}


def ref_of(ob, kind, n, fam=None, ms=None):
    """the CPU reference of a case, computed (or read) once and left unchanged"""
    key = (kind, n, fam, ms)
    if key not in _REF:
        _REF[key] = fs.reference(ob.lib(), kind, n, fam, ms)
    return _REF[key]


def load(vp, kind, n, env=None):
    x, point, _ = fs.case(kind, n)
    return Ctx(vp, np.ascontiguousarray(x["values"][:x["n_used"]]), n, env)


def commits(c, kind, n, fam=None, ms=None):
    """vp_commit_private(_masked) and vp_commit_public_eq(_masked) of a case on the context; returns the chain after D(1, root_h)"""
    x, point, f = fs.case(kind, n, fam, ms)
    if f is None:
        c.commit_private(); c.commit_public_eq(point)
        ms_, pm = 1, point[:0]
    else:
        c.commit_private(f["pri_mask"]); c.commit_public_eq(point, f["pub_mask"])
        ms_, pm = ms, f["pub_mask"]
    return lambda: fs.head(n, 33, ms_, point, pm, c.inner, c.root_l.raw, c.root_h.raw, c.alls).s


def commit_fs(c, state_in, expect=0):
    ln = c.n - 6
    roots, st, sin = ctypes.create_string_buffer(32 * ln), ctypes.create_string_buffer(32), ctypes.create_string_buffer(bytes(state_in), 32)
    r = np.zeros((ln, 2), np.uint64)
    rc = c.L.vp_fri_commit_fs(c.ctx, _cp(sin), _cp(roots), r.ctypes.data, _cp(st))
    assert rc == expect, (rc, c.err())
    return roots.raw, r, st.raw


def fields(c, roots, r, st, state_in):
    fin, fm = c.finals()
    return {"root_l": c.root_l.raw.hex(), "root_h": c.root_h.raw.hex(), "state_in": state_in.hex(), "state_out": st.hex(), "roots": roots.hex(), "r": r.tobytes().hex(),
            "final_code_sha256": hashlib.sha256(fin).hexdigest(), "final_mask": fm.hex()}


def device_fields(vp, kind, n, fam=None, ms=None, env=None, late=0, want_state=None):
    """one whole run on a context of its own; want_state: the state to start from when the roots of l and h are still owed (vp_pc_hash_late)"""
    c = load(vp, kind, n, env)
    try:
        assert c.L.vp_pc_hash_late(c.ctx, late) == 0
        state = commits(c, kind, n, fam, ms)
        state_in = want_state if want_state is not None else state()
        roots, r, st = commit_fs(c, state_in)
        assert state() == state_in, "the state the chain has once the owed roots are written"
        return fields(c, roots, r, st, state_in)
    finally:
        c.close()


def same(got, want, what):
    for k in got:
        assert got[k] == want[k], (what, k)


# ---- 1. against the CPU reference -------------------------------------------------------------------------------------------------------------------------------
UNMASKED = [("uniform", 7), ("uniform", 8), ("uniform", 9), ("uniform", 12), ("uniform", 14), ("uniform", 15), ("uniform", 16), ("edges", 9), ("edges", 12), ("sparse", 9),
            ("sparse", 12)]
MASKED = [(10, "uniform", 8), (10, "pub_zero", 8), (10, "short_pub", 8), (13, "uniform", 128), (13, "uniform", 256)]


@pytest.mark.parametrize("kind,n", UNMASKED)
def test_commit_phase_equals_the_cpu_reference(vp, ob, kind, n):
    want = ref_of(ob, kind, n)
    same(device_fields(vp, kind, n), want, (kind, n))
    if kind == "sparse":                            # a five-wire witness: fewer than 64 live slices, and every slice live gives the same bytes
        same(device_fields(vp, kind, n, env={"VP_PC_LIVE": "0"}), want, (kind, n, "VP_PC_LIVE=0"))


@pytest.mark.parametrize("n,fam,ms", MASKED)
def test_masked_commit_phase_equals_the_cpu_reference(vp, ob, n, fam, ms):
    want = ref_of(ob, "uniform", n, fam, ms)
    got = device_fields(vp, "uniform", n, fam, ms)
    same(got, want, (n, fam, ms))
    assert fam not in pmi.NONZERO_FAMILIES or any(bytes.fromhex(got["final_mask"])), "a vacuous masked case"


def test_the_cases_cover_what_they_are_there_for():
    assert {n for k, n in UNMASKED if k == "uniform"} == {7, 8, 9, 12, 14, 15, 16} and {k for k, n in UNMASKED} == {"uniform", "edges", "sparse"}
    assert [(n, ms, ms // (1 << (n - 6))) for n, f, ms in MASKED if n == 13] == [(13, 128, 1), (13, 256, 2)]
    f = pmi.family("short_pub", 10, 8)
    assert f["pub_mask"].shape[0] < f["pri_mask"].shape[0] and not pmi.family("pub_zero", 10, 8)["pub_mask"].any()


# ---- 2. device against device -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,fam,ms", [("uniform", 9, None, None), ("uniform", 15, None, None), ("uniform", 13, "uniform", 128)])
def test_the_one_pass_phase_on_the_drawn_challenges_gives_the_same_commitment(vp, ob, kind, n, fam, ms):
    want = ref_of(ob, kind, n, fam, ms)
    a, b = load(vp, kind, n), load(vp, kind, n)
    try:
        state = commits(a, kind, n, fam, ms)
        roots, r, st = commit_fs(a, state())
        commits(b, kind, n, fam, ms)
        fin, fm = a.finals()
        assert b.fri_commit(r) == roots and (fin, fm) == b.finals()
        lf = fs.tail(fs.Chain(st), n, 33, np.frombuffer(fin, np.uint64).reshape(-1, 2), np.frombuffer(fm, np.uint64).reshape(-1, 2))
        assert lf == want["leaf0"], "the positions the chain derives"
        qa, qb = vp.fri_query(a.ctx, lf), vp.fri_query(b.ctx, lf)
        assert qa[0] == 0 and qb[0] == 0 and qa[1] == qb[1] and len(qa[1]) == 33 * sum(2080 + 32 * p for _, _, p in fs.ref.query_leaves(n, 1 << (n - 7)))
    finally:
        a.close(); b.close()


# ---- 3. Session.commit_fs ---------------------------------------------------------------------------------------------------------------------------------------
def test_session_commit_fs_both_forms_one_proof_verified_on_host_and_device(vp):
    c = vp.Circuit.randomize(8, 12, seed=1)
    n = c.layer_bitlen(0)
    point = fs.point_of(n)
    f = pmi.family("short_pub", n, 8)
    s = vp.Session(c)
    try:
        for kw in ({}, {"mask": f["pri_mask"], "pub_mask": f["pub_mask"]}):
            dev = s.commit_fs(point, reps=9, **kw)
            host = s.commit_fs(point, reps=9, device_draws=False, **kw)
            assert dev == host, "the device-drawn phase and the vp_fri_step loop"
            ms, n_pub = struct.unpack_from("<2Q", dev, 16)
            assert struct.unpack_from("<4I", dev) == (fs.MAGIC, fs.VERSION, n, 9) and (ms, n_pub) == ((8, f["pub_mask"].shape[0]) if kw else (1, 0))
            r, lf = vp.Circuit.commitment_fs_challenges(dev)
            r_py, lf_py = fs.derive(dev)
            assert r.tobytes() == r_py.tobytes() and lf == lf_py
            assert vp.Circuit.verify_commitment_fs(dev) == (True, "") and vp.Circuit.verify_commitment_fs(dev, device=0) == (True, "")
            sec = fs.sections(n, 9, n_pub)
            for what, off in (("fri root 1", sec["fri_roots"] + 32 + 3), ("all_sum", sec["all_sum"] + 5), ("answer", sec["answer"] + 77)):
                bad = bytearray(dev); bad[off] ^= 0x02
                for d in (None, 0):
                    ok, why = vp.Circuit.verify_commitment_fs(bytes(bad), device=d)
                    assert not ok and why, (what, d)
    finally:
        s.close()
        c.close()


def test_a_session_with_a_sharded_commitment_refuses(vp):
    c = vp.Circuit.randomize(8, 12, seed=1)
    s = vp.Session(c, devices=[0] * 2, round_shard_min_log=2, shard_commitment=True)
    try:
        for form in (True, False):
            with pytest.raises(RuntimeError, match="not built for a sharded commitment"):
                s.commit_fs(fs.point_of(c.layer_bitlen(0)), reps=3, device_draws=form)
        tr, ok, _ = s.prove_and_verify_full(reps=3)                        # the session goes on working
        assert ok
    finally:
        s.close()
        c.close()


# ---- 4. the launch table ----------------------------------------------------------------------------------------------------------------------------------------
def _rows(c):
    k = ctypes.c_int(0)
    c.L.vp_get_launch_stats(c.ctx, None, 0, ctypes.byref(k))
    arr = (c.vp.LaunchStat * max(1, k.value))()
    c.L.vp_get_launch_stats(c.ctx, arr, k.value, ctypes.byref(k))
    return [(c.L.vp_kernel_name(e.kind).decode(), e.workgroups, e.rounds, e.first_round) for e in arr[:k.value]]


@pytest.mark.parametrize("n,fam,ms", [(15, None, None), (13, "uniform", 128)])
def test_launch_table_has_a_fold_a_leaf_launch_and_a_drawing_top_per_level(vp, n, fam, ms):
    ln, N = n - 6, 1 << (n - 6)
    c = load(vp, "uniform", n)
    try:
        state = commits(c, "uniform", n, fam, ms)
        c.profiling(True)
        commit_fs(c, state())
        rows = _rows(c)
        c.profiling(False)
    finally:
        c.close()
    folds = [r for r in rows if r[0] == "k_fri_fold"]
    per_level = lambda k: -(-(16 * 32 * ((N >> k) >> 1)) // 256)               # 64 live slices, four per thread, 256 threads: the by-level grids, none of the fused fold's
    mask_rows = [] if fam is None else [-(-(32 * N) // 256)] + [-(-(32 * ((N >> k) >> 1)) // 256) for k in range(ln)]
    assert sorted(r[1] for r in folds) == sorted([per_level(k) for k in range(ln)] + mask_rows), folds
    assert len(folds) - len(mask_rows) == ln, "one k_fri_fold0_vo and ln - 1 k_fri_fold launches: no level shares a launch"
    assert len([r for r in rows if r[0] == "k_leaf_hash"]) == ln
    tops = [r for r in rows if r[0] == "k_merkle" and r[2] == 1]
    assert [r[3] for r in tops] == list(range(1, ln + 1)) and all(r[1] == 1 for r in tops), tops      # first_round: the level, 1-based
    assert rows[-1] == tops[-1], "the last launch is the last level's drawing top"


# ---- 5. the draw hook -------------------------------------------------------------------------------------------------------------------------------------------
def _hook(vp, ctx, op, state, root, label, counter):
    L = vp.lib_gpu()
    out, r = ctypes.create_string_buffer(32), np.zeros(2, np.uint64)
    s = None if state is None else ctypes.create_string_buffer(bytes(state), 32)
    rc = L.vp_test_fs_draw(ctx, op, None if s is None else _cp(s), _cp(ctypes.create_string_buffer(bytes(root), 32)), label, counter, _cp(out), r.ctypes.data)
    return rc, out.raw, (int(r[0]), int(r[1]))


@pytest.fixture(scope="module")
def bare(vp):
    ctx = ctypes.c_void_p()
    assert vp.lib_gpu().vp_create(0, ctypes.byref(ctx)) == 0
    yield ctx
    vp.lib_gpu().vp_destroy(ctx)


def test_draw_hook_equals_hashlib(vp, bare):
    rng = np.random.default_rng(61)
    for state, root, label, counter in [(bytes(32), bytes(32), 2, 1), (rng.bytes(32), rng.bytes(32), 2, 1), (rng.bytes(32), rng.bytes(32), 20, 19),
                                        (rng.bytes(32), rng.bytes(32), (1 << 64) - 1, 1 << 63)]:
        ch = fs.Chain(state)
        ch.D(label, root)
        want_r = ch.C(counter)
        assert _hook(vp, bare, 0, state, root, label, counter) == (0, ch.s, want_r)
    assert _hook(vp, bare, 2, bytes(32), bytes(32), 0, 0)[0] == VP_EINVAL and _hook(vp, bare, 0, None, bytes(32), 0, 0)[0] == VP_EINVAL


def test_the_reduction_on_raw_words(vp, bare):
    """p -> 0 cannot be reached through a real chain (probability 2^-61 a limb): the hook is its only test"""
    words = [0, P - 1, P, 1 << 61, (1 << 64) - 1]
    want = [0, P - 1, 0, 0, 0]
    assert want == [fs.limb(w) for w in words]
    for i, a in enumerate(words):
        for j, b in enumerate(words):
            rc, out, r = _hook(vp, bare, 1, None, struct.pack("<4Q", a, b, b, a), 0, 0)
            assert rc == 0 and r == (want[i], want[j]) and struct.unpack("<4Q", out) == (want[i], want[j], want[j], want[i]), (a, b)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(vp, ob):
    kind, n = "uniform", 9
    ln = n - 6
    want = ref_of(ob, kind, n)
    x, point, _ = fs.case(kind, n)
    c = load(vp, kind, n)
    try:
        L = c.L
        roots, st, sin = ctypes.create_string_buffer(32 * ln), ctypes.create_string_buffer(32), ctypes.create_string_buffer(bytes.fromhex(want["state_in"]), 32)
        r = np.zeros((ln, 2), np.uint64)
        args = [c.ctx, _cp(sin), _cp(roots), r.ctypes.data, _cp(st)]

        def refused(word, a=args):
            assert L.vp_fri_commit_fs(*a) == VP_EINVAL
            assert a[0] is None or word in c.err(), c.err()
            assert roots.raw == bytes(32 * ln) and st.raw == bytes(32) and not r.any(), "a refused call wrote its output"

        c.commit_private()
        refused("vp_commit_public first")                                  # before vp_commit_public*
        state = commits(c, kind, n)
        for i in range(5):                                                 # a null argument, the context among them
            refused("null", args[:i] + [None] + args[i + 1:])
        assert L.vp_pc_set_shard(c.ctx, 0, 2) == 0                         # a sharded commitment: not built
        refused("sharded")
        assert L.vp_pc_set_shard(c.ctx, 0, 1) == 0
        state = commits(c, kind, n)
        same(fields(c, *commit_fs(c, state()), state()), want, "after the first refusals")
        refused("after")                                                   # a second phase on the same commitment
        state = commits(c, kind, n)
        c.fri_step(np.frombuffer(bytes.fromhex(want["r"]), np.uint64).reshape(ln, 2)[:1])
        refused("after")                                                   # after vp_fri_step
        state = commits(c, kind, n)
        c.fri_commit(np.frombuffer(bytes.fromhex(want["r"]), np.uint64).reshape(ln, 2))
        refused("after")                                                   # after vp_fri_commit
        state = commits(c, kind, n)
        same(fields(c, *commit_fs(c, state()), state()), want, "after every refusal")
    finally:
        c.close()


# ---- 7. other contexts ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("late,n,fam,ms", [(1, 12, None, None), (2, 12, None, None), (2, 10, "uniform", 8)])
def test_under_hash_late_the_bytes_are_the_same(vp, ob, late, n, fam, ms):
    """the roots of l and h are still owed when the phase is called: it hashes them first (as vp_fri_step does), and the state the caller hands in is the
    reference's — the chain over the roots, once written, is checked to be that state"""
    want = ref_of(ob, "uniform", n, fam, ms)
    same(device_fields(vp, "uniform", n, fam, ms, late=late, want_state=bytes.fromhex(want["state_in"])), want, (late, n, fam))


def test_one_context_through_several_sizes_masked_and_unmasked(vp, ob):
    c = load(vp, "uniform", 8)
    try:
        for n, fam, ms in ((8, None, None), (12, "uniform", 8), (9, None, None), (9, "uniform", 8), (12, None, None)):
            x, point, f = fs.case("uniform", n, fam, ms)
            vals = np.ascontiguousarray(x["values"][:x["n_used"]])
            assert c.L.vp_pc_load_input(c.ctx, vals.ctypes.data, vals.shape[0], n) == 0, c.err()
            c.n = n
            state = commits(c, "uniform", n, fam, ms)
            same(fields(c, *commit_fs(c, state()), state()), ref_of(ob, "uniform", n, fam, ms), (n, fam, ms))
    finally:
        c.close()
