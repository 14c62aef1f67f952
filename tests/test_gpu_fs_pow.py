"""GPU (-m gpu): the proof-of-work search on the device (vp_fs_grind, k_fs_grind) and the version-2 proofs around it (Session.commit_fs / prove_full_fs with
pow_bits).  The reference is tests/fs_pow_ref.py: the step and the smallest-nonce search with hashlib, version-2 proofs assembled from the oracle alone.

  against hashlib   bits 1 .. 16 on eight states (the all-zero and all-0xff states among them), nonce and state_out; and the cases a wrong kernel fails, each
                    CONSTRUCTED by searching with hashlib: an answer at nonce 0; bits = 1, where about half the lanes of every wave hit and the smallest must win;
                    answers at lanes 63 and 64, at the last lane of a workgroup (1 023) and the first of the next, at the last nonce of the first window (65 535)
                    and the first of the second; `first` no multiple of anything; first = 2^32 - 5 with the answer behind the carry into the nonce's high word;
                    first a few below 2^64 - max_tries; the two max_tries edges around a known hit; an empty range (VP_ELIMIT, outputs untouched)
  bits = 20         one case against vph_fs_grind_host (itself pinned to hashlib by tests/test_fs_pow_host.py); bits = 33 (the kernel's form that tests both
                    halves of the word) as far as hashlib reaches
  launch table      k_fs_grind ran; after a hit in window w no later window did work; max_tries bounds the windows queued
  commit_fs         n = 9, 10, the zero mask and ms = 8, pow_bits 8 and 12: byte-equal to the assembled proof, the same with device_draws=False, accepted on the
                    host and with device=0; pow_bits=0 is the version-1 proof
  prove_full_fs     the circuit of tests/test_gpu_full_fs.py at pow_bits = 8: byte-equal to the assembled proof, the same with device_gkr=True, accepted,
                    rejected under min_pow_bits=9
  refusals          bits 0 and 49 and null pointers at vp_fs_grind, 33 bits at the provers, a sharded session — all before any launch"""
import ctypes
import functools
import struct

import numpy as np
import pytest

import fs_pow_ref as pw
import full_fs_ref as ff
import pc_fs_ref as fs
import pc_masked_inputs as pmi

pytestmark = pytest.mark.gpu
VP_EINVAL, VP_ELIMIT = -1, -5
WINDOW0, BLOCK = 1 << 16, 1024                     # include/vpgpu.h: window w holds 2^min(16 + 2 w, 24) nonces — the default schedule; VP_GRIND_WINDOW_LOG /
                                                   # VP_GRIND_BATCH in the environment would move the launch table these tests read; a workgroup is 1 024 lanes
STATES = [bytes(32), b"\xff" * 32] + [bytes(np.random.default_rng(4200 + i).integers(0, 256, 32, dtype=np.uint8)) for i in range(6)]
_cp = lambda b: ctypes.cast(b, ctypes.c_void_p)


@pytest.fixture(scope="module")
def small(vp):
    _, layers, log_size, seed, reps = ff.FIXTURE
    c = vp.Circuit.randomize(layers, log_size, seed=seed)
    s = vp.Session(c, device=0)
    yield c, s, reps
    s.close()
    c.close()


def raw(vp, s, state, bits, first, tries, null=None):
    """vp_fs_grind itself: (rc, nonce, state_out) with the outputs preset to a pattern"""
    L = vp.lib_gpu()
    ctx = vp.lib_host().vph_session_ctx(s.h)
    st, out, nonce = ctypes.create_string_buffer(bytes(state), 32), ctypes.create_string_buffer(b"\x5a" * 32, 32), ctypes.c_uint64(0x1234)
    args = [ctx, _cp(st), bits, first, tries, ctypes.byref(nonce), _cp(out)]
    if null is not None:
        args[null] = None
    return L.vp_fs_grind(*args), nonce.value, out.raw


def agree(vp, s, state, bits, first=0, tries=None):
    """the device's answer on a range is hashlib's: the smallest nonce and the state behind W, or VP_ELIMIT with the outputs untouched"""
    tries = (64 << bits) if tries is None else tries
    want = pw.grind(state, bits, first, tries)
    rc, nonce, out = raw(vp, s, state, bits, first, tries)
    if want is None:
        assert (rc, nonce, out) == (VP_ELIMIT, 0x1234, b"\x5a" * 32), (bits, first, tries, rc, nonce)
    else:
        assert (rc, nonce, out) == (0, want, pw.step(state, bits, want)), (bits, first, tries, rc, nonce, want)
    return want


# ---- against hashlib -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(STATES)))
def test_bits_1_to_16_equal_hashlib(vp, small, i):
    _, s, _ = small
    for bits in range(1, 17):
        h = agree(vp, s, STATES[i], bits)
        assert h is not None
        assert s.fs_grind(STATES[i], bits) == (h, pw.step(STATES[i], bits, h))


@functools.lru_cache(maxsize=None)
def _gap_hit(state, bits, gap, span):
    """a hit h >= gap of `state` with no other hit in [h - gap, h), by hashlib"""
    hs = [-1] + pw.hits(state, bits, 0, span)
    return next((h for a, h in zip(hs, hs[1:]) if h - max(a, 0) > gap and h >= gap), None)


def test_constructed_positions(vp, small):
    _, s, _ = small
    # an answer at nonce 0
    st0 = next(st for st in (bytes([k]) * 32 for k in range(256)) if pw.met(pw.step(st, 4, 0), 4))
    assert agree(vp, s, st0, 4) == 0
    # bits = 1: about half the lanes hit; the smallest wins, whatever `first`
    for st in STATES:
        for first in (0, 1, 7, 63, 64, 255, 1000003):
            agree(vp, s, st, 1, first, 100000)
    # lanes 63 / 64, the last lane of a workgroup and the first of the next: one hit h with nothing in the 2 100 nonces before it, approached from every distance
    st = STATES[3]
    h = _gap_hit(st, 12, 2100, 1 << 17)
    assert h is not None
    for off in (0, 1, 62, 63, 64, 65, 127, 128, 255, 256, BLOCK - 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK):
        assert agree(vp, s, st, 12, h - off, 4096) == h, off
    # the last nonce of the first window and the first of the second; `first` is then no multiple of the window
    h = _gap_hit(st, 17, WINDOW0 + 2, 1 << 20)
    assert h is not None
    for off in (WINDOW0 - 2, WINDOW0 - 1, WINDOW0, WINDOW0 + 1):
        assert agree(vp, s, st, 17, h - off, 1 << 18) == h, off
    assert (h - WINDOW0) % BLOCK != 0 or (h - WINDOW0 + 1) % BLOCK != 0
    # the two max_tries edges around that hit; an empty range leaves the outputs
    first = h - 1000
    assert agree(vp, s, st, 17, first, 1000) is None and agree(vp, s, st, 17, first, 1001) == h
    assert agree(vp, s, st, 17, first, 1) is None and agree(vp, s, st, 17, h, 1) == h
    # first = 2^32 - 5, the answer behind the carry into the high word
    first = (1 << 32) - 5
    stc = next(x for x in STATES if (pw.grind(x, 6, first, 4096) or 0) >= 1 << 32)
    assert agree(vp, s, stc, 6, first, 4096) >= 1 << 32
    assert agree(vp, s, stc, 6, (1 << 32) - 1, 4096) >= 1 << 32 and agree(vp, s, stc, 6, 1 << 32, 4096) >= 1 << 32
    # first a few below 2^64 - max_tries, and the range that ends at 2^64 exactly
    for tries in (1000, WINDOW0 + 77):
        assert agree(vp, s, st, 5, (1 << 64) - tries - 3, tries) is not None
        assert agree(vp, s, st, 5, (1 << 64) - tries, tries) is not None
    assert agree(vp, s, st, 40, (1 << 64) - 300, 300) is None
    with pytest.raises(RuntimeError):
        s.fs_grind(st, 40, first=5, max_tries=300)


def test_twenty_bits_and_thirty_three_against_the_host_search(vp, small):
    _, s, _ = small
    st = STATES[5]
    want = vp.fs_grind_host(st, 20)
    assert s.fs_grind(st, 20) == want and pw.met(want[1], 20) and want[1] == pw.step(st, 20, want[0])
    # 33 bits: the kernel's form that tests both halves of the word.  No CPU search reaches 2^33, so: a range hashlib says is empty is empty; and the nonce the
    # device finds meets the work by hashlib, lies at or behind the device's own first 32-bit hit, and a search that ends in front of it finds nothing
    assert pw.grind(st, 33, 0, 1 << 16) is None and raw(vp, s, st, 33, 0, 1 << 16)[0] == VP_ELIMIT
    n33, out33 = s.fs_grind(st, 33)
    assert out33 == pw.step(st, 33, n33) and pw.met(out33, 33)
    n32 = s.fs_grind(st, 32)[0]
    assert n32 <= n33 and pw.met(pw.step(st, 32, n32), 32)
    assert raw(vp, s, st, 33, 0, n33)[0] == VP_ELIMIT and raw(vp, s, st, 33, n33, 1)[:2] == (0, n33)


# ---- the launch table ------------------------------------------------------------------------------------------------------------------------------------------
def _rows(s):
    return [(r["kernel"], r["first_round"], r["work"], r["workgroups"], r["jobs"]) for r in s.launch_stats()]


def test_launch_table_windows(vp, small):
    _, s, _ = small
    st = STATES[3]
    sizes = [1 << min(16 + 2 * w, 24) for w in range(8)]
    s.set_profiling(1)
    try:
        # a hit in window 0: eight windows were queued, only the first did work
        h = pw.grind(st, 8)
        assert h < WINDOW0 and s.fs_grind(st, 8, max_tries=1 << 40)[0] == h
        rows = _rows(s)
        assert [r[0] for r in rows] == ["k_fs_grind"] * 8 and [r[1] for r in rows] == list(range(8)), rows
        assert rows[0][2] == WINDOW0 and rows[0][3] == rows[0][4] == WINDOW0 // BLOCK and all(r[2] == 0 and r[4] == 0 for r in rows[1:]), rows
        assert [r[3] for r in rows] == [-(-sz // (BLOCK * max(1, sz // (BLOCK * 4096)))) for sz in sizes], rows
        # a hit at the first nonce of window 1: windows 0 and 1 worked, no later one
        h = _gap_hit(st, 17, WINDOW0 + 2, 1 << 20)
        assert s.fs_grind(st, 17, first=h - WINDOW0, max_tries=1 << 40)[0] == h
        rows = _rows(s)
        assert len(rows) == 8 and rows[0][2] == WINDOW0 and rows[1][2] == sizes[1] and all(r[2] == 0 for r in rows[2:]), rows
        # max_tries bounds the windows queued: one window of 100 nonces; two windows, the second cut to 10 nonces; an exhausted range ran every window of it
        assert s.fs_grind(st, 1, max_tries=100)[0] == pw.grind(st, 1)
        rows = _rows(s)
        assert len(rows) == 1 and rows[0][2:4] == (100, 1), rows
        first = h - WINDOW0 - 5                                             # the 65 546 nonces in front of h: nothing there
        with pytest.raises(RuntimeError):
            s.fs_grind(st, 17, first=first, max_tries=WINDOW0 + 5)
        rows = _rows(s)
        assert [(r[1], r[2], r[3]) for r in rows] == [(0, WINDOW0, WINDOW0 // BLOCK), (1, 5, 1)], rows
        assert s.fs_grind(st, 17, first=first, max_tries=WINDOW0 + 6)[0] == h
        # a search longer than one batch of eight windows: every window up to the one with the hit worked
        total = sum(sizes)
        with pytest.raises(RuntimeError):
            s.fs_grind(st, 44, max_tries=total + 300)
        rows = _rows(s)
        assert [r[2] for r in rows] == sizes + [300] and [r[1] for r in rows] == list(range(9)), rows
    finally:
        s.set_profiling(0)


# ---- the proofs ------------------------------------------------------------------------------------------------------------------------------------------------
def _oracle_inputs(oc, n):
    values = np.zeros((1 << n, 2), np.uint64)
    inputs = oc.export_layer(0)["u"]
    values[:len(inputs), 0] = inputs
    return {"values": values, "n_used": len(inputs)}


@pytest.mark.parametrize("n,masked", [(9, False), (10, False), (9, True), (10, True)])
def test_commit_fs_with_work_is_the_assembled_proof(vp, ob, n, masked):
    c = vp.Circuit.randomize(3, n, seed=40 + n)
    oc = ob.Circuit.randomize(3, n, seed=40 + n)
    assert c.hash() == oc.hash() and c.layer_bitlen(0) == n
    x, point = _oracle_inputs(oc, n), fs.point_of(n)
    f = pmi.family("short_pub" if n == 10 else "uniform", n, 8) if masked else None
    kw = {"mask": f["pri_mask"], "pub_mask": f["pub_mask"]} if masked else {}
    s = vp.Session(c, device=0)
    try:
        v1 = s.commit_fs(point, reps=5, **kw)
        assert v1 == s.commit_fs(point, reps=5, pow_bits=0, **kw) == fs.expected_proof(ob.lib(), n, x, point, f, reps=5)[0], "pow_bits = 0: the version-1 bytes"
        for bits in (8, 12):
            want, p, _ = pw.expected_proof(ob.lib(), n, x, point, f, 5, bits)
            got = s.commit_fs(point, reps=5, pow_bits=bits, **kw)
            assert got == want, "not the proof assembled from the oracle at %d bits" % bits
            assert s.commit_fs(point, reps=5, pow_bits=bits, device_draws=False, **kw) == want, "the host's search gives other bytes"
            assert vp.Circuit.fs_pow(got) == (bits, p["nonce"]) and struct.unpack_from("<I", got, 4)[0] == 2
            for dev in (None, 0):
                assert vp.Circuit.verify_commitment_fs(got, device=dev, min_pow_bits=bits) == (True, "")
                ok, why = vp.Circuit.verify_commitment_fs(got, device=dev, min_pow_bits=bits + 1)
                assert ok is False and "proof of work" in why
            assert vp.Circuit.commitment_fs_challenges(got)[1] == p["leaf0"]
    finally:
        s.close()
        c.close()


def test_prove_full_fs_with_work_is_the_assembled_proof(vp, ob, small):
    c, s, reps = small
    _, layers, log_size, seed, _ = ff.FIXTURE
    oc = ob.Circuit.randomize(layers, log_size, seed=seed)
    assert s.prove_full_fs(reps=reps, pow_bits=0) == ff.fixture(), "pow_bits = 0: the version-1 bytes"
    got, pt = s.prove_full_fs(reps=reps, pow_bits=8, return_point=True)
    want, d = pw.assemble_full(oc, got, 8)
    assert got == want and pt.tobytes() == d["point"].tobytes() and c.fs_pow(got) == (8, d["nonce"])
    assert s.prove_full_fs(reps=reps, pow_bits=8, device_gkr=True) == want
    assert c.verify_full_fs(got) == (True, "") and c.verify_full_fs(got, device=0, min_pow_bits=8) == (True, "")
    for dev in (None, 0):
        ok, why = c.verify_full_fs(got, device=dev, min_pow_bits=9)
        assert ok is False and "proof of work" in why


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(vp, small):
    c, s, reps = small
    L, ctx = vp.lib_gpu(), vp.lib_host().vph_session_ctx(s.h)
    s.set_profiling(1)
    try:
        assert s.fs_grind(STATES[2], 3)[0] == pw.grind(STATES[2], 3)
        table = _rows(s)
        for bits, first, tries, null in ((0, 0, 10, None), (49, 0, 10, None), (-1, 0, 10, None), (4, 0, 0, None), (4, (1 << 64) - 5, 6, None), (4, 0, 10, 1), (4, 0, 10, 5), (4, 0, 10, 6)):
            assert raw(vp, s, STATES[2], bits, first, tries, null)[:2] == (VP_EINVAL, 0x1234), (bits, first, tries, null)
            assert "vp_fs_grind" in (L.vp_last_error(ctx) or b"").decode()
            assert _rows(s) == table, "a refused call launched something"
        assert raw(vp, s, STATES[2], 4, 0, 10, 0)[0] == VP_EINVAL
        point = fs.point_of(c.layer_bitlen(0))
        for call in (lambda: s.commit_fs(point, reps=3, pow_bits=33), lambda: s.prove_full_fs(reps=3, pow_bits=33), lambda: s.commit_fs(point, reps=3, pow_bits=-1)):
            with pytest.raises(ValueError):
                call()
        # ... and at the C entry points behind them: a bad argument, -1
        err, ln = ctypes.create_string_buffer(256), ctypes.c_uint64(0)
        pt = np.ascontiguousarray(point, np.uint64)
        H = vp.lib_host()
        assert H.vph_commit_fs_pow(s.h, pt.ctypes.data, pt.shape[0], 3, None, 0, None, 0, 0, 33, None, 0, ctypes.byref(ln), err, 256) == -1 and b"pow_bits" in err.value
        assert H.vph_prove_full_fs_pow(s.h, 3, None, 0, None, 0, None, 0, ctypes.byref(ln), None, 0, 33, err, 256) == -1 and b"pow_bits" in err.value
        assert _rows(s) == table
    finally:
        s.set_profiling(0)
    assert s.prove_full_fs(reps=reps) == ff.fixture(), "the session goes on working"


def test_a_sharded_session_refuses(vp):
    c = vp.Circuit.randomize(8, 12, seed=1)
    s = vp.Session(c, devices=[0] * 2, round_shard_min_log=2, shard_commitment=True)
    try:
        with pytest.raises(RuntimeError, match="not built for a sharded"):
            s.prove_full_fs(reps=3, pow_bits=8)
        with pytest.raises(RuntimeError, match="not built for a sharded"):
            s.commit_fs(fs.point_of(c.layer_bitlen(0)), reps=3, pow_bits=8)
        tr, ok, _ = s.prove_and_verify_full(reps=3)                        # the session goes on working
        assert ok
    finally:
        s.close()
        c.close()
