"""vp_prove_gkr_fs (include/vpgpu.h) on the device: the GKR sumchecks with every challenge drawn on the device from the Fiat-Shamir chain, and what stands on it —
Session.prove_gkr_fs, Session.prove_fs(device_draws=True), Session.prove_full_fs(device_gkr=True).  Every comparison is bit-exact.

reference    tests/gkr_fs_cases.py: vph_prove_fs's schedule with hashlib over the returned transcript, and two provers that take their tape up front — vp_prove_gkr
             (the batched plan: first pass and graph replay) and orc_prove_gkr_tape — on the returned tape.  A transcript that both reproduce on the tape derived
             from it is, by induction over the chain, the one non-interactive proof from that state (tests/full_fs_ref.py).  Session.prove_fs() — the host's chain
             driving the interactive entry points — is a second implementation of the whole thing: same bytes.

circuit                                          what it is there for
randomize(3, 7, seed 11), randomize(3, 9, 12)    the recorded joined proofs' circuits: every round fits one workgroup (k_round_fused_fs)
the same under VP_ROUND_FUSED_MAX=4              tiny tables through the arrival-counted closing (k_round_main_fs on one workgroup) beside fused rounds
randomize(8, 12, seed 1)                         2^12-entry tables: k_round_main_fs on several workgroups by default, the arrival counter between rounds
custom_a                                         every gate type, constants, assert gates (assert_random in use)
custom_d                                         a layer of unary gates only: no phase 2 (the chain goes from claim_u straight to sig), empty subsets in Liu
zero_var                                         layers of bit length 0: sumchecks of zero rounds (finalize only), an output layer that draws no r_liu
SHA-256 x1                                       real phase-2 table concatenations, sig over the full layer count

Per circuit: (a) prove_fs(device_draws=True) is prove_fs(), byte for byte; (b) tape, draw count and closing state are the hashlib schedule's over the transcript;
(c) vp_prove_gkr (first pass, replay) and the oracle return the transcript on the tape; (d) Circuit.verify_fs accepts, and rejects one flipped element; (e) a
second run, and runs behind an interactive proof and behind a vp_prove_gkr, give the same bytes; (f) from the zero, the all-ones and a recorded head state."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import custom_circuits as cc
import full_fs_ref as ff
import gkr_fs_cases as gf
import gkr_tape_cases as gc
import pc_masked_inputs as pmi

pytestmark = pytest.mark.gpu
VP_EINVAL = -1


@contextlib.contextmanager
def session(vp, c, env=None, **kw):
    env = env or {}
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s = vp.Session(c, **kw)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        yield s
    finally:
        s.close()


def fixture_head_state(ob):
    _, layers, log_size, seed, _ = ff.FIXTURE
    return gf.full_fs_head_state(ob.Circuit.randomize(layers, log_size, seed=seed), ff.fixture())[0]


def builders(golden, pws_path):
    a, d = golden["custom_a"]["custom"], golden["custom_d"]["custom"]
    custom = lambda arrays: (lambda mod: mod.Circuit.custom(*arrays))
    return {
        "rand3_7": lambda mod: mod.Circuit.randomize(*ff.FIXTURE[1:3], seed=ff.FIXTURE[3]),
        "rand3_9": lambda mod: mod.Circuit.randomize(*ff.FIXTURE_MASKED[1:3], seed=ff.FIXTURE_MASKED[3]),
        "rand8_12": lambda mod: mod.Circuit.randomize(8, 12, seed=1),
        "custom_a": custom(cc.make(a["seed"], a["sizes"])),
        "custom_d": custom(cc.make_unary_mid(d["seed"])),
        "zero_var": custom(cc.make_zero_var(21)),
        "sha256_x1": lambda mod: mod.Circuit.from_pws(pws_path, 1, seed=1),
    }


CASES = [("rand3_7", {}), ("rand3_9", {}), ("rand3_7", {"VP_ROUND_FUSED_MAX": "4"}), ("rand3_9", {"VP_ROUND_FUSED_MAX": "4"}), ("rand8_12", {}), ("custom_a", {}),
         ("custom_d", {}), ("zero_var", {}), ("sha256_x1", {})]


def check_run(c, oc, s, state):
    """(b) and (c) for one run from `state`; returns what the run returned"""
    off = gc.Offsets.of(oc)
    tr, tape, draws, st = s.prove_gkr_fs(state)
    want, want_draws, want_st = gf.reference(state, off, tr)
    bad = [i for i in range(off.n) if tape[i].tobytes() != want[i].tobytes()]
    assert not bad, "tape slots %r are not the schedule's over the returned transcript" % bad[:8]
    assert draws == want_draws and st == want_st
    t2, d2, s2 = c.gkr_fs_tape(tr, state)
    assert t2.tobytes() == tape.tobytes() and d2 == draws and s2 == st, "Circuit.gkr_fs_tape"
    return tr, tape, draws, st


def check_tape_forms(oc, s, tr, tape):
    s.set_tape(tape)
    first, _ = s.prove_gkr()
    replay, _ = s.prove_gkr()
    assert first == tr, "vp_prove_gkr (first pass) on the returned tape: " + str(gc.elements(first)[:1])
    assert replay == tr, "vp_prove_gkr (graph replay) on the returned tape"
    assert oc.prove_gkr_tape(tape)[0] == tr, "orc_prove_gkr_tape on the returned tape"


@pytest.mark.parametrize("name,env", CASES, ids=lambda x: x if isinstance(x, str) else "-".join("%s=%s" % kv for kv in x.items()) or "default")
def test_every_circuit(vp, ob, golden, pws_path, name, env):
    build = builders(golden, pws_path)[name]
    c, oc = build(vp), build(ob)
    assert c.hash() == oc.hash()
    head = fixture_head_state(ob)
    with session(vp, c, env, device=0) as s:
        if env:
            assert s.options_in_effect().round_fused_max == 4
        # (a) the host-chain path is the second implementation
        host_proof, _, host_ok = s.prove_fs()
        assert host_ok
        proof, res, verified = s.prove_fs(device_draws=True)
        assert verified is None, "the device form verifies nothing"
        assert proof == host_proof, "prove_fs(device_draws=True) is not prove_fs()"
        off = gc.Offsets.of(oc)
        assert res["rounds"] == gf.n_rounds(off) and res["gkr_device_ms"] > 0
        # (d)
        assert c.verify_fs(proof)
        bad = bytearray(proof)
        bad[16 * (off.n_tr // 2)] ^= 0x04
        assert not c.verify_fs(bytes(bad))
        # (e) behind the runs above, behind an interactive proof, behind a vp_prove_gkr, twice in a row
        first = check_run(c, oc, s, head)
        check_tape_forms(oc, s, first[0], first[1])                  # (c); leaves a vp_prove_gkr (and its graph) behind
        same = lambda r: r[0] == first[0] and r[1].tobytes() == first[1].tobytes() and r[2:] == first[2:]
        assert same(s.prove_gkr_fs(head)), "behind vp_prove_gkr"
        assert same(s.prove_gkr_fs(head)), "a second run"
        tr_i, _, ok_i = s.prove_interactive()
        assert ok_i
        assert same(s.prove_gkr_fs(head)), "behind an interactive proof"
        assert s.prove_fs(device_draws=True)[0] == proof and s.prove_fs()[0] == proof
        # (f)
        seen = {first[0]}
        for st_name, state in gf.START_STATES.items():
            r = check_run(c, oc, s, state)
            assert r[0] not in seen, st_name
            seen.add(r[0])
            check_tape_forms(oc, s, r[0], r[1])
        assert s.prove_interactive()[0] == tr_i, "the interactive path behind the device form"
    c.close()


def rows_of(s, state):
    s.set_profiling(1)
    try:
        out = s.prove_gkr_fs(state)
        return out, s.launch_stats()
    finally:
        s.set_profiling(0)


@pytest.mark.parametrize("name,fused_max", [("rand3_7", 512), ("rand3_7", 4), ("rand8_12", 512)])
def test_launch_table(vp, ob, golden, pws_path, name, fused_max):
    build = builders(golden, pws_path)[name]
    c, oc = build(vp), build(ob)
    off = gc.Offsets.of(oc)
    big, total = gf.rounds_beyond(oc, fused_max)
    assert total == gf.n_rounds(off)
    with session(vp, c, {"VP_ROUND_FUSED_MAX": str(fused_max)} if fused_max != 512 else {}, device=0) as s:
        assert s.options_in_effect().round_fused_max == fused_max
        plain = s.prove_gkr_fs(bytes(32))
        out, rows = rows_of(s, bytes(32))
        assert out[0] == plain[0] and out[1].tobytes() == plain[1].tobytes(), "profiling changes the bytes"
        assert {r["kernel"] for r in rows} <= {"k_round", "k_merkle"}, rows
        rounds = [r for r in rows if r["kernel"] == "k_round"]
        assert len(rounds) == big, "VP_K_ROUND rows: one per round with more pairs than a fused launch takes"
        assert all(r["rounds"] == 1 and r["work"] > fused_max and r["workgroups"] == min(2048, -(-r["work"] // 256)) for r in rounds)
        if name == "rand8_12":
            assert big > 0 and max(r["workgroups"] for r in rounds) == 8, "2^12-entry tables: round 1 on eight workgroups"
        elif fused_max == 4:
            assert big > 0 and {r["workgroups"] for r in rounds} == {1}
        else:
            assert big == 0
        # the single-lane launches carry every chain step that no round carries: all draws but one per round, all elements but three per round
        spans = [r for r in rows if r["kernel"] == "k_merkle"]
        assert all(r["workgroups"] == 1 for r in spans) and sum(r["work"] for r in spans) == gf.chain_steps(off) - 4 * total
        assert s.prove_fs(device_draws=True)[1]["rounds"] == total
    c.close()


def check_joined(c, s, reps, oc, consts=None, asserts=None, **kw):
    host, pt_host = s.prove_full_fs(reps=reps, return_point=True, **kw)
    dev, pt_dev = s.prove_full_fs(reps=reps, return_point=True, device_gkr=True, **kw)
    assert dev == host, "prove_full_fs(device_gkr=True) is not prove_full_fs()"
    assert pt_dev.tobytes() == pt_host.tobytes()
    okw = {"pri_mask": kw["mask"], "oracle_pub_mask": kw["pub_mask"]} if kw else {}
    want, d = ff.assemble(oc, dev, consts=consts, asserts=asserts, **okw)
    assert want == dev, "not the record the oracle assembles on the derived challenges"
    assert d["point"].tobytes() == pt_dev.tobytes()
    assert c.verify_full_fs(dev) == (True, "") and c.verify_full_fs(dev, device=0) == (True, "")
    assert s.prove_full_fs(reps=reps, device_gkr=True, **kw) == dev, "a second run"
    return dev


def test_joined_proof_on_the_recorded_circuits(vp, ob):
    _, layers, log_size, seed, reps = ff.FIXTURE
    c = vp.Circuit.randomize(layers, log_size, seed=seed)
    with session(vp, c, device=0) as s:
        assert check_joined(c, s, reps, ob.Circuit.randomize(layers, log_size, seed=seed)) == ff.fixture()
    c.close()
    _, layers, log_size, seed, reps = ff.FIXTURE_MASKED
    f = ff.masked_family()
    c = vp.Circuit.randomize(layers, log_size, seed=seed)
    with session(vp, c, device=0) as s:
        assert check_joined(c, s, reps, ob.Circuit.randomize(layers, log_size, seed=seed), mask=f["pri_mask"], pub_mask=f["pub_mask"]) == ff.fixture(masked=True)
    c.close()


def test_joined_proof_custom_a(vp, ob, golden):
    g = golden["custom_a"]["custom"]
    arrays = cc.make(g["seed"], g["sizes"])
    c = vp.Circuit.custom(*arrays)
    with session(vp, c, device=0) as s:
        check_joined(c, s, 5, ob.Circuit.custom(*arrays), consts=arrays[5], asserts=arrays[6])
        f = pmi.family("short_pub", c.layer_bitlen(0), 8)
        check_joined(c, s, 5, ob.Circuit.custom(*arrays), consts=arrays[5], asserts=arrays[6], mask=f["pri_mask"], pub_mask=f["pub_mask"])
    c.close()


def test_joined_proof_sha256_x1(vp, ob, pws_path):
    c = vp.Circuit.from_pws(pws_path, 1, seed=1)
    with session(vp, c, device=0) as s:
        check_joined(c, s, 4, ob.Circuit.from_pws(pws_path, 1, seed=1))
    c.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def raw(vp, ctx, nt, nb, state=bytes(32), capacity=None, null=None):
    """vp_prove_gkr_fs as it is: (return code, transcript, tape)"""
    L = vp.lib_gpu()
    vpt, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.vp_prove_gkr_fs.argtypes = [vpt, vpt, vpt, u64, ctypes.POINTER(u64), vpt, ctypes.POINTER(u64), vpt]
    buf, tape = ctypes.create_string_buffer(max(nb, 1)), np.zeros((max(nt, 1), 2), np.uint64)
    si, so, nw, nd = ctypes.create_string_buffer(state, 32), ctypes.create_string_buffer(32), u64(0), u64(0)
    arg = {"state_in": ctypes.cast(si, vpt), "transcript": ctypes.cast(buf, vpt), "tape_out": tape.ctypes.data, "n_draws": ctypes.byref(nd), "state_out": ctypes.cast(so, vpt)}
    if null:
        arg[null] = None
    rc = L.vp_prove_gkr_fs(ctx, arg["state_in"], arg["transcript"], nb if capacity is None else capacity, ctypes.byref(nw), arg["tape_out"], arg["n_draws"], arg["state_out"])
    return rc, buf.raw[:nw.value], tape


def test_refusals_leave_the_context_as_it_was(vp):
    c = vp.Circuit.randomize(8, 12, seed=1)
    nt, nb = c.gkr_sizes()
    with session(vp, c, device=0) as s:
        honest = s.prove_gkr_fs(bytes(32))
        inter = s.prove_interactive()[0]
        s.draw_tape()
        batched = s.prove_gkr()[0]

        def unchanged(what):
            r = s.prove_gkr_fs(bytes(32))
            assert r[0] == honest[0] and r[1].tobytes() == honest[1].tobytes() and r[2:] == honest[2:], what
            assert s.prove_gkr()[0] == batched and s.prove_interactive()[0] == inter, what
        ctx = s.gpu_ctx()
        rc, tr, tape = raw(vp, ctx, nt, nb)
        assert rc == 0 and tr == honest[0] and tape.tobytes() == honest[1].tobytes()
        for null in ("state_in", "transcript", "tape_out", "n_draws", "state_out"):
            assert raw(vp, ctx, nt, nb, null=null)[0] == VP_EINVAL, null
        assert raw(vp, ctx, nt, nb, capacity=nb - 1)[0] == VP_EINVAL and raw(vp, ctx, nt, nb, capacity=0)[0] == VP_EINVAL
        unchanged("after null arguments and a short buffer")
        for bad_state in (b"", bytes(31), bytes(33)):
            with pytest.raises(ValueError):
                s.prove_gkr_fs(bad_state)
        # chain-sharded, then index-split on top of it
        s.set_shard(0, 2)
        assert raw(vp, ctx, nt, nb)[0] == VP_EINVAL
        for call in (lambda: s.prove_gkr_fs(bytes(32)), lambda: s.prove_fs(device_draws=True), lambda: s.prove_full_fs(reps=3, device_gkr=True)):
            with pytest.raises(RuntimeError, match="shard"):
                call()
        s.set_shard_split(11)
        assert raw(vp, ctx, nt, max(nb, 1 << 20))[0] == VP_EINVAL
        s.set_shard_split(0)
        s.set_shard(0, 1)
        unchanged("after the sharded refusals")
    # a round-sharded session
    with session(vp, c, devices=[0] * 2, round_shard_min_log=2) as s2:
        for r in range(2):
            assert raw(vp, s2.rank_ctx(r), nt, nb)[0] == VP_EINVAL
        for call in (lambda: s2.prove_gkr_fs(bytes(32)), lambda: s2.prove_fs(device_draws=True), lambda: s2.prove_full_fs(reps=3, device_gkr=True)):
            with pytest.raises(RuntimeError, match="sharded"):
                call()
        assert s2.prove_interactive()[0] == inter, "the round-sharded session goes on working"
    # a context that has not evaluated anything
    L, fresh = vp.lib_gpu(), ctypes.c_void_p()
    assert L.vp_create_with_options(0, None, ctypes.byref(fresh)) == 0
    try:
        assert raw(vp, fresh, nt, nb)[0] == VP_EINVAL
    finally:
        L.vp_destroy(fresh)
    c.close()
