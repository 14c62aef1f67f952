"""GPU (-m gpu): the interactive sumchecks of one proof sharded by index over ranks (include/vpgpu.h: vp_set_round_shard).  The ranks run as
contexts on one GPU; the prover sums their partial round polynomials, so the transcript must be the unsharded one, byte for byte."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN as GOLDEN_DIR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = (1 << 61) - 1
VP_EINVAL, VP_ELIMIT, VP_EXCHANGE = -1, -5, 1


def _sharded(vp, c, world, min_log=2):
    return vp.Session(c, devices=[0] * world, round_shard_min_log=min_log)


def _prove(vp, c, world, gold, min_log=2):
    s = _sharded(vp, c, world, min_log)
    assert s.world() == world
    tr, res, ok = s.prove_interactive()
    assert ok, "host verifier rejected the round-sharded proof (W=%d)" % world
    assert tr == gold, "round-sharded transcript differs (W=%d)" % world
    return s


@pytest.mark.parametrize("name,blocks,worlds", [("sha256_x16", 16, (2, 4, 8)), ("sha256_x64", 64, (2, 8))])
def test_round_sharded_sha256_matches_reference(vp, golden, gold_gkr, pws_path, name, blocks, worlds):
    c = vp.Circuit.from_pws(pws_path, blocks, seed=1)
    assert c.hash() == golden[name]["circuit_hash"]
    for w in worlds:
        _prove(vp, c, w, gold_gkr(name)).close()
    c.close()


def test_round_sharded_randomize_complex_values(vp, gold_gkr):
    c = vp.Circuit.randomize(8, 12, seed=1)
    for w in (2, 4, 8):
        _prove(vp, c, w, gold_gkr("randomize_8_12")).close()
    c.close()


def test_round_sharded_custom_circuits_every_gate_type(vp, ob):
    import custom_circuits as cc
    for seed, sizes in ((7, [3000, 2800, 1500, 2700, 900]), (77, [700, 300, 129, 257, 64, 5])):
        c = vp.Circuit.custom(*cc.make(seed, sizes)); oc = ob.Circuit.custom(*cc.make(seed, sizes))
        assert c.hash() == oc.hash()
        gold, st = oc.prove_gkr()
        assert st["verified"] == 1
        for w in (2, 4, 8):
            _prove(vp, c, w, gold).close()
        c.close(); oc.close()


def test_round_sharded_x1024(vp, golden, gold_gkr, pws_path):
    c = vp.Circuit.from_pws(pws_path, 1024, seed=1)
    assert c.hash() == golden["sha256_x1024"]["circuit_hash"]
    _prove(vp, c, 4, gold_gkr("sha256_x1024"), min_log=11).close()
    c.close()


def test_round_sharded_full_protocol_with_commitment(vp, golden, pws_path):
    c = vp.Circuit.from_pws(pws_path, 16, seed=1)
    gold = open(os.path.join(GOLDEN_DIR, golden["sha256_x16"]["transcript"]), "rb").read()
    s = _sharded(vp, c, 4)
    tr, ok, _ = s.prove_and_verify_full(reps=33)
    assert ok, "complete protocol rejected on a round-sharded session"
    assert tr[:len(gold)] == gold
    s.close(); c.close()


def test_round_sharded_batched_proof_and_device_predicates(vp, golden, gold_gkr, pws_path):
    """The verifier-side helpers on a round-sharded session: vp_liu_gr (device predicates) builds the whole Liu table on rank 0, so the batched
    complete protocol and a replay with the predicate loops on the device accept, after a sharded interactive proof as before it."""
    c = vp.Circuit.from_pws(pws_path, 16, seed=1)
    gold = open(os.path.join(GOLDEN_DIR, golden["sha256_x16"]["transcript"]), "rb").read()
    s = _sharded(vp, c, 4)
    for _ in range(2):
        tr, ok = s.prove_full(batched=True)
        assert ok and tr == gold, "batched complete protocol on a round-sharded session"
        s.draw_tape()
        ok, _ = s.check(gold_gkr("sha256_x16"), device_predicates=True)
        assert ok, "replay with device predicates rejected on a round-sharded session"
        tr, _, ok = s.prove_interactive()
        assert ok and tr == gold_gkr("sha256_x16")
    s.close(); c.close()


def test_round_sharded_work_is_split(vp, gold_gkr, pws_path):
    c = vp.Circuit.from_pws(pws_path, 16, seed=1)
    w = 4
    s = _prove(vp, c, w, gold_gkr("sha256_x16"))
    part = s.partials().astype(object)                      # (rounds, world, 3, 2)
    assert part.shape[0] > 0 and part.shape[1] == w
    full = part.sum(axis=1) % P
    # some rank's partial is not the round polynomial (the split rounds), and the partials always sum to it (the transcript is the golden one)
    assert any(not np.array_equal(part[r, k] % P, full[r]) for r in range(part.shape[0]) for k in range(w))
    # round stats of the split single-table phases (phase 1, Liu): before the gather the ranks' bytes add up to an unsharded context's, each a share
    one = vp.Session(c)
    one.prove_interactive()
    st1 = one.round_stats()
    sts = [s.round_stats(rank=r) for r in range(w)]
    assert all(len(x) == len(st1) for x in sts)
    split = 0
    for i, e in enumerate(st1):
        b = [sts[r][i]["bytes"] for r in range(w)]
        if e["phase"] in (1, 3) and max(b) < e["bytes"]:
            assert sum(b) == e["bytes"], (e, b)
            assert b[0] * w >= e["bytes"]          # rank 0 holds the fullest slice of a padded table
            assert all(sts[r][i]["how"] != 1 for r in range(w)), "resident kernel on a phase that is still split"
            split += 1
        elif e["phase"] in (1, 3):
            assert b == [e["bytes"]] * w
    assert split > 0, "no split round"
    # ranks that share a device run without the resident round kernel (host/prover.cpp): on one GPU every round is a direct launch
    assert all(x["how"] != 1 for r in range(w) for x in sts[r])
    one.close(); s.close(); c.close()


def test_round_sharded_missing_rank_is_rejected(vp, pws_path):
    c = vp.Circuit.from_pws(pws_path, 16, seed=1)
    s = _sharded(vp, c, 4)
    s.drop_rank(2)
    tr, res, ok = s.prove_interactive()
    assert not ok, "a proof without rank 2's partials was accepted"
    s.drop_rank(-1)
    tr, res, ok = s.prove_interactive()
    assert ok
    s.close(); c.close()


def test_round_shard_refusals(vp, gold_gkr, pws_path):
    L = vp.lib_gpu()
    c = vp.Circuit.from_pws(pws_path, 16, seed=1)
    s = vp.Session(c)
    ctx = s.gpu_ctx()
    assert L.vp_set_round_shard(ctx, 0, 3, 2) == VP_EINVAL
    assert L.vp_set_round_shard(ctx, 0, 16, 2) == VP_ELIMIT
    assert L.vp_set_round_shard(ctx, 4, 4, 2) == VP_EINVAL
    assert L.vp_set_round_shard(ctx, 0, 1, 2) == 0             # world 1: the ordinary context
    tr, res, ok = s.prove_interactive()
    assert ok and tr == gold_gkr("sha256_x16")
    s.close()
    # in the middle of a phase, and a repeated vp_round while the gather is pending, on the contexts of a sharded session
    s = _sharded(vp, c, 2)
    ctxs = [s.rank_ctx(r) for r in range(2)]
    n = c.layers
    one = (ctypes.c_uint64 * 2)(1, 0)
    r_liu = (ctypes.c_uint64 * (2 * 64))()
    for k in range(64):
        r_liu[2 * k] = k + 3
    for x in ctxs:
        assert L.vp_phase1_init(x, n - 1, r_liu, one) == 0
    assert L.vp_set_round_shard(ctxs[0], 0, 2, 2) == VP_EINVAL          # a sumcheck is in progress
    live = ctypes.c_int(0)
    assert L.vp_get_round_shard(ctxs[0], None, None, ctypes.byref(live)) == 0
    poly = (ctypes.c_uint64 * 6)()
    rv = (ctypes.c_uint64 * 2)(5, 0)
    rc = 0
    rounds = c.layer_bitlen(n - 2)
    got_x = False
    for k in range(rounds):
        rcs = [L.vp_round(x, rv, poly) for x in ctxs]
        if rcs[0] == VP_EXCHANGE:
            got_x = True
            assert rcs == [VP_EXCHANGE, VP_EXCHANGE]
            assert L.vp_round(ctxs[0], rv, poly) == VP_EXCHANGE         # still pending: again, nothing changes
            npend = ctypes.c_int(0)
            assert L.vp_shard_pending(ctxs[0], ctypes.byref(npend)) == 0 and npend.value == 1
            arr = (ctypes.c_void_p * 2)(*[x.value for x in ctxs])
            assert L.vp_shard_exchange_local(arr, 2) == 0
            assert [L.vp_round(x, rv, poly) for x in ctxs] == [0, 0]
        else:
            assert rcs == [0, 0]
    assert got_x == bool(live.value)
    claims = (ctypes.c_uint64 * 2)()
    for x in ctxs:
        assert L.vp_finalize(x, rv, claims, 1) == 0
    assert L.vp_set_round_shard(ctxs[0], 0, 2, 2) == 0
    s.close()
    c.close()


def test_round_shard_refused_with_a_communicator(vp):
    """RCCL inside vp_round is out of scope: a context with a communicator attached (one rank, this GPU) refuses vp_set_round_shard."""
    L = vp.lib_gpu()
    uid = ctypes.create_string_buffer(128)
    assert L.vp_comm_unique_id(ctypes.cast(uid, ctypes.c_void_p)) == 0
    ctx = ctypes.c_void_p()
    assert L.vp_create(0, ctypes.byref(ctx)) == 0
    try:
        assert L.vp_set_round_shard(ctx, 0, 2, 2) == 0 and L.vp_set_round_shard(ctx, 0, 1, 2) == 0       # no communicator yet: accepted
        assert L.vp_comm_init(ctx, ctypes.cast(uid, ctypes.c_void_p), 0, 1) == 0, L.vp_last_error(ctx)
        assert L.vp_set_round_shard(ctx, 0, 2, 2) == VP_EINVAL
        assert L.vp_comm_destroy(ctx) == 0
    finally:
        L.vp_destroy(ctx)


_CHECKED_WORKER = r"""
import sys
sys.path.insert(0, %r)
import vp_loader
vp = vp_loader.load()
vp.lib_host()
assert vp.lib_gpu().vp_checked_build() == 1, "VP_LIBGPU did not select the checked library"
pws, gold_path, a, b = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
c = vp.Circuit.from_pws(pws, 16, seed=1)
s = vp.Session(c, devices=[0] * 4, round_shard_min_log=2)
tr, _, ok = s.prove_interactive()
gold = open(gold_path, "rb").read()[a:b]
assert ok and tr == gold, "checked build: round-sharded transcript differs"
print("CHECKED OK", flush=True)
"""


def test_round_sharded_checked_build(vp, golden, pws_path):
    import subprocess, sys
    assert os.path.exists(vp.LIB_GPU_CHECKED)
    env = dict(os.environ, VP_LIBGPU=vp.LIB_GPU_CHECKED)
    g = golden["sha256_x16"]
    gold = os.path.join(GOLDEN_DIR, g["transcript"])
    r = subprocess.run([sys.executable, "-c", _CHECKED_WORKER % ROOT, pws_path, gold, str(g["gkr_slice"][0]), str(g["gkr_slice"][1])],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-2000:])
    assert "CHECKED OK" in r.stdout
