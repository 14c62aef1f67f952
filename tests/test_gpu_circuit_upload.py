"""GPU (-m gpu): vp_circuit_upload through the raw C ABI (vp.lib_gpu()) — what it refuses, what a refusal leaves behind, and what replacing a circuit on one
context leaves behind.  Descriptions come from tests/upload_desc.py (build: the reference's subset rule; validate: the contract as a function of the
description; CASES: the malformed rows; tests/test_upload_desc_host.py checks all three on the CPU).  Every transcript and root is compared byte for byte with
the oracle's on the same arrays and the same tape; there are no tolerances here.

Refusals: the helper asserts vp_circuit_upload's return code FIRST.  A library that accepts a malformed description fails there and the test ends there — such a
context is never evaluated, proved with or reused, only destroyed by the fixture's finaliser.  After a refusal past the argument checks every entry point must
answer VP_EINVAL without launching anything, and the unmutated description must then upload and prove on the same context.

Replacement (R1 - R6): two circuits in turn on one context, with a real-value witness, an open sumcheck, a captured graph, a commitment and an index split in
effect when the circuit is replaced; each proof equals the one of a fresh context and the oracle's."""
import ctypes
import functools

import numpy as np
import pytest

import custom_circuits as cc
import gkr_drive
import gkr_tape_cases as gc
import pc_array_inputs as pai
import upload_desc as ud
from test_gpu_parity import _kind

pytestmark = pytest.mark.gpu
VP_OK, VP_EINVAL, VP_ELIMIT = ud.VP_OK, ud.VP_EINVAL, ud.VP_ELIMIT


class Stats(ctypes.Structure):      # vp_stats
    _fields_ = [("gkr_ms", ctypes.c_double), ("evaluate_ms", ctypes.c_double), ("fold_ms", ctypes.c_double), ("fold_launches", ctypes.c_uint64),
                ("fold_bytes", ctypes.c_uint64), ("rounds", ctypes.c_uint64), ("launches", ctypes.c_uint64)]


def _bind(lib):
    p, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    gkr_drive._bind(lib)
    lib.vp_circuit_upload.argtypes = [p, i, p]
    lib.vp_evaluate.argtypes = [p, p, u64]
    lib.vp_layer_values.argtypes = [p, i, p, u64]
    lib.vp_layer_mle.argtypes = [p, i, p, i, p]
    lib.vp_prove_gkr.argtypes = [p, p, u64, p, u64, p]
    lib.vp_shard_chains.argtypes = [p, p, p, i, p]
    lib.vp_get_stats.argtypes = [p, p]
    lib.vp_set_shard.argtypes = [p, i, i]


class Raw:
    """One vp_ctx and the calls of this file on it."""

    def __init__(self, vp, options=None):
        self.vp, self.L = vp, vp.lib_gpu()
        _bind(self.L)
        self.c = ctypes.c_void_p()
        assert self.L.vp_create_with_options(0, ctypes.byref(options) if options is not None else None, ctypes.byref(self.c)) == 0

    def err(self):
        return (self.L.vp_last_error(self.c) or b"").decode()

    def upload_rc(self, desc, n_layers=None, null=False):
        arr, keep = ud.to_ctypes(desc)
        rc = self.L.vp_circuit_upload(self.c, len(desc) if n_layers is None else n_layers, None if null else ctypes.cast(arr, ctypes.c_void_p))
        del keep
        return rc

    def upload(self, desc):
        assert self.upload_rc(desc) == VP_OK, self.err()

    def evaluate_rc(self, inputs, n=None):
        w = np.ascontiguousarray(inputs, np.uint64)
        return self.L.vp_evaluate(self.c, w.ctypes.data, w.shape[0] if n is None else n)

    def sizes_rc(self):
        nt, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        return self.L.vp_gkr_sizes(self.c, ctypes.byref(nt), ctypes.byref(nb)), nt.value, nb.value

    def prove_rc(self, tape, n_tape=None):
        t = np.ascontiguousarray(tape, np.uint64)
        rc, _, nb = self.sizes_rc()
        buf = ctypes.create_string_buffer(max(nb if rc == 0 else 0, 16) + 64)
        n = ctypes.c_uint64(0)
        rc = self.L.vp_prove_gkr(self.c, t.ctypes.data, t.shape[0] if n_tape is None else n_tape, ctypes.cast(buf, ctypes.c_void_p), len(buf), ctypes.byref(n))
        return rc, buf.raw[:n.value]

    def prove(self, tape):
        rc, tr = self.prove_rc(tape)
        assert rc == VP_OK, self.err()
        return tr

    def layer_values_rc(self, layer, n):
        out = np.zeros((max(n, 1), 2), np.uint64)
        return self.L.vp_layer_values(self.c, layer, out.ctypes.data, n), out[:n]

    def shard_chains_rc(self):
        owner, cost, n = np.zeros(256, np.int32), np.zeros(256, np.float64), ctypes.c_int(0)
        rc = self.L.vp_shard_chains(self.c, owner.ctypes.data, cost.ctypes.data, 256, ctypes.byref(n))
        return rc, owner[:n.value]

    def vres_rc(self, bits):
        r, out = np.zeros((max(bits, 1), 2), np.uint64), np.zeros((1, 2), np.uint64)
        r[:, 0] = 3
        return self.L.vp_vres(self.c, r.ctypes.data, bits, out.ctypes.data)

    def phase1_rc(self, layer, bits):
        r, ar = np.zeros((max(bits, 1), 2), np.uint64), np.ones((1, 2), np.uint64)
        r[:, 0] = 5
        return self.L.vp_phase1_init(self.c, layer, r.ctypes.data, ar.ctypes.data)

    def round_rc(self):
        prev, poly = np.zeros((1, 2), np.uint64), np.zeros((3, 2), np.uint64)
        return self.L.vp_round(self.c, prev.ctypes.data, poly.ctypes.data), poly

    def finalize_rc(self, n_claims):
        prev, cl = np.zeros((1, 2), np.uint64), np.zeros((max(n_claims, 1), 2), np.uint64)
        return self.L.vp_finalize(self.c, prev.ctypes.data, cl.ctypes.data, n_claims)

    def commit_private_rc(self):
        root = ctypes.create_string_buffer(32)
        return self.L.vp_commit_private(self.c, ctypes.cast(root, ctypes.c_void_p)), root.raw

    def commit_public_eq_rc(self, point):
        root, inner, alls = ctypes.create_string_buffer(32), np.zeros(2, np.uint64), np.zeros((65, 2), np.uint64)
        pt = np.ascontiguousarray(point, np.uint64)
        return self.L.vp_commit_public_eq(self.c, pt.ctypes.data, pt.shape[0], inner.ctypes.data, alls.ctypes.data, ctypes.cast(root, ctypes.c_void_p)), root.raw

    def launches(self):
        st = Stats()
        assert self.L.vp_get_stats(self.c, ctypes.byref(st)) == 0
        return int(st.launches)

    def round_stats_n(self):
        n = ctypes.c_int(-1)
        assert self.L.vp_get_round_stats(self.c, None, 0, ctypes.byref(n)) == 0
        return n.value

    def real_values(self):
        o = self.vp.Options()
        assert self.L.vp_get_options(self.c, ctypes.byref(o)) == 0
        return o.real_values

    def close(self):
        if self.c:
            self.L.vp_destroy(self.c)
            self.c = None


@pytest.fixture
def ctxs(vp):
    """Function-scoped contexts: make() hands out a fresh one, the finaliser destroys every one of them — the only thing that ever happens to a context whose
    upload answered something the test did not expect."""
    made = []

    def make(options=None):
        made.append(Raw(vp, options))
        return made[-1]
    yield make
    for r in made:
        r.close()


class Circ:
    """A circuit of custom_circuits: its description, witness, the oracle's circuit, tape layout, uniform tape and the oracle's transcript on it."""

    def __init__(self, ob, arrays):
        self.arrays = arrays
        self.desc = ud.build(*arrays)
        self.inputs = ud.inputs_of(arrays[0], arrays[3])
        self.oc = ob.Circuit.custom(*arrays)
        self.off = gc.Offsets.of(self.oc)
        assert self.off.n == self.oc.gkr_draws()
        self.tape = gc.uniform(self.off, gc.SEED)
        self.gold, st = self.oc.prove_gkr_tape(self.tape)
        assert st["verified"] == 1 and len(self.gold) == 16 * self.off.n_tr

    def gold_on(self, tape):
        return self.oc.prove_gkr_tape(tape)[0]


_CIRCS = {}


def _circ(ob, key, make):
    """The reference of a circuit is computed once per process, shared by the tests that need it and never modified."""
    if key not in _CIRCS:
        _CIRCS[key] = Circ(ob, make())
    return _CIRCS[key]


def _base(ob, key):
    return _circ(ob, key, ud.BASES[key])


def _load_and_prove(r, c):
    """upload, evaluate, batched proof on the uniform tape == the oracle's"""
    r.upload(c.desc)
    assert r.evaluate_rc(c.inputs) == VP_OK, r.err()
    assert r.prove(c.tape) == c.gold


def _follow_ups_refused(r, c):
    """Every entry point on a context whose upload was refused: VP_EINVAL, nothing launched."""
    before = r.launches()
    n, off = len(c.desc), c.off
    assert r.evaluate_rc(c.inputs) == VP_EINVAL, "vp_evaluate with the refused circuit's input count"
    assert r.evaluate_rc(c.inputs, 0) == VP_EINVAL, "vp_evaluate with no inputs"
    assert r.sizes_rc()[0] == VP_EINVAL, "vp_gkr_sizes"
    assert r.shard_chains_rc()[0] == VP_EINVAL, "vp_shard_chains"
    assert r.layer_values_rc(0, 1)[0] == VP_EINVAL, "vp_layer_values(0)"
    assert r.vres_rc(off.bl[n - 1]) == VP_EINVAL, "vp_vres"
    assert r.phase1_rc(n - 1, off.bl[n - 1]) == VP_EINVAL, "vp_phase1_init"
    assert r.prove_rc(c.tape)[0] == VP_EINVAL and r.prove_rc(c.tape, 0)[0] == VP_EINVAL, "vp_prove_gkr"
    assert r.commit_private_rc()[0] == VP_EINVAL, "vp_commit_private"
    assert r.round_rc()[0] == VP_EINVAL, "vp_round"
    assert r.launches() == before


# ---- the refusal table ------------------------------------------------------------------------------------------------------------------------------------
_FIRST_OF_GROUP = {g: next(c.name for c in ud.CASES if c.group == g and c.want[0] != VP_OK and c.n_layers is None and not c.null_desc) for g in ud.GROUPS}


def _desc_arrays(desc, inputs):
    """The seven arrays of an (accepted) description, for the oracle."""
    sizes = np.array([d["size"] for d in desc], np.uint64)
    n0 = desc[0]["size"]
    cat = lambda k, dt, zero: np.concatenate([zero(n0)] + [np.asarray(d[k]).astype(dt) if d.get(k) is not None else zero(d["size"]) for d in desc[1:]])
    ty = cat("ty", np.int32, lambda n: np.full(n, cc.INPUT, np.int32))
    l = cat("l", np.int32, lambda n: np.full(n, -1, np.int32))
    u = cat("u", np.uint64, lambda n: inputs[:n, 0].copy())
    v = cat("v", np.uint64, lambda n: np.zeros(n, np.uint64))
    c = np.concatenate([np.zeros((n0, 2), np.uint64)] + [d["c"] if d.get("c") is not None else np.zeros((d["size"], 2), np.uint64) for d in desc[1:]])
    a = cat("is_assert", np.uint8, lambda n: np.zeros(n, np.uint8))
    return sizes, ty, l, u, v, c, a


@pytest.mark.parametrize("case", ud.CASES, ids=lambda c: c.name)
def test_upload_refusal_table(ctxs, ob, case):
    """One row: upload the mutated description — return code and vp_last_error are validate()'s — then the follow-ups.  The first refused row of each group also
    recovers: the unmutated description uploads on the same context and its proof is the oracle's.  Rows that validate() accepts (the controls) are proved against
    the oracle on the mutated arrays.  VP_UPLOAD_TABLE_ONLY=1 in the environment ends every row behind the return code and the error text: that is how the table is
    run against a library whose validation was weakened on purpose (README, mutation table), whose contexts must never be used after the upload."""
    import os
    base = _base(ob, case.base)
    desc = case.mutate(base.desc)
    want = ud.validate(None if case.null_desc else desc, case.n_layers)
    assert want == case.want                                     # (the host test's statement; the expected column is validate's)
    r = ctxs()
    rc = r.upload_rc(desc, n_layers=case.n_layers, null=case.null_desc)
    print("%s: rc %d, '%s'" % (case.name, rc, r.err()))
    assert rc == want[0], "vp_circuit_upload answered %d ('%s'), the contract says %r" % (rc, r.err(), want)
    if want[1] is not None:
        assert r.err() == want[1]
    if os.environ.get("VP_UPLOAD_TABLE_ONLY"):
        return
    if want[0] == VP_OK:
        if ud.differences(base.desc, desc) == [] or case.name == "empty_subset_bitlen_int_min_ok":
            gold = base.gold
        else:
            oc = ob.Circuit.custom(*_desc_arrays(desc, base.inputs))
            gold = oc.prove_gkr_tape(base.tape)[0]
            oc.close()
        assert r.evaluate_rc(base.inputs) == VP_OK, r.err()
        assert r.prove(base.tape) == gold
        return
    _follow_ups_refused(r, base)
    if case.name == _FIRST_OF_GROUP[case.group]:
        _load_and_prove(r, base)


def test_argument_refusals_keep_the_previous_circuit(ctxs, ob):
    """ld = NULL, n_layers 1 and 65 are refused before the context is touched: the circuit uploaded before them still proves."""
    base = _base(ob, "base")
    r = ctxs()
    r.upload(base.desc)
    assert r.evaluate_rc(base.inputs) == VP_OK
    assert r.upload_rc(base.desc, null=True) == VP_EINVAL
    assert r.upload_rc(base.desc, n_layers=1) == VP_EINVAL
    assert r.upload_rc(base.desc, n_layers=65) == VP_ELIMIT and r.err() == "too many layers"
    assert r.prove(base.tape) == base.gold


def test_refused_upload_discards_the_previous_circuit(ctxs, ob):
    """A refusal past the argument checks leaves an EMPTY context, not the previous circuit and not a half-built one: the follow-ups answer VP_EINVAL with the
    previous circuit's own arguments too."""
    base, wide = _base(ob, "base"), _base(ob, "wide")
    r = ctxs()
    _load_and_prove(r, wide)
    bad = [c for c in ud.CASES if c.name == "bad_u_layer_last_gate_last"][0].mutate(base.desc)       # layers 1 .. 3 are built before the last one is refused
    assert r.upload_rc(bad) == VP_EINVAL and r.err() == "gate.u out of range"
    _follow_ups_refused(r, base)
    _follow_ups_refused(r, wide)
    _load_and_prove(r, base)


# ---- the helper's positive control ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "unary_mid"])
def test_raw_upload_equals_the_session_and_the_oracle(vp, ctxs, ob, name):
    """build()'s description through the raw ABI gives the transcript of Session(Circuit.custom(...)) and of the oracle."""
    c = _base(ob, "base") if name == "base" else _circ(ob, "unary_mid", lambda: cc.make_unary_mid(104))
    r = ctxs()
    _load_and_prove(r, c)
    assert gkr_drive.prove(vp, r.c, c.off, c.tape)[0] == c.gold
    hc = vp.Circuit.custom(*c.arrays)
    s = vp.Session(hc)
    s.set_tape(c.tape)
    tr, _ = s.prove_gkr()
    vals = s.layer_values(len(c.desc) - 1)
    s.close(); hc.close()
    assert tr == c.gold
    rc, got = r.layer_values_rc(len(c.desc) - 1, c.desc[-1]["size"])
    assert rc == VP_OK and np.array_equal(got, vals)


# ---- replacement on one context ---------------------------------------------------------------------------------------------------------------------------
REAL_VALUES = (0, 1, 2, 3, 5, 7, cc.P - 1, cc.P - 2)


def _real(ob, key, seed, sizes):
    return _circ(ob, key, lambda: cc.make(seed, sizes, values=REAL_VALUES, real_consts=True))


def _assert_real_path(r, c):
    assert r.real_values() == 1
    for i, d in enumerate(c.desc):
        rc, v = r.layer_values_rc(i, d["size"])
        assert rc == VP_OK and not v[:, 1].any(), "layer %d has a complex value: the real-value path is not taken" % i


def test_r1_layer_count_changes_on_an_all_real_circuit(ctxs, ob):
    """5 layers, 9 layers, 5 layers on one context, every value real: the per-layer table of real parts is rebuilt for each circuit's own layer count."""
    a, b = _real(ob, "real5", 31, [40, 33, 50, 17, 9]), _real(ob, "real9", 32, [40, 33, 50, 17, 29, 12, 21, 9, 6])
    fresh = {}
    for k, c in (("a", a), ("b", b)):
        f = ctxs()
        _load_and_prove(f, c)
        _assert_real_path(f, c)
        fresh[k] = f.prove(c.tape)
    r = ctxs()
    for k, c in (("a", a), ("b", b), ("a", a)):
        _load_and_prove(r, c)
        _assert_real_path(r, c)
        assert r.prove(c.tape) == fresh[k] == c.gold


def _open_sumcheck(r, c):
    n = len(c.desc)
    assert r.vres_rc(c.off.bl[n - 1]) == VP_OK, r.err()
    assert r.phase1_rc(n - 1, c.off.bl[n - 1]) == VP_OK, r.err()
    assert r.round_rc()[0] == VP_OK, r.err()
    assert r.round_stats_n() == 1


def _sumcheck_is_closed(r):
    assert r.round_rc()[0] == VP_EINVAL, "vp_round folds the tables of the circuit that was replaced"
    assert r.finalize_rc(1) == VP_EINVAL, "vp_finalize"
    assert r.round_stats_n() == 0


@pytest.mark.parametrize("persistent", [1, 0])
def test_r2_open_sumcheck_when_the_circuit_is_replaced(vp, ctxs, ob, persistent):
    a, b = _base(ob, "base"), _base(ob, "wide")
    r = ctxs(vp.Options(persistent_rounds=persistent))
    _load_and_prove(r, a)
    _open_sumcheck(r, a)
    r.upload(b.desc)
    _sumcheck_is_closed(r)
    assert r.evaluate_rc(b.inputs) == VP_OK, r.err()
    _sumcheck_is_closed(r)
    assert gkr_drive.prove(vp, r.c, b.off, b.tape)[0] == b.gold
    assert r.prove(b.tape) == b.gold


@pytest.mark.parametrize("persistent", [1, 0])
def test_r3_open_sumcheck_when_an_input_layer_is_loaded(vp, ctxs, ob, persistent):
    a = _base(ob, "base")
    x = pai.inputs("uniform", 8)
    want = pai.split_record(pai.oracle_record(ob.lib(), x["values"], x["n_used"], x["pub"], 8, x["r"]), 8)
    r = ctxs(vp.Options(persistent_rounds=persistent))
    _load_and_prove(r, a)
    _open_sumcheck(r, a)
    before = r.launches()
    assert r.L.vp_pc_load_input(r.c, x["values"].ctypes.data, x["n_used"], 8) == VP_OK, r.err()
    _sumcheck_is_closed(r)
    # the GKR entry points: there is a witness (the loaded layer) but no circuit
    n = len(a.desc)
    assert r.vres_rc(8) == VP_EINVAL and r.vres_rc(a.off.bl[n - 1]) == VP_EINVAL, "vp_vres"
    assert r.phase1_rc(n - 1, a.off.bl[n - 1]) == VP_EINVAL and r.phase1_rc(1, 8) == VP_EINVAL, "vp_phase1_init"
    assert r.prove_rc(a.tape)[0] == VP_EINVAL and r.prove_rc(a.tape, 0)[0] == VP_EINVAL, "vp_prove_gkr"
    assert r.sizes_rc()[0] == VP_EINVAL and r.shard_chains_rc()[0] == VP_EINVAL
    pt, out = np.zeros((8, 2), np.uint64), np.zeros((1, 2), np.uint64)
    assert r.L.vp_layer_mle(r.c, 0, pt.ctypes.data, 8, out.ctypes.data) == VP_EINVAL, "vp_layer_mle"
    assert r.evaluate_rc(a.inputs) == VP_EINVAL
    assert r.launches() == before
    rc, root = r.commit_private_rc()
    assert rc == VP_OK and root == want["root_l"]
    _load_and_prove(r, a)


def test_r4_captured_graph_when_the_circuit_is_replaced(ctxs, ob):
    """A is proved twice (plan recorded, graph captured and replayed), then B with another plan shape, then A again: a graph or plan of the replaced circuit
    never runs on the new one."""
    a, b = _base(ob, "base"), _real(ob, "real9", 32, [40, 33, 50, 17, 29, 12, 21, 9, 6])
    r = ctxs()
    for c in (a, b, a):
        _load_and_prove(r, c)
        assert r.prove(c.tape) == c.gold
        t2 = gc.edge_limbs_complex(c.off, 7)
        assert r.prove(t2) == c.gold_on(t2)


def test_r5_commitment_when_the_circuit_is_replaced(ctxs, ob):
    """l, h and the FRI levels of A's witness are committed; B replaces A.  Nothing of A's commitment can be opened or continued, and B's root is its own."""
    a = _circ(ob, "pc_a", lambda: cc.make(41, [200, 120, 60]))
    b = _circ(ob, "pc_b", lambda: cc.make(42, [150, 90, 33]))
    n = 8
    r = ctxs()
    _load_and_prove(r, a)
    rc, root_a = r.commit_private_rc()
    assert rc == VP_OK, r.err()
    pt = pai.inputs("uniform", n)["r"]
    point = np.ascontiguousarray(np.vstack([pt, pt, pt, pt])[:n])
    assert r.commit_public_eq_rc(point)[0] == VP_OK, r.err()
    fr = np.ascontiguousarray(pt[:n - 6])
    roots = ctypes.create_string_buffer(32 * (n - 6))
    assert r.L.vp_fri_commit(r.c, fr.ctypes.data, n - 6, ctypes.cast(roots, ctypes.c_void_p)) == VP_OK, r.err()

    def commitment_is_gone():
        vals, path, k = np.zeros((130, 2), np.uint64), ctypes.create_string_buffer(32 * 40), ctypes.c_int(0)
        for oracle in (0, 1, 2):
            assert r.L.vp_fri_open(r.c, oracle, 0, vals.ctypes.data, ctypes.cast(path, ctypes.c_void_p), len(path), ctypes.byref(k)) == VP_EINVAL, "vp_fri_open(%d)" % oracle
        fin = np.zeros((2048, 2), np.uint64)
        assert r.L.vp_fri_final(r.c, fin.ctypes.data) == VP_EINVAL, "vp_fri_final"
        assert r.commit_public_eq_rc(point)[0] == VP_EINVAL, "vp_commit_public_eq before a private commit"
    r.upload(b.desc)
    commitment_is_gone()
    assert r.evaluate_rc(b.inputs) == VP_OK, r.err()
    commitment_is_gone()
    rc, root_b = r.commit_private_rc()
    assert rc == VP_OK, r.err()
    values = np.zeros((1 << n, 2), np.uint64)
    values[:len(b.inputs)] = b.inputs
    x = pai.inputs("uniform", n)
    want = pai.split_record(pai.oracle_record(ob.lib(), values, len(b.inputs), x["pub"], n, x["r"]), n)
    assert root_b == want["root_l"] and root_b != root_a
    assert r.prove(b.tape) == b.gold


def test_r6_index_split_in_effect_when_the_circuit_is_replaced(vp, ctxs, ob, monkeypatch):
    """vp_set_shard / vp_set_shard_split are the caller's settings and survive an upload ("What a circuit upload resets"); the split layout, the
    export area and the chain owners belong to the circuit and are laid out again.  The ranks are run in turn on one context, rank 1 of 2 last — the state A
    leaves behind — and B is then proved under the split, rank 1 first without any call between the upload and its proof."""
    monkeypatch.setenv("VP_SPLIT_COST_PERCENT", "0")
    a = _circ(ob, "split_a", lambda: cc.make(11, [1500, 2100, 900, 4100, 700]))
    b = _circ(ob, "split_b", lambda: cc.make(17, [2100, 1300, 3000]))
    r = ctxs()
    monkeypatch.delenv("VP_SPLIT_COST_PERCENT")
    L, W = r.L, 2

    def rank(k):
        assert L.vp_set_shard(r.c, k, W) == VP_OK and L.vp_set_shard_split(r.c, 9) == VP_OK, r.err()

    def finish(parts):
        summed = vp.sum_transcripts(parts)
        buf, n = ctypes.create_string_buffer(bytes(summed), len(summed)), ctypes.c_uint64(0)
        assert L.vp_shard_finish(r.c, buf, len(summed), ctypes.byref(n)) == VP_OK
        return buf.raw[:n.value]
    r.upload(a.desc)
    assert r.evaluate_rc(a.inputs) == VP_OK
    parts = []
    for k in range(W):
        rank(k)
        parts.append(r.prove(a.tape))
    assert (r.shard_chains_rc()[1] == -1).any(), "nothing of A was split"
    assert finish(parts) == a.gold
    r.upload(b.desc)
    assert r.evaluate_rc(b.inputs) == VP_OK
    rc, owner = r.shard_chains_rc()
    assert rc == VP_OK and len(owner) == 3 * (len(b.desc) - 1) + 1 and (owner == -1).any(), "the split did not survive the upload"
    _, _, nb = r.sizes_rc()
    assert nb > 16 * b.off.n_tr, "no export area behind B's transcript"
    part1 = r.prove(b.tape)                  # rank 1 of 2, as A left it
    rank(0)
    part0 = r.prove(b.tape)
    assert len(part0) == len(part1) == nb
    assert finish([part0, part1]) == b.gold
    assert L.vp_set_shard(r.c, 0, 1) == VP_OK
    assert r.prove(b.tape) == b.gold


# ---- more heavy rows than the first buffer of build_csr_dev holds ------------------------------------------------------------------------------------------
def _many_heavy_rows():
    """Layer 0: 8192 wires; layer 1: 4100 x 17 binary gates, gate k with u = v = k // 17 and l = 0, the seven binary types in turn; a small layer 2.  4100 rows
    of 17 contributions (> VP_LIGHT_MAX = 16) in the phase-1 list and 4100 slots of 17 in the phase-2 list: more than the 4096 heavy rows fetched at first."""
    rng = np.random.default_rng(77)
    n0, rows, per, n2 = 8192, 4100, 17, 6
    n1 = rows * per
    k = np.arange(n1)
    ty = np.concatenate([np.full(n0, cc.INPUT), np.array(cc.BINARY)[k % 7], [cc.ADD, cc.MUL, cc.XOR, cc.SUB, cc.COPY, cc.NOT]]).astype(np.int32)
    l = np.concatenate([np.full(n0, -1), np.zeros(n1), [1, 1, 0, 1, -1, -1]]).astype(np.int32)
    u = np.concatenate([rng.integers(0, cc.P, n0), k // per, rng.integers(0, n1, n2)]).astype(np.uint64)
    v = np.concatenate([np.zeros(n0), k // per, [5, 70000 % n1, 8191, 17, 0, 0]]).astype(np.uint64)
    return (np.array([n0, n1, n2], np.uint64), ty, l, u, v, np.zeros((n0 + n1 + n2, 2), np.uint64), np.zeros(n0 + n1 + n2, np.uint8))


def test_more_heavy_rows_than_the_first_fetch(vp, ctxs, ob):
    c = _circ(ob, "many_heavy", _many_heavy_rows)
    d1 = c.desc[1]
    assert d1["size"] == 4100 * 17 and int(d1["dad_size"][0]) == 4100
    assert np.bincount(d1["u"].astype(np.int64)).max() == 17 == np.bincount(d1["lv"].astype(np.int64)).min()
    r = ctxs()
    _load_and_prove(r, c)
    t2 = gc.edge_limbs_real(c.off, gc.SEED)
    assert r.prove(t2) == c.gold_on(t2)
    # the chunk kernels took all 4100 rows of each list: one chunk per row, four chunks per workgroup, `work` = contributions of the heavy rows
    r.L.vp_set_profiling(r.c, 1)
    assert r.prove(c.tape) == c.gold
    n = ctypes.c_int(0)
    r.L.vp_get_launch_stats(r.c, None, 0, ctypes.byref(n))
    arr = (vp.LaunchStat * max(1, n.value))()
    r.L.vp_get_launch_stats(r.c, arr, n.value, ctypes.byref(n))
    r.L.vp_set_profiling(r.c, 0)
    chunks = [(e.workgroups, e.jobs, e.work) for e in arr[:n.value] if r.L.vp_kernel_name(e.kind).decode() == _kind(vp, "CHUNKS")]
    print("chunk launches (workgroups, jobs, work):", chunks)
    assert chunks, "no chunk launch"
    assert sum(w for _, _, w in chunks) >= 2 * 4100 * 17 and sum(g for g, _, _ in chunks) >= 2 * ((4100 + 3) // 4)
