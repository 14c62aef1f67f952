"""GPU (-m gpu): the verifier's O(|C|) loops on the device — vp_predicates (k_pred_chunks + k_pred_combine over the bucket lists built at upload), vp_liu_gr and
vp_layer_mle (k_beta_half_direct + k_dot_multi + k_dotfin_multi) — compared VALUE BY VALUE with tests/verifier_sums.py (Python integers) and with the oracle's
own loops (orc_predicates / orc_liu_gr / orc_layer_mle), through the C ABI on Session.gpu_ctx().  Circuits and points: tests/verifier_sums_cases.py, the list
tests/test_verifier_sums_host.py has already checked the two references on.  Exact field elements: every comparison is word for word.

Under vp_set_profiling(1) the three entry points bracket their launches, and the tests assert the launch table: vp_layer_mle / vp_liu_gr list exactly
k_beta_half_direct, k_dot_multi (one workgroup per 256 entries, 128 at the most) and one k_dotfin_multi workgroup; vp_predicates lists its half-table launch
(k_pred_chunks / k_pred_combine have no kind in the table)."""
import ctypes

import numpy as np
import pytest

import custom_circuits as cc
import verifier_sums as vs
import verifier_sums_cases as cases
from test_gpu_parity import _both_modes, _drive_phase1

pytestmark = pytest.mark.gpu
P = cc.P
VP_OK, VP_EINVAL = 0, -1
VOIDP, INT = ctypes.c_void_p, ctypes.c_int


def _lib(vp):
    lib = vp.lib_gpu()
    lib.vp_predicates.argtypes = [VOIDP, INT, VOIDP, VOIDP, VOIDP, VOIDP, INT, VOIDP, ctypes.c_uint64]
    lib.vp_liu_gr.argtypes = [VOIDP, INT, VOIDP, VOIDP, VOIDP, VOIDP, VOIDP]
    lib.vp_layer_mle.argtypes = [VOIDP, INT, VOIDP, INT, VOIDP]
    lib.vp_vres.argtypes = [VOIDP, VOIDP, INT, VOIDP]
    lib.vp_last_error.restype = ctypes.c_char_p
    lib.vp_last_error.argtypes = [VOIDP]
    return lib


def _arr(pts):
    return np.ascontiguousarray(np.array([[int(a), int(b)] for a, b in pts], dtype=np.uint64).reshape(-1, 2))


def _ptr(a):
    return a.ctypes.data if len(a) else None            # a zero-variable layer has no challenges: NULL


def _pairs(a):
    return [(int(x), int(y)) for x, y in a]


def dev_predicates(lib, h, layer, rg, ar, ru, rv, n_v=None):
    g, a, u, v = _arr(rg), _arr([ar]), _arr(ru), _arr(rv)
    out = np.full((5 + 7 * layer, 2), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    rc = lib.vp_predicates(h, layer, _ptr(g), a.ctypes.data, _ptr(u), _ptr(v), len(v) if n_v is None else n_v, out.ctypes.data, len(out))
    return rc, _pairs(out)


def dev_liu_gr(lib, h, n_layers, layer, ru, rv, sig, rl):
    keep = [_arr(rv[j]) if (j >= layer and rv[j]) else None for j in range(n_layers)]
    ptrs = (VOIDP * n_layers)(*[k.ctypes.data if k is not None else None for k in keep])
    u, s, l = _arr(ru), _arr(sig), _arr(rl)
    out = np.full((1, 2), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    rc = lib.vp_liu_gr(h, layer, _ptr(u), ctypes.cast(ptrs, VOIDP), s.ctypes.data, _ptr(l), out.ctypes.data)
    return rc, _pairs(out)[0]


def dev_layer_mle(lib, h, layer, r):
    rr = _arr(r)
    out = np.full((1, 2), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    rc = lib.vp_layer_mle(h, layer, _ptr(rr), len(rr), out.ctypes.data)
    return rc, _pairs(out)[0]


def dev_vres(lib, h, r):
    rr = _arr(r)
    out = np.full((1, 2), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    rc = lib.vp_vres(h, _ptr(rr), len(rr), out.ctypes.data)
    return rc, _pairs(out)[0]


def _profiled(s, call):
    """call() with launch profiling on: (its result, [(kernel, workgroups)] of the launch table it leaves)."""
    s.set_profiling(1)
    try:
        res = call()
        table = [(e["kernel"], e["workgroups"]) for e in s.launch_stats()]
    finally:
        s.set_profiling(0)
    return res, table


def _circuit(vp, name):
    """The device circuit, tied to the oracle's subset numbering by its hash."""
    c = vp.Circuit.randomize(*cases.DEEP[:2], seed=cases.DEEP[2]) if name == "deep" else vp.Circuit.custom(*cases.arrays(name))
    assert c.hash() == cases.oracle_circuit(name).hash(), "loader mismatch: the export's numbering is not the device circuit's"
    return c


@pytest.fixture(scope="module")
def sessions(vp):
    """One session per circuit, created on first use and shared by the tests that only read from it."""
    made = {}

    def get(name):
        if name not in made:
            c = _circuit(vp, name)
            made[name] = (c, vp.Session(c))
        return made[name][1]
    yield get
    for c, s in made.values():
        s.close(); c.close()


def _check_predicates(lib, h, name, layer, only=None):
    oc, w = cases.oracle_circuit(name), cases.wiring(name)
    empty = [k for k in range(5 + 7 * layer) if k not in cases.filled_slots(w, layer)]
    for (label, rg, ar, ru, rv), ref in zip(cases.predicate_points(name, layer), cases.predicate_reference(name, layer)):
        if only is not None and label not in only:
            continue
        rc, got = dev_predicates(lib, h, layer, rg, ar, ru, rv)
        assert rc == VP_OK, (label, lib.vp_last_error(h))
        assert got == ref, "%s layer %d, %s: differs from the Python reference at %r" % (name, layer, label, [k for k in range(len(ref)) if got[k] != ref[k]][:8])
        assert got == oc.predicates(layer, rg, ar, ru, rv), label
        assert all(got[k] == (0, 0) for k in empty), label


@pytest.mark.parametrize("name,layer", cases.PREDICATE_LAYERS)
def test_predicates_by_value(vp, sessions, name, layer):
    """Every gate layer of the ladder circuit (buckets of 0, 1, 63, 64, 65, 511, 512, 513, 1024, 1025 and 33000 gates, scattered), the unary-only layer with
    n_v = 0, the zero-variable layers with NULL r_g / r_u, and the 446-bucket top layer of a 64-layer circuit; uniform, corner and edge-limb points,
    assert_random 0 / 1 / p - 1.  A bucket the circuit leaves empty is exactly (0, 0)."""
    lib, s = _lib(vp), sessions(name)
    w = cases.wiring(name)
    if (name, layer) == ("unary_mid", cc.UNARY_MID_LAYER):
        assert w.n_v(layer) == 0 and w.max_dad_bl[layer] == -1
    if name == "zero_var" and layer == 2:
        assert w.bl[layer] == 0 and w.bl[layer - 1] == 0
    if name == "deep" and layer == 63:
        assert 5 + 7 * layer == 446
    _check_predicates(lib, s.gpu_ctx(), name, layer)
    # the half tables of r_g, r_u and r_v in one launch: three jobs of as many workgroups as the longest pair of halves needs
    _, rg, ar, ru, rv = cases.predicate_points(name, layer)[0]
    (rc, got), table = _profiled(s, lambda: dev_predicates(lib, s.gpu_ctx(), layer, rg, ar, ru, rv))
    assert rc == VP_OK and got == cases.predicate_reference(name, layer)[0]
    assert table == [("k_beta_half_direct", 3 * max(cases.dot_launches(1, n)[0][1] for n in (len(rg), len(ru), len(rv))))]


def test_predicates_smallest_layer_first_then_largest(vp):
    """The scratch (piece sums, bucket sums) is allocated by the first call: the smallest layer first, then the largest, then the smallest again, on a fresh context."""
    lib = _lib(vp)
    c = _circuit(vp, "ladder")
    s = vp.Session(c)
    pick = ("uniform0", "edge0", "all p-1")
    for layer in (5, cc.LADDER_LAYER, 5, 1):
        _check_predicates(lib, s.gpu_ctx(), "ladder", layer, only=pick)
    s.close(); c.close()


@pytest.mark.parametrize("name,layer", cases.MLE_LAYERS)
def test_layer_mle_by_value(vp, sessions, name, layer):
    """<eq(r, .), values> at bit lengths 17 (real inputs), 17, 16, 15, 7, 2, 1, 0 (complex values): the small-table branch, the whole-runs branch with a partial last
    run, more than 128 x 256 entries.  On a top layer vp_vres at the same point is the same element."""
    lib, s = _lib(vp), sessions(name)
    oc, w = cases.oracle_circuit(name), cases.wiring(name)
    h = s.gpu_ctx()
    if name == "dot":
        assert cases.dot_launches(w.size[layer], w.bl[layer])[1] == ("k_dot_multi", 128 if layer <= 3 else 1)
    if layer in (0, 1, 2, 3, 4):
        assert np.array_equal(s.layer_values(layer), np.array(cases.values(name)[layer], dtype=np.uint64)), "evaluate differs: the inner product has other inputs"
    for (label, r), ref in zip(cases.mle_points(name, layer), cases.mle_reference(name, layer)):
        (rc, got), table = _profiled(s, lambda: dev_layer_mle(lib, h, layer, r))
        assert rc == VP_OK, (label, lib.vp_last_error(h))
        assert got == ref, "%s layer %d (n = %d), %s" % (name, layer, w.bl[layer], label)
        assert table == cases.dot_launches(w.size[layer], w.bl[layer]), label
        assert got == oc.layer_mle(layer, r), label
        if layer == w.n - 1:
            rc, top = dev_vres(lib, h, r)
            assert rc == VP_OK and top == ref, "vp_vres, " + label


def _check_liu(lib, h, name, layer, session=None):
    """session: run profiled and assert the launch table of the inner product over the Liu table of layer - 1."""
    oc, w = cases.oracle_circuit(name), cases.wiring(name)
    for (label, ru, rv, sig, rl), ref in zip(cases.liu_points(name, layer), cases.liu_reference(name, layer)):
        if session is not None:
            (rc, got), table = _profiled(session, lambda: dev_liu_gr(lib, h, w.n, layer, ru, rv, sig, rl))
            assert table == cases.dot_launches(w.size[layer - 1], w.bl[layer - 1]), label
        else:
            rc, got = dev_liu_gr(lib, h, w.n, layer, ru, rv, sig, rl)
        assert rc == VP_OK, (label, lib.vp_last_error(h))
        assert got == ref, "%s layer %d, %s" % (name, layer, label)
        assert got == oc.liu_gr(layer, ru, [x or [] for x in rv], sig, rl), label


@pytest.mark.parametrize("fast_init", [1, 0])
@pytest.mark.parametrize("name,layer", cases.LIU_LAYERS)
def test_liu_gr_by_value(vp, monkeypatch, name, layer, fast_init):
    """layer = 1 (every later layer contributes), the top layer (one), layers whose later layers include an empty subset (unary_mid 1 and 2); the table built by
    the batched path's init kernels (default) and by the per-sumcheck ones (VP_FAST_INIT=0)."""
    w = cases.wiring(name)
    if name == "unary_mid" and layer in (1, 2):
        assert any(w.dad_size[j][layer - 1] == 0 for j in range(layer, w.n))
    if not fast_init:
        monkeypatch.setenv("VP_FAST_INIT", "0")
    lib = _lib(vp)
    c = _circuit(vp, name)
    s = vp.Session(c)
    assert s.options_in_effect().interactive_fast_init == fast_init
    _check_liu(lib, s.gpu_ctx(), name, layer, session=s)
    s.close(); c.close()


@pytest.mark.parametrize("name,layer", [("ladder", 1), ("ladder", 5), ("unary_mid", 2)])
def test_liu_gr_on_a_round_sharded_session(vp, name, layer):
    """vp_liu_gr builds the WHOLE table on a round-sharded context: rank 0 returns the element of the unsharded context (= the references)."""
    lib = _lib(vp)
    c = _circuit(vp, name)
    s = vp.Session(c, devices=[0, 0], round_shard_min_log=2)
    assert s.world() == 2
    _check_liu(lib, s.gpu_ctx(), name, layer, session=s)
    s.close(); c.close()


@pytest.mark.parametrize("name", ["unary_mid", "ladder"])
def test_call_order_and_state(vp, name):
    """The shared scratch is allocated by whichever helper runs first: vp_layer_mle then vp_predicates on one fresh session (nothing else has run on it),
    the reverse on another — the same values.  After all three helpers have run, prove_gkr() and prove_interactive() on that session return the bytes a
    session of its own returned before."""
    lib = _lib(vp)
    w = cases.wiring(name)
    top = w.n - 1
    gold, st = cases.oracle_circuit(name).prove_gkr()
    assert st["verified"] == 1
    c = _circuit(vp, name)
    s = vp.Session(c)
    s.draw_tape()
    before_b, _ = s.prove_gkr()
    before_i, _, ok = s.prove_interactive()
    assert ok and before_b == gold and before_i == gold
    s.close()
    pick = ("uniform0", "edge1")
    for order in ("mle first", "predicates first"):
        s = vp.Session(c)
        h = s.gpu_ctx()

        def mle():
            for (label, r), ref in zip(cases.mle_points(name, top), cases.mle_reference(name, top)):
                assert dev_layer_mle(lib, h, top, r) == (VP_OK, ref), (order, label)

        def predicates():
            _check_predicates(lib, h, name, top, only=pick)
        steps = [mle, predicates]
        if order == "predicates first":
            steps.reverse()
        for step in steps:
            step()
        _check_liu(lib, h, name, 1)
        _check_predicates(lib, h, name, 1, only=pick)
        s.draw_tape()
        after_b, _ = s.prove_gkr()
        after_i, _, ok = s.prove_interactive()
        assert ok and after_b == before_b and after_i == before_i, order
        s.close()
    c.close()


def test_unary_only_circuit_end_to_end(vp):
    """A layer without binary gates (maxDadBitLength -1, no phase 2) through the prover and both verifiers: the oracle's transcript in both modes; the host
    verifier accepts with its own predicate loops and with the device's (predicatesOnDevice(layer, false): vp_predicates with n_v = 0), and both reject a
    flipped last claim."""
    c = _circuit(vp, "unary_mid")
    gold, st = cases.oracle_circuit("unary_mid").prove_gkr()
    assert st["verified"] == 1
    _both_modes(vp, c, gold)
    s = vp.Session(c)
    s.draw_tape()
    tr, _ = s.prove_gkr()
    assert tr == gold
    assert s.check(tr)[0] and s.check(tr, device_predicates=True)[0]
    bad = bytearray(tr); bad[-16] ^= 1
    assert not s.check(bytes(bad))[0] and not s.check(bytes(bad), device_predicates=True)[0]
    s.close(); c.close()


def test_predicates_refuse_another_n_v(vp, sessions):
    """n_v must be max(0, maxDadBitLength(layer)): too small, too large and 0 on a layer with binary gates are VP_EINVAL before anything is launched (a shorter
    beta_v table would be indexed past what the call wrote); 1 on the unary-only layer too.  The context answers correctly afterwards."""
    lib, s = _lib(vp), sessions("ladder")
    h, layer = s.gpu_ctx(), cc.LADDER_LAYER
    w = cases.wiring("ladder")
    _, rg, ar, ru, rv = cases.predicate_points("ladder", layer)[0]
    long_rv = rv + cases.uniform(np.random.default_rng(1), 31 - len(rv))
    assert w.n_v(layer) == 10
    for n_v in (9, 11, 0, 31, 1):
        rc, out = dev_predicates(lib, h, layer, rg, ar, ru, long_rv, n_v=n_v)
        assert rc == VP_EINVAL and b"n_v" in lib.vp_last_error(h), n_v
        assert all(x == (0x5a5a5a5a5a5a5a5a,) * 2 for x in out), "a refused call wrote to out"
    _check_predicates(lib, h, "ladder", layer, only=("uniform0",))
    su = sessions("unary_mid")
    _, rg, ar, ru, _ = cases.predicate_points("unary_mid", cc.UNARY_MID_LAYER)[0]
    rc, _ = dev_predicates(lib, su.gpu_ctx(), cc.UNARY_MID_LAYER, rg, ar, ru, long_rv, n_v=1)
    assert rc == VP_EINVAL
    _check_predicates(lib, su.gpu_ctx(), "unary_mid", cc.UNARY_MID_LAYER, only=("uniform0",))


def test_non_canonical_challenges_are_refused_on_the_host_side(vp, sessions):
    """A limb >= p in any challenge is VP_EINVAL in all three entry points, as in vp_round: refused before anything is queued, the output untouched, the context
    as good as before."""
    lib, s = _lib(vp), sessions("unary_mid")
    h, layer = s.gpu_ctx(), 3
    w = cases.wiring("unary_mid")
    untouched = (0x5a5a5a5a5a5a5a5a,) * 2
    _, rg, ar, ru, rv = cases.predicate_points("unary_mid", layer)[0]
    for bad in ((P, 0), (0, P), (1 << 61, 5), (7, (1 << 64) - 1)):
        for k in range(4):
            a = [list(rg), ar, list(ru), list(rv)]
            if k == 1:
                a[1] = bad
            else:
                a[k][-1] = bad
            rc, out = dev_predicates(lib, h, layer, *a)
            assert rc == VP_EINVAL and b"canonical" in lib.vp_last_error(h) and out[0] == untouched, (bad, k)
        _, r = cases.mle_points("unary_mid", layer)[0]
        rc, out = dev_layer_mle(lib, h, layer, [bad] + list(r[1:]))
        assert rc == VP_EINVAL and out == untouched
        _, lu, lv, sig, rl = cases.liu_points("unary_mid", layer)[0]
        for k in range(4):
            a = [list(lu), [list(x) if x else x for x in lv], list(sig), list(rl)]
            if k == 1:
                a[1][layer][0] = bad
            else:
                a[k][0] = bad
            rc, out = dev_liu_gr(lib, h, w.n, layer, *a)
            assert rc == VP_EINVAL and b"canonical" in lib.vp_last_error(h) and out == untouched, (bad, k)
    _check_predicates(lib, h, "unary_mid", layer, only=("uniform0",))
    _check_liu(lib, h, "unary_mid", layer)


def test_liu_gr_checks_its_arguments_before_it_touches_the_context(vp):
    """vp_liu_gr with a missing r_liu, a missing r_v of a later layer, or a layer out of range is refused BEFORE vp_liu_init replaces the sumcheck in progress:
    a phase-1 sumcheck interrupted by such calls continues and gives the messages of an undisturbed run."""
    lib = _lib(vp)
    c = _circuit(vp, "unary_mid")
    s = vp.Session(c)
    h = s.gpu_ctx()
    w = cases.wiring("unary_mid")
    undisturbed = _drive_phase1(vp, h, c)
    _, ru, rv, sig, rl = cases.liu_points("unary_mid", 3)[0]

    def refused_calls():
        assert dev_liu_gr(lib, h, w.n, 3, ru, rv, sig, [])[0] == VP_EINVAL                     # r_liu missing
        assert dev_liu_gr(lib, h, w.n, 3, ru, [None] * w.n, sig, rl)[0] == VP_EINVAL           # r_v of a layer with a subset missing
        assert dev_liu_gr(lib, h, w.n, 0, ru, rv, sig, rl)[0] == VP_EINVAL                     # layer bounds
        assert dev_liu_gr(lib, h, w.n, w.n, ru, rv, sig, rl)[0] == VP_EINVAL
    assert _drive_phase1(vp, h, c, disturb_at=2, disturb=refused_calls) == undisturbed
    _check_liu(lib, h, "unary_mid", 3)
    s.close(); c.close()
