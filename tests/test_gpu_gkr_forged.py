"""GPU (-m gpu): the forged GKR transcripts of tests/gkr_forged_cases.py through the verifier's device loops (vp_predicates, vp_liu_gr, vp_layer_mle behind
Session.check(device_predicates=True) and Circuit.verify_full_record(device=k)).  There the device's values decide a rejection, and until now they had only ever
rejected a flipped last claim.  Every expectation here is one tests/test_gkr_forged_host.py has checked without a device: the forger's declared check, the verdict of
the verifier written from the protocol (tests/gkr_verifier_ref.py) and the host loops' verdict agree on the same rows.

  table    every row on S, unary_mid, zero_var (all families), M (layers of 700 to 4100 gates: the chunked predicate kernels decide) and R (randomize(4, 12)):
           verdict and named check of the device loops equal the host loops' and the declared one; the profiled launch tables show one vp_predicates call per closing
           value reached, one vp_liu_gr call per Liu closing test reached and vp_layer_mle exactly where the input check is reached
  record   the GKR section of a live version-1 and a live version-2 (masked) record re-made to the end on the record's own challenges: rejected at claim != input_0
           with the loops on the host and on the device
  joined   the two forgeries of a joined proof from Session.prove_full_fs(device_gkr=True) through verify_full_fs(proof, device=0)
  honest   one honest run of each route, accepted with no failure recorded"""
import contextlib
import os

import pytest

import full_fs_ref as ff
import gkr_fs_cases as gfc
import gkr_forged_cases as fc
import gkr_tape_cases as gc
import gkr_verifier_ref as gv
import pc_masked_inputs as pmi
import verifier_sums as vs

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _session(vp, c, env, **kw):
    """A session created under `env` (the library reads the switches when the context is created)."""
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


def _device_calls(s):
    """(vp_predicates, vp_liu_gr + vp_layer_mle) calls of the last check, from the profiled launch tables: vp_predicates lists its half-table launch alone, the two
    inner products list k_beta_half_direct, k_dot_multi, k_dotfin_multi"""
    names = [e["kernel"] for e in s.verifier_launch_stats()]
    dots = names.count("k_dotfin_multi")
    assert names.count("k_dot_multi") == dots and set(names) <= {"k_beta_half_direct", "k_dot_multi", "k_dotfin_multi"}, names
    return names.count("k_beta_half_direct") - dots, dots


@pytest.mark.parametrize("name", list(fc.GPU_TABLE))
def test_forged_table_through_the_device_loops(vp, name):
    c, off = gc.build(vp, name), gc.offsets(name)
    assert c.hash() == gc.oracle_circuit(name).hash()
    kinds = set()
    try:
        with _session(vp, c, gc.env(name)) as s:
            s.set_profiling(1)
            for fam in fc.GPU_TABLE[name]:
                tape, tr = gc.tape(name, fam), gc.oracle(name, fam)[0]
                s.set_tape(tape)
                assert s.prove_gkr()[0] == tr, fam
                assert s.check(tr)[0] and vp.last_gkr_failure() is None, fam
                assert s.check(tr, device_predicates=True)[0] and vp.last_gkr_failure() is None, fam
                assert _device_calls(s) == (off.n_layers - 1, off.n_layers), fam
                for label, plan, bad, declared in fc.rows(name, fam):
                    what = "%s / %s / %s" % (name, fam, label)
                    assert bad is not None, what
                    assert s.check(bad)[0] == (declared is None) and vp.last_gkr_failure() == declared, what + ": the host loops"
                    assert s.check(bad, device_predicates=True)[0] == (declared is None), what + ": the device loops' verdict"
                    assert vp.last_gkr_failure() == declared, what + ": the check named with the device loops"
                    n_pred, n_liu, n_input = fc.reached(off, declared)
                    assert _device_calls(s) == (n_pred, n_liu + n_input), what + ": device calls"
                    if declared is not None:
                        kinds.add(declared[0])
                assert s.check(tr, device_predicates=True)[0] and vp.last_gkr_failure() is None, fam
            s.set_profiling(0)
    finally:
        c.close()
    # the device's values decided rejections of every kind that reads one: closing values, Liu closing tests, the input
    assert {"semi_final", "liu_semi_final", "input"} <= kinds and kinds <= set(gv.KINDS)


@pytest.fixture(scope="module")
def live(vp, golden):
    import custom_circuits as cc
    g = golden["custom_a"]
    args = cc.make(g["custom"]["seed"], g["custom"]["sizes"])
    c = vp.Circuit.custom(*args)
    n = c.layer_bitlen(0)
    f = pmi.family("short_pub", n, 1 << (n - 6))
    s = vp.Session(c)
    runs = {}
    try:
        for what, kw in (("version 1", {}), ("version 2", {"mask": f["pri_mask"], "pub_mask": f["pub_mask"]})):
            _, ok, _ = s.prove_and_verify_full(reps=3, **kw)
            assert ok
            runs[what] = (s.last_full_record(), f["pub_mask"].shape[0] if kw else None)
    finally:
        s.close()
    yield c, args, runs
    c.close()


@pytest.mark.parametrize("what", ["version 1", "version 2"])
def test_forged_records_of_a_live_pass(vp, live, what):
    c, args, runs = live
    rec, n_pub = runs[what]
    bad, old, new = fc.record_forgery(args, rec, n_pub)
    assert old != new and len(bad) == len(rec)
    for dev in (None, 0):
        assert c.verify_full_record(rec, device=dev) and vp.last_gkr_failure() is None, (what, dev)
        assert not c.verify_full_record(bad, device=dev), (what, dev)
        assert vp.last_gkr_failure() == ("input", 0, -1), "%s, device %r: not rejected at claim != input_0" % (what, dev)
        assert c.verify_full_record(rec, device=dev) and vp.last_gkr_failure() is None, (what, dev)


def test_forged_joined_proofs(vp, ob):
    _, layers, log_size, seed, reps = ff.FIXTURE
    c = vp.Circuit.randomize(layers, log_size, seed=seed)
    oc = ob.Circuit.randomize(layers, log_size, seed=seed)
    try:
        with _session(vp, c, {}, device=0) as s:
            proof = s.prove_full_fs(reps=reps, device_gkr=True)
        w, off, sec = vs.wiring_from(oc), gc.Offsets.of(oc), ff.sections(proof)
        state, gkr = gfc.full_fs_head_state(oc, proof)
        (remade, d0, tape0), (true_vr, d1, _) = fc.joined_forgeries(w, off, state, gkr)
        for dev in (None, 0):
            ok, why, point = c.verify_full_fs(proof, device=dev, return_point=True)
            assert ok and vp.last_gkr_failure() is None, dev
            ok, why, moved = c.verify_full_fs(proof[:sec["gkr"]] + remade + proof[sec["root_h"]:], device=dev, return_point=True)
            assert not ok and "final input check" in why and vp.last_gkr_failure() == d0, (dev, why)
            at = off.rl[1][0]
            assert moved.tobytes() == tape0[at:at + off.bl[0]].tobytes() != point.tobytes(), dev
            ok, why = c.verify_full_fs(proof[:sec["gkr"]] + true_vr + proof[sec["root_h"]:], device=dev)
            assert not ok and "GKR" in why and vp.last_gkr_failure() == d1, (dev, why)
    finally:
        c.close()
