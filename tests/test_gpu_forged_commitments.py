"""GPU (-m gpu): the device loops of the commitment's verifier held to their part in a REJECTION.  vp_pc_public_evals (k_pc_poly_eval), vp_pc_mask_evals
(k_pc_mask_eval_fin) and vp_fri_query_digests (k_pc_opening_digests) are compared value by value on honest inputs elsewhere; here their values feed the checks of
forged proofs that pass every Merkle check (tests/pc_forge.py), and the verdict and the name of the failed check must be the host loops' and the definition's.

  commitment level   the table of tests/pc_forged_cases.py (n = 9 and 10, the zero mask and a uniform one, pub= and point=) through Circuit.verify_commitment with
                     device=0, with the host loops, and through tests/pc_verifier_ref.py: one verdict, one name.  A changed last element of slice 63 of pub moves
                     the device's q value of that slice alone; a re-committed leaf produces the new root on the device.
  protocol level     one live pass on custom_a (n = 10), unmasked and masked: the record-level forgeries of pc_forge.record_cases on the version-1 and the
                     version-2 record, replayed on the host and with device=0 — controls accepted, forgeries rejected; the session hands out the verifier's own
                     draws (last_fri, last_point), so the same opened values also go through the commitment-level verifier in its three forms, by name."""
import numpy as np
import pytest

import pc_forge as forge
import pc_forged_cases as fc
import pc_masked_inputs as pmi
import pc_verifier_ref as vref
import test_gpu_pc_verifier_loops as loops
import test_gpu_query_phase as qp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", fc.FAMILIES)
@pytest.mark.parametrize("n,kind", fc.PROOFS + [(9, "point"), (10, "point")])
def test_device_loops_give_the_verdict_and_the_name(vp, ob, n, kind, family):
    p = fc.proof(ob, n, kind)
    assert fc.host_verify(vp, p, device=0) == (True, "")
    if kind == "point":
        assert fc.host_verify(vp, p, device=0, point=p["point"]) == (True, "")
    cs = [c for c in fc.cases(p) if c["family"] == family]
    assert cs
    controls = 0
    for c in cs:
        q, kw = c["q"], c["kw"]
        ok, name, _, _ = fc.ref_verify(q, **kw)
        assert (ok, name) == ((True, "") if c["must"] is None else (False, c["must"])), c["id"]
        assert fc.host_verify(vp, q, **kw) == (ok, name), "host loops: " + c["id"]
        assert fc.host_verify(vp, q, device=0, **kw) == (ok, name), "device loops: " + c["id"]
        cq, ckw = c["control"]
        if cq is not p and controls < 4:             # (every control is the honest proof byte for byte — tests/test_pc_forged_host.py; a few through the device)
            assert fc.host_verify(vp, cq, device=0, **ckw) == (True, "")
            controls += 1


@pytest.fixture(scope="module")
def bare(vp):
    ctx = qp._ctx(vp)
    yield ctx
    vp.lib_gpu().vp_destroy(ctx)


@pytest.mark.parametrize("n", [9, 10])
def test_a_changed_public_element_moves_the_devices_q_of_its_slice(vp, ob, bare, n):
    p = fc.proof(ob, n, "zero")
    lf = p["leaf0"]
    rc, q0 = loops._evals(vp, bare, n, lf, pub=np.ascontiguousarray(p["pub"]))
    assert rc == 0
    pub = fc._moved(p["pub"], (1 << n) - 1)          # the last element of slice 63
    rc, q1 = loops._evals(vp, bare, n, lf, pub=pub)
    assert rc == 0
    want = vref.ref.public_evals(n, [(int(a), int(b)) for a, b in pub], lf[:2] + lf[-1:])
    for i, q in enumerate([0, 1, len(lf) - 1]):
        for h in range(2):
            assert [tuple(int(v) for v in e) for e in q1[q, h]] == want[i][h]
    off = [i for i, s0 in enumerate(lf) if s0 % 32]  # (where x0 is itself an N-th root of unity, q(x0) is one element of the slice)
    assert (q1[:, :, :63] == q0[:, :, :63]).all() and (q1[off, :, 63] != q0[off, :, 63]).any(axis=-1).all()
    pt = fc.proof(ob, n, "point")
    rc, a = loops._evals(vp, bare, n, lf, point=np.ascontiguousarray(pt["point"]))
    rc2, b = loops._evals(vp, bare, n, lf, point=fc._moved(pt["point"], n - 1))
    assert rc == 0 and rc2 == 0 and (a != b).any(axis=-1).all()


@pytest.mark.parametrize("n", [9, 10])
def test_a_recommitted_leaf_gives_the_new_root_on_the_device(vp, ob, bare, n):
    p = fc.proof(ob, n, "uniform")
    per = n - 4                                      # openings of a repetition
    for oracle in range(per):
        rep = fc.MID
        _, leaf, _ = forge.opened(p, rep)[oracle]
        q = forge.forge(p, [(oracle, leaf, 2 * 31, forge.f_add(p["vals"][oracle][leaf, 62], fc.D))])
        roots = [q["root_l"], q["root_h"]] + [q["fri_roots"][32 * k:32 * k + 32] for k in range(n - 6)]
        old = [p["root_l"], p["root_h"]] + [p["fri_roots"][32 * k:32 * k + 32] for k in range(n - 6)]
        assert roots[oracle] != old[oracle] and [r for i, r in enumerate(roots) if i != oracle] == [r for i, r in enumerate(old) if i != oracle]
        rc, dg = loops._digests(vp, bare, n, q["leaf0"], q["answer"])
        assert rc == 0 and dg == vp.Circuit.pc_opening_digests_host(n, q["leaf0"], q["answer"])
        for r in range(len(q["leaf0"])):
            for o in range(per):
                at = 64 * (r * per + o)
                assert dg[at + 32:at + 64] == roots[o], (r, o)
        at = 64 * (rep * per + oracle)
        assert dg[at:at + 32] == q["levels"][oracle][0][leaf] != p["levels"][oracle][0][leaf]


# ---- protocol level ---------------------------------------------------------------------------------------------------------------------------------------------
def _replay(c, rec, device, capfd):
    capfd.readouterr()
    ok = c.verify_full_record(rec, device=device)
    err = [ln for ln in capfd.readouterr().err.strip().splitlines() if ln.startswith(("Fri ", "commitment:"))]
    return ok, err[-1] if err else ""


@pytest.fixture(scope="module")
def live(vp, golden):
    import custom_circuits as cc
    g = golden["custom_a"]
    c = vp.Circuit.custom(*cc.make(g["custom"]["seed"], g["custom"]["sizes"]))
    n = c.layer_bitlen(0)
    f = pmi.family("short_pub", n, 1 << (n - 6))
    s = vp.Session(c)
    runs = {}
    try:
        for what, kw in (("version 1", {}), ("version 2", {"mask": f["pri_mask"], "pub_mask": f["pub_mask"]})):
            _, ok, _ = s.prove_and_verify_full(reps=5, **kw)
            assert ok
            runs[what] = (s.last_full_record(), s.last_fri()[2], s.last_point()[:n], f["pub_mask"].shape[0] if kw else None)
    finally:
        s.close()
    yield c, runs
    c.close()


@pytest.mark.parametrize("what", ["version 1", "version 2"])
def test_forged_records_of_a_live_pass(vp, live, capfd, what):
    c, runs = live
    rec, r, point, n_pub = runs[what]
    sec = forge.sections(rec, n_pub)
    assert sec["n"] == 10 and sec["reps"] == 5
    honest = forge.commitment_of(rec, sec, r, point)
    assert (honest["ms"] > 1) == (what == "version 2") and honest["final_mask"].any() == (what == "version 2")
    assert fc.ref_verify(honest, point=honest["point"])[:2] == (True, "")
    for dev in (None, 0):
        assert _replay(c, rec, dev, capfd) == (True, "")
    cases = forge.record_cases(rec, sec, slices=(31,))
    assert len(cases) >= 2 + 6 * 2 * 2 - 2
    names, controls = set(), set()
    for id_, control, bad in cases:
        if control is not rec and control not in controls:
            controls.add(control)
            assert _replay(c, control, None, capfd) == (True, "") and _replay(c, control, 0, capfd) == (True, ""), "control of " + id_
        q = forge.commitment_of(bad, sec, r, point)
        ok, name, _, _ = fc.ref_verify(q, point=q["point"])
        assert not ok and name.startswith("Fri "), (id_, name)
        for dev in (None, 0):
            assert _replay(c, bad, dev, capfd) == (False, name), (id_, dev)
            assert fc.host_verify(vp, q, device=dev, point=q["point"]) == (False, name), (id_, dev)
        names.add(name)
    assert names == {vref.FINAL} | {vref.round_name(k) for k in range(4)}
