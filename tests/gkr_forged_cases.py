"""The table of forged GKR transcripts (tests/gkr_forge.py), each with the one check that must reject it, shared by tests/test_gkr_forged_host.py (CPU: the forger's
declared check against the definition, tests/gkr_verifier_ref.py, and against the host verifier's verdict and named check) and tests/test_gpu_gkr_forged.py (the
same rows through the verifier's device loops).  One list, so that the GPU file adds no expectation the CPU suite has not checked.  Everything is seeded, and every
row is built once per process and never modified.

Per (circuit, family) the plans depend on the circuit's shape alone (plans()): with top / middle / bottom the layers n - 1, n // 2 and 1,
  pair change      a + 1, b - 1 in the first, a middle and the last round of phase 1, phase 2 and Liu at each of the three layers, where the sumcheck has rounds;
  false Vres       rounds of the top layer re-made, honest claims; the same from a middle round of phase 1 of a lower layer ("claims");
  solved           claims solved at the top layer, honest below: the near claim and, where the top layer reads a far layer, a far one; the near one at the middle
                   layer, the lie carried down to it;
  liu_vr           Liu re-made with the honest vr, at the top and at the middle layer;
  vr_div           vr = S / gr, honest below, at the top and at the middle layer; at layer 1 it is the lie carried to the end, which only the input check sees;
  true_vr          the same with the last vr set to the input layer's true value.
FAMILIES are the tapes on which the forger carries a false Vres through every layer to the input on all five SMALL_CIRCUITS; DEAD_END is the tape on which it cannot
pass the first layer whose r_u and r_v are corners (the top layer; layer 1 on zero_var, whose layer 2 has no round): the closing value's slope in a claim is a sum
over the gates at one corner, and it is zero for every claim.
Fiat-Shamir form (rows_fs): the challenges are drawn from the chain as the forger goes and the bytes behind the repaired stretch are the honest proof's old ones;
joined_forgeries and record_forgery put a re-made GKR section into a joined proof and into a complete-protocol record."""
import functools

import gkr_forge as gf
import gkr_tape_cases as gc
import gkr_verifier_ref as gv
import verifier_sums as vs

FAMILIES = ("uniform", "sprinkle", "edge_limbs_complex", "stripes_0_m1", "stripes_1_m1", "stripes_2_m1", "stripes_0_m1m1", "stripes_1_m1m1", "stripes_2_m1m1",
            "minus_one_limbs", "sig_first_only", "assert_m1")
DEAD_END = "uv_corners"
FS_CIRCUITS = ("S", "unary_mid", "zero_var")
# the rows of tests/test_gpu_gkr_forged.py; M (layers of 700 to 4100 gates: the chunked predicate kernels) and R (randomize(4, 12)) on four tapes each
# (M / sprinkle is a dead end at layer 2: a sprinkled 1 among the upper coordinates of r_v takes every smaller subset's claim out of the closing value)
GPU_TABLE = {"S": FAMILIES, "unary_mid": FAMILIES, "zero_var": FAMILIES, "M": ("uniform", "edge_limbs_complex", "stripes_1_m1m1", "minus_one_limbs"),
             "R": ("uniform", "sprinkle", "edge_limbs_complex", "sig_first_only")}
SEED = 20611


@functools.lru_cache(maxsize=None)
def wiring(name):
    return vs.wiring_from(gc.oracle_circuit(name), gc.arrays(name))


@functools.lru_cache(maxsize=None)
def honest(name, family):
    return tuple(gv.elements(gc.oracle(name, family)[0]))


def three(k):
    """first, middle and last of k rounds"""
    return sorted({0, k // 2, k - 1}) if k > 0 else []


def layers_of(off):
    n = off.n_layers
    return sorted({n - 1, n // 2, 1}, reverse=True)


def plans(name, fs=False):
    """[(label, plan)] for the circuit: see the module's text.  fs: the rows of the Fiat-Shamir form."""
    off, w = gc.offsets(name), wiring(name)
    n = off.n_layers
    top, mid = n - 1, n // 2
    out = []
    for i in layers_of(off):
        for kind, k in (("phase1", off.bl[i - 1]), ("phase2", max(0, off.mdb[i])), ("liu", off.bl[i - 1])):
            for j in three(k):
                out.append(("pair change, %s, layer %d, round %d" % (kind, i, j), {"pair": (kind, i, j)}))
    if fs:
        out = [out[0], out[len(out) // 2], out[-1]]
    vres = lambda stop, **kw: dict({"lie": "vres", "stop": stop}, **kw)
    if not fs:
        out.append(("false Vres, honest claims", vres((top, "claims"))))
        lower = [i for i in range(top - 1, 0, -1) if off.bl[i - 1] > 0]
        m = mid if mid in lower else lower[0]
        out.append(("a lie from round %d of layer %d, honest claims" % (off.bl[m - 1] // 2, m), {"lie": (m, off.bl[m - 1] // 2), "stop": (m, "claims")}))
    out.append(("near claim solved at the top layer", vres((top, "solved"), k="near")))
    if off.mdb[top] != -1 and gf.subsets(w, top, "far"):
        out.append(("far claim solved at the top layer", vres((top, "solved"), k="far")))
    if not fs:
        if mid != top:
            out.append(("near claim solved at layer %d" % mid, vres((mid, "solved"), k="near")))
        for i in sorted({top, mid}, reverse=True):
            out.append(("Liu re-made at layer %d, honest vr" % i, vres((i, "liu_vr"))))
        for i in sorted({top, mid} - {1}, reverse=True):
            out.append(("vr = S / gr at layer %d, honest below" % i, vres((i, "vr_div"))))
    out.append(("everything re-made", vres((1, "vr_div"))))
    out.append(("everything re-made, true last vr", vres((1, "true_vr"))))
    return out


@functools.lru_cache(maxsize=None)
def rows(name, family):
    """[(label, plan, transcript bytes, declared check)] on the family's tape; a plan the forger cannot finish is (label, plan, None, DeadEnd)"""
    off, w, tape = gc.offsets(name), wiring(name), gc.tape(name, family)
    out = []
    for k, (label, plan) in enumerate(plans(name)):
        try:
            el, declared = gf.forge(w, off, gv.Tape(off, tape), honest(name, family), plan, seed=SEED + k)
            out.append((label, plan, gv.to_bytes(el), declared))
        except gf.DeadEnd as e:
            out.append((label, plan, None, e))
    return tuple(out)


def reached(off, declared):
    """(closing values, Liu closing tests, input checks) a verification makes up to and including the declared check: with the loops on the device, the number of
    vp_predicates, vp_liu_gr and vp_layer_mle calls"""
    order = gv.checks(off)
    upto = order if declared is None else order[:order.index(tuple(declared)) + 1]
    return tuple(sum(c[0] == kind for c in upto) for kind in ("semi_final", "liu_semi_final", "input"))


def reference(name, family, tr, **kw):
    off = gc.offsets(name)
    return gv.verify(wiring(name), off, gv.Tape(off, gc.tape(name, family)), tr, **kw)


# ---- the Fiat-Shamir form ---------------------------------------------------------------------------------------------------------------------------------------------
def honest_fs(oc, off, state):
    """The honest non-interactive proof from `state`, by a fixed point over the oracle's tape-form prover: challenge m depends only on the messages in front of it, and
    those on the challenges in front of them, so every pass of (prove on the tape, derive the tape from the proof) fixes at least one more challenge."""
    import full_fs_ref as ff
    import gkr_fs_cases as gfc
    import numpy as np
    import pc_fs_ref as fs
    tape = np.zeros((off.n, 2), np.uint64)
    for _ in range(gfc.n_draws(off) + 2):
        tr = oc.prove_gkr_tape(tape)[0]
        nxt = ff.gkr_schedule(fs.Chain(state), off, gfc.elements(tr))
        if nxt.tobytes() == tape.tobytes():
            return tr
        tape = nxt
    raise AssertionError("no fixed point")


def rows_fs(w, off, state, honest_proof, plan_list, seed=SEED):
    """[(label, plan, proof bytes, declared check, closing chain state, derived tape)] on the chain from `state`"""
    old = gv.elements(honest_proof)
    out = []
    for k, (label, plan) in enumerate(plan_list):
        src = gv.Chained(off, state)
        el, declared = gf.forge(w, off, src, old, plan, seed=seed + k)
        out.append((label, plan, gv.to_bytes(el), declared, src.ch.s, src.tape))
    return out


# ---- the joined proof and the record --------------------------------------------------------------------------------------------------------------------------------
def joined_forgeries(w, off, state, gkr):
    """The GKR section of a joined proof (full_fs_ref.sections; state and gkr: gkr_fs_cases.full_fs_head_state) re-made to the end, and the same with the input layer's
    true value as the last vr: [(section bytes, declared check, derived tape)]"""
    plan_list = [("everything re-made", {"lie": "vres", "stop": (1, "vr_div")}), ("everything re-made, true last vr", {"lie": "vres", "stop": (1, "true_vr")})]
    out = [(bad, declared, tape) for _, _, bad, declared, _, tape in rows_fs(w, off, state, gkr, plan_list)]
    assert [d for _, d, _ in out] == [("input", 0, -1), ("liu_semi_final", 1, -1)]
    return out


def record_forgery(c_arrays, rec, n_pub_mask=None):
    """(forged record, honest GKR section, forged GKR section) for a complete-protocol record of the circuit made from c_arrays: the GKR section re-made to the end on
    the record's own challenges — the verifier's seeded draws, gkr_tape_cases.uniform."""
    import oracle_binding as ob
    import pc_forge
    oc = ob.Circuit.custom(*c_arrays)
    w, off = vs.wiring_from(oc, c_arrays), gc.Offsets.of(oc)
    sec = pc_forge.sections(rec, n_pub_mask)
    lo, hi = sec["transcript"] + 32, sec["root_h"]
    assert hi - lo == 16 * off.n_tr
    tape = gc.uniform(off, gc.SEED)
    assert gv.verify(w, off, gv.Tape(off, tape), rec[lo:hi], input_check=False) is None, "the record's GKR section is not honest on the seeded tape"
    el, declared = gf.forge(w, off, gv.Tape(off, tape), gv.elements(rec[lo:hi]), {"lie": "vres", "stop": (1, "vr_div")}, seed=SEED)
    assert declared == ("input", 0, -1) and gv.verify(w, off, gv.Tape(off, tape), el, input_check=False) is None
    return rec[:lo] + gv.to_bytes(el) + rec[hi:], rec[lo:hi], gv.to_bytes(el)
