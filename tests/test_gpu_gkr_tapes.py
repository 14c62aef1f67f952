"""GPU (-m gpu): every device path of the GKR sumcheck on arbitrary challenge tapes (tests/gkr_tape_cases.py), against orc_prove_gkr_tape of the same arrays
and the same tape, byte for byte.  A difference is reported as (layer, phase, round, element) with both values.  tests/test_gkr_tape_host.py (CPU) pins the
oracle's tape entry to the real reference's records, checks that the oracle's own verifier and the host verifier accept every tape used here, and that the
transcripts of the value families are at most half zero.  Every test asserts that the path it names ran, from the profiled launch table, vp_tuning_get,
vp_get_round_stats or vp_get_round_shard.

circuit      arrays                                                   bit lengths      what it is there for
S            make(12, [40, 33, 50, 17])                               6, 6, 6, 5       closing kernels only; every interactive phase resident from round 1 or 2
M            make(11, [1500, 2100, 900, 4100, 700])                   11,12,10,13,10   seg kernels, multi-table phase 2, ragged layers
E_real       make(13, [4096, 1024, 3000], values=EDGE_VALUES),        12, 10, 12       edge witness x edge challenges: real values throughout ...
E_complex      real and complex constants                                              ... and the same set in both limbs of the constants
R            randomize(4, 12), VP_SF_BIG_LOG=12                       12 x 4           the three-round fold kernel on 2^12 tables, complex values
K_skewed     make_skewed(104, real_consts=True), VP_FUSE_MIN_LOG=14   14 ... 16        GenP1 / GenLiu / GenP2, heavy rows, all eleven gate types, real values
K_custom_c   the arrays of tests/golden custom_c, VP_FUSE_MIN_LOG=14  14 ... 16        the same with complex constants

switch (a fresh session each)        what it selects
VP_DROP_Y=0                          every round sums its own b instead of deriving it from the previous claim q(r)
VP_DROP_Y1=1                         round 1 leaves its b to the fix-up pass over the finished transcript
VP_REAL_V=0                          the general complex products on real values
VP_FUSE_INIT=0 / VP_FUSE_P2=0 (K)    no init / no phase-2 init generated inside the first fold launch
VP_PERSIST=0                         interactive: one launch per round, no resident mailbox kernel
VP_FAST_INIT=0                       interactive: the init calls through the per-sumcheck kernels
VP_PREFETCH_R1=0                     interactive: round 1 is not queued behind the init call
VP_SPLIT_COST_PERCENT=0              index split: every chain with a long enough table is cut"""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import gkr_drive
import gkr_tape_cases as gc
from test_gpu_parity import _engagement, _kind, _sharded_parts, _split_parts

pytestmark = pytest.mark.gpu
P = gc.P
VP_EINVAL = -1
SWITCHES = [{"VP_DROP_Y": "0"}, {"VP_DROP_Y1": "1"}, {"VP_REAL_V": "0"}]
K_SWITCHES = [{"VP_FUSE_INIT": "0"}, {"VP_FUSE_P2": "0"}]
MODES = {"default": {}, "launch_per_round": {"VP_PERSIST": "0"}, "round1_kernels": {"VP_FAST_INIT": "0"}, "no_prefetch": {"VP_PREFETCH_R1": "0"}}
_ids = lambda e: "-".join("%s=%s" % kv for kv in e.items()) if isinstance(e, dict) else str(e)


@pytest.fixture(scope="module")
def circuits(vp):
    made = {}

    def get(name):
        if name not in made:
            c = gc.build(vp, name)
            assert c.hash() == gc.oracle_circuit(name).hash()
            made[name] = c
        return made[name]
    yield get
    for c in made.values():
        c.close()


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


def _compare(name, families, prove):
    """prove(family) -> transcript, for every family; all differences are collected before the test fails."""
    bad = []
    for fam in families:
        d = gc.first_difference(name, fam, prove(fam), gc.expected(name, fam))
        if d:
            bad.append(d)
    assert not bad, "%d of %d tapes differ:\n%s" % (len(bad), len(families), "\n".join(bad))


def _batched(s, name, check=True):
    def prove(fam):
        s.set_tape(gc.tape(name, fam))
        tr, _ = s.prove_gkr()
        tr2, _ = s.prove_gkr()                  # the first proof of a session builds the plan, every later one replays its graph
        assert tr2 == tr, "%s / %s: the replay differs from the first pass" % (name, fam)
        if check and tr == gc.expected(name, fam):
            assert s.check(tr)[0], "%s / %s: the host verifier rejects the device's proof" % (name, fam)
        return tr
    return prove


def _launches(vp, s, name):
    s.set_tape(gc.tape(name, "uniform"))
    tr, launches, jobs = _engagement(vp, s)
    assert tr == gc.expected(name, "uniform")
    return {k: launches.get(_kind(vp, k), 0) for k in ("SFGEN", "SF", "SEG", "EMIT", "FIXUP", "CHUNKS", "LIGHT")}, jobs


def _assert_batched_path(vp, s, name):
    n, jobs = _launches(vp, s, name)
    print("%s: launches %r, generating jobs %d" % (name, n, jobs))
    if name == "S":
        assert n["SF"] == 0 and n["SFGEN"] == 0 and n["SEG"] + n["EMIT"] > 0, "S is meant to run the closing kernels only: %r" % n
    if name == "M":
        assert n["SEG"] > 0 and n["EMIT"] > 0, n
    if name == "R":
        assert s.options_in_effect().sf_big_log == 12 and n["SF"] + n["SFGEN"] > 0, "the fold kernel did not run on the 2^12 tables: %r" % n
    if name.startswith("K"):
        assert s.options_in_effect().fuse_min_log == 14 and n["SFGEN"] > 0 and jobs > 0 and n["CHUNKS"] > 0, (n, jobs)
    return n, jobs


# ---- 1. batched, default switches: every circuit, every family -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.GPU_CIRCUITS)
def test_batched_default_every_family(vp, circuits, name):
    with _session(vp, circuits(name), gc.env(name)) as s:
        _compare(name, list(gc.FAMILIES), _batched(s, name))
        _assert_batched_path(vp, s, name)


# ---- 2. batched under switches: the edge families, the same bytes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,switch", [(n, sw) for n in gc.GPU_CIRCUITS for sw in SWITCHES + (K_SWITCHES if n.startswith("K") else [])], ids=_ids)
def test_batched_under_switches(vp, circuits, name, switch):
    with _session(vp, circuits(name), dict(gc.env(name), **switch)) as s:
        eff = s.options_in_effect()
        if "VP_DROP_Y" in switch:
            assert eff.drop_y == 0
        if "VP_DROP_Y1" in switch:
            assert eff.drop_y_round1 == 1
        if "VP_REAL_V" in switch:
            assert eff.real_values == 0
        _compare(name, gc.EDGE_FAMILIES, _batched(s, name, check=False))
        n, jobs = _launches(vp, s, name)
        if "VP_DROP_Y1" in switch:
            assert n["FIXUP"] > 0, "no fix-up pass ran: %r" % n
        if "VP_FUSE_INIT" in switch:
            assert jobs == 0 and n["SFGEN"] == 0
        if "VP_FUSE_P2" in switch:
            with _session(vp, circuits(name), gc.env(name)) as s0:
                assert 0 < jobs < _launches(vp, s0, name)[1], "the phase-2 generator was not what the switch removed"


# ---- 3. interactive, message by message through the C ABI ------------------------------------------------------------------------------------------------------
def _interactive_families(name):
    return list(gc.STRIPES) if name.startswith("K") else list(gc.FAMILIES)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", gc.GPU_CIRCUITS)
def test_interactive_every_mode(vp, circuits, name, mode):
    """The limb-(p - 1) families (gkr_tape_cases.LIMB_M1_FAMILIES) are the ones whose challenges have all 61 low bits set below the mailbox's tag bits."""
    off = gc.offsets(name)
    with _session(vp, circuits(name), dict(gc.env(name), **MODES[mode])) as s:
        eff = s.options_in_effect()
        assert eff.persistent_rounds == (0 if mode == "launch_per_round" else 1)
        assert eff.interactive_fast_init == (0 if mode == "round1_kernels" else 1)
        assert eff.prefetch_round1 == (0 if mode == "no_prefetch" else 1)
        how = set()

        def prove(fam):
            tr, _ = gkr_drive.prove(vp, s.gpu_ctx(), off, gc.tape(name, fam))
            st = s.round_stats()
            assert len(st) == sum(rounds for _, _, _, rounds, _ in off.parts), "vp_get_round_stats does not list every round"
            how.update(e["how"] for e in st)
            return tr
        fams = _interactive_families(name)
        assert name.startswith("K") or set(gc.LIMB_M1_FAMILIES) <= set(fams)
        _compare(name, fams, prove)
        print("%s / %s: rounds answered by %r (0 direct launch, 1 resident kernel, 2 queued behind the init call)" % (name, mode, sorted(how)))
        assert (1 in how) == (mode != "launch_per_round"), how
        assert (2 in how) == (mode != "no_prefetch"), how
        if name == "S" and mode == "default":
            assert how == {1, 2}, "S is meant to be resident from round 1 or 2 in every phase: %r" % how


# ---- 4. chain-sharded, world 3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.GPU_CIRCUITS)
def test_chain_sharded_world_3(vp, circuits, name):
    with _session(vp, circuits(name), gc.env(name)) as s:
        busy = set()

        def prove(fam):
            s.set_tape(gc.tape(name, fam))
            parts = _sharded_parts(vp, s, 3)
            busy.update(r for r, p in enumerate(parts) if any(p))
            return vp.sum_transcripts(parts)
        _compare(name, gc.EDGE_FAMILIES + ("uniform", "minus_one_limbs"), prove)
        assert busy == {0, 1, 2}, "a rank proved nothing: %r" % busy


# ---- 5. index split: the last log2 W' rounds of the split tables are finished on the host ------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("name", ["R", "K_skewed", "K_custom_c"])
def test_index_split(vp, circuits, name, world):
    min_log = 12 - 3 if name == "R" else 11           # R: tables of 2^12 still split over 8 slices
    with _session(vp, circuits(name), dict(gc.env(name), VP_SPLIT_COST_PERCENT="0")) as s:
        s.set_tape(gc.tape(name, "uniform"))
        s.set_shard(0, world); s.set_shard_split(min_log)
        owner, _ = s.shard_chains()
        assert (owner == -1).any(), "nothing was split"
        s.set_shard(0, 1)
        for exchange in (True, False):
            def prove(fam):
                s.set_tape(gc.tape(name, fam))
                return _split_parts(vp, s, world, min_log=min_log, exchange=exchange)
            _compare(name, ("sprinkle",) + tuple(gc.STRIPES), prove)


# ---- 6. round-sharded interactive: world 2 and 4 on one device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("name", ["M", "R"])
def test_round_sharded_interactive(vp, circuits, name, world):
    off = gc.offsets(name)
    min_log = 5                                        # tables of >= 2^(log2 W + 5) entries are split: the gather falls several rounds into the phase
    with _session(vp, circuits(name), gc.env(name), devices=[0] * world, round_shard_min_log=min_log) as s:
        ctxs = [s.rank_ctx(r) for r in range(world)]
        w = ctypes.c_int(0)
        for r, x in enumerate(ctxs):
            rk = ctypes.c_int(-1)
            assert vp.lib_gpu().vp_get_round_shard(x, ctypes.byref(rk), ctypes.byref(w), None) == 0 and (rk.value, w.value) == (r, world)
        seen = []

        def prove(fam):
            tr, d = gkr_drive.prove(vp, ctxs, off, gc.tape(name, fam))
            seen.append((d.exchanges, d.partial_rounds))
            return tr
        _compare(name, gc.EDGE_FAMILIES + ("uniform", "minus_one_limbs"), prove)
        total = sum(rounds for _, _, _, rounds, _ in off.parts)
        print("%s W=%d: (gathers, rounds with partial polynomials) per proof %r of %d rounds" % (name, world, sorted(set(seen)), total))
        assert all(g > 0 and 0 < p < total for g, p in seen), "no gather, or no round before / after it: %r" % seen
        assert all(e["how"] != 1 for r in range(world) for e in s.round_stats(rank=r)), "resident kernel on ranks that share a device"


# ---- 7. uv_corners: the claims are witness values, looked up without arithmetic ---------------------------------------------------------------------------------
@pytest.mark.parametrize("interactive", [False, True], ids=["batched", "interactive"])
@pytest.mark.parametrize("name", gc.GPU_CIRCUITS)
def test_uv_corner_claims_are_witness_values(vp, circuits, name, interactive):
    """With r_u and r_v 0 / 1 patterns, claim_u = V_{i-1}(r_u) and every claims_v[j] is the value of one wire (gkr_tape_cases.corner_claims: which one; zero past
    the end of the layer or subset): an expectation that needs neither prover.  The bit order comes from a one-hot check of verifier_sums.layer_mle; the values
    from the device's own evaluation, which tests/test_gpu_parity.py pins against the oracle's (and, on S, from verifier_sums.evaluate in integers).  The
    CPU suite checks the same lookup against the oracle's transcripts (tests/test_gkr_tape_host.py)."""
    import verifier_sums as vs
    off, tape = gc.offsets(name), gc.tape(name, "uv_corners")
    assert vs.layer_mle([(0, 0), (0, 0), (1, 0), (0, 0)], [(0, 0), (1, 0)]) == (1, 0), "bit 0 of the index goes with r[0]"
    with _session(vp, circuits(name), gc.env(name)) as s:
        if interactive:
            tr, _ = gkr_drive.prove(vp, s.gpu_ctx(), off, tape)
        else:
            s.set_tape(tape)
            tr, _ = s.prove_gkr()
        got = gc.elements(tr)
        values = {i: s.layer_values(i) for i in range(off.n_layers - 1)}
        if name == "S":
            ev = vs.evaluate(vs.wiring_from(gc.oracle_circuit(name), gc.arrays(name)))
            for i in values:
                assert [(int(a), int(b)) for a, b in values[i]] == ev[i]
        want = gc.corner_claims(name, values)
        assert len(want) == sum(claims for ph, _, _, _, claims in off.parts if ph in ("phase 1", "phase 2")) and any(v != (0, 0) for v in want.values())
        for at, v in sorted(want.items()):
            assert got[at] == v, "%s: element %d (%s) is %r, the wire it names holds %r" % (name, at, off.locate(at), got[at], v)
        assert tr == gc.expected(name, "uv_corners")


# ---- refusals: a limb >= p never reaches a kernel -----------------------------------------------------------------------------------------------------------------
def test_non_canonical_challenges_are_refused_everywhere(vp, circuits):
    """p and 2^63 in each challenge argument of vp_prove_gkr, vp_shard_vu_partials, vp_vres, vp_phase1_init, vp_phase2_init and vp_liu_init: VP_EINVAL with a
    text, on the host.  An interactive phase interrupted by refused init calls continues bit-identically, and the context then proves the uniform tape's
    transcript.  Nothing is provoked on the device: no call here launches anything with a bad limb."""
    name = "M"
    off, tape, lib = gc.offsets(name), gc.tape(name, "sprinkle"), vp.lib_gpu()
    n = off.n_layers
    top = n - 1
    with _session(vp, circuits(name), gc.env(name)) as s:
        h = s.gpu_ctx()
        gkr_drive._bind(lib)
        lib.vp_prove_gkr.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        lib.vp_shard_vu_partials.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        d = gkr_drive.Drive(vp, h, off, tape)
        good = {"r0": d._slot(off.r0, off.max_bl), "ru": d._slot(off.ru[top], off.max_bl), "ar": d._slot(off.ar[top], 1), "sig": d._slot(off.sig[top], n),
                "rv": d._slot(off.rv[top], 0)}
        dad_bl = gc.oracle_circuit(name).subsets(top)[1][top - 1]     # vp_liu_init(top) reads this many entries of r_v[top]: the bit length of the top layer's subset of layer top - 1
        assert 1 <= dad_bl <= off.mdb[top]
        used = {"r0": off.bl[top], "ru": off.bl[top - 1], "ar": 1, "sig": 2, "rv": dad_bl}
        out = np.zeros((4, 2), np.uint64)
        buf = ctypes.create_string_buffer(16 * off.n_tr + 4096)
        wr = ctypes.c_uint64(0)

        def refused(rc, what):
            assert rc == VP_EINVAL, "%s accepted a non-canonical limb (%d)" % (what, rc)
            assert b"canonical" in lib.vp_last_error(h), (what, lib.vp_last_error(h))

        def bad_copies(key):
            """The argument with p, then 2^63, in the real and in the imaginary limb of its first and of its last used element."""
            for value in (P, 1 << 63):
                for at in {0, used[key] - 1}:
                    for limb in (0, 1):
                        a = good[key].copy()
                        a[at, limb] = value
                        yield a

        def rv_ptrs(a):
            return ctypes.cast((ctypes.c_void_p * n)(*[a.ctypes.data if k == top else None for k in range(n)]), ctypes.c_void_p)

        def init_calls_with_bad_limbs():
            for a in bad_copies("r0"):
                refused(lib.vp_phase1_init(h, top, a.ctypes.data, good["ar"].ctypes.data), "vp_phase1_init(r_liu)")
            for a in bad_copies("ar"):
                refused(lib.vp_phase1_init(h, top, good["r0"].ctypes.data, a.ctypes.data), "vp_phase1_init(assert_random)")
            for a in bad_copies("ru"):
                refused(lib.vp_liu_init(h, top, a.ctypes.data, rv_ptrs(good["rv"]), good["sig"].ctypes.data), "vp_liu_init(r_u)")
            for a in bad_copies("sig"):
                refused(lib.vp_liu_init(h, top, good["ru"].ctypes.data, rv_ptrs(good["rv"]), a.ctypes.data), "vp_liu_init(s)")
            for a in bad_copies("rv"):
                refused(lib.vp_liu_init(h, top, good["ru"].ctypes.data, rv_ptrs(a), good["sig"].ctypes.data), "vp_liu_init(r_v)")
            for a in bad_copies("r0"):
                refused(lib.vp_vres(h, a.ctypes.data, off.bl[top], out.ctypes.data), "vp_vres")

        # the batched calls: a bad limb in the first, a middle and the last tape element
        for value in (P, 1 << 63):
            for at in (0, off.n // 2, off.n - 1):
                for limb in (0, 1):
                    t = np.array(tape)
                    t[at, limb] = value
                    refused(lib.vp_prove_gkr(h, t.ctypes.data, off.n, buf, len(buf), ctypes.byref(wr)), "vp_prove_gkr")
                    refused(lib.vp_shard_vu_partials(h, t.ctypes.data, off.n, out.ctypes.data, 4, ctypes.byref(wr)), "vp_shard_vu_partials")
                    with pytest.raises(ValueError):
                        s.set_tape(t)
        init_calls_with_bad_limbs()
        # phase 1 of the top layer, undisturbed and with the refused calls between its rounds (and phase 2's init refused after it)
        runs = []
        for disturb in (False, True):
            msgs = []
            assert lib.vp_vres(h, good["r0"].ctypes.data, off.bl[top], out.ctypes.data) == 0
            assert lib.vp_phase1_init(h, top, good["r0"].ctypes.data, good["ar"].ctypes.data) == 0
            prev, poly = np.zeros((1, 2), np.uint64), np.zeros((3, 2), np.uint64)
            for j in range(off.bl[top - 1]):
                if disturb and j in (0, 1, 4, off.bl[top - 1] - 1):
                    init_calls_with_bad_limbs()
                assert lib.vp_round(h, prev.ctypes.data, poly.ctypes.data) == 0, lib.vp_last_error(h)
                msgs.append(poly.tobytes())
                prev = good["ru"][j:j + 1].copy()
            if disturb:
                init_calls_with_bad_limbs()
            assert lib.vp_finalize(h, prev.ctypes.data, out.ctypes.data, 1) == 0, lib.vp_last_error(h)
            msgs.append(out[:1].tobytes())
            if disturb:
                for a in bad_copies("ru"):
                    refused(lib.vp_phase2_init(h, top, a.ctypes.data), "vp_phase2_init")
            assert lib.vp_phase2_init(h, top, good["ru"].ctypes.data) == 0, lib.vp_last_error(h)
            assert lib.vp_round(h, np.zeros((1, 2), np.uint64).ctypes.data, poly.ctypes.data) == 0
            msgs.append(poly.tobytes())
            runs.append(b"".join(msgs))
        assert runs[0] == runs[1], "a refused init call disturbed the sumcheck in progress"
        at = off.claim_index("phase 1", top) - 3 * off.bl[top - 1]
        assert runs[0][:16 * (3 * off.bl[top - 1] + 1)] == gc.expected(name, "sprinkle")[16 * at:16 * (at + 3 * off.bl[top - 1] + 1)]
        # and the context is as good as new
        s.set_tape(gc.tape(name, "uniform"))
        tr, _ = s.prove_gkr()
        assert tr == gc.expected(name, "uniform")
        tr, _ = gkr_drive.prove(vp, h, off, gc.tape(name, "sprinkle"))
        assert tr == gc.expected(name, "sprinkle")
