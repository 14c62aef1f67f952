"""GPU (-m gpu): the commitment WITH masks (vp_commit_private_masked, vp_commit_public_masked / vp_commit_public_eq_masked, vp_fri_commit / vp_fri_step,
vp_fri_final_mask, vp_fri_open / vp_fri_open_many) against the oracle's restatement of the same calls (orc_commitment_array_masked, itself pinned by the real
reference's eleven records and by tests/pc_mask_ref.py) and, for masks that pad to at most 256 elements, against that Python reference directly — at every
input bit length and padded mask length at which the device takes another path:

  n = 7 .. 12   every accepted mask length (8 .. M/2; at n = 7, 8 all of them longer than a slice's message: k_mask_combine with c = 2 .. 16), the three input
                sets of pc_array_inputs (uniform, edges, a five-wire witness) crossed with the six mask families of pc_masked_inputs
  n = 13        ms in {8, N/2, N, 2N, 8N, 16N}, the uniform and the edges input set crossed with the six families
  n = 14 .. 16  the same mask lengths, the uniform set with the uniform family and the edges set with the edges family (one oracle run costs 1.5 .. 6.5 s of CPU
                there, so the sets and the families are paired, not crossed); n = 15, 16 reach the radix-8 pair for the ms-point inverse (2^13, 2^14) and for the
                2 ms-point inverse (2^14, 2^15); n = 16 also with masks of 5000 and 10000 elements
  n = 18, 20    from recorded oracle runs (tests/golden/pc_masked_array_*.bin): ms = 2^16 with a 2^17-point quotient transform, and ms = N under edge limbs

Every comparison is byte equality.  An expectation is computed once per case and shared (_EXP, _PY)."""
import ctypes
import json
import os

import numpy as np
import pytest

import pc_array_inputs as pai
import pc_mask_ref as ref
import pc_masked_inputs as pmi
from conftest import GOLDEN
from test_gpu_masked_fast_path import Ctx, _leaves_of, _sha3_leaf
from test_gpu_sharded_dropin_commitment import _opening_ok

pytestmark = pytest.mark.gpu
VP_EINVAL, VP_ELIMIT = -1, -5
P = pmi.P61

_EXP, _PY = {}, {}


def _n_leaves(n, oracle):
    return 1 << (n - 2) if oracle < 2 else 16 * ((1 << (n - 6)) >> (oracle - 1))


def _open_list(n):
    """(oracle, leaf): the first leaf, the last and the coset-block edges of l, h, the first two FRI levels and the 16-leaf last level; both ends of the others"""
    st, out = n - 6, []
    for o in range(2 + st):
        nl = _n_leaves(n, o)
        cnt = 16 if o == 1 + st else 8 if o < 2 else 6 if o < 4 else 2
        out += [(o, lf) for lf in (_leaves_of(nl, cnt) if cnt > 2 else [0, nl - 1])]
    return out


def _expected(ob, x, f, key, pub=None):
    """the oracle's record (split into fields), the opening list and the oracle's 130 values of each opening — once per key"""
    if key not in _EXP:
        n = x["n"]
        opens = _open_list(n)
        rec, vals = pmi.oracle_masked(ob.lib(), x["values"], x["n_used"], x["pub"] if pub is None else pub, n, f["r"], f["pri_mask"], f["pub_mask"], opens)
        _EXP[key] = (pmi.split_masked_record(rec, n), opens, vals)
    return _EXP[key]


def _python(ob, n, f, key):
    """the mask slice in Python integers (masks that pad to at most 256 elements) — once per (n, family, ms)"""
    if key not in _PY:
        pr = lambda a: [(int(u), int(v)) for u, v in a]
        _PY[key] = ref.MaskSlice(n, pr(f["pri_mask"]), pr(f["pub_mask"]), pr(f["r"]), ob.root_of_unity(n - 1))
    return _PY[key]


def _ctx(vp, x):
    c = Ctx(vp, x["values"], x["n"])
    if x["n_used"] != x["values"].shape[0]:                # the input layer's own size (a five-wire witness, three unused wires)
        assert c.L.vp_pc_load_input(c.ctx, c.values.ctypes.data, x["n_used"], x["n"]) == 0
    return c


def _device(c, x, f, public=None, late=False, cut=None, profile=False):
    """vp_commit_private_masked, the public commit (`public(c)`, default vp_commit_public_masked on x["pub"]), then the first `cut` challenges through
    vp_fri_commit (None: all of them) and the rest through vp_fri_step: the record's fields, and the launch tables of the three calls if asked for"""
    st, r = x["n"] - 6, f["r"]
    cut = st if cut is None else cut
    c.root_l.raw = c.root_h.raw = bytes(32); c.inner[:] = 0; c.alls[:] = 0
    c.hash_late(late)
    c.profiling(profile)
    rows = []
    c.commit_private(f["pri_mask"]); rows.append(c.rows() if profile else None)
    if public is None:
        c.commit_public(x["pub"], f["pub_mask"])
    else:
        public(c)
    rows.append(c.rows() if profile else None)
    roots = c.fri_commit(r[:cut], cut) if cut else b""
    rows.append(c.rows() if profile and cut else None)
    c.profiling(False)
    for k in range(cut, st):
        roots += c.fri_step(r[k])
    c.hash_late(False)
    fin, fm = c.finals()
    root_l, root_h, inner, alls = c.state()
    return {"root_l": root_l, "root_h": root_h, "public": inner + alls, "roots": [roots[32 * k:32 * k + 32] for k in range(st)], "final": fin, "final_mask": fm}, rows


def _compare(got, want, what):
    assert got["root_l"] == want["root_l"], what + ": merkle_root_l"
    assert got["root_h"] == want["root_h"], what + ": merkle_root_h"
    assert got["public"][:16] == want["public"][:16], what + ": input_0"
    g, w = np.frombuffer(got["public"][16:], np.uint64).reshape(65, 2), np.frombuffer(want["public"][16:], np.uint64).reshape(65, 2)
    assert np.array_equal(g, w), what + ": all_sum, first at slice %d" % int(np.argmax((g != w).any(axis=1)))
    for k, (a, b) in enumerate(zip(got["roots"], want["roots"])):
        assert a == b, what + ": FRI root %d" % k
    assert got["final"] == want["final"], what + ": final codeword"
    assert got["final_mask"] == want["final_mask"], what + ": final mask codeword"


def _check_openings(c, want, opens, vals, what, py=None, single=()):
    """vp_fri_open_many at `opens` (and vp_fri_open at `single`): the 130 values are the oracle's, the leaf digest is SHA3-256 over the 65 pairs (hashlib), the path
    climbs to the ORACLE's root of that level; with a Python reference, the mask pair is its polynomial's value at the two positions"""
    v, p, pl = c.open_many(opens)
    for i, (o, lf) in enumerate(opens):
        root = want["root_l"] if o == 0 else want["root_h"] if o == 1 else want["roots"][o - 2]
        path = [p[i, 32 * k:32 * k + 32].tobytes() for k in range(pl[i])]
        assert np.array_equal(v[i], vals[i]), "%s: values of oracle %d at leaf %d" % (what, o, lf)
        assert path[-1] == _sha3_leaf(v[i]), "%s: leaf digest of oracle %d at leaf %d" % (what, o, lf)
        assert len(path) == _n_leaves(c.n, o).bit_length() and _opening_ok(root, lf, v[i], path), "%s: path of oracle %d at leaf %d" % (what, o, lf)
        if py is not None:
            assert [(int(a), int(b)) for a, b in v[i][128:130]] == list(py.pair(o, lf)), "%s: mask pair of oracle %d at leaf %d against the Python reference" % (what, o, lf)
    for o, lf in single:
        i = opens.index((o, lf))
        assert c.open1(o, lf) == (v[i].tobytes(), p[i, :32 * pl[i]].tobytes()), "%s: vp_fri_open of oracle %d at leaf %d" % (what, o, lf)


def _ladder_case(c, ob, x, kind, fam, ms, m=None, openings=True):
    n = x["n"]
    f = pmi.family(fam, n, ms, m=m)
    what = "n=%d ms=%d inputs %s masks %s" % (n, ms, kind, fam)
    want, opens, vals = _expected(ob, x, f, (n, kind, fam, ms, m))
    got, _ = _device(c, x, f)
    _compare(got, want, what)
    py = _python(ob, n, f, (n, fam, ms, m)) if ms <= 256 else None
    if py is not None:
        assert got["public"][16 + 64 * 16:] == np.array(py.all_sum, np.uint64).tobytes(), what + ": all_sum[64] against the Python reference"
        assert got["final_mask"] == np.array(py.final_mask(), np.uint64).tobytes(), what + ": final mask codeword against the Python reference"
    if openings:
        _check_openings(c, want, opens, vals, what, py)
    return f, want, opens, vals


# ---- the ladder -------------------------------------------------------------------------------------------------------------------------------------------

SMALL = [(n, ms) for n in range(7, 13) for ms in pmi.accepted_ms(n)]


def _large_ms(n):
    N = 1 << (n - 6)
    return sorted(set(pmi.accepted_ms(n)) & {8, N // 2, N, 2 * N, 8 * N, 16 * N})


def test_the_ladders_cases():
    assert len(SMALL) == 3 + 4 + 5 + 6 + 7 + 8 and SMALL[0] == (7, 8) and SMALL[-1] == (12, 1024)
    assert [_large_ms(n) for n in (13, 14, 15, 16)] == [[8, 64, 128, 256, 1024, 2048], [8, 128, 256, 512, 2048, 4096], [8, 256, 512, 1024, 4096, 8192],
                                                       [8, 512, 1024, 2048, 8192, 16384]]
    assert pmi.padded_length(16, 5000)[1] == 1 << 13 and pmi.padded_length(16, 10000)[1] == 1 << 14


@pytest.mark.parametrize("kind", pai.SETS)
@pytest.mark.parametrize("n,ms", SMALL)
def test_ladder_every_mask_length_up_to_n12_vs_oracle(vp, ob, n, ms, kind):
    """n = 7 .. 12 (transforms of 2 .. 64 points per slice, one LDS launch each), every accepted padded mask length, one input set per case and the six mask
    families on ONE context, one after the other: roots of l and h, input_0, all_sum[65], every FRI root, both final codewords and the openings against the
    oracle; for ms <= 256 also all_sum[64], the final mask codeword and every opened mask pair against the Python reference."""
    x = pai.inputs(kind, n)
    c = _ctx(vp, x)
    try:
        for fam in pmi.FAMILIES:
            _ladder_case(c, ob, x, kind, fam, ms)
    finally:
        c.close()


@pytest.mark.parametrize("fam", pmi.FAMILIES)
@pytest.mark.parametrize("kind", ["uniform", "edges"])
@pytest.mark.parametrize("ms", _large_ms(13))
def test_ladder_n13_every_family_vs_oracle(vp, ob, ms, kind, fam):
    """n = 13 (the bit length of the real reference's records): ms = 8, N/2, N (the boundary between the two encode forms), 2N, 8N, 16N (k_mask_combine with
    c = 2, 8, 16), two input sets crossed with the six families."""
    x = pai.inputs(kind, 13)
    c = _ctx(vp, x)
    try:
        _ladder_case(c, ob, x, kind, fam, ms)
    finally:
        c.close()


@pytest.mark.parametrize("kind", ["uniform", "edges"])
@pytest.mark.parametrize("n,ms,m", [(n, ms, None) for n in (14, 15, 16) for ms in _large_ms(n)] + [(16, 1 << 13, 5000), (16, 1 << 14, 10000)])
def test_ladder_n14_to_n16_vs_oracle(vp, ob, n, ms, m, kind):
    """n = 14, 15, 16: the uniform input set under uniform masks and the edges set under edge masks and edge challenges.  ms = 2^13 (n = 15, 16) and 2^14
    (n = 16) run the mask's own inverse transform on the radix-8 pair — one row on a root table of a larger order — and 2 ms = 2^14, 2^15 its quotient's."""
    x = pai.inputs(kind, n)
    c = _ctx(vp, x)
    try:
        _ladder_case(c, ob, x, kind, kind, ms, m=m)
    finally:
        c.close()


def _ntt_rows(c):
    """(jobs, work) of the k_ntt_lds rows in the launch table of the last profiled call"""
    k = ctypes.c_int(0)
    c.L.vp_get_launch_stats(c.ctx, None, 0, ctypes.byref(k))
    arr = (c.vp.LaunchStat * max(1, k.value))()
    c.L.vp_get_launch_stats(c.ctx, arr, k.value, ctypes.byref(k))
    return [(arr[i].jobs, arr[i].work) for i in range(k.value) if c.L.vp_kernel_name(arr[i].kind) == b"k_ntt_lds"]


def test_the_encode_form_changes_above_a_slices_message_not_at_it(vp):
    """ms == N is the last length of the slices' own encode (one zero-padded array, 32 twisted cosets), 2 N the first of k_mask_combine's (32 plain transforms of
    combined rows).  The values cannot tell the two apart at ms == N — there the combined rows are the twisted array itself — so the launch table does: the last
    transform row of vp_commit_private_masked covers 32 N-point transforms in every case, and the twisted form counts one multiplication per point more."""
    n, N = 13, 128
    x = pai.inputs("uniform", n)
    c = _ctx(vp, x)
    try:
        last = {}
        for ms in (N // 2, N, 2 * N):
            c.profiling(True)
            c.commit_private(pmi.family("uniform", n, ms)["pri_mask"])
            last[ms] = _ntt_rows(c)[-1]
            c.profiling(False)
        assert [j for j, _ in last.values()] == [32, 32, 32], last
        assert last[N // 2] == last[N] and last[N][1] - last[2 * N][1] == 32 * N, last
    finally:
        c.close()


# ---- both public forms --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pt", ["uniform", "corner"])
@pytest.mark.parametrize("n,ms", [(7, 16), (10, 16), (10, 64), (13, 128), (13, 256)])
def test_both_public_forms_vs_oracle_on_its_own_eq_table(vp, ob, n, ms, pt):
    """vp_commit_public_eq_masked(point, mask) and vp_commit_public_masked(table, mask) against the oracle run on orc_beta_table(point) as the public vector, for a
    uniform point and a 0/1 corner (the table is a single 1: every slice but one is zero); the ladder above runs vp_commit_public_masked on a vector that is no
    tensor.  ms <= N, = N and > N."""
    x = pai.inputs("uniform", n)
    f = pmi.family("uniform", n, ms)
    point = np.random.default_rng(8000 + n).integers(0, P, size=(n, 2), dtype=np.uint64) if pt == "uniform" else \
        np.array([[(0x2d5a5 >> i) & 1, 0] for i in range(n)], dtype=np.uint64)
    table = np.zeros((1 << n, 2), dtype=np.uint64)
    one = np.array([1, 0], dtype=np.uint64)
    ob.lib().orc_beta_table(point.ctypes.data, n, one.ctypes.data, table.ctypes.data)
    assert table.any() and (pt == "uniform" or (table != 0).sum() == 1)
    want, opens, vals = _expected(ob, x, f, (n, "eq_" + pt, "uniform", ms, None), pub=table)
    py = _python(ob, n, f, (n, "uniform", ms, None))
    c = _ctx(vp, x)
    try:
        for form, public in (("eq", lambda cc: cc.commit_public_eq(point, f["pub_mask"])), ("table", lambda cc: cc.commit_public(table, f["pub_mask"]))):
            got, _ = _device(c, x, f, public=public)
            _compare(got, want, "n=%d ms=%d %s point, %s form" % (n, ms, pt, form))
            _check_openings(c, want, opens, vals, "n=%d ms=%d %s point, %s form" % (n, ms, pt, form), py)
    finally:
        c.close()


# ---- every phase form ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("late", [0, 2])
@pytest.mark.parametrize("n,ms,kind", [(9, 32, "edges"), (13, 64, "uniform"), (13, 1024, "edges"), (16, 512, "uniform")])
def test_every_phase_form_vs_oracle(vp, ob, n, ms, kind, late):
    """vp_fri_commit whole, vp_fri_commit for the first 1, 2 and 4 challenges (without and with the three-fold first pass) continued by vp_fri_step, and
    vp_fri_step alone; with vp_pc_hash_late 0 and 2.  Whole: the launch table shows ONE leaf-hash launch — over the n - 6 levels, or with the mode on over l, h
    and the levels, and none in the two commits.  Every form gives the oracle's bytes and openings."""
    x = pai.inputs(kind, n)
    f = pmi.family(kind, n, ms)
    st = n - 6
    want, opens, vals = _expected(ob, x, f, (n, kind, kind, ms, None))
    c = _ctx(vp, x)
    try:
        for cut in [None] + [k for k in (1, 2, 4) if k < st] + [0]:
            what = "n=%d ms=%d late=%d cut=%s" % (n, ms, late, cut)
            got, rows = _device(c, x, f, late=bool(late), cut=cut, profile=cut is None)
            _compare(got, want, what)
            if cut is None:
                leaf = [[r for r in t if r[0] == "k_leaf_hash"] for t in rows]
                if late:
                    assert [len(t) for t in leaf] == [0, 0, 1] and leaf[2][0][1] == st + 2, (what, rows)
                else:
                    assert len(leaf[2]) == 1 and leaf[2][0][1] == st, (what, rows)
            if cut in (None, 2, 0):
                _check_openings(c, want, opens[::3], vals[::3], what)
    finally:
        c.close()


# ---- openings ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,ms,kind", [(8, 64, "sparse"), (12, 64, "edges"), (13, 128, "uniform"), (15, 8192, "edges")])
def test_openings_one_by_one_and_many_vs_oracle(vp, ob, n, ms, kind):
    """vp_fri_open and vp_fri_open_many at the first leaf, the last leaf and the coset-block edges of l, h, the first two FRI levels and all 16 leaves of the last
    level: the same bytes from both calls, the oracle's 130 values, the leaf digest rebuilt from the 65 pairs with hashlib.sha3_256, and the path climbed to the
    oracle's root of that level — not the device's."""
    fam = "uniform" if kind == "sparse" else kind
    x = pai.inputs(kind, n)
    c = _ctx(vp, x)
    try:
        f, want, opens, vals = _ladder_case(c, ob, x, kind, fam, ms, openings=False)
        st = n - 6
        single = [(o, lf) for o, lf in opens if o in (0, 1, 2, 3, 1 + st)]
        assert {(0, 0), (0, (1 << (n - 2)) - 1), (1, 1), (1, 31), (1 + st, 0), (1 + st, 15)} <= set(single)
        _check_openings(c, want, opens, vals, "n=%d ms=%d" % (n, ms), _python(ob, n, f, (n, fam, ms, None)) if ms <= 256 else None, single=single)
    finally:
        c.close()


# ---- one context through a sequence ----------------------------------------------------------------------------------------------------------------------------

def test_one_context_through_bit_lengths_and_masks(vp, ob):
    """One context: masked n = 13 (ms 64), masked n = 10 (ms 32), unmasked n = 13, masked n = 13 (ms 512), masked n = 16 (ms 512) — the input layer reloaded
    in between (vp_pc_load_input).  The order-M root table, the compact root tables keyed by its address, the mask scratch and the level
    arrays are all rebuilt for the new length: each result is the oracle's."""
    seq = [(13, 64, "uniform"), (10, 32, "edges"), (13, None, "uniform"), (13, 512, "edges"), (16, 512, "uniform")]
    x0 = pai.inputs("uniform", 13)
    c = _ctx(vp, x0)
    try:
        for i, (n, ms, kind) in enumerate(seq):
            x = pai.inputs(kind, n)
            assert c.L.vp_pc_load_input(c.ctx, np.ascontiguousarray(x["values"]).ctypes.data, x["n_used"], n) == 0, c.err()
            c.n = n
            what = "step %d of the sequence (n=%d ms=%s)" % (i, n, ms)
            if ms is None:
                want = pai.split_record(pai.oracle_record(ob.lib(), x["values"], x["n_used"], x["pub"], n, x["r"]), n)
                c.commit_private(); c.commit_public(x["pub"])
                roots = c.fri_commit(x["r"])
                fin, fm = c.finals()
                root_l, root_h, inner, alls = c.state()
                got = {"root_l": root_l, "root_h": root_h, "public": inner + alls, "roots": [roots[32 * k:32 * k + 32] for k in range(n - 6)], "final": fin,
                       "final_mask": fm}
                _compare(got, dict(want, final_mask=bytes(32 * 16)), what)
            else:
                _ladder_case(c, ob, x, kind, kind, ms, openings=(n < 16))
    finally:
        c.close()


# ---- the recorded sizes ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(pmi.ARRAY_CASES))
def test_recorded_sizes_vs_oracle_fixture(vp, name):
    """n = 18 with a mask of 40000 elements (ms = 2^16, the longest the device takes: k_mask_combine with c = 16 and a 2^17-point quotient transform) and n = 20
    with 2^14 edge limbs (ms = N) under edge challenges, per call and under vp_pc_hash_late: the oracle's record is a fixture
    (tests/golden/make_pc_masked_array.py, minutes of CPU), the inputs are regenerated here and must hash to what the fixture was made from.  Openings: leaf
    digest and path against the recorded roots."""
    m = json.load(open(os.path.join(GOLDEN, "pc_masked_array.json")))[name]
    x = pmi.array_case(name)
    if x["n_used"] != m["n_used"] or pmi.array_digests(x) != {k: v for k, v in m.items() if k.endswith("_sha256") and k != "record_sha256"}:
        pytest.fail("input generator differs from the one tests/golden/%s was recorded with (no statement about the device)" % m["record"])
    n = m["n"]
    want = pmi.split_masked_record(open(os.path.join(GOLDEN, m["record"]), "rb").read(), n)
    opens = [(o, lf) for o, lf in _open_list(n) if o < 4 or o == n - 5]
    c = _ctx(vp, x)
    try:
        for late in (False, True):
            got, _ = _device(c, x, x, late=late)
            _compare(got, want, "%s late=%d" % (name, late))
            v, p, pl = c.open_many(opens)
            for i, (o, lf) in enumerate(opens):
                root = want["root_l"] if o == 0 else want["root_h"] if o == 1 else want["roots"][o - 2]
                path = [p[i, 32 * k:32 * k + 32].tobytes() for k in range(pl[i])]
                assert path[-1] == _sha3_leaf(v[i]) and _opening_ok(root, lf, v[i], path), (name, late, o, lf)
    finally:
        c.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_device_and_oracle_refuse_the_same_masks(vp, ob):
    """A mask that pads to fewer than 8 elements, to the whole slice (gap 1), one longer than a slice; a public mask longer than the padded private one; a
    non-canonical limb in either mask: VP_EINVAL from the device, -1 from the oracle's entry, and the neighbour of each is taken by both.  A mask that pads to
    2^17 at n = 19 stays VP_ELIMIT (the oracle has no such limit: a limit of the device's transforms, not of the scheme).  The context answers the oracle's
    bytes afterwards."""
    n = 10
    M = 1 << (n - 1)
    x, f = pai.inputs("uniform", n), pmi.family("uniform", n, 16)
    big = np.random.default_rng(2).integers(0, P, size=(M + 1, 2), dtype=np.uint64)
    orc = lambda pm, qm: pmi.oracle_masked_rc(ob.lib(), x["values"], x["n_used"], x["pub"], n, f["r"], pm, qm)[0]
    c = _ctx(vp, x)
    try:
        def dev(pm, qm):
            root = ctypes.create_string_buffer(32)
            pm, qm = np.ascontiguousarray(pm), np.ascontiguousarray(qm)
            rc = c.L.vp_commit_private_masked(c.ctx, pm.ctypes.data, pm.shape[0], ctypes.cast(root, ctypes.c_void_p))
            if rc == 0:
                rc = c.L.vp_commit_public_masked(c.ctx, x["pub"].ctypes.data, x["pub"].shape[0], qm.ctypes.data, qm.shape[0], c.inner.ctypes.data, c.alls.ctypes.data,
                                                 ctypes.cast(root, ctypes.c_void_p))
            return rc
        bad_pri, bad_pub = np.array(f["pri_mask"]), np.array(f["pub_mask"])
        bad_pri[3, 1] = P; bad_pub[0, 0] = P
        cases = [(big[:M // 128 + 1], big[:1], 0), (big[:M // 128], big[:1], -1), (big[:M // 4 + 1], big[:5], 0), (big[:M // 2 + 1], big[:1], -1),
                 (big[:M], big[:1], -1), (big, big[:1], -1), (f["pri_mask"], big[:16], 0), (f["pri_mask"], big[:17], -1), (bad_pri, f["pub_mask"], -1),
                 (f["pri_mask"], bad_pub, -1)]
        for i, (pm, qm, rc) in enumerate(cases):
            assert orc(pm, qm) == rc, "oracle, case %d" % i
            assert dev(pm, qm) == (0 if rc == 0 else VP_EINVAL), ("device, case %d" % i, c.err())
        want, opens, vals = _expected(ob, x, f, (n, "uniform", "uniform", 16, None))
        got, _ = _device(c, x, f)
        _compare(got, want, "after the refusals")
    finally:
        c.close()
    x19 = np.zeros((1 << 19, 2), np.uint64)
    x19[:4, 0] = (1, 2, 3, 4)
    c = Ctx(vp, x19, 19)
    try:
        root = ctypes.create_string_buffer(32)
        pm = np.ascontiguousarray(np.random.default_rng(3).integers(0, P, size=((1 << 16) + 1, 2), dtype=np.uint64))
        assert c.L.vp_commit_private_masked(c.ctx, pm.ctypes.data, pm.shape[0], ctypes.cast(root, ctypes.c_void_p)) == VP_ELIMIT and "2^16" in c.err()
        assert c.L.vp_commit_private_masked(c.ctx, pm.ctypes.data, 1 << 16, ctypes.cast(root, ctypes.c_void_p)) == 0, c.err()      # pads to 2^16: taken
    finally:
        c.close()
