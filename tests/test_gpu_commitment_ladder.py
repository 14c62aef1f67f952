"""GPU (-m gpu): the Virgo commitment on arbitrary inputs (vp_pc_load_input) against the oracle's restatement of the same calls (orc_commitment_array), at the
input bit lengths at which the device takes another path: n = 7 .. 12 (transforms of 2 .. 64 points, trees of a single launch), 14 (k_fri_fold0_vo as the
first fold of the one-pass phase), 15, 16 (k_fri_fold0_vo3<., 1>), 18 (the longest in-LDS transform) and 20 (k_fri_fold0_vo3<., VP_VO_GRP>) — with a public
vector that is no tensor, with field elements from the ends of the range and all-zero slices, with a five-wire witness, with vp_commit_public_eq against the
oracle's own eq table, with a commit phase that is part one pass and part step by step, and with the radix-4 transform pair (ntt_r8 = 0) against the real
reference's goldens.  Every comparison is byte equality; every opening is checked against the ORACLE's root of that level."""
import ctypes
import json
import os

import numpy as np
import pytest

import pc_array_inputs as pai
from conftest import GOLDEN
from test_gpu_sharded_dropin_commitment import _fri_golden, _opening_ok

pytestmark = pytest.mark.gpu
VP_EINVAL = -1


class Ctx:
    """a context that holds only an input layer (vp_pc_load_input), with the commitment calls of the C ABI"""

    def __init__(self, vp, x):
        self.L, self.n, self.ln = vp.lib_gpu(), x["n"], x["n"] - 6
        self.c = ctypes.c_void_p()
        assert self.L.vp_create_with_options(0, None, ctypes.byref(self.c)) == 0
        assert self.L.vp_pc_load_input(self.c, x["values"].ctypes.data, x["n_used"], self.n) == 0, self.err()

    def err(self):
        return (self.L.vp_last_error(self.c) or b"").decode()

    def commit_private(self):
        root = ctypes.create_string_buffer(32)
        assert self.L.vp_commit_private(self.c, ctypes.cast(root, ctypes.c_void_p)) == 0, self.err()
        return root.raw

    def _public(self, call):
        root, inner, alls = ctypes.create_string_buffer(32), np.zeros(2, np.uint64), np.zeros((65, 2), np.uint64)
        assert call(inner.ctypes.data, alls.ctypes.data, ctypes.cast(root, ctypes.c_void_p)) == 0, self.err()
        return root.raw, inner.tobytes() + alls.tobytes()

    def commit_public(self, pub):
        return self._public(lambda i, a, h: self.L.vp_commit_public(self.c, pub.ctypes.data, pub.shape[0], i, a, h))

    def commit_public_eq(self, point):
        return self._public(lambda i, a, h: self.L.vp_commit_public_eq(self.c, point.ctypes.data, point.shape[0], i, a, h))

    def fri_commit(self, r):
        r = np.ascontiguousarray(r)
        roots = ctypes.create_string_buffer(32 * r.shape[0])
        assert self.L.vp_fri_commit(self.c, r.ctypes.data, r.shape[0], ctypes.cast(roots, ctypes.c_void_p)) == 0, self.err()
        return [roots.raw[32 * k:32 * k + 32] for k in range(r.shape[0])]

    def fri_step(self, r_k):
        r_k = np.ascontiguousarray(r_k)
        root = ctypes.create_string_buffer(32)
        assert self.L.vp_fri_step(self.c, r_k.ctypes.data, ctypes.cast(root, ctypes.c_void_p)) == 0, self.err()
        return root.raw

    def fri_final_rc(self):
        fin = np.zeros((2048, 2), dtype=np.uint64)
        return self.L.vp_fri_final(self.c, fin.ctypes.data), fin.tobytes()

    def open(self, oracle, leaf):
        vals = np.zeros((130, 2), dtype=np.uint64)
        path = ctypes.create_string_buffer(32 * 40)
        k = ctypes.c_int(0)
        rc = self.L.vp_fri_open(self.c, oracle, leaf, vals.ctypes.data, ctypes.cast(path, ctypes.c_void_p), len(path), ctypes.byref(k))
        return rc, vals, [path.raw[32 * i:32 * i + 32] for i in range(k.value)]

    def close(self):
        if self.c:
            self.L.vp_destroy(self.c)
            self.c = None


_ORACLE = {}          # (n, input set or eq-point case) -> the oracle's record, computed once: the ladder, the partial phases and the openings share it


def _expected(ob, n, key, x, pub):
    if (n, key) not in _ORACLE:
        _ORACLE[(n, key)] = pai.oracle_record(ob.lib(), x["values"], x["n_used"], pub, n, x["r"])
    return pai.split_record(_ORACLE[(n, key)], n)


def _run(vp, x, public, one_pass, check_final_refused=False):
    """commit_private, `public(ctx)`, then the first `one_pass` challenges through vp_fri_commit and the rest through vp_fri_step, vp_fri_final: (the
    outputs in the record's fields, the context — still open, for the openings)"""
    cx = Ctx(vp, x)
    try:
        got = {"root_l": cx.commit_private()}
        got["root_h"], got["public"] = public(cx)
        r, ln = x["r"], cx.ln
        got["roots"] = cx.fri_commit(r[:one_pass]) if one_pass else []
        for k in range(one_pass, ln):
            if check_final_refused:
                assert cx.fri_final_rc()[0] == VP_EINVAL, "vp_fri_final answered after %d of %d steps" % (k, ln)
            got["roots"].append(cx.fri_step(r[k]))
        rc, got["final"] = cx.fri_final_rc()
        assert rc == 0, cx.err()
    except BaseException:
        cx.close()
        raise
    return got, cx


def _compare(got, want, what):
    assert got["root_l"] == want["root_l"], what + ": merkle_root_l"
    assert got["root_h"] == want["root_h"], what + ": merkle_root_h"
    assert got["public"][:16] == want["public"][:16], what + ": input_0"
    g, w = np.frombuffer(got["public"][16:], np.uint64).reshape(65, 2), np.frombuffer(want["public"][16:], np.uint64).reshape(65, 2)
    assert np.array_equal(g, w), what + ": all_sum, first at slice %d" % int(np.argmax((g != w).any(axis=1)))
    assert len(got["roots"]) == len(want["roots"])
    for k, (a, b) in enumerate(zip(got["roots"], want["roots"])):
        assert a == b, what + ": FRI root %d" % k
    assert got["final"] == want["final"], what + ": final codeword"


def _check_openings(cx, want, what):
    """l, h and every FRI level at leaf 0, the last leaf and one inside: the values and the path of the device verify against the oracle's root"""
    n, ln = cx.n, cx.ln
    for oracle in range(2 + ln):
        n_leaves = 1 << (n - 2) if oracle < 2 else 16 << (ln - 1 - (oracle - 2))
        root = want["root_l"] if oracle == 0 else want["root_h"] if oracle == 1 else want["roots"][oracle - 2]
        for leaf in (0, n_leaves - 1, n_leaves // 3 + 1):
            rc, vals, path = cx.open(oracle, leaf)
            assert rc == 0, (what, oracle, leaf, cx.err())
            assert len(path) == n_leaves.bit_length() and _opening_ok(root, leaf, vals, path), "%s: opening of oracle %d at leaf %d" % (what, oracle, leaf)
    assert cx.open(2 + ln, 0)[0] == VP_EINVAL and cx.open(0, 1 << (n - 2))[0] == VP_EINVAL


def _ladder(vp, x, want, what, stepwise):
    pub = x["pub"]
    got, cx = _run(vp, x, lambda c: c.commit_public(pub), x["n"] - 6)
    try:
        _compare(got, want, what + ", one pass")
        _check_openings(cx, want, what)
    finally:
        cx.close()
    if stepwise:
        got, cx = _run(vp, x, lambda c: c.commit_public(pub), 0)
        cx.close()
        _compare(got, want, what + ", step by step")


@pytest.mark.parametrize("n", [7, 8, 9, 10, 11, 12, 14, 15, 16])
def test_ladder_uniform_inputs_vs_oracle(vp, ob, n):
    """(a) complex uniform inputs (the last three wires unused) and a public vector that is no tensor: vp_commit_private, vp_commit_public, the FRI phase
    in one pass and step by step, vp_fri_final and the openings, against orc_commitment_array."""
    x = pai.inputs("uniform", n)
    _ladder(vp, x, _expected(ob, n, "uniform", x, x["pub"]), "uniform n=%d" % n, stepwise=True)


@pytest.mark.parametrize("n", [7, 9, 12, 15])
@pytest.mark.parametrize("kind", ["edges", "sparse"])
def test_ladder_edge_and_sparse_inputs_vs_oracle(vp, ob, kind, n):
    """(b) limbs from {0, 1, 2, p-1, p-2, (p-1)/2, 2^32-1, 2^32, 2^60} with all-zero input slices and an all-zero l.q product (the reference's shortcuts,
    poly_commit.h:89-99 and all_sum[i] = 0), and a real witness of five wires."""
    x = pai.inputs(kind, n)
    sl = 1 << (n - 6)
    if kind == "edges":
        assert not x["values"][5 * sl:6 * sl].any() and not x["values"][63 * sl:].any() and not x["pub"][7 * sl:8 * sl].any() and not x["pub"][0].any()
        assert x["values"][:5 * sl].any() and x["pub"][:7 * sl].any()
    else:
        assert x["n_used"] == 5 and x["values"][:5, 0].all() and not x["values"][:, 1].any() and not x["values"][5:].any()
    want = _expected(ob, n, kind, x, x["pub"])
    if kind == "edges":                   # the shortcuts were taken: a zero slice sums to zero
        alls = np.frombuffer(want["public"][16:], np.uint64).reshape(65, 2)
        assert not alls[5].any() and not alls[7].any() and not alls[63].any() and alls[0].any()
    _ladder(vp, x, want, "%s n=%d" % (kind, n), stepwise=False)


@pytest.mark.parametrize("one_pass", [2, 3])
@pytest.mark.parametrize("n", [15, 16])
def test_partial_one_pass_phase_then_steps_vs_oracle(vp, ob, n, one_pass):
    """(c) vp_fri_commit with fewer challenges than levels, vp_fri_step for the rest: 2 challenges run k_fri_fold0_vo at 2^9 / 2^10 points per slice, 3 run
    k_fri_fold0_vo3 and stop.  vp_fri_final refuses until the last step is done; roots, final codeword and openings are the oracle's."""
    x = pai.inputs("uniform", n)
    want = _expected(ob, n, "uniform", x, x["pub"])
    got, cx = _run(vp, x, lambda c: c.commit_public(x["pub"]), one_pass, check_final_refused=True)
    try:
        _compare(got, want, "uniform n=%d, %d steps in one pass" % (n, one_pass))
        _check_openings(cx, want, "uniform n=%d, %d steps in one pass" % (n, one_pass))
    finally:
        cx.close()


@pytest.mark.parametrize("case", ["random", "zero_coordinate", "one_coordinate"])
@pytest.mark.parametrize("n", [7, 8, 9, 10, 12])
def test_commit_public_eq_vs_oracle_on_its_own_eq_table(vp, ob, n, case):
    """(d) vp_commit_public_eq(point) against the oracle run on orc_beta_table(point) as the public vector: the public outputs and the whole FRI phase
    (the tensor forms of the first fold and of the virtual oracle) for a random point, one with a coordinate 0 and one with a coordinate 1 (pub[0] = 0)."""
    x = pai.inputs("uniform", n)
    point = np.random.default_rng(4000 + n).integers(0, pai.P61, size=(n, 2), dtype=np.uint64)
    if case == "zero_coordinate":
        point[n // 2] = 0
    if case == "one_coordinate":
        point[n - 2] = (1, 0)
    table = np.zeros((1 << n, 2), dtype=np.uint64)
    one = np.array([1, 0], dtype=np.uint64)
    ob.lib().orc_beta_table(point.ctypes.data, n, one.ctypes.data, table.ctypes.data)
    assert table.any() and (case != "one_coordinate" or not table[0].any())
    want = _expected(ob, n, "eq_" + case, x, table)
    what = "eq table of a point (%s) n=%d" % (case, n)
    got, cx = _run(vp, x, lambda c: c.commit_public_eq(point), n - 6)
    try:
        _compare(got, want, what + ", one pass")
        _check_openings(cx, want, what)
    finally:
        cx.close()
    got, cx = _run(vp, x, lambda c: c.commit_public_eq(point), 0)
    cx.close()
    _compare(got, want, what + ", step by step")


@pytest.mark.parametrize("n", [18, 20])
def test_recorded_sizes_vs_oracle_fixture(vp, n):
    """(e) the uniform set at n = 18 (the longest k_ntt_lds transform in default use) and n = 20 (k_fri_fold0_vo3<false, VP_VO_GRP>): the oracle's record
    is a fixture (tests/golden/make_pc_array.py, minutes of CPU), the inputs are regenerated here and must hash to what the fixture was made from."""
    m = json.load(open(os.path.join(GOLDEN, "pc_array.json")))["n%d" % n]
    x = pai.inputs(m["set"], n, seed=m["seed"])
    if x["n_used"] != m["n_used"] or pai.digests(x) != {k: v for k, v in m.items() if k.endswith("_sha256") and k != "record_sha256"}:
        pytest.fail("input generator differs from the one tests/golden/%s was recorded with (no statement about the device)" % m["record"])
    want = pai.split_record(open(os.path.join(GOLDEN, m["record"]), "rb").read(), n)
    _ladder(vp, x, want, "uniform n=%d" % n, stepwise=True)


@pytest.mark.parametrize("name,blocks", [("sha256_x16", 16), ("sha256_x64", 64)])
def test_radix4_transform_pair_vs_reference(vp, golden, pws_path, name, blocks):
    """(f) ntt_r8 = 0, the radix-4 kernels where the radix-8 pair runs by default.  sha256_x64 (n = 19): every transform of the commitment has 2^13 points
    (the 2^14-point inverse of the l.q product is two of them) and runs in k_ntt_lds with its largest LDS image, which no default path uses; sha256_x16 (2^11)
    stays in LDS either way.  k_ntt_split itself starts at 2^14 points: the test below and test_commitment_with_split_transforms_vs_oracle.  The real
    reference's transcript, FRI roots and final codeword."""
    c = vp.Circuit.from_pws(pws_path, blocks, seed=1)
    s = vp.Session(c, options=vp.Options(ntt_r8=0))
    try:
        gold = open(os.path.join(GOLDEN, golden[name]["transcript"]), "rb").read()
        s.set_profiling(1)
        root, _ = s.commit_private()
        kinds = {e["kernel"] for e in s.launch_stats()}
        assert "k_ntt_lds" in kinds and not any(k.startswith("k_ntt8") for k in kinds)            # the option took: no radix-8 launch, even at 2^13
        s.set_profiling(0)
        assert root == gold[:32]
        full, ok = s.prove_full(batched=True)
        assert ok
        assert full == gold
        r, roots_gold, fin_gold = _fri_golden(golden, name)
        roots, fin = s.fri_commit(r)
        assert roots == b"".join(roots_gold)
        assert np.array_equal(fin, fin_gold)
    finally:
        s.close(); c.close()


@pytest.mark.parametrize("ln", [14, 15, 16, 17])
def test_radix4_split_transforms_vs_oracle(vp, ob, monkeypatch, ln):
    """(f) k_ntt_split<1 .. 4> -> k_ntt_lds (ntt_r8 = 0) on one row of 2^ln points, every width of the register transform: the forward transform and the
    inverse against the oracle's (RS_polynomial.cpp:26-220), at 2^14 also the encoder's 32 twisted cosets.  (That the pair runs at these sizes is checked from
    the launch table in test_commitment_with_split_transforms_vs_oracle.)"""
    L, O = vp.lib_gpu(), ob.lib()
    O.orc_fft.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    O.orc_ifft.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    for k, v in vp.Options(ntt_r8=0).tuning_env().items():          # the library reads its tuning switches once, in vp_create
        monkeypatch.setenv(k, v)
    c = ctypes.c_void_p()
    assert L.vp_create_with_options(0, None, ctypes.byref(c)) == 0
    try:
        n = 1 << ln
        x = np.random.default_rng(5000 + ln).integers(0, pai.P61, size=(n, 2), dtype=np.uint64)
        for ratio, inverse in [(1, 0), (1, 1)] + ([(32, 0)] if ln == 14 else []):
            got, want = np.zeros((n * ratio, 2), dtype=np.uint64), np.zeros((n * ratio, 2), dtype=np.uint64)
            assert L.vp_test_fft(c, x.ctypes.data, n, n * ratio, inverse, got.ctypes.data) == 0
            if inverse:
                O.orc_ifft(x.ctypes.data, n, want.ctypes.data)
            else:
                O.orc_fft(x.ctypes.data, n, n * ratio, want.ctypes.data)
            assert np.array_equal(got, want), "2^%d points, %d coset(s), %s" % (ln, ratio, "inverse" if inverse else "forward")
    finally:
        L.vp_destroy(c)
