"""The masked commitment (vp_commit_private_masked / vp_commit_public_masked) on the protocol pass's fast path: the generated leaf chain with the mask
pair as its last block, the one-pass vp_fri_commit, vp_pc_hash_late, vp_commit_public_eq_masked and Session.prove_protocol(mask=...).  Every comparison is
byte equality: against the real reference's record (tests/golden/pc_masked_*.bin), against the compiler-form kernels (a context created with VP_LEAF_ASM=0),
against the per-call / per-step forms, and — independent of both — against hashlib's SHA3-256 over the opened pairs."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import pc_masked_inputs as pmi
import verifier_sums as vs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = pmi.P61
VP_EINVAL = -1


def _record(name):
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "pc_masked.json")))[name]
    rec = open(os.path.join(ROOT, "tests", "golden", meta["record"]), "rb").read()
    fri = open(os.path.join(ROOT, "tests", "golden", meta["fri"]), "rb").read()
    st = meta["fri_steps"]
    return {"root_l": rec[:32], "root_h": rec[32:64], "all_sum": rec[64:64 + 65 * 16], "openings": rec[64 + 65 * 16:],
            "r": np.frombuffer(b"".join(fri[48 * k:48 * k + 16] for k in range(st)), dtype=np.uint64).reshape(st, 2).copy(),
            "fri_roots": b"".join(fri[48 * k + 16:48 * k + 48] for k in range(st)),
            "final": fri[48 * st:48 * st + 2048 * 16], "final_mask": fri[48 * st + 2048 * 16:48 * st + 2048 * 16 + 32 * 16], "steps": st}


_CASES = {}


def _case(name):
    """inputs + golden record of a named case, computed once and left unchanged"""
    if name not in _CASES:
        _CASES[name] = (pmi.inputs(name), _record(name))
    return _CASES[name]


class Ctx:
    """A bare context of the C ABI with an input layer loaded (vp_pc_load_input) and the commitment's calls as methods that return bytes."""

    def __init__(self, vp, values, n, env=None):
        self.vp, self.L, self.n = vp, vp.lib_gpu(), n
        self.L.vp_fri_step.argtypes = [ctypes.c_void_p] * 3
        self.ctx = ctypes.c_void_p()
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            assert self.L.vp_create(0, ctypes.byref(self.ctx)) == 0
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        self.values = np.ascontiguousarray(values)
        assert self.L.vp_pc_load_input(self.ctx, self.values.ctypes.data, self.values.shape[0], n) == 0
        self.root_l, self.root_h = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
        self.inner, self.alls = np.zeros(2, np.uint64), np.zeros((65, 2), np.uint64)

    def close(self):
        if self.ctx:
            self.L.vp_destroy(self.ctx)
            self.ctx = None

    def err(self):
        return (self.L.vp_last_error(self.ctx) or b"").decode()

    def hash_late(self, on):
        """on: the mode that reaches masked commits, VP_HASH_LATE_MASKED = 2 (on = 1 keeps its meaning: masked commitments hash at once, which
        test_gpu_hash_once.py::test_masked_commitment_ignores_the_mode pins)"""
        assert self.L.vp_pc_hash_late(self.ctx, 2 if on else 0) == 0

    def profiling(self, on):
        assert self.L.vp_set_profiling(self.ctx, 1 if on else 0) == 0

    def rows(self):
        n = ctypes.c_int(0)
        self.L.vp_get_launch_stats(self.ctx, None, 0, ctypes.byref(n))
        arr = (self.vp.LaunchStat * max(1, n.value))()
        self.L.vp_get_launch_stats(self.ctx, arr, n.value, ctypes.byref(n))
        return [(self.L.vp_kernel_name(arr[i].kind).decode(), arr[i].jobs, arr[i].workgroups) for i in range(n.value)]

    def commit_private(self, mask=None):
        if mask is None:
            rc = self.L.vp_commit_private(self.ctx, ctypes.cast(self.root_l, ctypes.c_void_p))
        else:
            m = np.ascontiguousarray(mask)
            rc = self.L.vp_commit_private_masked(self.ctx, m.ctypes.data, m.shape[0], ctypes.cast(self.root_l, ctypes.c_void_p))
        assert rc == 0, self.err()

    def commit_public(self, pub, pub_mask=None, expect=0):
        pub = np.ascontiguousarray(pub)
        if pub_mask is None:
            rc = self.L.vp_commit_public(self.ctx, pub.ctypes.data, pub.shape[0], self.inner.ctypes.data, self.alls.ctypes.data, ctypes.cast(self.root_h, ctypes.c_void_p))
        else:
            q = np.ascontiguousarray(pub_mask)
            rc = self.L.vp_commit_public_masked(self.ctx, pub.ctypes.data, pub.shape[0], q.ctypes.data, q.shape[0], self.inner.ctypes.data, self.alls.ctypes.data,
                                                ctypes.cast(self.root_h, ctypes.c_void_p))
        assert rc == expect, self.err()

    def commit_public_eq(self, point, pub_mask=None, n_mask=None, expect=0):
        point = np.ascontiguousarray(point)
        if pub_mask is None:
            rc = self.L.vp_commit_public_eq(self.ctx, point.ctypes.data, point.shape[0], self.inner.ctypes.data, self.alls.ctypes.data, ctypes.cast(self.root_h, ctypes.c_void_p))
        else:
            q = np.ascontiguousarray(pub_mask)
            rc = self.L.vp_commit_public_eq_masked(self.ctx, point.ctypes.data, point.shape[0], q.ctypes.data, q.shape[0] if n_mask is None else n_mask,
                                                   self.inner.ctypes.data, self.alls.ctypes.data, ctypes.cast(self.root_h, ctypes.c_void_p))
        assert rc == expect, (rc, self.err())

    def fri_commit(self, r, steps=None):
        r = np.ascontiguousarray(r)
        steps = r.shape[0] if steps is None else steps
        roots = ctypes.create_string_buffer(32 * steps)
        rc = self.L.vp_fri_commit(self.ctx, r.ctypes.data, steps, ctypes.cast(roots, ctypes.c_void_p))
        assert rc == 0, self.err()
        return roots.raw

    def fri_step(self, r1):
        r1 = np.ascontiguousarray(r1)
        root = ctypes.create_string_buffer(32)
        rc = self.L.vp_fri_step(self.ctx, r1.ctypes.data, ctypes.cast(root, ctypes.c_void_p))
        assert rc == 0, self.err()
        return root.raw

    def finals(self):
        fin, fm = np.zeros((2048, 2), np.uint64), np.zeros((32, 2), np.uint64)
        assert self.L.vp_fri_final(self.ctx, fin.ctypes.data) == 0, self.err()
        assert self.L.vp_fri_final_mask(self.ctx, fm.ctypes.data) == 0, self.err()
        return fin.tobytes(), fm.tobytes()

    def open1(self, oracle, leaf):
        v = np.zeros((130, 2), np.uint64); path = ctypes.create_string_buffer(32 * 40); plen = ctypes.c_int(0)
        rc = self.L.vp_fri_open(self.ctx, oracle, leaf, v.ctypes.data, ctypes.cast(path, ctypes.c_void_p), len(path), ctypes.byref(plen))
        assert rc == 0, self.err()
        return v.tobytes(), path.raw[:32 * plen.value]

    def open_many(self, requests):
        rc, v, p, pl = self.vp.fri_open_many(self.ctx, requests)
        assert rc == 0, self.err()
        return v, p, pl

    def state(self):
        return self.root_l.raw, self.root_h.raw, self.inner.tobytes(), self.alls.tobytes()


def _leaves_of(n_leaves, count):
    """`count` leaves of an oracle with n_leaves = 32 x halfN leaves (thread t = b halfN + a hashes leaf 32 a + b): the first and the last, both ends of coset
    blocks, the leaves of the launch's last workgroup (b = 31, a at the end), the rest spread evenly"""
    if n_leaves <= count:
        return list(range(n_leaves))
    half = n_leaves // 32
    want = [0, n_leaves - 1, 32 * (half - 1), 1, 32 * (half - 1) + 1, 31, 32 * (half - 2) + 31, 32 * (half // 2) + 30, 32 * (half // 2 - 1) + 31, 32 * (half // 2) + 31]
    out = []
    for x in want + [(i * 2654435761) % n_leaves for i in range(1, 4 * count)]:
        if 0 <= x < n_leaves and x not in out:
            out.append(x)
        if len(out) == count:
            break
    return out


def _requests(n, steps, per_oracle):
    req = []
    for o in range(2 + steps):
        n_leaves = 1 << (n - 2) if o < 2 else 16 * ((1 << (n - 6)) >> (o - 1))
        req += [(o, lf) for lf in _leaves_of(n_leaves, per_oracle)]
    return req


def _sha3_leaf(values):
    """fri.cpp:96-124: the leaf digest from the 65 opened pairs — SHA3-256 over (pair of slice s || previous digest), the mask slice's pair last"""
    h = bytes(32)
    b = np.ascontiguousarray(values, dtype=np.uint64).tobytes()
    for s in range(65):
        h = hashlib.sha3_256(b[32 * s:32 * s + 32] + h).digest()
    return h


def _edge_mask(count, seed):
    """every limb one of 0, 1, p - 1 (the ends of the canonical range), no all-zero vector"""
    rng = np.random.default_rng(seed)
    m = np.array([0, 1, P - 1], dtype=np.uint64)[rng.integers(0, 3, size=(count, 2))]
    m[0] = (P - 1, 1)
    return m


def _uniform(count, seed):
    return np.random.default_rng(seed).integers(0, P, size=(count, 2), dtype=np.uint64)


# ---- the launch table of the one-pass masked vp_fri_commit ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["n13_m64", "n16_m100"])
def test_masked_fri_commit_is_one_pass_in_the_launch_table(vp, name):
    """Profiled, a masked vp_fri_commit shows ONE leaf-hash row over all levels, fold rows, and the Merkle rows of trees built together (the last one, the tops,
    over all n - 6 trees) — not a leaf launch and a tree chain per step.  (Before the masked branch joined the one-pass path it looped over vp_fri_step, whose
    launches are not even recorded: this test fails there.)  Roots and final codewords are the golden record's."""
    x, g = _case(name)
    c = Ctx(vp, x["values"], x["n"])
    try:
        st = g["steps"]
        c.profiling(True)
        c.commit_private(x["pri_mask"]); c.commit_public(x["pub"], x["pub_mask"])
        roots = c.fri_commit(g["r"])
        rows = c.rows()
        c.profiling(False)
        assert roots == g["fri_roots"]
        assert c.finals() == (g["final"], g["final_mask"])
        leaf = [r for r in rows if r[0] == "k_leaf_hash"]
        merkle = [r for r in rows if r[0] == "k_merkle"]
        folds = [r for r in rows if r[0] == "k_fri_fold"]
        assert len(leaf) == 1 and leaf[0][1] == st, rows                       # one launch, one entry per level
        assert merkle and merkle[-1][1] == st and merkle[0][1] > 1, rows       # rows of trees built together; the last one, the tops, covers all of them
        assert len(merkle) < st, rows                                           # (a per-step pattern has at least one row per step)
        assert len(folds) >= 1 + st, rows                                       # the slices' folds and the mask slice's (virtual oracle + one per level)
    finally:
        c.close()


# ---- vp_pc_hash_late on a masked commitment ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["n13_m64", "n16_m100"])
def test_hash_late_masked_pass_equals_the_golden_record_and_the_mode_off(vp, name):
    """vp_pc_hash_late(VP_HASH_LATE_MASKED), then vp_commit_private_masked, vp_commit_public_masked, vp_fri_commit: both commits stop behind their transforms, the FRI call hashes
    l, h and every level in ONE launch with the mask slices' pairs closing the chains.  Roots of l, h and all levels, all_sum[65], both final codewords and the
    record's openings are the real reference's; 8 openings per oracle (values and paths) equal a second context with the mode off.  An opening of l asked for
    between the private commit and the FRI call hashes l on the spot (the rule of pc_hash_outstanding) and matches too."""
    x, g = _case(name)
    n, st = x["n"], g["steps"]
    M = 1 << (n - 1)
    req = _requests(n, st, 8)
    a, b = Ctx(vp, x["values"], n), Ctx(vp, x["values"], n)
    try:
        b.commit_private(x["pri_mask"]); b.commit_public(x["pub"], x["pub_mask"])
        roots_b = b.fri_commit(g["r"])
        vb, pb, lb = b.open_many(req)
        assert b.state()[:2] == (g["root_l"], g["root_h"]) and b.state()[3] == g["all_sum"] and roots_b == g["fri_roots"]
        a.hash_late(True)
        a.profiling(True)
        leaf_rows = 0
        a.root_l.raw = b"\xee" * 32; a.root_h.raw = b"\xee" * 32
        a.commit_private(x["pri_mask"]); leaf_rows += sum(r[0] == "k_leaf_hash" for r in a.rows())
        a.commit_public(x["pub"], x["pub_mask"]); leaf_rows += sum(r[0] == "k_leaf_hash" for r in a.rows())
        assert a.root_l.raw == b"\xee" * 32 and a.root_h.raw == b"\xee" * 32      # not hashed yet: the roots come with the FRI call
        assert a.alls.tobytes() == g["all_sum"]
        roots_a = a.fri_commit(g["r"])
        rows = a.rows()
        leaf_rows += sum(r[0] == "k_leaf_hash" for r in rows)
        a.profiling(False)
        assert leaf_rows == 1 and [r[1] for r in rows if r[0] == "k_leaf_hash"] == [st + 2], rows       # one launch for the whole pass: l, h and the levels
        assert a.state() == b.state() and roots_a == roots_b
        assert a.finals() == b.finals() == (g["final"], g["final_mask"])
        va, pa, la = a.open_many(req)
        assert np.array_equal(va, vb) and np.array_equal(pa, pb) and np.array_equal(la, lb)
        at = 0                                                                    # the record's openings: 3 leaves of l, 3 of h, leaf 3 of levels 0 and 2
        for oracle, leaf in [(0, 0), (0, 5), (0, M // 2 - 1), (1, 0), (1, 5), (1, M // 2 - 1), (2, 3), (4, 3)]:
            assert a.open1(oracle, leaf)[0] == g["openings"][at:at + 130 * 16], (oracle, leaf)
            at += 130 * 16
        assert at == len(g["openings"])
        # once more on the same context, with an opening of l in between: l is hashed on the spot, h and the levels are merged
        a.root_l.raw = b"\xee" * 32
        a.commit_private(x["pri_mask"])
        assert a.root_l.raw == b"\xee" * 32
        got = a.open1(0, 5)
        assert a.root_l.raw == g["root_l"]                                       # the call that needed the tree delivered the root
        assert got == b.open1(0, 5) and got[0] == g["openings"][130 * 16:2 * 130 * 16]
        a.commit_public(x["pub"], x["pub_mask"])
        assert a.fri_commit(g["r"]) == g["fri_roots"] and a.state() == b.state()
        a.hash_late(False)
    finally:
        a.close(); b.close()


# ---- the generated chain with a mask pair, at each workgroup form -----------------------------------------------------------------------------------------

def _asm_case_inputs(n, kind):
    if kind == "golden":
        x, g = _case("n19_m3000")
        return x["values"], x["pri_mask"], x["pub_mask"], None, x["pub"], g
    vals = _uniform(1 << n, 100 + n)
    point = _uniform(n, 200 + n)
    if kind == "m5_uniform":
        return vals, _uniform(5, 300 + n), _uniform(5, 400 + n), point, None, None
    cnt = 1 << (n - 6)                                                          # a slice's message length
    return vals, _edge_mask(cnt, 500 + n), _edge_mask(cnt, 600 + n), point, None, None


@pytest.mark.parametrize("n,kind", [(18, "m5_uniform"), (18, "slice_edge"), (19, "golden"), (19, "m5_uniform"), (19, "slice_edge"), (20, "m5_uniform"), (20, "slice_edge")])
def test_asm_mask_chain_at_each_workgroup_form(vp, n, kind):
    """The generated chain with the mask pair as its last block (vp_leaf_chain_mask_asm), every form it is launched in:
         per call — the single-oracle launch: 2^17 leaves at n = 19 (512 threads + LDS blocker), 2^18 at n = 20 (1024 threads), the compiler's form at n = 18;
         vp_pc_hash_late — the merged launch: 3 x 2^16 - 16 leaves at n = 18 (512 threads), 3 x 2^17 - 16 at n = 19 and 3 x 2^18 - 16 at n = 20 (1024 threads;
         no multiple of 1024: the last workgroup's inactive tail runs and stores nothing).
    Reference: the same input on a context created with VP_LEAF_ASM=0 (the compiler-form kernels) — every root and 16 openings per oracle; at n = 19 also the
    real reference's record (n19_m3000).  Independently, for 42 leaves per run (first, last, both ends of coset blocks, the last workgroup's) the leaf digest is
    recomputed with hashlib.sha3_256 from the 65 opened pairs and compared with the path's leaf entry."""
    vals, pm, qm, point, pub, g = _asm_case_inputs(n, kind)
    st = n - 6
    r = g["r"] if g else _uniform(st, 700 + n)
    req = _requests(n, st, 16)

    def run(c, late):
        c.hash_late(late)
        c.commit_private(pm)
        if pub is not None:
            c.commit_public(pub, qm)
        else:
            c.commit_public_eq(point, qm)
        roots = c.fri_commit(r)
        c.hash_late(False)
        return c.state(), roots, c.finals()

    ref = Ctx(vp, vals, n, env={"VP_LEAF_ASM": "0"})
    try:
        want = run(ref, False)
        wv, wp, wl = ref.open_many(req)
    finally:
        ref.close()
    if g:
        assert want[0][:2] == (g["root_l"], g["root_h"]) and want[0][3] == g["all_sum"] and want[1] == g["fri_roots"] and want[2] == (g["final"], g["final_mask"])
    c = Ctx(vp, vals, n)
    try:
        for late in (False, True):
            assert run(c, late) == want, ("late" if late else "per call")
            v, p, pl = c.open_many(req)
            assert np.array_equal(v, wv) and np.array_equal(p, wp) and np.array_equal(pl, wl), late
            # 16 leaves of l and of h, 4 of the first two FRI levels (later entries of the merged launch), both ends of the single-value last level
            pick = {(o, lf) for o in (0, 1) for lf in _leaves_of(1 << (n - 2), 16)} | {(o, lf) for o in (2, 3) for lf in _leaves_of(16 * ((1 << (n - 6)) >> (o - 1)), 4)}
            pick |= {(2 + st - 1, 0), (2 + st - 1, 15)}
            checked = 0
            for i, (o, lf) in enumerate(req):
                if (o, lf) in pick:
                    assert p[i, 32 * (pl[i] - 1):32 * pl[i]].tobytes() == _sha3_leaf(v[i]), (late, o, lf)
                    checked += 1
            assert checked == len(pick) == 42
    finally:
        c.close()


# ---- partial phases --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,steps", [("n16_m100", 2), ("n16_m100", 4), ("n13_m5", 7)])
def test_partial_masked_fri_commit_then_steps(vp, name, steps):
    """vp_fri_commit with n_steps < n - 6 on a masked commitment (2 steps: no three-fold first pass; 4: with it), continued with vp_fri_step to the end, and with
    n_steps = n - 6 at n = 13: the golden record's roots and final codewords in each case."""
    x, g = _case(name)
    c = Ctx(vp, x["values"], x["n"])
    try:
        st = g["steps"]
        c.commit_private(x["pri_mask"]); c.commit_public(x["pub"], x["pub_mask"])
        roots = c.fri_commit(g["r"][:steps], steps)
        assert roots == g["fri_roots"][:32 * steps]
        for k in range(steps, st):
            assert c.fri_step(g["r"][k]) == g["fri_roots"][32 * k:32 * k + 32], k
        assert c.finals() == (g["final"], g["final_mask"])
        assert c.open1(2, 3)[0] == g["openings"][6 * 130 * 16:7 * 130 * 16]
    finally:
        c.close()


# ---- state -----------------------------------------------------------------------------------------------------------------------------------------------

def test_unmasked_masked_unmasked_on_one_context(vp):
    """One context: an unmasked commitment (n13_zero), a masked one (n13_m5, under vp_pc_hash_late so that the pc_unhashed bookkeeping is in play), an unmasked one
    again — each byte-equal to a fresh context's and to the golden record (stale mask buffers, a mask pointer left in the leaf launch, ...)."""
    xz, gz = _case("n13_zero")
    xm, gm = _case("n13_m5")

    def unmasked(c, late):
        c.hash_late(late)
        c.commit_private(); c.commit_public(xz["pub"])
        roots = c.fri_commit(gz["r"])
        c.hash_late(False)
        return c.state(), roots, c.finals(), c.open1(0, 5), c.open1(3, 1)

    def masked(c, late):
        c.hash_late(late)
        c.commit_private(xm["pri_mask"]); c.commit_public(xm["pub"], xm["pub_mask"])
        roots = c.fri_commit(gm["r"])
        c.hash_late(False)
        return c.state(), roots, c.finals(), c.open1(0, 5), c.open1(3, 1)

    assert np.array_equal(xz["values"], pmi.inputs("n13_zero")["values"])
    fresh = []
    for fn, x in ((unmasked, xz), (masked, xm)):
        f = Ctx(vp, x["values"], 13)
        try:
            fresh.append(fn(f, False))
        finally:
            f.close()
    for g, w in ((gz, fresh[0]), (gm, fresh[1])):
        assert w[0][:2] == (g["root_l"], g["root_h"]) and w[0][3] == g["all_sum"] and w[1] == g["fri_roots"] and w[2] == (g["final"], g["final_mask"])
    c = Ctx(vp, xz["values"], 13)
    try:
        for late in (False, True):
            assert unmasked(c, late) == fresh[0]
            assert c.L.vp_pc_load_input(c.ctx, np.ascontiguousarray(xm["values"]).ctypes.data, 1 << 13, 13) == 0
            assert masked(c, late) == fresh[1]
            assert c.L.vp_pc_load_input(c.ctx, np.ascontiguousarray(xz["values"]).ctypes.data, 1 << 13, 13) == 0
            assert unmasked(c, late) == fresh[0]
    finally:
        c.close()


# ---- vp_commit_public_eq_masked ----------------------------------------------------------------------------------------------------------------------------

def _eq_table(point):
    t = vs.eq_table([(int(a), int(b)) for a, b in point])
    return np.array(t, dtype=np.uint64).reshape(-1, 2)


_EQ = {}


def _eq_case(n, pt):
    """values, point and its eq table in Python integers — built once per (n, point kind)"""
    if (n, pt) not in _EQ:
        point = _uniform(n, 800 + n) if pt == "uniform" else np.array([[(0x5a5a5 >> i) & 1, 0] for i in range(n)], dtype=np.uint64)
        _EQ[(n, pt)] = (_uniform(1 << n, 900 + n), point, _eq_table(point))
    return _EQ[(n, pt)]


@pytest.mark.parametrize("pt", ["uniform", "corner"])
@pytest.mark.parametrize("m", [5, 64, 300])
@pytest.mark.parametrize("n", [13, 16])
def test_commit_public_eq_masked_equals_commit_public_masked_on_the_table(vp, n, m, pt):
    """vp_commit_public_eq_masked(point, mask) against vp_commit_public_masked fed eq(point, .) built in Python integers: input_0, all_sum[65], root_h, 8 openings of
    h and the FRI roots / final codewords behind it.  n = 13 (odd: uneven half tables) and 16; masks of 5, 64 and 300 elements (300 > 2^7, a slice's message at
    n = 13); a uniform point and a 0/1 corner (the table is one 1: its slice-0 corner is zero, so the one-slice encoding does not apply)."""
    vals, point, table = _eq_case(n, pt)
    pm, qm = _uniform(m, 1000 + m), _uniform(m, 1100 + m)
    r = _uniform(n - 6, 1200 + n)
    req = [(1, lf) for lf in _leaves_of(1 << (n - 2), 8)]
    c = Ctx(vp, vals, n)
    try:
        c.commit_private(pm); c.commit_public(table, qm)
        want = (c.state(), c.fri_commit(r), c.finals(), [x.tobytes() for x in c.open_many(req)])
        c.root_h.raw = bytes(32); c.inner[:] = 0; c.alls[:] = 0
        c.commit_private(pm); c.commit_public_eq(point, qm)
        got = (c.state(), c.fri_commit(r), c.finals(), [x.tobytes() for x in c.open_many(req)])
        assert got == want
    finally:
        c.close()


def test_commit_public_eq_masked_refusals_leave_the_context_usable(vp):
    """No masked private commitment; a public mask longer than the padded private one; a non-canonical coordinate: VP_EINVAL each, no output written, and the
    next valid call gives the bytes of a context that never saw the refusals.  vp_commit_public_eq keeps refusing a masked commitment."""
    n = 13
    vals, point, table = _eq_case(n, "uniform")
    pm, qm = _uniform(5, 1300), _uniform(9, 1301)                              # 5 elements pad to 8
    r = _uniform(n - 6, 1302)
    f = Ctx(vp, vals, n)
    try:
        f.commit_private(pm); f.commit_public_eq(point, qm[:5])
        want = (f.state(), f.fri_commit(r), f.finals())
    finally:
        f.close()
    c = Ctx(vp, vals, n)
    try:
        untouched = (bytes(32), bytes(16), bytes(65 * 16))
        c.commit_private()
        c.commit_public_eq(point, qm[:5], expect=VP_EINVAL)                     # no masked private commitment
        assert "vp_commit_private_masked first" in c.err() and c.state()[1:] == untouched
        c.commit_private(pm)
        c.commit_public_eq(point, qm, expect=VP_EINVAL)                         # 9 > padded length 8
        assert "longer than" in c.err() and c.state()[1:] == untouched
        bad = point.copy(); bad[n - 1, 1] = P
        c.commit_public_eq(bad, qm[:5], expect=VP_EINVAL)
        assert "non-canonical" in c.err() and c.state()[1:] == untouched
        c.commit_public_eq(point[:n - 1], qm[:5], expect=VP_EINVAL)             # wrong number of coordinates
        c.commit_public_eq(point, expect=VP_EINVAL)                             # the unmasked call on a masked commitment
        assert c.state()[1:] == untouched
        c.commit_public_eq(point, qm[:5])
        assert (c.state(), c.fri_commit(r), c.finals()) == want
    finally:
        c.close()


# ---- the protocol pass -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["sha256_x1", "randomize_8_12"])
def test_prove_protocol_with_masks_in_every_form(vp, pws_path, which):
    """Session.prove_protocol(mask=, pub_mask=) synchronous, deferred and hash_per_call: the same bytes (transcript, FRI roots, final codeword, the mask slice's
    final codeword), equal to the call sequence commit_private(mask) -> prove_gkr -> commit_public_eq(point, pub_mask) -> fri_commit(batched=False) on a second
    session with the same tape; fft_gkr's messages do not depend on the mask.  A zero mask is today's prove_protocol(); queue_next with a mask is refused."""
    make = (lambda: vp.Circuit.from_pws(pws_path, 1, seed=1)) if which == "sha256_x1" else (lambda: vp.Circuit.randomize(8, 12, seed=7))
    c = make()
    n = c.layer_bitlen(0)
    mask, pub_mask = _uniform(5, 1400 + n), _uniform(7, 1500 + n)
    s = vp.Session(c)
    s.draw_protocol_tape()
    plain = s.prove_protocol()
    fft_plain = s.last_fft_gkr()
    zero = s.prove_protocol(mask=np.zeros((5, 2), np.uint64), pub_mask=pub_mask)
    assert zero[0] == plain[0] and zero[1] == plain[1] and np.array_equal(zero[2], plain[2])
    assert not zero[4].any()
    runs = [s.prove_protocol(mask=mask, pub_mask=pub_mask, **kw) for kw in ({}, {"deferred": True}, {"hash_per_call": True}, {"deferred": True, "hash_per_call": True})]
    assert s.last_fft_gkr() == fft_plain
    point = s.last_point()
    _, _, r = s.last_fri()
    for t in runs[1:]:
        assert t[0] == runs[0][0] and t[1] == runs[0][1] and np.array_equal(t[2], runs[0][2]) and np.array_equal(t[4], runs[0][4])
    assert runs[0][0] != plain[0] and runs[0][4].any()
    with pytest.raises(RuntimeError, match="QUEUE_NEXT"):
        s.prove_protocol(mask=mask, pub_mask=pub_mask, queue_next=True)
    after = s.prove_protocol()                                                   # the session is back on the zero mask
    assert after[0] == plain[0] and after[1] == plain[1] and np.array_equal(after[2], plain[2])
    # the same thing call by call on a second session
    s2 = vp.Session(c)
    s2.draw_protocol_tape()
    root_l, _ = s2.commit_private(mask)
    gkr, _ = s2.prove_gkr()
    root_h, inner, all_sum, _ = s2.commit_public_eq(point, pub_mask)
    roots, fin = s2.fri_commit(r, batched=False)
    fm = np.zeros((32, 2), np.uint64)
    assert vp.lib_gpu().vp_fri_final_mask(s2.gpu_ctx(), fm.ctypes.data) == 0
    assert root_l + gkr + root_h + inner + all_sum == runs[0][0]
    assert roots == runs[0][1] and np.array_equal(fin, runs[0][2]) and np.array_equal(fm, runs[0][4])
    s.close(); s2.close(); c.close()
