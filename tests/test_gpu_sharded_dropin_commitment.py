"""GPU (-m gpu): the drop-in state machine on a commitment sharded over ranks (include/vpgpu.h: vp_pc_set_shard) — vp_fri_step, vp_commit_public_eq and
vp_fri_query on a shard, and a Session whose commitment runs on all its ranks.  The ranks are contexts on one GPU, the collectives between them are
done by vp_shard_exchange_local.  Expected values: the real reference's goldens (tests/golden) and, at the small shapes of the level cut, the same
calls on an unsharded context."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
P = (1 << 61) - 1
VP_EINVAL, VP_EXCHANGE = -1, 1
TAIL = 32 + 16 + 65 * 16                 # merkle_root_h | input_0 | all_sum[65] at the end of the golden transcript


def _fri_golden(golden, name):
    g = golden[name]
    fri = open(os.path.join(GOLDEN, g["fri"]), "rb").read()
    st = g["fri_steps"]
    rec = np.frombuffer(fri[: 48 * st], dtype=np.uint64).reshape(st, 6)
    return np.ascontiguousarray(rec[:, :2]), [rec[i, 2:].tobytes() for i in range(st)], np.frombuffer(fri[48 * st: 48 * st + 2048 * 16], dtype=np.uint64).reshape(2048, 2)


def _opening_ok(root, leaf, vals, path):
    """the verifier's opening check (lib/virgo/src/vpd_verifier.cpp:9-40): the leaf chains 65 SHA3-256 over (value pair || digest), then the path"""
    h = bytes(32)
    for k in range(65):
        h = hashlib.sha3_256(vals[2 * k].tobytes() + vals[2 * k + 1].tobytes() + h).digest()
    depth = len(path) - 1
    if h != path[depth]:
        return False
    pos = leaf
    for k in range(depth):
        h = hashlib.sha3_256((path[k] + h) if (pos & 1) else (h + path[k])).digest()
        pos >>= 1
    return h == root


_CASES = {}


@pytest.fixture(scope="module")
def case(vp, golden, pws_path):
    """name -> the witness, opening point and eq table of the unsharded proof of a golden circuit, made once"""
    def get(name):
        if name not in _CASES:
            blocks = {"sha256_x1": 1, "sha256_x16": 16}[name]
            gold = open(os.path.join(GOLDEN, golden[name]["transcript"]), "rb").read()
            c = vp.Circuit.from_pws(pws_path, blocks, seed=1)
            s = vp.Session(c)
            full, ok = s.prove_full(batched=True)
            assert ok and full == gold
            point = s.last_point()
            d = {"n": c.layer_bitlen(0), "inputs": np.ascontiguousarray(s.layer_values(0), dtype=np.uint64), "point": point,
                 "pub": np.ascontiguousarray(s.eq_table(point), dtype=np.uint64), "gold": gold, "fri": _fri_golden(golden, name)}
            for a in ("inputs", "point", "pub"):
                d[a].setflags(write=False)
            s.close(); c.close()
            _CASES[name] = d
        return _CASES[name]
    return get


class Ranks:
    """`world` contexts of one process holding the same input layer; world > 1: the commitment sharded over them"""

    def __init__(self, vp, inputs, n, world, options=None):
        self.vp, self.L, self.world, self.n = vp, vp.lib_gpu(), world, n
        self.ctx = []
        for r in range(world):
            c = ctypes.c_void_p()
            assert self.L.vp_create_with_options(0, ctypes.byref(options) if options is not None else None, ctypes.byref(c)) == 0
            self.ctx.append(c)
            assert self.L.vp_pc_load_input(c, inputs.ctypes.data, inputs.shape[0], n) == 0, self.err(r)
            assert self.L.vp_pc_set_shard(c, r, world) == 0, self.err(r)
        self.arr = (ctypes.c_void_p * world)(*[c.value for c in self.ctx])

    def err(self, r):
        return (self.L.vp_last_error(self.ctx[r]) or b"").decode()

    def run(self, call, what):
        """call(rank) on every rank until all return VP_OK, exchanging whenever all stop at a collective; returns the number of exchanges"""
        nx = 0
        while True:
            rcs = [call(r) for r in range(self.world)]
            if all(rc == 0 for rc in rcs):
                return nx
            assert all(rc == VP_EXCHANGE for rc in rcs), (what, rcs, [self.err(r) for r in range(self.world)])
            assert self.L.vp_shard_exchange_local(self.arr, self.world) == 0, self.err(0)
            nx += 1
            assert nx <= 4, what

    def same(self, outs):
        for o in outs[1:]:
            assert o == outs[0], "the ranks disagree"
        return outs[0]

    def commit_private(self):
        roots = [ctypes.create_string_buffer(32) for _ in self.ctx]
        self.run(lambda r: self.L.vp_commit_private(self.ctx[r], ctypes.cast(roots[r], ctypes.c_void_p)), "vp_commit_private")
        return self.same([x.raw for x in roots])

    def _public(self, call, what):
        roots = [ctypes.create_string_buffer(32) for _ in self.ctx]
        inner = [np.zeros(2, np.uint64) for _ in self.ctx]
        alls = [np.zeros((65, 2), np.uint64) for _ in self.ctx]
        self.run(lambda r: call(r, inner[r].ctypes.data, alls[r].ctypes.data, ctypes.cast(roots[r], ctypes.c_void_p)), what)
        return self.same([roots[r].raw + inner[r].tobytes() + alls[r].tobytes() for r in range(self.world)])

    def commit_public(self, pub):
        return self._public(lambda r, i, a, h: self.L.vp_commit_public(self.ctx[r], pub.ctypes.data, pub.shape[0], i, a, h), "vp_commit_public")

    def commit_public_eq(self, point):
        return self._public(lambda r, i, a, h: self.L.vp_commit_public_eq(self.ctx[r], point.ctypes.data, point.shape[0], i, a, h), "vp_commit_public_eq")

    def step(self, r_k):
        """one vp_fri_step on every rank: (root, exchanges it stopped at)"""
        r_k = np.ascontiguousarray(r_k, dtype=np.uint64)
        roots = [ctypes.create_string_buffer(32) for _ in self.ctx]
        nx = self.run(lambda r: self.L.vp_fri_step(self.ctx[r], r_k.ctypes.data, ctypes.cast(roots[r], ctypes.c_void_p)), "vp_fri_step")
        return self.same([x.raw for x in roots]), nx

    def step_rc(self, r_k):
        r_k = np.ascontiguousarray(r_k, dtype=np.uint64)
        root = ctypes.create_string_buffer(32)
        return [self.L.vp_fri_step(c, r_k.ctypes.data, ctypes.cast(root, ctypes.c_void_p)) for c in self.ctx]

    def fri_commit_rc(self, r):
        r = np.ascontiguousarray(r, dtype=np.uint64)
        roots = ctypes.create_string_buffer(32 * r.shape[0])
        return [self.L.vp_fri_commit(c, r.ctypes.data, r.shape[0], ctypes.cast(roots, ctypes.c_void_p)) for c in self.ctx]

    def fri_commit(self, r):
        r = np.ascontiguousarray(r, dtype=np.uint64)
        roots = [ctypes.create_string_buffer(32 * r.shape[0]) for _ in self.ctx]
        self.run(lambda k: self.L.vp_fri_commit(self.ctx[k], r.ctypes.data, r.shape[0], ctypes.cast(roots[k], ctypes.c_void_p)), "vp_fri_commit")
        return self.same([x.raw for x in roots])

    def final(self):
        fins = []
        for r, c in enumerate(self.ctx):
            fin = np.zeros((2048, 2), dtype=np.uint64)
            assert self.L.vp_fri_final(c, fin.ctypes.data) == 0, self.err(r)
            fins.append(fin.tobytes())
        return np.frombuffer(self.same(fins), dtype=np.uint64).reshape(2048, 2)

    def open(self, oracle, leaf, rank):
        vals = np.zeros((130, 2), dtype=np.uint64)
        path = ctypes.create_string_buffer(32 * 40)
        k = ctypes.c_int(0)
        rc = self.L.vp_fri_open(self.ctx[rank], oracle, leaf, vals.ctypes.data, ctypes.cast(path, ctypes.c_void_p), len(path), ctypes.byref(k))
        return rc, vals, [path.raw[32 * i:32 * i + 32] for i in range(k.value)]

    def pending(self):
        out = []
        for c in self.ctx:
            k = ctypes.c_int(-1)
            assert self.L.vp_shard_pending(c, ctypes.byref(k)) == 0
            out.append(k.value)
        return out

    def launch_stats(self, r):
        k = ctypes.c_int(0)
        self.L.vp_get_launch_stats(self.ctx[r], None, 0, ctypes.byref(k))
        arr = (self.vp.LaunchStat * max(1, k.value))()
        self.L.vp_get_launch_stats(self.ctx[r], arr, k.value, ctypes.byref(k))
        return [(self.L.vp_kernel_name(arr[i].kind).decode(), int(arr[i].bytes), int(arr[i].work)) for i in range(k.value)]

    def query(self, leaf0, rank, fill):
        """vp_fri_query of one rank into a buffer pre-filled with `fill`: (answer size it reports, the buffer)"""
        leaf0 = np.ascontiguousarray(leaf0, dtype=np.uint64)
        cap = ctypes.c_uint64(0)
        assert self.L.vp_fri_query_bytes(self.ctx[rank], leaf0.shape[0], ctypes.byref(cap)) == 0, self.err(rank)
        out = np.full(cap.value, fill, dtype=np.uint8)
        k = ctypes.c_uint64(0)
        assert self.L.vp_fri_query(self.ctx[rank], leaf0.shape[0], leaf0.ctypes.data, out.ctypes.data, cap.value, ctypes.byref(k)) == 0, self.err(rank)
        assert k.value == cap.value
        return cap.value, out

    def close(self):
        for c in self.ctx:
            self.L.vp_destroy(c)
        self.ctx = []


def _committed(vp, d, world, options=None):
    """ranks with commit_private and commit_public of the protocol's own public vector done, checked against the golden transcript"""
    rk = Ranks(vp, d["inputs"], d["n"], world, options)
    assert rk.commit_private() == d["gold"][:32]
    assert rk.commit_public(d["pub"]) == d["gold"][-TAIL:]
    return rk


def _check_openings(rk, d, roots):
    """owners' openings of l, h, level 0, the last locally hashed level, the first replicated level and the last level verify; a non-owner answers nothing"""
    n, W = d["n"], rk.world
    st, lw = n - 6, rk.world.bit_length() - 1
    gold = d["gold"]
    for oracle, root, n_leaves in [(0, gold[:32], 1 << (n - 2)), (1, gold[-TAIL:-TAIL + 32], 1 << (n - 2)), (2, roots[0], 1 << (n - 3)),
                                   (2 + st - lw - 2, roots[st - lw - 2], 16 << (lw + 1)), (2 + st - lw - 1, roots[st - lw - 1], 16 << lw),
                                   (2 + st - 1, roots[st - 1], 16)]:
        replicated = oracle >= 2 + st - lw - 1
        for leaf in sorted({0, 33 % n_leaves, n_leaves // 2 + 5 if n_leaves > 16 else 3, n_leaves - 1}):
            owner = 0 if replicated else (leaf >> 5) % W
            assert rk.L.vp_pc_shard_owner(rk.ctx[0], oracle, leaf) == (-1 if replicated else owner)
            rc, vals, path = rk.open(oracle, leaf, owner)
            assert rc == 0, (oracle, leaf, rk.err(owner))
            assert _opening_ok(root, leaf, vals, path), "world %d oracle %d leaf %d: opening does not verify" % (W, oracle, leaf)
            if not replicated:
                assert rk.open(oracle, leaf, (owner + 1) % W)[0] == VP_EINVAL, "a rank that does not own the leaf answered"


@pytest.mark.parametrize("name,world", [("sha256_x1", 2), ("sha256_x1", 4), ("sha256_x1", 8), ("sha256_x16", 8)])
def test_stepwise_fri_matches_reference(vp, case, name, world):
    """n - 6 vp_fri_step calls on a sharded commitment: every root is the real reference's on every rank, so is the final codeword, and owners' openings verify."""
    d = case(name)
    r, roots_gold, fin_gold = d["fri"]
    rk = _committed(vp, d, world)
    for k in range(r.shape[0]):
        root, _ = rk.step(r[k])
        assert root == roots_gold[k], "world %d step %d" % (world, k)
    assert np.array_equal(rk.final(), fin_gold)
    _check_openings(rk, d, roots_gold)
    rk.close()


def _check_openings_at_cut(rk, n, roots):
    """every oracle (l, h, each FRI level; roots: the unsharded run's): leaf 0, one in the middle and the last verify on the owning rank (rank 0 for a
    replicated level), and a rank that does not own the leaf answers VP_EINVAL"""
    W, st = rk.world, n - 6
    lw = W.bit_length() - 1
    for oracle in range(2 + st):
        n_leaves = 1 << (n - 2) if oracle < 2 else 1 << (n - 3 - (oracle - 2))
        replicated = oracle >= 2 and oracle - 2 >= st - lw - 1
        for leaf in sorted({0, n_leaves // 2 + min(33, n_leaves // 4), n_leaves - 1}):
            owner = 0 if replicated else (leaf >> 5) % W
            assert rk.L.vp_pc_shard_owner(rk.ctx[0], oracle, leaf) == (-1 if replicated else owner)
            rc, vals, path = rk.open(oracle, leaf, owner)
            assert rc == 0, (oracle, leaf, rk.err(owner))
            assert _opening_ok(roots[oracle], leaf, vals, path), "n %d world %d oracle %d leaf %d: opening does not verify" % (n, W, oracle, leaf)
            if not replicated:
                assert rk.open(oracle, leaf, (owner + 1) % W)[0] == VP_EINVAL, "a rank that does not own the leaf answered"


@pytest.mark.parametrize("n,world", [(8, 2), (9, 2), (9, 4), (10, 4)])
def test_level_cut_edges_against_unsharded(vp, n, world):
    """The smallest shapes of the level cut — one local step and no locally hashed level (n = 8, W = 2), one locally hashed level with a single
    level-5 node per rank (n = 9, W = 2), and their W = 4 neighbours — with complex inputs and a public vector that is no tensor: the same calls on
    an unsharded context give the expected bytes.  Every oracle of the sharded ranks then opens against the unsharded roots, after the step-wise phase
    and again after the one-pass vp_fri_commit on the same ranks, whose roots are the step-wise ones."""
    rng = np.random.default_rng(1000 * n + world)
    inputs = rng.integers(0, P, size=((1 << n) - 3, 2), dtype=np.uint64)
    pub = rng.integers(0, P, size=(1 << n, 2), dtype=np.uint64)
    r = rng.integers(0, P, size=(n - 6, 2), dtype=np.uint64)
    got = []
    for w in (1, world):
        rk = Ranks(vp, inputs, n, w)
        out = [rk.commit_private(), rk.commit_public(pub)]
        out += [rk.step(r[k])[0] for k in range(n - 6)]
        out.append(rk.final().tobytes())
        assert rk.step_rc(r[0]) == [VP_EINVAL] * w                    # step n - 6 + 1
        got.append(out)
        if w == 1:
            rk.close()
    names = ["root_l", "root_h | input_0 | all_sum"] + ["root of step %d" % k for k in range(n - 6)] + ["final codeword"]
    for what, a, b in zip(names, got[0], got[1]):
        assert a == b, what
    roots = [got[0][0], got[0][1][:32]] + got[0][2:2 + n - 6]        # per oracle, of the unsharded run
    _check_openings_at_cut(rk, n, roots)
    assert rk.commit_public(pub) == got[0][1]
    one_pass = rk.fri_commit(r)
    assert [one_pass[32 * k:32 * k + 32] for k in range(n - 6)] == got[1][2:2 + n - 6], "one-pass roots differ from the step-wise ones"
    assert rk.final().tobytes() == got[0][-1]
    _check_openings_at_cut(rk, n, roots)
    rk.close()


def test_collective_count_and_repeat_rule(vp, case):
    """W = 4 at n = 13: n_local = 5, so step 0 stops twice (the virtual oracle's all-to-all, its all-gather), steps 1 .. 4 once, steps 5 and 6 never:
    1 + n_local collectives.  A call repeated before the exchange returns VP_EXCHANGE and changes neither the pending collective nor the root."""
    d = case("sha256_x1")
    r, roots_gold, fin_gold = d["fri"]
    rk = _committed(vp, d, 4)
    n_local = (d["n"] - 6) - 2
    assert n_local == 5
    stops = []
    for k in range(r.shape[0]):
        if k == 1:                                                     # the repeat rule, at a step with one collective
            assert rk.step_rc(r[k]) == [VP_EXCHANGE] * 4 and rk.pending() == [1] * 4
            assert rk.step_rc(r[k]) == [VP_EXCHANGE] * 4 and rk.pending() == [1] * 4
            assert rk.L.vp_shard_exchange_local(rk.arr, 4) == 0 and rk.pending() == [0] * 4
            root, nx = rk.step(r[k])
            nx += 1
        else:
            root, nx = rk.step(r[k])
        assert root == roots_gold[k]
        stops.append(nx)
    assert stops == [2] + [1] * (n_local - 1) + [0] * 2 and sum(stops) == 1 + n_local
    assert np.array_equal(rk.final(), fin_gold)
    rk.close()


def test_ordering_refusals(vp, case):
    """vp_fri_commit after a step, a step after vp_fri_commit, an eighth step at n = 13 and a level not yet committed are VP_EINVAL; the phase then
    finishes with the reference's roots all the same."""
    d = case("sha256_x1")
    r, roots_gold, fin_gold = d["fri"]
    rk = _committed(vp, d, 2)
    assert rk.open(2, 0, 0)[0] == VP_EINVAL                            # no level committed yet
    assert rk.step(r[0])[0] == roots_gold[0]
    assert rk.fri_commit_rc(r) == [VP_EINVAL] * 2                      # vp_fri_commit after a step
    assert rk.open(3, 0, 0)[0] == VP_EINVAL                            # level 1: not yet
    rc, vals, path = rk.open(2, 0, 0)                                  # level 0: as soon as its step has returned
    assert rc == 0 and _opening_ok(roots_gold[0], 0, vals, path)
    for k in range(1, r.shape[0]):
        assert rk.step(r[k])[0] == roots_gold[k]
    assert rk.step_rc(r[0]) == [VP_EINVAL] * 2                         # an eighth step
    assert np.array_equal(rk.final(), fin_gold)
    _check_openings(rk, d, roots_gold)
    assert rk.commit_public(d["pub"]) == d["gold"][-TAIL:]             # a fresh public vector: the one-pass form, then no step
    assert rk.fri_commit(r) == b"".join(roots_gold)
    assert rk.step_rc(r[0]) == [VP_EINVAL] * 2
    assert np.array_equal(rk.final(), fin_gold)
    size = ctypes.c_uint64(0)                                          # the one-pass pattern keeps its rule: its caller merges vp_fri_open_many
    assert rk.L.vp_fri_query_bytes(rk.ctx[0], 3, ctypes.byref(size)) == VP_EINVAL
    rk.close()


@pytest.mark.parametrize("tensor", [1, 0])
@pytest.mark.parametrize("name,world", [("sha256_x1", 2), ("sha256_x1", 8), ("sha256_x16", 2), ("sha256_x16", 8)])
def test_sharded_eq_point(vp, case, name, world, tensor):
    """vp_commit_public_eq on a shard: the point in, the reference's merkle_root_h | input_0 | all_sum out on every rank, with and without the
    one-slice encoding, and no launch that moves a whole public vector."""
    d = case(name)
    n = d["n"]
    rk = Ranks(vp, d["inputs"], n, world, vp.Options(pc_tensor_pub=tensor))
    assert rk.commit_private() == d["gold"][:32]
    for c in rk.ctx:
        assert rk.L.vp_set_profiling(c, 1) == 0
    assert rk.commit_public_eq(d["point"]) == d["gold"][-TAIL:]
    # the pointwise launches of a rank, in order, as (bytes, work): the inner product against the half tables over its used share of V_0, its range of the
    # table (without the one-slice encoding only), the products and the quotient of its S slices: the rows the unsharded path records for these launches
    N, S, size = 1 << (n - 6), 64 // world, d["inputs"].shape[0]
    for q in range(world):
        used = min(max(size - q * S * N, 0), S * N)
        want = [(16 * used, used)] + ([] if tensor else [(16 * S * N, S * N)]) + [(96 * S * N, 2 * S * N), (48 * S * N, 2 * S * N)]
        assert [(b, w) for k, b, w in rk.launch_stats(q) if k == "k_pc_pointwise"] == want, "rank %d" % q
    # the FRI phase goes on from it like from vp_commit_public
    r, roots_gold, _ = d["fri"]
    assert rk.step(r[0])[0] == roots_gold[0]
    # refusals: a non-canonical coordinate, a short point, a mask
    out = [np.zeros(2, np.uint64), np.zeros((65, 2), np.uint64), ctypes.create_string_buffer(32)]
    bad = d["point"].copy(); bad[0, 0] = P
    for pt in (bad, np.ascontiguousarray(d["point"][:-1])):
        assert rk.L.vp_commit_public_eq(rk.ctx[0], pt.ctypes.data, pt.shape[0], out[0].ctypes.data, out[1].ctypes.data, ctypes.cast(out[2], ctypes.c_void_p)) == VP_EINVAL
    mask = np.random.default_rng(5).integers(1, P, size=(8, 2), dtype=np.uint64)
    assert rk.L.vp_commit_private_masked(rk.ctx[0], mask.ctypes.data, mask.shape[0], ctypes.cast(out[2], ctypes.c_void_p)) == VP_EINVAL
    rk.close()


def test_sharded_query_layout(vp, case):
    """33 repetitions from fixed positions, W = 4: every rank reports the full size, writes only the openings it owns, and the ranks' buffers merged
    are the unsharded context's answer on the same commitment, byte for byte."""
    d = case("sha256_x1")
    n = d["n"]
    r, roots_gold, _ = d["fri"]
    leaf0 = np.random.default_rng(33).integers(0, 1 << (n - 2), size=33, dtype=np.uint64)
    answers = []
    for w in (1, 4):
        rk = _committed(vp, d, w)
        for k in range(r.shape[0]):
            assert rk.step(r[k])[0] == roots_gold[k]
        per_rank = []
        for q in range(w):
            size, a = rk.query(leaf0, q, 0x00)
            _, b = rk.query(leaf0, q, 0xFF)
            per_rank.append((size, a, a == b))                        # what both runs agree on is what the rank wrote
        rk.close()
        answers.append(per_rank)
    (size1, whole, wrote1), = answers[0]
    assert wrote1.all() and size1 == 33 * sum(2080 + 32 * k for k in [n - 1, n - 1] + [n - 2 - j for j in range(n - 6)])
    merged = np.zeros(size1, dtype=np.uint8)
    covered = np.zeros(size1, dtype=bool)
    for size, a, wrote in answers[1]:
        assert size == size1
        assert not wrote.all(), "a rank answered everything"
        assert np.array_equal(a[wrote], whole[wrote])
        merged[wrote] = a[wrote]
        covered |= wrote
    assert covered.all() and np.array_equal(merged, whole)


def _leaf_hash_work(stats):
    return sum(w for k, _, w in stats if k == "k_leaf_hash")


def test_work_is_split(vp, case):
    """x16, W = 4, profiled: the Keccak permutations of the leaf hashes of oracle l and of oracle h, summed over the ranks, are the unsharded count, a
    quarter on each rank; above the leaves a rank hashes its quarter of the five local levels plus the replicated top of the tree."""
    d = case("sha256_x16")
    n = d["n"]
    per_world = {}
    for w in (1, 4):
        rk = Ranks(vp, d["inputs"], n, w)
        for c in rk.ctx:
            assert rk.L.vp_set_profiling(c, 1) == 0
        assert rk.commit_private() == d["gold"][:32]
        st_l = [rk.launch_stats(q) for q in range(w)]
        assert rk.commit_public_eq(d["point"]) == d["gold"][-TAIL:]
        st_h = [rk.launch_stats(q) for q in range(w)]
        per_world[w] = (st_l, st_h)
        rk.close()
    n_leaves = 1 << (n - 2)
    for oracle in (0, 1):
        whole = _leaf_hash_work(per_world[1][oracle][0])
        assert whole == 65 * n_leaves
        parts = [_leaf_hash_work(s) for s in per_world[4][oracle]]
        assert sum(parts) == whole and parts == [whole // 4] * 4
        for s in per_world[4][oracle]:
            merkle = sum(wk for k, _, wk in s if k == "k_merkle")
            assert 0 < merkle <= n_leaves // 4 + n_leaves // 32               # its quarter of the nodes of five levels + every node from level 5 up


def _flip_in_openings(rec, n, reps):
    """one byte of the record's last section (the openings) flipped"""
    per = sum(2080 + 32 * k for k in [n - 1, n - 1] + [n - 2 - j for j in range(n - 6)])
    bad = bytearray(rec)
    bad[len(rec) - reps * per + 2080 + 7] ^= 0x10                      # inside the first opening's path
    return bytes(bad)


def test_whole_protocol_on_sharded_session(vp, golden, pws_path):
    """Session(devices=[0]*4, shard_commitment=True) at x16: the complete protocol with the commitment on all ranks is accepted, its transcript is
    the real reference's, with one vp_fri_open per opening and with the query phase in one pass; the record replays on the CPU and a flipped byte fails."""
    gold = open(os.path.join(GOLDEN, golden["sha256_x16"]["transcript"]), "rb").read()
    c = vp.Circuit.from_pws(pws_path, 16, seed=1)
    n = c.layer_bitlen(0)
    s = vp.Session(c, devices=[0] * 4, round_shard_min_log=2, shard_commitment=True)
    assert s.world() == 4
    roots = None
    for batched in (False, True):
        tr, ok, _ = s.prove_and_verify_full(reps=33, batched_openings=batched)
        assert ok and tr[:len(gold)] == gold, "batched_openings=%r" % batched
        rec = s.last_full_record()
        assert c.verify_full_record(rec)
        assert not c.verify_full_record(_flip_in_openings(rec, n, 33))
        r_roots, fin, r = s.last_fri()
        roots = roots or r_roots
        assert r_roots == roots                                        # the same draws, the same FRI phase
    # the pieces on their own: prove_full, the two FRI commit forms, openings in one pass, the query phase
    full, ok = s.prove_full()
    assert ok and full == gold
    root_l, _ = s.commit_private()
    assert root_l == gold[:32]
    rh, inner, alls, _ = s.commit_public_eq(s.last_point())
    assert rh + inner + alls == gold[-TAIL:]
    r, roots_gold, fin_gold = _fri_golden(golden, "sha256_x16")
    got_roots, got_fin = s.fri_commit(r, batched=False)
    assert got_roots == b"".join(roots_gold) and np.array_equal(got_fin, fin_gold)
    reqs = [(0, 5), (1, 37), (2, 64), (2 + n - 7, 3)]
    v, p, pl = s.fri_open_many(reqs)
    for (oracle, leaf), vals, path, k, root in zip(reqs, v, p, pl, [gold[:32], rh, roots_gold[0], roots_gold[-1]]):
        assert k > 0 and _opening_ok(root, leaf, vals, [path[32 * i:32 * i + 32].tobytes() for i in range(k)])
    leaf0 = np.array([5, 1 << (n - 3)], dtype=np.uint64)
    ans = s.fri_query(leaf0)
    assert len(ans) == 2 * sum(2080 + 32 * k for k in [n - 1, n - 1] + [n - 2 - j for j in range(n - 6)])
    assert ans[:2080] == v[0].tobytes() and ans[2080:2080 + 32 * pl[0]] == p[0][:32 * pl[0]].tobytes()
    rh2, inner2, alls2, _ = s.commit_public(np.asarray(s.eq_table(s.last_point())))
    assert rh2 + inner2 + alls2 == gold[-TAIL:]
    got_roots, got_fin = s.fri_commit(r, batched=True)
    assert got_roots == b"".join(roots_gold) and np.array_equal(got_fin, fin_gold)
    assert s.fri_query(leaf0) == ans                                   # after the one-pass form the prover merges vp_fri_open_many: the same bytes
    s.close(); c.close()


def test_whole_protocol_sharded_complex_values(vp, golden):
    """randomize(8, 12): complex circuit values, W = 2"""
    gold = open(os.path.join(GOLDEN, golden["randomize_8_12"]["transcript"]), "rb").read()
    c = vp.Circuit.randomize(8, 12, seed=1)
    s = vp.Session(c, devices=[0] * 2, round_shard_min_log=2, shard_commitment=True)
    for batched in (False, True):
        tr, ok, _ = s.prove_and_verify_full(reps=33, batched_openings=batched)
        assert ok and tr[:len(gold)] == gold
        assert c.verify_full_record(s.last_full_record())
    s.close(); c.close()


def test_requests_that_cannot_be_met(vp, pws_path):
    """An input layer of 2^8 wires has 4 positions per slice: 8 ranks need 16 — refused at construction with the reason, no fall-back to rank 0.
    A non-zero mask is refused on a sharded session with the library's message."""
    import custom_circuits as cc
    c = vp.Circuit.custom(*cc.make(7, [200, 120, 60]))
    assert c.layer_bitlen(0) == 8
    with pytest.raises(RuntimeError, match="fewer than the 2 per rank"):
        vp.Session(c, devices=[0] * 8, round_shard_min_log=2, shard_commitment=True)
    s = vp.Session(c, devices=[0] * 2, round_shard_min_log=2, shard_commitment=True)      # 2 ranks fit
    s.commit_private()
    s.close(); c.close()
    c = vp.Circuit.from_pws(pws_path, 1, seed=1)
    s = vp.Session(c, devices=[0] * 2, round_shard_min_log=2, shard_commitment=True)
    mask = np.random.default_rng(6).integers(1, P, size=(8, 2), dtype=np.uint64)
    with pytest.raises(RuntimeError, match="not on a sharded commitment"):
        s.commit_private(mask=mask)
    root, _ = s.commit_private(mask=np.zeros((1, 2), dtype=np.uint64))     # the protocol's zero mask is the plain call
    assert len(root) == 32
    s.close(); c.close()
