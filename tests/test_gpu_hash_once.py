"""One leaf-hash launch and one sequence of Merkle launches for the l, h and FRI oracles of a protocol pass (vp_pc_hash_late, include/vpgpu.h; the
pass of vphost.h uses it by default, VPH_PASS_HASH_PER_CALL restores the three-launch form): the same bytes at every size at which the merged list takes
another path, and no call sequence of the C ABI that sees a missing tree.

Sizes: x1 / x16 — compiler-form kernels, trees of 2^11 / 2^15 leaves, the 16-leaf last FRI level in the same launch; x64 — trees of 2^17 leaves each (alone:
512-thread workgroups), the merged list crosses 2^18 leaves and takes 1024-thread ones; x256 — one case of the generated chains on 2^19-leaf trees."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_masked_fast_path as masked
import test_gpu_parity as parity
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
P = (1 << 61) - 1
VP = ctypes.c_void_p


def _seeded(shape, seed):
    return np.random.default_rng(seed).integers(0, P, size=shape, dtype=np.uint64)


def _same(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


_CIRCUITS = {}


@pytest.fixture(scope="module")
def circuit(vp, pws_path):
    """SHA-256 circuits by block count, built once for the module."""
    def get(blocks):
        if blocks not in _CIRCUITS:
            _CIRCUITS[blocks] = vp.Circuit.from_pws(pws_path, blocks, seed=1)
        return _CIRCUITS[blocks]
    yield get
    for c in _CIRCUITS.values():
        c.close()
    _CIRCUITS.clear()


# ---- 1. the pass: same bytes in both forms, and the real reference's ----------------------------------------------------------------------------
@pytest.mark.parametrize("asm", [1, 0])
@pytest.mark.parametrize("name,blocks", [("sha256_x1", 1), ("sha256_x16", 16), ("sha256_x64", 64)])
def test_merged_pass_equals_per_call_pass_and_the_reference(vp, golden, circuit, name, blocks, asm):
    """Two merged passes in a row (the second on the buffers of the first) equal the pass that hashes per call and the real reference's transcript, FRI roots
    and final codeword; generated chains (leaf_asm = 1) and the compiler's form (leaf_asm = 0)."""
    s = vp.Session(circuit(blocks), options=vp.Options(leaf_asm=asm))
    s.draw_protocol_tape()
    old = s.prove_protocol(hash_per_call=True)
    gold = open(os.path.join(GOLDEN, golden[name]["transcript"]), "rb").read()
    _, roots_gold, fin_gold = parity._fri_golden(golden, name)
    assert old[0] == gold and old[1] == roots_gold and np.array_equal(old[2], fin_gold)
    for _ in range(2):
        new = s.prove_protocol()
        assert new[0] == gold, "transcript (merkle_root_l | GKR | merkle_root_h | input_0 | all_sum)"
        assert new[1] == roots_gold and np.array_equal(new[2], fin_gold)
    assert _same(s.prove_protocol(deferred=True), old)
    assert _same(s.prove_protocol(deferred=True, hash_per_call=True), old)
    s.close()


def test_merged_pass_on_the_generated_chains_at_2_19_leaf_trees(vp, circuit):
    """x256: three trees of 2^19 leaves and the levels below in one launch of 1024-thread workgroups, against the per-call form."""
    s = vp.Session(circuit(256))
    s.draw_protocol_tape()
    old = s.prove_protocol(hash_per_call=True)
    for _ in range(2):
        assert _same(s.prove_protocol(), old)
    s.close()


# ---- 2. the C ABI ------------------------------------------------------------------------------------------------------------------------------
class _Abi:
    """A session's context with the synchronous answers recorded once: roots, input_0 / all_sum, FRI roots, one opening per oracle, a query answer."""

    def __init__(self, vp, c):
        self.vp, self.L = vp, vp.lib_gpu()
        L = self.L
        L.vp_pc_hash_late.argtypes = [VP, ctypes.c_int]
        L.vp_flush.argtypes = [VP, ctypes.c_int]
        L.vp_set_deferred.argtypes = [VP, ctypes.c_int]
        L.vp_fri_step.argtypes = [VP, VP, VP]
        L.vp_commit_public_eq.argtypes = [VP, VP, ctypes.c_int, VP, VP, VP]
        L.vp_fri_open.argtypes = [VP, ctypes.c_int, ctypes.c_uint64, VP, VP, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        self.s = vp.Session(c)
        self.ctx = self.s.gpu_ctx()
        self.n = c.layer_bitlen(0)
        self.st = self.n - 6
        self.point = _seeded((self.n, 2), 5)
        self.r = _seeded((self.st, 2), 6)
        self.leaf0 = np.array([0, 7, (1 << (self.n - 2)) - 1], dtype=np.uint64)
        self.mode(0)
        self.want_l = self.private()[1]
        _, self.want_h, self.want_sums = self.public()
        _, self.want_roots = self.fri_commit()
        self.want_open = [self.open(o, 3) for o in (0, 1, 2)]
        rc, self.want_query = vp.fri_query(self.ctx, self.leaf0)
        assert rc == 0 and all(w[0] == 0 for w in self.want_open)

    def mode(self, on):
        assert self.L.vp_pc_hash_late(self.ctx, on) == 0

    def private(self):
        root = ctypes.create_string_buffer(b"\xee" * 32, 32)
        rc = self.L.vp_commit_private(self.ctx, ctypes.cast(root, VP))
        assert rc == 0, self.L.vp_last_error(self.ctx)
        return root, root.raw

    def public(self):
        root = ctypes.create_string_buffer(b"\xee" * 32, 32)
        sums = np.zeros((66, 2), np.uint64)                   # input_0 | all_sum[65]
        self.keep = sums                                      # (written by vp_flush under deferred completion: alive until the next call)
        rc = self.L.vp_commit_public_eq(self.ctx, self.point.ctypes.data, self.n, sums.ctypes.data, sums.ctypes.data + 16, ctypes.cast(root, VP))
        assert rc == 0, self.L.vp_last_error(self.ctx)
        return root, root.raw, sums.tobytes()

    def fri_commit(self):
        roots = ctypes.create_string_buffer(b"\xee" * (32 * self.st), 32 * self.st)
        rc = self.L.vp_fri_commit(self.ctx, self.r.ctypes.data, self.st, ctypes.cast(roots, VP))
        assert rc == 0, self.L.vp_last_error(self.ctx)
        return roots, roots.raw

    def fri_steps(self):
        out = b""
        for k in range(self.st):
            root = ctypes.create_string_buffer(32)
            rk = np.ascontiguousarray(self.r[k])
            assert self.L.vp_fri_step(self.ctx, rk.ctypes.data, ctypes.cast(root, VP)) == 0, self.L.vp_last_error(self.ctx)
            out += root.raw
        return out

    def open(self, oracle, leaf):
        vals = np.zeros((130, 2), np.uint64)
        path = ctypes.create_string_buffer(32 * 40)
        plen = ctypes.c_int(0)
        rc = self.L.vp_fri_open(self.ctx, oracle, leaf, vals.ctypes.data, ctypes.cast(path, VP), len(path), ctypes.byref(plen))
        return rc, vals.tobytes(), path.raw[:32 * plen.value]

    def close(self):
        self.mode(0)
        self.s.close()


@pytest.fixture(scope="module", params=[16, 64], ids=["x16", "x64"])
def abi(request, vp, circuit):
    a = _Abi(vp, circuit(request.param))
    yield a
    a.close()


UNTOUCHED = b"\xee" * 32


def test_commit_private_under_the_mode_leaves_the_root_and_an_opening_hashes_it(abi):
    abi.mode(1)
    root, now = abi.private()
    assert now == UNTOUCHED, "vp_commit_private under vp_pc_hash_late wrote its root"
    got = abi.open(0, 3)                                        # path and root (the path's last digest) of the synchronous call
    assert got == abi.want_open[0]
    assert root.raw == abi.want_l
    abi.mode(0)


def test_commit_public_eq_under_the_mode_then_steps_and_query(abi):
    abi.mode(1)
    root_l, _ = abi.private()
    root_h, now_h, sums = abi.public()
    assert root_l.raw == UNTOUCHED and now_h == UNTOUCHED
    assert sums == abi.want_sums, "input_0 / all_sum are delivered by the call itself"
    assert abi.fri_steps() == abi.want_roots                    # vp_fri_step hashes what is outstanding first
    assert root_l.raw == abi.want_l and root_h.raw == abi.want_h
    rc, q = abi.vp.fri_query(abi.ctx, abi.leaf0)
    assert rc == 0 and q == abi.want_query
    abi.mode(0)


def test_fri_commit_merges_both_oracles_and_the_query_reads_its_trees(abi):
    abi.mode(1)
    root_l, _ = abi.private()
    root_h, _, sums = abi.public()
    assert root_l.raw == UNTOUCHED and root_h.raw == UNTOUCHED and sums == abi.want_sums
    _, roots = abi.fri_commit()
    assert roots == abi.want_roots
    assert root_l.raw == abi.want_l and root_h.raw == abi.want_h
    rc, q = abi.vp.fri_query(abi.ctx, abi.leaf0)
    assert rc == 0 and q == abi.want_query
    assert [abi.open(o, 3) for o in (0, 1, 2)] == abi.want_open
    abi.mode(0)


def test_fri_commit_merges_under_deferred_completion(abi):
    """Both modes together: nothing is written before vp_flush, everything by it; vp_pending counts the four calls as with the mode off."""
    L = abi.L
    abi.mode(1)
    assert L.vp_set_deferred(abi.ctx, 1) == 0
    root_l, _ = abi.private()
    root_h, _, _ = abi.public()
    roots, now = abi.fri_commit()
    sums = abi.keep
    n = ctypes.c_int(-1)
    assert L.vp_pending(abi.ctx, ctypes.byref(n)) == 0 and n.value == 3
    assert root_l.raw == UNTOUCHED and root_h.raw == UNTOUCHED and now == b"\xee" * len(now)
    assert L.vp_flush(abi.ctx, -1) == 0
    assert root_l.raw == abi.want_l and root_h.raw == abi.want_h and roots.raw == abi.want_roots and sums.tobytes() == abi.want_sums
    assert L.vp_set_deferred(abi.ctx, 0) == 0
    abi.mode(0)


def test_flush_with_the_mode_switched_off_writes_the_root(abi):
    abi.mode(1)
    root, now = abi.private()
    assert now == UNTOUCHED
    assert abi.L.vp_flush(abi.ctx, -1) == 0
    assert root.raw == UNTOUCHED, "vp_flush with the mode on keeps waiting for vp_fri_commit"
    abi.mode(0)
    assert root.raw == UNTOUCHED
    assert abi.L.vp_flush(abi.ctx, -1) == 0
    assert root.raw == abi.want_l


def test_two_commit_private_in_a_row_under_the_mode(abi):
    abi.mode(1)
    first, _ = abi.private()
    second, _ = abi.private()
    assert first.raw == abi.want_l, "the second call hashes what the first left"
    assert second.raw == UNTOUCHED
    abi.mode(0)
    assert abi.L.vp_flush(abi.ctx, -1) == 0
    assert second.raw == abi.want_l


def test_masked_commitment_ignores_the_mode(abi):
    """vp_commit_private_masked under the mode hashes at once (and first hashes an unmasked l left before it); the masked public commit and vp_fri_commit's
    per-step branch give the bytes of the mode off."""
    L = abi.L
    L.vp_commit_private_masked.argtypes = [VP, VP, ctypes.c_uint64, VP]
    L.vp_commit_public_masked.argtypes = [VP, VP, ctypes.c_uint64, VP, ctypes.c_uint64, VP, VP, VP]
    L.vp_fri_final_mask.argtypes = [VP, VP]
    pm, qm = _seeded((100, 2), 21), _seeded((64, 2), 22)
    pub = _seeded((1 << abi.n, 2), 23)

    def run():
        rl, rh = ctypes.create_string_buffer(b"\xee" * 32, 32), ctypes.create_string_buffer(b"\xee" * 32, 32)
        sums = np.zeros((66, 2), np.uint64)
        assert L.vp_commit_private_masked(abi.ctx, pm.ctypes.data, pm.shape[0], ctypes.cast(rl, VP)) == 0, L.vp_last_error(abi.ctx)
        first = rl.raw
        assert L.vp_commit_public_masked(abi.ctx, pub.ctypes.data, pub.shape[0], qm.ctypes.data, qm.shape[0], sums.ctypes.data, sums.ctypes.data + 16,
                                         ctypes.cast(rh, VP)) == 0, L.vp_last_error(abi.ctx)
        _, roots = abi.fri_commit()
        fm = np.zeros((32, 2), np.uint64)
        assert L.vp_fri_final_mask(abi.ctx, fm.ctypes.data) == 0
        return first, rl.raw, rh.raw, sums.tobytes(), roots, fm.tobytes(), abi.open(0, 3), abi.open(1, 3)

    abi.mode(0)
    want = run()
    assert want[0] != abi.want_l and want[5] != bytes(32 * 16)
    abi.mode(1)
    left, _ = abi.private()
    got = run()
    assert left.raw == abi.want_l
    assert got == want
    abi.mode(0)
    abi.private()                                               # the next test starts from an unmasked commitment


# ---- 2b. the unmasked chain at each workgroup form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [18, 19, 20])
def test_asm_chain_at_each_workgroup_form(vp, n):
    """The generated chain that ends in the all-zero block (vp_leaf_chain_asm), every form it is launched in — the unmasked twin of
    test_gpu_masked_fast_path.py::test_asm_mask_chain_at_each_workgroup_form, on arbitrary uniform inputs:
         per call — one oracle per launch: the compiler's form at n = 18, 2^17 leaves at n = 19 (512 threads + LDS blocker), 2^18 at n = 20 (1024 threads);
         vp_pc_hash_late(1) — the merged launch: 3 x 2^16 - 16 leaves at n = 18 (512 threads), 3 x 2^17 - 16 at n = 19 and 3 x 2^18 - 16 at n = 20 (1024
         threads; no multiple of 1024: the last workgroup's clamped tail runs and stores nothing).
    Reference: the same input on a context created with VP_LEAF_ASM=0 — every root, the FRI roots, the final codeword and 16 openings per oracle.
    Independently, for the 42 leaves the masked test picks (the ends of l and h, the ends of coset blocks, the first two levels, leaves 0 and 15 of the
    single-value last level), hashlib.sha3_256 over the 64 opened pairs and the zero pair equals the path's leaf entry."""
    st = n - 6
    vals, point, r = masked._uniform(1 << n, 800 + n), masked._uniform(n, 900 + n), masked._uniform(st, 1000 + n)
    req = masked._requests(n, st, 16)

    def run(c, late):
        assert c.L.vp_pc_hash_late(c.ctx, 1 if late else 0) == 0
        c.commit_private()
        c.commit_public_eq(point)
        roots = c.fri_commit(r)
        assert c.L.vp_pc_hash_late(c.ctx, 0) == 0
        fin = np.zeros((2048, 2), np.uint64)
        assert c.L.vp_fri_final(c.ctx, fin.ctypes.data) == 0, c.err()
        return c.state(), roots, fin.tobytes()

    ref = masked.Ctx(vp, vals, n, env={"VP_LEAF_ASM": "0"})
    try:
        want = run(ref, False)
        wv, wp, wl = ref.open_many(req)
    finally:
        ref.close()
    c = masked.Ctx(vp, vals, n)
    try:
        for late in (False, True):
            assert run(c, late) == want, ("late" if late else "per call")
            v, p, pl = c.open_many(req)
            assert np.array_equal(v, wv) and np.array_equal(p, wp) and np.array_equal(pl, wl), late
            pick = {(o, lf) for o in (0, 1) for lf in masked._leaves_of(1 << (n - 2), 16)}
            pick |= {(o, lf) for o in (2, 3) for lf in masked._leaves_of(16 * ((1 << (n - 6)) >> (o - 1)), 4)}
            pick |= {(2 + st - 1, 0), (2 + st - 1, 15)}
            checked = 0
            for i, (o, lf) in enumerate(req):
                if (o, lf) in pick:
                    pairs = np.zeros((130, 2), np.uint64)
                    pairs[:128] = v[i][:128]                                    # the 64 slices' pairs; the 65th block is the zero pair
                    assert p[i, 32 * (pl[i] - 1):32 * pl[i]].tobytes() == masked._sha3_leaf(pairs), (late, o, lf)
                    checked += 1
            assert checked == len(pick) == 42
    finally:
        c.close()


# ---- 3. passes that queue the next pass's head ------------------------------------------------------------------------------------------------
def test_queue_next_passes_merge_h_and_the_levels_only(vp, circuit):
    s = vp.Session(circuit(16))
    s.draw_protocol_tape()
    ref = s.prove_protocol(hash_per_call=True)
    for _ in range(2):
        assert _same(s.prove_protocol(queue_next=True), ref)
    n = ctypes.c_int(-1)
    assert vp.lib_gpu().vp_pending(s.gpu_ctx(), ctypes.byref(n)) == 0 and n.value == 1          # the next pass's complete commit_private
    assert _same(s.prove_protocol(deferred=True), ref)                                           # finds it: h and the FRI levels in the one launch
    assert vp.lib_gpu().vp_pending(s.gpu_ctx(), ctypes.byref(n)) == 0 and n.value == 0
    assert _same(s.prove_protocol(queue_next=True), ref)
    tr_i, _, ok_i = s.prove_interactive()
    assert ok_i and tr_i == ref[0][32:32 + len(tr_i)]
    s.draw_protocol_tape()
    assert _same(s.prove_protocol(), ref)
    root, _ = s.commit_private()
    assert root == ref[0][:32]
    s.close()


# ---- 4. the whole protocol behind a merged pass -------------------------------------------------------------------------------------------------
def test_whole_protocol_after_a_merged_pass(vp, golden, circuit):
    """x16: the query phase answered from the trees the merged launch built equals the one answered from the per-call trees; then verifier::verify() end to
    end with 33 repetitions on the same session: accepted, the transcript of the batched-openings run and the reference's."""
    n = 17
    leaf0 = np.random.default_rng(3).integers(0, 1 << (n - 2), size=33, dtype=np.uint64)
    s = vp.Session(circuit(16))
    s.draw_protocol_tape()
    s.prove_protocol(hash_per_call=True)
    want = s.fri_query(leaf0)
    merged = s.prove_protocol()
    assert s.fri_query(leaf0) == want
    tr, ok, _ = s.prove_and_verify_full(reps=33)
    tr_b, ok_b, _ = s.prove_and_verify_full(reps=33, batched_openings=True)
    assert ok and ok_b and tr == tr_b == merged[0]
    assert tr == open(os.path.join(GOLDEN, golden["sha256_x16"]["transcript"]), "rb").read()
    s.close()


# ---- 5. the -DVP_CHECKED flavour -----------------------------------------------------------------------------------------------------------------
_CHECKED_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import vp_loader
vp = vp_loader.load()
vp.lib_host()
assert vp.lib_gpu().vp_checked_build() == 1, "VP_LIBGPU did not select the checked library"
c = vp.Circuit.from_pws(sys.argv[1], 16, seed=1)
s = vp.Session(c)
s.draw_protocol_tape()
new = s.prove_protocol()
old = s.prove_protocol(hash_per_call=True)
assert new[0] == open(sys.argv[2], "rb").read() and new[0] == old[0] and new[1] == old[1] and np.array_equal(new[2], old[2])
print("CHECKED OK", flush=True)
"""


def test_checked_build_runs_a_merged_pass_without_a_reported_site(vp, golden, pws_path):
    """The compiler-form kernels with their index checks compiled in cover the merged list through blk_start: one merged pass at x16, the reference's
    transcript, and no check fires (a violated one fails the call with VP_EHIP and its site)."""
    assert os.path.exists(vp.LIB_GPU_CHECKED), "vp.build() did not produce the checked library"
    env = dict(os.environ, VP_LIBGPU=vp.LIB_GPU_CHECKED)
    gold = os.path.join(GOLDEN, golden["sha256_x16"]["transcript"])
    r = subprocess.run([sys.executable, "-c", _CHECKED_CHILD % ROOT, pws_path, gold], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0 and "CHECKED OK" in r.stdout, (r.stdout[-800:], r.stderr[-2000:])
