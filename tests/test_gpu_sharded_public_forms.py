"""GPU (-m gpu): every form of public vector through the one quotient pipeline (csrc/vpgpu_pc.inc: pc_quotient_slices), on an unsharded context and on the
W ranks of a sharded commitment holding the same data.  The ranks must give the unsharded context's bytes: merkle_root_h | inner | all_sum[65], every
root of vp_fri_commit, the final codeword, and for two of the forms the same through vp_fri_step.  Shapes: the smallest a rank may hold (N / W = 2
positions per slice) at W = 2 and W = 8, and n = 13, where the transforms are the radix-8 pair.  The unsharded side is pinned to the reference at these n
by tests/test_gpu_commitment_ladder.py."""
import numpy as np
import pytest

from test_gpu_sharded_dropin_commitment import Ranks

pytestmark = pytest.mark.gpu
P = (1 << 61) - 1
# (n, W, entries of the input layer that carry values): the short layer at (10, 8) leaves the unsharded context 38 live slices and ranks 5 .. 7 no input at all
SHAPES = [(8, 2, (1 << 8) - 3), (10, 8, 37 * 16 + 1), (13, 2, (1 << 13) - 3), (13, 8, (1 << 13) - 3)]
FORMS = ["random", "tensor", "tensor_rank0", "tensor_zero_corner", "eq_tensor", "eq_general"]


def _fmul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _tensor(rng, n):
    """pub[i N + k] = c_i v_k with every c_i and v_k non-zero"""
    N = 1 << (n - 6)
    c = [tuple(int(x) for x in row) for row in rng.integers(1, P, size=(64, 2), dtype=np.uint64)]
    v = [tuple(int(x) for x in row) for row in rng.integers(1, P, size=(N, 2), dtype=np.uint64)]
    return np.array([_fmul(ci, vk) for ci in c for vk in v], dtype=np.uint64)


_DATA = {}
_RANKS = {}


def _data(n, size):
    """inputs, the public vectors by form, an opening point and the fold challenges of a shape, made once and left unchanged"""
    if (n, size) not in _DATA:
        rng = np.random.default_rng(7000 + 100 * n + size % 97)
        d = {"inputs": rng.integers(0, P, size=(size, 2), dtype=np.uint64), "random": rng.integers(0, P, size=(1 << n, 2), dtype=np.uint64),
             "tensor": _tensor(rng, n), "noise": rng.integers(0, P, size=(1 << n, 2), dtype=np.uint64),
             "point": rng.integers(0, P, size=(n, 2), dtype=np.uint64), "r": rng.integers(0, P, size=(n - 6, 2), dtype=np.uint64)}
        d["tensor_zero_corner"] = d["tensor"].copy()
        d["tensor_zero_corner"][0] = 0
        for a in d.values():
            a.setflags(write=False)
        _DATA[(n, size)] = d
    return _DATA[(n, size)]


@pytest.fixture(scope="module")
def ranks(vp):
    """(n, size, world, pc_tensor_pub) -> contexts with vp_commit_private done, kept for the module"""
    def get(n, size, world, tensor_opt):
        key = (n, size, world, tensor_opt)
        if key not in _RANKS:
            rk = Ranks(vp, _data(n, size)["inputs"], n, world, vp.Options(pc_tensor_pub=tensor_opt))
            rk.commit_private()
            _RANKS[key] = rk
        return _RANKS[key]
    yield get
    for rk in _RANKS.values():
        rk.close()
    _RANKS.clear()


def _run(rk, commit, r, stepwise):
    got = [("merkle_root_h | inner | all_sum", commit(rk)), ("roots of vp_fri_commit", rk.fri_commit(r)), ("final codeword", rk.final().tobytes())]
    if stepwise:
        got += [("merkle_root_h | inner | all_sum, second call", commit(rk)),
                ("roots of vp_fri_step", b"".join(rk.step(r[k])[0] for k in range(r.shape[0]))), ("final codeword after the steps", rk.final().tobytes())]
    return got


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,world,size", SHAPES)
def test_ranks_match_unsharded(ranks, n, world, size, form):
    """random: no structure.  tensor: c_i v, every rank and the unsharded context take the one-slice encoding.  tensor_rank0: that tensor on slices 0 .. S - 1
    and random elsewhere, so rank 0 alone takes it.  tensor_zero_corner: the tensor with pub[0] = 0, which has no scalars: every slice is encoded.  eq_tensor /
    eq_general: vp_commit_public_eq of a random point with pc_tensor_pub 1 / 0."""
    d = _data(n, size)
    N, S = 1 << (n - 6), 64 // world
    if form.startswith("eq_"):
        def commit(rk):
            return rk.commit_public_eq(d["point"])
    else:
        if form == "tensor_rank0":
            pub = d["noise"].copy()
            pub[:S * N] = d["tensor"][:S * N]
        else:
            pub = d[form]

        def commit(rk):
            return rk.commit_public(pub)
    tensor_opt = 0 if form == "eq_general" else 1
    stepwise = form in ("random", "tensor_rank0")
    want = _run(ranks(n, size, 1, tensor_opt), commit, d["r"], stepwise)
    got = _run(ranks(n, size, world, tensor_opt), commit, d["r"], stepwise)
    for (what, a), (_, b) in zip(want, got):
        assert a == b, what
    if stepwise:
        assert want[1][1] == want[4][1] and want[2][1] == want[5][1], "unsharded: the step-wise phase differs from the one-pass one"
