"""Inputs of the commitment ladder (tests/test_gpu_commitment_ladder.py) and of its recorded sizes (tests/golden/make_pc_array.py writes pc_array_n*.bin
from the oracle with them; the GPU test hands the same arrays to the device): seeded with numpy's default_rng, canonical limbs, (count, 2) uint64.  Also the
one call of the oracle's orc_commitment_array and the layout of its record."""
import ctypes
import hashlib

import numpy as np

P61 = (1 << 61) - 1
EDGES = np.array([0, 1, 2, P61 - 1, P61 - 2, (P61 - 1) // 2, (1 << 32) - 1, 1 << 32, 1 << 60], dtype=np.uint64)
SETS = ("uniform", "edges", "sparse")


def seed_of(kind, n):
    return 1000 * (1 + SETS.index(kind)) + n


def inputs(kind, n, seed=None):
    """{"n", "n_used", "values" (2^n, zero from n_used on), "pub" (2^n), "r" (n - 6 fold challenges)} of one input set at bit length n"""
    rng = np.random.default_rng(seed_of(kind, n) if seed is None else seed)
    size, sl = 1 << n, 1 << (n - 6)
    uni = lambda cnt: rng.integers(0, P61, size=(cnt, 2), dtype=np.uint64)
    if kind == "uniform":              # complex values, a public vector that is no tensor, the last three wires unused
        n_used = size - 3
        values, pub = uni(size), uni(size)
        values[n_used:] = 0
    elif kind == "edges":              # both limbs from the ends of the range; all-zero input slices (5, 63) and an all-zero l.q product (slice 7)
        n_used = size
        values, pub = EDGES[rng.integers(0, len(EDGES), size=(size, 2))], EDGES[rng.integers(0, len(EDGES), size=(size, 2))]
        values[5 * sl:6 * sl] = 0
        values[63 * sl:] = 0
        pub[7 * sl:8 * sl] = 0
        pub[0] = 0
    elif kind == "sparse":             # a real witness of five wires: every slice behind them is all zero
        n_used = 5
        values = np.zeros((size, 2), dtype=np.uint64)
        values[:n_used, 0] = rng.integers(1, P61, size=n_used, dtype=np.uint64)
        pub = uni(size)
    else:
        raise KeyError(kind)
    x = {"n": n, "n_used": n_used, "values": np.ascontiguousarray(values), "pub": np.ascontiguousarray(pub), "r": uni(n - 6)}
    assert int(max(x[k].max() for k in ("values", "pub", "r"))) < P61
    for k in ("values", "pub", "r"):
        x[k].setflags(write=False)
    return x


def digests(x):
    return {k + "_sha256": hashlib.sha256(x[k].tobytes()).hexdigest() for k in ("values", "pub", "r")}


def record_bytes(n):
    return 64 + 16 + 65 * 16 + 32 * (n - 6) + 2048 * 16


def oracle_record(L, values, n_used, pub, n, r):
    """orc_commitment_array on the CPU: root_l | root_h | inner | all_sum[65] | roots[n - 6] | final[2048] as bytes"""
    vp_ = ctypes.c_void_p
    L.orc_commitment_array.restype = ctypes.c_int
    L.orc_commitment_array.argtypes = [vp_, ctypes.c_uint64, vp_, ctypes.c_int, vp_, ctypes.c_char_p, vp_, vp_, ctypes.c_char_p, ctypes.c_char_p, vp_]
    assert values.shape == (1 << n, 2) and pub.shape == (1 << n, 2) and r.shape == (n - 6, 2) and not values[n_used:].any()
    root_l, root_h, roots = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32), ctypes.create_string_buffer(32 * (n - 6))
    inner, all_sum, fin = np.zeros(2, np.uint64), np.zeros((65, 2), np.uint64), np.zeros((2048, 2), np.uint64)
    rc = L.orc_commitment_array(values.ctypes.data, n_used, pub.ctypes.data, n, r.ctypes.data, root_l, inner.ctypes.data, all_sum.ctypes.data, root_h, roots,
                                fin.ctypes.data)
    assert rc == 0
    return root_l.raw + root_h.raw + inner.tobytes() + all_sum.tobytes() + roots.raw + fin.tobytes()


def split_record(rec, n):
    """the record's fields: root_l, root_h, public (inner | all_sum[65], as vp_commit_public's outputs concatenate), the n - 6 FRI roots, the final codeword"""
    assert len(rec) == record_bytes(n)
    st, o = n - 6, 64 + 16 + 65 * 16
    return {"root_l": rec[:32], "root_h": rec[32:64], "public": rec[64:o], "roots": [rec[o + 32 * k:o + 32 * k + 32] for k in range(st)],
            "final": rec[o + 32 * st:]}
