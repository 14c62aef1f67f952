"""Inputs of the masked-commitment cases (tests/golden/make_pc_masked.py writes the goldens from the REAL reference with them; the GPU test hands the same
arrays to the device): seeded, canonical limbs, (count, 2) uint64."""
import numpy as np

P61 = (1 << 61) - 1
# name -> (input bit length n, mask length m, seed).  Masks that pad to fewer than 8 elements are not cases: the reference's own transforms of fewer than 8 points
# read stale scratch (RS_polynomial.cpp:104-133, and its packed leaf loop runs zero times below 4 coefficients), its commitment is not a function of such a mask.
CASES = {"n13_zero": (13, 1, 10), "n13_m5": (13, 5, 11), "n13_m64": (13, 64, 13), "n16_m100": (16, 100, 14), "n19_m3000": (19, 3000, 15),
         # masks longer than a slice's message (2^(n-6) elements): 4 and 16 blocks of it, the longest the reference takes (mask_position_gap = 2)
         "n13_m300": (13, 300, 16), "n13_m2000": (13, 2000, 17),
         # the boundary between the two encode forms (ms = N = 128), a public mask shorter than the private one's padded length, and 2 and 8 blocks of a slice's message
         "n13_m128": (13, 128, 18), "n13_m100_p37": (13, 100, 19), "n13_m200": (13, 200, 20), "n13_m1000": (13, 1000, 21)}
# cases whose public mask is shorter than the private one: its length.  The reference's IN file has one length for both, so the file carries the public mask
# zero-padded to m — the padding poly_commit.h:140-141 does itself; the device and the oracle are handed the short vector.
PUB_LEN = {"n13_m100_p37": 37}


def inputs(name):
    n, m, seed = CASES[name]
    rng = np.random.default_rng(seed)
    f = lambda cnt: rng.integers(0, P61, size=(cnt, 2), dtype=np.uint64)
    x = {"n": n, "m": m, "values": f(1 << n), "pub": f(1 << n), "pri_mask": f(m), "pub_mask": f(m)}
    x["n_pub"] = PUB_LEN.get(name, m)
    x["pub_mask"][x["n_pub"]:] = 0
    if name.endswith("_zero"):               # the protocol's own case (one zero each): what the unmasked entry points must reproduce from the same record layout
        x["pri_mask"][:] = 0; x["pub_mask"][:] = 0
    return x


def write_in_file(path, n, values, pub, pri_mask, pub_mask):
    """The IN file of `ref_run --pc-masked` / `ref_run_vpgpu_masked` (oracle/ref_driver.cpp): i32 n, i32 m, values[2^n], pub[2^n], pri_mask[m], pub_mask[m] (a
    shorter public mask zero-padded to m)."""
    import struct
    m = pri_mask.shape[0]
    q = np.zeros((m, 2), np.uint64)
    q[:pub_mask.shape[0]] = pub_mask
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", n, m))
        for a in (values, pub, pri_mask, q):
            f.write(np.ascontiguousarray(a, np.uint64).tobytes())


def write_case_file(name, path):
    x = inputs(name)
    write_in_file(path, x["n"], x["values"], x["pub"], x["pri_mask"], x["pub_mask"])
    return x


# what the reference's OWN verifier (poly_commit_verifier::verify_poly_commitment, vpd_verifier.cpp:76-328) says about the reference's own commitment of each
# case (oracle/_ref/ref_run --pc-masked IN --verify, measured in the build container): a mask that pads to MORE than a slice's message (2^(n-6) elements) is
# not reduced to a constant by the n - 6 folds, and the verifier's last check ("Fri msk rs code check fail", :318-324) rejects it — prover and verifier of
# lib/virgo agree only up to that length.  The device prover must get the same verdicts.
# (the four cases added for the oracle's masked entry were recorded with the prover only)
REFERENCE_VERIFIER_ACCEPTS = {"n13_zero": True, "n13_m5": True, "n13_m64": True, "n16_m100": True, "n19_m3000": True, "n13_m300": False, "n13_m2000": False}


# ---- mask families of the masked ladder (tests/test_pc_masked_host.py on the CPU, tests/test_gpu_masked_ladder.py on the device) ------------------------------
import ctypes

import pc_array_inputs as pai

FAMILIES = ("uniform", "edges", "pub_zero", "pri_zero", "short_pub", "one_hot")
NONZERO_FAMILIES = ("uniform", "edges", "short_pub", "one_hot")       # all_sum[64] != 0 and a final mask codeword that is not all zero (asserted on the CPU)


def padded_length(n, m):
    """(gap, ms) of poly_commit.h:55-63 for a private mask of m elements at input bit length n"""
    M = 1 << (n - 1)
    gap = 1 << ((M // m).bit_length() - 1)
    return gap, M // gap


def accepted_ms(n, cap=None):
    """every padded mask length the device takes at bit length n: 8 .. M / 2, and 2 ms <= 2^17"""
    out, ms = [], 8
    while ms <= (1 << (n - 2)) and ms <= (1 << 16) and (cap is None or ms <= cap):
        out.append(ms)
        ms *= 2
    return out


def family(kind, n, ms, seed=None, m=None):
    """{"pri_mask", "pub_mask" (its own length), "r" (n - 6 challenges)} of one family for a mask that pads to ms at bit length n.  The private mask has
    ms - ms / 4 elements (uniform, edges, short_pub: the padding is exercised) or ms (the others); edges: mask and challenge limbs from pc_array_inputs.EDGES, and
    (m: another length that pads to ms) among the challenges — as many as n - 6 allows, starting at a position that turns with ms — one (0, x), one 0 and one (p - 1, p - 1)."""
    lg = ms.bit_length() - 1
    rng = np.random.default_rng(7000 + 100 * FAMILIES.index(kind) + 1000 * n + lg if seed is None else seed)
    uni = lambda cnt: rng.integers(0, P61, size=(cnt, 2), dtype=np.uint64)
    edge = lambda cnt: pai.EDGES[rng.integers(0, len(pai.EDGES), size=(cnt, 2))]
    if m is None:
        m = ms - ms // 4 if kind in ("uniform", "edges", "short_pub") else ms
    st = n - 6
    r = uni(st)
    if kind == "uniform":
        pri, pub = uni(m), uni(m)
    elif kind == "edges":
        pri, pub, r = edge(m), edge(m), edge(st)
        special = [(0, int(pai.EDGES[rng.integers(1, len(pai.EDGES))])), (0, 0), (P61 - 1, P61 - 1)]
        for i, v in enumerate(special[:st]):
            r[(lg + i) % st] = v
    elif kind == "pub_zero":
        pri, pub = uni(m), np.zeros((m, 2), np.uint64)
    elif kind == "pri_zero":
        pri, pub = np.zeros((m, 2), np.uint64), uni(m)
    elif kind == "short_pub":
        pri, pub = uni(m), uni(max(1, m // 3))
    elif kind == "one_hot":
        pri, pub = np.zeros((m, 2), np.uint64), np.zeros((m, 2), np.uint64)
        pri[m - 1], pub[m - 1] = uni(1)[0] | np.uint64(1), uni(1)[0] | np.uint64(1)
    else:
        raise KeyError(kind)
    out = {"pri_mask": np.ascontiguousarray(pri), "pub_mask": np.ascontiguousarray(pub), "r": np.ascontiguousarray(r)}
    assert padded_length(n, m) == ((1 << (n - 1)) // ms, ms) and int(max(v.max() for v in out.values())) < P61
    for v in out.values():
        v.setflags(write=False)
    return out


def masked_record_bytes(n):
    return pai.record_bytes(n) + 32 * 16


def oracle_masked_rc(L, values, n_used, pub, n, r, pri_mask, pub_mask, opens=(), n_pri=None, n_pub=None):
    """orc_commitment_array_masked_open as it is: (return code, root_l | root_h | inner | all_sum[65] | roots[n - 6] | final[2048] | final_mask[32] as bytes,
    the openings as an (len(opens), 130, 2) array).  opens: (oracle, leaf) pairs."""
    vp_, u64 = ctypes.c_void_p, ctypes.c_uint64
    f = L.orc_commitment_array_masked_open
    f.restype = ctypes.c_int
    f.argtypes = [vp_, u64, vp_, ctypes.c_int, vp_, vp_, u64, vp_, u64, ctypes.c_char_p, vp_, vp_, ctypes.c_char_p, ctypes.c_char_p, vp_, vp_, ctypes.c_int, vp_, vp_]
    values, pub, r, pri_mask, pub_mask = (np.ascontiguousarray(a, np.uint64) for a in (values, pub, r, pri_mask, pub_mask))
    assert values.shape == (1 << n, 2) and pub.shape == (1 << n, 2) and r.shape == (n - 6, 2)
    root_l, root_h, roots = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32), ctypes.create_string_buffer(32 * (n - 6))
    inner, all_sum, fin, fm = np.zeros(2, np.uint64), np.zeros((65, 2), np.uint64), np.zeros((2048, 2), np.uint64), np.zeros((32, 2), np.uint64)
    at = np.ascontiguousarray(np.array(list(opens), dtype=np.int64).reshape(-1, 2))
    vals = np.zeros((max(1, len(at)), 130, 2), np.uint64)
    rc = f(values.ctypes.data, n_used, pub.ctypes.data, n, r.ctypes.data, pri_mask.ctypes.data, pri_mask.shape[0] if n_pri is None else n_pri, pub_mask.ctypes.data,
           pub_mask.shape[0] if n_pub is None else n_pub, root_l, inner.ctypes.data, all_sum.ctypes.data, root_h, roots, fin.ctypes.data, fm.ctypes.data, len(at),
           at.ctypes.data, vals.ctypes.data)
    return rc, root_l.raw + root_h.raw + inner.tobytes() + all_sum.tobytes() + roots.raw + fin.tobytes() + fm.tobytes(), vals[:len(at)]


def oracle_masked(L, values, n_used, pub, n, r, pri_mask, pub_mask, opens=()):
    rc, rec, vals = oracle_masked_rc(L, values, n_used, pub, n, r, pri_mask, pub_mask, opens)
    assert rc == 0, rc
    return rec, vals


def split_masked_record(rec, n):
    """pc_array_inputs.split_record's fields and "final_mask" """
    assert len(rec) == masked_record_bytes(n)
    f = pai.split_record(rec[:-32 * 16], n)
    f["final_mask"] = rec[-32 * 16:]
    return f


# the recorded sizes (tests/golden/make_pc_masked_array.py): name -> (n, input set of pc_array_inputs, mask family, ms, m)
ARRAY_CASES = {"n18_m40000": (18, "uniform", "uniform", 1 << 16, 40000), "n20_edges_m16384": (20, "edges", "edges", 1 << 14, 1 << 14)}


def array_case(name):
    """inputs of a recorded size: pc_array_inputs' set with the mask family's masks and challenges"""
    n, kind, fam, ms, m = ARRAY_CASES[name]
    x = dict(pai.inputs(kind, n))
    x.update(family(fam, n, ms, m=m))
    return x


def array_digests(x):
    import hashlib
    return {k + "_sha256": hashlib.sha256(x[k].tobytes()).hexdigest() for k in ("values", "pub", "r", "pri_mask", "pub_mask")}
