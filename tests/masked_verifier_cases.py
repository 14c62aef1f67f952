"""Complete commitment proofs for the commitment-level verifier (Circuit.verify_commitment), assembled in Python.

CPU (tests/test_masked_verifier_host.py): the oracle's masked commitment opens EVERY leaf of l, h and every FRI level (orc_commitment_array_masked_open);
the leaf chains and Merkle trees are built here with hashlib (the chain and the path walk of tests/pc_verify_ref.py), and the answers to seeded positions
are laid out as vp_fri_query lays them out.  The trees' roots are compared with the oracle's before anything is verified: a difference would be this
file's mistake, not the verifier's.  GPU (tests/test_gpu_masked_verifier.py): positions() and the argument order of verify() are shared."""
import numpy as np

import pc_array_inputs as pai
import pc_masked_inputs as pmi
import pc_verify_ref as ref

REPS = 33
VAL = ref.VAL
# what `ref_run --pc-masked IN --verify` printed for each of pc_masked_inputs.CASES (observed where the reference was built; tests/test_masked_verifier_host.py
# asks for the same again): the rule is ms <= N = 2^(n-6)
REFERENCE_VERDICTS = {"n13_zero": True, "n13_m5": True, "n13_m64": True, "n16_m100": True, "n19_m3000": True, "n13_m300": False, "n13_m2000": False,
                      "n13_m128": True, "n13_m100_p37": True, "n13_m200": False, "n13_m1000": False}


def positions(n, seed, reps=REPS):
    """reps seeded leaves in [N / 2, M / 2), both ends of the range among them"""
    lo, hi = 1 << (n - 7), 1 << (n - 2)
    rng = np.random.default_rng(seed)
    lf = [int(x) for x in rng.integers(lo, hi, size=reps)]
    lf[0], lf[-1] = lo, hi - 1
    return lf


def _tree(leaf_digests):
    """levels[0] = the leaf digests, levels[k + 1][i] = H(levels[k][2 i] || levels[k][2 i + 1]) (a node is SHA3-256 of left || right)"""
    levels = [leaf_digests]
    while len(levels[-1]) > 1:
        cur = levels[-1]
        levels.append([ref.hhash(cur[2 * i], cur[2 * i + 1]) for i in range(len(cur) // 2)])
    return levels


def _opening(levels, vals, leaf):
    """130 values | sibling at height 0 .. depth - 1 | the leaf digest (vp_fri_open's path order)"""
    out, pos = [vals[leaf].tobytes()], leaf
    for k in range(len(levels) - 1):
        out.append(levels[k][pos ^ 1])
        pos >>= 1
    out.append(levels[0][leaf])
    return b"".join(out)


def build(L, n, x, f, seed):
    """One complete proof: x = pc_array_inputs.inputs(..), f = {"pri_mask", "pub_mask", "r"}.  Returns the arguments of verify() as a dict, with the
    trees kept (\"levels\") so that a test can re-assemble an answer after changing an opened value."""
    st = n - 6
    n_leaves = [1 << (n - 2)] * 2 + [1 << (n - 3 - k) for k in range(st)]
    opens = [(o, lf) for o, cnt in enumerate(n_leaves) for lf in range(cnt)]
    rec, vals = pmi.oracle_masked(L, x["values"], x["n_used"], x["pub"], n, f["r"], f["pri_mask"], f["pub_mask"], opens)
    fld = pmi.split_masked_record(rec, n)
    per, at = [], 0
    for cnt in n_leaves:
        per.append(vals[at:at + cnt]); at += cnt
    trees = []
    for v in per:
        digs = []
        for leaf in range(v.shape[0]):
            b, h = v[leaf].tobytes(), bytes(32)
            for s in range(65):
                h = ref.hhash(b[32 * s:32 * s + 32], h)
            digs.append(h)
        trees.append(_tree(digs))
    roots = [t[-1][0] for t in trees]
    assert roots[0] == fld["root_l"] and roots[1] == fld["root_h"] and roots[2:] == fld["roots"], "this file's trees are not the oracle's"
    lf = positions(n, seed)
    pub = fld["public"]
    p = {"n": n, "claim": np.frombuffer(pub[:16], np.uint64).copy(), "root_l": fld["root_l"], "root_h": fld["root_h"],
         "all_sum": np.frombuffer(pub[16:], np.uint64).reshape(65, 2).copy(), "r": np.array(f["r"]), "fri_roots": b"".join(fld["roots"]),
         "final_code": np.frombuffer(fld["final"], np.uint64).reshape(2048, 2).copy(), "final_mask": np.frombuffer(fld["final_mask"], np.uint64).reshape(32, 2).copy(),
         "leaf0": lf, "pub": np.array(x["pub"]), "pub_mask": np.array(f["pub_mask"]), "ms": pmi.padded_length(n, f["pri_mask"].shape[0])[1],
         "vals": per, "levels": trees}
    p["answer"] = answer(p)
    return p


def answer(p, vals=None):
    """the openings of p's positions in vp_fri_query's layout (vals: other opened values than the committed ones, on the committed trees)"""
    vals = p["vals"] if vals is None else vals
    out = []
    for l0 in p["leaf0"]:
        for o, leaf, plen in ref.query_leaves(p["n"], l0):
            b = _opening(p["levels"][o], vals[o], leaf)
            assert len(b) == VAL + 32 * plen
            out.append(b)
    return b"".join(out)


def verify(vp, p, device=None, **change):
    """Circuit.verify_commitment on p with some arguments replaced"""
    a = dict(p, **change)
    return vp.Circuit.verify_commitment(a["n"], a["claim"], a["root_l"], a["root_h"], a["all_sum"], a["r"], a["fri_roots"], a["final_code"], a["final_mask"],
                                        a["leaf0"], a["answer"], pub=a["pub"], pub_mask=a["pub_mask"], ms=a["ms"], device=device)


def f_add(a, d):
    """a + d on (re, im) limb pairs of uint64"""
    return np.array([(int(a[0]) + int(d[0])) % ref.P, (int(a[1]) + int(d[1])) % ref.P], np.uint64)
