"""The non-interactive commitment proof in Python: the transcript chain with hashlib.sha3_256, written from its text in host/vphost.h ("The transcript
chain", "Proof bytes"), and the expected commitment without a device, by a fixed point over the oracle.

The chain.  H(m, s) = SHA3-256 of four little-endian u64 words followed by the 32-byte state; the state starts as 32 zero bytes and every step is s = H(m, s).
P(a, b, c, d) = {1, 0, 0, 0x50} then {a, b, c, d};  E(x) = {x.re, x.im, 0, 0x4d};  D(t, d) = {t, 0, 0, 0x44} then the digest's four words;
C(c) = {c, 0, 0, 0x43}, the element is (w0 & P, w1 & P) with P mapped to 0;  Q(q) = {q, 0, 0, 0x51}, leaf0 = 2^(n-7) + w0 mod (2^(n-2) - 2^(n-7)).

The fixed point.  r_k depends on r_0 .. r_(k-1) only, so the oracle's commitment is computed ln + 1 times with the challenges known so far and zeros behind
them; run i yields root_(i-1) (run 0: the parts that do not depend on any challenge), hence r_i.  The last run has every challenge."""
import hashlib
import struct

import numpy as np

import masked_verifier_cases as mvc
import pc_masked_inputs as pmi
import pc_verify_ref as ref

P = (1 << 61) - 1
MAGIC, VERSION = 0x46435056, 1


def limb(w):
    w &= P
    return 0 if w == P else w


class Chain:
    def __init__(self, state=None):
        self.s = bytes(32) if state is None else bytes(state)

    def step(self, a, b, c, d):
        self.s = hashlib.sha3_256(struct.pack("<4Q", a, b, c, d) + self.s).digest()

    def P(self, a, b, c, d):
        self.step(1, 0, 0, 0x50)
        self.step(a, b, c, d)

    def E(self, x):
        self.step(int(x[0]), int(x[1]), 0, 0x4d)

    def D(self, t, digest):
        self.step(t, 0, 0, 0x44)
        self.step(*struct.unpack("<4Q", digest))

    def C(self, c):
        self.step(c, 0, 0, 0x43)
        w = struct.unpack("<4Q", self.s)
        return (limb(w[0]), limb(w[1]))

    def Q(self, q, n):
        self.step(q, 0, 0, 0x51)
        lo = 1 << (n - 7)
        return lo + struct.unpack("<4Q", self.s)[0] % ((1 << (n - 2)) - lo)


def head(n, reps, ms, point, pub_mask, claim, root_l, root_h, all_sum):
    """steps 1 .. 7: the chain after D(1, root_h)"""
    ch = Chain()
    n_pub = 0 if ms == 1 else len(pub_mask)
    ch.P(n, reps, ms, n_pub)
    ch.D(0, root_l)
    for i in range(n):
        ch.E(point[i])
    for i in range(n_pub):
        ch.E(pub_mask[i])
    ch.E(claim)
    for i in range(65):
        ch.E(all_sum[i])
    ch.D(1, root_h)
    return ch


def commit_phase(ch, roots):
    """steps 8 and 9 on given roots: the challenges r_0 .. r_(ln-1), as far as the roots reach (one more than the roots given, at most ln = len(roots))"""
    r = [ch.C(0)]
    for k, root in enumerate(roots):
        if root is None:
            break
        ch.D(2 + k, root)
        if k + 1 < len(roots):
            r.append(ch.C(k + 1))
    return r


def tail(ch, n, reps, final_code, final_mask):
    """steps 10 .. 12: the positions"""
    for x in final_code:
        ch.E(x)
    for x in final_mask:
        ch.E(x)
    return [ch.Q(q, n) for q in range(reps)]


def derive(proof):
    """(r, leaf0) of a well-formed proof, by the chain alone"""
    magic, version, n, reps, ms, n_pub = struct.unpack_from("<4I2Q", proof)
    assert (magic, version) == (MAGIC, VERSION)
    ln, at = n - 6, 32
    def elems(k):
        nonlocal at
        a = np.frombuffer(proof, np.uint64, 2 * k, at).reshape(k, 2); at += 16 * k
        return a
    def raw(k):
        nonlocal at
        b = proof[at:at + k]; at += k
        return b
    point, pub_mask, claim = elems(n), elems(n_pub), elems(1)[0]
    root_l, root_h = raw(32), raw(32)
    all_sum = elems(65)
    roots = [raw(32) for _ in range(ln)]
    fin, fm = elems(2048), elems(32)
    ch = head(n, reps, ms, point, pub_mask, claim, root_l, root_h, all_sum)
    r = commit_phase(ch, roots)
    return np.array(r, np.uint64).reshape(ln, 2), tail(ch, n, reps, fin, fm)


def sections(n, reps, n_pub):
    """offset of every section of a proof"""
    ln, o, out = n - 6, 32, {"header": 0}
    for name, size in (("point", 16 * n), ("pub_mask", 16 * n_pub), ("claim", 16), ("root_l", 32), ("root_h", 32), ("all_sum", 65 * 16), ("fri_roots", 32 * ln),
                       ("final_code", 2048 * 16), ("final_mask", 32 * 16), ("answer", ref.answer_bytes(n, reps))):
        out[name] = o
        o += size
    out["end"] = o
    return out


def pack(n, reps, ms, point, pub_mask, claim, root_l, root_h, all_sum, fri_roots, final_code, final_mask, answer):
    u = lambda a: np.ascontiguousarray(a, np.uint64).tobytes()
    n_pub = 0 if ms == 1 else len(pub_mask)
    return (struct.pack("<4I2Q", MAGIC, VERSION, n, reps, ms, n_pub) + u(point) + (u(pub_mask) if n_pub else b"") + u(claim) + root_l + root_h + u(all_sum) + fri_roots +
            u(final_code) + u(final_mask) + answer)


def eq_table(point):
    """the public vector: eq(point, i) = prod_k (bit k of i ? point[k] : 1 - point[k]), by that product"""
    return np.array(ref.eq_table([(int(a), int(b)) for a, b in point]), dtype=np.uint64).reshape(-1, 2)


def masks_of(f):
    """(pri_mask, pub_mask, ms or None) as the oracle takes them: the zero mask is eight zeros against one zero (tests/test_masked_verifier_host.py)"""
    if f is None or not np.asarray(f["pri_mask"]).any():
        return np.zeros((8, 2), np.uint64), np.zeros((1, 2), np.uint64), 1
    return np.ascontiguousarray(f["pri_mask"]), np.ascontiguousarray(f["pub_mask"]), None


def fixed_point(L, n, values, n_used, point, f=None, reps=33, pub=None):
    """The commitment the chain fixes, from the oracle alone: ln + 1 runs of orc_commitment_array_masked.  Returns a dict: pub (the eq table), ms, pub_mask (what
    the chain absorbs), root_l, root_h, claim, all_sum, r (ln, 2), roots (list), state_in (after D(1, root_h)), state_out (after the last D), final_code,
    final_mask, leaf0."""
    ln = n - 6
    pub = eq_table(point) if pub is None else pub
    pri, pm, ms = masks_of(f)
    if ms is None:
        ms = pmi.padded_length(n, pri.shape[0])[1]
    chain_pm = pm if ms != 1 else pm[:0]
    r = np.zeros((ln, 2), np.uint64)
    roots, out = [None] * ln, None
    for run in range(ln + 1):
        rec, _ = pmi.oracle_masked(L, values, n_used, pub, n, r, pri, pm)
        fld = pmi.split_masked_record(rec, n)
        claim = np.frombuffer(fld["public"][:16], np.uint64)
        all_sum = np.frombuffer(fld["public"][16:], np.uint64).reshape(65, 2)
        ch = head(n, reps, ms, point, chain_pm, claim, fld["root_l"], fld["root_h"], all_sum)
        state_in = ch.s
        for k in range(run):
            assert roots[k] is None or roots[k] == fld["roots"][k], "a root moved although its challenges did not"
            roots[k] = fld["roots"][k]
        got = commit_phase(ch, roots)
        assert len(got) == min(run + 1, ln)
        for k, x in enumerate(got):
            assert run == 0 or k == len(got) - 1 or tuple(int(v) for v in r[k]) == x
            r[k] = x
        out = (fld, claim, all_sum, state_in, ch)
    fld, claim, all_sum, state_in, ch = out
    assert all(x is not None for x in roots)
    fin = np.frombuffer(fld["final"], np.uint64).reshape(2048, 2)
    fm = np.frombuffer(fld["final_mask"], np.uint64).reshape(32, 2)
    state_out = ch.s
    return {"n": n, "reps": reps, "pub": pub, "ms": ms, "pub_mask": chain_pm, "pri_mask": pri, "oracle_pub_mask": pm, "root_l": fld["root_l"], "root_h": fld["root_h"],
            "claim": claim.copy(), "all_sum": all_sum.copy(), "r": r.copy(), "roots": roots, "state_in": state_in, "state_out": state_out, "final_code": fin.copy(),
            "final_mask": fm.copy(), "leaf0": tail(ch, n, reps, fin, fm), "point": np.ascontiguousarray(point, np.uint64)}


def expected_proof(L, n, x, point, f=None, reps=33):
    """(proof bytes, the parts): the fixed point, then masked_verifier_cases.build once with its challenges for the openings, answered at the chain's positions"""
    fp = fixed_point(L, n, x["values"], x["n_used"], point, f, reps)
    p = mvc.build(L, n, dict(x, pub=fp["pub"]), {"pri_mask": fp["pri_mask"], "pub_mask": fp["oracle_pub_mask"], "r": fp["r"]}, seed=1)
    assert p["root_l"] == fp["root_l"] and p["fri_roots"] == b"".join(fp["roots"]) and p["final_code"].tobytes() == fp["final_code"].tobytes()
    p["leaf0"], p["ms"] = fp["leaf0"][:], fp["ms"]
    p["answer"] = mvc.answer(p)
    p["point"], p["chain_pub_mask"], p["pri_mask"] = fp["point"], fp["pub_mask"], fp["pri_mask"]
    return proof_of(p), p


def proof_of(p, **change):
    """a proof packed from the parts of p (masked_verifier_cases' dict with "point" and "chain_pub_mask"), some replaced"""
    a = dict(p, **change)
    return pack(a["n"], len(a["leaf0"]), a["ms"], a["point"], a["chain_pub_mask"], a["claim"], a["root_l"], a["root_h"], a["all_sum"], a["fri_roots"], a["final_code"],
                a["final_mask"], a["answer"])


# ---- cases shared by the CPU tests, the GPU tests and the recorded sizes ------------------------------------------------------------------------------------
import json
import os

import pc_array_inputs as pai

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pc_fs.json")
# The sizes whose fixed point takes the oracle longer than a test may (ln + 1 whole commitments on the CPU: 11 s at n = 14, a minute at n = 16) are recorded by
# tests/golden/make_pc_fs.py with the code above: name -> (input set of pc_array_inputs, n, mask family or None, ms or None)
RECORDED = {"uniform_n14": ("uniform", 14, None, None), "uniform_n15": ("uniform", 15, None, None), "uniform_n16": ("uniform", 16, None, None),
            "uniform_n13_m128": ("uniform", 13, "uniform", 128), "uniform_n13_m256": ("uniform", 13, "uniform", 256)}


def point_of(n):
    return np.random.default_rng(9000 + n).integers(0, P, size=(n, 2), dtype=np.uint64)


def case(kind, n, fam=None, ms=None):
    """(inputs of pc_array_inputs, the point, the mask family's vectors or None)"""
    return pai.inputs(kind, n), point_of(n), None if fam is None else pmi.family(fam, n, ms)


def record_of(fp):
    """what a recorded size keeps of its fixed point: everything vp_fri_commit_fs and the final codewords are compared with"""
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a, np.uint64).tobytes()).hexdigest()
    return {"root_l": fp["root_l"].hex(), "root_h": fp["root_h"].hex(), "state_in": fp["state_in"].hex(), "state_out": fp["state_out"].hex(),
            "roots": b"".join(fp["roots"]).hex(), "r": np.ascontiguousarray(fp["r"], np.uint64).tobytes().hex(), "final_code_sha256": sha(fp["final_code"]),
            "final_mask": np.ascontiguousarray(fp["final_mask"], np.uint64).tobytes().hex(), "ms": int(fp["ms"]), "leaf0": [int(v) for v in fp["leaf0"]],
            "inputs": {k: sha(v) for k, v in (("values", fp["values"]), ("point", fp["point"]), ("pri_mask", fp["pri_mask"]), ("pub_mask", fp["oracle_pub_mask"]))}}


def reference(L, kind, n, fam=None, ms=None):
    """record_of the fixed point of a case: computed with the oracle, or read from the recorded sizes (whose inputs are checked against the record's digests)"""
    x, point, f = case(kind, n, fam, ms)
    name = kind + "_n%d" % n + ("" if fam is None else "_m%d" % ms)
    if name in RECORDED and RECORDED[name] == (kind, n, fam, ms):
        rec = json.load(open(GOLDEN))[name]
        pri, pm, _ = masks_of(f)
        sha = lambda a: hashlib.sha256(np.ascontiguousarray(a, np.uint64).tobytes()).hexdigest()
        assert rec["inputs"] == {"values": sha(x["values"]), "point": sha(point), "pri_mask": sha(pri), "pub_mask": sha(pm)}, "the recorded inputs are not this case's"
        return rec
    fp = fixed_point(L, n, x["values"], x["n_used"], point, f)
    fp["values"] = x["values"]
    return record_of(fp)
