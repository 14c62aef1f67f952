"""Forgeries of the commitment that pass every Merkle check: changed opened values under RE-COMMITTED trees (hashlib only, no GPU, no library under test).

A byte flipped under a root that stays as it was is caught by the Merkle check before any algebra runs.  Here the prover is the cheat: it changes values and then
commits to them, so the roots, the paths and the leaf digests it sends are all consistent and only the verifier's algebra can tell.

  commitment level   forge(p, changes): p a proof of masked_verifier_cases.build (which keeps every leaf, p["vals"], and every tree, p["levels"]); the leaf chains
                     of the changed leaves and the nodes above them are recomputed; returns a new p with the new roots, fri_roots, vals, levels and answer.
                     forge(p, []) is byte-identical to p, and so is a change that writes the value a leaf already holds (which still re-hashes it).
  record level       the bytes of a complete-protocol record (host/vphost.h): sections(), openings() (every opening with the leaf index recovered from its own
                     path — the record stores no positions), recommit() — a FRESH tree for one oracle, arbitrary filler digests everywhere but at the opened
                     leaves, the given 130 values there, the new root and the new paths of every repetition written into the record.  Nothing in a record binds a
                     root: the verifier's challenges and positions come from its own seeded generator, not from the transcript, so l (root_l, the transcript's
                     first 32 bytes), h (root_h, in front of input_0) and every FRI level (the roots section) can be re-committed.

Oracles are numbered as in vp_fri_query: 0 = l, 1 = h, 2 + k = FRI level k."""
import struct

import numpy as np

import pc_verify_ref as ref

VAL = ref.VAL


def chain(value_bytes):
    """the leaf chain: 65 blocks of 32 bytes from the zero state"""
    h = bytes(32)
    for s in range(65):
        h = ref.hhash(value_bytes[32 * s:32 * s + 32], h)
    return h


# ---- commitment level ------------------------------------------------------------------------------------------------------------------------------------------
def forge(p, changes):
    """changes: (oracle, leaf, element 0 .. 129, (re, im)) — element 2 j + h of a leaf is slice j's value at the leaf's position (h = 0) or half a codeword
    further (h = 1), 128 + h the mask slice's.  Returns the re-committed proof."""
    from masked_verifier_cases import answer
    q = dict(p)
    vals, levels = list(p["vals"]), list(p["levels"])
    touched = {}
    for o, leaf, elem, value in changes:
        if o not in touched:
            vals[o] = vals[o].copy()
            levels[o] = [list(lv) for lv in levels[o]]
            touched[o] = set()
        assert 0 <= leaf < vals[o].shape[0] and 0 <= elem < 130 and 0 <= value[0] < ref.P and 0 <= value[1] < ref.P
        vals[o][leaf, elem] = value
        touched[o].add(leaf)
    for o, leaves in touched.items():
        lv = levels[o]
        for leaf in leaves:
            lv[0][leaf] = chain(vals[o][leaf].tobytes())
            pos = leaf
            for k in range(len(lv) - 1):
                pos >>= 1
                lv[k + 1][pos] = ref.hhash(lv[k][2 * pos], lv[k][2 * pos + 1])
    roots = [t[-1][0] for t in levels]
    q.update(vals=vals, levels=levels, root_l=roots[0], root_h=roots[1], fri_roots=b"".join(roots[2:]))
    q["answer"] = answer(q)
    return q


def with_positions(p, leaf0):
    """p answering other positions (the trees are kept: any leaf can be opened)"""
    from masked_verifier_cases import answer
    q = dict(p, leaf0=list(leaf0))
    q["answer"] = answer(q)
    return q


def opened(p, rep):
    """[(oracle, leaf, upper)] of repetition rep: upper — of a FRI level — says which element of the level's pair the fold of the pair before is compared with"""
    n, s0 = p["n"], p["leaf0"][rep]
    out, t = [], s0
    for o, leaf, _ in ref.query_leaves(n, s0):
        out.append((o, leaf, None if o < 2 else t != leaf))
        if o >= 2:
            t = leaf
    return out


def first_opener(p, oracle, leaf):
    """the first repetition that opens this leaf (a deep level has fewer leaves than a proof has repetitions)"""
    for rep in range(len(p["leaf0"])):
        if (oracle, leaf) in [(o, lf) for o, lf, _ in opened(p, rep)]:
            return rep
    return None


def f_add(a, d):
    return ((int(a[0]) + d[0]) % ref.P, (int(a[1]) + d[1]) % ref.P)


# ---- record level ----------------------------------------------------------------------------------------------------------------------------------------------
def sections(rec, n_pub_mask=None):
    """offsets of a record's sections, counted from its end (the transcript's length depends on the circuit); n_pub_mask: of a version-2 record"""
    magic, version, n, reps = struct.unpack_from("<4I", rec)
    assert magic == 0x52465056 and version == (1 if n_pub_mask is None else 2)
    lg = n - 6
    per_query = 2 * (VAL + 32 * (n - 1)) + sum(VAL + 32 * (n - 2 - k) for k in range(lg))
    op = len(rec) - reps * per_query
    mask = op - (0 if n_pub_mask is None else 8 + 16 * n_pub_mask + 32 * 16)
    final = mask - 2048 * 16
    roots = final - 32 * lg
    fft = roots - 16 * (64 + 3 * (2 * lg * lg + 2 * lg + 6) + 2 + 2 * lg)
    if n_pub_mask is not None:
        assert struct.unpack_from("<2I", rec, mask)[1] == n_pub_mask
    return {"n": n, "reps": reps, "transcript": 16, "root_l": 16, "root_h": fft - (32 + 16 + 65 * 16), "input_0": fft - (16 + 65 * 16), "all_sum": fft - 65 * 16,
            "fft_gkr": fft, "roots": roots, "final": final, "mask": mask, "openings": op, "per_query": per_query}


def root_offset(sec, oracle):
    return sec["root_l"] if oracle == 0 else sec["root_h"] if oracle == 1 else sec["roots"] + 32 * (oracle - 2)


def _leaf_from_path(digest, sibs, root):
    """the leaf indices whose order of concatenations leads from digest through sibs to root: one, unless a node on the way equals its sibling (a codeword that
    takes the same values in two neighbouring leaves), where both orders hash alike"""
    found = []

    def walk(h, k, idx):
        if k == len(sibs):
            if h == root:
                found.append(idx)
            return
        walk(ref.hhash(h, sibs[k]), k + 1, idx)
        walk(ref.hhash(sibs[k], h), k + 1, idx | (1 << k))
    walk(digest, 0, 0)
    return found


def openings(rec, sec):
    """[rep][oracle] = {"at": offset, "plen", "leaf", "vals": (130, 2) uint64} with the leaf recovered from the opening's own path"""
    n, out, at = sec["n"], [], sec["openings"]
    for rep in range(sec["reps"]):
        row = []
        for o, _, plen in ref.query_leaves(n, 0):
            v = rec[at:at + VAL]
            path = [rec[at + VAL + 32 * k:at + VAL + 32 * k + 32] for k in range(plen)]
            assert chain(v) == path[-1], "an opening whose leaf digest is not its values' chain"
            ro = root_offset(sec, o)
            cand = _leaf_from_path(path[-1], path[:-1], rec[ro:ro + 32])
            assert cand, "an opening that does not lead to the recorded root"
            row.append({"at": at, "plen": plen, "cand": cand, "vals": np.frombuffer(v, np.uint64).reshape(130, 2).copy()})
            at += VAL + 32 * plen
        out.append(row)
    assert at == len(rec)
    for row in out:                                  # the leaves of one query: l's and h's are the same, level k's is the leaf before modulo that level's leaves
        fits = [s0 for s0 in row[0]["cand"] if all(leaf in row[o]["cand"] for o, leaf, _ in ref.query_leaves(n, s0))]
        assert len(fits) == 1, "the paths of a repetition fit %d positions" % len(fits)
        for o, leaf, _ in ref.query_leaves(n, fits[0]):
            row[o]["leaf"] = leaf
    return out


def upper(ops, rep, k):
    """whether repetition rep compares its fold with the second element of level k's pair"""
    before = ops[rep][0 if k == 0 else 1 + k]["leaf"]
    return before != ops[rep][2 + k]["leaf"]


def recommit(rec, sec, oracle, values=None, seed=7):
    """The record with a fresh tree for `oracle`: values = {rep: (130, 2) uint64} replaces what those repetitions open (the others keep the recorded values);
    repetitions that open the same leaf must be given the same values."""
    ops = openings(rec, sec)
    values = values or {}
    at_leaf = {}
    for rep, row in enumerate(ops):
        v = np.ascontiguousarray(values.get(rep, row[oracle]["vals"]), np.uint64).tobytes()
        lf = row[oracle]["leaf"]
        assert at_leaf.setdefault(lf, v) == v, "two repetitions open leaf %d and were given different values" % lf
    depth = ops[0][oracle]["plen"] - 1
    filler = np.random.default_rng(seed).integers(0, 256, size=(1 << depth, 32), dtype=np.uint8)
    levels = [[filler[i].tobytes() for i in range(1 << depth)]]
    for lf, v in at_leaf.items():
        levels[0][lf] = chain(v)
    while len(levels[-1]) > 1:
        cur = levels[-1]
        levels.append([ref.hhash(cur[2 * i], cur[2 * i + 1]) for i in range(len(cur) // 2)])
    out = bytearray(rec)
    ro = root_offset(sec, oracle)
    out[ro:ro + 32] = levels[-1][0]
    for row in ops:
        e = row[oracle]
        lf, at = e["leaf"], e["at"]
        out[at:at + VAL] = at_leaf[lf]
        pos = lf
        for k in range(depth):
            out[at + VAL + 32 * k:at + VAL + 32 * k + 32] = levels[k][pos ^ 1]
            pos >>= 1
        out[at + VAL + 32 * depth:at + VAL + 32 * depth + 32] = levels[0][lf]
    return bytes(out)


def commitment_of(rec, sec, r, point):
    """The arguments of Circuit.verify_commitment held by a record (a proof dict as of masked_verifier_cases, without the trees): the positions are the leaves of l
    recovered from the paths; the fold challenges r and the point of the public vector are not in a record — they are the verifier's own draws."""
    n, ops = sec["n"], openings(rec, sec)
    el = lambda off, count: np.frombuffer(rec[off:off + 16 * count], np.uint64).reshape(count, 2).copy()
    p = {"n": n, "claim": el(sec["input_0"], 1)[0], "root_l": rec[sec["root_l"]:sec["root_l"] + 32], "root_h": rec[sec["root_h"]:sec["root_h"] + 32],
         "all_sum": el(sec["all_sum"], 65), "r": np.array(r, np.uint64).reshape(n - 6, 2), "fri_roots": rec[sec["roots"]:sec["final"]],
         "final_code": el(sec["final"], 2048), "final_mask": np.zeros((32, 2), np.uint64), "leaf0": [row[0]["leaf"] for row in ops],
         "answer": rec[sec["openings"]:], "pub": None, "point": np.array(point, np.uint64).reshape(n, 2), "pub_mask": np.zeros((1, 2), np.uint64), "ms": 1}
    if sec["mask"] != sec["openings"]:
        ms, n_pub = struct.unpack_from("<2I", rec, sec["mask"])
        p.update(ms=ms, pub_mask=el(sec["mask"] + 8, n_pub), final_mask=el(sec["mask"] + 8 + 16 * n_pub, 32))
    return p


def put_elem(rec, off, value):
    return rec[:off] + np.array(value, np.uint64).tobytes() + rec[off + 16:]


def get_elem(rec, off):
    return tuple(int(x) for x in np.frombuffer(rec[off:off + 16], np.uint64))


def record_cases(rec, sec, d=(3, 5), slices=(0, 63)):
    """The record-level forgeries: [(id, control record, forged record)] — another constant as a slice's final codeword; two slice sums moved against each
    other; for every oracle a fresh tree with, in repetition 0 and separately in the last one, the compared element and the pair's other element of a slice
    changed (repetitions that open the same leaf get the same values).  Every control holds the recorded values."""
    ops, out, last = openings(rec, sec), [], sec["reps"] - 1
    for s in slices:
        bad, other = rec, f_add(get_elem(rec, sec["final"] + 16 * (s << 1)), d)
        for i in range(16):
            for hi in range(2):
                bad = put_elem(bad, sec["final"] + 16 * ((i << 7) | (s << 1) | hi), other)
        out.append(("another final constant, slice %d" % s, rec, bad))
        a, b = sec["all_sum"] + 16 * s, sec["all_sum"] + 16 * ((s + 1) % 64)
        out.append(("all_sum[%d] + d, the next - d" % s, rec, put_elem(put_elem(rec, a, f_add(get_elem(rec, a), d)), b, f_add(get_elem(rec, b), (ref.P - d[0], ref.P - d[1])))))
    for oracle in range(sec["n"] - 4):
        fresh = recommit(rec, sec, oracle)
        for rep in sorted({0, last}):
            shared = [r for r in range(sec["reps"]) if ops[r][oracle]["leaf"] == ops[rep][oracle]["leaf"]]
            up = 0 if oracle < 2 else int(upper(ops, rep, oracle - 2))
            for j in slices:
                for e in (2 * j + up, 2 * j + 1 - up):
                    if oracle == 1 and ops[rep][1]["leaf"] % 32 == 0:
                        continue                     # h where x^N = 1: no part of the relation (tests/test_pc_forged_host.py)
                    v = ops[rep][oracle]["vals"].copy()
                    v[e] = f_add(v[e], d)
                    out.append(("oracle %d, repetition %d, element %d" % (oracle, rep, e), fresh, recommit(rec, sec, oracle, {r: v for r in shared})))
    return out
