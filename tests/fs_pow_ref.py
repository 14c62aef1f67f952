"""The proof of work of the non-interactive proofs in Python, written from its text in host/vphost.h ("The proof of work"): the chain step and the
smallest-nonce search with hashlib, and version-2 proofs assembled from the oracle alone on top of tests/pc_fs_ref.py and tests/full_fs_ref.py.

The step.  W(b, nonce) is s = SHA3-256({nonce, b, 0, 0x57} as little-endian u64 || s); the work is met when the low b bits of the new state's first
little-endian u64 word are zero.  It stands behind the two final codewords and in front of the positions Q(q), which are drawn from the state it leaves.

Version 2 of either proof: the 32-byte header with version = 2, then u64 pow_bits | u64 nonce, then the version-1 body.  Everything in front of the positions
is what the version-1 proof of the same commitment holds — the work moves the positions and, with them, only the answer.  So the assembly is the version-1
assembly of pc_fs_ref.expected_proof / full_fs_ref.assemble with ONE function replaced while it runs: pc_fs_ref.tail, the closing steps, by tail_with_work
below (the same steps with the search and W between the codewords and Q).  The answers are then mvc.answer at the positions that tail derives."""
import hashlib
import struct

import full_fs_ref as ff
import pc_fs_ref as fs

TAG = 0x57
VERSION_POW = 2


def step(state, bits, nonce):
    """the state W(bits, nonce) leaves behind `state`"""
    return hashlib.sha3_256(struct.pack("<4Q", nonce, bits, 0, TAG) + bytes(state)).digest()


def met(state_out, bits):
    return struct.unpack_from("<Q", state_out)[0] & ((1 << bits) - 1) == 0


def grind(state, bits, first=0, max_tries=None):
    """the smallest nonce in [first, first + max_tries) that meets the work, or None; max_tries None: 64 x 2^bits"""
    state = bytes(state)
    mask = (1 << bits) - 1
    tail = struct.pack("<3Q", bits, 0, TAG) + state
    sha, unpack = hashlib.sha3_256, struct.unpack_from
    for nonce in range(first, first + ((64 << bits) if max_tries is None else max_tries)):
        if unpack("<Q", sha(struct.pack("<Q", nonce) + tail).digest())[0] & mask == 0:
            return nonce
    return None


def hits(state, bits, first, count):
    """every nonce in [first, first + count) that meets the work, ascending"""
    out, at = [], first
    while at < first + count:
        h = grind(state, bits, at, first + count - at)
        if h is None:
            break
        out.append(h)
        at = h + 1
    return out


class _tail_with_work:
    """pc_fs_ref.tail with the work: E over the codewords, the search from 0, W(bits, nonce), the positions.  self.nonce / self.state: what it found, the
    state in front of W."""

    def __init__(self, bits, nonce=None):
        self.bits, self.forced, self.nonce, self.state = bits, nonce, None, None

    def __call__(self, ch, n, reps, final_code, final_mask):
        for x in final_code:
            ch.E(x)
        for x in final_mask:
            ch.E(x)
        self.state = ch.s
        self.nonce = grind(ch.s, self.bits) if self.forced is None else self.forced
        assert self.nonce is not None
        ch.step(self.nonce, self.bits, 0, TAG)
        return [ch.Q(q, n) for q in range(reps)]

    def __enter__(self):
        self.saved = fs.tail
        fs.tail = self
        return self

    def __exit__(self, *exc):
        fs.tail = self.saved


def with_header(body_v1, magic, bits, nonce):
    """a version-1 proof's bytes as version 2: the header's version word, the 16 bytes behind the header"""
    assert struct.unpack_from("<2I", body_v1) == (magic, 1)
    return body_v1[:4] + struct.pack("<I", VERSION_POW) + body_v1[8:32] + struct.pack("<2Q", bits, nonce) + body_v1[32:]


def as_version_1(proof_v2):
    """the header rewritten to version 1 and the 16 bytes dropped: the bytes in front of the answer are those of the version-1 proof of the same commitment"""
    assert struct.unpack_from("<I", proof_v2, 4)[0] == VERSION_POW
    return proof_v2[:4] + struct.pack("<I", 1) + proof_v2[8:32] + proof_v2[48:]


def pow_fields(proof):
    version = struct.unpack_from("<I", proof, 4)[0]
    return struct.unpack_from("<2Q", proof, 32) if version == VERSION_POW else (0, 0)


def expected_proof(L, n, x, point, f, reps, bits, nonce=None):
    """(version-2 commitment proof, the parts, the state in front of W): pc_fs_ref.expected_proof with the work in its closing steps.  nonce: forced instead of
    searched (a proof whose work is not met)."""
    with _tail_with_work(bits, nonce) as t:
        body, p = fs.expected_proof(L, n, x, point, f, reps=reps)
    p["pow_bits"], p["nonce"], p["state_before_work"] = bits, t.nonce, t.state
    return with_header(body, fs.MAGIC, bits, t.nonce), p, t.state


def proof_of(p, **change):
    """a version-2 commitment proof packed from the parts, some replaced (pow_bits, nonce among them)"""
    a = dict(p, **change)
    return with_header(fs.proof_of(a), fs.MAGIC, a["pow_bits"], a["nonce"])


def reanswered(p, bits, nonce):
    """the parts of p with another header pair: the positions the chain then derives, answered from the committed trees — what a prover who changes the pair
    and answers honestly would send"""
    import masked_verifier_cases as mvc
    ch = fs.Chain(p["state_before_work"])
    ch.step(nonce, bits, 0, TAG)
    q = dict(p, pow_bits=bits, nonce=nonce, leaf0=[ch.Q(k, p["n"]) for k in range(len(p["leaf0"]))])
    q["answer"] = mvc.answer(q)
    return q


def derive(proof):
    """(r, leaf0) of a well-formed version-2 commitment proof by the chain alone"""
    bits, nonce = pow_fields(proof)
    with _tail_with_work(bits, nonce):
        return fs.derive(as_version_1(proof))


def assemble_full(oc, candidate, bits, nonce=None, **kw):
    """The version-2 joined proof of the oracle's circuit: full_fs_ref.assemble (every stage checked against the oracle) with the work in its closing steps.
    candidate: a joined proof of either version of this circuit, input, reps and masks — only its bytes in front of the answer are read, and those do not
    depend on the work.  Returns (record, info with "nonce" and "state_before_work")."""
    v1 = as_version_1(candidate) if struct.unpack_from("<I", candidate, 4)[0] == VERSION_POW else candidate
    with _tail_with_work(bits, nonce) as t:
        rec, info = ff.assemble(oc, v1, **kw)
    info["nonce"], info["state_before_work"] = t.nonce, t.state
    return with_header(rec, ff.MAGIC, bits, t.nonce), info
