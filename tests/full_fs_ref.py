"""The joined proof's record (host/vphost.h, "The joined proof") in Python: where its sections lie, and the damaged copies the CPU and the GPU tests share.
The GKR section has no length field: it is what lies between root_l and the fixed-size sections in front of the answer."""
import os
import struct

MAGIC, VERSION = 0x46465056, 1
P = (1 << 61) - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = ("randomize", 3, 7, 11, 3)            # tests/golden/full_fs_rand3_7.bin: Circuit.randomize(3, 7, seed=11), 3 repetitions, the zero mask
FIXTURE_MASKED = ("randomize", 3, 9, 12, 3)     # tests/golden/full_fs_rand3_9_ms8.bin: Circuit.randomize(3, 9, seed=12), 3 repetitions, ms = 8 (the smallest n at
                                                # which the verifier accepts ms = 8 is 9: ms <= 2^(n-6)), masks: masked_family()


def masked_family():
    import pc_masked_inputs as pmi
    return pmi.family("short_pub", FIXTURE_MASKED[2], 8)


def answer_bytes(n, reps):
    return reps * (2 * (2080 + 32 * (n - 1)) + sum(2080 + 32 * (n - 2 - k) for k in range(n - 6)))


def n_fft_msgs(lg):
    return 84 + 6 * lg * lg + 8 * lg


def sections(proof):
    """offsets of every section, "end" = the proof's length by its own header"""
    magic, version, n, reps, ms, n_pub = struct.unpack_from("<4I2Q", proof)
    ln = n - 6
    tail = [("root_h", 32), ("input_0", 16), ("all_sum", 65 * 16), ("fft_gkr", 16 * n_fft_msgs(ln)), ("fri_roots", 32 * ln), ("final_code", 2048 * 16),
            ("final_mask", 32 * 16), ("answer", answer_bytes(n, reps))]
    sec = {"header": 0, "pub_mask": 32, "root_l": 32 + 16 * n_pub, "gkr": 32 + 16 * n_pub + 32}
    at = len(proof) - sum(k for _, k in tail)
    assert at > sec["gkr"], "no room for a GKR section"
    for name, k in tail:
        sec[name] = at
        at += k
    sec["end"] = at
    return sec


def tampered(proof):
    """{what: (damaged proof, a word the verdict's reason must contain)}: one bit in every section, every changed field element still canonical (bit 2 of
    a limb's low byte: the limb stays below p unless it was within 4 of it, which the fixture's are not)"""
    s = sections(proof)
    n = struct.unpack_from("<I", proof, 8)[0]
    ln = n - 6
    at = {"root_l": (s["root_l"] + 5, "GKR"), "the first GKR element": (s["gkr"], "GKR"), "a GKR element in the middle": ((s["gkr"] + (s["root_h"] - s["gkr"]) // 32 * 16), "GKR"),
          "the last GKR element": (s["root_h"] - 16, ""), "root_h": (s["root_h"] + 9, ""), "input_0": (s["input_0"], "input"),
          "all_sum[3]": (s["all_sum"] + 48, ""), "all_sum[64]": (s["all_sum"] + 64 * 16 + 8, ""), "an fft_gkr output": (s["fft_gkr"] + 16, "fft_gkr"),
          "the last fft_gkr element": (s["fri_roots"] - 8, ""), "the final codeword": (s["final_code"] + 1000 * 16, ""),
          "the final mask": (s["final_mask"] + 16, ""), "an opened value": (s["answer"] + 48, ""), "a path": (s["end"] - 1, "")}
    for k in range(ln):
        at["FRI root %d" % k] = (s["fri_roots"] + 32 * k + 7, "")
    out = {}
    for what, (off, word) in at.items():
        bad = bytearray(proof)
        bad[off] ^= 0x04
        out[what] = (bytes(bad), word)
    return out


def malformed(proof):
    s = sections(proof)
    vals = struct.unpack_from("<4I2Q", proof)
    head = lambda **kw: struct.pack("<4I2Q", *[kw.get(k, v) for k, v in zip(("magic", "version", "n", "reps", "ms", "n_pub"), vals)]) + proof[32:]
    limb = lambda off, v: proof[:off] + struct.pack("<Q", v) + proof[off + 8:]
    return {"empty": b"", "header only": proof[:32], "short by one": proof[:-1], "long by one": proof + b"\0", "long by an element": proof + bytes(16),
            "cut inside the GKR part": proof[:s["gkr"] + 40], "cut behind root_l": proof[:s["gkr"]], "cut inside fft_gkr": proof[:s["fft_gkr"] + 100],
            "without the answer": proof[:s["answer"]], "version 2": head(version=2), "version 0": head(version=0), "the commitment proof's magic": head(magic=0x46435056),
            "n = 6": head(n=6), "n + 1": head(n=vals[2] + 1), "n = 2^32 - 1": head(n=0xFFFFFFFF), "reps = 0": head(reps=0), "reps = 4097": head(reps=4097),
            "ms = 0": head(ms=0), "ms = 4": head(ms=4), "ms = 2^63": head(ms=1 << 63), "ms = 1 with a public mask": head(n_pub=1),
            "n_pub = 2^64 - 1": head(n_pub=(1 << 64) - 1), "a GKR limb = p": limb(s["gkr"] + 16, P), "a GKR limb = 2^64 - 1": limb(s["gkr"] + 8, (1 << 64) - 1),
            "input_0 limb = p": limb(s["input_0"] + 8, P), "an fft_gkr limb = p": limb(s["fft_gkr"] + 160, P), "a final-mask limb = 2^64 - 1": limb(s["final_mask"], (1 << 64) - 1)}


def fixture(masked=False):
    return open(os.path.join(GOLDEN, "full_fs_rand3_9_ms8.bin" if masked else "full_fs_rand3_7.bin"), "rb").read()


# ---- the reference: the record assembled from the oracle, stage by stage --------------------------------------------------------------------------------------
# Written from host/vphost.h ("The joined proof"), with hashlib and the oracle alone; nothing of virgo-plus_amd is imported.  The argument is the one of
# tests/fft_gkr_fs_ref.py, applied to every stage: every oracle entry point takes its challenges up front, every challenge of the chain depends only on bytes in
# front of it.  So if (a) the challenges derived with hashlib from a candidate's bytes, handed to the oracle, give back exactly those bytes, stage after stage,
# then by induction over the chain the candidate IS the oracle's joined proof — the unique one for this circuit, input, reps and masks.  assemble() returns the
# record packed from the ORACLE's outputs (the candidate supplies only the bytes the challenges are derived from, and every stage asserts that the oracle
# returned those bytes); a test compares the whole record with the candidate.
# A wrong head order, label, counter or digest variant in the code under test gives other challenges than this file derives, and the oracle other bytes.
# Circuits: Circuit.randomize (constants zero, no assert gates) and the generators of tests/custom_circuits.py, whose constants and assert flags are handed in: the
# statement digest is computed here from the oracle's gate tables, which carry neither.
import hashlib

import numpy as np


def statement_digest(oc, with_inputs, consts=None, asserts=None):
    """layeredCircuit::statementDigest as host/circuit.hpp describes it, from the oracle's circuit: SHA3-256 over u64 words — tag, layer count, per layer its
    size and bit length, per gate {ty | assert << 32, l, u, v, lv, c.re, c.im}, maxDadBitLength, maxDadSize, per earlier layer dadSize, dadBitLength (or ~0) and
    the subset's wire list.  with_inputs = False: the tag 0x76697268 and u, v, lv, c of every input-layer gate zero.  consts (all gates, 2) / asserts (all
    gates): the constants and assert flags of a circuit made by tests/custom_circuits.py, in layer order (the oracle's export has neither); none: all zero."""
    M64 = (1 << 64) - 1
    base = 0
    w = [0x76697267 if with_inputs else 0x76697268, oc.layers]
    for i in range(oc.layers):
        g = oc.export_layer(i)
        size = len(g["ty"])
        w += [size, oc.layer_bitlen(i)]
        for k in range(size):
            cre, cim = (int(consts[base + k][0]), int(consts[base + k][1])) if consts is not None else (0, 0)
            flag = int(asserts[base + k]) if asserts is not None else 0
            rec = [(int(g["ty"][k]) & 0xFFFFFFFF) | (flag << 32), int(g["l"][k]) & M64, int(g["u"][k]), int(g["v"][k]), int(g["lv"][k]), cre, cim]
            if not with_inputs and i == 0:
                rec[2:] = [0] * 5
            w += rec
        base += size
        if i == 0:
            w += [M64, 0]
            continue
        ds, db, mx = oc.subsets(i)
        w += [mx & M64, max(ds) if ds else 0]
        for j in range(i):
            w += [ds[j], (db[j] & M64) if ds[j] else M64]
            ids = [None] * ds[j]
            for k in range(size):
                if int(g["l"][k]) == j:
                    ids[int(g["lv"][k])] = int(g["v"][k])
            assert all(x is not None for x in ids)
            w += ids
    return hashlib.sha3_256(struct.pack("<%dQ" % len(w), *w)).digest()


def gkr_schedule(ch, off, gkr):
    """vph_prove_fs's schedule from the chain's state in ch over the GKR elements gkr (gkr_tape_cases.Offsets: off.n_tr of them): every prover element E, every
    challenge C(counter) with the counter from 0 — r_liu of the output layer; Vres; per layer from the top: assert_random, phase 1 (per round the polynomial, then
    r_u[j]), claim_u, phase 2 if the layer has one (per round the polynomial, then r_v[j]; the claims), sig (all of them), the Liu sumcheck (per round the
    polynomial, then r_liu[j]), vr.  Returns the draws where orc_prove_gkr_tape reads them (slots it never reads stay zero)."""
    tape = np.zeros((off.n, 2), np.uint64)
    ctr, pos = [0], [0]

    def draw(slot):
        tape[slot] = ch.C(ctr[0])
        ctr[0] += 1

    def absorb(k):
        for _ in range(k):
            ch.E(gkr[pos[0]])
            pos[0] += 1

    def rounds(slot, k):
        for j in range(k):
            absorb(3)
            draw(slot[0] + j)

    for j in range(off.r0[1]):
        draw(off.r0[0] + j)
    absorb(1)                                                    # Vres
    for i in range(off.n_layers - 1, 0, -1):
        draw(off.ar[i][0])
        rounds(off.ru[i], off.bl[i - 1])
        absorb(1)                                                # claim_u
        if off.mdb[i] != -1:
            rounds(off.rv[i], off.mdb[i])
            absorb(i)                                            # claims_v
        for j in range(off.n_layers):
            draw(off.sig[i][0] + j)
        rounds(off.rl[i], off.bl[i - 1])
        absorb(1)                                                # vr
    assert pos[0] == off.n_tr
    return tape


def assemble(oc, candidate, pri_mask=None, oracle_pub_mask=None, consts=None, asserts=None):
    """The joined proof of the oracle's circuit oc (its own input values) with the header of `candidate`, packed from the oracle's outputs; see above.  Returns
    (record, {"point", "gkr_tape", "fft_tape", "r", "leaf0"}).  pri_mask / oracle_pub_mask: the vectors of a masked run as the oracle takes them."""
    import fft_gkr_fs_ref as fr
    import gkr_tape_cases as gc
    import masked_verifier_cases as mvc
    import oracle_binding as ob
    import pc_fs_ref as fs
    import pc_masked_inputs as pmi
    magic, version, n, reps, ms, n_pub = struct.unpack_from("<4I2Q", candidate)
    assert (magic, version) == (MAGIC, VERSION) and n == oc.layer_bitlen(0) and n >= 7
    ln = n - 6
    elems = lambda off, k: np.frombuffer(candidate, np.uint64, 2 * k, off).reshape(k, 2)
    at = 32
    pub_mask = elems(at, n_pub); at += 16 * n_pub
    root_l = candidate[at:at + 32]; at += 32
    # ---- 1, 2: the statement without the input values, the head
    ch = fs.Chain()
    ch.step(*struct.unpack("<4Q", statement_digest(oc, False, consts, asserts)))
    ch.step(oc.layers, 0, 0, 0x53)
    ch.P(n, reps, ms, n_pub)
    for x in pub_mask:
        ch.E(x)
    ch.D(0, root_l)
    # ---- 3: the GKR part: vph_prove_fs's schedule on the candidate's elements; the draws go where orc_prove_gkr_tape reads them
    off = gc.Offsets.of(oc)
    gkr = elems(at, off.n_tr)
    tape = gkr_schedule(ch, off, gkr)
    tr, _ = oc.prove_gkr_tape(tape)
    assert tr == gkr.tobytes(), "stage 3: the oracle's GKR proof on the derived challenges is not the candidate's GKR section"
    at += 16 * off.n_tr
    point = tape[off.rl[1][0]:off.rl[1][0] + n].copy()
    # ---- 4: the commitment head at the derived point
    root_h = candidate[at:at + 32]
    input_0, all_sum = elems(at + 32, 1)[0], elems(at + 48, 65)
    at += 48 + 65 * 16
    ch.E(input_0)
    for x in all_sum:
        ch.E(x)
    ch.D(1, root_h)
    # ---- 5: fft_gkr at lg = n - 6 from that state
    fmsgs = elems(at, n_fft_msgs(ln)); at += 16 * n_fft_msgs(ln)
    ftape, st = fr.derive(ln, ch.s, fmsgs)
    ftape = np.array(ftape, np.uint64).reshape(-1, 2)
    raw, verified = ob.fft_gkr_tape(ln, ftape)
    assert raw == fmsgs.tobytes() and verified, "stage 5: the oracle's fft_gkr on the derived tape is not the candidate's fft_gkr section"
    ch.s = st
    # ---- 6: the FRI commit phase from the state fft_gkr leaves
    roots = [candidate[at + 32 * k:at + 32 * k + 32] for k in range(ln)]; at += 32 * ln
    r = np.array(fs.commit_phase(ch, roots), np.uint64).reshape(ln, 2)
    # ---- the commitment from the oracle at the derived point and fold challenges
    values = np.zeros((1 << n, 2), np.uint64)
    inputs = oc.export_layer(0)["u"]
    values[:len(inputs), 0] = inputs
    if ms == 1:
        pri, opm = np.zeros((8, 2), np.uint64), np.zeros((1, 2), np.uint64)
    else:
        pri, opm = np.ascontiguousarray(pri_mask, np.uint64), np.ascontiguousarray(oracle_pub_mask, np.uint64)
        assert pmi.padded_length(n, pri.shape[0])[1] == ms and opm[:n_pub].tobytes() == pub_mask.tobytes()
    p = mvc.build(ob.lib(), n, {"values": values, "n_used": len(inputs), "pub": fs.eq_table(point)}, {"pri_mask": pri, "pub_mask": opm, "r": r}, seed=1)
    assert p["root_l"] == root_l, "stage 2: the oracle's root_l is not the candidate's"
    assert p["root_h"] == root_h and p["claim"].tobytes() == input_0.tobytes() and p["all_sum"].tobytes() == all_sum.tobytes(), "stage 4: root_h, input_0, all_sum"
    assert p["fri_roots"] == b"".join(roots), "stage 6: the oracle's FRI roots on the derived challenges"
    # ---- 7: the closing steps
    p["leaf0"] = fs.tail(ch, n, reps, p["final_code"], p["final_mask"])
    answer = mvc.answer(p)
    rec = (struct.pack("<4I2Q", MAGIC, VERSION, n, reps, ms, n_pub) + pub_mask.tobytes() + p["root_l"] + tr + p["root_h"] + p["claim"].tobytes() + p["all_sum"].tobytes() +
           raw + p["fri_roots"] + p["final_code"].tobytes() + p["final_mask"].tobytes() + answer)
    return rec, {"point": point, "gkr_tape": tape, "fft_tape": ftape, "r": r, "leaf0": p["leaf0"]}
