"""Shared by tests/test_gkr_fs_host.py (CPU) and tests/test_gpu_gkr_fs.py: the reference of vp_prove_gkr_fs / vph_gkr_fs_tape.

The reference is full_fs_ref.gkr_schedule — vph_prove_fs's schedule written from host/vphost.h with hashlib — on the transcript under test.  As in full_fs_ref: a
prover that takes its tape up front (vp_prove_gkr, orc_prove_gkr_tape) and returns exactly this transcript on exactly the tape derived from it is, by induction
over the chain, the one non-interactive proof from that state."""
import struct

import numpy as np

import full_fs_ref as ff
import gkr_tape_cases as gc
import pc_fs_ref as fs

START_STATES = {"zero": bytes(32), "ones": b"\xff" * 32}


def elements(tr):
    return np.frombuffer(tr, np.uint64).reshape(-1, 2)


def n_draws(off):
    """challenges of the schedule: r_liu of the output layer; per layer assert_random, one per round of its (up to) three sumchecks, all of sig"""
    n = off.n_layers
    return off.r0[1] + sum(1 + 2 * off.bl[i - 1] + (off.mdb[i] if off.mdb[i] != -1 else 0) + n for i in range(1, n))


def n_rounds(off):
    return sum(2 * off.bl[i - 1] + (off.mdb[i] if off.mdb[i] != -1 else 0) for i in range(1, off.n_layers))


def chain_steps(off):
    """every transcript element absorbed once, every challenge drawn once"""
    return off.n_tr + n_draws(off)


def reference(state, off, tr):
    """(tape, n_draws, closing state) of the schedule from `state` over the transcript bytes tr, with hashlib"""
    assert len(tr) == 16 * off.n_tr
    ch = fs.Chain(state)
    tape = ff.gkr_schedule(ch, off, elements(tr))
    return tape, n_draws(off), ch.s


def statement_state(oc, with_inputs, consts=None, asserts=None):
    """the chain behind verifier::fsInit: the statement digest as one step, then {layers, 0, 0, 0x53}"""
    ch = fs.Chain()
    ch.step(*struct.unpack("<4Q", ff.statement_digest(oc, with_inputs, consts, asserts)))
    ch.step(oc.layers, 0, 0, 0x53)
    return ch.s


def full_fs_head_state(oc, proof):
    """the state in front of a joined proof's GKR section (full_fs_ref.assemble, steps 1 and 2), and that section's bytes"""
    magic, version, n, reps, ms, n_pub = struct.unpack_from("<4I2Q", proof)
    ch = fs.Chain(statement_state(oc, False))
    ch.P(n, reps, ms, n_pub)
    for x in np.frombuffer(proof, np.uint64, 2 * n_pub, 32).reshape(n_pub, 2):
        ch.E(x)
    s = ff.sections(proof)
    ch.D(0, proof[s["root_l"]:s["root_l"] + 32])
    off = gc.Offsets.of(oc)
    assert s["gkr"] + 16 * off.n_tr == s["root_h"]
    return ch.s, proof[s["gkr"]:s["root_h"]]


def rounds_beyond(oc, fused_max):
    """(rounds of the schedule with more pairs than one fused launch takes, all rounds) for the oracle's circuit oc: the pair count of round k of a table of
    `valid` entries and length 2^bl is ceil(ceil(valid / 2^(k-1)) / 2) while 2^bl >> (k - 1) >= 2, else none; a phase-2 round sums its tables' pairs."""
    def pairs(valid, bl, k):
        if ((1 << bl) >> (k - 1)) < 2:
            return 0
        v = -(-valid // (1 << (k - 1)))
        return (v + 1) // 2
    off = gc.Offsets.of(oc)
    sizes = [oc.layer_size(i) for i in range(oc.layers)]
    big = total = 0
    for i in range(off.n_layers - 1, 0, -1):
        pbl = off.bl[i - 1]
        for _ in range(2):                                          # phase 1 and the Liu sumcheck: one table, the previous layer
            for k in range(1, pbl + 1):
                total += 1
                big += pairs(sizes[i - 1], pbl, k) > fused_max
        if off.mdb[i] != -1:
            ds, db, _ = oc.subsets(i)
            for k in range(1, off.mdb[i] + 1):
                total += 1
                big += sum(pairs(ds[j], db[j], k) for j in range(i) if ds[j]) > fused_max
    return big, total
