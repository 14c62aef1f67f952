"""CPU: fft_gkr's part of the Fiat-Shamir chain (host/vphost.h, "The transcript chain: fft_gkr") without a device.

  the Python prover      fft_gkr_fs_ref.prove at lg 1 .. 6 from three start states (all zero, all 0xff, a hash): its tape and closing state are the hashlib
                         derivation's from its own messages; Circuit.fft_gkr_fs_tape (vph_fft_gkr_fs_tape) returns the same tape and state; the oracle on that
                         tape (orc_fft_gkr_tape) returns the same messages and its embedded verifier accepts; the host's fft_gkr_check accepts
  binding                one changed message element (kept canonical) changes every slot drawn after it, leaves every slot before it, and the changed pair is
                         rejected by fft_gkr_check; another start state gives another tape
  the schedule           a draw never precedes the polynomial it challenges; every message is absorbed once and every slot drawn once
  malformed              lg outside 1..19, a wrong message count, a limb >= p, a short state: ValueError
  sanitizers             tests/sanitize/fft_gkr_fs_main.cpp: the host's derivation and fft_gkr_check as a stand-alone program under ASan / UBSan on exact-size heap
                         blocks: the honest transcript, a stride of changed messages, wrong sizes — its tape and state are hashlib's
  headers and symbols    declared in both headers, exported; the tail's table size follows from 160 KB of LDS and three tables; the launch-table rules of the
                         header give tail-only sumchecks up to 2^T entries"""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fft_gkr_fs_cases as fc
import fft_gkr_fs_ref as fr
import fft_gkr_ref as ref
from conftest import ROOT

P = ref.P


@pytest.mark.parametrize("state", fc.STATES)
@pytest.mark.parametrize("lg", fc.REF_LGS)
def test_python_prover_derivation_oracle_and_check_agree(vp, ob, lg, state):
    msgs, tape, st = fc.python_fs(lg, state)
    s0 = fr.START_STATES[state]
    fc.assert_honest(lg, s0, msgs, tape, st)
    t_c, st_c = vp.Circuit.fft_gkr_fs_tape(lg, s0, msgs)
    assert t_c.tobytes() == tape.tobytes() and st_c == st
    raw, verified = ob.fft_gkr_tape(lg, tape)
    assert raw == msgs.tobytes(), "the oracle on the derived tape: other messages"
    assert verified, "the oracle's embedded verifier rejects the derived transcript"
    assert vp.Circuit.fft_gkr_check(lg, tape, msgs) is True


def test_start_states_give_different_transcripts():
    for lg in (1, 4):
        tapes = {fc.python_fs(lg, s)[1].tobytes() for s in fc.STATES}
        finals = {fc.python_fs(lg, s)[2] for s in fc.STATES}
        assert len(tapes) == len(finals) == len(fc.STATES)


@pytest.mark.parametrize("lg", [1, 4])
def test_one_changed_message_element_moves_every_later_draw_and_is_rejected(vp, lg):
    msgs, tape, st = fc.python_fs(lg, "random")
    s0 = fr.START_STATES["random"]
    n = ref.n_msgs(lg)
    # an output, coefficients of the addition layer's first and last round, the multiplication layer's value, a depth's phase-1 value, the last element
    picks = sorted({0, 63, 64, 64 + 3 * (lg + 6) - 1, 64 + 3 * (lg + 6) + 1 + 3 * lg, 64 + 3 * (lg + 6) + 1 + 3 * lg + 1 + 3 * lg, n - 1})
    for i in picks:
        bad = np.array(msgs)
        bad[i, 0] = (int(bad[i, 0]) + 1) % P                     # canonical, and another element
        t_bad, st_bad = vp.Circuit.fft_gkr_fs_tape(lg, s0, bad)
        t_py, st_py = fr.derive(lg, s0, bad)
        assert t_bad.tobytes() == np.array(t_py, np.uint64).tobytes() and st_bad == st_py
        after = set(fr.slots_after(lg, i))
        for slot in range(ref.n_tape(lg)):
            same = t_bad[slot].tobytes() == tape[slot].tobytes()
            assert same == (slot not in after), "message %d, slot %d" % (i, slot)
        assert st_bad != st
        assert vp.Circuit.fft_gkr_check(lg, t_bad, bad) is False, "message %d changed: accepted with the tape it derives" % i
        assert vp.Circuit.fft_gkr_check(lg, tape, bad) is False, "message %d changed: accepted with the honest tape" % i


@pytest.mark.parametrize("lg", [1, 2, 6, 11, 17, 19])
def test_schedule_never_draws_ahead_of_the_polynomial(lg):
    ops = fr.schedule(lg)
    assert len(ops) == fr.chain_steps(lg) == ref.n_msgs(lg) + ref.n_tape(lg)
    assert [i for k, i in ops if k == "E"] == list(range(ref.n_msgs(lg)))
    L = fr.Layout(lg)
    at = {op: j for j, op in enumerate(ops)}
    pos = 64
    for rounds, slot0 in [(lg + 6, L.ru_a), (lg, L.ru_m)] + [(lg, s) for d in range(lg) for s in (L.ru_d(d), L.rv_d(d))]:
        for k in range(rounds):
            assert at[("E", pos + 3 * k + 2)] + 1 == at[("C", slot0 + k)], "challenge k directly behind the polynomial of round k"
        pos += 3 * rounds + 1
    assert max(at[("C", s)] for s in range(L.x + 64)) < at[("E", 0)] < at[("E", 63)] < at[("C", L.r0)]


def test_malformed_arguments_are_refused(vp):
    msgs, tape, _ = fc.python_fs(2, "zero")
    s0 = fr.START_STATES["zero"]
    limb = np.array(msgs); limb[5, 1] = P
    big = np.array(msgs); big[ref.n_msgs(2) - 1, 0] = (1 << 64) - 1
    for what, args in {"lg = 0": (0, s0, msgs), "lg = 20": (20, s0, msgs), "another size's messages": (3, s0, msgs), "short by one": (2, s0, msgs[:-1]),
                       "a limb = p": (2, s0, limb), "a limb = 2^64 - 1": (2, s0, big), "a 31-byte state": (2, s0[:31], msgs)}.items():
        with pytest.raises(ValueError):
            vp.Circuit.fft_gkr_fs_tape(*args)
            pytest.fail(what)
    with pytest.raises(ValueError):
        vp.Circuit.fft_gkr_check(2, tape[:-1], msgs)
    with pytest.raises(ValueError):
        vp.Circuit.fft_gkr_check(2, tape, limb)


def test_new_symbols_are_declared_and_exported(vp):
    gpu_hdr = open(os.path.join(ROOT, "include", "vpgpu.h")).read()
    host_hdr = open(os.path.join(ROOT, "virgo-plus_amd", "host", "vphost.h")).read()
    for lib, hdr, names in ((vp.LIB_GPU, gpu_hdr, ("vp_fft_gkr_fs",)), (vp.LIB_HOST, host_hdr, ("vph_fft_gkr_fs_tape", "vph_fft_gkr_check", "vph_fft_gkr_fs"))):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in names:
            assert re.search(r"\b%s\s*\(" % s, hdr), s + " is not declared"
            assert re.search(r" T %s$" % s, out, flags=re.M), s + " is not exported"
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", gpu_hdr, flags=re.S))
    assert ("int vp_fft_gkr_fs(vp_ctx *, int lg, const uint8_t state_in[32], vp_F *msgs, uint64_t capacity, uint64_t *n_written, vp_F *tape_out , "
            "uint8_t state_out[32]);") in flat
    assert "The transcript chain: fft_gkr" in host_hdr
    assert hasattr(vp.Session, "fft_gkr_fs") and hasattr(vp.Circuit, "fft_gkr_fs_tape") and hasattr(vp.Circuit, "fft_gkr_check")


def test_tail_size_follows_from_lds_and_table_count():
    """T = the largest table size at which V, M and A (16-byte elements) fit the 160 KB of LDS of a workgroup with 1 KB left for the reduction: 2^11.  With it the
    header's launch-table rules give: every sumcheck of lg <= T - 6 tail-only, the addition layer alone above the tail for T - 5 <= lg <= T."""
    T = fc.tail_log()
    assert 3 * 16 * (1 << T) <= 160 * 1024 - 1024 < 3 * 16 * (1 << (T + 1)) and T == 11
    kinds = lambda lg: [r[0] for r in fc.expected_rows(lg, T)]
    assert "k_round" not in kinds(T - 6) and kinds(T - 6).count("k_seg_multi") == 2 + 2 * (T - 6)
    assert kinds(T - 5).count("k_round") == 1 and kinds(T).count("k_round") == 6
    assert kinds(T + 1).count("k_round") == 7 + (1 + 2 * (T + 1))
    assert sum(r[1] for r in fc.expected_rows(17, T) if r[0] != "k_emit_multi") == sum(fc.sumcheck_rounds(17)) == 2 * 17 * 17 + 2 * 17 + 6


@pytest.mark.parametrize("lg,state", [(1, "ones"), (5, "random")])
def test_derivation_and_check_under_asan_ubsan(ob, tmp_path, lg, state):
    """tests/sanitize/fft_gkr_fs_main.cpp (header code only: it compiles in seconds), -fsanitize=address,undefined: must end in its verdict, not in a report"""
    msgs, tape, st = fc.python_fs(lg, state)
    src = os.path.join(ROOT, "tests", "sanitize", "fft_gkr_fs_main.cpp")
    host = os.path.join(ROOT, "virgo-plus_amd", "host")
    out_dir = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "fft_gkr_fs_asan")
    deps = [src] + [os.path.join(host, f) for f in ("fft_gkr_fs.hpp", "fft_gkr_verify.hpp", "field.hpp", "sha3.hpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-Wall"] + san + ["-o", exe, src], check=True)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<I", lg) + fr.START_STATES[state] + msgs.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(fin), str(fout)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "fft_gkr_fs_asan ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert fout.read_bytes() == tape.tobytes() + st
