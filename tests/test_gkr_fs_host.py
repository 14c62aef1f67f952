"""CPU: the GKR part of the Fiat-Shamir chain by value (vph_gkr_fs_tape, Circuit.gkr_fs_tape; the schedule: host/vphost.h, "The GKR part on the device") — the walk
the host holds vp_prove_gkr_fs to, without a device.

The reference is tests/full_fs_ref.py's gkr_schedule with hashlib (tests/gkr_fs_cases.py).  The transcripts are GKR proofs that exist without this change: the GKR
sections of the two recorded joined proofs under tests/golden/ (from the state behind their heads) and the oracle's own Fiat-Shamir proof (orc_prove_fs, from the
statement with the input values).

  derivation   tape by slot, number of draws and closing state equal the hashlib schedule's; the drawn slots are the ones orc_prove_gkr_tape reads plus the rest of
               sig, every other slot is zero; the oracle's tape-form prover returns the transcript on the derived tape (the induction's other half)
  sensitivity  one changed transcript element leaves every draw in front of it and moves every draw behind it, and the state; another start state moves everything
  malformed    a truncated or over-long transcript, a non-canonical limb, a state that is not 32 bytes: ValueError
  symbols      the new entries are declared and exported; the declarations of vph_prove_fs, vph_prove_full_fs, vp_prove_gkr and vp_fft_gkr_fs are the ones they were
  sanitizers   tests/sanitize/gkr_fs_main.cpp: the derivation under ASan / UBSan as a stand-alone program"""
import os
import re
import subprocess

import numpy as np
import pytest

import full_fs_ref as ff
import gkr_fs_cases as gf
import gkr_tape_cases as gc
from conftest import ROOT

P = ff.P


def cases(vp, ob):
    """(name, circuit, oracle circuit, start state, transcript) of every recorded transcript"""
    out = []
    for masked in (False, True):
        _, layers, log_size, seed, _ = ff.FIXTURE_MASKED if masked else ff.FIXTURE
        oc = ob.Circuit.randomize(layers, log_size, seed=seed)
        state, tr = gf.full_fs_head_state(oc, ff.fixture(masked))
        out.append(("joined proof, ms = 8" if masked else "joined proof, zero mask", vp.Circuit.randomize(layers, log_size, seed=seed), oc, state, tr))
    _, layers, log_size, seed, _ = ff.FIXTURE
    oc = ob.Circuit.randomize(layers, log_size, seed=seed)
    proof, _ = oc.prove_fs()
    out.append(("orc_prove_fs", vp.Circuit.randomize(layers, log_size, seed=seed), oc, gf.statement_state(oc, True), proof))
    return out


@pytest.fixture(scope="module")
def recorded(vp, ob):
    cs = cases(vp, ob)
    yield cs
    for _, c, _, _, _ in cs:
        c.close()


def test_the_derivation_is_the_hashlib_schedule(vp, recorded):
    for name, c, oc, state, tr in recorded:
        off = gc.Offsets.of(oc)
        assert c.gkr_sizes() == (off.n, 16 * off.n_tr), name
        tape, draws, st = c.gkr_fs_tape(tr, state)
        want, want_draws, want_st = gf.reference(state, off, tr)
        assert tape.shape == (off.n, 2) and int(tape.max()) < P
        bad = [i for i in range(off.n) if tape[i].tobytes() != want[i].tobytes()]
        assert not bad, "%s: tape slots %r are not the schedule's" % (name, bad[:8])
        assert draws == want_draws and st == want_st, name
        # where the draws went: every slot the tape-form prover reads, the whole of sig, nothing else
        drawn = np.zeros(off.n, bool)
        for s, used, _ in off.vectors():
            drawn[s:s + used] = True
        for i in range(1, off.n_layers):
            drawn[off.ar[i][0]] = True
            drawn[off.sig[i][0]:off.sig[i][0] + off.n_layers] = True
        assert int(drawn.sum()) == draws and not tape[~drawn].any() and tape[drawn].any(axis=1).all(), name
        assert len({tape[i].tobytes() for i in np.flatnonzero(drawn)}) == draws, name + ": two slots hold the same draw"
        # the induction's other half: the tape-form prover gives these bytes back on this tape
        assert oc.prove_gkr_tape(tape)[0] == tr, name


def test_one_changed_element_moves_every_later_draw_and_the_state(vp, recorded):
    name, c, oc, state, tr = recorded[0]
    off = gc.Offsets.of(oc)
    tape, draws, st = c.gkr_fs_tape(tr, state)
    # the order the schedule draws in, from the reference run with a counter in place of the chain
    order = []

    class Count:
        s = state

        def E(self, x):
            pass

        def C(self, k):
            order.append(k)
            return (k + 1, 0)
    marks = ff.gkr_schedule(Count(), off, gf.elements(tr))
    slot_of = {int(marks[i][0]) - 1: i for i in range(off.n) if int(marks[i][0])}
    assert sorted(slot_of) == list(range(draws)) == order
    _, mid_start, mid_rounds, _ = [p for p in off.parts if p[0] == "Liu"][0][1:]
    for what, elem in (("Vres", 0), ("a round polynomial's b", mid_start + 1), ("a claim", mid_start + 3 * mid_rounds), ("the last element", off.n_tr - 1)):
        bad = bytearray(tr)
        bad[16 * elem] ^= 0x04
        t2, d2, s2 = c.gkr_fs_tape(bytes(bad), state)
        want, _, want_st = gf.reference(state, off, bytes(bad))
        assert t2.tobytes() == want.tobytes() and s2 == want_st and d2 == draws and s2 != st, what
        same = [k for k in range(draws) if t2[slot_of[k]].tobytes() == tape[slot_of[k]].tobytes()]
        assert same == list(range(len(same))), what + ": a draw behind a moved one stayed"
        if elem == 0:
            assert len(same) == off.r0[1], "only r_liu of the output layer precedes Vres"
        if elem == off.n_tr - 1:
            assert len(same) == draws, "nothing is drawn behind the last element: only the state moves"
        else:
            assert len(same) < draws, what
    for other in gf.START_STATES.values():
        t2, _, s2 = c.gkr_fs_tape(tr, other)
        assert s2 != st and all(t2[slot_of[k]].tobytes() != tape[slot_of[k]].tobytes() for k in range(draws))


def test_malformed_transcripts_are_refused(vp, recorded):
    name, c, oc, state, tr = recorded[0]
    limb = lambda off, v: tr[:off] + int(v).to_bytes(8, "little") + tr[off + 8:]
    bad = {"empty": b"", "short by a byte": tr[:-1], "short by an element": tr[:-16], "long by a byte": tr + b"\0", "long by an element": tr + bytes(16),
           "a limb = p": limb(16, P), "an imaginary limb = p": limb(len(tr) - 8, P), "a limb = 2^64 - 1": limb(40, (1 << 64) - 1)}
    for what, x in bad.items():
        with pytest.raises(ValueError):
            c.gkr_fs_tape(x, state)
            pytest.fail(what)
    for st in (b"", bytes(31), bytes(33)):
        with pytest.raises(ValueError):
            c.gkr_fs_tape(tr, st)
    assert c.gkr_fs_tape(limb(16, P - 1), state)[1] == gf.n_draws(gc.Offsets.of(oc)), "p - 1 is canonical"
    import ctypes
    L, nd = vp.lib_host(), ctypes.c_uint64(0)
    buf, so = ctypes.create_string_buffer(tr, len(tr)), ctypes.create_string_buffer(32)
    tape = np.zeros((gc.Offsets.of(oc).n, 2), np.uint64)
    args = [c.h, ctypes.cast(ctypes.create_string_buffer(state, 32), ctypes.c_void_p), ctypes.cast(buf, ctypes.c_void_p), len(tr), tape.ctypes.data, ctypes.byref(nd),
            ctypes.cast(so, ctypes.c_void_p)]
    assert L.vph_gkr_fs_tape(*args) == 0
    for k in (0, 1, 2, 4, 6):
        a = list(args)
        a[k] = None
        assert L.vph_gkr_fs_tape(*a) == -1, "null argument %d" % k


def test_new_symbols_are_declared_and_exported_and_the_old_declarations_stand(vp):
    host_hdr = open(os.path.join(ROOT, "virgo-plus_amd", "host", "vphost.h")).read()
    gpu_hdr = open(os.path.join(ROOT, "include", "vpgpu.h")).read()
    host = subprocess.run(["nm", "-D", "--defined-only", vp.LIB_HOST], stdout=subprocess.PIPE, text=True, check=True).stdout
    gpu = subprocess.run(["nm", "-D", "--defined-only", vp.LIB_GPU], stdout=subprocess.PIPE, text=True, check=True).stdout
    for s in ("vph_gkr_sizes", "vph_gkr_fs_tape", "vph_prove_gkr_fs", "vph_prove_fs_ex", "vph_prove_full_fs_ex"):
        assert re.search(r"\b%s\s*\(" % s, host_hdr), s + " is not declared"
        assert re.search(r" T %s$" % s, host, flags=re.M), s + " is not exported"
    assert re.search(r"\bvp_prove_gkr_fs\s*\(", gpu_hdr) and re.search(r" T vp_prove_gkr_fs$", gpu, flags=re.M)
    assert "The GKR part on the device" in host_hdr and re.search(r"VPH_FS_DEVICE_GKR\s*=\s*2\b", host_hdr)
    for name in ("prove_gkr_fs", "prove_fs", "prove_full_fs"):
        assert hasattr(vp.Session, name)
    assert hasattr(vp.Circuit, "gkr_fs_tape")
    import inspect
    assert inspect.signature(vp.Session.prove_fs).parameters["device_draws"].default is False
    assert inspect.signature(vp.Session.prove_full_fs).parameters["device_gkr"].default is False
    # the declarations other code is built against, character for character
    assert "int vph_prove_fs(vph_session *, uint8_t *proof, uint64_t capacity, uint64_t *n_written, vph_result *res, char *err, int errlen);" in host_hdr
    assert ("int vph_prove_full_fs(vph_session *, int reps, const uint64_t *mask_pairs, uint64_t n_mask, const uint64_t *pub_mask_pairs, uint64_t n_pub_mask, uint8_t *out, uint64_t cap,\n"
            "                      uint64_t *len, uint64_t *point_pairs /* n, or null */, char *err, int errlen);") in host_hdr
    assert ("int vp_prove_gkr(vp_ctx *, const vp_F *tape, uint64_t n_tape, uint8_t *transcript, uint64_t capacity,\n"
            "                 uint64_t *n_written);") in gpu_hdr
    assert ("int vp_fft_gkr_fs(vp_ctx *, int lg, const uint8_t state_in[32], vp_F *msgs, uint64_t capacity, uint64_t *n_written,\n"
            "                  vp_F *tape_out /* vp_fft_gkr_sizes' n_tape */, uint8_t state_out[32]);") in gpu_hdr


def test_derivation_under_asan_ubsan(vp, recorded, tmp_path):
    """tests/sanitize/gkr_fs_main.cpp with the host sources, -fsanitize=address,undefined: the recorded transcript derived (and compared with Circuit.gkr_fs_tape's
    answer), then every length around it and non-canonical limbs on heap copies exactly as long as what they hold — each must end in a verdict, none in a report"""
    name, c, oc, state, tr = recorded[0]
    tape, draws, st = c.gkr_fs_tape(tr, state)
    (tmp_path / "tr.bin").write_bytes(tr)
    (tmp_path / "state.bin").write_bytes(state)
    (tmp_path / "want.bin").write_bytes(tape.tobytes() + st)
    out_dir = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "gkr_fs_asan")
    host = os.path.join(ROOT, "virgo-plus_amd", "host")
    csrc = os.path.join(ROOT, "virgo-plus_amd", "csrc")
    src = [os.path.join(host, f) for f in ("circuit.cpp", "prover.cpp", "verifier.cpp", "vphost.cpp")] + [os.path.join(ROOT, "tests", "sanitize", "gkr_fs_main.cpp")]
    deps = src + [os.path.join(host, f) for f in os.listdir(host) if f.endswith((".hpp", ".h"))]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-pthread"] + san + ["-o", exe] + src + ["-L" + csrc, "-lvpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    args = [str(v) for v in ff.FIXTURE[1:4]] + [str(tmp_path / "tr.bin"), str(tmp_path / "state.bin"), str(tmp_path / "want.bin"), str(draws)]
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "gkr_fs_asan ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
