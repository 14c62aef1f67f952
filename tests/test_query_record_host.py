"""CPU: the record of a complete-protocol run (host/vphost.h: vph_last_full_record) replayed by the host verifier with no GPU and no prover —
the first test of the commitment's verifier (verifier::verifyPoly) that needs no device.  The fixture tests/golden/full_record_custom_a.bin was
written on the GPU box by tests/golden/make_full_record.py (custom_a: n = 10, 4 FRI levels, 2 repetitions)."""
import hashlib
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

NAME = "custom_a"
VAL = 130 * 16


@pytest.fixture(scope="module")
def case(vp, golden):
    import custom_circuits as cc
    g = golden[NAME]
    args = cc.make(g["custom"]["seed"], g["custom"]["sizes"])
    c = vp.Circuit.custom(*args)
    assert c.hash() == g["circuit_hash"]
    rec = open(os.path.join(GOLDEN, "full_record_%s.bin" % NAME), "rb").read()
    meta = json.load(open(os.path.join(GOLDEN, "full_record_%s.json" % NAME)))
    gold = open(os.path.join(GOLDEN, g["transcript"]), "rb").read()
    n, lg, reps = meta["n"], meta["n"] - 6, meta["reps"]
    per_query = 2 * (VAL + 32 * (n - 1)) + sum(VAL + 32 * (n - 2 - k) for k in range(lg))
    sec = {"header": 0, "transcript": 16}
    sec["fft_gkr"] = 16 + len(gold)
    sec["roots"] = sec["fft_gkr"] + 16 * (64 + 3 * (2 * lg * lg + 2 * lg + 6) + 2 + 2 * lg)
    sec["final"] = sec["roots"] + 32 * lg
    sec["openings"] = sec["final"] + 2048 * 16
    sec["end"] = sec["openings"] + reps * per_query
    yield {"c": c, "args": args, "rec": rec, "meta": meta, "gold": gold, "g": g, "sec": sec, "per_query": per_query, "n": n}
    c.close()


def _offsets(case):
    """One byte in each section: header (each word), root_l, a GKR message, root_h, input_0, all_sum, an fft_gkr message, a FRI root, the final
    codeword, a value and a path digest of the first, a middle and the last opening."""
    sec, g, n = case["sec"], case["g"], case["n"]
    tr = sec["transcript"]
    gold_len = len(case["gold"])
    offs = {"magic": 1, "version": 4, "n": 8, "reps": 12, "root_l": tr + 7, "gkr first": tr + g["gkr_slice"][0] + 3,
            "gkr middle": tr + (g["gkr_slice"][0] + g["gkr_slice"][1]) // 2, "gkr last": tr + g["gkr_slice"][1] - 16,
            "root_h": tr + gold_len - (32 + 16 + 65 * 16) + 9, "input_0": tr + gold_len - (16 + 65 * 16) + 2,
            "all_sum first": tr + gold_len - 65 * 16 + 1, "all_sum mask term": tr + gold_len - 16,
            "fft_gkr first": sec["fft_gkr"] + 5, "fft_gkr middle": (sec["fft_gkr"] + sec["roots"]) // 2, "fft_gkr last": sec["roots"] - 16,
            "fri root 0": sec["roots"] + 4, "fri root last": sec["final"] - 1,
            "final first": sec["final"], "final middle": sec["final"] + 1024 * 16 + 8, "final last": sec["openings"] - 16,
            "value l": sec["openings"] + 40, "mask pair l": sec["openings"] + 128 * 16, "path l sibling": sec["openings"] + VAL + 3,
            "path l leaf digest": sec["openings"] + VAL + 32 * (n - 1) - 1,
            "value h": sec["openings"] + VAL + 32 * (n - 1) + 64 * 16,
            "value level 0": sec["openings"] + 2 * (VAL + 32 * (n - 1)) + 16, "path level 0": sec["openings"] + 2 * (VAL + 32 * (n - 1)) + VAL + 33,
            "value last level, second repetition": sec["end"] - 32 * 4 - VAL + 8, "path last digest": sec["end"] - 1}
    return offs


def test_fixture_is_what_its_json_says(case):
    rec, meta, sec = case["rec"], case["meta"], case["sec"]
    assert hashlib.sha256(rec).hexdigest() == meta["sha256"] and len(rec) == meta["bytes"] == sec["end"] < 100 * 1024
    assert struct.unpack("<4I", rec[:16]) == (0x52465056, 1, meta["n"], meta["reps"]) and meta["n"] == 10 and meta["reps"] == 2 and meta["fri_steps"] == 4


def test_record_sections_equal_the_real_references_records(case):
    """The transcript section is tests/golden/transcript_custom_a.bin; the FRI roots and the final codeword are those of fri_custom_a.bin."""
    rec, sec, g = case["rec"], case["sec"], case["g"]
    assert rec[sec["transcript"]:sec["fft_gkr"]] == case["gold"]
    fri = open(os.path.join(GOLDEN, g["fri"]), "rb").read()
    st = g["fri_steps"]
    assert rec[sec["roots"]:sec["final"]] == b"".join(fri[48 * k + 16:48 * k + 48] for k in range(st))
    assert rec[sec["final"]:sec["openings"]] == fri[48 * st:48 * st + 2048 * 16]


def test_record_accepted(case):
    assert case["c"].verify_full_record(case["rec"])
    assert case["c"].verify_full_record(case["rec"])          # the replay reseeds the generator itself: twice the same verdict


def test_record_rejected_with_one_byte_flipped_in_each_section(case):
    c, rec = case["c"], case["rec"]
    for what, off in _offsets(case).items():
        assert 0 <= off < len(rec), what
        for bit in (0x01, 0x80):
            bad = bytearray(rec)
            bad[off] ^= bit
            assert not c.verify_full_record(bytes(bad)), "accepted with a flipped byte: %s (offset %d, bit %#x)" % (what, off, bit)


def test_record_rejected_when_short_long_foreign_or_non_canonical(case):
    c, rec, sec = case["c"], case["rec"], case["sec"]
    assert not c.verify_full_record(rec[:-1])
    assert not c.verify_full_record(rec + b"\0")
    assert not c.verify_full_record(b"") and not c.verify_full_record(rec[:15]) and not c.verify_full_record(rec[:16])
    for cut in sec.values():
        assert not c.verify_full_record(rec[:cut]) or cut == sec["end"]
    assert not c.verify_full_record(rec[:8] + struct.pack("<I", 11) + rec[12:])                  # another circuit's n
    assert not c.verify_full_record(rec[:4] + struct.pack("<I", 2) + rec[8:])                    # another version
    assert not c.verify_full_record(rec[:12] + struct.pack("<I", 1) + rec[16:])                  # fewer repetitions than openings
    assert not c.verify_full_record(rec[:12] + struct.pack("<I", 0xFFFFFFFF) + rec[16:])
    p = (1 << 61) - 1
    for off in (sec["openings"] + 16, sec["final"] + 32, sec["fft_gkr"], sec["fft_gkr"] - 16):   # x + p: the same element, not its canonical form
        x = struct.unpack("<Q", rec[off:off + 8])[0]
        assert x < p
        assert not c.verify_full_record(rec[:off] + struct.pack("<Q", x + p) + rec[off + 8:])
    other = np.random.default_rng(1).integers(0, 256, size=len(rec), dtype=np.uint8).tobytes()
    assert not c.verify_full_record(rec[:16] + other[16:])


def test_record_replay_under_asan_ubsan(case, tmp_path):
    """The same calls from tests/sanitize/record_main.cpp with the host sources under -fsanitize=address,undefined: a record that is tampered
    with, cut at any of the offsets or extended is rejected without one out-of-bounds read."""
    from test_sanitizers import ENV, SAN
    out_dir = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "record_asan")
    host = os.path.join(ROOT, "virgo-plus_amd", "host")
    csrc = os.path.join(ROOT, "virgo-plus_amd", "csrc")
    src = [os.path.join(host, f) for f in ("circuit.cpp", "prover.cpp", "verifier.cpp", "vphost.cpp")] + [os.path.join(ROOT, "tests", "sanitize", "record_main.cpp")]
    deps = src + [os.path.join(host, f) for f in os.listdir(host) if f.endswith((".hpp", ".h"))]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-pthread"] + SAN + ["-o", exe] + src +
                       ["-L" + csrc, "-lvpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    sizes, ty, l, u, v, cp, a = case["args"]
    circ = tmp_path / "circuit.bin"
    circ.write_bytes(struct.pack("<Q", len(sizes)) + sizes.tobytes() + struct.pack("<Q", len(ty)) + ty.tobytes() + l.tobytes() + u.tobytes() + v.tobytes() +
                     np.ascontiguousarray(cp).tobytes() + a.tobytes())
    offs = sorted(set(_offsets(case).values()) | set(case["sec"].values()) - {case["sec"]["end"], 0})
    env = dict(ENV, ASAN_OPTIONS="detect_leaks=0:exitcode=99")
    r = subprocess.run([exe, str(circ), os.path.join(GOLDEN, "full_record_%s.bin" % NAME)] + [str(o) for o in offs],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "record_asan ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_new_entry_points_are_declared_and_exported(vp):
    gpu_hdr = open(os.path.join(ROOT, "include", "vpgpu.h")).read()
    host_hdr = open(os.path.join(ROOT, "virgo-plus_amd", "host", "vphost.h")).read()
    for lib, hdr, names in ((vp.LIB_GPU, gpu_hdr, ("vp_fri_open_many", "vp_fri_query_bytes", "vp_fri_query")),
                            (vp.LIB_HOST, host_hdr, ("vph_prove_and_verify_full_ex", "vph_last_full_record", "vph_verify_full_record"))):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in names:
            assert re.search(r"\b%s\s*\(" % s, hdr), s + " is not declared"
            assert re.search(r" T %s$" % s, out, flags=re.M), s + " is not exported"
    assert "VPH_VERIFY_BATCHED_OPENINGS" in host_hdr and "VP_K_PC_OPEN_MANY, VP_K_COUNT" in gpu_hdr
    lib = vp.lib_gpu()
    kinds = re.search(r"enum \{ (VP_K_BETA = 0.*?), VP_K_COUNT \}", gpu_hdr, flags=re.S).group(1).replace(" = 0", "").split(",")
    assert lib.vp_kernel_name([k.strip() for k in kinds].index("VP_K_PC_OPEN_MANY")) == b"k_pc_open_many"
    for m in ("fri_open_many", "fri_query", "last_full_record"):
        assert hasattr(vp.Session, m)
    assert hasattr(vp.Circuit, "verify_full_record") and hasattr(vp.ShardedCommitment, "open_many")
