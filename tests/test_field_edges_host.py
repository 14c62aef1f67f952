"""Host leg of the operand-contract tests ("Operand contracts"): virgo-plus_amd/csrc/vp_field.h is written __host__ __device__, so the
MS = false instantiation of every split form compiles with g++ and runs here without a GPU.  tests/sanitize/field_edges_main.cpp drives each form
with the cross product of boundary operands at the form's STATED range (not [0, p)) plus seeded random operands over that range, against
unsigned __int128 `%` arithmetic; strict forms must give the canonical residue, WEAK forms a congruent value below 2^61 + 4.  Built twice: plain,
and with the sanitizer flags of tests/test_sanitizers.py (an unsigned wrap is not undefined behaviour, so the sanitized run adds what it can: shifts,
conversions, memory).  The device-only forms (c31_add<true>, the lz_* butterflies, the reductions) are tests/test_gpu_field_edges.py."""
import os
import re
import subprocess

import pytest

from test_sanitizers import ENV, SAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sanitize", "field_edges_main.cpp")
HDR = os.path.join(ROOT, "virgo-plus_amd", "csrc", "vp_field.h")
# every form the program must report, with the least number of operand tuples (the boundary cross product alone)
C, CP, L, W = 7, 8, 12, 13          # sizes of the boundary sets: canonical, canonical or p, [0, 2p], < 2^62
FORMS = {"dot2_31<strict>": W ** 4 * 4, "dot2_31<weak>": W ** 4 * 4, "dot2_31c<strict>": CP * W * CP * W * 4, "dot2_31c<weak>": CP * W * CP * W * 4,
         "dot1_31<strict>": W * W * 4, "dot1_31<weak>": W * W * 4, "dot1_31c<strict>": CP * W * 4, "dot1_31c<weak>": CP * W * 4,
         "f_mad31<strict>": L ** 4 * 9, "f_mad31<weak>": L ** 4 * 9, "f_mad31c<strict>": C * C * L * L * 9, "f_mad31c<weak>": C * C * L * L * 9,
         "f_mad31_rb<strict>": L ** 3 * 9, "f_mad31_rb<weak>": L ** 3 * 9, "f_mad31c_rb<strict>": C * C * L * 9, "f_mad31c_rb<weak>": C * C * L * 9,
         "dot4_31cc": C ** 6 * CP ** 2, "f_dot2cc (split wiring)": 5 ** 8, "c31_add<shift>": 60, "m_add / m_sub": 121, "f_half": 121, "f_neg": 121,
         "m_red128": W * W, "f_mul128 / f_mul_plain (host)": C ** 4}


@pytest.mark.parametrize("flavour,flags", [("plain", ["-O2"]), ("sanitized", SAN)])
def test_split_forms_at_the_edges_of_their_ranges(flavour, flags):
    out_dir = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "field_edges_" + flavour)
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in (SRC, HDR, os.path.abspath(__file__))):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, SRC], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=ENV)
    print(r.stdout)
    assert r.returncode == 0 and "field_edges ok" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    seen = {m.group(1).strip(): int(m.group(2)) for m in re.finditer(r"^(.+?)\s+(\d+) tuples$", r.stdout, re.M)}
    for form, least in FORMS.items():
        assert seen.get(form, 0) >= least, (form, seen.get(form), least)
