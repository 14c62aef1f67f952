"""The live-slice rule of the commitment (csrc/vp_pc_live.h: which of the 64 input-layer slices hold anything, and how the real-pair encode pairs them) as a
stand-alone program under -fsanitize=address,undefined: tests/sanitize/pc_live_main.cpp, plain g++, nothing but the header under test.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_pc_live_rule_under_asan_ubsan():
    """live against a slice-by-slice count at every bit length 7 .. 25 with n_used on and beside each slice boundary; the pairs cover 0 .. live - 1 once each, no
    index reaches 64, a full layer pairs 32 / 32, the switch restores 64."""
    out_dir = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "pc_live_asan")
    src = os.path.join(ROOT, "tests", "sanitize", "pc_live_main.cpp")
    deps = [src, os.path.join(ROOT, "virgo-plus_amd", "csrc", "vp_pc_live.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN + ["-o", exe, src], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and "pc_live ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
