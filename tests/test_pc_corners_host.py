"""The slice corners of an eq table (csrc/vp_pc_corners.h: corner[i] = eq(point, i 2^(n-6)), what vp_commit_public_eq forms on the host, sharded or not) as a
stand-alone program under -fsanitize=address,undefined: tests/sanitize/pc_corners_main.cpp, plain g++, nothing but the header under test and vp_field.h.
No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_pc_eq_corners_under_asan_ubsan():
    """pc_eq_corners equals entries i N of the textbook eq table (the product over all n bits, in unsigned __int128 arithmetic of the program's own) at
    n = 7, 8, 13, 25, for points that contain 0, 1, p - 1 and complex coordinates with both limbs at p - 1; it writes 64 elements and nothing beside them."""
    out_dir = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "pc_corners_asan")
    src = os.path.join(ROOT, "tests", "sanitize", "pc_corners_main.cpp")
    deps = [src] + [os.path.join(ROOT, "virgo-plus_amd", "csrc", h) for h in ("vp_pc_corners.h", "vp_field.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN + ["-o", exe, src], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and "pc_corners ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
