#!/usr/bin/env python3
"""The proof-of-work search on the device (vp_fs_grind, k_fs_grind) measured: the record is profiles/fs_grind.md.
    python tools/fs_grind_rate.py all [OUT.md]        every step below, each a child process under its own `timeout`, in order; stops at the first that fails
    python tools/fs_grind_rate.py rate [BLOCKS]       the yardstick and the search in ONE process, alternated three times: Keccak-f/s of k_leaf_hash in a profiled
                                                      commit_private of the SHA-256 x BLOCKS input layer (leaves x 65 permutations over the kernel's time: the
                                                      roofline leg of bench.py --full), and of k_fs_grind over a range of 2^32 nonces that holds no hit (48 bits), every
                                                      nonce counted from the launch table's `work`; the rate per window size; the same range unprofiled by the wall clock
    python tools/fs_grind_rate.py hit BITS [STATES]   wall time of Session.fs_grind to a hit at BITS bits on STATES states, against 2^BITS / rate
    python tools/fs_grind_rate.py schedule            the window schedule: (grind_window_log, grind_batch) alternatives, a context each, time to a hit at 8, 16, 24
                                                      bits and the rate over 2^32 nonces
    python tools/fs_grind_rate.py reps N              proof bytes and verifier time of one repetition of the commitment proof of an input layer of 2^N wires
Prints markdown."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (arguments, seconds): a step that runs longer is ended, and nothing is started behind it
STEPS = [(["rate", "1024"], 240), (["hit", "8"], 60), (["hit", "16"], 60), (["hit", "20"], 60), (["hit", "24"], 90), (["hit", "28"], 180), (["hit", "32", "3"], 420),
         (["schedule"], 300), (["reps", "16"], 300), (["reps", "20"], 420)]


def load():
    sys.path.insert(0, ROOT)
    import vp_loader
    vp = vp_loader.load()
    vp.lib_host()
    return vp


def sha_circuit(vp, blocks):
    import gzip
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        pws = os.path.join(tmp, "s.pws")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "SHA256_64.pws.gz"), "rb") as f, open(pws, "wb") as o:
            o.write(f.read())
        return vp.Circuit.from_pws(pws, blocks, seed=1)


def state(i):
    import hashlib
    return hashlib.sha3_256(b"fs_grind_rate %d" % i).digest()


def grind_rows(s, st, bits, tries):
    """one profiled search that finds nothing: the rows of its launch table"""
    s.set_profiling(1)
    try:
        s.fs_grind(st, bits, max_tries=tries)
        raise SystemExit("a %d-bit hit in 2^32 nonces: take another state" % bits)
    except RuntimeError:
        pass
    rows = [r for r in s.launch_stats() if r["kernel"] == "k_fs_grind"]
    s.set_profiling(0)
    return rows


def rate(blocks):
    vp = load()
    c = sha_circuit(vp, blocks)
    s = vp.Session(c)
    n = c.layer_bitlen(0)
    s.commit_private(); s.fs_grind(state(0), 8)                                       # warm-up: tables, buffers, code objects
    print("## the rate: k_fs_grind against k_leaf_hash in one process (SHA-256 x%d, n = %d), alternated\n" % (blocks, n))
    print("| run | k_leaf_hash: Keccak-f | ms | G Keccak-f/s | k_fs_grind: nonces | ms (kernels) | G Keccak-f/s | the same range unprofiled: wall ms | G/s |")
    print("|---|---|---|---|---|---|---|---|---|")
    leaf_r, grind_r, by_size = [], [], {}
    for run in range(3):
        s.set_profiling(1)
        s.commit_private()
        leaf = [r for r in s.launch_stats() if r["kernel"] == "k_leaf_hash"]
        s.set_profiling(0)
        lw, lus = sum(r["work"] for r in leaf), sum(r["us"] for r in leaf)
        rows = grind_rows(s, state(run), 48, 1 << 32)
        gw, gus = sum(r["work"] for r in rows), sum(r["us"] for r in rows)
        assert gw == 1 << 32, "not every nonce of the range was tried"
        for r in rows:
            by_size.setdefault(r["work"], []).append(r["work"] / r["us"] * 1e-3)
        t0 = time.perf_counter()
        try:
            s.fs_grind(state(run), 48, max_tries=1 << 32)
        except RuntimeError:
            pass
        wall = time.perf_counter() - t0
        leaf_r.append(lw / lus * 1e-3); grind_r.append(gw / gus * 1e-3)
        print("| %d | %d | %.3f | %.2f | %d | %.3f | %.2f | %.3f | %.2f |" % (run, lw, lus * 1e-3, leaf_r[-1], gw, gus * 1e-3, grind_r[-1], 1e3 * wall, (1 << 32) / wall * 1e-9))
    print("\nmedian: k_leaf_hash %.2f, k_fs_grind %.2f G Keccak-f/s; ratio %.3f\n" % (statistics.median(leaf_r), statistics.median(grind_r),
                                                                                     statistics.median(grind_r) / statistics.median(leaf_r)))
    print("| window (nonces) | launches | G Keccak-f/s: median | min | max |")
    print("|---|---|---|---|---|")
    for size in sorted(by_size):
        v = by_size[size]
        print("| 2^%.0f | %d | %.2f | %.2f | %.2f |" % (__import__("math").log2(size), len(v), statistics.median(v), min(v), max(v)))
    print("\nRATE %.4f" % statistics.median(grind_r))


def hit(bits, n_states):
    vp = load()
    c = vp.Circuit.randomize(3, 7, seed=11)
    s = vp.Session(c)
    s.fs_grind(state(0), 8)
    print("## time to a hit at %d bits (Session.fs_grind from nonce 0, wall clock), %d states\n" % (bits, n_states))
    print("| state | nonce | nonce / 2^bits | ms | G nonces/s |")
    print("|---|---|---|---|---|")
    ms, per = [], []
    for i in range(n_states):
        t0 = time.perf_counter()
        nonce, out = s.fs_grind(state(100 + i), bits)
        dt = time.perf_counter() - t0
        assert out == vp.fs_grind_host(state(100 + i), bits, first=nonce, max_tries=1)[1], "the host's step on the device's nonce"
        ms.append(1e3 * dt); per.append(1e3 * dt / ((nonce + 1) / 2.0 ** bits))
        print("| %d | %d | %.3f | %.3f | %.2f |" % (i, nonce, nonce / 2.0 ** bits, 1e3 * dt, (nonce + 1) / dt * 1e-9))
    print("\nmedian %.3f ms, mean %.3f ms; scaled to a nonce of exactly 2^bits: median %.3f ms\n" % (statistics.median(ms), statistics.mean(ms), statistics.median(per)))


def schedule():
    vp = load()
    c = vp.Circuit.randomize(3, 7, seed=11)
    print("## the window schedule: windows of 2^16 x 4^w nonces up to 2^grind_window_log, grind_batch windows per host wait; a context each\n")
    print("| window log | batch | 8 bits: median ms of 9 | 16 bits | 24 bits | 2^32 nonces without a hit: ms | G/s |")
    print("|---|---|---|---|---|---|---|")
    for wl, batch in ((24, 8), (16, 1), (16, 8), (20, 8), (24, 1), (24, 2), (24, 32), (28, 8)):
        os.environ["VP_GRIND_WINDOW_LOG"], os.environ["VP_GRIND_BATCH"] = str(wl), str(batch)
        s = vp.Session(c)
        s.fs_grind(state(0), 8)
        cells = []
        for bits in (8, 16, 24):
            t = []
            for i in range(9):
                t0 = time.perf_counter()
                s.fs_grind(state(200 + i), bits)
                t.append(1e3 * (time.perf_counter() - t0))
            cells.append("%.3f" % statistics.median(t))
        t0 = time.perf_counter()
        try:
            s.fs_grind(state(1), 48, max_tries=1 << 32)
        except RuntimeError:
            pass
        dt = time.perf_counter() - t0
        print("| %d | %d | %s | %.1f | %.2f |" % (wl, batch, " | ".join(cells), 1e3 * dt, (1 << 32) / dt * 1e-9))
        s.close()
    print()


def reps(n):
    import numpy as np
    vp = load()
    c = vp.Circuit.randomize(3, n, seed=1)
    assert c.layer_bitlen(0) == n
    s = vp.Session(c)
    point = np.random.default_rng(5).integers(0, (1 << 61) - 1, size=(n, 2), dtype=np.uint64)
    per_rep = vp.lib_host().vph_pc_query_answer_bytes(n, 1)
    print("## one repetition at n = %d (Circuit.randomize(3, %d))\n" % (n, n))
    print("proof bytes per repetition (vph_pc_query_answer_bytes(n, 1)): %d = %d openings of 2080 bytes + their Merkle paths\n" % (per_rep, n - 4))
    proofs = {r: s.commit_fs(point, reps=r, pow_bits=8) for r in (8, 40)}
    print("| verifier | 8 repetitions: ms | 40 repetitions: ms | per repetition: ms |")
    print("|---|---|---|---|")
    for dev in (0, None):
        t = {}
        for r, proof in proofs.items():
            best = []
            for _ in range(3):
                t0 = time.perf_counter()
                ok, why = vp.Circuit.verify_commitment_fs(proof, device=dev, min_pow_bits=8)
                best.append(1e3 * (time.perf_counter() - t0))
                assert ok, why
            t[r] = statistics.median(best)
        print("| %s | %.1f | %.1f | %.2f |" % ("heavy loops on the device" if dev == 0 else "host alone", t[8], t[40], (t[40] - t[8]) / 32))
    print("\nproof: %d bytes at 8 repetitions, %d at 40; a bit of work adds none\n" % (len(proofs[8]), len(proofs[40])))


def run_all(out):
    text = []
    for args, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        text.append(r.stdout)
        if out:
            open(out, "w").write("".join(text))
        print(r.stdout, flush=True)
        if r.returncode != 0:
            print("step %r ended with status %d; nothing is started behind it\n%s" % (args, r.returncode, r.stderr[-2000:]), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.stdout.reconfigure(line_buffering=True)                   # a step ended at its time limit keeps what it had printed
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what == "all":
        sys.exit(run_all(sys.argv[2] if len(sys.argv) > 2 else None))
    elif what == "rate":
        rate(int(sys.argv[2]) if len(sys.argv) > 2 else 1024)
    elif what == "hit":
        hit(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 9)
    elif what == "schedule":
        schedule()
    elif what == "reps":
        reps(int(sys.argv[2]))
    else:
        sys.exit(__doc__)
