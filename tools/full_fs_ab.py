#!/usr/bin/env python3
"""The joined non-interactive proof against the sum of its parts, alternated in one process:
    python tools/full_fs_ab.py BLOCKS [REPEATS] [--cold]
Session.prove_full_fs on the SHA-256 x BLOCKS circuit against prove_fs + commit_fs (at a fixed point) + vp_fft_gkr on a tape — the three pieces a caller had before
the joined proof, which bind nothing to each other — after one warm-up of each; host wall clock per run.  The joined proof's fft_gkr draws its challenges on the
device (tools/fft_gkr_fs_ab.py has that gap on its own).  --cold: no warm-up proofs and no verification in front of the runs (a proof of a large circuit takes
most of a minute; the first row then carries the first-use costs).  Prints markdown, each row as soon as it is measured."""
import gzip
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(blocks, repeats, cold):
    sys.path.insert(0, ROOT)
    import ctypes
    import numpy as np
    import vp_loader
    vp = vp_loader.load()
    with tempfile.TemporaryDirectory() as tmp:
        pws = os.path.join(tmp, "s.pws")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "SHA256_64.pws.gz"), "rb") as f, open(pws, "wb") as o:
            o.write(f.read())
        c = vp.Circuit.from_pws(pws, blocks, seed=1)
    n = c.layer_bitlen(0)
    lg = n - 6
    point = np.random.default_rng(5).integers(0, (1 << 61) - 1, size=(n, 2), dtype=np.uint64)
    tape = np.random.default_rng(6).integers(0, (1 << 61) - 1, size=(2 * lg * lg + 9 * lg + 96, 2), dtype=np.uint64)
    msgs = np.zeros((84 + 6 * lg * lg + 8 * lg, 2), np.uint64)
    s = vp.Session(c)
    L, ctx = vp.lib_gpu(), vp.lib_host().vph_session_ctx(s.h)

    def timed(fn):
        t = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t)

    def fft():
        nw = ctypes.c_uint64(0)
        assert L.vp_fft_gkr(ctx, lg, tape.ctypes.data, tape.shape[0], msgs.ctypes.data, msgs.shape[0], ctypes.byref(nw)) == 0

    if not cold:
        proof = s.prove_full_fs()
        assert c.verify_full_fs(proof) == (True, "")
        s.prove_fs(); s.commit_fs(point); fft()
    print("## x%d (n = %d, fft_gkr at lg = %d), %d alternated runs%s, host ms\n" % (blocks, n, lg, repeats, ", no warm-up" if cold else ""))
    print("| run | prove_full_fs | prove_fs | commit_fs | vp_fft_gkr on a tape | sum of the parts |")
    print("|---|---|---|---|---|---|", flush=True)
    rows = []
    for i in range(repeats):
        full = timed(lambda: s.prove_full_fs())
        parts = (timed(lambda: s.prove_fs()), timed(lambda: s.commit_fs(point)), timed(fft))
        rows.append((full,) + parts)
        print("| %d | %.2f | %.2f | %.2f | %.3f | %.2f |" % ((i,) + rows[-1] + (sum(parts),)), flush=True)
    med = statistics.median
    a, b = [r[0] for r in rows], [sum(r[1:]) for r in rows]
    print("\nmedian: joined %.2f ms (spread %.2f), parts %.2f ms (spread %.2f); joined - parts = %.2f ms\n" % (med(a), max(a) - min(a), med(b), max(b) - min(b), med(a) - med(b)))
    s.close()
    c.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(int(args[0]), int(args[1]) if len(args) > 1 else 5, "--cold" in sys.argv)
