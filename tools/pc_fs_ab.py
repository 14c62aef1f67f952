#!/usr/bin/env python3
"""The commit phase of the non-interactive commitment proof, device-drawn against host-drawn, alternated in one process:
    python tools/pc_fs_ab.py BLOCKS [REPEATS] [--once]
Session.commit_fs(device_draws=True) (vp_fri_commit_fs: the device draws every fold challenge from the root it has just computed) against
device_draws=False (the vp_fri_step loop, the chain on the host) on the commitment of the SHA-256 x BLOCKS input layer, after two warm-up proofs of each
form; per run the commit phase alone (prover::fsPhaseSec / fsPhaseDeviceMs: host wall clock and device time).  Beside them the one-pass vp_fri_commit on the
drawn challenges — the floor that interactivity allows.  Then one profiled vp_fri_commit_fs: device time per level from the launch table.  Prints markdown.
--once: one proof of each form and nothing else (for a kernel trace of its own)."""
import ctypes
import gzip
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(blocks, repeats, once):
    sys.path.insert(0, ROOT)
    import numpy as np
    import vp_loader
    vp = vp_loader.load()
    vp.lib_host()
    with tempfile.TemporaryDirectory() as tmp:
        pws = os.path.join(tmp, "s.pws")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "SHA256_64.pws.gz"), "rb") as f, open(pws, "wb") as o:
            o.write(f.read())
        c = vp.Circuit.from_pws(pws, blocks, seed=1)
    n = c.layer_bitlen(0)
    ln = n - 6
    point = np.random.default_rng(5).integers(0, (1 << 61) - 1, size=(n, 2), dtype=np.uint64)
    s = vp.Session(c)
    proofs = {}
    for form in (True, False) * (1 if once else 2):                        # warm-up: tables, buffers, pinned staging, code objects
        proofs[form] = s.commit_fs(point, device_draws=form)
    assert proofs[True] == proofs[False], "the two forms give different proofs"
    if once:
        print("x%d: one proof of each form, %d bytes, the same bytes" % (blocks, len(proofs[True])))
        return
    ok, why = vp.Circuit.verify_commitment_fs(proofs[True])
    assert ok, why
    runs = {True: [], False: []}
    for _ in range(repeats):
        for form in (True, False):
            assert s.commit_fs(point, device_draws=form) == proofs[True]
            runs[form].append(s.last_commit_fs_times())
    r, _ = vp.Circuit.commitment_fs_challenges(proofs[True])
    floor = []
    for _ in range(repeats):
        s.commit_private(); s.commit_public_eq(point)
        s.fri_commit(r, batched=True)
        floor.append(s.commit_device_ms())
    print("## x%d (n = %d, %d levels), %d alternated runs, commit phase alone\n" % (blocks, n, ln, repeats))
    print("| run | device-drawn: host ms | device ms | host-drawn loop: host ms | device ms (levels' sum) | one-pass vp_fri_commit: device ms |")
    print("|---|---|---|---|---|---|")
    for i in range(repeats):
        print("| %d | %.3f | %.3f | %.3f | %.3f | %.3f |" % (i, 1e3 * runs[True][i][0], runs[True][i][1], 1e3 * runs[False][i][0], runs[False][i][1], floor[i]))
    med = lambda v: statistics.median(v)
    spread = lambda v: max(v) - min(v)
    a, b = [1e3 * t[0] for t in runs[True]], [1e3 * t[0] for t in runs[False]]
    print("\nmedian host ms: device-drawn %.3f (spread %.3f), host-drawn loop %.3f (spread %.3f), one-pass floor %.3f device ms; loop / device-drawn = %.3f"
          % (med(a), spread(a), med(b), spread(b), med(floor), med(b) / med(a)))
    # one profiled phase through the C ABI: the launch table of vp_fri_commit_fs itself
    L, ctx = vp.lib_gpu(), vp.lib_host().vph_session_ctx(s.h)
    s.commit_private(); s.commit_public_eq(point)
    L.vp_set_profiling(ctx, 1)
    roots, st, sin = ctypes.create_string_buffer(32 * ln), ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    rr = np.zeros((ln, 2), np.uint64)
    cp = lambda x: ctypes.cast(x, ctypes.c_void_p)
    assert L.vp_fri_commit_fs(ctx, cp(sin), cp(roots), rr.ctypes.data, cp(st)) == 0
    rows = s.launch_stats()
    L.vp_set_profiling(ctx, 0)
    print("\nprofiled vp_fri_commit_fs (every launch bracketed by events), device us per level:\n")
    print("| level | fold | leaf hash | tree levels | drawing top | sum |")
    print("|---|---|---|---|---|---|")
    level, acc, tot = 0, {"k_fri_fold": 0.0, "k_leaf_hash": 0.0, "k_merkle": 0.0, "top": 0.0}, 0.0
    for e in rows:
        if e["kernel"] == "k_merkle" and e["rounds"] == 1:
            acc["top"] = e["us"]
            sm = sum(acc.values()); tot += sm
            print("| %d | %.1f | %.1f | %.1f | %.1f | %.1f |" % (level, acc["k_fri_fold"], acc["k_leaf_hash"], acc["k_merkle"], acc["top"], sm))
            level, acc = level + 1, {"k_fri_fold": 0.0, "k_leaf_hash": 0.0, "k_merkle": 0.0, "top": 0.0}
        elif e["kernel"] in acc:
            acc[e["kernel"]] += e["us"]
    print("\n%d launches in the table, %.3f ms in them" % (len(rows), tot / 1e3))
    s.close()
    c.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(int(args[0]), int(args[1]) if len(args) > 1 else 8, "--once" in sys.argv)
